// logitstats.hip — one batch of logits against VTM's labels, on the GPU: the numbers behind the reference's validation, and the
// objective the nets are trained on with its gradient with respect to the logits.  Both are sums of the same float32 terms, formed once.
//
// Replaces the arithmetic of
//   Metrics.validation_QBD (Metrics.py:313-385), Metrics.pre_validation predID 0 / 1 (:196-274) and the losses under them,
//   loss_func_QBD_val / loss_func_MSBD_val with weight_mat (:148-194):
//     twenty numbers S[0..19] (include/pmp.h: pmp_val_stats) from which every L1 loss, accuracy and validation loss of the batch
//     follows by a division;
//   Train_QBD.loss_func_QBD (Train_QBD.py:68-90), Train_QBD.loss_func_MSBD (:44-66), the plain L1_Loss of pre_train_Q (:161) and
//   torch's backward pass through them:
//     thirteen sums T[0..12] (include/pmp.h: pmp_train_loss; term for term S[0..12], with the component's weight matrix in w), the
//     loss as a float64 and the gradient of that loss with respect to every logit.
// Labels arrive in the dtypes the label files hold and are converted as the reference's loader does (Metrics.py:127-135):
// bl = float(msbt), dl = float(msdire), ql = float(u8(qt8 - 1)) - numpy subtracts on the u8 array, so a raw qtDepth of 0 becomes
// 255.0, not -1.0.
//
// Every per-element term is formed as torch forms it: float32 operations in the reference's order (w * out, w * label, the
// subtraction, abs; for the layer differences the two differences first), never contracted into an FMA (this file is built
// with -ffp-contract=off), w_k = dl_k * dl_k + float32(weight matrix[row][k]).  torch.round is round-half-to-even (rintf =
// v_rndne_f32); a NaN logit is never a hit; nothing is clamped, so NaN / inf logits give NaN / inf sums.  The two block kernels
// share the loads, the weights and the terms (load_qt, load_layer, cell_terms, LayerSums), so for PMP_LUMA the thirteen sums are
// pmp_val_stats' first thirteen, bit for bit.
//
// Sums are float64 in a fixed order, without atomics:
//   val_block_kernel    one wavefront per block.  Lane l holds qt cell l and, of each of the three 16x16 maps, cells 4l..4l+3
//                       (one 16-byte load per logit map, one 4-byte load per label map): 12 bt and 12 dire cells.  A lane adds its
//                       terms in cell order, the 64 lane partials are added by a __shfl_xor butterfly (offsets 32, 16, .. 1: every
//                       lane ends with the same bits), hits are counted by ballot + popcount.  Lane s < 20 stores S_block[s]:
//                       f64[n][20], hit counts as exact integers in float64.
//   train_block_kernel  the same thirteen sums, lane s < 13 stores T_block[s]: f64[n][13].  With gradients: one 16-byte store per
//                       gradient map and lane (4 bytes for the qt map, which has one cell per lane).  A gradient is computed in
//                       float64 from the float32 w, the double lambdas and the sign of the float32 term, left to right as
//                       include/pmp.h writes it, and rounded once to float32.  Every cell is written.
//   sum_rows_kernel     one workgroup of 16 row groups x NC columns: 320 threads for the 20 statistics, 208 for the 13 sums.
//                       Thread (g, s) adds rows g, g + 16, g + 32, ... in order (its loads are coalesced: address = thread + 16 NC j),
//                       then thread s adds the 16 group partials in order; for the 13 sums thread 0 then forms the loss
//                       (train_loss_value).  The order depends on n only: same inputs, same bits - on every run, stream and context.
#include "../../include/pmp.h"
#include "pmp_kernels.h"

namespace pmp {

__host__ __device__ double train_loss_value(const double T[PMP_LOSS_NTERMS], const pmp_loss_params &L, int64_t n)
{
    const double d64 = (double)(64 * n), d256 = (double)(256 * n);
    return L.lambq * T[0] / d64 + (L.lambb[0] * T[1] + L.lambb[1] * T[2] + L.lambb[2] * T[3] + L.lambd[0] * T[7] + L.lambd[1] * T[8] +
                                   L.lambd[2] * T[9] + L.lambresb[0] * T[10] + L.lambresb[1] * T[11] + L.lambresb[2] * T[12]) / d256;
}

namespace {

constexpr int NS = PMP_VAL_NSTATS;
constexpr int NT = PMP_LOSS_NTERMS;
constexpr int RG = 16;                 // row groups of the reduction

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double hits(bool p) { return (double)__popcll(__ballot(p)); }

// torch.sign, which is what abs' backward multiplies by: +1, -1, and 0 for zero AND for NaN
__device__ __forceinline__ double sgn(float t) { return (double)((int)(t > 0.f) - (int)(t < 0.f)); }

// ---- what a lane holds of block b, and the terms of its cells -----------------------------------------------------------------
struct QtCell {
    float x, ql;                                                             // logit and label of qt cell `lane`
    __device__ __forceinline__ float term() const { return x - ql; }
};

__device__ __forceinline__ QtCell load_qt(const LogitLabels &p, int64_t b, int lane)
{
    return {p.qt[b * 64 + lane], (float)(uint8_t)(p.qt8[b * 64 + lane] - 1)};   // the loader's u8 subtraction: raw 0 -> 255.0
}

struct Layer {
    float xb[4], xd[4], bl[4], dl[4], w[4];                                  // cells 4 lane .. 4 lane + 3 of layer k: logits, labels, weight
};

__device__ __forceinline__ Layer load_layer(const LogitLabels &p, int64_t b, int k, int lane, const LogitWeights &lw)
{
    const int64_t at = (b * 3 + k) * 256;
    const float4 vb = reinterpret_cast<const float4 *>(p.bt + at)[lane];
    const float4 vd = reinterpret_cast<const float4 *>(p.dire + at)[lane];
    const uint32_t ub = reinterpret_cast<const uint32_t *>(p.msbt + at)[lane];
    const uint32_t ud = reinterpret_cast<const uint32_t *>(p.msdire + at)[lane];
    Layer y = {{vb.x, vb.y, vb.z, vb.w}, {vd.x, vd.y, vd.z, vd.w}, {}, {}, {}};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        y.bl[c] = (float)((ub >> (8 * c)) & 255u);
        y.dl[c] = (float)(int8_t)((ud >> (8 * c)) & 255u);
        y.w[c] = (k == 0 && lw.w0_one) ? 1.0f : y.dl[c] * y.dl[c] + lw.wm[k];
    }
    return y;
}

struct Terms { float b, d, wd, wb; };                                        // before abs: plain bt, plain dire, weighted dire, weighted bt layer difference

// cell c of layer k; y[0..k] are loaded (layer 0's difference is against nothing)
__device__ __forceinline__ Terms cell_terms(const Layer *y, int k, int c)
{
    const Layer &a = y[k];
    const float w = a.w[c];
    Terms t;
    t.b = a.xb[c] - a.bl[c];
    t.d = a.xd[c] - a.dl[c];
    t.wd = w * a.xd[c] - w * a.dl[c];
    if (k == 0) t.wb = w * a.xb[c] - w * a.bl[c];
    else t.wb = w * (a.xb[c] - y[k - 1].xb[c]) - w * (a.bl[c] - y[k - 1].bl[c]);
    return t;
}

// |terms| of a lane's cells of layer k, added in cell order; then the 64 lanes: S[1 + k], S[4 + k], S[7 + k], S[10 + k]
struct LayerSums {
    double l1b = 0.0, l1d = 0.0, wd = 0.0, wb = 0.0;
    __device__ __forceinline__ void add(const Terms &t)
    {
        l1b += (double)fabsf(t.b);
        l1d += (double)fabsf(t.d);
        wd += (double)fabsf(t.wd);
        wb += (double)fabsf(t.wb);
    }
    __device__ __forceinline__ void store(int k, double *s) const
    {
        s[1 + k] = wave_sum(l1b);
        s[4 + k] = wave_sum(l1d);
        s[7 + k] = wave_sum(wd);
        s[10 + k] = wave_sum(wb);
    }
};

// lane i stores number i of the block's row (every lane holds all N, bit for bit)
template <int N>
__device__ __forceinline__ void store_row(const double (&s)[N], int lane, double *__restrict__ row)
{
    double mine = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) mine = lane == i ? s[i] : mine;
    if (lane < N) row[lane] = mine;
}

// ---- the block kernels --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void val_block_kernel(LogitLabels p, int64_t n, LogitWeights lw, double *__restrict__ out)
{
    const int64_t b = blockIdx.x;
    if (b >= n) return;
    const int lane = threadIdx.x;
    double s[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;

    if (p.has_q()) {
        const QtCell q = load_qt(p, b, lane);
        s[0] = wave_sum((double)fabsf(q.term()));
        s[13] = hits(rintf(q.x) == q.ql);
    }
    if (p.has_m()) {
        Layer y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            y[k] = load_layer(p, b, k, lane, lw);
            LayerSums sums;
            double hb = 0.0, hd = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sums.add(cell_terms(y, k, c));
                hb += hits(rintf(y[k].xb[c]) == y[k].bl[c]);
                hd += hits(rintf(y[k].xd[c]) == y[k].dl[c]);
            }
            sums.store(k, s);
            s[14 + k] = hb;
            s[17 + k] = hd;
        }
    }
    store_row(s, lane, out + b * NS);
}

__global__ __launch_bounds__(64) void train_block_kernel(LogitLabels p, int64_t n, LogitWeights lw, pmp_loss_params L, double d64, double d256,
                                                          double *__restrict__ out, float *__restrict__ g_qt, float *__restrict__ g_bt,
                                                          float *__restrict__ g_dire)
{
    const int64_t b = blockIdx.x;
    if (b >= n) return;
    const int lane = threadIdx.x;
    double s[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) s[i] = 0.0;

    if (p.has_q()) {
        const float t = load_qt(p, b, lane).term();
        s[0] = wave_sum((double)fabsf(t));
        if (g_qt) g_qt[b * 64 + lane] = (float)(L.lambq * sgn(t) / d64);
    }
    if (p.has_m()) {
        Layer y[3];
        Terms t[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            y[k] = load_layer(p, b, k, lane, lw);
            LayerSums sums;
            float gd[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                t[k][c] = cell_terms(y, k, c);
                sums.add(t[k][c]);
                gd[c] = (float)(L.lambd[k] * (double)y[k].w[c] * sgn(t[k][c].wd) / d256);
            }
            sums.store(k, s);
            if (g_dire) reinterpret_cast<float4 *>(g_dire + (b * 3 + k) * 256)[lane] = make_float4(gd[0], gd[1], gd[2], gd[3]);
        }
        if (g_bt) {                                                          // bt layer k is in the plain term k and the differences k, k + 1
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float g[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double v = L.lambb[k] * sgn(t[k][c].b) + L.lambresb[k] * (double)y[k].w[c] * sgn(t[k][c].wb);
                    if (k < 2) v = v - L.lambresb[k + 1] * (double)y[k + 1].w[c] * sgn(t[k + 1][c].wb);
                    g[c] = (float)(v / d256);
                }
                reinterpret_cast<float4 *>(g_bt + (b * 3 + k) * 256)[lane] = make_float4(g[0], g[1], g[2], g[3]);
            }
        }
    }
    store_row(s, lane, out + b * NT);
}

// ---- the fixed-order sum of the block rows ------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(RG * NC) void sum_rows_kernel(const double *__restrict__ part, int64_t n, double *__restrict__ sums,
                                                           pmp_loss_params L, int64_t n_div, double *__restrict__ loss)
{
    __shared__ double sh[RG * NC];
    const int t = threadIdx.x;
    double a = 0.0;
    const int64_t total = n * NC;
    for (int64_t i = t; i < total; i += 8 * RG * NC) {                       // row t / NC + 16 j, column t % NC
        double v[8];                                                         // eight loads in flight, added in row order
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int64_t k = i + j * (RG * NC); v[j] = k < total ? part[k] : 0.0; }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (i + j * (RG * NC) < total) a += v[j];
    }
    sh[t] = a;
    __syncthreads();
    double r = 0.0;
    if (t < NC) {
        r = sh[t];
#pragma unroll
        for (int g = 1; g < RG; ++g) r += sh[g * NC + t];
        sums[t] = r;
    }
    if constexpr (NC == NT) {                                                // the training losses' epilogue
        __shared__ double tot[NT];
        if (t < NT) tot[t] = r;
        __syncthreads();
        if (t == 0 && loss) *loss = train_loss_value(tot, L, n_div);
    }
}

// launch(first block, blocks) over grids of at most 2^20 blocks (gridDim.x is 32-bit); blocks are independent
template <class F>
void for_grids(int64_t N, F launch)
{
    for (int64_t o = 0; o < N; o += (int64_t)1 << 20) launch(o, (N - o) < ((int64_t)1 << 20) ? (N - o) : ((int64_t)1 << 20));
}

}  // namespace

hipError_t launch_val_stats(hipStream_t st, const LogitLabels &in, int64_t N, const LogitWeights &lw, double *block_stats, double *stats)
{
    for_grids(N, [&](int64_t o, int64_t m) {
        hipLaunchKernelGGL(val_block_kernel, dim3((unsigned)m), dim3(64), 0, st, in.from(o), m, lw, block_stats + o * NS);
    });
    hipLaunchKernelGGL(sum_rows_kernel<NS>, dim3(1), dim3(RG * NS), 0, st, block_stats, N, stats, pmp_loss_params{}, (int64_t)0, nullptr);
    return hipGetLastError();
}

hipError_t launch_train_loss(hipStream_t st, const LogitLabels &in, int64_t N, int64_t n_div, const LogitWeights &lw, const pmp_loss_params &L,
                             double *block_terms, double *terms, double *loss, const LogitGrads &g)
{
    const double d64 = (double)(64 * n_div), d256 = (double)(256 * n_div);
    for_grids(N, [&](int64_t o, int64_t m) {
        const LogitGrads go = g.from(o);
        hipLaunchKernelGGL(train_block_kernel, dim3((unsigned)m), dim3(64), 0, st, in.from(o), m, lw, L, d64, d256, block_terms + o * NT, go.qt,
                           go.bt, go.dire);
    });
    hipLaunchKernelGGL(sum_rows_kernel<NT>, dim3(1), dim3(RG * NT), 0, st, block_terms, N, terms, L, n_div, loss);
    return hipGetLastError();
}

}  // namespace pmp
