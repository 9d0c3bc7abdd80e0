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
// pmp_val_confusion counts instead of adding: per map the joint histogram of (label class, class of rintf(logit)), 7 x 5 x 5 integers
// (include/pmp.h).  No floating-point value is added anywhere in it, so its bits depend on no order at all.
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
//   confusion_block_kernel  the third block kernel: the same wavefront per block and the same cells per lane, through the same load_qt /
//                       load_layer.  The 175 cells are counted in an LDS histogram with integer LDS atomics (ds_add_u32: integer
//                       addition commutes, so the counts are exact whatever order the lanes arrive in; ballot + popcount would give the
//                       same bits at 25 ballots per cell), in eight copies that spread the lanes' turns at one word.  Lanes j,
//                       j + 64, j + 128 < 175 store cell j of the block's row: u16[n][175] (a block's cell is at most 256).  Labels
//                       without logits (the census) count every prediction as "other".
//   sum_counts_kernel   the rows' column sums in int64: 7 maps x 32 row slices of workgroups, each 16 row groups x 25 columns (the
//                       shape of sum_rows_kernel), a slice's sums added to the call's counts with int64 vector atomics - integers again,
//                       so the same bits in any order.
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

// the labels of cells 4 lane .. 4 lane + 3 of layer k, and the weight they give
__device__ __forceinline__ void load_layer_labels(const LogitLabels &p, int64_t at, int k, int lane, const LogitWeights &lw, Layer &y)
{
    const uint32_t ub = reinterpret_cast<const uint32_t *>(p.msbt + at)[lane];
    const uint32_t ud = reinterpret_cast<const uint32_t *>(p.msdire + at)[lane];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        y.bl[c] = (float)((ub >> (8 * c)) & 255u);
        y.dl[c] = (float)(int8_t)((ud >> (8 * c)) & 255u);
        y.w[c] = (k == 0 && lw.w0_one) ? 1.0f : y.dl[c] * y.dl[c] + lw.wm[k];
    }
}

__device__ __forceinline__ Layer load_layer(const LogitLabels &p, int64_t b, int k, int lane, const LogitWeights &lw)
{
    const int64_t at = (b * 3 + k) * 256;
    const float4 vb = reinterpret_cast<const float4 *>(p.bt + at)[lane];
    const float4 vd = reinterpret_cast<const float4 *>(p.dire + at)[lane];
    Layer y = {{vb.x, vb.y, vb.z, vb.w}, {vd.x, vd.y, vd.z, vd.w}, {}, {}, {}};
    load_layer_labels(p, at, k, lane, lw, y);
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

// ---- the confusion counts: class of a label or of a rounded logit (both hold an integer, NaN or +-inf) -----------------------------
constexpr int NCC = PMP_CONF_CLASSES, NMC = NCC * NCC, NCNT = PMP_CONF_NCOUNTS;   // 5 classes, 25 cells per map, 175 per block
constexpr int HC = 8;                                                           // copies of a block's histogram in LDS
__device__ __forceinline__ int depth_class(float v) { return (v >= 0.f && v <= 3.f) ? (int)v : 4; }       // -0.0 is 0; NaN fails both
__device__ __forceinline__ int dire_class(float v) { return (v >= -1.f && v <= 1.f) ? (int)v + 1 : 3; }

// A group given without its logits (p.qt, p.bt null) is the labels' census: every prediction is NaN, the class "other"
// zero: the call's counts i64[175], cleared here by the first block of the call's first grid for sum_counts_kernel to add into; else null
__global__ __launch_bounds__(64) void confusion_block_kernel(LogitLabels p, int64_t n, uint16_t *__restrict__ out, int64_t *__restrict__ zero)
{
    const int64_t b = blockIdx.x;
    if (b >= n) return;
    const int lane = threadIdx.x;
    if (zero && b == 0)
        for (int j = lane; j < NCNT; j += 64) zero[j] = 0;
    // eight copies of the histogram, lane l counting in copy l % 8: labels crowd into a few cells, and lanes that add to one LDS word
    // take turns (one copy against eight: profiles/val_confusion.txt)
    __shared__ unsigned hist[HC][NCNT];
    for (int j = lane; j < HC * NCNT; j += 64) (&hist[0][0])[j] = 0u;
    __syncthreads();
    unsigned *h = hist[lane % HC];
    const float other = __builtin_nanf("");
    if (p.qt8) {
        QtCell q = {other, 0.f};
        if (p.has_q()) q = load_qt(p, b, lane);
        else q.ql = (float)(uint8_t)(p.qt8[b * 64 + lane] - 1);
        atomicAdd(&h[depth_class(q.ql) * NCC + depth_class(rintf(q.x))], 1u);
    }
    if (p.msbt) {
        const LogitWeights none = {{0.f, 0.f, 0.f}, 0};                      // nothing here is weighted
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Layer y = {{other, other, other, other}, {other, other, other, other}, {}, {}, {}};
            if (p.has_m()) y = load_layer(p, b, k, lane, none);
            else load_layer_labels(p, (b * 3 + k) * 256, k, lane, none, y);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                atomicAdd(&h[(1 + k) * NMC + depth_class(y.bl[c]) * NCC + depth_class(rintf(y.xb[c]))], 1u);
                atomicAdd(&h[(4 + k) * NMC + dire_class(y.dl[c]) * NCC + dire_class(rintf(y.xd[c]))], 1u);
            }
        }
    }
    __syncthreads();
    for (int j = lane; j < NCNT; j += 64) {
        unsigned v = 0u;
#pragma unroll
        for (int k = 0; k < HC; ++k) v += hist[k][j];
        out[b * NCNT + j] = (uint16_t)v;
    }
}

// counts[m][..] += the column sums of a slice of the rows u16[n][175]: workgroup (map m, slice z) = blockIdx (x, y), thread (g, s) adds
// rows 16 z + g, + 16 CS, + 32 CS, ..., thread s the 16 groups and then, with one int64 vector atomic, the slice into counts (zeroed by the
// block kernel).  With one workgroup per map - 2-byte gathers on 7 CUs - a call on 4096 blocks took 76 us, not 12 (profiles/val_confusion.txt).
constexpr int CS = 32;                                                          // row slices of the column sum
__global__ __launch_bounds__(RG * NMC) void sum_counts_kernel(const uint16_t *__restrict__ part, int64_t n, unsigned long long *__restrict__ counts)
{
    __shared__ int64_t sh[RG * NMC];
    const int t = threadIdx.x, col = blockIdx.x * NMC + t % NMC;
    int64_t a = 0;
    for (int64_t r = (int64_t)blockIdx.y * RG + t / NMC; r < n; r += 8 * RG * CS) {   // eight loads in flight
        unsigned v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int64_t k = r + (int64_t)j * RG * CS; v[j] = k < n ? (unsigned)part[k * NCNT + col] : 0u; }
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (int64_t)v[j];
    }
    sh[t] = a;
    __syncthreads();
    if (t < NMC) {
        int64_t r = sh[t];
#pragma unroll
        for (int g = 1; g < RG; ++g) r += sh[g * NMC + t];
        if (r) atomicAdd(&counts[col], (unsigned long long)r);
    }
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

hipError_t launch_val_confusion(hipStream_t st, const LogitLabels &in, int64_t N, uint16_t *block_counts, int64_t *counts)
{
    for_grids(N, [&](int64_t o, int64_t m) {
        hipLaunchKernelGGL(confusion_block_kernel, dim3((unsigned)m), dim3(64), 0, st, in.from(o), m, block_counts + o * NCNT,
                           o == 0 ? counts : nullptr);
    });
    hipLaunchKernelGGL(sum_counts_kernel, dim3(PMP_CONF_MAPS, CS), dim3(RG * NMC), 0, st, block_counts, N,
                       reinterpret_cast<unsigned long long *>(counts));
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
