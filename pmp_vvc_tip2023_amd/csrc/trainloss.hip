// trainloss.hip — the objective the nets are trained on, and its gradient with respect to the logits, in one pass over logits and labels.
//
// Replaces the arithmetic of
//   Train_QBD.loss_func_QBD (Train_QBD.py:68-90), Train_QBD.loss_func_MSBD (:44-66) and the plain L1_Loss of pre_train_Q (:161)
// and of torch's backward pass through them, for ONE batch: thirteen sums T[0..12] (include/pmp.h: pmp_train_loss; term for term
// S[0..12] of pmp_val_stats, with the component's weight matrix in w), the loss as a float64, and the gradient of that loss with
// respect to every logit.  Labels arrive in the dtypes of the label files and are converted as valstats.hip converts them.
//
// Terms are formed exactly as in valstats.hip (float32 operations in torch's order, no FMA: built with -ffp-contract=off) and added
// in the same order, so for PMP_LUMA the thirteen sums are pmp_val_stats' first thirteen, bit for bit:
//   train_block_kernel   one wavefront per block.  Lane l holds qt cell l and cells 4l..4l+3 of each 16x16 map (one 16-byte load per
//                        logit map, one 4-byte load per label map).  Lane partials in cell order, a __shfl_xor butterfly over the
//                        64 lanes, lane s < 13 stores T_block[s]: f64[n][13].  With gradients: one 16-byte store per gradient map
//                        and lane (4 bytes for the qt map, which has one cell per lane).  A gradient is computed in float64 from
//                        the float32 w, the double lambdas and the sign of the float32 term, left to right as include/pmp.h writes
//                        it, and rounded once to float32.  Every cell is written.
//   train_reduce_kernel  one workgroup of 208 threads = 16 row groups x 13 sums, the order of val_reduce_kernel; then thread 0 forms
//                        the loss from the thirteen sums (train_loss_value).
// The order depends on n only and there are no atomics: the same inputs give the same bits on every run.
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

constexpr int NT = PMP_LOSS_NTERMS;
constexpr int RG = 16;                 // row groups of the reduction

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// torch.sign, which is what abs' backward multiplies by: +1, -1, and 0 for zero AND for NaN
__device__ __forceinline__ double sgn(float t) { return (double)((int)(t > 0.f) - (int)(t < 0.f)); }

__global__ __launch_bounds__(64) void train_block_kernel(const float *__restrict__ qt, const float *__restrict__ bt,
                                                          const float *__restrict__ dire, const uint8_t *__restrict__ qt8,
                                                          const uint8_t *__restrict__ msbt, const int8_t *__restrict__ msdire, int64_t n,
                                                          float wm0, float wm1, float wm2, int w0_one, pmp_loss_params L, double d64,
                                                          double d256, double *__restrict__ out, float *__restrict__ g_qt,
                                                          float *__restrict__ g_bt, float *__restrict__ g_dire)
{
    const int64_t b = blockIdx.x;
    if (b >= n) return;
    const int lane = threadIdx.x;
    double s[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) s[i] = 0.0;

    if (qt) {
        const float x = qt[b * 64 + lane];
        const float ql = (float)(uint8_t)(qt8[b * 64 + lane] - 1);          // the loader's u8 subtraction: raw 0 -> 255.0
        const float t = x - ql;
        s[0] = wave_sum((double)fabsf(t));
        if (g_qt) g_qt[b * 64 + lane] = (float)(L.lambq * sgn(t) / d64);
    }
    if (bt) {
        const float wm[3] = {wm0, wm1, wm2};
        float w[3][4];
        double a[3][4], e[3][4];                                             // signs of the bt terms: plain L1 and layer difference
        float pb[4] = {0.f, 0.f, 0.f, 0.f}, pl[4] = {0.f, 0.f, 0.f, 0.f};   // layer k - 1: logits and labels
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 vb = reinterpret_cast<const float4 *>(bt + (b * 3 + k) * 256)[lane];
            const float4 vd = reinterpret_cast<const float4 *>(dire + (b * 3 + k) * 256)[lane];
            const uint32_t ub = reinterpret_cast<const uint32_t *>(msbt + (b * 3 + k) * 256)[lane];
            const uint32_t ud = reinterpret_cast<const uint32_t *>(msdire + (b * 3 + k) * 256)[lane];
            const float xb[4] = {vb.x, vb.y, vb.z, vb.w}, xd[4] = {vd.x, vd.y, vd.z, vd.w};
            double l1b = 0.0, l1d = 0.0, wd = 0.0, wb = 0.0;
            float gd[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float bl = (float)((ub >> (8 * c)) & 255u);
                const float dl = (float)(int8_t)((ud >> (8 * c)) & 255u);
                w[k][c] = (k == 0 && w0_one) ? 1.0f : dl * dl + wm[k];
                const float tb = xb[c] - bl;
                const float td = w[k][c] * xd[c] - w[k][c] * dl;
                const float tr = k == 0 ? w[k][c] * xb[c] - w[k][c] * bl : w[k][c] * (xb[c] - pb[c]) - w[k][c] * (bl - pl[c]);
                l1b += (double)fabsf(tb);
                l1d += (double)fabsf(xd[c] - dl);
                wd += (double)fabsf(td);
                wb += (double)fabsf(tr);
                a[k][c] = sgn(tb);
                e[k][c] = sgn(tr);
                gd[c] = (float)(L.lambd[k] * (double)w[k][c] * sgn(td) / d256);
                pb[c] = xb[c];
                pl[c] = bl;
            }
            s[1 + k] = wave_sum(l1b);
            s[4 + k] = wave_sum(l1d);
            s[7 + k] = wave_sum(wd);
            s[10 + k] = wave_sum(wb);
            if (g_dire) reinterpret_cast<float4 *>(g_dire + (b * 3 + k) * 256)[lane] = make_float4(gd[0], gd[1], gd[2], gd[3]);
        }
        if (g_bt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float g[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double v = L.lambb[k] * a[k][c] + L.lambresb[k] * (double)w[k][c] * e[k][c];
                    if (k < 2) v = v - L.lambresb[k + 1] * (double)w[k + 1][c] * e[k + 1][c];
                    g[c] = (float)(v / d256);
                }
                reinterpret_cast<float4 *>(g_bt + (b * 3 + k) * 256)[lane] = make_float4(g[0], g[1], g[2], g[3]);
            }
        }
    }
    // lane i stores sum i (every lane holds all thirteen, bit for bit)
    double mine = 0.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) mine = lane == i ? s[i] : mine;
    if (lane < NT) out[b * NT + lane] = mine;
}

__global__ __launch_bounds__(RG * NT) void train_reduce_kernel(const double *__restrict__ part, int64_t n, pmp_loss_params L, int64_t n_div,
                                                               double *__restrict__ terms, double *__restrict__ loss)
{
    __shared__ double sh[RG * NT];
    __shared__ double tot[NT];
    const int t = threadIdx.x;
    double a = 0.0;
    const int64_t total = n * NT;
    for (int64_t i = t; i < total; i += 8 * RG * NT) {                       // row t / 13 + 16 j, sum t % 13
        double v[8];                                                         // eight loads in flight, added in row order
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int64_t k = i + j * (RG * NT); v[j] = k < total ? part[k] : 0.0; }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (i + j * (RG * NT) < total) a += v[j];
    }
    sh[t] = a;
    __syncthreads();
    if (t < NT) {
        double r = sh[t];
#pragma unroll
        for (int g = 1; g < RG; ++g) r += sh[g * NT + t];
        terms[t] = r;
        tot[t] = r;
    }
    __syncthreads();
    if (t == 0 && loss) *loss = train_loss_value(tot, L, n_div);
}

}  // namespace

hipError_t launch_train_loss(hipStream_t st, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                             const int8_t *msdire, int64_t N, int64_t n_div, const float wm[3], int w0_one, const pmp_loss_params &L,
                             double *block_terms, double *terms, double *loss, float *g_qt, float *g_bt, float *g_dire)
{
    const double d64 = (double)(64 * n_div), d256 = (double)(256 * n_div);
    // grids of at most 2^20 blocks (gridDim.x is 32-bit); blocks are independent
    for (int64_t o = 0; o < N; o += (int64_t)1 << 20) {
        const int64_t m = (N - o) < ((int64_t)1 << 20) ? (N - o) : ((int64_t)1 << 20);
        hipLaunchKernelGGL(train_block_kernel, dim3((unsigned)m), dim3(64), 0, st, qt ? qt + o * 64 : nullptr, bt ? bt + o * 768 : nullptr,
                           bt ? dire + o * 768 : nullptr, qt ? qt8 + o * 64 : nullptr, bt ? msbt + o * 768 : nullptr,
                           bt ? msdire + o * 768 : nullptr, m, wm[0], wm[1], wm[2], w0_one, L, d64, d256, block_terms + o * NT,
                           g_qt ? g_qt + o * 64 : nullptr, g_bt ? g_bt + o * 768 : nullptr, g_dire ? g_dire + o * 768 : nullptr);
    }
    hipLaunchKernelGGL(train_reduce_kernel, dim3(1), dim3(RG * NT), 0, st, block_terms, N, L, n_div, terms, loss);
    return hipGetLastError();
}

}  // namespace pmp
