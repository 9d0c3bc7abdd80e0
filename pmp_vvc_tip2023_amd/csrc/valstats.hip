// valstats.hip — the per-batch numbers behind the reference's validation, on the GPU: logits against VTM labels.
//
// Replaces the arithmetic of
//   Metrics.validation_QBD (Metrics.py:313-385), Metrics.pre_validation predID 0 / 1 (:196-274) and the losses under them,
//   loss_func_QBD_val / loss_func_MSBD_val with weight_mat (:148-194),
// for ONE batch: twenty numbers S[0..19] (include/pmp.h: pmp_val_stats) from which every L1 loss, accuracy and validation loss
// of the batch follows by a division.  Labels arrive in the dtypes the label files hold and are converted as the reference's
// loader does (Metrics.py:127-135): bl = float(msbt), dl = float(msdire), ql = float(u8(qt8 - 1)) - numpy subtracts on the u8
// array, so a raw qtDepth of 0 becomes 255.0, not -1.0.
//
// Every per-element term is formed as torch forms it: float32 operations in the reference's order (w * out, w * label, the
// subtraction, abs; for the layer differences the two differences first), never contracted into an FMA (this file is built
// with -ffp-contract=off), w_k = dl_k * dl_k + float32(weight_mat[row][k]).  torch.round is round-half-to-even (rintf =
// v_rndne_f32); a NaN logit is never a hit; nothing is clamped, so NaN / inf logits give NaN / inf sums.
//
// Sums are float64 in a fixed order, without atomics:
//   val_block_kernel   one wavefront per block.  Lane l holds qt cell l and, of each of the three 16x16 maps, cells 4l..4l+3
//                      (one 16-byte load per logit map, one 4-byte load per label map): 12 bt and 12 dire cells.  A lane adds its
//                      terms in cell order, the 64 lane partials are added by a __shfl_xor butterfly (offsets 32, 16, .. 1: every
//                      lane ends with the same bits), hits are counted by ballot + popcount.  Lane s < 20 stores S_block[s]:
//                      f64[n][20], hit counts as exact integers in float64.
//   val_reduce_kernel  one workgroup of 320 threads = 16 row groups x 20 statistics.  Thread (g, s) adds rows g, g + 16, g + 32, ...
//                      in order (its loads are coalesced: address = thread + 320 j), then thread s adds the 16 group partials in
//                      order.  The order depends on n only: same inputs, same bits - on every run, stream and context.
#include "../../include/pmp.h"
#include "pmp_kernels.h"

namespace pmp {

namespace {

constexpr int NS = PMP_VAL_NSTATS;
constexpr int RG = 16;                 // row groups of the reduction

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double hits(bool p) { return (double)__popcll(__ballot(p)); }

__global__ __launch_bounds__(64) void val_block_kernel(const float *__restrict__ qt, const float *__restrict__ bt,
                                                        const float *__restrict__ dire, const uint8_t *__restrict__ qt8,
                                                        const uint8_t *__restrict__ msbt, const int8_t *__restrict__ msdire, int64_t n,
                                                        float wm0, float wm1, float wm2, int w0_one, double *__restrict__ out)
{
    const int64_t b = blockIdx.x;
    if (b >= n) return;
    const int lane = threadIdx.x;
    double s[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = 0.0;

    if (qt) {
        const float x = qt[b * 64 + lane];
        const float ql = (float)(uint8_t)(qt8[b * 64 + lane] - 1);          // the loader's u8 subtraction: raw 0 -> 255.0
        s[0] = wave_sum((double)fabsf(x - ql));
        s[13] = hits(rintf(x) == ql);
    }
    if (bt) {
        const float wm[3] = {wm0, wm1, wm2};
        float pb[4] = {0.f, 0.f, 0.f, 0.f}, pl[4] = {0.f, 0.f, 0.f, 0.f};   // layer k - 1: logits and labels
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 vb = reinterpret_cast<const float4 *>(bt + (b * 3 + k) * 256)[lane];
            const float4 vd = reinterpret_cast<const float4 *>(dire + (b * 3 + k) * 256)[lane];
            const uint32_t ub = reinterpret_cast<const uint32_t *>(msbt + (b * 3 + k) * 256)[lane];
            const uint32_t ud = reinterpret_cast<const uint32_t *>(msdire + (b * 3 + k) * 256)[lane];
            const float xb[4] = {vb.x, vb.y, vb.z, vb.w}, xd[4] = {vd.x, vd.y, vd.z, vd.w};
            double l1b = 0.0, l1d = 0.0, wd = 0.0, wb = 0.0;
            double hb = 0.0, hd = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float bl = (float)((ub >> (8 * c)) & 255u);
                const float dl = (float)(int8_t)((ud >> (8 * c)) & 255u);
                const float w = (k == 0 && w0_one) ? 1.0f : dl * dl + wm[k];
                l1b += (double)fabsf(xb[c] - bl);
                l1d += (double)fabsf(xd[c] - dl);
                wd += (double)fabsf(w * xd[c] - w * dl);
                if (k == 0) wb += (double)fabsf(w * xb[c] - w * bl);
                else wb += (double)fabsf(w * (xb[c] - pb[c]) - w * (bl - pl[c]));
                hb += hits(rintf(xb[c]) == bl);
                hd += hits(rintf(xd[c]) == dl);
                pb[c] = xb[c];
                pl[c] = bl;
            }
            s[1 + k] = wave_sum(l1b);
            s[4 + k] = wave_sum(l1d);
            s[7 + k] = wave_sum(wd);
            s[10 + k] = wave_sum(wb);
            s[14 + k] = hb;
            s[17 + k] = hd;
        }
    }
    // lane i stores statistic i (every lane holds all twenty, bit for bit)
    double mine = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) mine = lane == i ? s[i] : mine;
    if (lane < NS) out[b * NS + lane] = mine;
}

__global__ __launch_bounds__(RG * NS) void val_reduce_kernel(const double *__restrict__ part, int64_t n, double *__restrict__ stats)
{
    __shared__ double sh[RG * NS];
    const int t = threadIdx.x;
    double a = 0.0;
    const int64_t total = n * NS;
    for (int64_t i = t; i < total; i += 8 * RG * NS) {                       // row t / 20 + 16 j, statistic t % 20
        double v[8];                                                         // eight loads in flight, added in row order
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int64_t k = i + j * (RG * NS); v[j] = k < total ? part[k] : 0.0; }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (i + j * (RG * NS) < total) a += v[j];
    }
    sh[t] = a;
    __syncthreads();
    if (t < NS) {
        double r = sh[t];
#pragma unroll
        for (int g = 1; g < RG; ++g) r += sh[g * NS + t];
        stats[t] = r;
    }
}

}  // namespace

hipError_t launch_val_stats(hipStream_t st, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                            const int8_t *msdire, int64_t N, const float wm[3], int w0_one, double *block_stats, double *stats)
{
    // grids of at most 2^20 blocks (gridDim.x is 32-bit); blocks are independent
    for (int64_t o = 0; o < N; o += (int64_t)1 << 20) {
        const int64_t m = (N - o) < ((int64_t)1 << 20) ? (N - o) : ((int64_t)1 << 20);
        hipLaunchKernelGGL(val_block_kernel, dim3((unsigned)m), dim3(64), 0, st, qt ? qt + o * 64 : nullptr, bt ? bt + o * 768 : nullptr,
                           bt ? dire + o * 768 : nullptr, qt ? qt8 + o * 64 : nullptr, bt ? msbt + o * 768 : nullptr,
                           bt ? msdire + o * 768 : nullptr, m, wm[0], wm[1], wm[2], w0_one, block_stats + o * NS);
    }
    hipLaunchKernelGGL(val_reduce_kernel, dim3(1), dim3(RG * NS), 0, st, block_stats, N, stats);
    return hipGetLastError();
}

}  // namespace pmp
