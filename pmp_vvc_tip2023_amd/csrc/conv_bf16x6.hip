// conv_bf16x6.hip — fp32-accurate convolution on the bf16 matrix cores by 3-term operand splitting.
//
// Every fp32 value v is carried as three bf16 values v = v0 + v1 + v2 (exact: 3 x 8 significand bits = 24).
// A product x*w is evaluated as the six bf16 MFMA products with weight >= 2^-16:
//      x0w0 + (x0w1 + x1w0) + (x0w2 + x1w1 + x2w0)            (dropped terms are <= 2^-24 relative)
// accumulated in the MFMA's fp32 accumulator.  tools/precision_study.py: on the real Luma_Q_22 net this is as
// close to the reference as fp32 arithmetic itself (9.2e-5 vs 8.2e-5 for fp64-vs-fp32), while the 3-product split
// (4.6e-3) and single bf16 (0.79) break the 1e-3 tolerance.  Six v_mfma_f32_16x16x32_bf16 (16 cycles, K=32) replace
// sixteen v_mfma_f32_16x16x4_f32 (32 cycles, K=4 each) per 32 channels: 2.67x the fp32-MFMA peak.
//
// Activation format ("split-3"): three bf16 planes, each blocked channels-last [n][C/16][H][W][16] (32 B per pixel and
// group), plane stride = N*C*H*W elements.  Same bytes-per-lane coalescing as the fp32 layout: 16 pixels x 32 B = 512 B
// contiguous per plane per tile row.
//
// GEMM mapping: D[cout][pixel], A = weights, B = pixels (as conv_mfma.hip).  One MFMA K-step (K = 32) covers
// 16 channels x a PAIR of taps: lane group g = l>>4 reads channels 8(g&1)..+7 of tap 2p+(g>>1).  An odd tap count pads
// the last pair with zero weights (3x3: 10 % padding, 5x5: 4 %).
#include "conv_tile.h"

namespace pmp {

template <int KH, int KW>
__device__ __forceinline__ void x6_stage_store(const TilePlan<GeoX<KH, KW>> &p, u32x4 *lds, const u32x4 (&r)[GeoX<KH, KW>::NLD])
{
    typedef GeoX<KH, KW> G;
#pragma unroll
    for (int k = 0; k < G::NLD; ++k) {
        const int i = threadIdx.x + k * 256;
        const u32x4 z = {0u, 0u, 0u, 0u};
        if (i < G::PIECES) lds[i] = ((p.valid >> k) & 1u) ? r[k] : z;   // LDS image: [split][pixel][2 halves], linear
    }
}

template <int KH, int KW, int NT>
__device__ __forceinline__ void x6_accumulate(const unsigned short *__restrict__ x, size_t plane_stride,
                                              const unsigned short *__restrict__ wpk, int C, int H, int W, int n, int ty,
                                              int tx, u32x4 *lds, f32x4 (&acc)[4][NT])
{
    typedef GeoX<KH, KW> G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, xl = lane & 15, g = lane >> 4;
    const int CB = C >> 4;
    const size_t grp_sz = (size_t)H * W * 16;
    const unsigned short *grp0 = x + (size_t)n * CB * grp_sz;
    u32x4 r[G::NLD];
    TilePlan<G> plan;
    tile_plan<KH, KW>(plan, plane_stride, H, W, ty, tx);
    __syncthreads();
    tile_load(plan, grp0, r);
    x6_stage_store<KH, KW>(plan, lds, r);
    __syncthreads();
    // ---- K-step schedule -------------------------------------------------------------------------------------
    // Weight fragments live in ONE register set that is refilled in place, split by split, as soon as its last MFMA
    // of the K-step has been issued: w2 is used once (with x0), w1 twice, w0 three times, so the products are ordered
    //   phase A: x0*w2            -> request next K-step's w2
    //   phase B: x0*w1, x1*w1     -> request next w1 and the next K-step's x0 fragments (second register set)
    //   phase C: x0*w0, x1*w0, x2*w0 -> request next w0
    // Every request has at least one full phase (256..768 MFMA cycles) before its first use.  All loads are
    // unconditional so hipcc's s_waitcnt vmcnt(N) are exact counts; scheduling fences pin the phase order.
    // Tap pairing.  A K-step covers 16 channels x 2 taps.  With an odd tap count the last tap has no partner inside its
    // channel group; when the number of groups is even ("paired" packing, see pack_x6) the last tap of an EVEN group is
    // deferred and paired with the last tap of the following ODD group, as that group's first K-step - both halo tiles
    // are resident then, the even one in the other LDS buffer (it is overwritten only at the end of the odd group) - so
    // no MFMA work is spent on zero padding (3x3: 9 K-steps per two groups instead of 10).
    //   mode 0 (plain): NKS = ceil(T/2) per group, last pair padded with zero weights
    //   mode 1 (even group of a pair): (T-1)/2 K-steps;  mode 2 (odd group): (T-1)/2 + 1 K-steps
    typedef TapPairs<G> TP;
    const bool paired = TP::paired(CB);
    const bf16x8 *wl = reinterpret_cast<const bf16x8 *>(wpk) + lane;
    const int last = TP::last(CB);   // last K-step of the weight stream
    bf16x8 w0[NT], w1[NT], w2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { w2[nt] = wl[(2 * NT + nt) * 64]; w1[nt] = wl[(1 * NT + nt) * 64]; w0[nt] = wl[(0 * NT + nt) * 64]; }
    const int pb = ((wave * 4 * G::TW + xl) * 2 + (g & 1)) * 16;   // bytes inside a split plane, tap (0,0)
    int stream = 0;                                                  // K-step index inside the weight stream
    int tapsel = g >> 1;

    auto group = [&](auto mode_tag, int cb) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr int NK = TP::nk(MODE);
        constexpr int PER = (G::NLD + (NK > 0 ? NK : 1) - 1) / (NK > 0 ? NK : 1);   // staging loads issued per K-step
        const bool more = cb + 1 < CB;
        const unsigned short *nxt_grp = grp0 + (size_t)min(cb + 1, CB - 1) * grp_sz;   // clamped: loads stay unconditional
        const char *buf = reinterpret_cast<const char *>(lds + (cb & 1) * G::PIECES);
        const char *prv = reinterpret_cast<const char *>(lds + ((cb + 1) & 1) * G::PIECES);
        // per-lane address of this lane's tap of K-step ks (lanes g < 2: first tap of the pair, g >= 2: second)
        auto xaddr = [&](int ks) -> const char * {
            int tA = 2 * ks, tB = 2 * ks + 1;
            bool prevA = false;
            if (MODE == 0 && tB >= G::TAPS) tB = tA;
            if (MODE == 2) {   // first K-step of an odd group: the deferred tap of the even group + this group's last tap
                if (ks == 0) { tA = tB = G::TAPS - 1; prevA = true; }
                else { tA = 2 * (ks - 1); tB = tA + 1; }
            }
            const int oA = tap_off(tA, KW, G::TW), oB = tap_off(tB, KW, G::TW);
            return (tapsel ? buf + oB : (prevA ? prv : buf) + oA) + pb;
        };
        bf16x8 xa[4], xb[4], x1[4], x2[4];   // x0 fragments alternate between xa (even K-steps) and xb (odd)
        if (NK == 0) {   // 1x1 source, even group: nothing to compute yet, only fetch the partner group
            tile_load(plan, nxt_grp, r);
        } else {
            const char *p0 = xaddr(0);
#pragma unroll
            for (int m = 0; m < 4; ++m) xa[m] = *reinterpret_cast<const bf16x8 *>(p0 + m * G::TW * 32);
        }
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            asm volatile("" : "+v"(tapsel));   // keeps hipcc from hoisting every K-step's tap offset out of the group loop
            const char *px = xaddr(ks);
            ++stream;
            const bf16x8 *wk = wl + (size_t)min(stream, last) * (3 * NT * 64);
            bf16x8 (&x0)[4] = (ks & 1) ? xb : xa;
            bf16x8 (&x0n)[4] = (ks & 1) ? xa : xb;
            {
#pragma unroll
                for (int m = 0; m < 4; ++m) x1[m] = *reinterpret_cast<const bf16x8 *>(px + G::PLANE * 16 + m * G::TW * 32);
#pragma unroll
                for (int m = 0; m < 4; ++m) x2[m] = *reinterpret_cast<const bf16x8 *>(px + 2 * G::PLANE * 16 + m * G::TW * 32);
            }
            tile_load(plan, nxt_grp, r, ks * PER, (ks + 1) * PER);
            __builtin_amdgcn_sched_barrier(0);
            // phase A
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[nt], x0[m], acc[m][nt], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w2[nt] = wk[(2 * NT + nt) * 64];
            __builtin_amdgcn_sched_barrier(0);
            // phase B
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[nt], x0[m], acc[m][nt], 0, 0, 0);
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[nt], x1[m], acc[m][nt], 0, 0, 0);
                }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w1[nt] = wk[(1 * NT + nt) * 64];
            if (ks + 1 < NK) {
                const char *pn = xaddr(ks + 1);
#pragma unroll
                for (int m = 0; m < 4; ++m) x0n[m] = *reinterpret_cast<const bf16x8 *>(pn + m * G::TW * 32);
            }
            __builtin_amdgcn_sched_barrier(0);
            // phase C
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0[nt], x0[m], acc[m][nt], 0, 0, 0);
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0[nt], x1[m], acc[m][nt], 0, 0, 0);
                    acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0[nt], x2[m], acc[m][nt], 0, 0, 0);
                }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w0[nt] = wk[(0 * NT + nt) * 64];
            __builtin_amdgcn_sched_barrier(0);
            // The cross-group K-step is the only one that reads the OTHER halo buffer; every wave must be past it before any
            // wave overwrites that buffer at the end of this group (the waves of a workgroup are only loosely in step).
            if (MODE == 2 && ks == 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        // the partner buffer is only overwritten here, after the last K-step that may read the previous group from it
        if (more) x6_stage_store<KH, KW>(plan, lds + ((cb + 1) & 1) * G::PIECES, r);
        __syncthreads();
    };

    if (paired) {
        for (int cb = 0; cb < CB; cb += 2) {
            group(std::integral_constant<int, 1>{}, cb);
            group(std::integral_constant<int, 2>{}, cb + 1);
        }
    } else {
        for (int cb = 0; cb < CB; ++cb) group(std::integral_constant<int, 0>{}, cb);
    }
}

template <int KH, int KW, int NT>
__global__ __launch_bounds__(256, 2) void conv_x6_kernel(ConvX6Args a)
{
    typedef GeoX<KH, KW> G;
    __shared__ u32x4 lds[2 * G::PIECES];
    const int tiles_x = a.W >> 4, tiles = tiles_x * (a.H >> 4);
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles, ty = t / tiles_x, tx = t - ty * tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, xl = lane & 15, g = lane >> 4;

    f32x4 acc[4][NT];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    x6_accumulate<KH, KW, NT>(a.x, a.x_stride, a.w, a.Cin, a.H, a.W, n, ty, tx, lds, acc);
    if (a.x_sc) x6_accumulate<1, 1, NT>(a.x_sc, a.sc_stride, a.w_sc, a.Csc, a.H, a.W, n, ty, tx, lds, acc);

    const int H = a.H, W = a.W;
    const size_t grp = (size_t)H * W * 16;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int y = ty * 16 + wave * 4 + m, x = tx * 16 + xl;
            const size_t off = ((size_t)n * NT + nt) * grp + ((size_t)y * W + x) * 16 + g * 4;
            f32x4 v = acc[m][nt];
            if (a.res) v += load_split4(a.res + off, a.res_stride);
            if (a.relu) v = relu4(v);
            if (a.gate) v *= load_split4(a.gate + off, a.gate_stride);
            acc[m][nt] = v;
        }
        if (!a.pool) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int y = ty * 16 + wave * 4 + m, x = tx * 16 + xl;
                const size_t off = ((size_t)n * NT + nt) * grp + ((size_t)y * W + x) * 16 + g * 4;
                if (a.out_f32) *reinterpret_cast<f32x4 *>(a.out_f32 + off) = acc[m][nt];
                else store_split4(a.out + off, a.out_stride, acc[m][nt]);
            }
        } else {
            const int Ho = H >> 1, Wo = W >> 1;
#pragma unroll
            for (int m = 0; m < 4; m += 2) {
                const f32x4 v = pool2x2_max(acc[m][nt], acc[m + 1][nt]);
                if ((xl & 1) == 0) {
                    const int yo = ty * 8 + wave * 2 + (m >> 1), xo = tx * 8 + (xl >> 1);
                    const size_t off = (((size_t)n * NT + nt) * Ho + yo) * Wo * 16 + (size_t)xo * 16 + g * 4;
                    if (a.out_f32) *reinterpret_cast<f32x4 *>(a.out_f32 + off) = v;
                    else store_split4(a.out + off, a.out_stride, v);
                }
            }
        }
    }
}

template <int KH, int KW>
static hipError_t launch_x6(hipStream_t s, const ConvX6Args &a)
{
    const int grid = a.N * (a.H >> 4) * (a.W >> 4);
    return dispatch_cout(a.Cout, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        note_launch("conv_x6_kernel", KH, KW, NT);
        hipLaunchKernelGGL((conv_x6_kernel<KH, KW, NT>), dim3(grid), dim3(256), 0, s, a);
    });
}

hipError_t launch_conv_x6(hipStream_t s, const ConvX6Args &a)
{
    if (!conv_shape_ok(a)) return hipErrorInvalidValue;
    if (a.KH == 3 && a.KW == 3) return launch_x6<3, 3>(s, a);
    if (a.KH == 5 && a.KW == 5) return launch_x6<5, 5>(s, a);
    if (a.KH == 1 && a.KW == 1) return launch_x6<1, 1>(s, a);
    return hipErrorInvalidValue;
}

// ---- format converters (conv_tile.h) ------------------------------------------------------------------------------
hipError_t launch_f32_to_split3(hipStream_t s, const float *x, unsigned short *out, size_t n, size_t plane_stride)
{
    return launch_f32_to_split<FMT_B3>(s, x, out, n, plane_stride, nullptr);
}

hipError_t launch_split3_to_f32(hipStream_t s, const unsigned short *x, float *out, size_t n, size_t plane_stride)
{
    return launch_split_to_f32<FMT_B3>(s, x, out, n, plane_stride);
}

}  // namespace pmp
