// conv_tile.h — what the MFMA convolution kernels share (conv_mfma.hip, conv_bf16x6.hip, conv_f16x3.hip; the epilogue helpers also
// rbfuse32.hip and tail16_dev.h): the staging plan of a halo tile, the ReLU and 2x2 max-pool of an accumulator, the arithmetic of the tap
// pairing, the launchers' validation and dispatch, and the format converters.  Product kernels only: the measurement library's forks of
// these kernels keep their own copies.
#pragma once
#include <type_traits>

#include "pmp_kernels.h"
#include "split3.h"

namespace pmp {

// ---- halo-tile staging of the split-plane kernels (G = GeoX<KH, KW> / GeoH<KH, KW>, split3.h; 256 staging threads) ----------------
// Per-lane staging plan, computed ONCE per workgroup: element offset (inside one 16-channel group, split plane
// included) of each 16-B piece this thread copies, and a validity mask for the zero padding.  The per-group work is then
// one add per piece; recomputing the div/mod chain per group cost ~80 VALU issue slots per K-step, which matters when a
// 16-cycle bf16 MFMA leaves only 8 free issue cycles.
template <class G>
struct TilePlan {
    unsigned off[G::NLD];
    unsigned valid;
};

template <int KH, int KW, class G>
__device__ __forceinline__ void tile_plan(TilePlan<G> &p, size_t plane_stride, int H, int W, int ty, int tx)
{
    constexpr int PY = KH / 2, PX = KW / 2;
    p.valid = 0;
#pragma unroll
    for (int k = 0; k < G::NLD; ++k) {
        const int i = min((int)threadIdx.x + k * 256, G::PIECES - 1);
        const int sp = i / G::PLANE, j = i - sp * G::PLANE, pix = j >> 1, half = j & 1;
        const int row = pix / G::TW, col = pix - row * G::TW;
        const int gy = ty * 16 + row - PY, gx = tx * 16 + col - PX;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W && (int)threadIdx.x + k * 256 < G::PIECES;
        if (in) p.valid |= 1u << k;
        const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);   // clamped: loads stay unconditional
        p.off[k] = (unsigned)(sp * plane_stride + ((size_t)cy * W + cx) * 16 + half * 8);
    }
}

// (The stores to LDS stay with their kernels: they differ on purpose.)
template <class G, bool OPQ = false>
__device__ __forceinline__ void tile_load(const TilePlan<G> &p, const unsigned short *__restrict__ grp, u32x4 (&r)[G::NLD], int k0 = 0,
                                          int k1 = 1 << 20)
{
#pragma unroll
    for (int k = 0; k < G::NLD; ++k) {
        if (k < k0 || k >= k1) continue;   // folds away: callers pass constants into unrolled code
        unsigned off = p.off[k];
        if (OPQ) asm volatile("" : "+v"(off));   // opaque: the offset stays ONE register across the group loop (hipcc otherwise keeps its 64-bit extension, NLD more registers)
        r[k] = *reinterpret_cast<const u32x4 *>(grp + off);   // default cache policy: the non-temporal hint measured 1 % slower
    }
}

// ---- tap pairing of the split-plane kernels.  A K-step covers 16 channels x 2 taps (conv_bf16x6.hip: "Tap pairing"); a channel group
// runs in one of three modes: 0 plain (last pair zero-padded), 1 even group of a pair (its last tap is deferred), 2 odd group (its
// first K-step = the deferred tap + its own last tap).
template <class G>
struct TapPairs {
    static constexpr int nk(int mode) { return mode == 0 ? G::NKS : (mode == 1 ? (G::TAPS - 1) / 2 : (G::TAPS - 1) / 2 + 1); }   // K-steps of a group
    static constexpr bool paired(int CB) { return (CB & 1) == 0 && (G::TAPS & 1); }                                            // CB = channel groups of the pass
    static constexpr int last(int CB) { return paired(CB) ? (CB / 2) * G::TAPS - 1 : CB * G::NKS - 1; }                        // last K-step of the weight stream
};
// byte offset of tap t inside a split plane of a halo tile TW pixels wide (32 B per pixel)
constexpr int tap_off(int t, int KW, int TW) { return ((t / KW) * TW + t % KW) * 32; }

// ---- epilogue pieces on an accumulator fragment (4 couts of one pixel per lane, 16 pixels of a row across the lanes xl) -----------
__device__ __forceinline__ f32x4 relu4(f32x4 v)   // max(v, 0): maps a NaN to 0
{
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    return v;
}

// 2x2 max-pool: rows (m, m+1) live in this lane (v, u), columns (x, x^1) in the neighbouring lane; lanes with even xl store the result
__device__ __forceinline__ f32x4 pool2x2_max(f32x4 v, f32x4 u)
{
    v.x = fmaxf(v.x, u.x); v.y = fmaxf(v.y, u.y); v.z = fmaxf(v.z, u.z); v.w = fmaxf(v.w, u.w);
    f32x4 o;
    o.x = __shfl_xor(v.x, 1); o.y = __shfl_xor(v.y, 1); o.z = __shfl_xor(v.z, 1); o.w = __shfl_xor(v.w, 1);
    v.x = fmaxf(v.x, o.x); v.y = fmaxf(v.y, o.y); v.z = fmaxf(v.z, o.z); v.w = fmaxf(v.w, o.w);
    return v;
}

// ---- launch entry ------------------------------------------------------------------------------------------------------------------
template <class Args>   // ConvMfmaArgs / ConvX6Args
inline bool conv_shape_ok(const Args &a)
{
    if ((a.H & 15) || (a.W & 15) || (a.Cin & 15) || (a.Cout & 15) || (a.x_sc && (a.Csc & 15)) || a.N <= 0) return false;
    return !(a.pool && a.gate);
}

// launch(std::integral_constant<int, NT>) for the NT = Cout / 16 the kernels are built for
template <class F>
inline hipError_t dispatch_cout(int Cout, F launch)
{
    switch (Cout >> 4) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- format converters: fp32 blocked tensor <-> split planes of format FMT (n4 = elements / 4) ---------------------------------------
// (Internal linkage, as tail16_dev.h's: neither the kernels nor their launchers are the library's dynamic symbols.)
namespace {

template <int FMT>
__global__ __launch_bounds__(256) void f32_to_split_kernel(const float *__restrict__ x, unsigned short *__restrict__ out, size_t n4,
                                                           size_t plane_stride, unsigned *sat)
{
    float amax = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(x + i * 4);
        if (FMT == FMT_H2) amax = sat_amax4(amax, v);
        store_fmt4<FMT>(out + i * 4, plane_stride, v);
    }
    if (FMT == FMT_H2) sat_report(sat, amax);   // only the split-2 store clamps
}

template <int FMT>
__global__ __launch_bounds__(256) void split_to_f32_kernel(const unsigned short *__restrict__ x, float *__restrict__ out, size_t n4,
                                                           size_t plane_stride)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
        *reinterpret_cast<f32x4 *>(out + i * 4) = load_fmt4<FMT>(x + i * 4, plane_stride);
}

inline unsigned convert_grid(size_t n4)   // the kernels stride over what the grid does not cover
{
    const size_t blocks = (n4 + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

template <int FMT>
inline hipError_t launch_f32_to_split(hipStream_t s, const float *x, unsigned short *out, size_t n, size_t plane_stride, unsigned *sat)
{
    const size_t n4 = n / 4;
    if (n4) hipLaunchKernelGGL(f32_to_split_kernel<FMT>, dim3(convert_grid(n4)), dim3(256), 0, s, x, out, n4, plane_stride, sat);
    return hipGetLastError();
}

template <int FMT>
inline hipError_t launch_split_to_f32(hipStream_t s, const unsigned short *x, float *out, size_t n, size_t plane_stride)
{
    const size_t n4 = n / 4;
    if (n4) hipLaunchKernelGGL(split_to_f32_kernel<FMT>, dim3(convert_grid(n4)), dim3(256), 0, s, x, out, n4, plane_stride);
    return hipGetLastError();
}

}  // namespace

}  // namespace pmp
