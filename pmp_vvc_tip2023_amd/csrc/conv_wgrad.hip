// conv_wgrad.hip — what a ResidualBlock's backward pass needs beside the forward convolution kernel (api_train.cpp):
// the weight gradient on the fp32 matrix cores, and the small kernels between torch's dense tensors and the blocked layout.
//
// Weight gradient:  dW[co][ci][dy][dx] = sum over (n, y, x) of G[n][co][y][x] * A[n][ci][y + dy - K/2][x + dx - K/2], zero outside
// the image.  A GEMM that reduces over PIXELS, where the forward kernel reduces over (tap, channel):
//   MFMA 16x16x4:  A operand = G       (lane: co = l&15, pixel 4s + (l>>4) of a tile row),
//                  B operand = A's pixels shifted by the tap (lane: ci = l&15, the same pixel),
//                  D: lane holds dW[co = 4(l>>4) .. +3][ci = l&15] of one (co-group, ci-group, tap): one 16x16 tile per triple.
// Work unit: the forward kernel's - one 16x16 pixel tile of one block - for ONE 16-channel group of A, whose (16+K-1)^2 halo tile
// is staged in LDS with the channels of a pixel contiguous, so the 64 lanes of a B read (4 pixels x 16 channels) hit 64 consecutive
// words.  G needs no halo and no reuse across lanes: each lane reads its operand word straight from global memory, one row ahead.
// A workgroup (4 waves) owns the NCO x K*K accumulator tiles of its channel group: wave w takes co-group w % NCO and every
// (4/NCO)-th tap - 25 tiles = 100 VGPRs for a 5x5 layer with 64 output channels - and keeps them in registers over all its tiles.
// Where that leaves a wave short of taps (K = 1, the shortcut's gradient, with fewer than 64 output channels: 4/NCO waves share ONE
// tap) it repeats the last tap and throws the result away: correct, and wasted work on a reduction that is 1/K^2 of its neighbours'.
// Splitting the 16 tile rows over those waves instead would need a cross-wave add of the accumulators; not built.
//
// The reduction over (n, tile) is two-stage and deterministic.  Stage 1: workgroup (p, cb) adds the work items p, p + NP, ... in
// that order and writes its accumulators as they lie in the registers; NP = min(ceil(items / 2), 256 / groups) depends on the
// shape only.  Stage 2 adds the NP partials of every element in the order 0 .. NP-1 and writes torch's dense [cout][cin][K][K],
// leaving the padded channels out.  No atomics: the same bits on every run, stream, context and device.
#include "pmp_kernels.h"

namespace pmp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
struct WgradArgs {
    const float *a;     // [N][CB][H][W][16]
    const float *g;     // [N][NCO][H][W][16]
    float *part;        // [NP][CB][NCO][K*K][64 lanes][4]
    int N, H, W;
};
}  // namespace

template <int K, int NCO>
__global__ __launch_bounds__(256) void wgrad_partial_kernel(WgradArgs a)
{
    constexpr int TW = 16 + K - 1, TAPS = K * K, NS = 4 / NCO, NACC = (TAPS + NS - 1) / NS, PAD = K / 2;
    __shared__ float lds[TW * TW * 16];
    const int tid = threadIdx.x, lane = tid & 63, ch = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = wave % NCO, ts = wave / NCO;                 // this wave's co-group and its taps ts, ts + NS, ...
    const int p = blockIdx.x, NP = gridDim.x, cb = blockIdx.y, CB = gridDim.y;
    const int H = a.H, W = a.W, tiles_x = W >> 4, tiles = tiles_x * (H >> 4), items = a.N * tiles;

    f32x4 acc[NACC];
    int toff[NACC];                                             // the tap's offset in the halo tile, in words (wave-uniform)
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int t = min(ts + NS * i, TAPS - 1);               // a wave short of taps repeats the last one and does not store it
        toff[i] = ((t / K) * TW + t % K) * 16;
    }

    for (int it = p; it < items; it += NP) {
        const int n = it / tiles, tt = it - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
        __syncthreads();                                        // everyone is done reading the previous tile
        const float *plane = a.a + ((size_t)n * CB + cb) * H * W * 16;
        for (int i = tid; i < TW * TW * 4; i += 256) {
            const int pix = i >> 2, s = i & 3, row = pix / TW, col = pix - row * TW;
            const int gy = ty * 16 + row - PAD, gx = tx * 16 + col - PAD;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const f32x4 *>(plane + ((size_t)gy * W + gx) * 16 + s * 4);
            *reinterpret_cast<f32x4 *>(lds + pix * 16 + s * 4) = v;
        }
        __syncthreads();
        // lane (ch, g) of k-step s in row y: G's pixel (y, 4s + g), channel ch
        const float *gp = a.g + ((((size_t)n * NCO + cg) * H + ty * 16) * W + tx * 16 + g) * 16 + ch;
        const size_t grow = (size_t)W * 16;
        float gv[4], gn[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) gv[s] = gp[s * 64];
        for (int y = 0; y < 16; ++y) {
            const float *gq = gp + (size_t)min(y + 1, 15) * grow;
#pragma unroll
            for (int s = 0; s < 4; ++s) gn[s] = gq[s * 64];
            const float *lrow = lds + (y * TW + g) * 16 + ch;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < NACC; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[s], lrow[toff[i] + s * 64], acc[i], 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s) gv[s] = gn[s];
        }
    }

    f32x4 *out = reinterpret_cast<f32x4 *>(a.part) + (((size_t)p * CB + cb) * NCO + cg) * TAPS * 64 + lane;
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        const int t = ts + NS * i;
        if (t < TAPS) out[t * 64] = acc[i];
    }
}

// Stage 2: one thread per word of a partial (coalesced reads), partials added in the order 0 .. NP-1, dense store of the real channels
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, int NP, int CB, int NCO,
                                                           int TAPS, int cout, int cin)
{
    const int words = CB * NCO * TAPS * 256, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    float s = part[i];
    for (int p = 1; p < NP; ++p) s += part[(size_t)p * words + i];
    const int r = i & 3, lane = (i >> 2) & 63, tile = i >> 8, t = tile % TAPS, cg = (tile / TAPS) % NCO, cb = tile / (TAPS * NCO);
    const int co = cg * 16 + (lane >> 4) * 4 + r, ci = cb * 16 + (lane & 15);
    if (co < cout && ci < cin) dw[((size_t)co * cin + ci) * TAPS + t] = s;
}

static int wgrad_np(int N, int H, int W, int Ca)
{
    const int items = N * (H >> 4) * (W >> 4), cap = 256 / (Ca >> 4);
    return (items + 1) / 2 < cap ? (items + 1) / 2 : cap;
}

size_t wgrad_partial_floats(int N, int H, int W, int Ca, int Cg, int K)
{
    return (size_t)wgrad_np(N, H, W, Ca) * (Ca >> 4) * (Cg >> 4) * K * K * 256;
}

template <int K>
static hipError_t launch_wgrad_k(hipStream_t s, const WgradArgs &a, int NP, int CB, int NCO)
{
    const dim3 grid(NP, CB);
    switch (NCO) {
    case 1: hipLaunchKernelGGL((wgrad_partial_kernel<K, 1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((wgrad_partial_kernel<K, 2>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((wgrad_partial_kernel<K, 4>), grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_wgrad(hipStream_t s, const float *a, const float *g, int N, int H, int W, int Ca, int Cg, int K, float *part,
                        float *dw, int cout, int cin)
{
    if (N <= 0 || (H & 15) || (W & 15) || H <= 0 || W <= 0 || (Ca != 16 && Ca != 32 && Ca != 64 && Ca != 128) || (Cg != 16 && Cg != 32 && Cg != 64) ||
        cout < 1 || cout > Cg || cin < 1 || cin > Ca)
        return hipErrorInvalidValue;
    const int NP = wgrad_np(N, H, W, Ca), CB = Ca >> 4, NCO = Cg >> 4;
    const WgradArgs wa{a, g, part, N, H, W};
    hipError_t e;
    if (K == 1) e = launch_wgrad_k<1>(s, wa, NP, CB, NCO);
    else if (K == 3) e = launch_wgrad_k<3>(s, wa, NP, CB, NCO);
    else if (K == 5) e = launch_wgrad_k<5>(s, wa, NP, CB, NCO);
    else return hipErrorInvalidValue;
    if (e != hipSuccess) return e;
    const int words = CB * NCO * K * K * 256;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((words + 255) / 256), dim3(256), 0, s, part, dw, NP, CB, NCO, K * K, cout, cin);
    return hipGetLastError();
}

// ---- dense NCHW <-> blocked.  One workgroup per (block, channel group, row, 16 columns): 16 channels x 16 pixels through LDS, so both
// sides move whole 64-byte pieces.  Channels C .. Cp-1 of the blocked side are written as zeros and dropped on the way back.
// mode 0: v = src;  1: v = m > 0 ? src : 0 (the upstream gradient behind a ReLU)
__global__ __launch_bounds__(256) void dense_to_blocked_kernel(const float *__restrict__ src, const float *__restrict__ m, int mode,
                                                               float *__restrict__ dst, int C, int G, int H, int W)
{
    __shared__ float tile[16][17];
    const int tid = threadIdx.x, wc = W >> 4;
    unsigned b = blockIdx.x;
    const int xc = b % wc; b /= wc;
    const int y = b % H; b /= H;
    const int grp = b % G, n = b / G;
    const int c = grp * 16 + (tid >> 4), x = xc * 16 + (tid & 15);
    float v = 0.f;
    if (c < C) {
        const size_t i = (((size_t)n * C + c) * H + y) * W + x;
        v = src[i];
        if (mode == 1) v = relu_on(m[i]) ? v : 0.f;
    }
    tile[tid >> 4][tid & 15] = v;
    __syncthreads();
    dst[((((size_t)n * G + grp) * H + y) * W + xc * 16) * 16 + tid] = tile[tid & 15][tid >> 4];
}

__global__ __launch_bounds__(256) void blocked_to_dense_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int G, int H, int W)
{
    __shared__ float tile[16][17];
    const int tid = threadIdx.x, wc = W >> 4;
    unsigned b = blockIdx.x;
    const int xc = b % wc; b /= wc;
    const int y = b % H; b /= H;
    const int grp = b % G, n = b / G;
    tile[tid & 15][tid >> 4] = src[((((size_t)n * G + grp) * H + y) * W + xc * 16) * 16 + tid];
    __syncthreads();
    const int c = grp * 16 + (tid >> 4), x = xc * 16 + (tid & 15);
    if (c < C) dst[(((size_t)n * C + c) * H + y) * W + x] = tile[tid >> 4][tid & 15];
}

hipError_t launch_dense_to_blocked(hipStream_t s, const float *src, const float *m, int mode, float *dst, int N, int C, int Cp, int H, int W)
{
    if (N <= 0 || C < 1 || C > Cp || (Cp & 15) || (W & 15) || H <= 0 || W <= 0 || mode < 0 || mode > 1 || (mode == 1 && !m))
        return hipErrorInvalidValue;
    const size_t blocks = (size_t)N * (Cp >> 4) * H * (W >> 4);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dense_to_blocked_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, m, mode, dst, C, Cp >> 4, H, W);
    return hipGetLastError();
}

hipError_t launch_blocked_to_dense(hipStream_t s, const float *src, float *dst, int N, int C, int Cp, int H, int W)
{
    if (N <= 0 || C < 1 || C > Cp || (Cp & 15) || (W & 15) || H <= 0 || W <= 0) return hipErrorInvalidValue;
    const size_t blocks = (size_t)N * (Cp >> 4) * H * (W >> 4);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blocked_to_dense_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, C, Cp >> 4, H, W);
    return hipGetLastError();
}

// ---- weights: torch's [cout][cin][K][K] on the device -> pack_mfma's fragment order [CB][K*K][NT][64 lanes][4] (pack.cpp), padded with
// zeros.  flip_t = 0: the forward convolution's weights (NT covers cout, CB covers cin).  flip_t = 1: the data gradient's - taps
// mirrored, cin and cout swapped (NT covers cin, CB covers cout).
__global__ __launch_bounds__(256) void pack_mfma_kernel(const float *__restrict__ w, float *__restrict__ out, int cout, int cin, int TAPS,
                                                        int NT, int CB, int flip_t)
{
    const int total = CB * TAPS * NT * 256, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = i & 3, l = (i >> 2) & 63, f = i >> 8, nt = f % NT, t = (f / NT) % TAPS, cb = f / (NT * TAPS);
    const int o = nt * 16 + (l & 15), c = cb * 16 + 4 * (l >> 4) + j;      // the packed convolution's output and input channel
    float v = 0.f;
    if (!flip_t) { if (o < cout && c < cin) v = w[((size_t)o * cin + c) * TAPS + t]; }
    else if (o < cin && c < cout) v = w[((size_t)c * cin + o) * TAPS + (TAPS - 1 - t)];
    out[i] = v;
}

hipError_t launch_pack_mfma(hipStream_t s, const float *w, float *out, int cout, int cin, int K, int NT, int CB, int flip_t)
{
    const int o = flip_t ? cin : cout, c = flip_t ? cout : cin;
    // flip_t with more than 16 NT input channels: the first 16 NT of them (a QT tail's 128-channel gradient is packed in two halves)
    if (cout < 1 || cin < 1 || (o > NT * 16 && !flip_t) || c > CB * 16 || (K != 1 && K != 3 && K != 5)) return hipErrorInvalidValue;
    const int total = CB * K * K * NT * 256;
    hipLaunchKernelGGL(pack_mfma_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w, out, cout, cin, K * K, NT, CB, flip_t);
    return hipGetLastError();
}

}  // namespace pmp
