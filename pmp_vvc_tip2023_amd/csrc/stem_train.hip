// stem_train.hip — a net's first layer for a trainer (include/pmp.h: pmp_stem_*; api_train.cpp): forward, weight and bias gradient and
// input gradient of a bias convolution with CIN = 1..4 input channels, 32 outputs and a ReLU, on the exact fp32 matrix cores.
//
// ONE statement of the convolution.  With p = K/2, x is [N][CIN][H+p][W+p] with zeros to its right and below, and
//   y[n][co][yy][xx] = relu(b[co] + sum over (ci, dy, dx) of wu[co][ci][dy][dx] * x[n][ci][yy+dy][xx+dx]),   dy, dx = 0..K-1.
// wu is the UNIFIED K x K kernel: the QT nets' conv_q1 as it is; for the MTT nets (split) conv_b1_1 in outputs 0..15, conv_b1_2
// ((p+1) x K, rows 0..p) in 16..23 and conv_b1_3 (K x (p+1), columns 0..p) in 24..31, zeros elsewhere - stem_slot() below says where
// a tap of wu lives in the caller's three tensors, or that it does not exist; every kernel here goes through it, so the split form
// costs that one mask and no kernels of its own.  The reduction index is r = (ci * K + dy) * K + dx, R = CIN * K * K of them.
//
// Work unit everywhere: one 16x16 tile of one image, whose (16+K-1)^2 x CIN input tile is staged in LDS by dword loads (rows of x are
// only 4-byte aligned), zeros beyond H+p / W+p.  MFMA 16x16x4 f32: A lane l = [row l&15][k l>>4], B lane l = [k l>>4][col l&15],
// D lane l = rows 4(l>>4)..+3 of column l&15; one MFMA is a k-ordered chain of four fused multiply-adds.
//
// Every kernel takes cin and K at run time (the input gradient: K as a template argument, for its unrolled taps): the library
// is held to a size, and a kernel per (cin, K) costs 160 KB of code for shapes whose launches are MFMA- or LDS-bound either way.
//
// stem_pack_kernel    wu -> the forward's A fragments [2 co-groups][ceil(R/4) steps][64 lanes] (co = 16 cg + (l&15), r = 4 s + (l>>4),
//                     zero for r >= R) and the 32 biases behind them.  Every call: the weights change every optimiser step.
// stem_forward_kernel wave v of 4 owns rows 4v..4v+3 of the tile for both co-groups: 8 accumulators; the tile offset of every
//                     reduction index comes from a table in LDS, built once per workgroup.  ORDER of one output element:
//                     acc = b[co]; then acc = fma(wu[co][r], x[..r..], acc) for r = 0 .. R-1 in that order (indices R .. 4 ceil(R/4) - 1
//                     add +0 * 0); relu; store.
// stem_wgrad_kernel   the GEMM that reduces over pixels (conv_wgrad.hip's): A = gm (16 outputs x 4 pixels), gm = g_y where y > 0 or NaN, else
//                     0, staged in LDS per tile; B = the shifted input pixels from the staged tile (4 pixels x 16 columns), column
//                     c < R the reduction index r = c, column R the constant 1.0 - the BIAS gradient, its lanes reading a run of 1.0s
//                     kept behind the tile in LDS - and columns above R up to the next multiple of 16 padding that is never stored.  NT = ceil((R + 1) / 16) column tiles x 2 co-groups of
//                     accumulators stay in registers over a workgroup's tiles: wave v takes co-group v & 1 and the column tiles v >> 1,
//                     (v >> 1) + 2, ... - registers for the 11 tiles of cin = 4, K = 9 (44 AGPRs) in every launch, and a wave-uniform
//                     branch around the MFMAs of the tiles a smaller shape does not have.
//                     ORDER, stage 1: items = N * (H/16) * (W/16) tiles, item = (n * H/16 + ty) * W/16 + tx; NP = min(ceil(items / 2),
//                     512) workgroups, a function of the shape only; workgroup q starts from +0 and adds the items q, q + NP, ... in
//                     that order, every item pixel by pixel in row order (yy = 0..15, xx = 0..15 of the tile), acc = fma(gm, x, acc) -
//                     one rounding per pixel.  It writes its accumulators as they lie in the registers: [NP][2][NT][64 lanes][4].
// stem_reduce_kernel  stage 2: s = partial 0, then s += partial q for q = 1 .. NP-1 in that order, and the dense store into g_w[j]
//                     and g_b[j] through stem_slot(): taps a split kernel does not have are not written anywhere.
// stem_dgrad_kernel<K> g_x[n][ci][Y][X] = sum over (co, dy, dx) of wu[co][ci][dy][dx] * gm[n][co][Y-dy][X-dx], gm zero outside
//                     [0,H) x [0,W): a direct kernel, one thread per (n, Y, X) for four input channels (zero weights above cin, the
//                     first cin stored), gm's halo tile and wu staged in LDS eight outputs at a time.  ORDER of one element:
//                     acc = +0; acc = fma(wu, gm, acc) for co = 0..31, inside that dy = 0..K-1, inside that dx = 0..K-1 (a gm outside
//                     the image enters as 0).  Every element of g_x is written.
// No atomics anywhere: the same bits on every run, stream, context and device.  No kernel reads outside x, y, g_y and the weights, and
// none reads a word of the workspace that this call did not write (the packed weights and the partials are written in full).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 256 threads; no scratch, no VGPR and no SGPR spills in any of them):
//   kernel                 VGPRs + AGPRs   LDS bytes   waves / SIMD
//   stem_pack_kernel        8 +  0              0       8
//   stem_forward_kernel    47 + 32          10528       6     (registers)
//   stem_wgrad_kernel      40 + 44          44032       3     (LDS: 33280 bytes of gm, the largest input tile, 1536 of 1.0s)
//   stem_reduce_kernel      9 +  0              0       8
//   stem_dgrad_kernel<5>   40 +  0          16000       8
//   stem_dgrad_kernel<9>   62 +  0          28800       5     (LDS: 8 outputs of gm's 24 x 24 halo tile + their weights)
#include "pmp_kernels.h"

namespace pmp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// Where tap (co, ci, dy, dx) of the unified kernel lives: tensor j of the caller's three and the element idx in it.  -> false: the
// tap is outside that kernel's support (its weight is zero and it has no gradient)
__device__ __forceinline__ bool stem_slot(int split, int cin, int k, int co, int ci, int dy, int dx, int &j, int &idx)
{
    const int p = k >> 1;
    if (!split || co < 16) { j = 0; idx = ((co * cin + ci) * k + dy) * k + dx; return true; }
    if (co < 24) { j = 1; idx = (((co - 16) * cin + ci) * (p + 1) + dy) * k + dx; return dy <= p; }
    j = 2; idx = (((co - 24) * cin + ci) * k + dy) * (p + 1) + dx; return dx <= p;
}

__device__ __forceinline__ void stem_bias_slot(int split, int co, int &j, int &idx)
{
    if (!split || co < 16) { j = 0; idx = co; }
    else if (co < 24) { j = 1; idx = co - 16; }
    else { j = 2; idx = co - 24; }
}

template <class T>
__device__ __forceinline__ T *pick(T *const p[3], int j) { return j == 0 ? p[0] : j == 1 ? p[1] : p[2]; }

__device__ __forceinline__ float stem_wu(const StemTrainArgs &a, int co, int ci, int dy, int dx)
{
    int j, idx;
    return stem_slot(a.split, a.cin, a.K, co, ci, dy, dx, j, idx) ? pick(a.w, j)[idx] : 0.f;
}

constexpr int ONES = 16 * 24, MAX_TW = 24, MAX_XS = 4 * MAX_TW * MAX_TW, MAX_RS4 = 328, MAX_NACC = 11;   // K = 9, cin = 4: 324 indices, 21 column tiles

// the (16+K-1)^2 x cin input tile of tile (ty, tx) of image n, zeros beyond x.  One division per element: the words of a row of the
// tile are spread over 32 threads (TW <= 24 of them load).
__device__ __forceinline__ void stage_x(const StemTrainArgs &a, float *xs, int n, int ty, int tx, int tid)
{
    const int TW = 16 + a.K - 1, HX = a.H + a.K / 2, WX = a.W + a.K / 2, col = tid & 31;
    const float *img = a.x + (size_t)n * a.cin * HX * WX;
    for (int rc = tid >> 5; rc < a.cin * TW; rc += 8) {
        const int ci = rc / TW, row = rc - ci * TW, gy = ty * 16 + row, gx = tx * 16 + col;
        if (col < TW) xs[rc * TW + col] = gy < HX && gx < WX ? img[((size_t)ci * HX + gy) * WX + gx] : 0.f;
    }
}

// reduction index r -> the offset of x[ci][dy][dx] in the staged tile
__device__ __forceinline__ int tile_offset(int r, int K, int TW)
{
    const int KK = K * K, ci = r / KK, t = r - ci * KK, dy = t / K;
    return ci * TW * TW + dy * TW + (t - dy * K);
}

}  // namespace

__global__ __launch_bounds__(256) void stem_pack_kernel(StemTrainArgs a, float *__restrict__ out)
{
    const int R = a.cin * a.K * a.K, RS = (R + 3) >> 2, frag = 2 * RS * 64, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= frag + 32) return;
    float v = 0.f;
    if (i < frag) {
        const int l = i & 63, s = (i >> 6) % RS, cg = (i >> 6) / RS, co = cg * 16 + (l & 15), r = 4 * s + (l >> 4);
        if (r < R) {
            const int ci = r / (a.K * a.K), t = r - ci * a.K * a.K;
            v = stem_wu(a, co, ci, t / a.K, t % a.K);
        }
    } else {
        int j, idx;
        stem_bias_slot(a.split, i - frag, j, idx);
        v = pick(a.b, j)[idx];
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void stem_forward_kernel(StemTrainArgs a, const float *__restrict__ packed)
{
    __shared__ float xs[MAX_XS];
    __shared__ int offs[MAX_RS4];                               // r -> its offset in the tile, -1 for the padding indices
    const int K = a.K, TW = 16 + K - 1, R = a.cin * K * K, RS = (R + 3) >> 2;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = a.W >> 4, tiles = tiles_x * (a.H >> 4);
    const int n = blockIdx.x / tiles, tt = blockIdx.x - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    stage_x(a, xs, n, ty, tx, tid);
    for (int r = tid; r < 4 * RS; r += 256) offs[r] = r < R ? tile_offset(r, K, TW) : -1;
    __syncthreads();

    f32x4 acc[2][4];
#pragma unroll
    for (int cg = 0; cg < 2; ++cg) {
        const f32x4 b = *reinterpret_cast<const f32x4 *>(packed + 2 * RS * 64 + cg * 16 + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[cg][j] = b;
    }
    const float *wp = packed + lane;
    const float *lrow = xs + wave * 4 * TW + c;                 // row 4 wave + j of the tile, column c
    for (int s = 0; s < RS; ++s) {
        const int off = offs[4 * s + g];
        const float a0 = wp[s * 64], a1 = wp[(RS + s) * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = lrow[(off < 0 ? 0 : off) + j * TW], b = off < 0 ? 0.f : v;
            acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][j], 0, 0, 0);
            acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int cg = 0; cg < 2; ++cg)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = cg * 16 + 4 * g + r;
                a.y_out[(((size_t)n * 32 + co) * a.H + ty * 16 + wave * 4 + j) * a.W + tx * 16 + c] = relu_nan(acc[cg][j][r]);
            }
}

__global__ __launch_bounds__(256) void stem_wgrad_kernel(StemTrainArgs a, float *__restrict__ part)
{
    constexpr int GS = 260;
    __shared__ float xs[MAX_XS + ONES];                         // the input tile, and behind it 1.0s: the bias column's "pixels"
    __shared__ float gs[32 * GS];                               // gm [co][256 pixels], rows 260 apart: an A read hits 64 banks
    const int K = a.K, TW = 16 + K - 1, R = a.cin * K * K, NT = (R + 1 + 15) >> 4;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = wave & 1, half = wave >> 1;
    const int nacc = __builtin_amdgcn_readfirstlane((NT - half + 1) >> 1);     // this wave's column tiles: half, half + 2, ... below NT
    const int q = blockIdx.x, NP = gridDim.x;
    const int H = a.H, W = a.W, tiles_x = W >> 4, tiles = tiles_x * (H >> 4), items = a.N * tiles;

    // accumulator i is column tile half + 2 i; the tiles at and above NT do not exist: a wave-uniform branch skips them
    f32x4 acc[MAX_NACC];
    int off[MAX_NACC];                                          // this lane's column in the staged tile; MAX_XS: the bias column
#pragma unroll
    for (int i = 0; i < MAX_NACC; ++i) {
        acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int col = (half + 2 * i) * 16 + c;
        off[i] = col == R ? MAX_XS : tile_offset(col < R ? col : 0, K, TW);  // padding columns read word 0 and are never stored
    }
    for (int i = tid; i < ONES; i += 256) xs[MAX_XS + i] = 1.f;  // a pixel's offset in the tile, (yy, xx) -> yy TW + xx, stays below ONES

    for (int it = q; it < items; it += NP) {
        const int n = it / tiles, tt = it - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
        __syncthreads();                                        // everyone is done reading the previous tile
        stage_x(a, xs, n, ty, tx, tid);
        for (int i = tid; i < 32 * 256; i += 256) {
            const int co = i >> 8, pix = i & 255;
            const size_t at = (((size_t)n * 32 + co) * H + ty * 16 + (pix >> 4)) * W + tx * 16 + (pix & 15);
            gs[co * GS + pix] = relu_on(a.y[at]) ? a.g_y[at] : 0.f;
        }
        __syncthreads();
        const float *ga = gs + (cg * 16 + c) * GS + g;          // lane (c, g) of k-step s in row yy: gm[co c][pixel (yy, 4 s + g)]
        const float *xb = xs + g;
        for (int yy = 0; yy < 16; ++yy) {
#pragma unroll 1
            for (int s = 0; s < 4; ++s) {
                const float av = ga[yy * 16 + 4 * s];
                const float *xp = xb + yy * TW + 4 * s;
#pragma unroll
                for (int i = 0; i < MAX_NACC; ++i)
                    if (i < nacc) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xp[off[i]], acc[i], 0, 0, 0);
            }
        }
    }

    f32x4 *out = reinterpret_cast<f32x4 *>(part) + ((size_t)q * 2 + cg) * NT * 64 + lane;
#pragma unroll
    for (int i = 0; i < MAX_NACC; ++i) {
        if (i < nacc) out[(half + 2 * i) * 64] = acc[i];
    }
}

// Stage 2: one thread per word of a partial (coalesced reads), partials added in the order 0 .. NP-1, dense stores through stem_slot
__global__ __launch_bounds__(256) void stem_reduce_kernel(StemTrainArgs a, const float *__restrict__ part, int NP, int NT)
{
    const int words = 2 * NT * 256, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    float s = part[i];
    for (int q = 1; q < NP; ++q) s += part[(size_t)q * words + i];
    const int r = i & 3, lane = (i >> 2) & 63, f = i >> 8, tile = f % NT, cg = f / NT;
    const int co = cg * 16 + (lane >> 4) * 4 + r, col = tile * 16 + (lane & 15), KK = a.K * a.K, R = a.cin * KK;
    int j, idx;
    if (col == R) {
        stem_bias_slot(a.split, co, j, idx);
        pick(a.g_b, j)[idx] = s;
    } else if (col < R) {
        const int ci = col / KK, t = col - ci * KK;
        if (stem_slot(a.split, a.cin, a.K, co, ci, t / a.K, t % a.K, j, idx)) pick(a.g_w, j)[idx] = s;
    }
}

// All four input channels are computed, with zero weights above cin, and the first cin stored
template <int K>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(StemTrainArgs a)
{
    constexpr int TW = 16 + K - 1, KK = K * K, COC = 8;
    __shared__ float gs[COC * TW * TW];                         // gm [co][row][col] of rows and columns -(K-1) .. 15 around the tile
    __shared__ f32x4 ws[COC * KK];                              // wu [co][dy][dx][ci, zeros above cin]
    const int tid = threadIdx.x, ly = tid >> 4, lx = tid & 15;
    const int H = a.H, W = a.W, HX = H + K / 2, WX = W + K / 2, tiles_x = (WX + 15) >> 4, tiles = tiles_x * ((HX + 15) >> 4);
    const int n = blockIdx.x / tiles, tt = blockIdx.x - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < 32; c0 += COC) {
        __syncthreads();
        for (int i = tid; i < COC * TW * TW; i += 256) {
            const int co = i / (TW * TW), r = i - co * TW * TW, row = r / TW, col = r - row * TW;
            const int gy = ty * 16 + row - (K - 1), gx = tx * 16 + col - (K - 1);
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t at = (((size_t)n * 32 + c0 + co) * H + gy) * W + gx;
                v = relu_on(a.y[at]) ? a.g_y[at] : 0.f;
            }
            gs[i] = v;
        }
        for (int i = tid; i < COC * KK * 4; i += 256) {
            const int ci = i & 3, t = (i >> 2) % KK, co = (i >> 2) / KK;
            reinterpret_cast<float *>(ws)[i] = ci < a.cin ? stem_wu(a, c0 + co, ci, t / K, t % K) : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int co = 0; co < COC; ++co) {
            const float *gp = gs + co * TW * TW + (ly + K - 1) * TW + lx + K - 1;
            const f32x4 *wp = ws + co * KK;
#pragma unroll 1
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const float gv = gp[-dy * TW - dx];
                    const f32x4 wv = wp[dy * K + dx];
#pragma unroll
                    for (int ci = 0; ci < 4; ++ci) acc[ci] = fmaf(wv[ci], gv, acc[ci]);
                }
        }
    }
    const int Y = ty * 16 + ly, X = tx * 16 + lx;
    if (Y < HX && X < WX)
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
            if (ci < a.cin) a.g_x[(((size_t)n * a.cin + ci) * HX + Y) * WX + X] = acc[ci];
}

// ---- launchers.  The shapes are pmp_stem_*'s (train_check.h stem_shape_ok), checked again here: nothing else has a kernel
static bool stem_args_ok(const StemTrainArgs &a)
{
    return a.N >= 1 && a.H >= 16 && a.W >= 16 && !(a.H & 15) && !(a.W & 15) && a.cin >= 1 && a.cin <= 4 && (a.K == 5 || a.K == 9) &&
           (a.split == 0 || a.split == 1);
}

static int stem_r(int cin, int K) { return cin * K * K; }
static int stem_nt(int cin, int K) { return (stem_r(cin, K) + 1 + 15) / 16; }

static int stem_np(int N, int H, int W)
{
    const int items = N * (H >> 4) * (W >> 4);
    return (items + 1) / 2 < 512 ? (items + 1) / 2 : 512;
}

size_t stem_packed_floats(int cin, int K) { return (size_t)2 * ((stem_r(cin, K) + 3) / 4) * 64 + 32; }

size_t stem_partial_floats(int N, int H, int W, int cin, int K) { return (size_t)stem_np(N, H, W) * 2 * stem_nt(cin, K) * 256; }

hipError_t launch_stem_forward(hipStream_t s, const StemTrainArgs &a, float *packed)
{
    if (!stem_args_ok(a) || !a.x || !a.w[0] || !a.b[0] || !a.y_out || !packed) return hipErrorInvalidValue;
    const int total = (int)stem_packed_floats(a.cin, a.K);
    hipLaunchKernelGGL(stem_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a, packed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stem_forward_kernel, dim3((unsigned)(a.N * (a.H >> 4) * (a.W >> 4))), dim3(256), 0, s, a, (const float *)packed);
    return hipGetLastError();
}

hipError_t launch_stem_wgrad(hipStream_t s, const StemTrainArgs &a, float *part)
{
    if (!stem_args_ok(a) || !a.x || !a.y || !a.g_y || !a.g_w[0] || !a.g_b[0] || !part) return hipErrorInvalidValue;
    const int NP = stem_np(a.N, a.H, a.W), NT = stem_nt(a.cin, a.K);
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3((unsigned)NP), dim3(256), 0, s, a, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stem_reduce_kernel, dim3((2 * NT * 256 + 255) / 256), dim3(256), 0, s, a, (const float *)part, NP, NT);
    return hipGetLastError();
}

hipError_t launch_stem_dgrad(hipStream_t s, const StemTrainArgs &a)
{
    if (!stem_args_ok(a) || !a.y || !a.g_y || !a.w[0] || !a.g_x) return hipErrorInvalidValue;
    const int p = a.K / 2;
    const dim3 grid((unsigned)(a.N * ((a.H + p + 15) >> 4) * ((a.W + p + 15) >> 4)));
    if (a.K == 5) hipLaunchKernelGGL(stem_dgrad_kernel<5>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(stem_dgrad_kernel<9>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace pmp
