// head_train.hip — an MTT net's head for a trainer (include/pmp.h: pmp_head_*, pmp_gate_*; api_train.cpp): the 3x3 bias convolution
// conv_B1..3 (cin 1..16 inputs, cout 1 or 2 outputs), the carry into its channel 0, the next attention trunk's input written in the
// same pass, their gradients, and the gate product.  Dense NCHW fp32 in and out.  The formulas and every order of summation are
// stated ONCE, in include/pmp.h; the kernels below only say how the work is laid out.
//
// Direct fp32 kernels, no MFMA: with at most 2 outputs a 16-wide matrix tile would be 7/8 padding (DESIGN.md section 10 gives the
// same reason for the stem's input gradient).  The file is built with -ffp-contract=off: every fused multiply-add below is written
// as fmaf(), and the bias, the carry, the window sums and the gate's product and sum round one operation at a time.
//
// head_forward_kernel   one 16x16 tile of one image per workgroup, one pixel per thread, both outputs: the (cin x 18 x 18) halo tile
//                       of x and the weights (zeros above cout) in LDS.  Writes y and, with up_y, the pixel's up_y x up_y cells of
//                       every channel of att.  Threads beyond H or W (8-multiples) only help staging.
// head_dgrad_kernel     the same tiling: the halo tile of the effective gradient gy (head_gy) in LDS, its 2 x 9 values of a pixel in
//                       registers, then one chain per input channel.
// head_wgrad_kernel     stage 1 of g_w and g_b: workgroup p of NP takes the 8x8-tile items p, p + NP, ...; thread c < 9 cin + 1 owns
//                       column c - tap (ci, dy, dx) = c, or the bias at c = 9 cin, whose "pixels" are 1.0 - for both outputs.  It
//                       writes its partial [NP][cout][9 cin + 1] in full, and g_prev of its items' pixels when that is asked for
//                       (every pixel belongs to exactly one item).
// head_reduce_kernel    stage 2: partials added in the order 0 .. NP-1, stored dense into g_w and g_b.
// head_gq_kernel        g_q: one thread per element, its up_q x up_q window of g_att's channel 0 in row-major order.
// gate_forward_kernel / gate_backward_kernel   grid-stride, VEC = 4: float4 accesses (all pointers 16-byte aligned) with the last
//                       count % 4 elements scalar; VEC = 1: scalar throughout.
// No atomics anywhere; no kernel reads the workspace beyond the partials this call wrote.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 256 threads; no scratch, no VGPR and no SGPR spills in any of them):
//   kernel                   VGPRs   LDS bytes   waves / SIMD
//   head_forward_kernel       30      21888       7
//   head_dgrad_kernel         70       3744       7
//   head_wgrad_kernel         38       6912       8
//   head_reduce_kernel         7          0       8
//   head_gq_kernel            14          0       8
//   gate_forward_kernel<4>    18          0       8
//   gate_forward_kernel<1>    10          0       8
//   gate_backward_kernel<4>   20          0       8
//   gate_backward_kernel<1>   10          0       8
#include <initializer_list>

#include "pmp_kernels.h"

namespace pmp {

namespace {

constexpr int HEAD_MAX_CIN = 16, HEAD_MAX_W = 2 * HEAD_MAX_CIN * 9, HEAD_TW = 18, HEAD_CAP = 128;

// the weights [cout][cin][3][3] into LDS as [2][cin][9], zeros for the output a cout = 1 head does not have
__device__ __forceinline__ void stage_w(const HeadTrainArgs &a, float *ws, int tid)
{
    for (int i = tid; i < 2 * a.cin * 9; i += 256) ws[i] = i < a.cout * a.cin * 9 ? a.w[i] : 0.f;
}

// the effective gradient of the carried y (include/pmp.h): g_y, then the up_y x up_y window of g_att in row-major order
__device__ __forceinline__ float head_gy(const HeadTrainArgs &a, int n, int co, int Y, int X)
{
    float v = a.g_y[(((size_t)n * a.cout + co) * a.H + Y) * a.W + X];
    if (a.up_y) {
        const int U = a.up_y, WA = U * a.W;
        const float *g = a.g_att + (((size_t)n * (1 + a.cout) + 1 + co) * U * a.H + (size_t)U * Y) * WA + U * X;
        for (int i = 0; i < U; ++i)
            for (int j = 0; j < U; ++j) v = v + g[(size_t)i * WA + j];
    }
    return v;
}

}  // namespace

__global__ __launch_bounds__(256) void head_forward_kernel(HeadTrainArgs a)
{
    __shared__ float xs[HEAD_MAX_CIN * HEAD_TW * HEAD_TW];
    __shared__ float ws[HEAD_MAX_W];
    constexpr int TW = HEAD_TW, TT = TW * TW;
    const int tid = threadIdx.x, ly = tid >> 4, lx = tid & 15, H = a.H, W = a.W, cin = a.cin;
    const int tiles_x = (W + 15) >> 4, tiles = tiles_x * ((H + 15) >> 4);
    const int n = blockIdx.x / tiles, tt = blockIdx.x - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const float *img = a.x + (size_t)n * cin * H * W;
    for (int i = tid; i < cin * TT; i += 256) {
        const int ci = i / TT, r = i - ci * TT, row = r / TW, col = r - row * TW, gy = ty * 16 + row - 1, gx = tx * 16 + col - 1;
        xs[i] = gy >= 0 && gy < H && gx >= 0 && gx < W ? img[((size_t)ci * H + gy) * W + gx] : 0.f;
    }
    stage_w(a, ws, tid);
    __syncthreads();
    const int Y = ty * 16 + ly, X = tx * 16 + lx;
    if (Y >= H || X >= W) return;

    float acc[2] = {0.f, 0.f};
    const float *w1 = ws + cin * 9;
    for (int ci = 0; ci < cin; ++ci) {
        const float *xp = xs + ci * TT + ly * TW + lx;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float xv = xp[dy * TW + dx];
                acc[0] = fmaf(ws[ci * 9 + dy * 3 + dx], xv, acc[0]);
                acc[1] = fmaf(w1[ci * 9 + dy * 3 + dx], xv, acc[1]);
            }
    }
    const int U = a.up_y, HA = U * H, WA = U * W;
    for (int co = 0; co < a.cout; ++co) {
        const size_t at = (((size_t)n * a.cout + co) * H + Y) * W + X;
        float v = acc[co] + a.b[co];
        if (a.prev && co == 0) v = v + a.prev[at];
        a.y[at] = v;
        for (int i = 0; i < U; ++i)
            for (int j = 0; j < U; ++j) a.att[(((size_t)n * (1 + a.cout) + 1 + co) * HA + U * Y + i) * WA + U * X + j] = v;
    }
    if (U) {
        const int HQ = HA / a.up_q, WQ = WA / a.up_q;
        for (int i = 0; i < U; ++i)
            for (int j = 0; j < U; ++j) {
                const int YA = U * Y + i, XA = U * X + j;
                a.att[((size_t)n * (1 + a.cout) * HA + YA) * WA + XA] = a.q[((size_t)n * HQ + YA / a.up_q) * WQ + XA / a.up_q];
            }
    }
}

__global__ __launch_bounds__(256) void head_dgrad_kernel(HeadTrainArgs a)
{
    __shared__ float gs[2 * HEAD_TW * HEAD_TW];
    __shared__ float ws[HEAD_MAX_W];
    constexpr int TW = HEAD_TW, TT = TW * TW;
    const int tid = threadIdx.x, ly = tid >> 4, lx = tid & 15, H = a.H, W = a.W, cin = a.cin;
    const int tiles_x = (W + 15) >> 4, tiles = tiles_x * ((H + 15) >> 4);
    const int n = blockIdx.x / tiles, tt = blockIdx.x - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    for (int i = tid; i < 2 * TT; i += 256) {
        const int co = i / TT, r = i - co * TT, row = r / TW, col = r - row * TW, gy = ty * 16 + row - 1, gx = tx * 16 + col - 1;
        gs[i] = co < a.cout && gy >= 0 && gy < H && gx >= 0 && gx < W ? head_gy(a, n, co, gy, gx) : 0.f;
    }
    stage_w(a, ws, tid);
    __syncthreads();
    const int Y = ty * 16 + ly, X = tx * 16 + lx;
    if (Y >= H || X >= W) return;

    float g[2][9];                                               // g[co][dy * 3 + dx] = gy[co][Y + 1 - dy][X + 1 - dx]
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) g[co][dy * 3 + dx] = gs[co * TT + (ly + 2 - dy) * TW + lx + 2 - dx];
    for (int ci = 0; ci < cin; ++ci) {
        float acc = 0.f;
#pragma unroll
        for (int co = 0; co < 2; ++co)                           // the second output of a cout = 1 head adds +0 * +0
#pragma unroll
            for (int t = 0; t < 9; ++t) acc = fmaf(ws[(co * cin + ci) * 9 + t], g[co][t], acc);
        a.g_x[(((size_t)n * cin + ci) * H + Y) * W + X] = acc;
    }
}

__global__ __launch_bounds__(256) void head_wgrad_kernel(HeadTrainArgs a, float *__restrict__ part)
{
    __shared__ float xs[HEAD_MAX_CIN * 100];                     // the 10 x 10 halo of an item's 8 x 8 tile, per input channel
    __shared__ float gs[2 * 64];                                 // gy of its pixels, zeros for the output a cout = 1 head lacks
    const int tid = threadIdx.x, H = a.H, W = a.W, cin = a.cin, CW = cin * 9 + 1;
    const int p = blockIdx.x, NP = gridDim.x, tiles_x = W >> 3, tiles = tiles_x * (H >> 3), items = a.N * tiles;
    const int ci = tid / 9, t = tid - ci * 9, off = tid < cin * 9 ? ci * 100 + (t / 3) * 10 + t % 3 : -1;   // -1: the bias column
    float acc0 = 0.f, acc1 = 0.f;
    for (int it = p; it < items; it += NP) {
        const int n = it / tiles, tt = it - n * tiles, ty = tt / tiles_x, tx = tt - ty * tiles_x;
        __syncthreads();                                         // everyone is done reading the previous item
        for (int i = tid; i < cin * 100; i += 256) {
            const int c = i / 100, r = i - c * 100, row = r / 10, col = r - row * 10, gy = ty * 8 + row - 1, gx = tx * 8 + col - 1;
            xs[i] = gy >= 0 && gy < H && gx >= 0 && gx < W ? a.x[(((size_t)n * cin + c) * H + gy) * W + gx] : 0.f;
        }
        if (tid < 128) {
            const int co = tid >> 6, px = tid & 63, Y = ty * 8 + (px >> 3), X = tx * 8 + (px & 7);
            const float v = co < a.cout ? head_gy(a, n, co, Y, X) : 0.f;
            gs[tid] = v;
            if (a.g_prev && co < a.cout) a.g_prev[(((size_t)n * a.cout + co) * H + Y) * W + X] = co == 0 ? v : 0.f;
        }
        __syncthreads();
        if (tid < CW) {
#pragma unroll 1
            for (int py = 0; py < 8; ++py)
#pragma unroll
                for (int px = 0; px < 8; ++px) {
                    const float xv = off < 0 ? 1.f : xs[(off < 0 ? 0 : off) + py * 10 + px];
                    acc0 = fmaf(gs[py * 8 + px], xv, acc0);
                    acc1 = fmaf(gs[64 + py * 8 + px], xv, acc1);
                }
        }
    }
    if (tid < CW) {
        part[((size_t)p * a.cout) * CW + tid] = acc0;
        if (a.cout == 2) part[((size_t)p * 2 + 1) * CW + tid] = acc1;
    }
}

__global__ __launch_bounds__(256) void head_reduce_kernel(HeadTrainArgs a, const float *__restrict__ part, int NP)
{
    const int CW = a.cin * 9 + 1, words = a.cout * CW, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    float s = part[i];
    for (int p = 1; p < NP; ++p) s = s + part[(size_t)p * words + i];
    const int co = i / CW, col = i - co * CW;
    if (col == CW - 1) a.g_b[co] = s;
    else a.g_w[co * (CW - 1) + col] = s;
}

__global__ __launch_bounds__(256) void head_gq_kernel(HeadTrainArgs a)
{
    const int HA = a.up_y * a.H, WA = a.up_y * a.W, Q = a.up_q, HQ = HA / Q, WQ = WA / Q;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.N * HQ * WQ) return;
    const int X = (int)(i % WQ), Y = (int)(i / WQ % HQ), n = (int)(i / ((size_t)WQ * HQ));
    const float *g = a.g_att + ((size_t)n * (1 + a.cout) * HA + (size_t)Q * Y) * WA + Q * X;
    float s = 0.f;
    for (int r = 0; r < Q; ++r)
        for (int c = 0; c < Q; ++c) s = s + g[(size_t)r * WA + c];
    a.g_q[i] = s;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int VEC>
__global__ __launch_bounds__(256) void gate_forward_kernel(size_t count, const float *__restrict__ x, const float *__restrict__ g, float *__restrict__ y)
{
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x, body = VEC == 4 ? count >> 2 : 0;
    if (VEC == 4)
        for (size_t i = first; i < body; i += stride)
            reinterpret_cast<f32x4 *>(y)[i] = reinterpret_cast<const f32x4 *>(x)[i] * reinterpret_cast<const f32x4 *>(g)[i];
    for (size_t i = 4 * body + first; i < count; i += stride) y[i] = x[i] * g[i];
}

template <int VEC>
__global__ __launch_bounds__(256) void gate_backward_kernel(size_t count, const float *__restrict__ x, const float *__restrict__ g,
                                                            const float *__restrict__ g_y, const float *__restrict__ g_acc,
                                                            float *__restrict__ g_x, float *__restrict__ g_a)
{
    const size_t stride = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x, body = VEC == 4 ? count >> 2 : 0;
    if (VEC == 4)
        for (size_t i = first; i < body; i += stride) {
            const f32x4 gy = reinterpret_cast<const f32x4 *>(g_y)[i];
            reinterpret_cast<f32x4 *>(g_a)[i] = gy * reinterpret_cast<const f32x4 *>(x)[i];
            const f32x4 v = gy * reinterpret_cast<const f32x4 *>(g)[i];
            reinterpret_cast<f32x4 *>(g_x)[i] = g_acc ? reinterpret_cast<const f32x4 *>(g_acc)[i] + v : v;
        }
    for (size_t i = 4 * body + first; i < count; i += stride) {
        const float gy = g_y[i], v = gy * g[i];
        g_a[i] = gy * x[i];
        g_x[i] = g_acc ? g_acc[i] + v : v;
    }
}

// ---- launchers.  The shapes are pmp_head_*'s (train_check.h head_shape_ok), checked again here: nothing else has a kernel
static bool head_args_ok(const HeadTrainArgs &a)
{
    auto side = [](int v) { return v >= 8 && v <= 256 && !(v & 7); };
    return a.N >= 1 && a.N <= 256 && side(a.H) && side(a.W) && a.cin >= 1 && a.cin <= HEAD_MAX_CIN && (a.cout == 1 || a.cout == 2) &&
           ((a.up_q == 0 && a.up_y == 0) || (a.up_q == 2 && a.up_y == 1) || (a.up_q == 4 && a.up_y == 2));
}

static int head_np(int N, int H, int W)
{
    const int items = N * (H >> 3) * (W >> 3);
    return (items + 1) / 2 < HEAD_CAP ? (items + 1) / 2 : HEAD_CAP;
}

size_t head_partial_floats(int N, int H, int W, int cin, int cout) { return (size_t)head_np(N, H, W) * cout * (cin * 9 + 1); }

hipError_t launch_head_forward(hipStream_t s, const HeadTrainArgs &a)
{
    if (!head_args_ok(a) || !a.x || !a.w || !a.b || !a.y || (a.up_y != 0) != (a.att != nullptr) || (a.up_y != 0) != (a.q != nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(head_forward_kernel, dim3((unsigned)(a.N * ((a.H + 15) >> 4) * ((a.W + 15) >> 4))), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_head_backward(hipStream_t s, const HeadTrainArgs &a, float *part)
{
    if (!head_args_ok(a) || !a.x || !a.w || !a.g_y || !a.g_w || !a.g_b || !part || (a.up_y != 0) != (a.g_att != nullptr) || (a.g_q && !a.g_att))
        return hipErrorInvalidValue;
    const int NP = head_np(a.N, a.H, a.W);
    hipLaunchKernelGGL(head_wgrad_kernel, dim3((unsigned)NP), dim3(256), 0, s, a, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_reduce_kernel, dim3((a.cout * (a.cin * 9 + 1) + 255) / 256), dim3(256), 0, s, a, (const float *)part, NP);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.g_x) {
        hipLaunchKernelGGL(head_dgrad_kernel, dim3((unsigned)(a.N * ((a.H + 15) >> 4) * ((a.W + 15) >> 4))), dim3(256), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (a.g_q) {
        const size_t cells = (size_t)a.N * (a.up_y * a.H / a.up_q) * (a.up_y * a.W / a.up_q);
        hipLaunchKernelGGL(head_gq_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, a);
        e = hipGetLastError();
    }
    return e;
}

static unsigned gate_grid(size_t count, int vec)
{
    const size_t blocks = (count / vec + 255) / 256 + (count < (size_t)vec);      // at least one: the tail's threads are block 0's
    return (unsigned)(blocks < 4096 ? blocks : 4096);
}

static bool aligned16(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}

hipError_t launch_gate_forward(hipStream_t s, size_t count, const float *x, const float *a, float *y)
{
    if (!count || !x || !a || !y) return hipErrorInvalidValue;
    if (aligned16({x, a, y})) hipLaunchKernelGGL(gate_forward_kernel<4>, dim3(gate_grid(count, 4)), dim3(256), 0, s, count, x, a, y);
    else hipLaunchKernelGGL(gate_forward_kernel<1>, dim3(gate_grid(count, 1)), dim3(256), 0, s, count, x, a, y);
    return hipGetLastError();
}

hipError_t launch_gate_backward(hipStream_t s, size_t count, const float *x, const float *a, const float *g_y, const float *g_acc, float *g_x,
                                float *g_a)
{
    if (!count || !x || !a || !g_y || !g_x || !g_a) return hipErrorInvalidValue;
    if (aligned16({x, a, g_y, g_acc, g_x, g_a}))
        hipLaunchKernelGGL(gate_backward_kernel<4>, dim3(gate_grid(count, 4)), dim3(256), 0, s, count, x, a, g_y, g_acc, g_x, g_a);
    else
        hipLaunchKernelGGL(gate_backward_kernel<1>, dim3(gate_grid(count, 1)), dim3(256), 0, s, count, x, a, g_y, g_acc, g_x, g_a);
    return hipGetLastError();
}

}  // namespace pmp
