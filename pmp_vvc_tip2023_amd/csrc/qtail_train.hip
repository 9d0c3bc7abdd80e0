// qtail_train.hip — what a QT net's tail (include/pmp.h: pmp_qtail_*, api_train.cpp) needs between its four ResidualBlocks, which run
// on conv_mfma.hip and conv_wgrad.hip like every other block: the multi-scale pool and its backward, q5's 2x2 pool into q6's map and
// back, and the way between q6's map and the caller's dense x9 / g_x9.  Everything is blocked [n][c/16][y][x][c%16]; a thread moves
// one 16-byte piece, four channels of one pixel.  These kernels take maxima, select and add - there is no product in them - and
// every sum is written one addition at a time in the order include/pmp.h states.
//
// q6's map: the h/2 x w/2 pixels lie top-left in a map of H2 x W2 (the sides rounded up to 16) whose other pixels are +0.
#include "pmp_kernels.h"

namespace pmp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {       // the kernels too: the launcher below is this file's one name (and the library is held to a size)

__device__ __forceinline__ f32x4 vmax(f32x4 a, f32x4 b)
{
    return (f32x4){max_nan(a.x, b.x), max_nan(a.y, b.y), max_nan(a.z, b.z), max_nan(a.w, b.w)};
}

// The grid of every kernel here: x = the pieces of a row, 256 per workgroup, y = the row, z = (image, channel group) of a tensor
// [N][G][H][W][16] with G = 1 << LG groups.  ok: the thread has a piece; i: the piece's index in that tensor.
struct Piece {
    int q, x, y, grp, n;
    bool ok;
    size_t i;
    __device__ Piece(int LG, int H, int W)
    {
        const int xq = blockIdx.x * 256 + threadIdx.x;
        q = xq & 3; x = xq >> 2; y = blockIdx.y;
        grp = blockIdx.z & ((1 << LG) - 1); n = blockIdx.z >> LG;
        ok = x < W;
        i = (((size_t)blockIdx.z * H + y) * W + x) * 4 + q;
    }
};

__device__ __forceinline__ size_t piece_at(int n, int G, int grp, int H, int W, int y, int x, int q)
{
    return ((((size_t)n * G + grp) * H + y) * W + x) * 4 + q;
}

// x5 [N][2][H][W][16] -> x6 [N][8][H][W][16]: groups 0, 1 = x5; groups 2 ls, 2 ls + 1 = the maximum of x5 over the 2^ls-window
__global__ __launch_bounds__(256) void qt_multipool_kernel(const f32x4 *__restrict__ x5, f32x4 *__restrict__ x6, int H, int W)
{
    const Piece p(1, H, W);
    if (!p.ok) return;
    const size_t i = p.i;
    const int y8 = p.y & ~7, x8 = p.x & ~7;
    f32x4 m[4];
    m[0] = x5[i];
    m[1] = m[2] = m[3] = m[0];
    for (int dy = 0; dy < 8; ++dy)
        for (int dx = 0; dx < 8; ++dx) {
            const int yy = y8 + dy, xx = x8 + dx;
            const f32x4 v = x5[piece_at(p.n, 2, p.grp, H, W, yy, xx, p.q)];
            m[3] = vmax(m[3], v);
            if ((yy >> 2) == (p.y >> 2) && (xx >> 2) == (p.x >> 2)) m[2] = vmax(m[2], v);
            if ((yy >> 1) == (p.y >> 1) && (xx >> 1) == (p.x >> 1)) m[1] = vmax(m[1], v);
        }
#pragma unroll
    for (int ls = 0; ls < 4; ++ls) x6[piece_at(p.n, 8, 2 * ls + p.grp, H, W, p.y, p.x, p.q)] = m[ls];
}

// g6 as two tensors [N][4][H][W][16] (channels 0..63 and 64..127) and x5 -> q3's upstream gradient [N][2][H][W][16]:
// g = g6[c]; g = g + r2; g = g + r4; g = g + r8; out = relu_on(x5) ? g : +0 (x5 > 0 or NaN)  (include/pmp.h: MULTI-SCALE POOL, BACKWARD)
__global__ __launch_bounds__(256) void qt_multipool_back_kernel(const f32x4 *__restrict__ ga, const f32x4 *__restrict__ gb,
                                                                const f32x4 *__restrict__ x5, f32x4 *__restrict__ out, int H, int W)
{
    const Piece p(1, H, W);
    if (!p.ok) return;
    const size_t i = p.i;
    const int y8 = p.y & ~7, x8 = p.x & ~7, mine = ((p.y & 7) << 3) | (p.x & 7);
    float best[3][4];
    int first[3][4];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) { best[l][j] = -__builtin_inff(); first[l][j] = -1; }
    for (int dy = 0; dy < 8; ++dy)
        for (int dx = 0; dx < 8; ++dx) {
            const int yy = y8 + dy, xx = x8 + dx;
            const f32x4 v4 = x5[piece_at(p.n, 2, p.grp, H, W, yy, xx, p.q)];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const int sh = l + 1;                                    // the window of side 2^sh that holds this thread's pixel
                if ((yy >> sh) != (p.y >> sh) || (xx >> sh) != (p.x >> sh)) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pool_takes(v[j], best[l][j])) { best[l][j] = v[j]; first[l][j] = (dy << 3) | dx; }
            }
        }
    const f32x4 g0 = ga[piece_at(p.n, 4, p.grp, H, W, p.y, p.x, p.q)];
    float g[4] = {g0.x, g0.y, g0.z, g0.w};
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const int sh = l + 1, s = 1 << sh, ys = p.y & ~(s - 1), xs = p.x & ~(s - 1);
        const bool any = first[l][0] == mine || first[l][1] == mine || first[l][2] == mine || first[l][3] == mine;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        if (any) {
            const f32x4 *src = l == 0 ? ga : gb;                         // channels 32 + c: ga's groups 2, 3;  64 + c, 96 + c: gb's 0, 1 and 2, 3
            const int grp = (l == 1 ? 0 : 2) + p.grp;
            for (int dy = 0; dy < s; ++dy)
                for (int dx = 0; dx < s; ++dx) {
                    const f32x4 v = src[piece_at(p.n, 4, grp, H, W, ys + dy, xs + dx, p.q)];
                    r[0] = r[0] + v.x; r[1] = r[1] + v.y; r[2] = r[2] + v.z; r[3] = r[3] + v.w;
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = g[j] + (first[l][j] == mine ? r[j] : 0.f);
    }
    const f32x4 me = x5[i];
    out[i] = (f32x4){relu_on(me.x) ? g[0] : 0.f, relu_on(me.y) ? g[1] : 0.f, relu_on(me.z) ? g[2] : 0.f, relu_on(me.w) ? g[3] : 0.f};
}

// q5's out [N][2][H][W][16] -> x8 [N][2][H2][W2][16]: the 2x2 maximum inside the H/2 x W/2 region, +0 outside it; and, if asked for,
// the region's mask [N][1][H2][W2][16]: 1 inside, 0 outside
__global__ __launch_bounds__(256) void qt_pool_embed_kernel(const f32x4 *__restrict__ o5, f32x4 *__restrict__ x8, f32x4 *__restrict__ mask,
                                                            int H, int W, int H2, int W2)
{
    const Piece p(1, H2, W2);
    if (!p.ok) return;
    const size_t i = p.i;
    const bool in = p.y < (H >> 1) && p.x < (W >> 1);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (in) {
        const size_t a = piece_at(p.n, 2, p.grp, H, W, 2 * p.y, 2 * p.x, p.q), row = (size_t)W * 4;
        v = vmax(vmax(o5[a], o5[a + 4]), vmax(o5[a + row], o5[a + row + 4]));
    }
    x8[i] = v;
    const float one = in ? 1.f : 0.f;
    if (mask && p.grp == 0) mask[piece_at(p.n, 1, 0, H2, W2, p.y, p.x, p.q)] = (f32x4){one, one, one, one};
}

// q6's data gradient g8 [N][2][H2][W2][16] and q5's out [N][2][H][W][16] -> q5's upstream gradient [N][2][H][W][16]:
// g8[y/2][x/2] where out > 0 or NaN (relu_on) and (y, x) is the first maximum of its 2x2 window in the order (0,0), (0,1), (1,0), (1,1) - or
// the window's last NaN (pool_takes) -, else +0
__global__ __launch_bounds__(256) void qt_pool_back_kernel(const f32x4 *__restrict__ g8, const f32x4 *__restrict__ o5, f32x4 *__restrict__ out,
                                                           int H, int W, int H2, int W2)
{
    const Piece p(1, H, W);
    if (!p.ok) return;
    const size_t i = p.i;
    const size_t a = piece_at(p.n, 2, p.grp, H, W, p.y & ~1, p.x & ~1, p.q), row = (size_t)W * 4;
    const f32x4 e[4] = {o5[a], o5[a + 4], o5[a + row], o5[a + row + 4]};
    const f32x4 g = g8[piece_at(p.n, 2, p.grp, H2, W2, p.y >> 1, p.x >> 1, p.q)];
    const int mine = (p.y & 1) * 2 + (p.x & 1);
    float res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float best = e[0][j];
        int first = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (pool_takes(e[k][j], best)) { best = e[k][j]; first = k; }
        res[j] = (first == mine && relu_on(e[mine][j])) ? g[j] : 0.f;
    }
    out[i] = (f32x4){res[0], res[1], res[2], res[3]};
}

// the dense g_x9 [N][8][H/2][W/2] and q6's out [N][1][H2][W2][16] -> q6's upstream gradient [N][1][H2][W2][16]: g where out > 0 or NaN (which
// is inside the region and in channels 0..7 only), else +0
__global__ __launch_bounds__(256) void qt_embed_grad_kernel(const float *__restrict__ g, const f32x4 *__restrict__ o6, f32x4 *__restrict__ out,
                                                            int H, int W, int H2, int W2)
{
    const Piece p(0, H2, W2);
    if (!p.ok) return;
    const size_t i = p.i;
    const int hh = H >> 1, wh = W >> 1;
    const f32x4 o = o6[i];
    float res[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.y < hh && p.x < wh && p.q < 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (relu_on(o[j])) res[j] = g[(((size_t)p.n * 8 + p.q * 4 + j) * hh + p.y) * wh + p.x];
    }
    out[i] = (f32x4){res[0], res[1], res[2], res[3]};
}

// a tensor of q6's map [N][1][H2][W2][16] -> dense [N][8][H/2][W/2]
__global__ __launch_bounds__(256) void qt_crop_dense_kernel(const float *__restrict__ src, float *__restrict__ dst, int H, int W, int H2, int W2)
{
    // grid: x = the columns, y = the row, z = (image, channel)
    const int hh = H >> 1, wh = W >> 1, x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, c = blockIdx.z & 7, n = blockIdx.z >> 3;
    if (x < wh) dst[(((size_t)blockIdx.z * hh) + y) * wh + x] = src[(((size_t)n * H2 + y) * W2 + x) * 16 + c];
}

}  // namespace

hipError_t launch_qtail_step(hipStream_t s, int step, const float *a, const float *b, const float *c, float *out, float *out2, int N, int H, int W)
{
    if (N <= 0 || N > 4096 || H <= 0 || W <= 0 || (H & 15) || (W & 15) || H > 32768 || W > 32768) return hipErrorInvalidValue;
    const int H2 = (H / 2 + 15) & ~15, W2 = (W / 2 + 15) & ~15;
    const dim3 blk(256), full((W * 4 + 255) / 256, H, N * 2), emb2((W2 * 4 + 255) / 256, H2, N * 2), emb1(emb2.x, H2, N),
        crop((W / 2 + 255) / 256, H / 2, N * 8);
    const f32x4 *a4 = reinterpret_cast<const f32x4 *>(a), *b4 = reinterpret_cast<const f32x4 *>(b), *c4 = reinterpret_cast<const f32x4 *>(c);
    f32x4 *o4 = reinterpret_cast<f32x4 *>(out);
    switch (step) {
    case QT_MULTIPOOL: hipLaunchKernelGGL(qt_multipool_kernel, full, blk, 0, s, a4, o4, H, W); break;
    case QT_MULTIPOOL_BACK: hipLaunchKernelGGL(qt_multipool_back_kernel, full, blk, 0, s, a4, b4, c4, o4, H, W); break;
    case QT_POOL_EMBED: hipLaunchKernelGGL(qt_pool_embed_kernel, emb2, blk, 0, s, a4, o4, reinterpret_cast<f32x4 *>(out2), H, W, H2, W2); break;
    case QT_POOL_BACK: hipLaunchKernelGGL(qt_pool_back_kernel, full, blk, 0, s, a4, b4, o4, H, W, H2, W2); break;
    case QT_EMBED_GRAD: hipLaunchKernelGGL(qt_embed_grad_kernel, emb1, blk, 0, s, a, b4, o4, H, W, H2, W2); break;
    case QT_CROP_DENSE: hipLaunchKernelGGL(qt_crop_dense_kernel, crop, blk, 0, s, a, out, H, W, H2, W2); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pmp
