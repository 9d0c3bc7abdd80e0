// trunk_glue.hip — what a trunk of ResidualBlocks needs between its convolutions when the activations STAY in the blocked layout
// [n][c/16][y][x][c%16] (api_train.cpp: pmp_trunk_*): the ReLU backward and the ReLU mask blocked -> blocked, the 2x2 max-pool behind
// the last block blocked -> dense, and its backward (fused with the last block's ReLU backward) dense -> blocked.  All of them move
// every element once and are bound by HBM: 16-byte loads and stores on the blocked side, a lane's four words being four channels of
// one pixel, so that a wave covers 1 KiB of consecutive bytes.  Padded channels (>= the real count) are zero in every blocked input
// and come out as zero: `> 0` is false for them, and the dense side supplies zeros.  (For FINITE inputs: 0 * inf = NaN in a padded lane,
// and a NaN opens a mask as it opens torch's - include/pmp.h, NON-FINITE VALUES IN THE TRAINING CALLS.)
#include "pmp_kernels.h"

namespace pmp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// mode 1: dst = a where m > 0 or m is NaN (relu_on), else +0;  2: dst = [relu_on(a)], the ReLU mask itself.  In both dst may be a: every thread reads its own
// words before it writes them, and no other thread touches them (mode 2 in place: a single block's backward, api_train.cpp).
// A workgroup moves 1024 consecutive 16-byte pieces, four per thread; n4 (a whole number of 16x16 tiles of 16 channels) is a multiple
// of 1024, and the guard is there for a caller that breaks that.
template <int MODE>
__global__ __launch_bounds__(256) void blocked_relu_kernel(const f32x4 *a, const f32x4 *m, f32x4 *dst, size_t n4)
{
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    f32x4 v[4], w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t j = base + i * 256;
        if (j < n4) {
            v[i] = a[j];
            if (MODE == 1) w[i] = m[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t j = base + i * 256;
        if (j >= n4) continue;
        f32x4 r;
        if (MODE == 1) {
            r.x = relu_on(w[i].x) ? v[i].x : 0.f; r.y = relu_on(w[i].y) ? v[i].y : 0.f;
            r.z = relu_on(w[i].z) ? v[i].z : 0.f; r.w = relu_on(w[i].w) ? v[i].w : 0.f;
        } else {
            r.x = relu_on(v[i].x) ? 1.f : 0.f; r.y = relu_on(v[i].y) ? 1.f : 0.f;
            r.z = relu_on(v[i].z) ? 1.f : 0.f; r.w = relu_on(v[i].w) ? 1.f : 0.f;
        }
        dst[j] = r;
    }
}

hipError_t launch_blocked_relu(hipStream_t s, int mode, const float *a, const float *m, float *dst, int N, int Cp, int H, int W)
{
    if (N <= 0 || Cp <= 0 || (Cp & 15) || H <= 0 || W <= 0 || (H & 15) || (W & 15) || (mode != 1 && mode != 2) || (mode == 1 && !m))
        return hipErrorInvalidValue;
    const size_t n4 = (size_t)N * Cp * H * W / 4, blocks = (n4 + 1023) / 1024;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const f32x4 *a4 = reinterpret_cast<const f32x4 *>(a), *m4 = reinterpret_cast<const f32x4 *>(m);
    if (mode == 1) hipLaunchKernelGGL(blocked_relu_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a4, m4, reinterpret_cast<f32x4 *>(dst), n4);
    else hipLaunchKernelGGL(blocked_relu_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, a4, m4, reinterpret_cast<f32x4 *>(dst), n4);
    return hipGetLastError();
}

// ---- the work unit of the two pool kernels: 4 rows x 16 columns of one 16-channel group of one image - 256 pieces of 16 bytes, one
// per thread: thread (row r = tid >> 6, pixel px = (tid >> 2) & 15, channel quad q = tid & 3).  A wave moves one row of the unit:
// 1 KiB of consecutive bytes.
struct PoolUnit {
    int n, grp, y0, x0;
    __device__ PoolUnit(int G, int H, int W)
    {
        const int wc = W >> 4, hc = H >> 2;
        unsigned b = blockIdx.x;
        x0 = (b % wc) * 16; b /= wc;
        y0 = (b % hc) * 4; b /= hc;
        grp = b % G; n = b / G;
    }
};

// out (blocked, un-pooled) -> y dense [N][C][H/2][W/2], y = max of the 2x2 window.  The maximum is taken as conv_mfma's pool epilogue
// takes it - the two rows of a column first, then the even column with the odd one - so that the bits are that epilogue's.
__global__ __launch_bounds__(256) void pool_to_dense_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int G, int H, int W)
{
    __shared__ f32x4 tile[4][16][4 + 1];                        // [row][pixel][quad], a pixel's 16 channels padded to 20 words
    const PoolUnit u(G, H, W);
    const int tid = threadIdx.x, r = tid >> 6, px = (tid >> 2) & 15, q = tid & 3;
    tile[r][px][q] = *reinterpret_cast<const f32x4 *>(src + ((((size_t)u.n * G + u.grp) * H + u.y0 + r) * W + u.x0 + px) * 16 + q * 4);
    __syncthreads();
    // thread (channel ch = tid >> 4, output row ro = (tid >> 3) & 1, output column xo = tid & 7): 8 lanes store 32 consecutive bytes
    const int ch = tid >> 4, ro = (tid >> 3) & 1, xo = tid & 7, c = u.grp * 16 + ch;
    const float *t = reinterpret_cast<const float *>(tile);
    auto at = [&](int row, int col) { return t[((row * 16 + col) * 5) * 4 + ch]; };
    const float v = max_nan(max_nan(at(2 * ro, 2 * xo), at(2 * ro + 1, 2 * xo)), max_nan(at(2 * ro, 2 * xo + 1), at(2 * ro + 1, 2 * xo + 1)));
    if (c < C) dst[(((size_t)u.n * C + c) * (H >> 1) + (u.y0 >> 1) + ro) * (W >> 1) + (u.x0 >> 1) + xo] = v;
}

hipError_t launch_pool_to_dense(hipStream_t s, const float *src, float *dst, int N, int C, int Cp, int H, int W)
{
    if (N <= 0 || C < 1 || C > Cp || (Cp & 15) || (H & 15) || (W & 15) || H <= 0 || W <= 0) return hipErrorInvalidValue;
    const size_t blocks = (size_t)N * (Cp >> 4) * (H >> 2) * (W >> 4);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pool_to_dense_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, C, Cp >> 4, H, W);
    return hipGetLastError();
}

// The upstream gradient of a trunk, dense, -> the blocked gu of its last block (every element written, padded channels +0).
// POOL = 0: g [N][C][H][W],      gu = g where out > 0, else +0.
// POOL = 1: g [N][C][H/2][W/2],  gu[y][x] = g[y/2][x/2] where out[y][x] > 0 and (y, x) is the FIRST maximum of its 2x2 window in the
//           order (0,0), (0,1), (1,0), (1,1) - torch's max_pool2d keeps the earlier element on a tie (`val > maxval` replaces) - or the
//           window's LAST NaN (`|| isnan(val)`), else +0.
template <int POOL>
__global__ __launch_bounds__(256) void grad_to_blocked_kernel(const float *__restrict__ g, const float *__restrict__ out, float *__restrict__ dst,
                                                              int C, int G, int H, int W)
{
    constexpr int GR = POOL ? 2 : 4, GX = POOL ? 8 : 16, GS = GR * GX + 1;      // the unit's piece of g: GR rows x GX columns per channel
    __shared__ float gl[16 * GS];
    __shared__ f32x4 tile[POOL ? 4 * 16 * 5 : 1];
    const PoolUnit u(G, H, W);
    const int tid = threadIdx.x, r = tid >> 6, px = (tid >> 2) & 15, q = tid & 3;
    const int Hg = POOL ? H >> 1 : H, Wg = POOL ? W >> 1 : W, gy0 = POOL ? u.y0 >> 1 : u.y0, gx0 = POOL ? u.x0 >> 1 : u.x0;
    for (int i = tid; i < 16 * GR * GX; i += 256) {
        const int ch = i / (GR * GX), rr = (i / GX) % GR, xx = i % GX, c = u.grp * 16 + ch;
        gl[ch * GS + rr * GX + xx] = c < C ? g[(((size_t)u.n * C + c) * Hg + gy0 + rr) * Wg + gx0 + xx] : 0.f;
    }
    const size_t off = ((((size_t)u.n * G + u.grp) * H + u.y0 + r) * W + u.x0 + px) * 16 + q * 4;
    const f32x4 o = *reinterpret_cast<const f32x4 *>(out + off);
    if (POOL) tile[(r * 16 + px) * 5 + q] = o;
    __syncthreads();
    const float ov[4] = {o.x, o.y, o.z, o.w};
    float res[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ch = q * 4 + j;
        bool take = relu_on(ov[j]);
        if (POOL) {
            const float *t = reinterpret_cast<const float *>(tile);
            const int wy = r & ~1, wx = px & ~1;
            int first = 0;
            float best = t[((wy * 16 + wx) * 5) * 4 + ch];
#pragma unroll
            for (int e = 1; e < 4; ++e) {
                const float v = t[(((wy + (e >> 1)) * 16 + wx + (e & 1)) * 5) * 4 + ch];
                if (pool_takes(v, best)) { best = v; first = e; }
            }
            take = take && first == ((r & 1) * 2 + (px & 1));
        }
        res[j] = take ? gl[ch * GS + (POOL ? (r >> 1) * GX + (px >> 1) : r * GX + px)] : 0.f;
    }
    *reinterpret_cast<f32x4 *>(dst + off) = (f32x4){res[0], res[1], res[2], res[3]};
}

hipError_t launch_grad_to_blocked(hipStream_t s, int pool, const float *g, const float *out, float *dst, int N, int C, int Cp, int H, int W)
{
    if (N <= 0 || C < 1 || C > Cp || (Cp & 15) || (H & 15) || (W & 15) || H <= 0 || W <= 0) return hipErrorInvalidValue;
    const size_t blocks = (size_t)N * (Cp >> 4) * (H >> 2) * (W >> 4);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (pool) hipLaunchKernelGGL(grad_to_blocked_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, g, out, dst, C, Cp >> 4, H, W);
    else hipLaunchKernelGGL(grad_to_blocked_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, g, out, dst, C, Cp >> 4, H, W);
    return hipGetLastError();
}

}  // namespace pmp
