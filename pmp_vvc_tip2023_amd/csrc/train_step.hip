// train_step.hip — the two ends of a training step (include/pmp.h, TRAINING STEP): a batch gathered on the device from a data set that
// stays there as bytes, and Adam over every tensor of the step in one launch.  Both are latency-bound at a trainer's sizes (4 MB a
// batch, 43 MB an Adam step): what counts is one launch each and no host in the loop.  Built with -ffp-contract=off: every fused
// multiply-add below is written as fmaf().  And the gradient buckets of data-parallel training: the gradients of a rank packed into one
// buffer, and the ranks' buffers added in rank order, one rounded float32 addition at a time.
#include "pmp_kernels.h"

namespace pmp {
namespace {

constexpr int THREADS = 256;

// four bytes of a row -> four floats.  wide: the output row is 16-byte aligned (a row's length is a multiple of 16 bytes, so one
// row's alignment is every row's)
__device__ inline void put4(float *o, bool wide, uint32_t b, uint32_t minus)
{
    const float4 f = make_float4((float)(uint8_t)((b & 0xFF) - minus), (float)(uint8_t)(((b >> 8) & 0xFF) - minus),
                                 (float)(uint8_t)(((b >> 16) & 0xFF) - minus), (float)(uint8_t)((b >> 24) - minus));
    if (wide) *reinterpret_cast<float4 *>(o) = f;
    else { o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = f.w; }
}

// words 32-bit words of row i of src (ok: i is a row of the set; otherwise nothing is read and zeros go out) -> floats or a copy
__device__ inline void row_floats(const uint8_t *src, int64_t i, bool ok, int words, float *o, uint32_t minus)
{
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src + i * (4 * words));
    const bool wide = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
    for (int w = threadIdx.x; w < words; w += THREADS) put4(o + 4 * w, wide, ok ? s[w] : minus * 0x01010101u, minus);
}

__device__ inline void row_copy(const void *src, int64_t i, bool ok, int words, void *dst, int row)
{
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src) + i * words;
    uint32_t *o = reinterpret_cast<uint32_t *>(dst) + (size_t)row * words;
    for (int w = threadIdx.x; w < words; w += THREADS) o[w] = ok ? s[w] : 0u;
}

// One workgroup per row of the batch.  A row of the set starts on a 4-byte boundary and no better (4624 and 1156 bytes a row), so the
// set is read as 32-bit words, the 2x2 windows of a chroma set's Y as two 16-bit halves
__global__ __launch_bounds__(THREADS) void batch_gather_kernel(pmp_batch_src src, const int64_t *index, pmp_batch_dst dst, int32_t *status)
{
    const int row = blockIdx.x, t = threadIdx.x;
    const int64_t at = index[row];
    const bool ok = at >= 0 && at < src.count;
    const int64_t i = ok ? at : 0;                        // never a pointer outside the set, dereferenced or not
    if (!ok && t == 0) atomicOr(status, 1);
    if (dst.x && !src.u) row_floats(src.y, i, ok, 1156, dst.x + (size_t)row * 4624, 0);
    if (dst.x && src.u) {
        float *o = dst.x + (size_t)row * 3468;
        const uint16_t *y = reinterpret_cast<const uint16_t *>(src.y + i * 4624);      // pair c of line l: y[34 l + c]
        for (int p = t; p < 1156; p += THREADS) {
            const int r = p / 34, c = p - 34 * r;
            const uint32_t a = ok ? y[68 * r + c] : 0, b = ok ? y[68 * r + 34 + c] : 0;
            o[p] = (float)max(max(a & 0xFF, a >> 8), max(b & 0xFF, b >> 8));
        }
        row_floats(src.u, i, ok, 289, o + 1156, 0);
        row_floats(src.v, i, ok, 289, o + 2312, 0);
    }
    if (dst.qt_f) row_floats(src.qt8, i, ok, 16, dst.qt_f + (size_t)row * 64, ok ? 1 : 0);
    if (dst.qt8) row_copy(src.qt8, i, ok, 16, dst.qt8, row);
    if (dst.msbt) row_copy(src.msbt, i, ok, 192, dst.msbt, row);
    if (dst.msdire) row_copy(src.msdire, i, ok, 192, dst.msdire, row);
}

constexpr unsigned ADAM_PER_GROUP = 2048;                 // floats of one tensor to a workgroup: 8 to a thread

__device__ inline void adam_one(float &p, float g, float &m, float &v, const AdamConsts &k)
{
    m = fmaf(k.d1, g - m, m);
    v = fmaf(k.d2 * g, g, k.b2 * v);
    p = p + (k.neg_af * m) / (sqrtf(v) / k.rf + k.ef);
}

// A workgroup finds its entry in the argument block (the same for all its threads: scalar loads) and walks 2048 floats of it, as
// 16-byte accesses where all four pointers allow them: torch's allocator hands out such tensors, a view may sit 4 bytes behind
__global__ __launch_bounds__(THREADS) void adam_step_kernel(AdamTable t, int nt, AdamConsts k)
{
    int lo = 0, hi = nt - 1;
    while (lo < hi) {                                     // the last entry whose first workgroup is not behind this one
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const unsigned base = (blockIdx.x - t.first[lo]) * ADAM_PER_GROUP;
    const unsigned left = min(t.count[lo] - base, ADAM_PER_GROUP);
    float *p = t.param[lo] + base, *m = t.m[lo] + base, *v = t.v[lo] + base;
    const float *g = t.grad[lo] + base;
    const bool wide = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                        reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const unsigned quads = wide ? left / 4 : 0;
    for (unsigned q = threadIdx.x; q < quads; q += THREADS) {
        float4 pp = reinterpret_cast<float4 *>(p)[q], mm = reinterpret_cast<float4 *>(m)[q], vv = reinterpret_cast<float4 *>(v)[q];
        const float4 gg = reinterpret_cast<const float4 *>(g)[q];
        adam_one(pp.x, gg.x, mm.x, vv.x, k);
        adam_one(pp.y, gg.y, mm.y, vv.y, k);
        adam_one(pp.z, gg.z, mm.z, vv.z, k);
        adam_one(pp.w, gg.w, mm.w, vv.w, k);
        reinterpret_cast<float4 *>(p)[q] = pp;
        reinterpret_cast<float4 *>(m)[q] = mm;
        reinterpret_cast<float4 *>(v)[q] = vv;
    }
    for (unsigned e = 4 * quads + threadIdx.x; e < left; e += THREADS) adam_one(p[e], g[e], m[e], v[e], k);
}

// Gradient buckets.  Both kernels are HBM-bound: 16-byte accesses on the bucket side, no LDS, no scratch, a table in the argument block.
// A workgroup finds its entry as Adam's does and writes 2048 floats of the entry's slice, the zero padding behind the tensor
// included: every float of the bucket belongs to exactly one workgroup.  A gradient that is 16-byte aligned is read as float4s
__global__ __launch_bounds__(THREADS) void grad_pack_kernel(GradPackTable t, int nt, float *bucket)
{
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const unsigned count = t.count[lo], base = (blockIdx.x - t.first[lo]) * ADAM_PER_GROUP;
    const unsigned quads = min(((count + 3) & ~3u) - base, ADAM_PER_GROUP) / 4;
    const float *g = t.grad[lo];
    float4 *o = reinterpret_cast<float4 *>(bucket + t.at[lo] + base);
    const bool wide = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    for (unsigned q = threadIdx.x; q < quads; q += THREADS) {
        const unsigned e = base + 4 * q;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g && wide && e + 4 <= count) f = *reinterpret_cast<const float4 *>(g + e);
        else if (g) {
            if (e < count) f.x = g[e];
            if (e + 1 < count) f.y = g[e + 1];
            if (e + 2 < count) f.z = g[e + 2];
            if (e + 3 < count) f.w = g[e + 3];
        }
        o[q] = f;
    }
}

// One float4 of every source to a thread, added in the table's order, one rounded addition each (-ffp-contract=off, no fast-math);
// a thread reads its float4 of src[0] before it writes the same float4 of dst: dst may be src[0]
__global__ __launch_bounds__(THREADS) void grad_sum_kernel(GradSumTable t, int nsrc, int64_t quads, float *dst)
{
    for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * THREADS) {
        float4 a = reinterpret_cast<const float4 *>(t.src[0])[q];
        for (int j = 1; j < nsrc; ++j) {
            const float4 b = reinterpret_cast<const float4 *>(t.src[j])[q];
            a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
        }
        reinterpret_cast<float4 *>(dst)[q] = a;
    }
}

}  // namespace

hipError_t launch_grad_pack(hipStream_t s, GradPackTable &t, int nt, float *bucket)
{
    unsigned groups = 0;
    for (int i = 0; i < nt; ++i) {
        t.first[i] = groups;
        groups += (t.count[i] + ADAM_PER_GROUP - 1) / ADAM_PER_GROUP;
    }
    hipLaunchKernelGGL(grad_pack_kernel, dim3(groups), dim3(THREADS), 0, s, t, nt, bucket);
    return hipGetLastError();
}

hipError_t launch_grad_sum(hipStream_t s, const GradSumTable &t, int nsrc, int64_t quads, float *dst)
{
    const unsigned groups = (unsigned)std::min<int64_t>((quads + THREADS - 1) / THREADS, 2048);
    hipLaunchKernelGGL(grad_sum_kernel, dim3(groups), dim3(THREADS), 0, s, t, nsrc, quads, dst);
    return hipGetLastError();
}

hipError_t launch_batch_gather(hipStream_t s, const pmp_batch_src &src, const int64_t *index, int n, const pmp_batch_dst &dst, int32_t *status)
{
    hipLaunchKernelGGL(batch_gather_kernel, dim3(n), dim3(THREADS), 0, s, src, index, dst, status);
    return hipGetLastError();
}

hipError_t launch_adam_step(hipStream_t s, AdamTable &t, int nt, const AdamConsts &k)
{
    unsigned groups = 0;
    for (int i = 0; i < nt; ++i) {
        t.first[i] = groups;
        groups += (t.count[i] + ADAM_PER_GROUP - 1) / ADAM_PER_GROUP;
    }
    hipLaunchKernelGGL(adam_step_kernel, dim3(groups), dim3(THREADS), 0, s, t, nt, k);
    return hipGetLastError();
}

}  // namespace pmp
