// train_step.hip — the two ends of a training step (include/pmp.h, TRAINING STEP): a batch gathered on the device from a data set that
// stays there as bytes, and Adam over every tensor of the step in one launch.  Both are latency-bound at a trainer's sizes (4 MB a
// batch, 43 MB an Adam step): what counts is one launch each and no host in the loop.  Built with -ffp-contract=off: every fused
// multiply-add below is written as fmaf().  And the gradient buckets of data-parallel training: the gradients of a rank packed into one
// buffer, and the ranks' buffers added in rank order, one rounded float32 addition at a time.  And the divergence guard: the global norm
// and non-finite census of a step's gradients in an order fixed by the shapes, and an Adam step that takes its orders from that record.
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

// the gradient a guarded step uses: one rounded multiply, none at coef 1
template <bool GUARDED>
__device__ inline float clipped(float g, float coef) { return GUARDED && coef != 1.0f ? g * coef : g; }

// A workgroup finds its entry in the argument block (the same for all its threads: scalar loads) and walks 2048 floats of it, as
// 16-byte accesses where all four pointers allow them: torch's allocator hands out such tensors, a view may sit 4 bytes behind.
// GUARDED (pmp_adam_step_guarded_device): coef and action come from the record in device memory; with the skip bit nothing is written
template <bool GUARDED>
__device__ inline void adam_walk(const AdamTable &t, int nt, const AdamConsts &k, const pmp_guard_record *rec)
{
    float coef = 1.0f;
    if (GUARDED) {
        if (rec->action & 1u) return;
        coef = rec->coef;
    }
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
        adam_one(pp.x, clipped<GUARDED>(gg.x, coef), mm.x, vv.x, k);
        adam_one(pp.y, clipped<GUARDED>(gg.y, coef), mm.y, vv.y, k);
        adam_one(pp.z, clipped<GUARDED>(gg.z, coef), mm.z, vv.z, k);
        adam_one(pp.w, clipped<GUARDED>(gg.w, coef), mm.w, vv.w, k);
        reinterpret_cast<float4 *>(p)[q] = pp;
        reinterpret_cast<float4 *>(m)[q] = mm;
        reinterpret_cast<float4 *>(v)[q] = vv;
    }
    for (unsigned e = 4 * quads + threadIdx.x; e < left; e += THREADS) adam_one(p[e], clipped<GUARDED>(g[e], coef), m[e], v[e], k);
}

__global__ __launch_bounds__(THREADS) void adam_step_kernel(AdamTable t, int nt, AdamConsts k) { adam_walk<false>(t, nt, k, nullptr); }

__global__ __launch_bounds__(THREADS) void adam_step_guarded_kernel(AdamTable t, int nt, AdamConsts k, const pmp_guard_record *rec)
{
    adam_walk<true>(t, nt, k, rec);
}

// grad_guard, first launch (include/pmp.h, THE ORDER OF THE CENSUS): one workgroup per tile of 4096 elements.  The tile goes through LDS,
// as 16-byte loads where the tensor's pointer allows them (a tile starts a multiple of 16 KB behind it), so that lane l then reads its
// own elements l, l + 256, ...; the tree runs in LDS, a barrier between its levels.  The count of non-finite elements rides along:
// integers, whose order does not matter
constexpr unsigned GUARD_TILE = 4096;

__device__ inline void guard_tree(double *a, unsigned long long *c, double &sum, unsigned long long &cnt)
{
    const unsigned l = threadIdx.x;
    a[l] = sum;
    c[l] = cnt;
    __syncthreads();
    for (unsigned h = THREADS / 2; h >= 1; h >>= 1) {
        if (l < h) { a[l] = a[l] + a[l + h]; c[l] += c[l + h]; }
        __syncthreads();
    }
    sum = a[0];
    cnt = c[0];
}

__global__ __launch_bounds__(THREADS) void grad_census_kernel(GuardTable t, int nt, int64_t tile0, double *part, unsigned long long *bad)
{
    __shared__ float tile[GUARD_TILE];
    __shared__ double a[THREADS];
    __shared__ unsigned long long c[THREADS];
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const unsigned base = (blockIdx.x - t.first[lo]) * GUARD_TILE;
    const unsigned left = min(t.count[lo] - base, GUARD_TILE);
    const float *g = t.grad[lo] + base;
    const unsigned quads = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? left / 4 : 0;
    for (unsigned q = threadIdx.x; q < quads; q += THREADS) reinterpret_cast<float4 *>(tile)[q] = reinterpret_cast<const float4 *>(g)[q];
    for (unsigned e = 4 * quads + threadIdx.x; e < left; e += THREADS) tile[e] = g[e];
    __syncthreads();
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (unsigned e = threadIdx.x; e < left; e += THREADS) {
        const float f = tile[e];
        const bool finite = (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u;
        const double d = (double)f;
        if (finite) sum = sum + d * d;                    // -ffp-contract=off: the square, exact in double, then one rounded addition
        else ++cnt;
    }
    guard_tree(a, c, sum, cnt);
    if (threadIdx.x == 0) {
        part[tile0 + blockIdx.x] = sum;
        bad[tile0 + blockIdx.x] = cnt;
    }
}

// grad_guard, second launch: one workgroup adds the tiles' partials in the same fixed order, and lane 0 finishes the record in double
// and steps the running counters
__global__ __launch_bounds__(THREADS) void grad_guard_finish_kernel(const double *part, const unsigned long long *bad, int64_t tiles, double max_norm,
                                                                    int skip_nonfinite, pmp_guard_record *rec, pmp_guard_state *st)
{
    __shared__ double a[THREADS];
    __shared__ unsigned long long c[THREADS];
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (int64_t i = threadIdx.x; i < tiles; i += THREADS) { sum = sum + part[i]; cnt += bad[i]; }
    guard_tree(a, c, sum, cnt);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sum), cc = max_norm / (norm + 1e-6);
    const float coef = max_norm > 0.0 && cc < 1.0 ? (float)cc : 1.0f;
    const bool skip = skip_nonfinite && cnt > 0, clip = coef < 1.0f;
    rec->sumsq = sum;
    rec->norm = norm;
    rec->nonfinite = (int64_t)cnt;
    rec->coef = coef;
    rec->action = (skip ? 1u : 0u) | (clip ? 2u : 0u);
    if (!st) return;
    pmp_guard_state s = *st;
    s.steps += 1;
    if (skip) {
        s.skipped += 1;
        s.run += 1;
        s.max_run = s.run > s.max_run ? s.run : s.max_run;
    } else {
        s.run = 0;
        if (clip) s.clipped += 1;
    }
    s.max_norm = norm > s.max_norm ? norm : s.max_norm;
    *st = s;
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

hipError_t launch_adam_step(hipStream_t s, AdamTable &t, int nt, const AdamConsts &k, const pmp_guard_record *rec)
{
    unsigned groups = 0;
    for (int i = 0; i < nt; ++i) {
        t.first[i] = groups;
        groups += (t.count[i] + ADAM_PER_GROUP - 1) / ADAM_PER_GROUP;
    }
    if (rec) hipLaunchKernelGGL(adam_step_guarded_kernel, dim3(groups), dim3(THREADS), 0, s, t, nt, k, rec);
    else hipLaunchKernelGGL(adam_step_kernel, dim3(groups), dim3(THREADS), 0, s, t, nt, k);
    return hipGetLastError();
}

hipError_t launch_grad_census(hipStream_t s, GuardTable &t, int nt, int64_t tile0, void *scratch, int64_t tiles_all)
{
    unsigned groups = 0;
    for (int i = 0; i < nt; ++i) {
        t.first[i] = groups;
        groups += (t.count[i] + GUARD_TILE - 1) / GUARD_TILE;
    }
    hipLaunchKernelGGL(grad_census_kernel, dim3(groups), dim3(THREADS), 0, s, t, nt, tile0, (double *)scratch,
                       (unsigned long long *)scratch + tiles_all);
    return hipGetLastError();
}

hipError_t launch_grad_guard_finish(hipStream_t s, const void *scratch, int64_t tiles, const pmp_guard_params &p, pmp_guard_record *rec,
                                    pmp_guard_state *st)
{
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(THREADS), 0, s, (const double *)scratch, (const unsigned long long *)scratch + tiles,
                       tiles, p.max_norm, p.skip_nonfinite, rec, st);
    return hipGetLastError();
}

}  // namespace pmp
