// dataset.hip — data set assembly (include/pmp.h, DATA SET ASSEMBLY): one index of the rows a set keeps, and any array of the set
// gathered by it.  pmp_select_rows_device is a prefix sum of fixed shape in five small launches - candidates per tile of 1024 rows, a
// scan of the tile counts and a running maximum of the segment ends by ONE workgroup, the candidates in front of every segment end,
// a scan of the segments' kept counts by one workgroup, the scatter - and no workgroup ever waits for another: what a launch reads of
// another workgroup's was written by an earlier launch.  No atomics: every word of every output has exactly one writer.
#include "pmp_kernels.h"

namespace pmp {
namespace {

constexpr int THREADS = 256;
constexpr int TILE = SELECT_TILE;                         // rows of a workgroup: TILE / THREADS rounds of one row to a thread

// 1 where row i is a candidate: no flag array has a bit of mask set in it
__device__ inline uint32_t candidate(const SelectFlags &f, int nflags, uint32_t mask, int64_t i)
{
    uint32_t bad = 0;
    for (int k = 0; k < nflags; ++k) bad |= f.p[k][i] & mask;
    return bad ? 0u : 1u;
}

// Inclusive scan over the workgroup's THREADS values, sums or maxima, in eight fixed steps; lds: THREADS words, free on return
__device__ inline uint32_t block_scan(uint32_t v, uint32_t *lds, bool maxima)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const uint32_t a = t >= d ? lds[t - d] : 0u;
        __syncthreads();
        lds[t] = maxima ? max(lds[t], a) : lds[t] + a;
        __syncthreads();
    }
    const uint32_t r = lds[t];
    __syncthreads();
    return r;
}

// tile g -> part[g] = its candidates
__global__ __launch_bounds__(THREADS) void select_count_kernel(SelectFlags f, int nflags, uint32_t mask, int64_t n, uint32_t *part)
{
    __shared__ uint32_t lds[THREADS];
    const int64_t base = (int64_t)blockIdx.x * TILE;
    uint32_t mine = 0;
    for (int r = 0; r < TILE / THREADS; ++r) {
        const int64_t i = base + r * THREADS + threadIdx.x;
        if (i < n) mine += candidate(f, nflags, mask, i);
    }
    const uint32_t sum = block_scan(mine, lds, false);
    if (threadIdx.x == THREADS - 1) part[blockIdx.x] = sum;
}

// One workgroup.  count words at v, in place: sums -> the exclusive prefix sums and v[count] = the total; maxima -> the inclusive
// running maxima.  In chunks of THREADS with a carry.
__device__ inline void scan_words(uint32_t *v, int64_t count, bool maxima, uint32_t *lds)
{
    uint32_t carry = 0;
    for (int64_t at = 0; at < count; at += THREADS) {
        const int64_t i = at + threadIdx.x;
        const uint32_t x = i < count ? v[i] : 0u;
        const uint32_t incl = block_scan(x, lds, maxima);
        if (i < count) v[i] = maxima ? max(carry, incl) : carry + incl - x;
        lds[threadIdx.x] = incl;                          // block_scan's last barrier lies behind every read of lds
        __syncthreads();
        carry = maxima ? max(carry, lds[THREADS - 1]) : carry + lds[THREADS - 1];
        __syncthreads();
    }
    if (!maxima && threadIdx.x == 0) v[count] = carry;
}

// One workgroup: part[0 .. tiles] becomes the candidates in front of every tile (and their total); seg_e[s] = the end of segment s
// made safe: clamped into 0 .. n, never below an earlier end, and n for the last segment
__global__ __launch_bounds__(THREADS) void select_scan_kernel(uint32_t *part, int64_t tiles, const int64_t *seg_end, int nseg, int64_t n, uint32_t *seg_e)
{
    __shared__ uint32_t lds[THREADS];
    scan_words(part, tiles, false, lds);
    for (int s = threadIdx.x; s < nseg; s += THREADS) {
        const int64_t e = seg_end[s];
        seg_e[s] = s == nseg - 1 ? (uint32_t)n : (uint32_t)(e < 0 ? 0 : e > n ? n : e);
    }
    __syncthreads();
    scan_words(seg_e, nseg, true, lds);
}

// Workgroup s: seg_c[s] = the candidates in front of row seg_e[s] = those in front of its tile and those of the tile's rows before it
__global__ __launch_bounds__(THREADS) void select_segment_kernel(SelectFlags f, int nflags, uint32_t mask, const uint32_t *part, const uint32_t *seg_e,
                                                                 uint32_t *seg_c)
{
    __shared__ uint32_t lds[THREADS];
    const int64_t e = seg_e[blockIdx.x], tile = e / TILE, base = tile * TILE;
    uint32_t mine = 0;
    for (int r = 0; r < TILE / THREADS; ++r) {
        const int64_t i = base + r * THREADS + threadIdx.x;
        if (i < e) mine += candidate(f, nflags, mask, i);
    }
    const uint32_t sum = block_scan(mine, lds, false);
    if (threadIdx.x == THREADS - 1) seg_c[blockIdx.x] = part[tile] + sum;      // part[tiles] exists: e = n may be the end of the last tile
}

// One workgroup: count[s] = the rows segment s keeps, count[nseg] = their total m; seg_base[s] = the kept rows of the segments before
// s and seg_base[nseg] = m
__global__ __launch_bounds__(THREADS) void select_kept_kernel(const uint32_t *seg_c, int nseg, int64_t cap, uint32_t *seg_base, int64_t *count)
{
    __shared__ uint32_t lds[THREADS];
    for (int s = threadIdx.x; s < nseg; s += THREADS) {
        const uint32_t cand = seg_c[s] - (s ? seg_c[s - 1] : 0u);
        const uint32_t kept = cap && (int64_t)cand > cap ? (uint32_t)cap : cand;
        seg_base[s] = kept;
        count[s] = kept;
    }
    __syncthreads();
    scan_words(seg_base, nseg, false, lds);
    __syncthreads();
    if (threadIdx.x == 0) count[nseg] = seg_base[nseg];
}

// Tile g: every row finds its rank among the candidates (the tile's offset, the rounds before it, the threads before it), its segment
// (the first whose end lies behind the row) and, if the segment keeps it, its place in index.  Row i also writes the -1 of index[i]
// where i >= m: together every word of index, each once.
__global__ __launch_bounds__(THREADS) void select_scatter_kernel(SelectFlags f, int nflags, uint32_t mask, int64_t n, int64_t cap, const uint32_t *part,
                                                                 const uint32_t *seg_e, const uint32_t *seg_c, const uint32_t *seg_base, int nseg,
                                                                 int64_t *index)
{
    __shared__ uint32_t lds[THREADS];
    const int64_t base = (int64_t)blockIdx.x * TILE;
    const uint32_t m = seg_base[nseg];
    uint32_t carry = part[blockIdx.x];
    for (int r = 0; r < TILE / THREADS; ++r) {
        const int64_t i = base + r * THREADS + threadIdx.x;
        const uint32_t c = i < n ? candidate(f, nflags, mask, i) : 0u;
        const uint32_t incl = block_scan(c, lds, false);
        if (i < n) {
            if (i >= m) index[i] = -1;
            if (c) {
                int lo = 0, hi = nseg - 1;                // seg_e ascends and seg_e[nseg - 1] = n > i
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (seg_e[mid] > i) hi = mid;
                    else lo = mid + 1;
                }
                const uint32_t rank = carry + incl - 1 - (lo ? seg_c[lo - 1] : 0u);   // candidates of the segment before this one
                if (!cap || (int64_t)rank < cap) index[seg_base[lo] + rank] = i;
            }
        }
        lds[threadIdx.x] = incl;
        __syncthreads();
        carry += lds[THREADS - 1];
        __syncthreads();
    }
}

// Rows of `units` words of type T; 2^lanes_log2 threads to a row, THREADS >> lanes_log2 rows to a workgroup
template <typename T>
__global__ __launch_bounds__(THREADS) void gather_rows_kernel(const T *src, int64_t nsrc, int units, const int64_t *index, int64_t m, T *dst, int lanes_log2,
                                                              int32_t *status)
{
    const int lanes = 1 << lanes_log2, lane = threadIdx.x & (lanes - 1);
    const int64_t row = (int64_t)blockIdx.x * (THREADS >> lanes_log2) + (threadIdx.x >> lanes_log2);
    if (row >= m) return;
    const int64_t at = index[row];
    const bool ok = at >= 0 && at < nsrc;
    if (!ok && lane == 0) atomicOr(status, 1);
    const T *s = src + (ok ? at : 0) * units;             // never a pointer outside the source, dereferenced or not
    T *o = dst + row * units;
    for (int u = lane; u < units; u += lanes) o[u] = ok ? s[u] : T{};
}

}  // namespace

size_t select_scratch_words(int64_t n, int nseg) { return (size_t)((n + TILE - 1) / TILE + 1) + 3 * (size_t)nseg + 1; }

hipError_t launch_select_rows(hipStream_t s, const SelectFlags &f, int nflags, int mask, const int64_t *seg_end, int nseg, int64_t cap, int64_t n,
                              uint32_t *scratch, int64_t *index, int64_t *count)
{
    const int64_t tiles = (n + TILE - 1) / TILE;
    uint32_t *part = scratch, *seg_e = part + tiles + 1, *seg_c = seg_e + nseg, *seg_base = seg_c + nseg;     // tiles + 1, nseg, nseg, nseg + 1 words
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, s, f, nflags, (uint32_t)mask, n, part);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(THREADS), 0, s, part, tiles, seg_end, nseg, n, seg_e);
    hipLaunchKernelGGL(select_segment_kernel, dim3(nseg), dim3(THREADS), 0, s, f, nflags, (uint32_t)mask, part, seg_e, seg_c);
    hipLaunchKernelGGL(select_kept_kernel, dim3(1), dim3(THREADS), 0, s, seg_c, nseg, cap, seg_base, count);
    hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, s, f, nflags, (uint32_t)mask, n, cap, part, seg_e, seg_c, seg_base,
                       nseg, index);
    return hipGetLastError();
}

hipError_t launch_gather_rows(hipStream_t s, const void *src, int64_t nsrc, int64_t row_bytes, const int64_t *index, int64_t m, void *dst, int32_t *status)
{
    // 16-byte accesses where the call allows them: then every row of both arrays starts on a 16-byte boundary
    const bool wide = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)row_bytes) & 15) == 0;
    const int units = (int)(row_bytes / (wide ? 16 : 4));
    int lanes_log2 = 0;
    while (lanes_log2 < 8 && (1 << lanes_log2) < units) ++lanes_log2;
    const int64_t rows = THREADS >> lanes_log2, groups = (m + rows - 1) / rows;
    if (wide)
        hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3((unsigned)groups), dim3(THREADS), 0, s, (const uint4 *)src, nsrc, units, index, m, (uint4 *)dst,
                           lanes_log2, status);
    else
        hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, dim3((unsigned)groups), dim3(THREADS), 0, s, (const uint32_t *)src, nsrc, units, index, m,
                           (uint32_t *)dst, lanes_log2, status);
    return hipGetLastError();
}

}  // namespace pmp
