// postproc.hip — Map2Partition on the GPU: four wavefronts per 64x64 block, one per QT quadrant.
//
// Replaces, bit-exactly:
//   eli_structual_error / check_square_unity   Metrics.py:612-637
//   Map_to_Partition                           Map2Partition.py:98-373
//   output_block_yuv (block cutter)            Inference_QBD.py:104-149
//
// The reference's candidate-tree search (Map2Partition.py:203-266) is a depth-3 DFS whose control flow is identical for all
// lanes.  Its frame - cells on lanes, the quadtree walk, split modes, combinations, child CU lists - is m2p_tree.h's, shared with
// the label kernels (labels.hip); here are Map2Partition's rules (can_split: the call's thresholds on the rounded logits of each
// level), its direction map, its leaf cost, the edge planes in LDS, and the three tree levels unrolled at compile time (template
// recursion), so every level's maps are registers.
// The float32 L1 error (:307-312) must reproduce numpy's pairwise summation order bit for bit: cell values are
// scattered to LDS in region-flattened order and 8 (or 2x8) lanes run the interleaved accumulators exactly as
// numpy's FLOAT_pairwise_sum does; the combine tree is done with xor-shuffles (fp add is commutative, so the
// tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) is reproduced exactly).  This file is compiled with
// -ffp-contract=off so `s + 0.8f*d` is not fused.
#include "m2p_tree.h"
#include "pmp_kernels.h"

namespace pmp {

using namespace tree;

namespace {

struct Search {
    // per-lane constants of this block
    int row, col0;
    int mb[3][4];     // np.round(bt) (Map2Partition.py:104) as an integer saturated to +-100; NaN -> +100.  The reference keeps the float and
                      // has no clamp, but the rounded map is only ever compared (`== 0`, `< 0` of msbt - candidate, candidate depths 0..6,
                      // :142,189-190): a value beyond 100 - or NaN, on which both comparisons are False - behaves like 100, one below
                      // -100 like -100.  Pinned by tests/golden/g3b_m2p_range.npz (|bt| up to 3e38, +-inf, NaN; made by the reference)
    int md[3][4];     // th_round(dire, thd) (Map2Partition.py:30-35,105; thd = 0.5 there)
    float ob[3][4];   // raw MTT depth logits
    float od[3][4];   // raw direction logits
    int cf;           // chroma_factor
    double lamb[5];   // Map_to_Partition's lamb1..lamb5 of this call (kernel argument; uniform)
    // tree levels 0..3 (Map_Node, Map2Partition.py:89-96)
    int bt[4][4], dr[4][4];
    int cu[4];        // lane c holds CU c of the level: x | y<<4 | (h-1)<<8 | (w-1)<<12
    int ncu[4];       // uniform
    float sb[4], sd[4];
    // QT-leaf region and best leaf so far
    int rx, ry, rh, rw;
    float best_err;
    int have_best;
    int best_dr[3][4];
    int best_cu, best_ncu;
    float *valb, *vald;  // LDS scratch, 256 floats each
};

// np.sum(np.abs(map - ori)) over the region for the depth map (lanes 0..15) and the direction map (16..31).
__device__ __forceinline__ void region_sums(Search &s, const int (&btm)[4], const int (&drm)[4], const float (&ob)[4],
                                            const float (&od)[4], float &out_b, float &out_d)
{
    const int lane = threadIdx.x & 63;
    const int n = s.rh * s.rw;
    // wave-local ordering only (the scratch is private to the wave and the four waves of a block search different quadrants,
    // so a workgroup barrier here would not even be reached the same number of times)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = s.row - s.rx, c = s.col0 + k - s.ry;
        if (r >= 0 && r < s.rh && c >= 0 && c < s.rw) {
            const int f = r * s.rw + c;
            s.valb[f] = fabsf((float)btm[k] - ob[k]);
            s.vald[f] = fabsf((float)drm[k] - od[k]);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const float *v = (lane & 16) ? s.vald : s.valb;
    const int j = lane & 15, half = j >> 3, k = j & 7;
    float r = 0.f;
    if (n >= 8) {
        const int per = n > 128 ? 128 : n;          // numpy PW_BLOCKSIZE = 128; n = 256 splits into 128 + 128
        const float *p = v + half * 128 + k;
        if (half == 0 || n > 128) {
            r = p[0];
            for (int i = 8; i < per; i += 8) r = r + p[i];
        }
        r = r + __shfl_xor(r, 1);
        r = r + __shfl_xor(r, 2);
        r = r + __shfl_xor(r, 4);
        if (n > 128) r = r + __shfl_xor(r, 8);
    } else {                                         // n < 8: sequential from 0.
        for (int i = 0; i < n; ++i) r = r + v[i];
    }
    out_b = rlanef(r, 0);
    out_d = rlanef(r, 16);
}

// can_split_mode_list (Map2Partition.py:140-201): returns modes packed 3 bits each (first entry 0), count in `n`.
template <int L>
__device__ __forceinline__ int can_split(const Search &s, int cu, int &n)
{
    const CU u = unpack_cu(cu);
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = s.row >= u.x && s.row < u.x + u.h && s.col0 + k >= u.y && s.col0 + k < u.y + u.w;
    // lamb1..lamb5 as Python compares them (Map2Partition.py:144,150-153,194): an int count against a double product, left to right
    const double l1 = s.lamb[0], l2 = s.lamb[1], l3 = s.lamb[2], l4 = s.lamb[3], l5 = s.lamb[4];
    int zero = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) zero += cnt(in[k] && s.mb[2][k] == s.bt[L][k]);
    n = 1;
    if ((double)zero >= l1 * u.h * u.w) return 0;  // lamb1
    int hor = 0, ver = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hor += cnt(in[k] && s.md[L][k] == 1);
        ver += cnt(in[k] && s.md[L][k] == -1);
    }
    int direction = 0;
    if ((double)(ver + hor) >= l2 * u.h * u.w) {  // lamb2, lamb3
        if ((double)hor >= l3 * ver) direction = 1;
        else if ((double)ver >= l3 * hor) direction = 2;
    }
    return split_modes(u.h, u.w, s.cf, direction, 0, n, [&](bool horiz, int o0, int o1, int inc, int np_) {
        int minus = 0, zer = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = horiz ? (s.row - u.x) : (s.col0 + k - u.y);
            const bool ins = in[k] && t >= o0 && t < o1;
            const int tgt = s.bt[L][k] + inc;
            minus += cnt(ins && s.mb[L][k] < tgt);
            zer += cnt(ins && s.mb[L][k] == tgt);
        }
        return (double)minus < np_ * l4 && (double)zer > np_ * l5;  // lamb4, lamb5
    });
}

// get_candidate_map_tree (Map2Partition.py:203-266) for a node at level L; leaves (level 3) are scored in DFS
// order with a strict '<' so the FIRST minimum wins, as list.index(min(list)) does (:315).
template <int L>
__device__ __forceinline__ void expand(Search &s)
{
    const int lane = threadIdx.x & 63;
    const int ncu = s.ncu[L];
    int my_list = 0, my_n = 1;
    for (int c = 0; c < ncu; ++c) {
        int n;
        const int list = can_split<L>(s, rlane(s.cu[L], c), n);
        if (lane == c) { my_list = list; my_n = n; }
    }
    const auto [my_p, total] = combos(my_n, ncu);   // Search, Map2Partition.py:53-87
    for (int t = 0; t < total; ++t) {
        int nb[4], nd[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { nb[k] = s.bt[L][k]; nd[k] = 0; }  // child dire map starts from zeros (:240)
        s.ncu[L + 1] = apply_combination(s.row, s.col0, s.cu[L], ncu, mode_in(my_list, my_n, my_p, t), nb, s.cu[L + 1],
                                         [&](int k, bool horiz) { nd[k] = horiz ? 1 : -1; });
#pragma unroll
        for (int k = 0; k < 4; ++k) { s.bt[L + 1][k] = nb[k]; s.dr[L + 1][k] = nd[k]; }
        region_sums(s, nb, nd, s.ob[L], s.od[L], s.sb[L + 1], s.sd[L + 1]);
        if constexpr (L == 2) {
            // error of the leaf and its two ancestors, float32 left to right (Map2Partition.py:307-312)
            const float eb = (s.sb[1] + s.sb[2]) + s.sb[3];
            const float ed = (s.sd[1] + s.sd[2]) + s.sd[3];
            const float err = eb + 0.8f * ed;
            if (!s.have_best || err < s.best_err) {
                s.have_best = 1;
                s.best_err = err;
#pragma unroll
                for (int k = 0; k < 4; ++k) { s.best_dr[0][k] = s.dr[1][k]; s.best_dr[1][k] = s.dr[2][k]; s.best_dr[2][k] = s.dr[3][k]; }
                s.best_cu = s.cu[3];
                s.best_ncu = s.ncu[3];
            }
        } else {
            expand<L + 1>(s);
        }
    }
}

}  // namespace

// One wave per block.  LDS per workgroup: 2 x 256 floats (sum scratch) + 2 x 256 bytes (edge planes).
// Four waves per block: the QT leaves under the four 32x32 quadrants are independent searches writing disjoint cells, so wave
// w takes the nodes of quadrant w (a block that is one 64x64 leaf is searched by wave 0 alone).  Every wave keeps the whole
// block's maps - the search code is the single-wave one - and has its own pairwise-sum scratch.
// DEF: the reference's default thresholds as compile-time constants - the code the kernel had before the thresholds became arguments
// (runtime doubles cost this already spilling kernel 7 more SGPRs and 11 more VGPRs of spill); !DEF: the call's own `prm`.
template <bool DEF>
__global__ __launch_bounds__(256, 4) void postprocess_kernel(const float *__restrict__ qt, const float *__restrict__ bt,
                                                          const float *__restrict__ dire, int64_t N, int cf, M2PParams prm,
                                                          uint8_t *__restrict__ hor_o, uint8_t *__restrict__ ver_o,
                                                          uint8_t *__restrict__ qt_o, int8_t *__restrict__ dire_o,
                                                          int s_edge, int s_qt, int s_dire)   // bytes between consecutive blocks
{
    __shared__ float valb_all[4][256], vald_all[4][256];
    __shared__ uint32_t horw[64], verw[64];
    uint8_t *hor = reinterpret_cast<uint8_t *>(horw), *ver = reinterpret_cast<uint8_t *>(verw);
    const int64_t b = blockIdx.x;
    if (b >= N) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *valb = valb_all[wv], *vald = vald_all[wv];

    // ---- eli_structual_error (Metrics.py:630-637): lanes 0..15 own the 4x4 pooled map
    float pv = 0.f;
    {
        const int i = lane & 15, pr = i >> 2, pc = i & 3;
        const float *q = qt + b * 64 + (2 * pr) * 8 + 2 * pc;
        pv = q[0];                                        // F.max_pool2d propagates NaN (v_max_f32 would drop it)
        if (q[1] > pv || q[1] != q[1]) pv = q[1];
        if (q[8] > pv || q[8] != q[8]) pv = q[8];
        if (q[9] > pv || q[9] != q[9]) pv = q[9];
        pv = rintf(pv);                                   // torch.round: half to even
        pv = pv < 0.f ? 0.f : (pv > 3.f ? 3.f : pv);      // clamp(0, 3); -0.0 compares equal to 0; NaN stays NaN (torch.clamp)
    }
    // a NaN depth travels as -1: every comparison the reference makes on it (== 0, == 1, == depth, > depth) is False, and so is
    // every comparison below; its quadrant's sum is NaN (Metrics.py:618-619: no rule applies); it is emitted as 0 (.astype(np.uint8))
    int m = pv != pv ? -1 : (int)pv;
    {
        const unsigned long long z = __ballot(m == 0) & 0xFFFFull;
        const int num0 = __popcll(z);
        if (num0 <= 12) {                                 // check_square_unity (Metrics.py:612-628)
            if (m == 0) m = 1;
            int sum = m + __shfl_xor(m, 1);
            sum += __shfl_xor(sum, 4);
            int one = (m == 1) ? 1 : 0;
            int n1 = one + __shfl_xor(one, 1);
            n1 += __shfl_xor(n1, 4);
            int nnan = (m < 0) ? 1 : 0;
            nnan += __shfl_xor(nnan, 1);
            nnan += __shfl_xor(nnan, 4);
            if (nnan == 0 && sum >= 5 && sum <= 10) {
                if (n1 < 3) { if (m == 1) m = 2; }
                else m = 1;
            }
        } else if (num0 < 16) {
            m = 0;
        }
    }
    // nearest x2 (Metrics.py:635): lane l holds the 8x8 value at (l>>3, l&7)
    const int qt8 = rlane(m, 0) * 0 + __shfl(m, ((lane >> 4) << 2) + ((lane & 7) >> 1));
    if (wv == 0) qt_o[b * s_qt + lane] = (uint8_t)(qt8 < 0 ? 0 : qt8);

    // ---- Map_to_Partition.__init__ (Map2Partition.py:100-122)
    Search s;
    s.row = lane >> 2;
    s.col0 = (lane & 3) << 2;
    s.cf = cf;
#pragma unroll
    for (int i = 0; i < 5; ++i) s.lamb[i] = DEF ? M2P_DEFAULT.lamb[i] : prm.lamb[i];
    // th_round(dire, thd) (Map2Partition.py:30-35) on float32: numpy compares against float32(thd).  Its third np.where zeroes what lies in
    // (-thd, thd) AFTER the first two have written +-1, so for thd > 1 every direction ends up 0 (NaN never compares: 0 here, as before)
    const float thd = DEF ? M2P_DEFAULT.thd : prm.thd;
    const bool thd_keeps = !(1.f < thd);
    s.valb = valb;
    s.vald = vald;
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {
        const float4 vb = *reinterpret_cast<const float4 *>(bt + (b * 3 + k3) * 256 + lane * 4);
        const float4 vd = *reinterpret_cast<const float4 *>(dire + (b * 3 + k3) * 256 + lane * 4);
        const float fb[4] = {vb.x, vb.y, vb.z, vb.w}, fd[4] = {vd.x, vd.y, vd.z, vd.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s.ob[k3][k] = fb[k];
            s.od[k3][k] = fd[k];
            float r = rintf(fb[k]);                       // np.round: half to even
            r = !(r <= 100.f) ? 100.f : (r < -100.f ? -100.f : r);   // see Search::mb; NaN -> 100
            s.mb[k3][k] = (int)r;
            s.md[k3][k] = !thd_keeps ? 0 : (fd[k] >= thd ? 1 : (fd[k] <= -thd ? -1 : 0));
        }
    }
    if (wv == 0) { horw[lane] = 0; verw[lane] = 0; }
    int outd[3][4];
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
        for (int k = 0; k < 4; ++k) outd[k3][k] = 0;
    __syncthreads();

    // ---- set_partition_vector (Map2Partition.py:348-362), flattened: a node is reached iff every ancestor split
    walk_quadrant(qt8, wv, [&](int d, int qx, int qy, int sms, int c) {
        if (c > d) {
            if (d < 3 && lane < 2 * sms) {                // paint the QT cross
                hor[(2 * qx + sms) * 16 + 2 * qy + lane] = 1;
                ver[(2 * qx + lane) * 16 + 2 * qy + sms] = 1;
            }
            return;
        }
        if (c < d) return;                                // hole: no MTT edges, dire stays 0
        // ---- set_bt_partition_vector (Map2Partition.py:287-346) on [2qx, 2qy, 2sms, 2sms]
        set_region(s, qx, qy, sms);
#pragma unroll
        for (int k = 0; k < 4; ++k) s.dr[0][k] = 0;
        s.have_best = 0;
        s.best_err = 0.f;
        s.best_ncu = 0;
        s.best_cu = 0;
        expand<0>(s);
        copy_region(s, outd, s.best_dr);
        const int j = lane & 15, part = lane >> 4;
        for (int ci = 0; ci < s.best_ncu; ++ci) {
            const CU u = unpack_cu(rlane(s.best_cu, ci));
            // par_vec is 17x17 in the reference; row/column 16 is cropped away (Map2Partition.py:373)
            if (part == 0 && j < u.w) hor[u.x * 16 + u.y + j] = 1;
            if (part == 1 && j < u.w && u.x + u.h < 16) hor[(u.x + u.h) * 16 + u.y + j] = 1;
            if (part == 2 && j < u.h) ver[(u.x + j) * 16 + u.y] = 1;
            if (part == 3 && j < u.h && u.y + u.w < 16) ver[(u.x + j) * 16 + u.y + u.w] = 1;
        }
    });
    __syncthreads();
    if (wv == 0) {
        reinterpret_cast<uint32_t *>(hor_o + b * s_edge)[lane] = horw[lane];
        reinterpret_cast<uint32_t *>(ver_o + b * s_edge)[lane] = verw[lane];
    }
    store_planes(dire_o + b * s_dire, outd, qt8, wv);
}

hipError_t launch_postprocess(hipStream_t st, const float *qt, const float *bt, const float *dire, int64_t N,
                              int chroma_factor, const M2PParams &prm, uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8,
                              int record_stride)
{
    if (N <= 0) return hipSuccess;
    // four dense arrays (strides 256 / 256 / 64 / 768 bytes per block), or one packed record per block (include/pmp.h)
    const int se = record_stride ? record_stride : 256, sq = record_stride ? record_stride : 64, sd = record_stride ? record_stride : 768;
    if (m2p_is_default(prm))
        hipLaunchKernelGGL(postprocess_kernel<true>, dim3((unsigned)N), dim3(256), 0, st, qt, bt, dire, N, chroma_factor, prm, hor, ver,
                           qt_u8, dire_i8, se, sq, sd);
    else
        hipLaunchKernelGGL(postprocess_kernel<false>, dim3((unsigned)N), dim3(256), 0, st, qt, bt, dire, N, chroma_factor, prm, hor, ver,
                           qt_u8, dire_i8, se, sq, sd);
    return hipGetLastError();
}

// =============================================================================================== block cutter
// output_block_yuv (Inference_QBD.py:104-149): zero-pad top/left by the overlap, slice (bs+ov)^2 windows.
// 10-bit input: np.round(x / 4) in float64 = round half to even, then clip to 255 (:106-109) - done in integers.
template <typename T>
__global__ __launch_bounds__(256) void cut_plane_kernel(const T *__restrict__ plane, int F, int H, int W, int bs, int ov,
                                                        int bh, int bw, int tenbit, uint8_t *__restrict__ out)
{
    const int S = bs + ov;
    const size_t total = (size_t)F * bh * bw * S * S;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % S);
        size_t r = i / S;
        const int rr = (int)(r % S); r /= S;
        const int j = (int)(r % bw); r /= bw;
        const int bi = (int)(r % bh);
        const int f = (int)(r / bh);
        const int yy = bi * bs + rr - ov, xx = j * bs + c - ov;
        unsigned v = 0;
        if (yy >= 0 && xx >= 0) {
            v = plane[((size_t)f * H + yy) * W + xx];
            if (tenbit) {
                const unsigned qv = v >> 2, rem = v & 3;
                v = qv + (rem == 3 ? 1u : (rem == 2 ? (qv & 1u) : 0u));
                v = v > 255u ? 255u : v;
            }
        }
        out[i] = (uint8_t)v;
    }
}

hipError_t launch_cut_blocks(hipStream_t st, const void *y, const void *u, const void *v, int F, int H, int W,
                             int bitdepth, uint8_t *by, uint8_t *bu, uint8_t *bv)
{
    const int bh = H / 64, bw = W / 64;
    if (F <= 0 || bh <= 0 || bw <= 0) return hipSuccess;
    const size_t ny = (size_t)F * bh * bw * 68 * 68, nc = (size_t)F * bh * bw * 34 * 34;
    const unsigned gy = (unsigned)((ny + 255) / 256 > 8192 ? 8192 : (ny + 255) / 256);
    const unsigned gc = (unsigned)((nc + 255) / 256 > 8192 ? 8192 : (nc + 255) / 256);
    if (bitdepth == 8) {
        hipLaunchKernelGGL(cut_plane_kernel<uint8_t>, dim3(gy), dim3(256), 0, st, (const uint8_t *)y, F, H, W, 64, 4, bh, bw, 0, by);
        hipLaunchKernelGGL(cut_plane_kernel<uint8_t>, dim3(gc), dim3(256), 0, st, (const uint8_t *)u, F, H / 2, W / 2, 32, 2, bh, bw, 0, bu);
        hipLaunchKernelGGL(cut_plane_kernel<uint8_t>, dim3(gc), dim3(256), 0, st, (const uint8_t *)v, F, H / 2, W / 2, 32, 2, bh, bw, 0, bv);
    } else {
        hipLaunchKernelGGL(cut_plane_kernel<uint16_t>, dim3(gy), dim3(256), 0, st, (const uint16_t *)y, F, H, W, 64, 4, bh, bw, 1, by);
        hipLaunchKernelGGL(cut_plane_kernel<uint16_t>, dim3(gc), dim3(256), 0, st, (const uint16_t *)u, F, H / 2, W / 2, 32, 2, bh, bw, 1, bu);
        hipLaunchKernelGGL(cut_plane_kernel<uint16_t>, dim3(gc), dim3(256), 0, st, (const uint16_t *)v, F, H / 2, W / 2, 32, 2, bh, bw, 1, bv);
    }
    return hipGetLastError();
}

}  // namespace pmp
