// labels.hip — GenMSBtMap on the GPU: the per-layer MTT depth labels (MSBT) of the training set, one workgroup per 64x64 block.
//
// Replaces, bit-exactly wherever the reference finishes:
//   Map_to_SubMap(qt, bt, dire, cf).get_sub_map()   GenMSBtMap.py:89-368  (called per block by gen_seq_sub_map, :434-449)
//
// The search's frame - cells on lanes, the quadtree walk, split modes, combinations, child CU lists; wave w searching the QT leaves of
// quadrant w - is m2p_tree.h's, shared with Map2Partition (postproc.hip).  GenMSBtMap's own rules, all reproduced here:
//   * lamb1..lamb5 = 0.8, 1.0, 1.2, 0.2, 0.2 (:91), counts compared with double products in Python's order;
//   * the depth map is the integer LABEL bt (u8), one map for every level, and the direction map the i8 label dire (:125-130);
//   * a direction map that does not dominate returns [0] (:138-139);
//   * the candidate list starts EMPTY (:157); a sub-part qualifies if minus < n*lamb4 and (zero < n*lamb5 or zero > n*(1-lamb5));
//   * a CU with an empty list leaves its node WITHOUT children (:201-202): leaves can sit above depth 3;
//   * the leaf error is np.sum(np.abs(leaf - bt)) (:338) with a u8 leaf map: the subtraction wraps mod 256 (the root's map is i8,
//     so a root leaf costs sum(bt)); integers, first minimum in DFS leaf order wins (:340);
//   * outputs: the maps of the best leaf's depth-1 and depth-2 ancestors and of the leaf itself (:341-363).
// Where the reference has no answer (include/pmp.h: pmp_msbt_labels) a status bit is set and the kernel stays bounded.
//
// The same search also serves Map_to_SubMap(qt, bt, dire, cf).get_partition() (:262-312, map_to_parititon :377-382): the split flags
// of the labels' own partition (label_partition_kernel below; include/pmp.h: pmp_label_partition).  The templates' PART argument
// selects what a best leaf remembers: its CU list (PART) or the maps of its ancestors (!PART).
#include "../../include/pmp.h"
#include "m2p_tree.h"
#include "pmp_kernels.h"

namespace pmp {

using namespace tree;

namespace {

// GenMSBtMap.py:91 - Python's float64 values; (1 - lamb5) is formed in float64 as Python does (:180), and it is not 0.8
constexpr double L1 = 0.8, L2 = 1.0, L3 = 1.2, L4 = 0.2, L5 = 0.2, L5C = 1.0 - L5;

struct Sub {
    int row, col0;
    int lb[4];        // the label bt_map (u8)
    int ld[3][4];     // the label dire_map (i8), per layer
    int cf;
    // tree levels 0..3 (Map_Node, :81-87)
    int bt[4][4];
    int cu[4];        // lane c holds CU c of the level: x | y<<4 | (h-1)<<8 | (w-1)<<12
    int ncu[4];       // uniform
    // QT-leaf region, best leaf so far, leaf budget
    int rx, ry, rh, rw;
    int best_err, best_depth, have_best;
    int best[3][4];
    int best_cu, best_ncu;   // PART: the best leaf's CU list (lane c holds CU c)
    int nleaf, stop;
};

// can_split_mode_list (:123-186): returns the modes packed 3 bits each, their count in `n` (0: the empty list).
template <int L>
__device__ __forceinline__ int can_split(const Sub &s, int cu, int &n)
{
    const CU u = unpack_cu(cu);
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = s.row >= u.x && s.row < u.x + u.h && s.col0 + k >= u.y && s.col0 + k < u.y + u.w;
    int zero = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) zero += cnt(in[k] && s.lb[k] == s.bt[L][k]);
    n = 1;
    if ((double)zero >= L1 * u.h * u.w) return 0;            // no partition: [0]
    int hor = 0, ver = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hor += cnt(in[k] && s.ld[L][k] == 1);
        ver += cnt(in[k] && s.ld[L][k] == -1);
    }
    int direction = 0;
    if ((double)(ver + hor) >= L2 * u.h * u.w) {
        if ((double)hor >= L3 * ver) direction = 1;
        else if ((double)ver >= L3 * hor) direction = 2;
    } else {
        return 0;                                        // [0]
    }
    n = 0;                                               // the list starts empty (:157)
    return split_modes(u.h, u.w, s.cf, direction, 0, n, [&](bool horiz, int o0, int o1, int inc, int np_) {
        int minus = 0, zer = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = horiz ? (s.row - u.x) : (s.col0 + k - u.y);
            const bool ins = in[k] && t >= o0 && t < o1;
            const int tgt = s.bt[L][k] + inc;            // bt_map_temp (i8) after the += 1 (+1): u8 - i8 -> i16, no wrap
            minus += cnt(ins && s.lb[k] < tgt);
            zer += cnt(ins && s.lb[k] == tgt);
        }
        return (double)minus < np_ * L4 && ((double)zer < np_ * L5 || (double)zer > np_ * L5C);
    });
}

// A leaf at depth D (get_leaf_nodes order = the order the DFS reaches it).  Budget: the (PMP_MSBT_LEAF_BUDGET + 1)-th leaf stops the
// region's search; the best of the leaves scored so far stands.
template <int D, bool PART>
__device__ __forceinline__ void score_leaf(Sub &s)
{
    if (s.nleaf >= PMP_MSBT_LEAF_BUDGET) { s.stop = 1; return; }
    ++s.nleaf;
    int e = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (in_region(s, k))
            e += D == 0 ? s.lb[k] : ((s.bt[D][k] - s.lb[k]) & 255);   // i8 root map: |0 - bt|; u8 child maps: (leaf - bt) mod 256
    }
    e += __shfl_xor(e, 32);
    e += __shfl_xor(e, 16);
    e += __shfl_xor(e, 8);
    e += __shfl_xor(e, 4);
    e += __shfl_xor(e, 2);
    e += __shfl_xor(e, 1);
    e = uni(e);
    if (!s.have_best || e < s.best_err) {
        s.have_best = 1;
        s.best_err = e;
        s.best_depth = D;
        if constexpr (PART) {       // best_cus (:278); set_bt_partition_vector never walks parents, so any depth is legal
            s.best_cu = s.cu[D];
            s.best_ncu = s.ncu[D];
            return;
        }
        // sub_map[k] = map of the ancestor at depth min(k+1, D) (D = 3: the reference's :361-363; D < 3: the carry-down rule)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s.best[0][k] = D >= 1 ? s.bt[1][k] : 0;
            s.best[1][k] = D >= 2 ? s.bt[2][k] : (D >= 1 ? s.bt[1][k] : 0);
            s.best[2][k] = D >= 1 ? s.bt[D][k] : 0;
        }
    }
}

// get_candidate_map_tree (:188-241) for a node at level L.
template <int L, bool PART>
__device__ __forceinline__ void expand(Sub &s)
{
    if constexpr (L == 3) {
        score_leaf<3, PART>(s);
    } else {
        const int lane = threadIdx.x & 63;
        const int ncu = s.ncu[L];
        int my_list = 0, my_n = 1;
        for (int c = 0; c < ncu; ++c) {
            int n;
            const int list = can_split<L>(s, rlane(s.cu[L], c), n);
            if (n == 0) { score_leaf<L, PART>(s); return; }    // a CU without a proper partition: the node has no children (:201-202)
            if (lane == c) { my_list = list; my_n = n; }
        }
        const auto [my_p, total] = combos(my_n, ncu);   // Search, :45-79
        for (int t = 0; t < total && !s.stop; ++t) {
            int nb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) nb[k] = s.bt[L][k];
            s.ncu[L + 1] = apply_combination(s.row, s.col0, s.cu[L], ncu, mode_in(my_list, my_n, my_p, t), nb, s.cu[L + 1], [](int, bool) {});
#pragma unroll
            for (int k = 0; k < 4; ++k) s.bt[L + 1][k] = nb[k];
            expand<L + 1, PART>(s);
        }
    }
}

}  // namespace

// One workgroup of four waves per block.  Wave 0 takes a block that is one QT leaf; otherwise wave w takes the QT nodes of quadrant w.
__global__ __launch_bounds__(256) void msbt_labels_kernel(const uint8_t *__restrict__ qt, const uint8_t *__restrict__ bt,
                                                          const int8_t *__restrict__ dire, int64_t N, int cf,
                                                          uint8_t *__restrict__ msbt, uint8_t *__restrict__ status)
{
    __shared__ int st_w[4];
    const int64_t b = blockIdx.x;
    if (b >= N) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

    Sub s;
    s.row = lane >> 2;
    s.col0 = (lane & 3) << 2;
    s.cf = cf;
    {
        const uint32_t vb = reinterpret_cast<const uint32_t *>(bt + b * 256)[lane];
#pragma unroll
        for (int k = 0; k < 4; ++k) s.lb[k] = (vb >> (8 * k)) & 255;
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) {
            const uint32_t vd = reinterpret_cast<const uint32_t *>(dire + (b * 3 + k3) * 256)[lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) s.ld[k3][k] = (int)(int8_t)((vd >> (8 * k)) & 255);
        }
    }
    const int q8 = qt[b * 64 + lane];            // lane l holds qt[l>>3][l&7]
    int outd[3][4];
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
        for (int k = 0; k < 4; ++k) outd[k3][k] = 0;
    int st = 0;

    // ---- set_sub_map (:314-324), flattened: a node at depth d is reached iff every ancestor's qt (read at its top-left cell) exceeds
    // the ancestor's depth.  Beyond depth 3 the reference recurses on empty regions only: such a region stays zero (status bit 2).
    // walk_quadrant's loop and set_region's lines stand here in the open: behind the shared forms this kernel alone is allotted 133
    // VGPRs with 24 B of scratch per lane, or 205-207 VGPRs at two waves per SIMD, against 150 and 12 B like this (and 152 / 12 B
    // before the search was shared; profiles/m2p_tree_shared.txt)
    for (int d = 0; d < 4; ++d) {
        const int sms = 8 >> d, nside = 1 << d;
        for (int node = 0; node < nside * nside; ++node) {
            const int qx = (node / nside) * sms, qy = (node % nside) * sms;
            if (!node_is_mine(q8, wv, d, qx, qy)) continue;
            const int c = rlane(q8, qx * 8 + qy);
            if (c > d) {
                if (d == 3) st |= PMP_MSBT_QT_DEEP;
                continue;
            }
            if (c < d) continue;                          // neither == nor >: nothing is written (zeros)
            // ---- set_bt_sub_map (:326-364) on [2qx, 2qy, 2sms, 2sms]
            s.rx = 2 * qx; s.ry = 2 * qy; s.rh = 2 * sms; s.rw = 2 * sms;
#pragma unroll
            for (int k = 0; k < 4; ++k) s.bt[0][k] = 0;
            s.cu[0] = pack_cu(s.rx, s.ry, s.rh, s.rw);
            s.ncu[0] = 1;
            s.have_best = 0;
            s.best_err = 0;
            s.best_depth = 0;
            s.nleaf = 0;
            s.stop = 0;
            expand<0, false>(s);
            if (s.best_depth < 3) st |= PMP_MSBT_INCONSISTENT;
            if (s.stop) st |= PMP_MSBT_BUDGET;
            copy_region(s, outd, s.best);
        }
    }
    if (lane == 0) st_w[wv] = st;
    store_planes(msbt + b * 768, outd, q8, wv);
    __syncthreads();
    if (threadIdx.x == 0) status[b] = (uint8_t)(st_w[0] | st_w[1] | st_w[2] | st_w[3]);
}

// Map_to_SubMap.get_partition (:262-312) cropped as map_to_parititon does (:382): the split flags of the labels' own partition.
// The same flattened QT walk and the same search as above; a region's best leaf hands over its CU list, whose edges are painted as
// :285-292 do, and every QT node that splits further paints its cross (:300-304; sms = 8 >> d, at d = 3 as well, where nothing else
// follows: status bit 2).  c < d paints nothing.  A best leaf above depth 3 is legal here, so bit 1 is never set.
// Edges cross wave ownership (a CU's bottom edge on row 8 lies in the quadrant below), so every wave keeps its own 16-bit row masks in
// registers - lane r: hor row r, lane 16 + r: ver row r; bit c = column c; row / column 16 of the reference's 17x17 par_vec has no
// lane and no bit - and hands them over through one LDS slot per wave; they are OR-ed after the barrier.  No atomics.
// Outputs: hor, ver u8[256] per block at `stride` bytes from block to block; qt_o / dire_o (records form, else null) receive byte
// copies of the inputs at the same stride.
__global__ __launch_bounds__(256) void label_partition_kernel(const uint8_t *__restrict__ qt, const uint8_t *__restrict__ bt,
                                                              const int8_t *__restrict__ dire, int64_t N, int cf,
                                                              uint8_t *__restrict__ hor_o, uint8_t *__restrict__ ver_o,
                                                              uint8_t *__restrict__ qt_o, int8_t *__restrict__ dire_o, int stride,
                                                              uint8_t *__restrict__ status)
{
    __shared__ int st_w[4];
    __shared__ uint32_t msk[4][32];
    const int64_t b = blockIdx.x;
    if (b >= N) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

    Sub s;
    s.row = lane >> 2;
    s.col0 = (lane & 3) << 2;
    s.cf = cf;
    uint32_t vd[3];
    {
        const uint32_t vb = reinterpret_cast<const uint32_t *>(bt + b * 256)[lane];
#pragma unroll
        for (int k = 0; k < 4; ++k) s.lb[k] = (vb >> (8 * k)) & 255;
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) {
            vd[k3] = reinterpret_cast<const uint32_t *>(dire + (b * 3 + k3) * 256)[lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) s.ld[k3][k] = (int)(int8_t)((vd[k3] >> (8 * k)) & 255);
        }
    }
    const int q8 = qt[b * 64 + lane];            // lane l holds qt[l>>3][l&7]
    const int j = lane & 15, part = lane >> 4;   // part 0: hor row j, part 1: ver row j
    uint32_t em = 0;                             // a wave that paints nothing hands over zeros
    int st = 0;

    walk_quadrant(q8, wv, [j, part](int d, int qx, int qy, int sms, int c, Sub &s, int &st, uint32_t &em) {
        if (c > d) {
            // the QT cross of [2qx, 2qy, 2sms, 2sms]: row 2qx + sms and column 2qy + sms (both <= 15)
            if (part == 0 && j == 2 * qx + sms) em |= ((1u << (2 * sms)) - 1u) << (2 * qy);
            if (part == 1 && j >= 2 * qx && j < 2 * qx + 2 * sms) em |= 1u << (2 * qy + sms);
            if (d == 3) st |= PMP_MSBT_QT_DEEP;           // the reference recurses on empty regions from here: nothing more is painted
            return;
        }
        if (c < d) return;                                // neither == nor >: nothing is painted
        // ---- set_bt_partition_vector (:262-292) on [2qx, 2qy, 2sms, 2sms]
        set_region(s, qx, qy, sms);
        s.have_best = 0;
        s.best_err = 0;
        s.best_depth = 0;
        s.best_cu = 0;
        s.best_ncu = 0;
        s.nleaf = 0;
        s.stop = 0;
        expand<0, true>(s);
        if (s.stop) st |= PMP_MSBT_BUDGET;
        const int ncu = uni(s.best_ncu);
        for (int ci = 0; ci < ncu; ++ci) {
            const CU u = unpack_cu(rlane(s.best_cu, ci));
            // rows x and x + h over columns y..y+w-1; columns y and y + w over rows x..x+h-1.  x + h = 16 matches no lane and
            // bit y + w = 16 is masked off: the crop of :382
            if (part == 0 && (j == u.x || j == u.x + u.h)) em |= ((1u << u.w) - 1u) << u.y;
            if (part == 1 && j >= u.x && j < u.x + u.h) em |= (1u << u.y) | ((1u << (u.y + u.w)) & 0xFFFFu);
        }
    }, s, st, em);
    if (lane < 32) msk[wv][lane] = em;
    if (lane == 0) st_w[wv] = st;
    __syncthreads();
    if (wv < 2) {                                 // wave 0 writes hor, wave 1 ver: lane l the cells of row l>>2, columns 4*(l&3)..+3
        const int r = wv * 16 + s.row;
        const uint32_t m = ((msk[0][r] | msk[1][r] | msk[2][r] | msk[3][r]) >> s.col0) & 15u;
        const uint32_t pk = (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
        reinterpret_cast<uint32_t *>((wv == 0 ? hor_o : ver_o) + b * stride)[lane] = pk;
    } else if (wv == 2) {
        if (qt_o && lane < 16) reinterpret_cast<uint32_t *>(qt_o + b * stride)[lane] = reinterpret_cast<const uint32_t *>(qt + b * 64)[lane];
    } else if (dire_o) {
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) reinterpret_cast<uint32_t *>(dire_o + b * stride + k3 * 256)[lane] = vd[k3];
    }
    if (threadIdx.x == 0) status[b] = (uint8_t)(st_w[0] | st_w[1] | st_w[2] | st_w[3]);
}

// Grids of at most 2^20 blocks (gridDim.x is 32-bit; blocks are independent): launch(o, m) takes blocks o..o+m-1.
template <class Launch>
static hipError_t for_grids(int64_t N, Launch &&launch)
{
    for (int64_t o = 0; o < N; o += (int64_t)1 << 20) launch(o, (N - o) < ((int64_t)1 << 20) ? (N - o) : ((int64_t)1 << 20));
    return hipGetLastError();
}

hipError_t launch_label_partition(hipStream_t st, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t N, int chroma_factor,
                                  uint8_t *hor, uint8_t *ver, uint8_t *rec, uint8_t *status)
{
    // rec: one packed PMP_RECORD_BYTES record per block (hor | ver | qt | dire) instead of the two dense arrays
    const int stride = rec ? PMP_RECORD_BYTES : 256;
    return for_grids(N, [&](int64_t o, int64_t m) {
        uint8_t *h = rec ? rec + o * stride : hor + o * stride, *v = rec ? h + 256 : ver + o * stride;
        hipLaunchKernelGGL(label_partition_kernel, dim3((unsigned)m), dim3(256), 0, st, qt + o * 64, bt + o * 256, dire + o * 768, m,
                           chroma_factor, h, v, rec ? h + 512 : (uint8_t *)nullptr, rec ? (int8_t *)(h + 576) : (int8_t *)nullptr, stride,
                           status + o);
    });
}

hipError_t launch_msbt_labels(hipStream_t st, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t N, int chroma_factor,
                              uint8_t *msbt, uint8_t *status)
{
    return for_grids(N, [&](int64_t o, int64_t m) {
        hipLaunchKernelGGL(msbt_labels_kernel, dim3((unsigned)m), dim3(256), 0, st, qt + o * 64, bt + o * 256, dire + o * 768, m,
                           chroma_factor, msbt + o * 768, status + o);
    });
}

}  // namespace pmp
