// labels.hip — GenMSBtMap on the GPU: the per-layer MTT depth labels (MSBT) of the training set, one workgroup per 64x64 block.
//
// Replaces, bit-exactly wherever the reference finishes:
//   Map_to_SubMap(qt, bt, dire, cf).get_sub_map()   GenMSBtMap.py:89-368  (called per block by gen_seq_sub_map, :434-449)
//
// Same design as postproc.hip (Map2Partition): the block's 16x16 cells spread over the 64 lanes, 4 per lane (lane l: row l>>2,
// columns 4*(l&3)..+3); the candidate-tree search (get_candidate_map_tree, :188-241) as wave-uniform DFS with region counts by
// ballot + popcount, CU lists lane-distributed, the three MTT levels unrolled at compile time; four waves per block, wave w
// searching the QT leaves of quadrant w.  What differs from Map2Partition (all reproduced):
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
#include "pmp_kernels.h"

namespace pmp {

namespace {

__device__ __forceinline__ int rlane(int v, int lane)
{
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int cnt(bool p) { return __popcll(__ballot(p)); }

__device__ __forceinline__ int pack_cu(int x, int y, int h, int w) { return x | (y << 4) | ((h - 1) << 8) | ((w - 1) << 12); }

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
    const int x = cu & 15, y = (cu >> 4) & 15, h = ((cu >> 8) & 15) + 1, w = ((cu >> 12) & 15) + 1;
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = s.row >= x && s.row < x + h && s.col0 + k >= y && s.col0 + k < y + w;
    int zero = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) zero += cnt(in[k] && s.lb[k] == s.bt[L][k]);
    n = 1;
    if ((double)zero >= L1 * h * w) return 0;            // no partition: [0]
    int hor = 0, ver = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hor += cnt(in[k] && s.ld[L][k] == 1);
        ver += cnt(in[k] && s.ld[L][k] == -1);
    }
    int direction = 0;
    if ((double)(ver + hor) >= L2 * h * w) {
        if ((double)hor >= L3 * ver) direction = 1;
        else if ((double)ver >= L3 * hor) direction = 2;
    } else {
        return 0;                                        // [0]
    }
    const int cf = s.cf;
    int list = 0;
    n = 0;
    for (int mode = 1; mode <= 4; ++mode) {
        const bool horiz = (mode & 1) != 0;      // 1 BT-H, 3 TT-H
        const int ext = horiz ? h : w;
        const int div = (mode <= 2 ? 2 : 4) * cf;
        if (ext / div == 0 || ext % div != 0) continue;
        if (horiz && direction == 2) continue;
        if (!horiz && direction == 1) continue;
        const int parts = mode <= 2 ? 2 : 3;
        int ok = 0;
        for (int p = 0; p < parts; ++p) {
            int o0, o1, inc;
            if (mode <= 2) { o0 = p * (ext / 2); o1 = o0 + ext / 2; inc = 1; }
            else if (p == 0) { o0 = 0; o1 = ext / 4; inc = 2; }
            else if (p == 1) { o0 = ext / 4; o1 = o0 + ext / 2; inc = 1; }
            else { o0 = (ext * 3) / 4; o1 = ext; inc = 2; }
            int minus = 0, zer = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = horiz ? (s.row - x) : (s.col0 + k - y);
                const bool ins = in[k] && t >= o0 && t < o1;
                const int tgt = s.bt[L][k] + inc;        // bt_map_temp (i8) after the += 1 (+1): u8 - i8 -> i16, no wrap
                minus += cnt(ins && s.lb[k] < tgt);
                zer += cnt(ins && s.lb[k] == tgt);
            }
            const int np_ = (o1 - o0) * (horiz ? w : h);
            if ((double)minus < np_ * L4 && ((double)zer < np_ * L5 || (double)zer > np_ * L5C)) ++ok;
        }
        if (ok == parts) { list |= mode << (3 * n); ++n; }
    }
    return list;
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
        const int r = s.row - s.rx, c = s.col0 + k - s.ry;
        if (r >= 0 && r < s.rh && c >= 0 && c < s.rw)
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
        // mixed-radix combination index, first CU slowest (Search, :45-79)
        int my_p = 1, total = 1;
        for (int c = ncu - 1; c >= 0; --c) {
            if (lane == c) my_p = total;
            total *= rlane(my_n, c);
        }
        total = uni(total);
        for (int t = 0; t < total && !s.stop; ++t) {
            const int my_mode = (my_list >> (3 * ((t / my_p) % my_n))) & 7;
            int nb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) nb[k] = s.bt[L][k];
            int child_cu = 0, nchild = 0;
            for (int c = 0; c < ncu; ++c) {
                const int mode = rlane(my_mode, c), cu = rlane(s.cu[L], c);
                const int x = cu & 15, y = (cu >> 4) & 15, h = ((cu >> 8) & 15) + 1, w = ((cu >> 12) & 15) + 1;
                if (mode == 0) {
                    if (lane == nchild) child_cu = cu;
                    nchild += 1;
                    continue;
                }
                const bool horiz = (mode & 1) != 0;
                const int ext = horiz ? h : w;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = s.row - x, cc = s.col0 + k - y;
                    if (r >= 0 && r < h && cc >= 0 && cc < w) {
                        const int tt = horiz ? r : cc;
                        nb[k] += (mode >= 3 && (tt < ext / 4 || tt >= (ext * 3) / 4)) ? 2 : 1;
                    }
                }
                // split_cur_map (:107-121): sub-CUs appended in order
                if (mode <= 2) {
                    const int e = ext / 2;
                    const int c0 = horiz ? pack_cu(x, y, e, w) : pack_cu(x, y, h, e);
                    const int c1 = horiz ? pack_cu(x + e, y, e, w) : pack_cu(x, y + e, h, e);
                    if (lane == nchild) child_cu = c0;
                    if (lane == nchild + 1) child_cu = c1;
                    nchild += 2;
                } else {
                    const int q = ext / 4, e = ext / 2, o2 = (ext * 3) / 4;
                    const int c0 = horiz ? pack_cu(x, y, q, w) : pack_cu(x, y, h, q);
                    const int c1 = horiz ? pack_cu(x + q, y, e, w) : pack_cu(x, y + q, h, e);
                    const int c2 = horiz ? pack_cu(x + o2, y, q, w) : pack_cu(x, y + o2, h, q);
                    if (lane == nchild) child_cu = c0;
                    if (lane == nchild + 1) child_cu = c1;
                    if (lane == nchild + 2) child_cu = c2;
                    nchild += 3;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) s.bt[L + 1][k] = nb[k];
            s.cu[L + 1] = child_cu;
            s.ncu[L + 1] = uni(nchild);
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
    for (int d = 0; d < 4; ++d) {
        const int sms = 8 >> d, nside = 1 << d;
        for (int node = 0; node < nside * nside; ++node) {
            const int qx = (node / nside) * sms, qy = (node % nside) * sms;
            bool reached = true;
            for (int a = 0; a < d; ++a) {
                const int am = ~((8 >> a) - 1);
                if (!(rlane(q8, (qx & am) * 8 + (qy & am)) > a)) reached = false;
            }
            if (!reached) continue;
            if (wv != (d == 0 ? 0 : ((qx >= 4 ? 2 : 0) + (qy >= 4 ? 1 : 0)))) continue;   // another wave's quadrant
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
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = s.row - s.rx, cc = s.col0 + k - s.ry;
                if (r >= 0 && r < s.rh && cc >= 0 && cc < s.rw) {
                    outd[0][k] = s.best[0][k]; outd[1][k] = s.best[1][k]; outd[2][k] = s.best[2][k];
                }
            }
        }
    }
    if (lane == 0) st_w[wv] = st;
    // a lane's four cells lie in one quadrant: its owner holds their labels
    const bool whole = rlane(q8, 0) == 0;
    const int quad = ((lane >> 2) >= 8 ? 2 : 0) + ((lane & 3) >= 2 ? 1 : 0);
    if (whole ? wv == 0 : wv == quad) {
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) {
            const uint32_t pk = (uint32_t)(uint8_t)outd[k3][0] | ((uint32_t)(uint8_t)outd[k3][1] << 8) |
                                ((uint32_t)(uint8_t)outd[k3][2] << 16) | ((uint32_t)(uint8_t)outd[k3][3] << 24);
            reinterpret_cast<uint32_t *>(msbt + (b * 3 + k3) * 256)[lane] = pk;
        }
    }
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

    for (int d = 0; d < 4; ++d) {
        const int sms = 8 >> d, nside = 1 << d;
        for (int node = 0; node < nside * nside; ++node) {
            const int qx = (node / nside) * sms, qy = (node % nside) * sms;
            bool reached = true;
            for (int a = 0; a < d; ++a) {
                const int am = ~((8 >> a) - 1);
                if (!(rlane(q8, (qx & am) * 8 + (qy & am)) > a)) reached = false;
            }
            if (!reached) continue;
            if (wv != (d == 0 ? 0 : ((qx >= 4 ? 2 : 0) + (qy >= 4 ? 1 : 0)))) continue;   // another wave's quadrant
            const int c = rlane(q8, qx * 8 + qy);
            if (c > d) {
                // the QT cross of [2qx, 2qy, 2sms, 2sms]: row 2qx + sms and column 2qy + sms (both <= 15)
                if (part == 0 && j == 2 * qx + sms) em |= ((1u << (2 * sms)) - 1u) << (2 * qy);
                if (part == 1 && j >= 2 * qx && j < 2 * qx + 2 * sms) em |= 1u << (2 * qy + sms);
                if (d == 3) st |= PMP_MSBT_QT_DEEP;       // the reference recurses on empty regions from here: nothing more is painted
                continue;
            }
            if (c < d) continue;                          // neither == nor >: nothing is painted
            // ---- set_bt_partition_vector (:262-292) on [2qx, 2qy, 2sms, 2sms]
            s.rx = 2 * qx; s.ry = 2 * qy; s.rh = 2 * sms; s.rw = 2 * sms;
#pragma unroll
            for (int k = 0; k < 4; ++k) s.bt[0][k] = 0;
            s.cu[0] = pack_cu(s.rx, s.ry, s.rh, s.rw);
            s.ncu[0] = 1;
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
                const int cu = rlane(s.best_cu, ci);
                const int x = cu & 15, y = (cu >> 4) & 15, h = ((cu >> 8) & 15) + 1, w = ((cu >> 12) & 15) + 1;
                // rows x and x + h over columns y..y+w-1; columns y and y + w over rows x..x+h-1.  x + h = 16 matches no lane and
                // bit y + w = 16 is masked off: the crop of :382
                if (part == 0 && (j == x || j == x + h)) em |= ((1u << w) - 1u) << y;
                if (part == 1 && j >= x && j < x + h) em |= (1u << y) | ((1u << (y + w)) & 0xFFFFu);
            }
        }
    }
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

hipError_t launch_label_partition(hipStream_t st, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t N, int chroma_factor,
                                  uint8_t *hor, uint8_t *ver, uint8_t *rec, uint8_t *status)
{
    // rec: one packed PMP_RECORD_BYTES record per block (hor | ver | qt | dire) instead of the two dense arrays
    const int stride = rec ? PMP_RECORD_BYTES : 256;
    for (int64_t o = 0; o < N; o += (int64_t)1 << 20) {
        const int64_t m = (N - o) < ((int64_t)1 << 20) ? (N - o) : ((int64_t)1 << 20);
        uint8_t *h = rec ? rec + o * stride : hor + o * stride, *v = rec ? h + 256 : ver + o * stride;
        hipLaunchKernelGGL(label_partition_kernel, dim3((unsigned)m), dim3(256), 0, st, qt + o * 64, bt + o * 256, dire + o * 768, m,
                           chroma_factor, h, v, rec ? h + 512 : (uint8_t *)nullptr, rec ? (int8_t *)(h + 576) : (int8_t *)nullptr, stride,
                           status + o);
    }
    return hipGetLastError();
}

hipError_t launch_msbt_labels(hipStream_t st, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t N, int chroma_factor,
                              uint8_t *msbt, uint8_t *status)
{
    // grids of at most 2^20 blocks (gridDim.x is 32-bit); blocks are independent
    for (int64_t o = 0; o < N; o += (int64_t)1 << 20) {
        const int64_t m = (N - o) < ((int64_t)1 << 20) ? (N - o) : ((int64_t)1 << 20);
        hipLaunchKernelGGL(msbt_labels_kernel, dim3((unsigned)m), dim3(256), 0, st, qt + o * 64, bt + o * 256, dire + o * 768, m,
                           chroma_factor, msbt + o * 768, status + o);
    }
    return hipGetLastError();
}

}  // namespace pmp
