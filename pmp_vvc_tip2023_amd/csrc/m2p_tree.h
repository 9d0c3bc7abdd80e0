// m2p_tree.h — the wave-uniform partition-tree search that Map2Partition (postproc.hip, on logits) and GenMSBtMap (labels.hip, on
// labels) share, stated once.  The reference states it twice as well (Map2Partition.py:53-266, GenMSBtMap.py:45-241), with two rule sets.
//
// Common ground: the 16x16 grid of 4x4-pixel cells of a 64x64 block lies on the 64 lanes of a wave, 4 cells per lane in row-major
// order (lane l: row l>>2, columns 4*(l&3)..+3); four waves per block, wave w searching the QT leaves under quadrant w (a block
// that is one 64x64 leaf is wave 0's); control flow is uniform, region counts are ballot + popcount, and "arrays indexed by a
// uniform index" (a level's CU list, its candidate lists) lie one entry per lane and are read with v_readlane.
// Here: the lane helpers and the packed CU word, the flattened quadtree walk, the split modes of a CU with their sub-parts, the
// combination counter, a combination applied to a node, and the owner's store of three cell planes.  What a rule set accepts, what
// a leaf costs and what a kernel does at a QT node stay with the callers, as lambdas: everything here inlines into their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmp {
namespace tree {

__device__ __forceinline__ int rlane(int v, int lane)
{
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}
__device__ __forceinline__ float rlanef(float v, int lane) { return __int_as_float(rlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int cnt(bool p) { return __popcll(__ballot(p)); }

// A CU in cells: rows x..x+h-1, columns y..y+w-1 of the 16x16 grid, as one word x | y<<4 | (h-1)<<8 | (w-1)<<12.
struct CU { int x, y, h, w; };
__device__ __forceinline__ int pack_cu(int x, int y, int h, int w) { return x | (y << 4) | ((h - 1) << 8) | ((w - 1) << 12); }
__device__ __forceinline__ CU unpack_cu(int cu) { return {cu & 15, (cu >> 4) & 15, ((cu >> 8) & 15) + 1, ((cu >> 12) & 15) + 1}; }

// ---- the quadtree of a block, flattened: lane l holds the 8x8 QT depth map's value at (l>>3, l&7) in `qt8`.  A node at depth d
// (side sms = 8 >> d, top-left (qx, qy), all in 8x8 units) is reached iff every ancestor's value, read at the ancestor's top-left,
// exceeds the ancestor's depth; it is wave wv's if it lies in quadrant wv (the root is wave 0's).
__device__ __forceinline__ bool node_is_mine(int qt8, int wv, int d, int qx, int qy)
{
    bool reached = true;
    for (int a = 0; a < d; ++a) {
        const int am = ~((8 >> a) - 1);
        if (!(rlane(qt8, (qx & am) * 8 + (qy & am)) > a)) reached = false;
    }
    return reached && wv == (d == 0 ? 0 : ((qx >= 4 ? 2 : 0) + (qy >= 4 ? 1 : 0)));   // else: another wave's quadrant
}
// Calls at(d, qx, qy, sms, c, state...), c the node's own value, for wave wv's reached nodes in depth-major, row-major order: c > d
// splits further, c == d is a QT leaf, c < d a hole.  A kernel's mutable state reaches `at` through `state`, by reference, or
// through the lambda's captures: the same program, but a closure that holds references stands between the kernel and its registers
// long enough to change what the compiler allots, so each kernel takes the form that measured no worse than the code it had before
// (profiles/m2p_tree_shared.txt: label_partition_kernel by `state`, postprocess_kernel by captures, msbt_labels_kernel by neither).
template <class At, class... State>
__device__ __forceinline__ void walk_quadrant(int qt8, int wv, At &&at, State &...state)
{
    for (int d = 0; d < 4; ++d) {
        const int sms = 8 >> d, nside = 1 << d;
        for (int node = 0; node < nside * nside; ++node) {
            const int qx = (node / nside) * sms, qy = (node % nside) * sms;
            if (node_is_mine(qt8, wv, d, qx, qy)) at(d, qx, qy, sms, rlane(qt8, qx * 8 + qy), state...);
        }
    }
}

// The search's root at a QT leaf: the region [2qx, 2qy, 2sms, 2sms] in cells as the one CU of level 0, on a zero depth map.
template <class S>
__device__ __forceinline__ void set_region(S &s, int qx, int qy, int sms)
{
    s.rx = 2 * qx; s.ry = 2 * qy; s.rh = 2 * sms; s.rw = 2 * sms;
#pragma unroll
    for (int k = 0; k < 4; ++k) s.bt[0][k] = 0;
    s.cu[0] = pack_cu(s.rx, s.ry, s.rh, s.rw);
    s.ncu[0] = 1;
}
template <class S>
__device__ __forceinline__ bool in_region(const S &s, int k)   // this lane's cell k
{
    const int r = s.row - s.rx, c = s.col0 + k - s.ry;
    return r >= 0 && r < s.rh && c >= 0 && c < s.rw;
}

// A region's result into the block's: the lane's cells inside the region take src, the others keep what they have.
template <class S>
__device__ __forceinline__ void copy_region(const S &s, int (&dst)[3][4], const int (&src)[3][4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (in_region(s, k)) { dst[0][k] = src[0][k]; dst[1][k] = src[1][k]; dst[2][k] = src[2][k]; }
}

// ---- split modes: 1 BT-H, 2 BT-V, 3 TT-H, 4 TT-V.  Sub-part p of a split of extent ext: offsets o0..o1-1 along the split axis and
// the depth it adds (split_cur_map; a TT's outer quarters are two levels down).
struct Part { int o0, o1, inc; };
__device__ __forceinline__ int parts_of(int mode) { return mode <= 2 ? 2 : 3; }
__device__ __forceinline__ Part sub_part(int mode, int p, int ext)
{
    if (mode <= 2) return {p * (ext / 2), p * (ext / 2) + ext / 2, 1};
    if (p == 0) return {0, ext / 4, 2};
    if (p == 1) return {ext / 4, ext / 4 + ext / 2, 1};
    return {(ext * 3) / 4, ext, 2};
}

// The tail of can_split_mode_list: appends to `list` (3 bits per entry, `n` entries so far) every mode that fits an h x w CU at
// chroma factor cf, that the dominant direction (0 none, 1 horizontal, 2 vertical) allows, and whose sub-parts all pass
// part_ok(horiz, o0, o1, inc, cells of the part).  Every part is asked, as the reference does.
template <class Ok>
__device__ __forceinline__ int split_modes(int h, int w, int cf, int direction, int list, int &n, Ok &&part_ok)
{
    for (int mode = 1; mode <= 4; ++mode) {
        const bool horiz = (mode & 1) != 0;
        const int ext = horiz ? h : w;
        const int div = (mode <= 2 ? 2 : 4) * cf;
        if (ext / div == 0 || ext % div != 0) continue;
        if (horiz && direction == 2) continue;
        if (!horiz && direction == 1) continue;
        const int parts = parts_of(mode);
        int ok = 0;
        for (int p = 0; p < parts; ++p) {
            const Part pt = sub_part(mode, p, ext);
            if (part_ok(horiz, pt.o0, pt.o1, pt.inc, (pt.o1 - pt.o0) * (horiz ? w : h))) ++ok;
        }
        if (ok == parts) { list |= mode << (3 * n); ++n; }
    }
    return list;
}

// ---- combinations of a level (Search): lane c holds CU c's candidate count my_n; combination t of `total` takes candidate
// (t / my_p) % my_n of CU c - mixed radix, first CU slowest.
struct Combos { int my_p, total; };
__device__ __forceinline__ Combos combos(int my_n, int ncu)
{
    const int lane = threadIdx.x & 63;
    int my_p = 1, total = 1;
    for (int c = ncu - 1; c >= 0; --c) {
        if (lane == c) my_p = total;
        total *= rlane(my_n, c);
    }
    return {my_p, uni(total)};
}
__device__ __forceinline__ int mode_in(int my_list, int my_n, int my_p, int t) { return (my_list >> (3 * ((t / my_p) % my_n))) & 7; }

// One combination applied to a node (get_candidate_map_tree's inner loop with split_cur_map): lane c holds CU c of the node in `cus`
// and its mode in this combination in `my_mode`.  Adds the split depth to the lane's cells nb[] at (row, col0..col0+3), calls
// cell(k, horiz) for each cell k inside a CU that splits, and returns the child CU list - unsplit CUs as they are, sub-CUs in
// split_cur_map's order - one per lane in child_cu, its length as the result.
template <class Cell>
__device__ __forceinline__ int apply_combination(int row, int col0, int cus, int ncu, int my_mode, int (&nb)[4], int &child_cu, Cell &&cell)
{
    const int lane = threadIdx.x & 63;
    int nchild = 0;
    child_cu = 0;
    auto push = [&](int cu) { if (lane == nchild) child_cu = cu; ++nchild; };
    for (int c = 0; c < ncu; ++c) {
        const int mode = rlane(my_mode, c), cu = rlane(cus, c);
        if (mode == 0) { push(cu); continue; }
        const CU u = unpack_cu(cu);
        const bool horiz = (mode & 1) != 0;
        const int ext = horiz ? u.h : u.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = row - u.x, cc = col0 + k - u.y;
            if (r >= 0 && r < u.h && cc >= 0 && cc < u.w) {
                cell(k, horiz);
                const int tt = horiz ? r : cc;
                nb[k] += (mode >= 3 && (tt < ext / 4 || tt >= (ext * 3) / 4)) ? 2 : 1;
            }
        }
        // split_cur_map: the sub-CUs appended in order (each branch forms its CUs before it places them: the hot kernel's register
        // allocation follows this text closely, profiles/m2p_tree_shared.txt)
        auto sub = [&](int p) {
            const Part pt = sub_part(mode, p, ext);
            return horiz ? pack_cu(u.x + pt.o0, u.y, pt.o1 - pt.o0, u.w) : pack_cu(u.x, u.y + pt.o0, u.h, pt.o1 - pt.o0);
        };
        if (mode <= 2) {
            const int c0 = sub(0), c1 = sub(1);
            if (lane == nchild) child_cu = c0;
            if (lane == nchild + 1) child_cu = c1;
            nchild += 2;
        } else {
            const int c0 = sub(0), c1 = sub(1), c2 = sub(2);
            if (lane == nchild) child_cu = c0;
            if (lane == nchild + 1) child_cu = c1;
            if (lane == nchild + 2) child_cu = c2;
            nchild += 3;
        }
    }
    return uni(nchild);
}

// ---- epilogue: a lane's four cells lie in one quadrant, whose owner wave holds their results.
__device__ __forceinline__ bool owns_my_cells(int qt8, int wv)
{
    const int lane = threadIdx.x & 63;
    const bool whole = rlane(qt8, 0) == 0;   // the block is one 64x64 leaf: wave 0 searched it
    const int quad = ((lane >> 2) >= 8 ? 2 : 0) + ((lane & 3) >= 2 ? 1 : 0);
    return whole ? wv == 0 : wv == quad;
}
__device__ __forceinline__ uint32_t pack4(const int (&v)[4])
{
    return (uint32_t)(uint8_t)v[0] | ((uint32_t)(uint8_t)v[1] << 8) | ((uint32_t)(uint8_t)v[2] << 16) | ((uint32_t)(uint8_t)v[3] << 24);
}
// Three consecutive 256-byte planes at `planes`, one byte per cell: the owner of this lane's cells stores them, four bytes a plane.
template <class T>
__device__ __forceinline__ void store_planes(T *planes, const int (&v)[3][4], int qt8, int wv)
{
    if (!owns_my_cells(qt8, wv)) return;
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) reinterpret_cast<uint32_t *>(planes + k3 * 256)[threadIdx.x & 63] = pack4(v[k3]);
}

}  // namespace tree
}  // namespace pmp
