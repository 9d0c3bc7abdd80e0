// train_check.h — what pmp_resblock_*, pmp_trunk_*, pmp_stem_*, pmp_head_* and pmp_gate_* (api_train.cpp) accept: the shape rules, a
// trunk's blocks and its d_saved layout, a stem's and a head's sizes, and the rules on a call's tensors.  A single block is checked as
// the one-block trunk it is.  Pure host code without the HIP runtime, so that it also builds, with a main of its own, for the CPU
// under a sanitizer (train_check_main.cpp, `make traincheck`).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <vector>

#include "../../include/pmp.h"

namespace pmp {

// the channel counts the convolution kernels have; 128 only as an input: a QT net's resblock_q4 (pmp_qtail_*)
inline int pad_channels(int c) { return c <= 16 ? 16 : c <= 32 ? 32 : c <= 64 ? 64 : 128; }

constexpr const char *TRAIN_SHAPE_RULE =
    "null or unsupported shape (n 1..256, h and w multiples of 16 in 16..256, channels 1..64, k 3 or 5, 1..8 blocks, pool 0 or 1)";

inline bool train_shape_ok(const pmp_trunk_shape *s)
{
    auto side = [](int v) { return v >= 16 && v <= 256 && !(v & 15); };
    if (!s || s->n < 1 || s->n > 256 || !side(s->h) || !side(s->w) || s->cin < 1 || s->cin > 64 || s->nblocks < 1 ||
        s->nblocks > PMP_TRUNK_MAX_BLOCKS || (s->pool != 0 && s->pool != 1))
        return false;
    for (int i = 0; i < s->nblocks; ++i)
        if (s->cout[i] < 1 || s->cout[i] > 64 || (s->k[i] != 3 && s->k[i] != 5)) return false;
    return true;
}

inline pmp_trunk_shape one_block(const pmp_rb_shape &s) { return pmp_trunk_shape{s.n, s.h, s.w, s.cin, 1, {s.cout}, {s.k}, 0}; }

struct BlockShape {
    int cin, cout, k;
    int cip() const { return pad_channels(cin); }
    int cop() const { return pad_channels(cout); }
};

inline BlockShape block_shape(const pmp_trunk_shape &s, int i) { return BlockShape{i ? s.cout[i - 1] : s.cin, s.cout[i], s.k[i]}; }

// d_saved: blocked x, then t_i and out_i of every block, each [n][pad_channels(c)/16][h][w][16]
struct TrunkLayout {
    int nt;
    int c[2 * PMP_TRUNK_MAX_BLOCKS + 1];         // the real channels of saved tensor 0 .. nt-1 (pmp_trunk_unpack_device's index)
    size_t off[2 * PMP_TRUNK_MAX_BLOCKS + 2];    // bytes; off[nt] = the size
    explicit TrunkLayout(const pmp_trunk_shape &s) : nt(2 * s.nblocks + 1)
    {
        const size_t px = (size_t)s.n * s.h * s.w * sizeof(float);
        off[0] = 0;
        for (int i = 0; i < nt; ++i) {
            c[i] = i == 0 ? s.cin : s.cout[(i - 1) / 2];
            off[i + 1] = off[i] + px * pad_channels(c[i]);
        }
    }
};

// A tensor of a call.  optional: may be NULL (a g_x that is not asked for, the shortcut's weights of a block that has none)
struct Span { const void *p; size_t bytes; bool optional = false; unsigned align = 4; };

inline bool overlaps(const Span &a, const Span &b)
{
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}

// The weights of the blocks, w0, w2, wsc per block as in pmp_trunk_*'s d_w and d_g_w (a single block's: three pointers), go IN
// FRONT of the call's other tensors in ins / outs (the gradients only backward).  -> why the call is refused, or NULL
inline const char *weights_refused(const BlockShape *blocks, int nblocks, const float *const *w, float *const *g_w, bool backward,
                                   std::vector<Span> &ins, std::vector<Span> &outs)
{
    if (!w || (backward && !g_w)) return "null tensor";
    std::vector<Span> wi, wo;
    for (int i = 0; i < nblocks; ++i) {
        const BlockShape b = blocks[i];
        const size_t kk = (size_t)b.k * b.k * 4, bytes[3] = {kk * b.cout * b.cin, kk * b.cout * b.cout, (size_t)4 * b.cout * b.cin};
        for (int j = 0; j < 3; ++j) {
            const bool need = j < 2 || b.cin != b.cout;                 // w0, w2 required; wsc and g_wsc exactly when cin != cout
            const float *p = w[3 * i + j];
            if (j < 2 && !p) return "null tensor";
            if ((p != nullptr) != need) return "a shortcut's tensors are passed exactly when its cin != cout";
            if (backward && (g_w[3 * i + j] != nullptr) != need) return "a weight gradient must be NULL exactly where its weight is";
            wi.push_back({p, bytes[j], true});
            if (backward) wo.push_back({g_w[3 * i + j], bytes[j], true});
        }
    }
    ins.insert(ins.begin(), wi.begin(), wi.end());
    outs.insert(outs.begin(), wo.begin(), wo.end());
    return nullptr;
}

// ... of every block of the trunk s
inline const char *weights_refused(const pmp_trunk_shape &s, const float *const *w, float *const *g_w, bool backward, std::vector<Span> &ins,
                                   std::vector<Span> &outs)
{
    BlockShape blocks[PMP_TRUNK_MAX_BLOCKS];
    for (int i = 0; i < s.nblocks; ++i) blocks[i] = block_shape(s, i);
    return weights_refused(blocks, s.nblocks, w, g_w, backward, ins, outs);
}

// Every tensor that is not optional present, no output over an input or another output and, for device pointers, every one aligned.
// -> why the call is refused, or NULL
inline const char *spans_refused(const std::vector<Span> &ins, const std::vector<Span> &outs, bool device)
{
    for (const std::vector<Span> *v : {&ins, &outs})
        for (const Span &t : *v)
            if (!t.p && !t.optional) return "null tensor";
    for (size_t i = 0; i < outs.size(); ++i) {
        for (const Span &in : ins)
            if (overlaps(outs[i], in)) return "an output tensor overlaps an input";
        for (size_t j = 0; j < i; ++j)
            if (overlaps(outs[i], outs[j])) return "two output tensors overlap";
    }
    for (const std::vector<Span> *v : {&ins, &outs})
        for (const Span &t : *v)
            if (device && ((uintptr_t)t.p & (t.align - 1))) return "every tensor must be 4-byte aligned, d_saved 16-byte";
    return nullptr;
}

// ---- a stem (pmp_stem_*): the shape rule, the sizes of its three convolutions and the rule on its pointer arrays
constexpr const char *STEM_SHAPE_RULE =
    "null or unsupported shape (n 1..256, h and w multiples of 16 in 16..256, cin 1..4, k 5 or 9, split 0 or 1)";

inline bool stem_shape_ok(const pmp_stem_shape *s)
{
    auto side = [](int v) { return v >= 16 && v <= 256 && !(v & 15); };
    return s && s->n >= 1 && s->n <= 256 && side(s->h) && side(s->w) && s->cin >= 1 && s->cin <= 4 && (s->k == 5 || s->k == 9) &&
           (s->split == 0 || s->split == 1);
}

// bytes of x and g_x [n][cin][h + p][w + p], of y and g_y [n][32][h][w], and of w[j] and b[j] (0 for the entries a QT stem lacks)
struct StemSizes {
    size_t x, y, w[3], b[3];
    explicit StemSizes(const pmp_stem_shape &s)
    {
        const size_t p = s.k / 2, k = s.k, c = s.cin;
        x = (size_t)s.n * c * (s.h + p) * (s.w + p) * 4;
        y = (size_t)s.n * 32 * s.h * s.w * 4;
        const size_t ws[3] = {(s.split ? 16 : 32) * c * k * k, 8 * c * (p + 1) * k, 8 * c * k * (p + 1)}, bs[3] = {s.split ? 16u : 32u, 8, 8};
        for (int j = 0; j < 3; ++j) { w[j] = j && !s.split ? 0 : ws[j] * 4; b[j] = j && !s.split ? 0 : bs[j] * 4; }
    }
};

// One of a stem call's arrays of three pointers (d_w, d_b, d_g_w, d_g_b), its tensors appended to v.  -> why refused, or NULL
// (one copy for the call's four uses, not four inlined ones: the product library is held to a size)
__attribute__((noinline)) inline const char *stem_array_refused(const pmp_stem_shape &s, const float *const *arr, const size_t bytes[3], std::vector<Span> &v)
{
    if (!arr || !arr[0]) return "null tensor";
    for (int j = 1; j < 3; ++j)
        if ((arr[j] != nullptr) != (s.split == 1)) return "entries 1 and 2 of a stem's pointer arrays are passed exactly when split = 1";
    for (int j = 0; j < (s.split ? 3 : 1); ++j) v.push_back({arr[j], bytes[j]});
    return nullptr;
}

// ---- a head (pmp_head_*): the shape rule, its sizes, and which of its tensors go with an attention input
constexpr const char *HEAD_SHAPE_RULE =
    "null or unsupported shape (n 1..256, h and w multiples of 8 in 8..256, cin 1..16, cout 1 or 2, (up_q, up_y) (0,0), (2,1) or (4,2))";

inline bool head_shape_ok(const pmp_head_shape *s)
{
    auto side = [](int v) { return v >= 8 && v <= 256 && !(v & 7); };
    return s && s->n >= 1 && s->n <= 256 && side(s->h) && side(s->w) && s->cin >= 1 && s->cin <= 16 && (s->cout == 1 || s->cout == 2) &&
           ((s->up_q == 0 && s->up_y == 0) || (s->up_q == 2 && s->up_y == 1) || (s->up_q == 4 && s->up_y == 2));
}

// bytes of x and g_x [n][cin][h][w], of y, prev, g_y and g_prev [n][cout][h][w], of w [cout][cin][3][3] and b [cout], and with an
// attention input of att and g_att [n][1+cout][up_y h][up_y w] and of q and g_q [n][1][up_y h / up_q][up_y w / up_q] (0 without)
struct HeadSizes {
    size_t x, y, w, b, att, q;
    explicit HeadSizes(const pmp_head_shape &s)
    {
        const size_t px = (size_t)s.n * s.h * s.w * 4, u = s.up_y;
        x = px * s.cin;
        y = px * s.cout;
        w = (size_t)4 * 9 * s.cout * s.cin;
        b = (size_t)4 * s.cout;
        att = px * u * u * (1 + s.cout);
        q = u ? px * u * u / ((size_t)s.up_q * s.up_q) : 0;
    }
};

// The tensors of a head call that exist exactly when the head has an attention input (forward: q, att; backward: g_att), and g_q,
// which may be asked for only then.  -> why refused, or NULL  (out of line, one copy for both directions)
__attribute__((noinline)) inline const char *head_att_refused(const pmp_head_shape &s, std::initializer_list<const void *> tied, const void *g_q)
{
    for (const void *p : tied)
        if ((p != nullptr) != (s.up_y != 0)) return "q, att and g_att are passed exactly when up_y != 0";
    if (g_q && !s.up_y) return "g_q may be asked for only with g_att";
    return nullptr;
}

// ---- a QT net's tail (pmp_qtail_*): resblock_q3, the multi-scale pool, resblock_q4, resblock_q5 + max_pool2d, resblock_q6
constexpr const char *QTAIL_SHAPE_RULE = "null or unsupported shape (n 1..256, h and w multiples of 16 in 16..256)";

inline bool qtail_shape_ok(const pmp_qtail_shape *s)
{
    auto side = [](int v) { return v >= 16 && v <= 256 && !(v & 15); };
    return s && s->n >= 1 && s->n <= 256 && side(s->h) && side(s->w);
}

constexpr int QTAIL_BLOCKS = 4, QTAIL_SAVED = 9;
inline BlockShape qtail_block(int i) { return BlockShape{i == 0 ? 64 : i == 1 ? 128 : 32, i == 3 ? 8 : 32, 3}; }

// d_saved: blocked x4, then t and out of q3, q4, q5 at h x w, then t and out of q6: its h/2 x w/2 map lies top-left in a map of
// h2 x w2, the sides rounded up to 16, whose other pixels are zero (the convolution kernels work on 16x16 tiles).  x6 is not saved.
struct QtailLayout {
    int h2, w2;
    int c[QTAIL_SAVED];                          // the real channels of saved tensor 0 .. 8 (pmp_qtail_unpack_device's index)
    size_t off[QTAIL_SAVED + 1];                 // bytes; off[9] = the size
    size_t x4, x9;                               // bytes of the dense x4 / g_x4 and x9 / g_x9
    explicit QtailLayout(const pmp_qtail_shape &s) : h2((s.h / 2 + 15) & ~15), w2((s.w / 2 + 15) & ~15)
    {
        const size_t px = (size_t)s.n * s.h * s.w * sizeof(float), px2 = (size_t)s.n * h2 * w2 * sizeof(float);
        off[0] = 0;
        for (int i = 0; i < QTAIL_SAVED; ++i) {
            c[i] = i == 0 ? 64 : i < 7 ? 32 : 8;
            off[i + 1] = off[i] + (i < 7 ? px : px2) * pad_channels(c[i]);
        }
        x4 = px * 64;
        x9 = px / 4 * 8;
    }
    size_t dense_bytes(int i) const { return i < 7 ? x4 / 64 * c[i] : x9; }
};

// ---- the gate (pmp_gate_*)
constexpr const char *GATE_COUNT_RULE = "count must be in 1 .. 2^31 - 1";

inline bool gate_count_ok(int64_t count) { return count >= 1 && count <= INT32_MAX; }

}  // namespace pmp
