// train_check.h — what pmp_resblock_*, pmp_trunk_*, pmp_qtail_*, pmp_stem_*, pmp_head_* and pmp_gate_* (api_train.cpp) accept, whole:
// the shape rules, a chain's blocks and its d_saved layout (SavedLayout: a trunk's and a QT tail's), a stem's and a head's sizes, the
// rules on a call's tensors, and per call family ONE function that states everything the call is refused for (rb_refused,
// chain_refused, stem_refused, head_refused, gate_refused): which tensors the call has, which are optional, which need 16 bytes.
// Likewise a step's ends (gather_refused, adam_refused), the divergence guard (guard_refused, adam_guarded_refused), the gradient buckets (grad_pack_refused, grad_sum_refused) and data set assembly (api_dataset.cpp: select_refused, rows_gather_refused).
// A single block is checked as the one-block trunk it is.  Pure host code without the HIP runtime, no pointer is dereferenced, so
// that it also builds, with a main of its own, for the CPU under a sanitizer (train_check_main.cpp, `make traincheck`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <utility>
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

// d_saved of a chain of blocks (a trunk, a QT net's tail): nt blocked tensors, each [n][pad_channels(c)/16][rows][cols][16] on the map
// h x w or, the tail's last two, on h2 x w2: h/2 x w/2 top-left in a map of whole 16x16 tiles (the kernels' unit) whose other pixels are 0
constexpr int SAVED_MAX = 2 * PMP_TRUNK_MAX_BLOCKS + 1;
struct SavedLayout {
    int nt = 0, n, h, w, h2, w2;
    int c[SAVED_MAX];                            // the real channels of saved tensor 0 .. nt-1 (pmp_*_unpack_device's index)
    bool half[SAVED_MAX];                        // on h2 x w2; dense [n][c][h/2][w/2]
    size_t off[SAVED_MAX + 1];                   // bytes; off[nt] = the size
    SavedLayout(int n = 0, int h = 0, int w = 0) : n(n), h(h), w(w), h2((h / 2 + 15) & ~15), w2((w / 2 + 15) & ~15) { off[0] = 0; }
    void add(int ch, bool on_half = false)
    {
        c[nt] = ch;
        half[nt] = on_half;
        off[nt + 1] = off[nt] + (size_t)n * (on_half ? h2 * w2 : h * w) * sizeof(float) * pad_channels(ch);
        ++nt;
    }
    size_t dense_bytes(int i) const { return (size_t)n * (half[i] ? (h / 2) * (w / 2) : h * w) * sizeof(float) * c[i]; }
};

// a trunk's: blocked x, then t_i and out_i of every block
inline SavedLayout saved_layout(const pmp_trunk_shape &s)
{
    SavedLayout lay(s.n, s.h, s.w);
    lay.add(s.cin);
    for (int i = 0; i < s.nblocks; ++i) { lay.add(s.cout[i]); lay.add(s.cout[i]); }
    return lay;
}

// A tensor of a call.  optional: may be NULL (a g_x that is not asked for, the shortcut's weights of a block that has none)
struct Span { const void *p; size_t bytes; bool optional = false; unsigned align = 4; };

inline bool overlaps(const Span &a, const Span &b)
{
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}

// The weights of the blocks, w0, w2, wsc per block as in pmp_trunk_*'s d_w and d_g_w (a single block's: three pointers), go IN
// FRONT of the call's other tensors in ins / outs (the gradients only backward).  -> why the call is refused, or NULL
// (out of line: one copy for a block's call and a chain's)
__attribute__((noinline)) inline const char *weights_refused(const BlockShape *blocks, int nblocks, const float *const *w, float *const *g_w,
                                                             bool backward, std::vector<Span> &ins, std::vector<Span> &outs)
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

// Every tensor that is not optional present, no output over an input or another output and, for device pointers, every one aligned.
// -> why the call is refused, or NULL  (out of line: every *_refused below ends in it)
__attribute__((noinline)) inline const char *spans_refused(const std::vector<Span> &ins, const std::vector<Span> &outs, bool device)
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

// ---- one block (pmp_resblock_*).  The tensors of a call, in the order of the context's staging buffers.  in: w0, w2, wsc, x and, backward,
// t, out, g_out;  out: t, out (forward) or g_w0, g_w2, g_wsc, g_x (backward): the weights in front, as a one-block trunk's d_w and d_g_w
struct RbCall {
    enum { X = 3, T, OUT, G_OUT, T_O = 0, OUT_O, G_X = 3 };
    bool backward;
    const float *in[7];
    float *out[4];
};

// -> why the call is refused, or NULL; ins and outs: its tensors, which the host forms stage one by one
inline const char *rb_refused(const pmp_rb_shape *rs, const RbCall &q, bool device, std::vector<Span> &ins, std::vector<Span> &outs)
{
    const pmp_trunk_shape s = rs ? one_block(*rs) : pmp_trunk_shape{};
    if (!train_shape_ok(&s)) return TRAIN_SHAPE_RULE;
    const size_t px = (size_t)s.n * s.h * s.w * 4, bx = px * s.cin, by = px * s.cout[0];
    ins = {{q.in[q.X], bx}};
    outs = {{q.out[q.T_O], by}, {q.out[q.OUT_O], by}};
    if (q.backward) {
        ins.insert(ins.end(), {{q.in[q.T], by}, {q.in[q.OUT], by}, {q.in[q.G_OUT], by}});
        outs = {{q.out[q.G_X], bx, true}};
    }
    const BlockShape b = block_shape(s, 0);
    const char *why = weights_refused(&b, 1, q.in, q.out, q.backward, ins, outs);
    return why ? why : spans_refused(ins, outs, device);
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

// The tensors of a stem call.  forward: x, w, b -> y_out;  backward: x, y, w, g_y -> g_x (optional), g_w, g_b
struct StemPtrs {
    const float *x, *y, *g_y;
    const float *const *w, *const *b;
    float *y_out, *g_x;
    float *const *g_w, *const *g_b;
};

// -> why the call is refused, or NULL
inline const char *stem_refused(const pmp_stem_shape *s, const StemPtrs &q, bool backward)
{
    if (!stem_shape_ok(s)) return STEM_SHAPE_RULE;
    const StemSizes z(*s);
    std::vector<Span> ins = {{q.x, z.x}}, outs;
    if (backward) ins.insert(ins.end(), {{q.y, z.y}, {q.g_y, z.y}});
    outs.push_back(backward ? Span{q.g_x, z.x, true} : Span{q.y_out, z.y});
    const char *why = stem_array_refused(*s, q.w, z.w, ins);
    if (!why && !backward) why = stem_array_refused(*s, q.b, z.b, ins);
    if (!why && backward) why = stem_array_refused(*s, q.g_w, z.w, outs);
    if (!why && backward) why = stem_array_refused(*s, q.g_b, z.b, outs);
    return why ? why : spans_refused(ins, outs, true);
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

// The tensors of a head call.  forward: x, w, b, prev?, q? -> y, att?;  backward: x, w, g_y, g_att? -> g_w, g_b, g_x?, g_q?, g_prev?  (?: optional)
struct HeadPtrs {
    const float *x, *w, *b, *prev, *q;
    float *y, *att;
    const float *g_y, *g_att;
    float *g_x, *g_w, *g_b, *g_q, *g_prev;
};

// -> why the call is refused, or NULL
inline const char *head_refused(const pmp_head_shape *s, const HeadPtrs &t, bool backward)
{
    if (!head_shape_ok(s)) return HEAD_SHAPE_RULE;
    const HeadSizes z(*s);
    std::vector<Span> ins = {{t.x, z.x}, {t.w, z.w}}, outs;
    const char *why;
    if (!backward) {
        why = head_att_refused(*s, {t.q, t.att}, nullptr);
        ins.insert(ins.end(), {{t.b, z.b}, {t.prev, z.y, true}, {t.q, z.q, true}});
        outs = {{t.y, z.y}, {t.att, z.att, true}};
    } else {
        why = head_att_refused(*s, {t.g_att}, t.g_q);
        ins.insert(ins.end(), {{t.g_y, z.y}, {t.g_att, z.att, true}});
        outs = {{t.g_x, z.x, true}, {t.g_w, z.w}, {t.g_b, z.b}, {t.g_q, z.q, true}, {t.g_prev, z.y, true}};
    }
    return why ? why : spans_refused(ins, outs, true);
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

// d_saved: blocked x4, then t and out of q3, q4, q5 at h x w, then t and out of q6 on its own map.  x6 is not saved.
inline SavedLayout saved_layout(const pmp_qtail_shape &s)
{
    SavedLayout lay(s.n, s.h, s.w);
    for (int i = 0; i < QTAIL_SAVED; ++i) lay.add(i == 0 ? 64 : i < 7 ? 32 : 8, i >= 7);
    return lay;
}

// ---- a chain of blocks whose activations stay blocked in the caller's d_saved (pmp_trunk_*, pmp_qtail_*): what tells one chain from
// another, and the tensors of a call.  forward: x, w -> saved, y;  backward: saved, w, g_y -> g_x (optional), g_w;  unpack: saved -> dense
struct Chain {
    const char *refused;                         // the shape rule where the shape breaks it (nothing else is set then), else NULL
    const char *index_rule, *unpack_name;        // unpack's message for an index outside 0 .. nt-1; how it names a failed launch
    SavedLayout lay;
    int nblocks, pool;
    BlockShape blocks[PMP_TRUNK_MAX_BLOCKS];
    size_t y_bytes;                              // of the dense y and g_y; x and g_x: lay.dense_bytes(0)
};

struct ChainPtrs {
    const float *x, *g_y;
    const float *const *w;
    const void *saved;
    float *y, *g_x, *dense;
    float *const *g_w;
};

inline Chain chain_of(const pmp_trunk_shape *s)
{
    Chain ch{};
    ch.index_rule = "index out of range (0 .. 2 * nblocks)";
    ch.unpack_name = "blocked_to_dense";
    if (!train_shape_ok(s)) { ch.refused = TRAIN_SHAPE_RULE; return ch; }
    ch.lay = saved_layout(*s);
    ch.nblocks = s->nblocks;
    ch.pool = s->pool;
    for (int i = 0; i < s->nblocks; ++i) ch.blocks[i] = block_shape(*s, i);
    ch.y_bytes = ch.lay.dense_bytes(ch.lay.nt - 1) / (s->pool ? 4 : 1);
    return ch;
}

inline Chain chain_of(const pmp_qtail_shape *s)
{
    Chain ch{};
    ch.index_rule = "index out of range (0 .. 8)";
    ch.unpack_name = "qtail_step";
    if (!qtail_shape_ok(s)) { ch.refused = QTAIL_SHAPE_RULE; return ch; }
    ch.lay = saved_layout(*s);
    ch.nblocks = QTAIL_BLOCKS;
    for (int i = 0; i < QTAIL_BLOCKS; ++i) ch.blocks[i] = qtail_block(i);
    ch.y_bytes = ch.lay.dense_bytes(QTAIL_SAVED - 1);
    return ch;
}

// forward (dir 0), backward (1) and unpack of saved tensor `index` (2)  -> why the call is refused, or NULL; ins and outs: its tensors
inline const char *chain_refused(const Chain &ch, const ChainPtrs &q, int dir, int index, std::vector<Span> &ins, std::vector<Span> &outs)
{
    if (ch.refused) return ch.refused;
    const SavedLayout &lay = ch.lay;
    if (dir == 2 && (index < 0 || index >= lay.nt)) return ch.index_rule;
    const Span saved{q.saved, lay.off[lay.nt], false, 16};
    const size_t x_bytes = lay.dense_bytes(0);
    if (dir == 0) { ins = {{q.x, x_bytes}}; outs = {saved, {q.y, ch.y_bytes}}; }
    if (dir == 1) { ins = {saved, {q.g_y, ch.y_bytes}}; outs = {{q.g_x, x_bytes, true}}; }
    if (dir == 2) { ins = {saved}; outs = {{q.dense, lay.dense_bytes(index)}}; }
    const char *why = dir == 2 ? nullptr : weights_refused(ch.blocks, ch.nblocks, q.w, q.g_w, dir == 1, ins, outs);
    return why ? why : spans_refused(ins, outs, true);
}

// ---- the gate (pmp_gate_*)
constexpr const char *GATE_COUNT_RULE = "count must be in 1 .. 2^31 - 1";

inline bool gate_count_ok(int64_t count) { return count >= 1 && count <= INT32_MAX; }

// forward: x, a -> o0 = y;  backward: x, a, g_y, g_acc (optional) -> o0 = g_x, o1 = g_a  -> why the call is refused, or NULL
inline const char *gate_refused(int64_t count, bool backward, const float *x, const float *a, const float *g_y, const float *g_acc,
                                const float *o0, const float *o1)
{
    if (backward && !g_y) return "null tensor";
    if (!gate_count_ok(count)) return GATE_COUNT_RULE;
    const size_t bytes = (size_t)count * 4;
    std::vector<Span> ins = {{x, bytes}, {a, bytes}}, outs = {{o0, bytes}};
    if (backward) {
        ins.insert(ins.end(), {{g_y, bytes}, {g_acc, bytes, true}});
        outs.push_back({o1, bytes});
    }
    return spans_refused(ins, outs, true);
}

// ---- a step's ends (pmp_batch_gather_device, pmp_adam_step_device)
inline const char *gather_refused(const pmp_batch_src *src, const int64_t *index, int64_t n, const pmp_batch_dst *dst, const int32_t *status)
{
    if (!src || !dst || !index || !status) return "null src, dst, d_index or d_status";
    if (src->count < 1) return "count must be >= 1";
    if (n < 1 || n > PMP_BATCH_MAX) return "n must be in 1 .. 65536";
    if (!src->y || (src->u != nullptr) != (src->v != nullptr)) return "y is required, u and v go together";
    if (!dst->x && !dst->qt_f && !dst->qt8 && !dst->msbt && !dst->msdire) return "no output asked for";
    if (((dst->qt_f || dst->qt8) && !src->qt8) || (dst->msbt && !src->msbt) || (dst->msdire && !src->msdire))
        return "an output whose source is NULL";
    const size_t N = (size_t)src->count, rows = (size_t)n, xrow = src->u ? 3468 * 4 : 4624 * 4;
    const std::vector<Span> ins = {{src->y, N * 4624},         {src->u, N * 1156, true},      {src->v, N * 1156, true}, {src->qt8, N * 64, true},
                                   {src->msbt, N * 768, true}, {src->msdire, N * 768, true}, {index, rows * 8, false, 8}};
    const std::vector<Span> outs = {{dst->x, rows * xrow, true},    {dst->qt_f, rows * 256, true},   {dst->qt8, rows * 64, true},
                                    {dst->msbt, rows * 768, true}, {dst->msdire, rows * 768, true}, {status, 4}};
    if (const char *why = spans_refused(ins, outs, false)) return why;
    for (const std::vector<Span> *v : {&ins, &outs})
        for (const Span &t : *v)
            if ((uintptr_t)t.p & (t.align - 1)) return "every pointer must be 4-byte aligned, d_index 8-byte";
    return nullptr;
}

inline const char *adam_refused(const pmp_adam_params *p, int ntensors, float *const *param, const float *const *grad, float *const *m,
                                float *const *v, const int64_t *count, int64_t step)
{
    if (!p || !param || !grad || !m || !v || !count) return "null params or array";
    if (ntensors < 1) return "ntensors must be >= 1";
    if (step < 1) return "step must be >= 1";
    if (!std::isfinite(p->lr) || !std::isfinite(p->beta1) || !std::isfinite(p->beta2) || !std::isfinite(p->eps)) return "lr, beta1, beta2 and eps must be finite";
    if (p->beta1 < 0 || p->beta1 >= 1 || p->beta2 < 0 || p->beta2 >= 1) return "beta1 and beta2 must be in [0, 1)";
    if (p->eps <= 0) return "eps must be > 0";
    std::vector<std::pair<uintptr_t, uintptr_t>> at;        // [first byte, behind the last) of all 4 ntensors tensors
    for (int i = 0; i < ntensors; ++i) {
        if (count[i] < 1) return "every count must be >= 1";
        for (const float *t : {(const float *)param[i], grad[i], (const float *)m[i], (const float *)v[i]}) {
            if (!t) return "null tensor";
            if ((uintptr_t)t & 3) return "every tensor must be 4-byte aligned";
            at.push_back({(uintptr_t)t, (uintptr_t)t + (uintptr_t)count[i] * 4});
        }
    }
    std::sort(at.begin(), at.end());
    for (size_t i = 1; i < at.size(); ++i)
        if (at[i].first < at[i - 1].second) return "two tensors of the call overlap";
    return nullptr;
}

// ---- the divergence guard (pmp_grad_guard_scratch_bytes, pmp_grad_guard_device, pmp_adam_step_guarded_device)
constexpr int64_t GUARD_TILE_ELEMS = 4096;

// the tiles of the table, or -1 for a bad one
inline int64_t guard_tiles(int ntensors, const int64_t *count)
{
    if (ntensors < 1 || !count) return -1;
    int64_t tiles = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (count[i] < 1 || count[i] >= ((int64_t)1 << 30)) return -1;
        tiles += (count[i] + GUARD_TILE_ELEMS - 1) / GUARD_TILE_ELEMS;
    }
    return tiles;
}

// 16 bytes a tile: its partial sum and its count of non-finite elements
inline int64_t guard_scratch_bytes(int ntensors, const int64_t *count)
{
    const int64_t tiles = guard_tiles(ntensors, count);
    return tiles < 0 ? -1 : 16 * tiles;
}

inline const char *guard_refused(const pmp_guard_params *p, int ntensors, const float *const *grad, const int64_t *count, const void *scratch,
                                 const pmp_guard_record *record, const pmp_guard_state *state)
{
    if (!p || !grad || !count || !scratch || !record) return "null params, array, d_scratch or d_record";
    const int64_t bytes = guard_scratch_bytes(ntensors, count);
    if (bytes < 0) return "ntensors must be >= 1 and every count in 1 .. 2^30 - 1";
    if (!std::isfinite(p->max_norm) || p->max_norm < 0) return "max_norm must be finite and >= 0";
    if (((uintptr_t)scratch | (uintptr_t)record | (uintptr_t)state) & 7) return "d_scratch, d_record and d_state must be 8-byte aligned";
    const Span own[3] = {{scratch, (size_t)bytes}, {record, sizeof(pmp_guard_record)}, {state, sizeof(pmp_guard_state)}};
    if (overlaps(own[0], own[1]) || overlaps(own[0], own[2]) || overlaps(own[1], own[2])) return "d_scratch, d_record and d_state overlap";
    for (int i = 0; i < ntensors; ++i) {
        if (!grad[i]) return "null tensor";
        if ((uintptr_t)grad[i] & 3) return "every gradient must be 4-byte aligned";
        for (const Span &o : own)
            if (overlaps(o, Span{grad[i], (size_t)count[i] * 4})) return "d_scratch, d_record or d_state overlaps a gradient";
    }
    return nullptr;
}

inline const char *adam_guarded_refused(const pmp_adam_params *p, int ntensors, float *const *param, const float *const *grad, float *const *m,
                                        float *const *v, const int64_t *count, int64_t step, const pmp_guard_record *record)
{
    if (const char *why = adam_refused(p, ntensors, param, grad, m, v, count, step)) return why;
    if (!record) return "null d_record";
    if ((uintptr_t)record & 7) return "d_record must be 8-byte aligned";
    const Span rec{record, sizeof(pmp_guard_record)};
    for (int i = 0; i < ntensors; ++i)
        for (const float *t : {(const float *)param[i], grad[i], (const float *)m[i], (const float *)v[i]})
            if (overlaps(rec, Span{t, (size_t)count[i] * 4})) return "d_record overlaps a tensor of the call";
    return nullptr;
}

// ---- gradient buckets (pmp_grad_bucket_floats, pmp_grad_pack_device, pmp_grad_sum_device)
// tensor i at offset[i] floats, a multiple of 4  -> the bucket's floats, or -1 for a bad table
inline int64_t grad_bucket_floats(int ntensors, const int64_t *count, int64_t *offset)
{
    if (ntensors < 1 || !count) return -1;
    int64_t at = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (count[i] < 1 || count[i] >= ((int64_t)1 << 30)) return -1;
        if (offset) offset[i] = at;
        at += (count[i] + 3) & ~(int64_t)3;
    }
    return at;
}

inline const char *grad_pack_refused(int ntensors, const float *const *grad, const int64_t *count, const float *bucket)
{
    if (!grad || !count || !bucket) return "null array or bucket";
    const int64_t total = grad_bucket_floats(ntensors, count, nullptr);
    if (total < 0) return "ntensors must be >= 1 and every count in 1 .. 2^30 - 1";
    if ((uintptr_t)bucket & 15) return "the bucket must be 16-byte aligned";
    const Span out{bucket, (size_t)total * 4};
    for (int i = 0; i < ntensors; ++i) {
        if ((uintptr_t)grad[i] & 3) return "every gradient must be 4-byte aligned";
        if (overlaps(out, Span{grad[i], (size_t)count[i] * 4})) return "a gradient overlaps the bucket";
    }
    return nullptr;
}

inline const char *grad_sum_refused(int nsrc, const float *const *src, int64_t count, const float *dst)
{
    if (nsrc < 1 || nsrc > PMP_GRAD_SUM_MAX) return "nsrc must be in 1 .. 64";
    if (!src || !dst) return "null array or d_dst";
    if (count < 4 || (count & 3)) return "count must be a multiple of 4, at least 4";
    if ((uintptr_t)dst & 15) return "every pointer must be 16-byte aligned";
    const Span out{dst, (size_t)count * 4};
    for (int j = 0; j < nsrc; ++j) {
        if (!src[j]) return "null source";
        if ((uintptr_t)src[j] & 15) return "every pointer must be 16-byte aligned";
        if (!(j == 0 && src[0] == dst) && overlaps(out, Span{src[j], (size_t)count * 4})) return "d_dst overlaps a source that is not d_src[0] itself";
    }
    return nullptr;
}

// ---- data set assembly (pmp_select_rows_device, pmp_gather_rows_device).  What d_seg_end holds is the device's to read, not the host's
constexpr int64_t ROWS_MAX = (int64_t)1 << 30;

// spans_refused with these calls' alignment rule in its message
inline const char *rows_spans_refused(const std::vector<Span> &ins, const std::vector<Span> &outs)
{
    const char *why = spans_refused(ins, outs, true);
    return why && strstr(why, "aligned") ? "d_seg_end, d_index and d_count must be 8-byte aligned, d_src, d_dst and d_status 4-byte" : why;
}

inline const char *select_refused(const uint8_t *const *flags, int nflags, int mask, const int64_t *seg_end, int nseg, int64_t cap, int64_t n,
                                  const int64_t *index, const int64_t *count)
{
    if (n < 1 || n > ROWS_MAX) return "n must be in 1 .. 2^30";
    if (nseg < 1 || nseg > 65536) return "nseg must be in 1 .. 65536";
    if (nflags < 0 || nflags > PMP_SELECT_MAX_FLAGS) return "nflags must be in 0 .. 64";
    if (mask < 1 || mask > 255) return "mask must be in 1 .. 255";
    if (cap < 0) return "cap must be >= 0";
    if (nflags > 0 && !flags) return "null d_flags";
    std::vector<Span> ins = {{seg_end, (size_t)nseg * 8, false, 8}};
    for (int k = 0; k < nflags; ++k) ins.push_back({flags[k], (size_t)n, false, 1});
    return rows_spans_refused(ins, {{index, (size_t)n * 8, false, 8}, {count, ((size_t)nseg + 1) * 8, false, 8}});
}

inline const char *rows_gather_refused(const void *src, int64_t nsrc, int64_t row_bytes, const int64_t *index, int64_t m, const void *dst,
                                       const int32_t *status)
{
    if (nsrc < 1) return "nsrc must be >= 1";
    if (m < 1 || m > ROWS_MAX) return "m must be in 1 .. 2^30";
    if (row_bytes < 4 || row_bytes > 65536 || (row_bytes & 3)) return "row_bytes must be a multiple of 4 in 4 .. 65536";
    return rows_spans_refused({{src, (size_t)nsrc * (size_t)row_bytes}, {index, (size_t)m * 8, false, 8}},
                              {{dst, (size_t)m * (size_t)row_bytes}, {status, 4}});
}

}  // namespace pmp
