// train_check_main.cpp — train_check.h on the CPU, with a main of its own, for `make traincheck` (-fsanitize=address,undefined): the
// shapes of the refusal matrices of tests/test_gpu_resblock_grad.py and tests/test_gpu_trunk_grad.py, the weight rule per block, and
// spans that overlap, are missing or are misaligned, a stem's shapes, sizes and pointer arrays (tests/test_gpu_stem_grad.py), a
// head's shapes, sizes and the tensors tied to its attention input (tests/test_gpu_head_grad.py), a QT tail's (tests/
// test_gpu_qtail_grad.py), and the pointer-level rows of those matrices through the functions the entry points call: chain_refused,
// rb_refused, stem_refused, head_refused and gate_refused on fake addresses, and those of data set assembly (tests/
// test_gpu_dataset.py) through select_refused and rows_gather_refused, and the gradient buckets' layout and refusals (tests/
// test_gpu_grad_bucket.py) through grad_bucket_floats, grad_pack_refused and grad_sum_refused, and the divergence guard's (tests/
// test_gpu_grad_guard.py) through guard_scratch_bytes, guard_refused and adam_guarded_refused.  No pointer is dereferenced; exit status 0 and
// "train_check: ok" when all hold.
#include <stdio.h>
#include <string.h>

#include "train_check.h"

using namespace pmp;

static int failures = 0;

static void expect(bool ok, const char *what)
{
    if (!ok) { ++failures; fprintf(stderr, "train_check: FAILED: %s\n", what); }
}

static bool says(const char *why, const char *word) { return why && strstr(why, word); }

// the weight rule over every block of the trunk s
static const char *weights_refused(const pmp_trunk_shape &s, const float *const *w, float *const *g_w, bool backward, std::vector<Span> &ins,
                                   std::vector<Span> &outs)
{
    return weights_refused(chain_of(&s).blocks, s.nblocks, w, g_w, backward, ins, outs);
}

// the arrays of the data set assembly calls below stand at file scope: they are the default arguments of its lambdas
static uint8_t ds_flag[3][304] __attribute__((aligned(16)));
static int64_t ds_seg[3], ds_index[300], ds_count[4];
static uint8_t ds_src[300 * 68 + 16] __attribute__((aligned(16))), ds_dst[300 * 68 + 16] __attribute__((aligned(16)));
static int32_t ds_status;

int main()
{
    // ---- shapes: a single block as a one-block trunk
    const int n = 2, h = 16, w = 16, ci = 16, co = 16, k = 3;
    const pmp_rb_shape bad[] = {{0, h, w, ci, co, k}, {257, h, w, ci, co, k}, {n, 8, w, ci, co, k}, {n, 24, w, ci, co, k}, {n, 272, w, ci, co, k},
                                {n, h, 0, ci, co, k}, {n, h, 40, ci, co, k}, {n, h, 272, ci, co, k}, {n, h, w, 0, co, k}, {n, h, w, 65, co, k},
                                {n, h, w, ci, 0, k}, {n, h, w, ci, 65, k}, {n, h, w, ci, co, 1}, {n, h, w, ci, co, 4}, {n, h, w, ci, co, 7},
                                {-1, h, w, ci, co, k}, {n, -16, w, ci, co, k}, {n, h, w, ci, co, -3}};
    for (const pmp_rb_shape &s : bad) {
        const pmp_trunk_shape t = one_block(s);
        expect(!train_shape_ok(&t), "a shape of the refusal matrix is refused");
    }
    const pmp_rb_shape good[] = {{n, h, w, ci, co, k}, {1, 16, 16, 1, 1, 3}, {256, 256, 256, 64, 64, 5}, {3, 32, 48, 17, 33, 5}};
    for (const pmp_rb_shape &s : good) {
        const pmp_trunk_shape t = one_block(s);
        expect(train_shape_ok(&t) && t.nblocks == 1 && t.pool == 0 && block_shape(t, 0).cin == s.cin && block_shape(t, 0).cout == s.cout &&
                   block_shape(t, 0).k == s.k,
               "an accepted shape is a one-block trunk");
    }
    // ---- shapes: trunks
    pmp_trunk_shape m1{200, 64, 64, 32, 6, {64, 64, 64, 64, 64, 64}, {5, 3, 3, 3, 3, 3}, 1};
    expect(train_shape_ok(&m1), "trunk_M1's shape");
    expect(!train_shape_ok(nullptr), "a null shape");
    for (int v : {0, -1, PMP_TRUNK_MAX_BLOCKS + 1}) { pmp_trunk_shape t = m1; t.nblocks = v; expect(!train_shape_ok(&t), "nblocks out of range"); }
    for (int v : {-1, 2}) { pmp_trunk_shape t = m1; t.pool = v; expect(!train_shape_ok(&t), "pool out of range"); }
    { pmp_trunk_shape t = m1; t.cout[5] = 65; expect(!train_shape_ok(&t), "a late block's channels"); }
    { pmp_trunk_shape t = m1; t.k[3] = 4; expect(!train_shape_ok(&t), "a late block's k"); }
    { pmp_trunk_shape t = m1; t.cout[7] = 1000; t.k[7] = 9; expect(train_shape_ok(&t), "entries behind nblocks are not read"); }
    // ---- d_saved of the largest trunk: 17 tensors, offsets that add up, every one a multiple of 16 bytes
    pmp_trunk_shape big{256, 256, 256, 64, 8, {64, 33, 17, 1, 64, 16, 32, 48}, {3, 5, 3, 5, 3, 5, 3, 5}, 0};
    expect(train_shape_ok(&big), "the largest trunk");
    const SavedLayout lay = saved_layout(big);
    size_t sum = 0;
    for (int i = 0; i < lay.nt; ++i) {
        expect(lay.off[i] == sum && !(lay.off[i] & 15), "d_saved offsets");
        sum += (size_t)256 * 256 * 256 * 4 * pad_channels(lay.c[i]);
    }
    expect(lay.nt == 17 && lay.off[17] == sum && lay.c[0] == 64 && lay.c[1] == 64 && lay.c[2] == 64 && lay.c[3] == 33 && lay.c[16] == 48, "d_saved layout");
    expect(block_shape(big, 0).cin == 64 && block_shape(big, 1).cin == 64 && block_shape(big, 7).cin == 32 && block_shape(big, 7).cout == 48, "block_shape");
    // ---- the weights of every block
    alignas(16) static float mem[16 * 2560 + 1024 * 1024];                      // 2560 floats apart: the largest tensor here has 9 * 16 * 16;
                                                                               // behind them, room for the whole calls further down (place())
    auto at = [&](int i) { return mem + i * 2560; };
    const pmp_trunk_shape two{n, h, w, 16, 2, {16, 8}, {3, 3}, 0};             // block 0 identity, block 1 with a 1x1 shortcut
    const float *wt[6] = {at(0), at(1), nullptr, at(2), at(3), at(4)};
    float *gw[6] = {at(5), at(6), nullptr, at(7), at(8), at(9)};
    std::vector<Span> ins = {{at(10), 64}}, outs = {{at(11), 64}};
    expect(!weights_refused(two, wt, gw, true, ins, outs) && ins.size() == 7 && outs.size() == 7 && ins[6].p == at(10) && ins[0].p == mem &&
               outs[5].p == at(9) && ins[5].bytes == (size_t)4 * 8 * 16 && ins[4].bytes == (size_t)4 * 9 * 8 * 8 && ins[0].bytes == (size_t)4 * 9 * 256,
           "weights go in front, with their sizes");
    expect(!spans_refused(ins, outs, true), "the spans of an accepted call");
    std::vector<Span> a, b;
    expect(!weights_refused(two, wt, nullptr, false, a, b) && a.size() == 6 && b.empty(), "forward: no gradients");
    expect(says(weights_refused(two, nullptr, gw, true, a, b), "null") && says(weights_refused(two, wt, nullptr, true, a, b), "null"), "no weight array");
    for (int j : {0, 1, 3, 4}) {
        const float *v[6]; memcpy(v, wt, sizeof v); v[j] = nullptr;
        expect(says(weights_refused(two, v, gw, true, a, b), "null tensor"), "a missing w0 or w2");
    }
    { const float *v[6]; memcpy(v, wt, sizeof v); v[2] = at(12); expect(says(weights_refused(two, v, gw, true, a, b), "shortcut"), "wsc with an identity shortcut"); }
    { const float *v[6]; memcpy(v, wt, sizeof v); v[5] = nullptr; expect(says(weights_refused(two, v, gw, true, a, b), "shortcut"), "no wsc with a conv shortcut"); }
    for (int j = 0; j < 6; ++j) {
        float *v[6]; memcpy(v, gw, sizeof v); v[j] = v[j] ? nullptr : at(12);
        expect(says(weights_refused(two, wt, v, true, a, b), "NULL exactly"), "a gradient's NULL pattern differs from its weight's");
        expect(!weights_refused(two, wt, v, false, a, b), "... which forward does not look at");
    }
    expect(a.size() == 6 * 7 && b.empty(), "a refused call appends nothing");
    // ---- spans
    auto refused = [](std::vector<Span> i, std::vector<Span> o, bool device = true) { return spans_refused(i, o, device); };
    const Span x{mem, 256}, y{mem + 64, 256}, y2{mem + 128, 256};
    expect(!refused({x}, {y, y2}), "adjacent spans do not overlap");
    expect(says(refused({x}, {{mem + 63, 8}}), "overlaps an input"), "an output's first byte range in an input's last word");
    expect(says(refused({x}, {{mem, 4}}), "overlaps an input") && says(refused({{mem + 1, 4}}, {x}), "overlaps an input"), "containment both ways");
    expect(says(refused({x}, {y, {mem + 127, 256}}), "two output") && says(refused({x}, {y, y}), "two output"), "two outputs");
    expect(!refused({x, x}, {y}), "inputs may alias");
    expect(says(refused({{nullptr, 4}}, {y}), "null") && says(refused({x}, {{nullptr, 4}}), "null"), "a missing tensor");
    expect(!refused({x, {nullptr, 1 << 20, true}}, {y, {nullptr, 1 << 20, true}}), "an optional tensor may be NULL and overlaps nothing");
    expect(says(refused({{(char *)mem + 2, 16}}, {y}), "aligned") && says(refused({x}, {{(char *)(mem + 64) + 1, 16}}), "aligned"), "4-byte alignment");
    expect(!refused({{(char *)mem + 2, 16}}, {y}, false), "host pointers need no alignment");
    expect(says(refused({{mem + 1, 64, false, 16}}, {y}), "aligned") && !refused({{mem + 4, 64, false, 16}}, {y}), "d_saved's 16 bytes");
    // ---- a stem: the shapes of the refusal matrix of tests/test_gpu_stem_grad.py, the sizes, and the rule on the pointer arrays
    const pmp_stem_shape sbad[] = {{0, 16, 16, 1, 9, 0}, {257, 16, 16, 1, 9, 0}, {-1, 16, 16, 1, 9, 0}, {2, 8, 16, 1, 9, 0}, {2, 24, 16, 1, 9, 0},
                                   {2, 272, 16, 1, 9, 0}, {2, -16, 16, 1, 9, 0}, {2, 16, 0, 1, 9, 0}, {2, 16, 40, 1, 9, 0}, {2, 16, 272, 1, 9, 0},
                                   {2, 16, 16, 0, 9, 0}, {2, 16, 16, 5, 9, 0}, {2, 16, 16, -1, 9, 0}, {2, 16, 16, 1, 3, 0}, {2, 16, 16, 1, 7, 0},
                                   {2, 16, 16, 1, 4, 0}, {2, 16, 16, 1, 11, 0}, {2, 16, 16, 1, -9, 0}, {2, 16, 16, 1, 9, 2}, {2, 16, 16, 1, 9, -1}};
    for (const pmp_stem_shape &t : sbad) expect(!stem_shape_ok(&t), "a stem shape of the refusal matrix is refused");
    const pmp_stem_shape sgood[] = {{1, 16, 16, 1, 9, 0}, {200, 64, 64, 2, 9, 1}, {200, 32, 32, 3, 5, 0}, {200, 32, 32, 4, 5, 1}, {256, 256, 256, 4, 9, 1},
                                    {3, 48, 16, 2, 5, 1}};
    for (const pmp_stem_shape &t : sgood) expect(stem_shape_ok(&t), "an accepted stem shape");
    expect(!stem_shape_ok(nullptr), "a null stem shape");
    {
        const StemSizes q(pmp_stem_shape{2, 16, 32, 3, 5, 0}), m(pmp_stem_shape{3, 48, 16, 2, 9, 1});
        expect(q.x == (size_t)4 * 2 * 3 * 18 * 34 && q.y == (size_t)4 * 2 * 32 * 16 * 32 && q.w[0] == (size_t)4 * 32 * 3 * 25 && q.b[0] == 128 &&
                   !q.w[1] && !q.w[2] && !q.b[1] && !q.b[2],
               "the sizes of a QT stem");
        expect(m.x == (size_t)4 * 3 * 2 * 52 * 20 && m.y == (size_t)4 * 3 * 32 * 48 * 16 && m.w[0] == (size_t)4 * 16 * 2 * 81 &&
                   m.w[1] == (size_t)4 * 8 * 2 * 45 && m.w[2] == m.w[1] && m.b[0] == 64 && m.b[1] == 32 && m.b[2] == 32,
               "the sizes of an MTT stem");
        const pmp_stem_shape qs{2, 16, 32, 3, 5, 0}, ms{3, 48, 16, 2, 9, 1};
        const float *w1[3] = {at(0), nullptr, nullptr}, *w3[3] = {at(0), at(1), at(2)};
        float *g3[3] = {at(3), at(4), at(5)};
        std::vector<Span> v;
        expect(!stem_array_refused(qs, w1, q.w, v) && v.size() == 1 && v[0].p == at(0) && v[0].bytes == q.w[0], "a QT stem's array: one tensor");
        expect(!stem_array_refused(ms, w3, m.w, v) && v.size() == 4 && v[3].p == at(2) && v[3].bytes == m.w[2], "an MTT stem's array: three");
        expect(!stem_array_refused(ms, g3, m.b, v) && v.size() == 7 && v[4].bytes == 64, "an array of outputs");
        const size_t before = v.size();
        expect(says(stem_array_refused(qs, nullptr, q.w, v), "null"), "no array");
        { const float *u[3] = {nullptr, nullptr, nullptr}; expect(says(stem_array_refused(qs, u, q.w, v), "null"), "no entry 0"); }
        { const float *u[3] = {nullptr, at(1), at(2)}; expect(says(stem_array_refused(ms, u, m.w, v), "null"), "no entry 0, split"); }
        expect(says(stem_array_refused(qs, w3, q.w, v), "exactly when split"), "three tensors without split");
        expect(says(stem_array_refused(ms, w1, m.w, v), "exactly when split"), "one tensor with split");
        { const float *u[3] = {at(0), at(1), nullptr}; expect(says(stem_array_refused(ms, u, m.w, v), "exactly when split") && says(stem_array_refused(qs, u, q.w, v), "exactly when split"), "two tensors"); }
        { const float *u[3] = {at(0), nullptr, at(2)}; expect(says(stem_array_refused(ms, u, m.w, v), "exactly when split") && says(stem_array_refused(qs, u, q.w, v), "exactly when split"), "entries 0 and 2"); }
        expect(v.size() == before, "a refused array appends nothing");
    }
    // ---- a head: the shapes of the refusal matrix of tests/test_gpu_head_grad.py, the sizes, and the tensors tied to up_y
    const pmp_head_shape hbad[] = {{0, 16, 16, 8, 2, 0, 0}, {257, 16, 16, 8, 2, 0, 0}, {-1, 16, 16, 8, 2, 0, 0}, {2, 0, 16, 8, 2, 0, 0},
                                   {2, 4, 16, 8, 2, 0, 0}, {2, 12, 16, 8, 2, 0, 0}, {2, 264, 16, 8, 2, 0, 0}, {2, -8, 16, 8, 2, 0, 0},
                                   {2, 16, 0, 8, 2, 0, 0}, {2, 16, 20, 8, 2, 0, 0}, {2, 16, 264, 8, 2, 0, 0}, {2, 16, 16, 0, 2, 0, 0},
                                   {2, 16, 16, 17, 2, 0, 0}, {2, 16, 16, -1, 2, 0, 0}, {2, 16, 16, 8, 0, 0, 0}, {2, 16, 16, 8, 3, 0, 0},
                                   {2, 16, 16, 8, -1, 0, 0}, {2, 16, 16, 8, 2, 2, 2}, {2, 16, 16, 8, 2, 4, 1}, {2, 16, 16, 8, 2, 0, 1},
                                   {2, 16, 16, 8, 2, 2, 0}, {2, 16, 16, 8, 2, 1, 1}, {2, 16, 16, 8, 2, 8, 4}, {2, 16, 16, 8, 2, -2, -1}};
    for (const pmp_head_shape &t : hbad) expect(!head_shape_ok(&t), "a head shape of the refusal matrix is refused");
    const pmp_head_shape hgood[] = {{1, 8, 8, 8, 1, 0, 0}, {200, 16, 16, 8, 2, 2, 1}, {200, 16, 16, 8, 2, 4, 2}, {200, 16, 16, 8, 2, 0, 0},
                                    {256, 256, 256, 16, 2, 4, 2}, {3, 24, 16, 5, 1, 2, 1}, {1, 256, 8, 1, 2, 0, 0}};
    for (const pmp_head_shape &t : hgood) expect(head_shape_ok(&t), "an accepted head shape");
    expect(!head_shape_ok(nullptr), "a null head shape");
    {
        const pmp_head_shape plain{3, 24, 16, 5, 1, 0, 0}, a1{2, 16, 16, 8, 2, 2, 1}, a2{2, 16, 24, 8, 2, 4, 2};
        const HeadSizes p(plain), u(a1), v(a2);
        expect(p.x == (size_t)4 * 3 * 5 * 24 * 16 && p.y == (size_t)4 * 3 * 24 * 16 && p.w == (size_t)4 * 45 && p.b == 4 && !p.att && !p.q,
               "the sizes of a head without an attention input");
        expect(u.x == (size_t)4 * 2 * 8 * 256 && u.y == (size_t)4 * 2 * 2 * 256 && u.w == (size_t)4 * 144 && u.b == 8 &&
                   u.att == (size_t)4 * 2 * 3 * 256 && u.q == (size_t)4 * 2 * 64,
               "the sizes of conv_B1's head");
        expect(v.att == (size_t)4 * 2 * 3 * 32 * 48 && v.q == (size_t)4 * 2 * 8 * 12, "the sizes of conv_B2's head");
        expect(!head_att_refused(plain, {nullptr, nullptr}, nullptr) && !head_att_refused(a1, {at(0), at(1)}, nullptr) &&
                   !head_att_refused(a2, {at(0)}, at(1)) && !head_att_refused(a2, {at(0)}, nullptr),
               "the accepted patterns");
        expect(says(head_att_refused(plain, {at(0), nullptr}, nullptr), "exactly when up_y") &&
                   says(head_att_refused(plain, {nullptr, at(0)}, nullptr), "exactly when up_y") &&
                   says(head_att_refused(plain, {at(0)}, nullptr), "exactly when up_y"),
               "q, att or g_att without up_y");
        expect(says(head_att_refused(a1, {nullptr, at(0)}, nullptr), "exactly when up_y") &&
                   says(head_att_refused(a1, {at(0), nullptr}, nullptr), "exactly when up_y") && says(head_att_refused(a2, {nullptr}, nullptr), "exactly when up_y"),
               "up_y without q, att or g_att");
        expect(says(head_att_refused(plain, {nullptr}, at(0)), "only with g_att"), "g_q without g_att");
        // a backward call's spans: prev-like optional tensors may be absent, an output over an input is refused
        std::vector<Span> hi = {{at(0), u.x}, {at(4), u.w}, {at(5), u.y}, {at(6), u.att, true}};
        std::vector<Span> ho = {{nullptr, u.x, true}, {at(8), u.w}, {at(9), u.b}, {nullptr, u.q, true}, {nullptr, u.y, true}};
        expect(!spans_refused(hi, ho, true), "a head's backward call without its optional outputs");
        ho[0].p = at(5);
        expect(says(spans_refused(hi, ho, true), "overlaps an input"), "g_x over g_y");
        ho[0].p = nullptr; ho[1].p = nullptr;
        expect(says(spans_refused(hi, ho, true), "null"), "no g_w");
    }
    // ---- a QT net's tail: the shapes of the refusal matrix of tests/test_gpu_qtail_grad.py, d_saved, and the weight rule of its blocks
    const pmp_qtail_shape qbad[] = {{0, 16, 16}, {257, 16, 16}, {-1, 16, 16}, {2, 8, 16}, {2, 24, 16}, {2, 272, 16}, {2, -16, 16},
                                    {2, 16, 0}, {2, 16, 8}, {2, 16, 40}, {2, 16, 272}};
    for (const pmp_qtail_shape &t : qbad) expect(!qtail_shape_ok(&t), "a tail shape of the refusal matrix is refused");
    const pmp_qtail_shape qgood[] = {{1, 16, 16}, {200, 16, 16}, {3, 32, 16}, {2, 16, 48}, {256, 256, 256}};
    for (const pmp_qtail_shape &t : qgood) expect(qtail_shape_ok(&t), "an accepted tail shape");
    expect(!qtail_shape_ok(nullptr), "a null tail shape");
    {
        const pmp_qtail_shape s200{200, 16, 16}, swide{2, 16, 48}, sbig{256, 256, 256};
        const SavedLayout nets = saved_layout(s200), wide = saved_layout(swide), big = saved_layout(sbig);
        const size_t x4 = (size_t)4 * 200 * 64 * 256, x9 = (size_t)4 * 200 * 8 * 64;
        expect(nets.nt == QTAIL_SAVED && nets.h2 == 16 && nets.w2 == 16 && nets.off[QTAIL_SAVED] == (size_t)58982400 && nets.dense_bytes(0) == x4 &&
                   nets.dense_bytes(6) == x4 / 2 && nets.dense_bytes(7) == x9 && nets.dense_bytes(8) == x9 && chain_of(&s200).y_bytes == x9,
               "the tail's d_saved at the nets' shape");
        expect(wide.h2 == 16 && wide.w2 == 32 && wide.off[7] == (size_t)4 * 2 * 16 * 48 * 256 &&
                   wide.off[9] == wide.off[7] + (size_t)4 * 2 * 16 * 32 * 32 && wide.dense_bytes(8) == (size_t)4 * 2 * 8 * 8 * 24,
               "q6's map is rounded up to whole tiles");
        expect(big.h2 == 128 && big.w2 == 128, "a map of whole tiles is not padded");
        for (int i = 0; i <= QTAIL_SAVED; ++i) expect(!(big.off[i] & 15) && !(wide.off[i] & 15), "the tail's d_saved offsets");
        expect(big.c[0] == 64 && big.c[1] == 32 && big.c[6] == 32 && big.c[7] == 8 && big.c[8] == 8, "the tail's saved channels");
        BlockShape qb[QTAIL_BLOCKS];
        for (int i = 0; i < QTAIL_BLOCKS; ++i) qb[i] = qtail_block(i);
        expect(qb[0].cin == 64 && qb[1].cin == 128 && qb[1].cip() == 128 && qb[2].cin == 32 && qb[2].cout == 32 && qb[3].cout == 8 &&
                   qb[3].cop() == 16 && qb[1].k == 3,
               "the tail's blocks");
        const float *qw[12];
        float *qg[12];
        for (int j = 0; j < 12; ++j) { qw[j] = j == 8 ? nullptr : at(0); qg[j] = j == 8 ? nullptr : at(1); }
        std::vector<Span> qi, qo;
        expect(!weights_refused(qb, QTAIL_BLOCKS, qw, qg, true, qi, qo) && qi.size() == 12 && qo.size() == 12 &&
                   qi[3].bytes == (size_t)4 * 9 * 32 * 128 && qi[5].bytes == (size_t)4 * 32 * 128 && qi[11].bytes == (size_t)4 * 8 * 32,
               "the tail's weights, with their sizes");
        { const float *v[12]; memcpy(v, qw, sizeof v); v[8] = at(2); expect(says(weights_refused(qb, 4, v, qg, true, qi, qo), "shortcut"), "q5 with a wsc"); }
        { const float *v[12]; memcpy(v, qw, sizeof v); v[5] = nullptr; expect(says(weights_refused(qb, 4, v, qg, true, qi, qo), "shortcut"), "q4 without its wsc"); }
        { float *v[12]; memcpy(v, qg, sizeof v); v[8] = at(2); expect(says(weights_refused(qb, 4, qw, v, true, qi, qo), "NULL exactly"), "a g_wsc for q5"); }
        { float *v[12]; memcpy(v, qg, sizeof v); v[3] = nullptr; expect(says(weights_refused(qb, 4, qw, v, true, qi, qo), "NULL exactly"), "no g_w0 for q4"); }
        expect(says(weights_refused(qb, 4, nullptr, qg, true, qi, qo), "null") && says(weights_refused(qb, 4, qw, nullptr, true, qi, qo), "null"),
               "the tail without a weight array");
    }
    expect(gate_count_ok(1) && gate_count_ok(INT32_MAX) && !gate_count_ok(0) && !gate_count_ok(-5) && !gate_count_ok((int64_t)INT32_MAX + 1),
           "the gate's count");
    // ---- whole calls through the functions the entry points call, on fake addresses: the tensors of a call laid out one behind the
    // other in mem, behind the slots of at(), 64 bytes between them (a tensor moved by a few bytes is misaligned, not over its neighbour:
    // overlaps are looked at first)
    const size_t slots = 16 * 2560 * sizeof(float);
    size_t used = slots;
    auto place = [&](size_t bytes) {
        float *p = (float *)((char *)mem + used);
        used += ((bytes + 15) & ~(size_t)15) + 64;
        expect(used <= sizeof mem, "mem holds the call's tensors");
        return p;
    };
    auto off = [](const void *p, long bytes) { return (float *)((char *)const_cast<void *>(p) + bytes); };
    auto is = [](const char *why, const char *all) {
        const bool same = why && !strcmp(why, all);
        if (!same) fprintf(stderr, "train_check: \"%s\" where \"%s\" was expected\n", why ? why : "(accepted)", all);
        return same;
    };
    // a chain: forward (0), backward (1), unpack (2) of a trunk and of the tail
    std::vector<Span> c_in, c_out;
    auto chain_why = [&](const Chain &ch, const ChainPtrs &q, int dir, int index = 0) { return chain_refused(ch, q, dir, index, c_in, c_out); };
    auto chain_rows = [&](const Chain &ch, const Chain &null_shape, const char *index_rule) {
        used = slots;
        const SavedLayout &lay = ch.lay;
        const float *wt[3 * PMP_TRUNK_MAX_BLOCKS] = {};
        float *gw[3 * PMP_TRUNK_MAX_BLOCKS] = {};
        int conv_sc = -1, id_sc = -1;                                          // some wsc that exists / that does not
        for (int i = 0; i < ch.nblocks; ++i) {
            const BlockShape b = ch.blocks[i];
            const size_t kk = (size_t)4 * b.k * b.k, bytes[3] = {kk * b.cout * b.cin, kk * b.cout * b.cout, (size_t)4 * b.cout * b.cin};
            for (int j = 0; j < (b.cin != b.cout ? 3 : 2); ++j) { wt[3 * i + j] = place(bytes[j]); gw[3 * i + j] = place(bytes[j]); }
            (b.cin != b.cout ? conv_sc : id_sc) = 3 * i + 2;
        }
        size_t dense = 0;
        for (int i = 0; i < lay.nt; ++i) dense = lay.dense_bytes(i) > dense ? lay.dense_bytes(i) : dense;
        ChainPtrs ok{};
        ok.w = wt; ok.g_w = gw;
        ok.saved = place(lay.off[lay.nt]);
        ok.x = place(lay.dense_bytes(0)); ok.g_x = place(lay.dense_bytes(0));
        ok.y = place(ch.y_bytes); ok.g_y = place(ch.y_bytes);
        ok.dense = place(dense);
        float *spare = place(dense), *room = place(lay.off[lay.nt] + dense);
        for (int dir = 0; dir < 3; ++dir) {
            auto why = [&](const ChainPtrs &q, int index = 1) { return chain_why(ch, q, dir, index); };
            expect(!why(ok), "an accepted call of a chain");
            expect(says(chain_why(null_shape, ok, dir, 1), "null or unsupported shape"), "a chain's null shape");
            ChainPtrs q = ok;
            q.saved = nullptr; expect(is(why(q), "null tensor"), "null d_saved");
            expect(says(chain_why(null_shape, q, dir, 1), "null or unsupported shape"), "the shape is looked at first");
            for (int d : {4, 8}) { q.saved = off(ok.saved, d); expect(says(why(q), "d_saved 16-byte"), "d_saved at +4 and +8 bytes"); }
            q.saved = off(ok.saved, 16); expect(!why(q), "d_saved at +16 bytes");
            q = ok;
            (dir == 0 ? q.y : dir == 1 ? q.g_x : q.dense) = off(ok.saved, 256 << dir);
            expect(is(why(q), dir ? "an output tensor overlaps an input" : "two output tensors overlap"), "an output inside d_saved");
            q = ok; q.saved = room;
            (dir == 0 ? q.y : dir == 1 ? q.g_x : q.dense) = off(room, (long)lay.off[lay.nt]);
            expect(!why(q), "an output right behind d_saved");
            (dir == 0 ? q.y : dir == 1 ? q.g_x : q.dense) = off(room, (long)lay.off[lay.nt] - 4);
            expect(is(why(q), dir ? "an output tensor overlaps an input" : "two output tensors overlap"), "an output over d_saved's last word");
            q = ok;
            (dir == 0 ? q.y : dir == 1 ? q.g_x : q.dense) = nullptr;
            expect(dir == 1 ? !why(q) : is(why(q), "null tensor"), "only g_x is optional");
            if (dir == 2) continue;
            q = ok; q.w = nullptr; expect(is(why(q), "null tensor"), "null d_w");
            q = ok; (dir ? q.g_y : q.x) = nullptr; expect(is(why(q), "null tensor"), "null x, null g_y");
            q = ok; (dir ? q.g_y : q.x) = off(dir ? ok.g_y : ok.x, 2); expect(says(why(q), "aligned"), "misaligned x, g_y");
            const float *v[3 * PMP_TRUNK_MAX_BLOCKS];
            float *g[3 * PMP_TRUNK_MAX_BLOCKS];
            q = ok; q.w = v; q.g_w = g;
            auto fresh = [&] { memcpy(v, wt, sizeof v); memcpy(g, gw, sizeof g); };
            fresh(); v[1] = nullptr; g[1] = nullptr; expect(is(why(q), "null tensor"), "null w2 of block 0");
            fresh(); v[0] = off(wt[0], 2); expect(says(why(q), "aligned"), "misaligned w0");
            if (conv_sc >= 0) { fresh(); v[conv_sc] = nullptr; g[conv_sc] = nullptr; expect(says(why(q), "shortcut"), "no wsc with a conv shortcut"); }
            if (id_sc >= 0) {
                fresh(); v[id_sc] = spare; g[id_sc] = spare + 64; expect(says(why(q), "shortcut"), "wsc with an identity shortcut");
                q.y = off(ok.x, 64); q.g_x = const_cast<float *>(ok.g_y);
                expect(says(why(q), "shortcut"), "the weights' pattern is looked at before overlaps");
                q.y = ok.y; q.g_x = ok.g_x;
            }
        }
        ChainPtrs q = ok;
        q.y = off(ok.x, 64); expect(is(chain_why(ch, q, 0), "an output tensor overlaps an input"), "y overlaps x");
        q = ok; q.saved = ok.x; expect(is(chain_why(ch, q, 0), "an output tensor overlaps an input"), "d_saved is x");
        q = ok; q.saved = wt[1]; expect(is(chain_why(ch, q, 0), "an output tensor overlaps an input"), "d_saved overlaps w2");
        q = ok; q.g_w = nullptr; expect(!chain_why(ch, q, 0) && is(chain_why(ch, q, 1), "null tensor"), "d_g_w: backward only");
        q = ok; q.g_x = const_cast<float *>(ok.g_y); expect(is(chain_why(ch, q, 1), "an output tensor overlaps an input"), "g_x over g_y");
        float *g[3 * PMP_TRUNK_MAX_BLOCKS];
        q = ok; q.g_w = g;
        memcpy(g, gw, sizeof g); g[1] = gw[0]; expect(is(chain_why(ch, q, 1), "two output tensors overlap"), "g_w2 is g_w0");
        memcpy(g, gw, sizeof g); g[1] = off(wt[0], 4); expect(is(chain_why(ch, q, 1), "an output tensor overlaps an input"), "g_w2 overlaps w0");
        memcpy(g, gw, sizeof g); g[1] = off(ok.g_x, 16); expect(is(chain_why(ch, q, 1), "two output tensors overlap"), "g_w2 overlaps g_x");
        memcpy(g, gw, sizeof g); g[0] = nullptr; expect(says(chain_why(ch, q, 1), "NULL exactly"), "null g_w0");
        memcpy(g, gw, sizeof g); g[0] = off(gw[0], 2); expect(says(chain_why(ch, q, 1), "aligned"), "misaligned g_w0");
        // unpack: every index of the layout and no other, the tensors' sizes, and which one is written
        for (int i = 0; i < lay.nt; ++i) {
            std::vector<Span> in, out;
            expect(!chain_refused(ch, ok, 2, i, in, out) && in.size() == 1 && out.size() == 1 && in[0].p == ok.saved && in[0].bytes == lay.off[lay.nt] &&
                       in[0].align == 16 && out[0].p == ok.dense && out[0].bytes == lay.dense_bytes(i) && !out[0].optional,
                   "unpack reads d_saved and writes the dense tensor of that index");
        }
        for (int i : {-1, lay.nt, lay.nt + 1, 1 << 30}) expect(is(chain_why(ch, ok, 2, i), index_rule), "an index outside 0 .. nt-1");
        q = ok; q.saved = nullptr; expect(is(chain_why(ch, q, 2, lay.nt), index_rule), "the index is looked at before the tensors");
        q = ok; q.dense = off(ok.dense, 2); expect(says(chain_why(ch, q, 2, 1), "aligned"), "misaligned dense");
        std::vector<Span> in, out;
        expect(!chain_refused(ch, ok, 0, 0, in, out) && in.size() == (size_t)3 * ch.nblocks + 1 && out.size() == 2 && in.back().p == ok.x &&
                   in.back().bytes == lay.dense_bytes(0) && out[0].p == ok.saved && out[0].align == 16 && out[1].p == ok.y && out[1].bytes == ch.y_bytes,
               "forward's tensors");
        in.clear(); out.clear();
        expect(!chain_refused(ch, ok, 1, 0, in, out) && in.size() == (size_t)3 * ch.nblocks + 2 && out.size() == (size_t)3 * ch.nblocks + 1 &&
                   in[in.size() - 2].p == ok.saved && in.back().p == ok.g_y && in.back().bytes == ch.y_bytes && out.back().p == ok.g_x &&
                   out.back().optional && out.back().bytes == lay.dense_bytes(0),
               "backward's tensors");
    };
    {
        const pmp_trunk_shape one_pool{1, 16, 16, 16, 1, {16}, {3}, 1}, mixed{2, 16, 32, 16, 3, {16, 8, 8}, {3, 5, 3}, 0};
        const pmp_qtail_shape tail{1, 16, 16}, wide{1, 16, 48};
        const char *trunk_rule = "index out of range (0 .. 2 * nblocks)", *tail_rule = "index out of range (0 .. 8)";
        chain_rows(chain_of(&one_pool), chain_of((const pmp_trunk_shape *)nullptr), trunk_rule);
        chain_rows(chain_of(&mixed), chain_of((const pmp_trunk_shape *)nullptr), trunk_rule);
        chain_rows(chain_of(&tail), chain_of((const pmp_qtail_shape *)nullptr), tail_rule);
        chain_rows(chain_of(&wide), chain_of((const pmp_qtail_shape *)nullptr), tail_rule);
        const Chain p = chain_of(&one_pool), m = chain_of(&mixed), t = chain_of(&wide);
        expect(p.lay.nt == 3 && p.y_bytes == (size_t)4 * 16 * 8 * 8 && p.pool == 1 && m.lay.nt == 7 && m.y_bytes == (size_t)4 * 2 * 8 * 16 * 32 && !m.pool &&
                   m.blocks[1].cin == 16 && m.blocks[1].cout == 8 && m.blocks[1].k == 5 && !m.lay.half[6],
               "a trunk as a chain");
        expect(t.lay.nt == 9 && t.nblocks == 4 && t.y_bytes == (size_t)4 * 8 * 8 * 24 && !t.lay.half[6] && t.lay.half[7] && t.lay.half[8] &&
                   t.blocks[1].cin == 128 && !strcmp(t.unpack_name, "qtail_step") && !strcmp(m.unpack_name, "blocked_to_dense"),
               "the tail as a chain");
        const pmp_trunk_shape bad = {1, 24, 16, 16, 1, {16}, {3}, 1};
        expect(chain_of(&bad).refused == TRAIN_SHAPE_RULE && chain_of(&one_pool).refused == nullptr, "a chain of a refused shape");
    }
    // a single block: the device forms and the host forms, whose staging goes by the order of ins and outs
    {
        used = slots;
        const pmp_rb_shape rs{2, 16, 16, 16, 8, 3};
        const size_t bx = (size_t)4 * 2 * 16 * 256, by = bx / 2, w0 = (size_t)4 * 9 * 8 * 16, w2 = w0 / 2, wsc = (size_t)4 * 8 * 16;
        float *x = place(bx), *t = place(by), *out = place(by), *g_out = place(by), *g_x = place(bx);
        float *pw0 = place(w0), *pw2 = place(w2), *pwsc = place(wsc), *g0 = place(w0), *g2 = place(w2), *gsc = place(wsc);
        const RbCall fwd{false, {pw0, pw2, pwsc, x}, {t, out}}, bwd{true, {pw0, pw2, pwsc, x, t, out, g_out}, {g0, g2, gsc, g_x}};
        std::vector<Span> in, o;
        for (bool device : {true, false}) {
            expect(!rb_refused(&rs, fwd, device, in, o) && in.size() == 4 && o.size() == 2 && in[3].p == x && in[3].bytes == bx && in[2].bytes == wsc &&
                       o[0].p == t && o[1].p == out && o[1].bytes == by,
                   "a block's forward call and its tensors");
            expect(!rb_refused(&rs, bwd, device, in, o) && in.size() == 7 && o.size() == 4 && in[4].p == t && in[6].p == g_out && o[0].p == g0 &&
                       o[3].p == g_x && o[3].optional && o[3].bytes == bx,
                   "a block's backward call and its tensors");
            expect(says(rb_refused(nullptr, fwd, device, in, o), "null or unsupported shape"), "a block's null shape");
            RbCall q = bwd;
            q.out[q.G_X] = nullptr; expect(!rb_refused(&rs, q, device, in, o), "g_x is optional");
            q.out[q.G_X] = off(g_out, 64); expect(is(rb_refused(&rs, q, device, in, o), "an output tensor overlaps an input"), "g_x inside g_out");
            q = bwd; q.out[0] = g2; expect(is(rb_refused(&rs, q, device, in, o), "two output tensors overlap"), "g_w0 is g_w2");
            q = bwd; q.in[q.T] = nullptr; expect(is(rb_refused(&rs, q, device, in, o), "null tensor"), "null t");
            q = fwd; q.out[q.T_O] = off(x, 16); expect(is(rb_refused(&rs, q, device, in, o), "an output tensor overlaps an input"), "t overlaps x");
            q = fwd; q.in[2] = nullptr; expect(says(rb_refused(&rs, q, device, in, o), "shortcut"), "no wsc with cin != cout");
            q = fwd; q.in[q.X] = off(x, 2); expect(device ? says(rb_refused(&rs, q, device, in, o), "aligned") : !rb_refused(&rs, q, device, in, o), "misaligned x: device forms only");
        }
    }
    // a stem: the pointer-level rows of tests/test_gpu_stem_grad.py
    {
        used = slots;
        const pmp_stem_shape qs{1, 16, 16, 1, 9, 0}, ms{1, 16, 16, 4, 9, 1};
        const StemSizes z(ms);                                                 // the larger of the two
        float *w[3], *b[3], *g_w[3], *g_b[3];
        for (int j = 0; j < 3; ++j) { w[j] = place(z.w[j]); b[j] = place(z.b[j]); g_w[j] = place(z.w[j]); g_b[j] = place(z.b[j]); }
        float *x = place(z.x), *y = place(z.y), *g_y = place(z.y), *g_x = place(z.x);
        const float *w1[3] = {w[0], nullptr, nullptr}, *b1[3] = {b[0], nullptr, nullptr};
        float *gw1[3] = {g_w[0], nullptr, nullptr}, *gb1[3] = {g_b[0], nullptr, nullptr};
        StemPtrs f{}, r{};                                                     // of the QT stem; f3, r3 below of the MTT stem
        f.x = x; f.w = w1; f.b = b1; f.y_out = y;
        r.x = x; r.y = y; r.w = w1; r.g_y = g_y; r.g_x = g_x; r.g_w = gw1; r.g_b = gb1;
        StemPtrs f3 = f, r3 = r;
        f3.w = w; f3.b = b; r3.w = w; r3.g_w = g_w; r3.g_b = g_b;
        expect(!stem_refused(&qs, f, false) && !stem_refused(&qs, r, true) && !stem_refused(&ms, f3, false) && !stem_refused(&ms, r3, true), "accepted stem calls");
        expect(says(stem_refused(nullptr, f, false), "null or unsupported shape") && says(stem_refused(nullptr, r, true), "null or unsupported shape"), "a stem's null shape");
        expect(says(stem_refused(&ms, f, false), "exactly when split") && says(stem_refused(&qs, r3, true), "exactly when split"), "split against the arrays");
        StemPtrs q = f;
        q.x = nullptr; expect(is(stem_refused(&qs, q, false), "null tensor"), "null x");
        expect(says(stem_refused(nullptr, q, false), "null or unsupported shape"), "a stem's shape is looked at first");
        q = f; q.w = nullptr; expect(is(stem_refused(&qs, q, false), "null tensor"), "null d_w");
        q = f; q.b = nullptr; expect(is(stem_refused(&qs, q, false), "null tensor"), "null d_b");
        q = f; q.y_out = nullptr; expect(is(stem_refused(&qs, q, false), "null tensor"), "null y");
        q = f; q.x = off(x, 2); expect(says(stem_refused(&qs, q, false), "aligned"), "misaligned x");
        q = f; q.y_out = off(x, 64); expect(is(stem_refused(&qs, q, false), "an output tensor overlaps an input"), "y overlaps x");
        q = f; q.y_out = off(x, 4 * (20 * 20 - 1)); expect(is(stem_refused(&qs, q, false), "an output tensor overlaps an input"), "y overlaps the end of x");
        q = f; q.y_out = off(x, 4 * 20 * 20); expect(!stem_refused(&qs, q, false), "y right behind x");
        q = f; q.y_out = w[0]; expect(is(stem_refused(&qs, q, false), "an output tensor overlaps an input"), "y is w[0]");
        q = f3; q.y_out = off(b[1], -4 * 100); expect(is(stem_refused(&ms, q, false), "an output tensor overlaps an input"), "y overlaps b[1]");
        q = r; q.b = nullptr; q.y_out = nullptr; expect(!stem_refused(&qs, q, true), "backward has neither b nor y_out");
        q = r; q.g_x = nullptr; expect(!stem_refused(&qs, q, true), "a stem's g_x is optional");
        q = r; q.y = nullptr; expect(is(stem_refused(&qs, q, true), "null tensor"), "backward without y");
        q = r; q.g_y = nullptr; expect(is(stem_refused(&qs, q, true), "null tensor"), "null g_y");
        q = r; q.g_w = nullptr; expect(is(stem_refused(&qs, q, true), "null tensor"), "null d_g_w");
        q = r; q.g_b = nullptr; expect(is(stem_refused(&qs, q, true), "null tensor"), "null d_g_b");
        q = r; q.g_x = off(x, 16); expect(is(stem_refused(&qs, q, true), "an output tensor overlaps an input"), "g_x overlaps x");
        q = r; q.g_x = g_y; expect(is(stem_refused(&qs, q, true), "an output tensor overlaps an input"), "g_x is g_y");
        q = r; q.g_x = off(y, 1024); expect(is(stem_refused(&qs, q, true), "an output tensor overlaps an input"), "g_x inside y");
        { float *u[3] = {w[0], nullptr, nullptr}; q = r; q.g_w = u; expect(is(stem_refused(&qs, q, true), "an output tensor overlaps an input"), "g_w[0] is w[0]"); }
        { float *u[3] = {off(g_x, 16), nullptr, nullptr}; q = r; q.g_w = u; expect(is(stem_refused(&qs, q, true), "two output tensors overlap"), "g_w[0] overlaps g_x"); }
        { float *u[3] = {off(g_w[0], 64), nullptr, nullptr}; q = r; q.g_b = u; expect(is(stem_refused(&qs, q, true), "two output tensors overlap"), "g_b[0] inside g_w[0]"); }
        { float *u[3] = {g_w[0], g_w[2], g_w[2]}; q = r3; q.g_w = u; expect(is(stem_refused(&ms, q, true), "two output tensors overlap"), "g_w[1] is g_w[2]"); }
        { float *u[3] = {g_b[0], g_b[1], off(g_b[2], 2)}; q = r3; q.g_b = u; expect(says(stem_refused(&ms, q, true), "aligned"), "misaligned g_b[2]"); }
    }
    // a head and the gate: the pointer-level rows of tests/test_gpu_head_grad.py
    {
        used = slots;
        const pmp_head_shape plain{3, 16, 16, 8, 2, 0, 0}, att{3, 24, 16, 8, 2, 4, 2};
        const HeadSizes z(att);                                                // the larger of the two
        HeadPtrs f{}, r{};                                                     // of the head with an attention input
        f.x = place(z.x); f.w = place(z.w); f.b = place(z.b); f.prev = place(z.y); f.q = place(z.q); f.y = place(z.y); f.att = place(z.att);
        r.x = f.x; r.w = f.w; r.g_y = place(z.y); r.g_att = place(z.att); r.g_x = place(z.x); r.g_w = place(z.w); r.g_b = place(z.b);
        r.g_q = place(z.q); r.g_prev = place(z.y);
        HeadPtrs fp = f, rp = r;                                               // of the plain head
        fp.q = nullptr; fp.att = nullptr; rp.g_att = nullptr; rp.g_q = nullptr;
        float *spare = place(z.att);
        expect(!head_refused(&att, f, false) && !head_refused(&att, r, true) && !head_refused(&plain, fp, false) && !head_refused(&plain, rp, true), "accepted head calls");
        expect(says(head_refused(nullptr, f, false), "null or unsupported shape") && says(head_refused(nullptr, r, true), "null or unsupported shape"), "a head's null shape");
        HeadPtrs q = fp;
        q.prev = nullptr; expect(!head_refused(&plain, q, false), "prev is optional");
        q = rp; q.g_x = nullptr; q.g_prev = nullptr; expect(!head_refused(&plain, q, true), "g_x and g_prev are optional");
        q = r; q.g_q = nullptr; expect(!head_refused(&att, q, true), "g_q is optional");
        q = fp; q.x = nullptr; expect(is(head_refused(&plain, q, false), "null tensor"), "a head's null x");
        expect(says(head_refused(nullptr, q, false), "null or unsupported shape"), "a head's shape is looked at first");
        q = f; q.w = off(f.w, 1); expect(says(head_refused(&att, q, false), "aligned"), "misaligned w");
        q = fp; q.b = nullptr; expect(is(head_refused(&plain, q, false), "null tensor"), "null b");
        q = fp; q.y = nullptr; expect(is(head_refused(&plain, q, false), "null tensor"), "a head's null y");
        q = fp; q.q = spare; expect(says(head_refused(&plain, q, false), "exactly when up_y"), "q without up_y");
        q = fp; q.att = spare; q.y = const_cast<float *>(fp.x); expect(says(head_refused(&plain, q, false), "exactly when up_y"), "att without up_y, before overlaps");
        q = f; q.att = nullptr; expect(says(head_refused(&att, q, false), "exactly when up_y"), "up_y without att");
        q = fp; q.y = off(fp.x, 64); expect(is(head_refused(&plain, q, false), "an output tensor overlaps an input"), "a head's y overlaps x");
        q = fp; q.y = const_cast<float *>(fp.prev); expect(is(head_refused(&plain, q, false), "an output tensor overlaps an input"), "y is prev");
        q = fp; q.y = off(fp.w, 4 * 143); expect(is(head_refused(&plain, q, false), "an output tensor overlaps an input"), "y overlaps the end of w");
        q = f; q.att = off(f.q, -16); expect(is(head_refused(&att, q, false), "an output tensor overlaps an input"), "att overlaps q");
        q = f; q.att = f.y; expect(is(head_refused(&att, q, false), "two output tensors overlap"), "att is y");
        q = rp; q.g_y = nullptr; expect(is(head_refused(&plain, q, true), "null tensor"), "a head's null g_y");
        q = rp; q.g_w = nullptr; expect(is(head_refused(&plain, q, true), "null tensor"), "null g_w");
        q = r; q.g_b = nullptr; expect(is(head_refused(&att, q, true), "null tensor"), "null g_b");
        q = rp; q.g_att = spare; expect(says(head_refused(&plain, q, true), "exactly when up_y"), "g_att without up_y");
        q = r; q.g_att = nullptr; expect(says(head_refused(&att, q, true), "exactly when up_y"), "up_y without g_att");
        q = rp; q.g_q = spare; expect(says(head_refused(&plain, q, true), "only with g_att"), "g_q without g_att");
        q = rp; q.g_x = const_cast<float *>(rp.g_y); expect(is(head_refused(&plain, q, true), "an output tensor overlaps an input"), "a head's g_x is g_y");
        q = rp; q.g_w = const_cast<float *>(rp.w); expect(is(head_refused(&plain, q, true), "an output tensor overlaps an input"), "g_w is w");
        q = rp; q.g_b = off(rp.g_w, 64); expect(is(head_refused(&plain, q, true), "two output tensors overlap"), "g_b inside g_w");
        q = r; q.g_q = off(r.g_att, 1024); expect(is(head_refused(&att, q, true), "an output tensor overlaps an input"), "g_q inside g_att");
        q = r; q.g_prev = r.g_x; expect(is(head_refused(&att, q, true), "two output tensors overlap"), "g_prev is g_x");
        q = r; q.g_q = off(r.g_q, 1); expect(says(head_refused(&att, q, true), "aligned"), "misaligned g_q");
        // the gate: 1024 floats each
        float *a = spare, *b = spare + 1024, *o = spare + 4096, *o2 = spare + 8192, *acc = spare + 12288, *g_y = spare + 2048;
        auto fw = [&](int64_t count, const float *x, const float *g, const float *y) { return gate_refused(count, false, x, g, nullptr, nullptr, y, nullptr); };
        expect(!fw(1024, a, b, o) && !fw(1024, a, a, o) && !fw(1024, a, b, b + 1024), "accepted gate calls");
        for (int64_t count : {(int64_t)0, (int64_t)-1, (int64_t)1 << 31}) expect(is(fw(count, a, b, o), GATE_COUNT_RULE), "the gate's count");
        expect(is(fw(1024, nullptr, b, o), "null tensor") && is(fw(1024, a, nullptr, o), "null tensor") && is(fw(1024, a, b, nullptr), "null tensor"), "the gate's null tensors");
        expect(is(fw(1024, a, b, a), "an output tensor overlaps an input") && is(fw(1024, a, b, b + 1023), "an output tensor overlaps an input"), "y over x, over the end of a");
        expect(says(fw(1024, off(a, 2), b, o), "aligned") && says(fw(1024, a, b, off(o, 1)), "aligned"), "the gate's alignment");
        auto bw = [&](int64_t count, const float *gy, const float *gacc, const float *gx, const float *ga) { return gate_refused(count, true, a, b, gy, gacc, gx, ga); };
        expect(!bw(1024, g_y, acc, o, o2) && !bw(1024, g_y, nullptr, o, o2), "accepted gate backward calls; g_acc is optional");
        expect(is(bw(1024, nullptr, acc, o, o2), "null tensor") && is(bw(0, nullptr, acc, o, o2), "null tensor"), "a null g_y is looked at before the count");
        expect(is(bw(0, g_y, acc, o, o2), GATE_COUNT_RULE), "the gate's backward count");
        expect(is(bw(1024, g_y, acc, nullptr, o2), "null tensor") && is(bw(1024, g_y, acc, o, nullptr), "null tensor"), "null g_x, null g_a");
        expect(is(bw(1024, g_y, acc, acc, o2), "an output tensor overlaps an input") && is(bw(1024, g_y, acc, o, a), "an output tensor overlaps an input"), "g_x is g_acc, g_a is x");
        expect(is(bw(1024, g_y, acc, o, o), "two output tensors overlap") && is(bw(1024, g_y, acc, o + 512, o), "two output tensors overlap"), "g_a over g_x");
        expect(says(bw(1024, g_y, off(acc, 2), o, o2), "aligned"), "misaligned g_acc");
    }
    {   // a step's ends: the gather's set of 7 blocks and batch of 5 rows, Adam's three tensors; host arrays stand in for device memory
        static uint8_t set[7 * 4624 + 2 * 7 * 1156 + 7 * 64 + 2 * 7 * 768 + 64] __attribute__((aligned(16)));
        static float out[5 * 4624 + 5 * 64 + 64] __attribute__((aligned(16)));
        static uint8_t lab[5 * 64 + 2 * 5 * 768 + 64] __attribute__((aligned(16)));
        static int64_t index[5];
        static int32_t status;
        const pmp_batch_src luma{set, nullptr, nullptr, set + 7 * 4624 + 14 * 1156, set + 7 * 4624 + 14 * 1156 + 7 * 64,
                                 (const int8_t *)(set + 7 * 4624 + 14 * 1156 + 7 * 64 + 7 * 768), 7};
        pmp_batch_src chroma = luma;
        chroma.u = set + 7 * 4624; chroma.v = set + 7 * 4624 + 7 * 1156;
        const pmp_batch_dst all{out, out + 5 * 4624, lab, lab + 5 * 64, (int8_t *)(lab + 5 * 64 + 5 * 768)};
        auto gr = [&](const pmp_batch_src &s, const pmp_batch_dst &d, int64_t n = 5) { return gather_refused(&s, index, n, &d, &status); };
        expect(!gr(luma, all) && !gr(chroma, all) && !gr(luma, pmp_batch_dst{out, nullptr, nullptr, nullptr, nullptr}), "accepted gather calls");
        expect(gather_refused(nullptr, index, 5, &all, &status) && gather_refused(&luma, nullptr, 5, &all, &status) &&
               gather_refused(&luma, index, 5, nullptr, &status) && gather_refused(&luma, index, 5, &all, nullptr), "the gather's null arguments");
        expect(says(gr(luma, all, 0), "n must be") && says(gr(luma, all, 65537), "n must be"), "the gather's n");
        pmp_batch_src s = luma; s.count = 0; expect(says(gr(s, all), "count"), "an empty set");
        s = luma; s.y = nullptr; expect(says(gr(s, all), "y is required"), "no y");
        s = chroma; s.v = nullptr; expect(says(gr(s, all), "go together"), "u without v");
        s = luma; s.msbt = nullptr; expect(says(gr(s, all), "source is NULL"), "msbt without its source");
        s = luma; s.qt8 = nullptr; expect(says(gr(s, pmp_batch_dst{nullptr, out, nullptr, nullptr, nullptr}), "source is NULL"), "qt_f without its source");
        expect(says(gr(luma, pmp_batch_dst{}), "no output"), "no output asked for");
        s = luma; s.y = set + 2; expect(says(gr(s, all), "aligned"), "a source two bytes off");
        pmp_batch_dst d = all; d.qt_f = out + 16; expect(is(gr(luma, d), "two output tensors overlap"), "qt_f inside x");
        d = all; d.qt8 = (uint8_t *)index; expect(is(gr(luma, d), "an output tensor overlaps an input"), "an output over the index");
        d = all; d.qt8 = (uint8_t *)&status; expect(is(gr(luma, d), "two output tensors overlap"), "an output over the status word");
        d = all; d.msbt = const_cast<uint8_t *>(luma.msbt); expect(is(gr(luma, d), "an output tensor overlaps an input"), "an output over the set");

        static float t[12][300];
        float *p[3] = {t[0], t[1], t[2]}, *m[3] = {t[6], t[7], t[8]}, *v[3] = {t[9], t[10], t[11]};
        const float *g[3] = {t[3], t[4], t[5]};
        int64_t count[3] = {5, 64, 257};
        pmp_adam_params hp{1e-3, 0.9, 0.999, 1e-8};
        auto ar = [&](int nt = 3, int64_t step = 1) { return adam_refused(&hp, nt, p, g, m, v, count, step); };
        expect(!ar() && !ar(1) && !ar(3, (int64_t)1 << 40), "accepted Adam calls");
        expect(says(ar(0), "ntensors") && says(ar(-1), "ntensors") && says(ar(3, 0), "step") && says(ar(3, -1), "step"), "Adam's ntensors and step");
        expect(adam_refused(nullptr, 3, p, g, m, v, count, 1) && adam_refused(&hp, 3, nullptr, g, m, v, count, 1) && adam_refused(&hp, 3, p, nullptr, m, v, count, 1) &&
               adam_refused(&hp, 3, p, g, nullptr, v, count, 1) && adam_refused(&hp, 3, p, g, m, nullptr, count, 1) && adam_refused(&hp, 3, p, g, m, v, nullptr, 1), "Adam's null arguments");
        for (double *f : {&hp.lr, &hp.beta1, &hp.beta2, &hp.eps})
            for (double bad : {(double)NAN, (double)INFINITY}) {
                const double keep = *f;
                *f = bad; expect(says(ar(), "finite"), "a hyperparameter that is not finite");
                *f = keep;
            }
        hp.beta1 = 1.0; expect(says(ar(), "[0, 1)"), "beta1 1"); hp.beta1 = -0.1; expect(says(ar(), "[0, 1)"), "beta1 negative"); hp.beta1 = 0.0; expect(!ar(), "beta1 0"); hp.beta1 = 0.9;
        hp.beta2 = 1.0; expect(says(ar(), "[0, 1)"), "beta2 1"); hp.beta2 = 0.999;
        hp.eps = 0.0; expect(says(ar(), "eps"), "eps 0"); hp.eps = -1e-8; expect(says(ar(), "eps"), "eps negative"); hp.eps = 1e-8;
        count[1] = 0; expect(says(ar(), "count"), "count 0"); count[1] = 64;
        m[1] = nullptr; expect(is(ar(), "null tensor"), "a null entry"); m[1] = t[7];
        v[0] = off(t[9], 2); expect(says(ar(), "aligned"), "a tensor two bytes off"); v[0] = t[9];
        m[1] = t[0]; expect(says(ar(), "overlap"), "m over a param"); m[1] = t[7];
        g[2] = t[0] + 2; expect(says(ar(), "overlap"), "a gradient inside a param"); g[2] = t[5];
        p[1] = t[0]; expect(says(ar(), "overlap"), "the same param twice"); p[1] = t[1];
        v[2] = t[10] + 43; expect(says(ar(), "overlap"), "v over the end of another v"); v[2] = t[10] + 64; expect(!ar(), "tensors that touch"); v[2] = t[11];

        // the divergence guard on the same tensors: the matrix of tests/test_gpu_grad_guard.py through guard_refused and adam_guarded_refused
        static double own[64];                               // scratch [0, 8), the record [8, 12), the counters [16, 22)
        pmp_guard_params gp{1.0, 1};
        pmp_guard_record *rec = (pmp_guard_record *)(own + 8);
        pmp_guard_state *st = (pmp_guard_state *)(own + 16);
        int64_t big[3] = {5, 4097, 2 * 4096 + 1};
        expect(guard_scratch_bytes(3, count) == 48 && guard_scratch_bytes(3, big) == 16 * 6 && guard_scratch_bytes(1, count) == 16, "the guard's scratch");
        expect(guard_scratch_bytes(0, count) == -1 && guard_scratch_bytes(-1, count) == -1 && guard_scratch_bytes(3, nullptr) == -1, "no table for the guard's scratch");
        auto gu = [&](int nt = 3, const void *sc = nullptr, const pmp_guard_record *r = nullptr, const pmp_guard_state *s = nullptr) {
            return guard_refused(&gp, nt, g, count, sc ? sc : own, r ? r : rec, s);
        };
        expect(!gu() && !gu(1) && !gu(3, own, rec, st), "accepted guard calls, with counters and without");
        gp.max_norm = 0.0; gp.skip_nonfinite = 0; expect(!gu(), "max_norm 0: no clipping"); gp.max_norm = 1.0;
        expect(says(guard_refused(nullptr, 3, g, count, own, rec, st), "null") && says(guard_refused(&gp, 3, nullptr, count, own, rec, st), "null") &&
               says(guard_refused(&gp, 3, g, nullptr, own, rec, st), "null") && says(guard_refused(&gp, 3, g, count, nullptr, rec, st), "null") &&
               says(guard_refused(&gp, 3, g, count, own, nullptr, st), "null"), "the guard's null arguments");
        expect(says(gu(0), "ntensors") && says(gu(-1), "ntensors"), "the guard's ntensors");
        g[1] = nullptr; expect(is(gu(), "null tensor"), "a null gradient"); g[1] = off(t[4], 2); expect(says(gu(), "4-byte"), "a gradient two bytes off"); g[1] = t[4];
        for (int64_t bad : {(int64_t)0, (int64_t)-1, (int64_t)1 << 30}) { count[1] = bad; expect(says(gu(), "count"), "the guard's counts"); }
        count[1] = 64;
        for (double bad : {-1.0, (double)NAN, (double)INFINITY}) { gp.max_norm = bad; expect(says(gu(), "max_norm"), "the guard's max_norm"); }
        gp.max_norm = 1.0;
        expect(says(gu(3, off(own, 4)), "8-byte") && says(gu(3, own, (pmp_guard_record *)off(rec, 4)), "8-byte") &&
               says(gu(3, own, rec, (pmp_guard_state *)off(st, 4)), "8-byte"), "scratch, record and counters four bytes off");
        expect(says(gu(3, t[3]), "overlaps a gradient") && says(gu(3, own, (pmp_guard_record *)t[4]), "overlaps a gradient") &&
               says(gu(3, own, rec, (pmp_guard_state *)(t[5] + 250)), "overlaps a gradient"), "scratch, record and counters over a gradient");
        expect(says(gu(3, own, (pmp_guard_record *)(own + 5)), "overlap") && says(gu(3, own, rec, (pmp_guard_state *)(own + 4)), "overlap") &&
               says(gu(3, own, rec, (pmp_guard_state *)(own + 11)), "overlap") && !gu(3, own, rec, (pmp_guard_state *)(own + 12)) &&
               !gu(3, own, (pmp_guard_record *)(own + 6)), "scratch, record and counters over one another; right behind one another");

        auto ga = [&](const pmp_guard_record *r, int64_t step = 1) { return adam_guarded_refused(&hp, 3, p, g, m, v, count, step, r); };
        expect(!ga(rec), "an accepted guarded Adam call");
        expect(says(ga(rec, 0), "step"), "what Adam refuses, the guarded call refuses");
        expect(says(ga(nullptr), "null d_record") && says(ga((pmp_guard_record *)off(rec, 4)), "8-byte"), "a null record, one four bytes off");
        expect(says(ga((pmp_guard_record *)t[0]), "d_record overlaps") && says(ga((pmp_guard_record *)t[4]), "d_record overlaps") &&
               says(ga((pmp_guard_record *)(t[8] + 250)), "d_record overlaps") && says(ga((pmp_guard_record *)t[9]), "d_record overlaps"),
               "the record over a param, a gradient, an m and a v");
    }
    {   // gradient buckets: the layout, and the matrix of tests/test_gpu_grad_bucket.py through grad_pack_refused and grad_sum_refused
        const int64_t count[5] = {1, 3, 4, 5, 1023};
        int64_t at[5] = {-1, -1, -1, -1, -1};
        expect(grad_bucket_floats(5, count, at) == 1044 && at[0] == 0 && at[1] == 4 && at[2] == 8 && at[3] == 12 && at[4] == 20, "a bucket's layout");
        expect(grad_bucket_floats(5, count, nullptr) == 1044 && grad_bucket_floats(1, count, nullptr) == 4, "the offsets are optional");
        expect(grad_bucket_floats(0, count, at) == -1 && grad_bucket_floats(-1, count, at) == -1 && grad_bucket_floats(5, nullptr, at) == -1, "no table");
        for (int64_t bad : {(int64_t)0, (int64_t)-1, (int64_t)1 << 30, (int64_t)1 << 40}) {
            int64_t c3[3] = {5, bad, 7};
            expect(grad_bucket_floats(3, c3, at) == -1, "a count outside 1 .. 2^30 - 1");
        }
        { int64_t c1[1] = {((int64_t)1 << 30) - 1}; expect(grad_bucket_floats(1, c1, at) == (int64_t)1 << 30 && at[0] == 0, "the largest count"); }
        static float mem[8192] __attribute__((aligned(16)));
        float *bucket = mem + 4096;
        const float *g[5] = {mem, mem + 1, mem + 8, nullptr, mem + 16};
        auto pr = [&](int nt = 5, const float *b = nullptr) { return grad_pack_refused(nt, g, count, b ? b : bucket); };
        expect(!pr() && !pr(1), "accepted pack calls: a NULL entry, gradients that are only 4-byte aligned");
        expect(says(pr(0), "ntensors") && says(pr(-1), "ntensors"), "pack's ntensors");
        expect(says(grad_pack_refused(5, nullptr, count, bucket), "null") && says(grad_pack_refused(5, g, nullptr, bucket), "null") &&
                   says(grad_pack_refused(5, g, count, nullptr), "null"), "pack's null arguments");
        { int64_t c5[5] = {1, 3, 0, 5, 1023}; expect(says(grad_pack_refused(5, g, c5, bucket), "count"), "pack's count 0"); }
        { int64_t c5[5] = {1, 3, 4, (int64_t)1 << 30, 1023}; expect(says(grad_pack_refused(5, g, c5, bucket), "count"), "a count of 2^30, also of a NULL entry"); }
        expect(says(pr(5, bucket + 1), "16-byte") && says(pr(5, bucket + 2), "16-byte") && !pr(5, bucket + 4), "the bucket's 16 bytes");
        g[1] = off(mem + 1, 2); expect(says(pr(), "4-byte"), "a gradient two bytes off"); g[1] = mem + 1;
        g[4] = bucket + 1040; expect(says(pr(), "overlaps"), "a gradient inside the bucket's last quad"); g[4] = bucket + 1044; expect(!pr(), "right behind it");
        g[4] = bucket - 1023; expect(!pr(), "right in front of it"); g[4] = bucket - 1022; expect(says(pr(), "overlaps"), "over its first float"); g[4] = mem + 16;

        const float *s[64];
        for (int j = 0; j < 64; ++j) s[j] = mem + 64 * j;
        float *dst = mem + 4096;
        auto sr = [&](int nsrc = 3, int64_t n = 64, const float *d = nullptr) { return grad_sum_refused(nsrc, s, n, d ? d : dst); };
        expect(!sr() && !sr(1) && !sr(64) && !sr(3, 4) && !sr(3, 64, mem) && !sr(1, 64, mem), "accepted sum calls, in place too");
        expect(says(sr(0), "nsrc") && says(sr(-1), "nsrc") && says(sr(65), "nsrc"), "sum's nsrc");
        expect(says(grad_sum_refused(3, nullptr, 64, dst), "null") && says(grad_sum_refused(3, s, 64, nullptr), "null"), "sum's null arguments");
        for (int64_t n : {(int64_t)0, (int64_t)-4, (int64_t)1, (int64_t)3, (int64_t)5, (int64_t)66}) expect(says(sr(3, n), "multiple of 4"), "sum's count");
        expect(says(sr(3, 64, dst + 1), "16-byte") && says(sr(3, 64, dst + 2), "16-byte"), "a destination off 16 bytes");
        s[2] = mem + 130; expect(says(sr(), "16-byte"), "a source off 16 bytes"); s[2] = nullptr; expect(says(sr(), "null source"), "a null source");
        expect(!sr(2), "entries behind nsrc are not read"); s[2] = mem + 128;
        expect(says(sr(3, 64, mem + 64), "overlaps") && says(sr(3, 64, mem + 128), "overlaps"), "the destination is a source other than the first");
        expect(says(sr(3, 64, mem + 4), "overlaps") && says(sr(3, 64, mem + 188), "overlaps") && !sr(3, 64, mem + 192), "the destination partly over a source; right behind the last");
        s[1] = mem; expect(!sr(3, 64, dst), "sources may alias"); expect(says(sr(3, 64, mem), "overlaps"), "in place, and the first source given twice"); s[1] = mem + 64;
    }
    {   // data set assembly: the matrix of tests/test_gpu_dataset.py through select_refused and rows_gather_refused; 300 rows in 3 segments
        auto sh = [](auto *p, long bytes) { return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + bytes); };
        const uint8_t *fl[3] = {ds_flag[0], ds_flag[1], ds_flag[2]};
        auto sr = [&](const uint8_t *const *f = nullptr, int nflags = 3, int mask = 5, const int64_t *se = ds_seg, int nseg = 3, int64_t cap = 0,
                      int64_t n = 300, const int64_t *ix = ds_index, const int64_t *ct = ds_count) {
            return select_refused(f ? f : fl, nflags, mask, se, nseg, cap, n, ix, ct);
        };
        expect(!sr() && !sr(fl, 0) && !select_refused(nullptr, 0, 5, ds_seg, 3, 0, 300, ds_index, ds_count) && !sr(fl, 3, 255, ds_seg, 3, 7) && !sr(fl, 1, 1, ds_seg, 1),
               "accepted select calls");
        expect(says(sr(fl, 3, 5, ds_seg, 3, 0, 0), "n must be") && says(sr(fl, 3, 5, ds_seg, 3, 0, -1), "n must be") &&
                   says(sr(fl, 3, 5, ds_seg, 3, 0, ((int64_t)1 << 30) + 1), "n must be"), "select's n");
        expect(says(sr(fl, 3, 5, ds_seg, 0), "nseg") && says(sr(fl, 3, 5, ds_seg, 65537), "nseg"), "select's nseg");
        expect(says(sr(fl, -1), "nflags") && says(sr(fl, 65), "nflags"), "select's nflags");
        expect(says(sr(fl, 3, 0), "mask") && says(sr(fl, 3, 256), "mask") && says(sr(fl, 3, -1), "mask"), "select's mask");
        expect(says(sr(fl, 3, 5, ds_seg, 3, -1), "cap"), "a negative cap");
        expect(says(select_refused(nullptr, 1, 5, ds_seg, 3, 0, 300, ds_index, ds_count), "null d_flags"), "flags asked for, no array");
        { const uint8_t *g[3] = {ds_flag[0], nullptr, ds_flag[2]}; expect(is(sr(g), "null tensor"), "a null flag array"); }
        expect(is(sr(fl, 3, 5, nullptr), "null tensor") && is(sr(fl, 3, 5, ds_seg, 3, 0, 300, nullptr), "null tensor") &&
                   is(sr(fl, 3, 5, ds_seg, 3, 0, 300, ds_index, nullptr), "null tensor"), "select's null pointers");
        expect(says(sr(fl, 3, 5, sh(ds_seg, 4)), "aligned") && says(sr(fl, 3, 5, ds_seg, 3, 0, 296, sh(ds_index, 4)), "aligned") &&
                   says(sr(fl, 3, 5, ds_seg, 3, 0, 300, ds_index, sh(ds_count, 4)), "aligned"), "select's alignment");
        { const uint8_t *g[3] = {ds_flag[0], sh(ds_flag[1], 1), sh(ds_flag[2], 3)}; expect(!sr(g), "flag arrays need no alignment"); }
        { const uint8_t *g[3] = {ds_flag[0], (const uint8_t *)ds_index + 2392, ds_flag[2]}; expect(is(sr(g), "an output tensor overlaps an input"), "the index over the end of a flag array"); }
        expect(is(sr(fl, 3, 5, ds_index + 299), "an output tensor overlaps an input") && is(sr(fl, 3, 5, ds_seg, 3, 0, 300, ds_index, ds_seg), "an output tensor overlaps an input"),
               "an output over d_seg_end");
        expect(is(sr(fl, 3, 5, ds_seg, 3, 0, 300, ds_index, ds_index + 299), "two output tensors overlap") && !sr(fl, 3, 5, ds_seg, 3, 0, 296, ds_index, ds_index + 296),
               "d_count over the end of d_index; right behind it");

        auto gr = [&](const void *s = ds_src, int64_t nsrc = 300, int64_t rb = 68, const int64_t *ix = ds_index, int64_t m = 300, const void *d = ds_dst,
                      const int32_t *st = &ds_status) { return rows_gather_refused(s, nsrc, rb, ix, m, d, st); };
        expect(!gr() && !gr(ds_src + 4, 300, 68, ds_index, 300, ds_dst + 4) && !gr(ds_src, 1, 4, ds_index, 1) && !gr(ds_src, 1, 65536 / 4, ds_index, 1, ds_dst) && !gr(ds_src, 5100, 4, ds_index, 300),
               "accepted gather calls");
        expect(says(gr(ds_src, 0), "nsrc") && says(gr(ds_src, -3), "nsrc"), "an empty source");
        expect(says(gr(ds_src, 300, 68, ds_index, 0), "m must be") && says(gr(ds_src, 300, 68, ds_index, ((int64_t)1 << 30) + 1), "m must be"), "the gather's m");
        for (int64_t rb : {(int64_t)0, (int64_t)-4, (int64_t)2, (int64_t)66, (int64_t)65540, (int64_t)1 << 33})
            expect(says(gr(ds_src, 300, rb), "row_bytes"), "row_bytes");
        expect(is(gr(nullptr), "null tensor") && is(gr(ds_src, 300, 68, nullptr), "null tensor") && is(gr(ds_src, 300, 68, ds_index, 300, nullptr), "null tensor") &&
                   is(gr(ds_src, 300, 68, ds_index, 300, ds_dst, nullptr), "null tensor"), "the gather's null pointers");
        expect(says(gr(ds_src + 2), "aligned") && says(gr(ds_src, 300, 68, ds_index, 300, ds_dst + 1), "aligned") && says(gr(ds_src, 300, 68, sh(ds_index, 4), 299), "aligned") &&
                   says(gr(ds_src, 300, 68, ds_index, 300, ds_dst, sh(&ds_status, 2)), "aligned"), "the gather's alignment");
        expect(is(gr(ds_src, 300, 68, ds_index, 300, ds_src), "an output tensor overlaps an input") && is(gr(ds_src, 300, 68, ds_index, 300, ds_src + 300 * 68 - 4), "an output tensor overlaps an input") &&
                   !gr(ds_src, 200, 68, ds_index, 100, ds_src + 200 * 68), "the rows over the source; right behind it");
        expect(is(gr(ds_src, 300, 68, ds_index, 300, ds_index), "an output tensor overlaps an input") && is(gr(ds_src, 300, 68, ds_index, 300, ds_dst, (const int32_t *)(ds_index + 7)), "an output tensor overlaps an input") &&
                   is(gr(ds_src, 300, 68, ds_index, 300, ds_dst, (const int32_t *)(ds_src + 64)), "an output tensor overlaps an input"), "an output over the index; the status word over an input");
        expect(is(gr(ds_src, 300, 68, ds_index, 300, ds_dst, (const int32_t *)(ds_dst + 128)), "two output tensors overlap"), "the status word inside the rows");
    }
    if (!failures) printf("train_check: ok\n");
    return failures ? 1 : 0;
}
