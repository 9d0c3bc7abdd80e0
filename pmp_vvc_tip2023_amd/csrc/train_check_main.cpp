// train_check_main.cpp — train_check.h on the CPU, with a main of its own, for `make traincheck` (-fsanitize=address,undefined): the
// shapes of the refusal matrices of tests/test_gpu_resblock_grad.py and tests/test_gpu_trunk_grad.py, the weight rule per block, and
// spans that overlap, are missing or are misaligned, a stem's shapes, sizes and pointer arrays (tests/test_gpu_stem_grad.py), and a
// head's shapes, sizes and the tensors tied to its attention input (tests/test_gpu_head_grad.py).  No pointer is dereferenced; exit
// status 0 and "train_check: ok" when all hold.
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
    const TrunkLayout lay(big);
    size_t sum = 0;
    for (int i = 0; i < lay.nt; ++i) {
        expect(lay.off[i] == sum && !(lay.off[i] & 15), "d_saved offsets");
        sum += (size_t)256 * 256 * 256 * 4 * pad_channels(lay.c[i]);
    }
    expect(lay.nt == 17 && lay.off[17] == sum && lay.c[0] == 64 && lay.c[1] == 64 && lay.c[2] == 64 && lay.c[3] == 33 && lay.c[16] == 48, "d_saved layout");
    expect(block_shape(big, 0).cin == 64 && block_shape(big, 1).cin == 64 && block_shape(big, 7).cin == 32 && block_shape(big, 7).cout == 48, "block_shape");
    // ---- the weights of every block
    alignas(16) static float mem[16 * 2560];                                   // 2560 floats apart: the largest tensor here has 9 * 16 * 16
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
        const QtailLayout nets(pmp_qtail_shape{200, 16, 16}), wide(pmp_qtail_shape{2, 16, 48}), big(pmp_qtail_shape{256, 256, 256});
        expect(nets.h2 == 16 && nets.w2 == 16 && nets.off[QTAIL_SAVED] == (size_t)58982400 && nets.x4 == (size_t)4 * 200 * 64 * 256 &&
                   nets.x9 == (size_t)4 * 200 * 8 * 64 && nets.dense_bytes(0) == nets.x4 && nets.dense_bytes(6) == nets.x4 / 2 &&
                   nets.dense_bytes(8) == nets.x9,
               "the tail's d_saved at the nets' shape");
        expect(wide.h2 == 16 && wide.w2 == 32 && wide.off[7] == (size_t)4 * 2 * 16 * 48 * 256 &&
                   wide.off[9] == wide.off[7] + (size_t)4 * 2 * 16 * 32 * 32 && wide.x9 == (size_t)4 * 2 * 8 * 8 * 24,
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
    if (!failures) printf("train_check: ok\n");
    return failures ? 1 : 0;
}
