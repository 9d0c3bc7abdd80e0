// api_train.cpp — a trunk of Model_QBD.ResidualBlocks, forward and backward, for a trainer (include/pmp.h: pmp_trunk_*), its
// activations blocked between the blocks and between the two directions (trunk_glue.hip), ONE block (pmp_resblock_forward /
// _backward): a shell around the trunk's block that takes the caller's dense tensors through the blocked layout in the context's
// workspace arena, and a net's stem (pmp_stem_*, stem_train.hip), dense in and out, and an MTT net's heads and gate products
// (pmp_head_*, pmp_gate_*, head_train.hip), dense too, and a QT net's tail (pmp_qtail_*, qtail_train.hip): four blocks, one with
// 128 inputs and one on a map of half the size, and the pools between them.  There is one statement of the block, TrainGraph::block_forward /
// block_backward, one of a chain of blocks with a d_saved (Chain, ChainPtrs of train_check.h, chain_entry here: trunk and tail differ in
// layout, blocks and bodies), one of what a call must satisfy (train_check.h's *_refused: no memory is read, so they also run on the CPU),
// one of what an entry does before it runs (admit).  The convolutions are conv_mfma.hip's (the data gradients are ordinary convolutions
// with mirrored, transposed weights), the weight gradients conv_wgrad.hip's.  Always the exact fp32 MFMA datapath: the Pass says so,
// whatever pmp_set_precision chose for inference.
#include <initializer_list>

#include "pmp_host.h"
#include "train_check.h"

using namespace pmp;

namespace {

struct Block : BlockShape {            // a block and its weights; the gradients only backward
    const float *w0, *w2, *wsc;
    float *g_w0, *g_w2, *g_wsc;
};

// block i, of shape s, of a chain whose weights are d_w / d_g_w of pmp_trunk_* and pmp_qtail_*: w0, w2, wsc per block
Block block_of(const BlockShape &s, const float *const *w, float *const *g_w, int i)
{
    Block b{s, w[3 * i], w[3 * i + 1], w[3 * i + 2], nullptr, nullptr, nullptr};
    if (g_w) { b.g_w0 = g_w[3 * i]; b.g_w2 = g_w[3 * i + 1]; b.g_wsc = g_w[3 * i + 2]; }
    return b;
}

struct Tensor { float *p; size_t off, bytes; };   // bytes != 0: the arena's, and the call's to reuse;  0: a view of the caller's memory

Tensor view(const SavedLayout &lay, const void *saved, int i) { return Tensor{(float *)((char *)saved + lay.off[i]), 0, 0}; }

// The graph of one call on a Pass: run_train() runs it twice, measuring (no launches, null pointers) and live.  rc is the call's: behind
// a failed launch nothing more is launched, and the arena's bookkeeping runs on to the end.
struct TrainGraph {
    pmp_ctx *c;
    Pass &ps;
    int n, h, w;
    int rc = PMP_OK;
    bool live() const { return !ps.arena.measuring && rc == PMP_OK; }
    void check(hipError_t e, const char *what)
    {
        if (e != hipSuccess && rc == PMP_OK) rc = hip_fail(c, e, what);
    }
    Tensor floats(size_t count)
    {
        const size_t off = ps.arena.take(count * sizeof(float));
        return Tensor{ps.arena.ptr(off), off, count * sizeof(float)};
    }
    Tensor act(int cp) { return floats((size_t)n * cp * h * w); }
    void release(Tensor &t)
    {
        if (t.bytes) ps.arena.give(t.off, t.bytes);
        t.bytes = 0;
    }
    void to_blocked(const float *src, const float *m, int mode, int C, const Tensor &dst)
    {
        if (live()) check(launch_dense_to_blocked(ps.stream, src, m, mode, dst.p, n, C, pad_channels(C), h, w), "dense_to_blocked");
    }
    Tensor blocked(const float *src, const float *m, int mode, int C)
    {
        Tensor t = act(pad_channels(C));
        to_blocked(src, m, mode, C, t);
        return t;
    }
    void dense(const Tensor &t, float *dst, int C)
    {
        if (live()) check(launch_blocked_to_dense(ps.stream, t.p, dst, n, C, pad_channels(C), h, w), "blocked_to_dense");
    }
    // w [cout][cin][k][k] -> the fragments of the convolution that reads 16 CB channels and writes 16 NT
    Tensor packed(const float *wt, int cout, int cin, int k, int nt_ch, int cb_ch, bool flip_t)
    {
        Tensor t = floats((size_t)(cb_ch / 16) * k * k * (nt_ch / 16) * 256);
        if (live()) check(launch_pack_mfma(ps.stream, wt, t.p, cout, cin, k, nt_ch / 16, cb_ch / 16, flip_t ? 1 : 0), "pack_mfma");
        return t;
    }
    void conv(const Tensor &x, int cin_p, const Tensor &wt, int k, const Tensor *x_sc, int csc_p, const Tensor *w_sc, const Tensor *res,
              const Tensor *gate, bool relu, Tensor &out, int cout_p)
    {
        if (!live()) return;
        ConvMfmaArgs a{};
        a.x = x.p; a.w = wt.p; a.out = out.p;
        if (x_sc) { a.x_sc = x_sc->p; a.w_sc = w_sc->p; a.Csc = csc_p; }
        if (res) a.res = res->p;
        if (gate) a.gate = gate->p;
        a.N = n; a.H = h; a.W = w; a.Cin = cin_p; a.Cout = cout_p; a.KH = a.KW = k; a.relu = relu ? 1 : 0; a.nan = 1;
        check(launch_conv_mfma(ps.stream, a), "conv_mfma");
    }
    void wgrad(const Tensor &a, int ca_p, const Tensor &g, int cg_p, int k, float *dw, int cout, int cin)
    {
        Tensor part = floats(wgrad_partial_floats(n, h, w, ca_p, cg_p, k));
        if (live()) check(launch_wgrad(ps.stream, a.p, g.p, n, h, w, ca_p, cg_p, k, part.p, dw, cout, cin), "wgrad");
        release(part);
    }

    // ---- the block, on blocked tensors
    // t = relu(conv0(x)), out = relu(conv2(t) + sc(x))  (Model_QBD.py:40-44): the launches of Graph::rb() on the fp32 datapath
    // region: a 0/1 tensor both results are multiplied by behind their ReLU (a QT tail's q6, whose map fills a corner of its tiles)
    void block_forward(const Block &b, const Tensor &x, Tensor &t, Tensor &y, const Tensor *region = nullptr)
    {
        const bool sc = b.cin != b.cout;
        Tensor w0 = packed(b.w0, b.cout, b.cin, b.k, b.cop(), b.cip(), false), w2 = packed(b.w2, b.cout, b.cout, b.k, b.cop(), b.cop(), false);
        Tensor wsc = sc ? packed(b.wsc, b.cout, b.cin, 1, b.cop(), b.cip(), false) : Tensor{};
        conv(x, b.cip(), w0, b.k, nullptr, 0, nullptr, nullptr, region, true, t, b.cop());
        conv(t, b.cop(), w2, b.k, sc ? &x : nullptr, b.cip(), sc ? &wsc : nullptr, sc ? nullptr : &x, region, true, y, b.cop());
        for (Tensor *p : {&w0, &w2, &wsc}) release(*p);
    }

    // include/pmp.h: dW2, dWsc, gt, dW0, dx in that order, behind the caller's gu.  The weight gradients go out dense; the data
    // gradient, where dx is asked for, as a blocked tensor of the arena that the caller releases.  x and t are views of the caller's
    // memory (a trunk's d_saved), read only, or the call's own copies in the arena (a single block's).  Own copies end here: t's words
    // become the mask [t > 0] in place, as Graph::rb() decides in_place, and both are released behind their last reader.  That keeps the
    // workspace need of a single block's call where a mask of its own would add an activation to it; nothing else here asks who owns what.
    // A block of 128 inputs (a QT tail's q4) hands its data gradient back as two tensors, dx = channels 0..63 and dx_hi = 64..127:
    // conv_mfma writes at most 64.
    void block_backward(const Block &b, Tensor &x, Tensor &t, const Tensor &gu, Tensor *dx, Tensor *dx_hi = nullptr)
    {
        const bool sc = b.cin != b.cout;
        wgrad(t, b.cop(), gu, b.cop(), b.k, b.g_w2, b.cout, b.cout);
        if (sc) wgrad(x, b.cip(), gu, b.cop(), 1, b.g_wsc, b.cout, b.cin);
        Tensor fresh{};
        Tensor &mask = t.bytes ? t : (fresh = act(b.cop()));                     // [t > 0], the convolution's gate
        if (live()) check(launch_blocked_relu(ps.stream, 2, t.p, nullptr, mask.p, n, b.cop(), h, w), "blocked_relu");
        Tensor w2t = packed(b.w2, b.cout, b.cout, b.k, b.cop(), b.cop(), true);
        Tensor gt = act(b.cop());
        conv(gu, b.cop(), w2t, b.k, nullptr, 0, nullptr, nullptr, &mask, false, gt, b.cop());
        release(mask);
        release(w2t);
        wgrad(x, b.cip(), gt, b.cop(), b.k, b.g_w0, b.cout, b.cin);
        release(x);
        const int part = b.cip() > 64 ? 64 : b.cip();
        for (int c0 = 0; dx && c0 < b.cip(); c0 += part) {
            Tensor w0t = packed(b.w0 + c0 * b.k * b.k, b.cout, b.cin, b.k, part, b.cop(), true);
            Tensor wsct = sc ? packed(b.wsc + c0, b.cout, b.cin, 1, part, b.cop(), true) : Tensor{};
            Tensor &d = c0 ? *dx_hi : *dx;
            d = act(part);
            conv(gt, b.cop(), w0t, b.k, sc ? &gu : nullptr, b.cop(), sc ? &wsct : nullptr, sc ? nullptr : &gu, nullptr, false, d, part);
            release(w0t);
            release(wsct);
        }
        release(gt);
    }

    // ---- pmp_resblock_*: dense -> blocked, the block, blocked -> dense
    void resblock_forward(const BlockShape &s, const RbCall &q)
    {
        const Block b = block_of(s, q.in, nullptr, 0);
        Tensor x = blocked(q.in[q.X], nullptr, 0, b.cin), t = act(b.cop()), y = act(b.cop());
        block_forward(b, x, t, y);
        dense(t, q.out[q.T_O], b.cout);
        dense(y, q.out[q.OUT_O], b.cout);
        for (Tensor *p : {&x, &t, &y}) release(*p);
    }

    // gu, x, t in THIS order, all three the call's own: block_backward writes the mask over t and releases x behind dW0.  The arena's
    // peak is then gu, x, t and gt with the packed w2 - at a trainer's sizes, to the byte, what the call needed when it converted x
    // only behind dW2 and kept a mask of its own (test_workspace_need_of_block_calls, profiles/train_workspace.txt).  With t in front
    // of x small shapes, where partial sums and packed weights dominate, need up to a fifth more.
    void resblock_backward(const BlockShape &s, const RbCall &q)
    {
        const Block b = block_of(s, q.in, q.out, 0);
        Tensor gu = blocked(q.in[q.G_OUT], q.in[q.OUT], 1, b.cout);              // g where out > 0
        Tensor x = blocked(q.in[q.X], nullptr, 0, b.cin), t = blocked(q.in[q.T], nullptr, 0, b.cout), dx{};
        block_backward(b, x, t, gu, q.out[q.G_X] ? &dx : nullptr);
        if (q.out[q.G_X]) dense(dx, q.out[q.G_X], b.cin);
        release(dx);
        release(gu);
    }

    // ---- pmp_trunk_*: a chain of blocks whose activations stay blocked, in the caller's d_saved between forward and backward
    void trunk_forward(const Chain &ch, const ChainPtrs &q)
    {
        const SavedLayout &lay = ch.lay;
        const int clast = lay.c[lay.nt - 1];
        Tensor x = view(lay, q.saved, 0);
        to_blocked(q.x, nullptr, 0, lay.c[0], x);
        for (int i = 0; i < ch.nblocks; ++i) {
            Tensor t = view(lay, q.saved, 2 * i + 1), y = view(lay, q.saved, 2 * i + 2);
            block_forward(block_of(ch.blocks[i], q.w, nullptr, i), x, t, y);
            x = y;
        }
        if (!ch.pool) dense(x, q.y, clast);
        else if (live()) check(launch_pool_to_dense(ps.stream, x.p, q.y, n, clast, pad_channels(clast), h, w), "pool_to_dense");
    }

    void trunk_backward(const Chain &ch, const ChainPtrs &q)
    {
        const SavedLayout &lay = ch.lay;
        const int L = ch.nblocks, clast = lay.c[2 * L];
        // the running gradient, g_out of block i behind its ReLU: the pool's backward and the last ReLU's in one pass over the dense g_y
        Tensor gu = act(pad_channels(clast));
        if (live())
            check(launch_grad_to_blocked(ps.stream, ch.pool, q.g_y, view(lay, q.saved, 2 * L).p, gu.p, n, clast, pad_channels(clast), h, w),
                  "grad_to_blocked");
        for (int i = L - 1; i >= 0; --i) {
            const Block b = block_of(ch.blocks[i], q.w, q.g_w, i);
            Tensor x = view(lay, q.saved, 2 * i), t = view(lay, q.saved, 2 * i + 1), dx{};
            if (i < L - 1 && live())             // gu holds block i + 1's g_x: this block's g_out, masked in place
                check(launch_blocked_relu(ps.stream, 1, gu.p, view(lay, q.saved, 2 * i + 2).p, gu.p, n, b.cop(), h, w), "blocked_relu");
            block_backward(b, x, t, gu, i > 0 || q.g_x ? &dx : nullptr);
            release(gu);
            gu = dx;
        }
        if (q.g_x) dense(gu, q.g_x, lay.c[0]);
        release(gu);
    }

    // ---- pmp_qtail_*: q3, the multi-scale pool, q4, q5 and its pool, q6 on its own map (qtail_train.hip); d_saved as a trunk's
    void qstep(int step, const float *a, const float *b, const float *c3, float *out, float *out2, int hh, int ww)
    {
        if (live()) check(launch_qtail_step(ps.stream, step, a, b, c3, out, out2, n, hh, ww), "qtail_step");
    }
    void qtail_forward(const Chain &ch, const ChainPtrs &q)
    {
        const SavedLayout &lay = ch.lay;
        const int H = h, W = w;
        Tensor s[QTAIL_SAVED];
        for (int i = 0; i < QTAIL_SAVED; ++i) s[i] = view(lay, q.saved, i);
        to_blocked(q.x, nullptr, 0, 64, s[0]);
        block_forward(block_of(ch.blocks[0], q.w, q.g_w, 0), s[0], s[1], s[2]);
        Tensor x6 = act(128);
        qstep(QT_MULTIPOOL, s[2].p, nullptr, nullptr, x6.p, nullptr, H, W);
        block_forward(block_of(ch.blocks[1], q.w, q.g_w, 1), x6, s[3], s[4]);
        release(x6);
        block_forward(block_of(ch.blocks[2], q.w, q.g_w, 2), s[4], s[5], s[6]);
        h = lay.h2; w = lay.w2;                                                  // q6's map
        Tensor x8 = act(32), region = act(16);
        qstep(QT_POOL_EMBED, s[6].p, nullptr, nullptr, x8.p, region.p, H, W);
        block_forward(block_of(ch.blocks[3], q.w, q.g_w, 3), x8, s[7], s[8], &region);
        qstep(QT_CROP_DENSE, s[8].p, nullptr, nullptr, q.y, nullptr, H, W);
        release(region);
        release(x8);
        h = H; w = W;
    }

    void qtail_backward(const Chain &ch, const ChainPtrs &q)
    {
        const SavedLayout &lay = ch.lay;
        const int H = h, W = w;
        Tensor s[QTAIL_SAVED];
        for (int i = 0; i < QTAIL_SAVED; ++i) s[i] = view(lay, q.saved, i);
        h = lay.h2; w = lay.w2;
        Tensor gu = act(16), x8 = act(32), dx{}, dx_hi{};
        qstep(QT_EMBED_GRAD, q.g_y, s[8].p, nullptr, gu.p, nullptr, H, W);
        qstep(QT_POOL_EMBED, s[6].p, nullptr, nullptr, x8.p, nullptr, H, W);
        block_backward(block_of(ch.blocks[3], q.w, q.g_w, 3), x8, s[7], gu, &dx);                 // x8 is the call's own: released behind dW0
        release(gu);
        h = H; w = W;
        gu = act(32);
        qstep(QT_POOL_BACK, dx.p, s[6].p, nullptr, gu.p, nullptr, H, W);
        release(dx);
        block_backward(block_of(ch.blocks[2], q.w, q.g_w, 2), s[4], s[5], gu, &dx);
        release(gu);
        gu = dx;
        if (live()) check(launch_blocked_relu(ps.stream, 1, gu.p, s[4].p, gu.p, n, 32, H, W), "blocked_relu");
        Tensor x6 = act(128);
        qstep(QT_MULTIPOOL, s[2].p, nullptr, nullptr, x6.p, nullptr, H, W);
        block_backward(block_of(ch.blocks[1], q.w, q.g_w, 1), x6, s[3], gu, &dx, &dx_hi);
        release(gu);
        gu = act(32);
        qstep(QT_MULTIPOOL_BACK, dx.p, dx_hi.p, s[2].p, gu.p, nullptr, H, W);
        release(dx);
        release(dx_hi);
        dx = Tensor{};
        block_backward(block_of(ch.blocks[0], q.w, q.g_w, 0), s[0], s[1], gu, q.g_x ? &dx : nullptr);
        if (q.g_x) dense(dx, q.g_x, 64);
        release(dx);
        release(gu);
    }

    // ---- pmp_stem_*: dense in and out (stem_train.hip); the arena holds the packed weights, or the partial sums of g_w and g_b
    void stem(const StemTrainArgs &q, bool backward)
    {
        Tensor scratch = floats(backward ? stem_partial_floats(q.N, q.H, q.W, q.cin, q.K) : stem_packed_floats(q.cin, q.K));
        if (live()) check(backward ? launch_stem_wgrad(ps.stream, q, scratch.p) : launch_stem_forward(ps.stream, q, scratch.p), "stem");
        release(scratch);
        if (backward && q.g_x && live()) check(launch_stem_dgrad(ps.stream, q), "stem_dgrad");
    }

    // ---- pmp_head_*: dense in and out (head_train.hip); the arena holds the partial sums of g_w and g_b
    void head(const HeadTrainArgs &q, bool backward)
    {
        if (!backward) {
            if (live()) check(launch_head_forward(ps.stream, q), "head_forward");
            return;
        }
        Tensor part = floats(head_partial_floats(q.N, q.H, q.W, q.cin, q.cout));
        if (live()) check(launch_head_backward(ps.stream, q, part.p), "head_backward");
        release(part);
    }
};

int run_train(pmp_ctx *c, int n, int h, int w, const std::function<void(TrainGraph &)> &body)
{
    Pass ps{c->stream, c->ws, PMP_PRECISION_F32, /*taps*/ false, /*cal*/ false, /*caller*/ true};
    return run_graph(c, ps, [&] {
        TrainGraph g{c, ps, n, h, w};
        body(g);
        return g.rc;
    });
}

// Every entry point, before it runs.  why: the call's *_refused of train_check.h, so nothing is launched or written before the checks
// pass.  Then, like pmp_train_loss_device, whatever is in flight on the context is made final (nothing, for a trainer's own tensors)
int admit(pmp_ctx *c, const char *fn, const char *why)
{
    CHECK_CTX(c);
    if (why) return set_err(c, PMP_E_INVALID, std::string(fn) + ": " + why);
    return settle_before_host_call(c);
}

int rb_run(pmp_ctx *c, const pmp_rb_shape &s, const RbCall &q)
{
    const BlockShape b{s.cin, s.cout, s.k};
    return run_train(c, s.n, s.h, s.w, [&](TrainGraph &g) { q.backward ? g.resblock_backward(b, q) : g.resblock_forward(b, q); });
}

// The host forms: every tensor through a staging buffer of the context, the device form in between
int rb_staged(pmp_ctx *c, const pmp_rb_shape &s, const RbCall &q, const std::vector<Span> &ins, const std::vector<Span> &outs)
{
    int rc;
    RbCall dq{q.backward, {}, {}};
    for (size_t i = 0; i < ins.size(); ++i) {
        if (!ins[i].p) continue;
        if ((rc = h2d(c, c->d_rb[i], ins[i].p, ins[i].bytes))) return rc;
        dq.in[i] = (const float *)c->d_rb[i].p;
    }
    for (size_t i = 0; i < outs.size(); ++i) {
        DevBuf &d = c->d_rb[ins.size() + i];
        if (!outs[i].p) continue;
        if ((rc = ensure(c, d, outs[i].bytes))) return rc;
        if (c->poison) {                               // pmp_debug_poison_workspace: the kernels must write every byte they hand back
            const hipError_t e = hipMemsetAsync(d.p, poison_byte(c), outs[i].bytes, c->stream);
            if (e != hipSuccess) return hip_fail(c, e, "poison resblock staging");
        }
        dq.out[i] = (float *)d.p;
    }
    if ((rc = rb_run(c, s, dq))) return rc;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].p && (rc = d2h(c, const_cast<void *>(outs[i].p), dq.out[i], outs[i].bytes))) return rc;
    return sync_idle(c);
}

// pmp_resblock_forward, _backward and their _device forms
int rb_entry(pmp_ctx *c, const char *fn, bool device, const pmp_rb_shape *s, const RbCall &q)
{
    std::vector<Span> ins, outs;
    if (int rc = admit(c, fn, rb_refused(s, q, device, ins, outs))) return rc;
    return device ? rb_run(c, *s, q) : rb_staged(c, *s, q, ins, outs);
}

int rb_forward(pmp_ctx *c, const char *fn, bool device, const pmp_rb_shape *s, const float *x, const float *w0, const float *w2,
               const float *wsc, float *t, float *out)
{
    return rb_entry(c, fn, device, s, RbCall{false, {w0, w2, wsc, x}, {t, out}});
}

int rb_backward(pmp_ctx *c, const char *fn, bool device, const pmp_rb_shape *s, const float *x, const float *t, const float *out,
                const float *w0, const float *w2, const float *wsc, const float *g_out, float *g_x, float *g_w0, float *g_w2, float *g_wsc)
{
    return rb_entry(c, fn, device, s, RbCall{true, {w0, w2, wsc, x, t, out, g_out}, {g_w0, g_w2, g_wsc, g_x}});
}

// pmp_trunk_* and pmp_qtail_*: _forward_device (dir 0), _backward_device (1), each with its body, and _unpack_device (2), which has none.
// ch holds what tells the chains apart: layout, blocks, n, h, w, and which saved tensors lie on the half map: QT_CROP_DENSE unpacks those
using ChainBody = void (TrainGraph::*)(const Chain &, const ChainPtrs &);

int chain_entry(pmp_ctx *c, const char *fn, const Chain &ch, const ChainPtrs &q, int dir, ChainBody body = nullptr, int index = 0)
{
    std::vector<Span> ins, outs;
    if (int rc = admit(c, fn, chain_refused(ch, q, dir, index, ins, outs))) return rc;
    const SavedLayout &lay = ch.lay;
    if (dir == 2) {
        const float *src = view(lay, q.saved, index).p;
        const hipError_t e = lay.half[index]
                                 ? launch_qtail_step(c->stream, QT_CROP_DENSE, src, nullptr, nullptr, q.dense, nullptr, lay.n, lay.h, lay.w)
                                 : launch_blocked_to_dense(c->stream, src, q.dense, lay.n, lay.c[index], pad_channels(lay.c[index]), lay.h, lay.w);
        return e == hipSuccess ? PMP_OK : hip_fail(c, e, ch.unpack_name);
    }
    return run_train(c, lay.n, lay.h, lay.w, [&](TrainGraph &g) { (g.*body)(ch, q); });
}

int64_t saved_bytes(const Chain &ch) { return ch.refused ? PMP_E_INVALID : (int64_t)ch.lay.off[ch.lay.nt]; }

// pmp_stem_forward_device (backward = false) and pmp_stem_backward_device
int stem_entry(pmp_ctx *c, const char *fn, const pmp_stem_shape *s, bool backward, const StemPtrs &t)
{
    if (int rc = admit(c, fn, stem_refused(s, t, backward))) return rc;
    StemTrainArgs q{};
    q.N = s->n; q.H = s->h; q.W = s->w; q.cin = s->cin; q.K = s->k; q.split = s->split;
    q.x = t.x; q.y = t.y; q.g_y = t.g_y; q.y_out = t.y_out; q.g_x = t.g_x;
    for (int j = 0; j < (s->split ? 3 : 1); ++j) {
        q.w[j] = t.w[j];
        if (!backward) q.b[j] = t.b[j];
        else { q.g_w[j] = t.g_w[j]; q.g_b[j] = t.g_b[j]; }
    }
    return run_train(c, s->n, s->h, s->w, [&](TrainGraph &g) { g.stem(q, backward); });
}

// pmp_head_forward_device (backward = false) and pmp_head_backward_device
int head_entry(pmp_ctx *c, const char *fn, const pmp_head_shape *s, bool backward, const HeadPtrs &t)
{
    if (int rc = admit(c, fn, head_refused(s, t, backward))) return rc;
    const HeadTrainArgs q{s->n, s->h, s->w, s->cin, s->cout, s->up_q, s->up_y, t.x, t.w, t.b, t.prev, t.q, t.y, t.att, t.g_y, t.g_att,
                          t.g_x, t.g_w, t.g_b, t.g_q, t.g_prev};
    return run_train(c, s->n, s->h, s->w, [&](TrainGraph &g) { g.head(q, backward); });
}

// pmp_gate_forward_device and pmp_gate_backward_device
int gate_entry(pmp_ctx *c, const char *fn, int64_t count, bool backward, const float *x, const float *a, const float *g_y, const float *g_acc,
               float *o0, float *o1)
{
    if (int rc = admit(c, fn, gate_refused(count, backward, x, a, g_y, g_acc, o0, o1))) return rc;
    const hipError_t e = backward ? launch_gate_backward(c->stream, (size_t)count, x, a, g_y, g_acc, o0, o1)
                                  : launch_gate_forward(c->stream, (size_t)count, x, a, o0);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "gate");
}

// pmp_adam_step_device and, with rec, pmp_adam_step_guarded_device: the tensors, cut into entries of at most 2^30 floats, go out PMP_ADAM_TABLE entries to a launch
int adam_run(pmp_ctx *c, const pmp_adam_params &p, int ntensors, float *const *param, const float *const *grad, float *const *m,
             float *const *v, const int64_t *count, int64_t step, const pmp_guard_record *rec = nullptr)
{
    const double c1 = 1.0 - std::pow(p.beta1, (double)step), c2 = 1.0 - std::pow(p.beta2, (double)step);
    const AdamConsts k{(float)(1.0 - p.beta1), (float)p.beta2, (float)(1.0 - p.beta2), -(float)(p.lr / c1), (float)std::sqrt(c2), (float)p.eps};
    constexpr int64_t PART = (int64_t)1 << 30;
    AdamTable t;
    int nt = 0;
    const auto flush = [&] {
        const hipError_t e = nt ? launch_adam_step(c->stream, t, nt, k, rec) : hipSuccess;
        nt = 0;
        return e == hipSuccess ? PMP_OK : hip_fail(c, e, "adam_step");
    };
    for (int i = 0; i < ntensors; ++i)
        for (int64_t at = 0; at < count[i]; at += PART) {
            t.param[nt] = param[i] + at; t.grad[nt] = grad[i] + at; t.m[nt] = m[i] + at; t.v[nt] = v[i] + at;
            t.count[nt] = (unsigned)std::min(PART, count[i] - at);
            if (++nt == PMP_ADAM_TABLE)
                if (int rc = flush()) return rc;
        }
    return flush();
}

// pmp_grad_guard_device: the census PMP_ADAM_TABLE tensors to a launch, in the order given, the tiles numbered on across the launches;
// then the launch that adds the tiles' partials and writes the record
int grad_guard_run(pmp_ctx *c, const pmp_guard_params &p, int ntensors, const float *const *grad, const int64_t *count, void *scratch,
                   pmp_guard_record *rec, pmp_guard_state *st)
{
    const int64_t tiles = guard_tiles(ntensors, count);
    GuardTable t;
    int64_t tile0 = 0, in_table = 0;
    for (int i = 0, nt = 0; i < ntensors; ++i) {
        t.grad[nt] = grad[i]; t.count[nt] = (unsigned)count[i];
        in_table += (count[i] + GUARD_TILE_ELEMS - 1) / GUARD_TILE_ELEMS;
        if (++nt == PMP_ADAM_TABLE || i == ntensors - 1) {
            const hipError_t e = launch_grad_census(c->stream, t, nt, tile0, scratch, tiles);
            if (e != hipSuccess) return hip_fail(c, e, "grad_census");
            tile0 += in_table;
            in_table = nt = 0;
        }
    }
    const hipError_t e = launch_grad_guard_finish(c->stream, scratch, tiles, p, rec, st);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "grad_guard_finish");
}

// pmp_grad_pack_device: PMP_ADAM_TABLE tensors to a launch, in the order given
int grad_pack_run(pmp_ctx *c, int ntensors, const float *const *grad, const int64_t *count, float *bucket)
{
    GradPackTable t;
    int64_t at = 0;
    for (int i = 0, nt = 0; i < ntensors; ++i) {
        t.grad[nt] = grad[i]; t.at[nt] = at; t.count[nt] = (unsigned)count[i];
        at += (count[i] + 3) & ~(int64_t)3;
        if (++nt == PMP_ADAM_TABLE || i == ntensors - 1) {
            const hipError_t e = launch_grad_pack(c->stream, t, nt, bucket);
            if (e != hipSuccess) return hip_fail(c, e, "grad_pack");
            nt = 0;
        }
    }
    return PMP_OK;
}

}  // namespace

extern "C" {

int64_t pmp_grad_bucket_floats(int ntensors, const int64_t *count, int64_t *offset) { return grad_bucket_floats(ntensors, count, offset); }

int pmp_grad_pack_device(pmp_ctx *c, int ntensors, const float *const *grad, const int64_t *count, float *d_bucket)
{
    if (int rc = admit(c, "pmp_grad_pack_device", grad_pack_refused(ntensors, grad, count, d_bucket))) return rc;
    return grad_pack_run(c, ntensors, grad, count, d_bucket);
}

int pmp_grad_sum_device(pmp_ctx *c, int nsrc, const float *const *d_src, int64_t count, float *d_dst)
{
    if (int rc = admit(c, "pmp_grad_sum_device", grad_sum_refused(nsrc, d_src, count, d_dst))) return rc;
    if (nsrc == 1 && d_src[0] == d_dst) return PMP_OK;
    GradSumTable t;
    for (int j = 0; j < nsrc; ++j) t.src[j] = d_src[j];
    const hipError_t e = launch_grad_sum(c->stream, t, nsrc, count / 4, d_dst);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "grad_sum");
}

int pmp_batch_gather_device(pmp_ctx *c, const pmp_batch_src *src, const int64_t *d_index, int64_t n, const pmp_batch_dst *dst, int32_t *d_status)
{
    if (int rc = admit(c, "pmp_batch_gather_device", gather_refused(src, d_index, n, dst, d_status))) return rc;
    const hipError_t e = launch_batch_gather(c->stream, *src, d_index, (int)n, *dst, d_status);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "batch_gather");
}

int pmp_adam_step_device(pmp_ctx *c, const pmp_adam_params *p, int ntensors, float *const *param, const float *const *grad, float *const *m,
                         float *const *v, const int64_t *count, int64_t step)
{
    if (int rc = admit(c, "pmp_adam_step_device", adam_refused(p, ntensors, param, grad, m, v, count, step))) return rc;
    return adam_run(c, *p, ntensors, param, grad, m, v, count, step);
}

int64_t pmp_grad_guard_scratch_bytes(int ntensors, const int64_t *count) { return guard_scratch_bytes(ntensors, count); }

int pmp_grad_guard_device(pmp_ctx *c, const pmp_guard_params *p, int ntensors, const float *const *grad, const int64_t *count, void *d_scratch,
                          pmp_guard_record *d_record, pmp_guard_state *d_state)
{
    if (int rc = admit(c, "pmp_grad_guard_device", guard_refused(p, ntensors, grad, count, d_scratch, d_record, d_state))) return rc;
    return grad_guard_run(c, *p, ntensors, grad, count, d_scratch, d_record, d_state);
}

int pmp_adam_step_guarded_device(pmp_ctx *c, const pmp_adam_params *p, int ntensors, float *const *param, const float *const *grad,
                                 float *const *m, float *const *v, const int64_t *count, int64_t step, const pmp_guard_record *d_record)
{
    if (int rc = admit(c, "pmp_adam_step_guarded_device", adam_guarded_refused(p, ntensors, param, grad, m, v, count, step, d_record))) return rc;
    return adam_run(c, *p, ntensors, param, grad, m, v, count, step, d_record);
}

int pmp_head_forward_device(pmp_ctx *c, const pmp_head_shape *s, const float *x, const float *w, const float *b, const float *prev,
                            const float *q, float *y, float *att)
{
    return head_entry(c, "pmp_head_forward_device", s, false, HeadPtrs{x, w, b, prev, q, y, att});
}

int pmp_head_backward_device(pmp_ctx *c, const pmp_head_shape *s, const float *x, const float *w, const float *g_y, const float *g_att,
                             float *g_x, float *g_w, float *g_b, float *g_q, float *g_prev)
{
    HeadPtrs t{};
    t.x = x; t.w = w; t.g_y = g_y; t.g_att = g_att; t.g_x = g_x; t.g_w = g_w; t.g_b = g_b; t.g_q = g_q; t.g_prev = g_prev;
    return head_entry(c, "pmp_head_backward_device", s, true, t);
}

int pmp_gate_forward_device(pmp_ctx *c, int64_t count, const float *x, const float *a, float *y)
{
    return gate_entry(c, "pmp_gate_forward_device", count, false, x, a, nullptr, nullptr, y, nullptr);
}

int pmp_gate_backward_device(pmp_ctx *c, int64_t count, const float *x, const float *a, const float *g_y, const float *g_acc, float *g_x,
                             float *g_a)
{
    return gate_entry(c, "pmp_gate_backward_device", count, true, x, a, g_y, g_acc, g_x, g_a);
}

int pmp_stem_forward_device(pmp_ctx *c, const pmp_stem_shape *s, const float *x, const float *const w[3], const float *const b[3], float *y)
{
    StemPtrs t{};
    t.x = x; t.w = w; t.b = b; t.y_out = y;
    return stem_entry(c, "pmp_stem_forward_device", s, false, t);
}

int pmp_stem_backward_device(pmp_ctx *c, const pmp_stem_shape *s, const float *x, const float *y, const float *const w[3], const float *g_y,
                             float *g_x, float *const g_w[3], float *const g_b[3])
{
    StemPtrs t{};
    t.x = x; t.y = y; t.w = w; t.g_y = g_y; t.g_x = g_x; t.g_w = g_w; t.g_b = g_b;
    return stem_entry(c, "pmp_stem_backward_device", s, true, t);
}

int64_t pmp_qtail_saved_bytes(const pmp_qtail_shape *s) { return saved_bytes(chain_of(s)); }

int pmp_qtail_forward_device(pmp_ctx *c, const pmp_qtail_shape *s, const float *x4, const float *const *w, void *saved, float *x9)
{
    ChainPtrs q{};
    q.x = x4; q.w = w; q.saved = saved; q.y = x9;
    return chain_entry(c, "pmp_qtail_forward_device", chain_of(s), q, 0, &TrainGraph::qtail_forward);
}

int pmp_qtail_backward_device(pmp_ctx *c, const pmp_qtail_shape *s, const void *saved, const float *const *w, const float *g_x9, float *g_x4,
                              float *const *g_w)
{
    ChainPtrs q{};
    q.saved = saved; q.w = w; q.g_y = g_x9; q.g_x = g_x4; q.g_w = g_w;
    return chain_entry(c, "pmp_qtail_backward_device", chain_of(s), q, 1, &TrainGraph::qtail_backward);
}

int pmp_qtail_unpack_device(pmp_ctx *c, const pmp_qtail_shape *s, const void *saved, int index, float *dense)
{
    ChainPtrs q{};
    q.saved = saved; q.dense = dense;
    return chain_entry(c, "pmp_qtail_unpack_device", chain_of(s), q, 2, nullptr, index);
}

int64_t pmp_trunk_saved_bytes(const pmp_trunk_shape *s) { return saved_bytes(chain_of(s)); }

int pmp_trunk_forward_device(pmp_ctx *c, const pmp_trunk_shape *s, const float *x, const float *const *w, void *saved, float *y)
{
    ChainPtrs q{};
    q.x = x; q.w = w; q.saved = saved; q.y = y;
    return chain_entry(c, "pmp_trunk_forward_device", chain_of(s), q, 0, &TrainGraph::trunk_forward);
}

int pmp_trunk_backward_device(pmp_ctx *c, const pmp_trunk_shape *s, const void *saved, const float *const *w, const float *g_y, float *g_x,
                              float *const *g_w)
{
    ChainPtrs q{};
    q.saved = saved; q.w = w; q.g_y = g_y; q.g_x = g_x; q.g_w = g_w;
    return chain_entry(c, "pmp_trunk_backward_device", chain_of(s), q, 1, &TrainGraph::trunk_backward);
}

int pmp_trunk_unpack_device(pmp_ctx *c, const pmp_trunk_shape *s, const void *saved, int index, float *dense)
{
    ChainPtrs q{};
    q.saved = saved; q.dense = dense;
    return chain_entry(c, "pmp_trunk_unpack_device", chain_of(s), q, 2, nullptr, index);
}

int pmp_resblock_forward_device(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *w0, const float *w2, const float *wsc,
                                float *t, float *out)
{
    return rb_forward(c, "pmp_resblock_forward_device", true, s, x, w0, w2, wsc, t, out);
}

int pmp_resblock_forward(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *w0, const float *w2, const float *wsc, float *t,
                         float *out)
{
    return rb_forward(c, "pmp_resblock_forward", false, s, x, w0, w2, wsc, t, out);
}

int pmp_resblock_backward_device(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *t, const float *out, const float *w0,
                                 const float *w2, const float *wsc, const float *g_out, float *g_x, float *g_w0, float *g_w2, float *g_wsc)
{
    return rb_backward(c, "pmp_resblock_backward_device", true, s, x, t, out, w0, w2, wsc, g_out, g_x, g_w0, g_w2, g_wsc);
}

int pmp_resblock_backward(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *t, const float *out, const float *w0,
                          const float *w2, const float *wsc, const float *g_out, float *g_x, float *g_w0, float *g_w2, float *g_wsc)
{
    return rb_backward(c, "pmp_resblock_backward", false, s, x, t, out, w0, w2, wsc, g_out, g_x, g_w0, g_w2, g_wsc);
}

}  // extern "C"
