// api_train.cpp — one Model_QBD.ResidualBlock, forward and backward, for a trainer (include/pmp.h: pmp_resblock_forward / _backward),
// and a trunk of them whose activations stay blocked between the blocks and between the two directions (pmp_trunk_*; trunk_glue.hip).
// The caller's dense tensors go through the blocked layout in the context's workspace arena; the convolutions are conv_mfma.hip's
// (the data gradients are ordinary convolutions with mirrored, transposed weights), the weight gradients conv_wgrad.hip's.  Always
// the exact fp32 MFMA datapath: the Pass says so, whatever pmp_set_precision chose for inference.
#include <initializer_list>

#include "pmp_host.h"

using namespace pmp;

namespace {

int pad_channels(int c) { return c <= 16 ? 16 : c <= 32 ? 32 : 64; }      // the channel counts the convolution kernels have

struct RbPtrs {                        // everything either direction touches; what a direction does not use stays null
    const float *x, *t_in, *out_in, *w0, *w2, *wsc, *g_out;
    float *t, *out, *g_x, *g_w0, *g_w2, *g_wsc;
};

struct Tensor { float *p; size_t off, bytes; };

// The graph of one call on a Pass: run_graph() runs it twice, measuring (no launches, null pointers) and live
struct TrainGraph {
    pmp_ctx *c;
    Pass &ps;
    const pmp_rb_shape &s;
    int rc = PMP_OK;
    int cip() const { return pad_channels(s.cin); }
    int cop() const { return pad_channels(s.cout); }
    bool live() const { return !ps.arena.measuring && rc == PMP_OK; }
    bool check(hipError_t e, const char *what)
    {
        if (e != hipSuccess && rc == PMP_OK) rc = hip_fail(c, e, what);
        return rc == PMP_OK;
    }
    Tensor floats(size_t n)
    {
        const size_t off = ps.arena.take(n * sizeof(float));
        return Tensor{ps.arena.ptr(off), off, n * sizeof(float)};
    }
    Tensor act(int cp) { return floats((size_t)s.n * cp * s.h * s.w); }
    void release(Tensor &t)
    {
        if (t.bytes) ps.arena.give(t.off, t.bytes);
        t.bytes = 0;
    }
    Tensor blocked(const float *src, const float *m, int mode, int C, int cp)
    {
        Tensor t = act(cp);
        if (live()) check(launch_dense_to_blocked(ps.stream, src, m, mode, t.p, s.n, C, cp, s.h, s.w), "dense_to_blocked");
        return t;
    }
    void dense(const Tensor &t, float *dst, int C, int cp)
    {
        if (live()) check(launch_blocked_to_dense(ps.stream, t.p, dst, s.n, C, cp, s.h, s.w), "blocked_to_dense");
    }
    // w [cout][cin][k][k] -> the fragments of the convolution that reads 16 CB channels and writes 16 NT
    Tensor packed(const float *w, int cout, int cin, int k, int nt_ch, int cb_ch, bool flip_t)
    {
        Tensor t = floats((size_t)(cb_ch / 16) * k * k * (nt_ch / 16) * 256);
        if (live()) check(launch_pack_mfma(ps.stream, w, t.p, cout, cin, k, nt_ch / 16, cb_ch / 16, flip_t ? 1 : 0), "pack_mfma");
        return t;
    }
    void conv(const Tensor &x, int cin_p, const Tensor &w, int k, const Tensor *x_sc, int csc_p, const Tensor *w_sc, const Tensor *res,
              const Tensor *gate, bool relu, Tensor &out, int cout_p)
    {
        if (!live()) return;
        ConvMfmaArgs a{};
        a.x = x.p; a.w = w.p; a.out = out.p;
        if (x_sc) { a.x_sc = x_sc->p; a.w_sc = w_sc->p; a.Csc = csc_p; }
        if (res) a.res = res->p;
        if (gate) a.gate = gate->p;
        a.N = s.n; a.H = s.h; a.W = s.w; a.Cin = cin_p; a.Cout = cout_p; a.KH = a.KW = k; a.relu = relu ? 1 : 0;
        check(launch_conv_mfma(ps.stream, a), "conv_mfma");
    }
    void wgrad(const Tensor &a, int ca_p, const Tensor &g, int cg_p, int k, float *dw, int cout, int cin)
    {
        Tensor part = floats(wgrad_partial_floats(s.n, s.h, s.w, ca_p, cg_p, k));
        if (live()) check(launch_wgrad(ps.stream, a.p, g.p, s.n, s.h, s.w, ca_p, cg_p, k, part.p, dw, cout, cin), "wgrad");
        release(part);
    }

    // t = relu(conv0(x)), out = relu(conv2(t) + sc(x))  (Model_QBD.py:40-44): the launches of Graph::rb() on the fp32 datapath
    int forward(const RbPtrs &q)
    {
        const bool sc = s.cin != s.cout;
        Tensor x = blocked(q.x, nullptr, 0, s.cin, cip());
        Tensor w0 = packed(q.w0, s.cout, s.cin, s.k, cop(), cip(), false), w2 = packed(q.w2, s.cout, s.cout, s.k, cop(), cop(), false);
        Tensor wsc = sc ? packed(q.wsc, s.cout, s.cin, 1, cop(), cip(), false) : Tensor{};
        Tensor t = act(cop()), y = act(cop());
        conv(x, cip(), w0, s.k, nullptr, 0, nullptr, nullptr, nullptr, true, t, cop());
        conv(t, cop(), w2, s.k, sc ? &x : nullptr, cip(), sc ? &wsc : nullptr, sc ? nullptr : &x, nullptr, true, y, cop());
        dense(t, q.t, s.cout, cop());
        dense(y, q.out, s.cout, cop());
        for (Tensor *b : {&x, &w0, &w2, &wsc, &t, &y}) release(*b);
        return rc;
    }

    // The same two launches for a block of a trunk: blocked x in, blocked t and y out, all three the caller's (pmp_trunk_*: d_saved)
    int forward_blocked(const RbPtrs &q, const Tensor &x, Tensor &t, Tensor &y)
    {
        const bool sc = s.cin != s.cout;
        Tensor w0 = packed(q.w0, s.cout, s.cin, s.k, cop(), cip(), false), w2 = packed(q.w2, s.cout, s.cout, s.k, cop(), cop(), false);
        Tensor wsc = sc ? packed(q.wsc, s.cout, s.cin, 1, cop(), cip(), false) : Tensor{};
        conv(x, cip(), w0, s.k, nullptr, 0, nullptr, nullptr, nullptr, true, t, cop());
        conv(t, cop(), w2, s.k, sc ? &x : nullptr, cip(), sc ? &wsc : nullptr, sc ? nullptr : &x, nullptr, true, y, cop());
        for (Tensor *b : {&w0, &w2, &wsc}) release(*b);
        return rc;
    }

    // include/pmp.h: gu, dW2, dWsc, gt, dW0, dx in that order
    int backward(const RbPtrs &q)
    {
        const bool sc = s.cin != s.cout;
        Tensor gu = blocked(q.g_out, q.out_in, 1, s.cout, cop());                // g where out > 0
        Tensor t = blocked(q.t_in, nullptr, 0, s.cout, cop());
        wgrad(t, cop(), gu, cop(), s.k, q.g_w2, s.cout, s.cout);
        release(t);
        Tensor x = blocked(q.x, nullptr, 0, s.cin, cip());
        if (sc) wgrad(x, cip(), gu, cop(), 1, q.g_wsc, s.cout, s.cin);
        Tensor mask = blocked(q.t_in, nullptr, 2, s.cout, cop());                // [t > 0], the convolution's gate
        Tensor w2t = packed(q.w2, s.cout, s.cout, s.k, cop(), cop(), true);
        Tensor gt = act(cop());
        conv(gu, cop(), w2t, s.k, nullptr, 0, nullptr, nullptr, &mask, false, gt, cop());
        release(mask);
        release(w2t);
        wgrad(x, cip(), gt, cop(), s.k, q.g_w0, s.cout, s.cin);
        release(x);
        if (q.g_x) {
            Tensor w0t = packed(q.w0, s.cout, s.cin, s.k, cip(), cop(), true);
            Tensor wsct = sc ? packed(q.wsc, s.cout, s.cin, 1, cip(), cop(), true) : Tensor{};
            Tensor dx = act(cip());
            conv(gt, cop(), w0t, s.k, sc ? &gu : nullptr, cop(), sc ? &wsct : nullptr, sc ? nullptr : &gu, nullptr, false, dx, cip());
            dense(dx, q.g_x, s.cin, cip());
            for (Tensor *b : {&w0t, &wsct, &dx}) release(*b);
        }
        release(gt);
        release(gu);
        return rc;
    }

    // backward()'s steps behind gu, in its order, for a block of a trunk: blocked x and t (the caller's) and gu in; the weight
    // gradients dense out; the data gradient, where dx is asked for, as a blocked tensor of the arena that the caller releases
    int backward_blocked(const RbPtrs &q, const Tensor &x, const Tensor &t, const Tensor &gu, Tensor *dx)
    {
        const bool sc = s.cin != s.cout;
        wgrad(t, cop(), gu, cop(), s.k, q.g_w2, s.cout, s.cout);
        if (sc) wgrad(x, cip(), gu, cop(), 1, q.g_wsc, s.cout, s.cin);
        Tensor mask = act(cop());                                                // [t > 0], the convolution's gate
        if (live()) check(launch_blocked_relu(ps.stream, 2, t.p, nullptr, mask.p, s.n, cop(), s.h, s.w), "blocked_relu");
        Tensor w2t = packed(q.w2, s.cout, s.cout, s.k, cop(), cop(), true);
        Tensor gt = act(cop());
        conv(gu, cop(), w2t, s.k, nullptr, 0, nullptr, nullptr, &mask, false, gt, cop());
        release(mask);
        release(w2t);
        wgrad(x, cip(), gt, cop(), s.k, q.g_w0, s.cout, s.cin);
        if (dx) {
            Tensor w0t = packed(q.w0, s.cout, s.cin, s.k, cip(), cop(), true);
            Tensor wsct = sc ? packed(q.wsc, s.cout, s.cin, 1, cip(), cop(), true) : Tensor{};
            *dx = act(cip());
            conv(gt, cop(), w0t, s.k, sc ? &gu : nullptr, cop(), sc ? &wsct : nullptr, sc ? nullptr : &gu, nullptr, false, *dx, cip());
            release(w0t);
            release(wsct);
        }
        release(gt);
        return rc;
    }
};

struct Span { const void *p; size_t bytes; };

bool overlaps(const Span &a, const Span &b)
{
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}

// Every check of pmp_resblock_*: nothing is launched or written before it passes.  device: the pointers are the GPU's and must be
// 4-byte aligned.  ins / outs come back as the spans of the tensors the call reads and writes (a null g_x is no output).
int rb_check(pmp_ctx *c, const char *fn, const pmp_rb_shape *s, const RbPtrs &q, bool backward, bool device, std::vector<Span> &ins,
             std::vector<Span> &outs)
{
    const std::string f(fn);
    if (!s) return set_err(c, PMP_E_INVALID, f + ": null shape");
    if (s->n < 1 || s->n > 256 || s->h < 16 || s->h > 256 || (s->h & 15) || s->w < 16 || s->w > 256 || (s->w & 15) || s->cin < 1 || s->cin > 64 ||
        s->cout < 1 || s->cout > 64 || (s->k != 3 && s->k != 5))
        return set_err(c, PMP_E_INVALID, f + ": unsupported shape (n 1..256, h and w multiples of 16 in 16..256, cin and cout 1..64, k 3 or 5)");
    const bool sc = s->cin != s->cout;
    const size_t px = (size_t)s->n * s->h * s->w * 4, kk = (size_t)s->k * s->k * 4;
    const size_t bx = px * s->cin, by = px * s->cout, bw0 = kk * s->cout * s->cin, bw2 = kk * s->cout * s->cout, bsc = (size_t)4 * s->cout * s->cin;
    if (!q.x || !q.w0 || !q.w2 || (backward ? (!q.t_in || !q.out_in || !q.g_out || !q.g_w0 || !q.g_w2) : (!q.t || !q.out)))
        return set_err(c, PMP_E_INVALID, f + ": null tensor");
    if ((q.wsc != nullptr) != sc || (backward && (q.g_wsc != nullptr) != sc))
        return set_err(c, PMP_E_INVALID, f + ": the shortcut's tensors are passed exactly when cin != cout");
    ins = {{q.x, bx}, {q.w0, bw0}, {q.w2, bw2}, {q.wsc, bsc}};
    if (backward) {
        ins.insert(ins.end(), {{q.t_in, by}, {q.out_in, by}, {q.g_out, by}});
        outs = {{q.g_x, bx}, {q.g_w0, bw0}, {q.g_w2, bw2}, {q.g_wsc, bsc}};
    } else
        outs = {{q.t, by}, {q.out, by}};
    for (size_t i = 0; i < outs.size(); ++i) {
        for (const Span &in : ins)
            if (overlaps(outs[i], in)) return set_err(c, PMP_E_INVALID, f + ": an output tensor overlaps an input");
        for (size_t j = 0; j < i; ++j)
            if (overlaps(outs[i], outs[j])) return set_err(c, PMP_E_INVALID, f + ": two output tensors overlap");
    }
    if (device) {
        uintptr_t bits = 0;
        for (const Span &t : ins) bits |= (uintptr_t)t.p;
        for (const Span &t : outs) bits |= (uintptr_t)t.p;
        if (bits & 3) return set_err(c, PMP_E_INVALID, f + "_device: every tensor must be 4-byte aligned");
    }
    return PMP_OK;
}

int rb_run(pmp_ctx *c, const pmp_rb_shape &s, const RbPtrs &q, bool backward)
{
    Pass ps{c->stream, c->ws, PMP_PRECISION_F32, /*taps*/ false, /*cal*/ false, /*caller*/ true};
    TrainGraph g{c, ps, s};
    return run_graph(c, ps, [&] { g.rc = PMP_OK; return backward ? g.backward(q) : g.forward(q); });
}

// The host forms: every tensor through a staging buffer of the context, the device form in between
int rb_staged(pmp_ctx *c, const pmp_rb_shape &s, const RbPtrs &q, bool backward, const std::vector<Span> &ins, const std::vector<Span> &outs)
{
    int rc;
    DevBuf *d = c->d_rb;
    std::vector<void *> dev;
    for (size_t i = 0; i < ins.size() + outs.size(); ++i) {
        const bool in = i < ins.size();
        const Span &t = in ? ins[i] : outs[i - ins.size()];
        dev.push_back(nullptr);
        if (!t.p) continue;
        if (in) rc = h2d(c, d[i], t.p, t.bytes);
        else {
            rc = ensure(c, d[i], t.bytes);
            if (rc == PMP_OK && c->poison) {           // pmp_debug_poison_workspace: the kernels must write every byte they hand back
                const hipError_t e = hipMemsetAsync(d[i].p, poison_byte(c), t.bytes, c->stream);
                if (e != hipSuccess) rc = hip_fail(c, e, "poison resblock staging");
            }
        }
        if (rc != PMP_OK) return rc;
        dev.back() = d[i].p;
    }
    auto in = [&](int i) { return (const float *)dev[i]; };
    auto out = [&](int i) { return (float *)dev[ins.size() + i]; };
    RbPtrs dq{};
    dq.x = in(0); dq.w0 = in(1); dq.w2 = in(2); dq.wsc = in(3);
    if (backward) { dq.t_in = in(4); dq.out_in = in(5); dq.g_out = in(6); dq.g_x = out(0); dq.g_w0 = out(1); dq.g_w2 = out(2); dq.g_wsc = out(3); }
    else { dq.t = out(0); dq.out = out(1); }
    if ((rc = rb_run(c, s, dq, backward))) return rc;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].p && (rc = d2h(c, const_cast<void *>(outs[i].p), dev[ins.size() + i], outs[i].bytes))) return rc;
    return sync(c);
}

int rb_entry(pmp_ctx *c, const char *fn, const pmp_rb_shape *s, const RbPtrs &q, bool backward, bool device)
{
    CHECK_CTX(c);
    std::vector<Span> ins, outs;
    int rc;
    if ((rc = rb_check(c, fn, s, q, backward, device, ins, outs))) return rc;
    // like pmp_train_loss_device: whatever is in flight on the context is made final first (nothing, for a trainer's own tensors)
    if ((rc = settle_before_host_call(c))) return rc;
    return device ? rb_run(c, *s, q, backward) : rb_staged(c, *s, q, backward, ins, outs);
}

// ---- pmp_trunk_*: a chain of blocks whose activations stay blocked, in the caller's d_saved between forward and backward

struct TrunkPtrs {
    const float *x, *g_y;
    const float *const *w;
    const char *saved_in;
    char *saved_out;
    float *y, *g_x;
    float *const *g_w;
};

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
    Tensor view(const void *saved, int i) const { return Tensor{(float *)((char *)saved + off[i]), 0, 0}; }     // bytes 0: not the arena's
};

pmp_rb_shape trunk_block(const pmp_trunk_shape &s, int i)
{
    return pmp_rb_shape{s.n, s.h, s.w, i ? s.cout[i - 1] : s.cin, s.cout[i], s.k[i]};
}

bool trunk_shape_ok(const pmp_trunk_shape *s)
{
    if (!s || s->n < 1 || s->n > 256 || s->h < 16 || s->h > 256 || (s->h & 15) || s->w < 16 || s->w > 256 || (s->w & 15) || s->cin < 1 ||
        s->cin > 64 || s->nblocks < 1 || s->nblocks > PMP_TRUNK_MAX_BLOCKS || (s->pool != 0 && s->pool != 1))
        return false;
    for (int i = 0; i < s->nblocks; ++i)
        if (s->cout[i] < 1 || s->cout[i] > 64 || (s->k[i] != 3 && s->k[i] != 5)) return false;
    return true;
}

RbPtrs trunk_block_ptrs(const TrunkPtrs &q, int i)
{
    RbPtrs b{};
    b.w0 = q.w[3 * i]; b.w2 = q.w[3 * i + 1]; b.wsc = q.w[3 * i + 2];
    if (q.g_w) { b.g_w0 = q.g_w[3 * i]; b.g_w2 = q.g_w[3 * i + 1]; b.g_wsc = q.g_w[3 * i + 2]; }
    return b;
}

int trunk_forward(pmp_ctx *c, Pass &ps, const pmp_trunk_shape &s, const TrunkPtrs &q)
{
    const TrunkLayout lay(s);
    const int L = s.nblocks, clast = s.cout[L - 1];
    Tensor x = lay.view(q.saved_out, 0);
    {
        const pmp_rb_shape b0 = trunk_block(s, 0);
        TrainGraph g{c, ps, b0};
        if (g.live()) g.check(launch_dense_to_blocked(ps.stream, q.x, nullptr, 0, x.p, s.n, s.cin, pad_channels(s.cin), s.h, s.w), "dense_to_blocked");
        if (g.rc) return g.rc;
    }
    for (int i = 0; i < L; ++i) {
        const pmp_rb_shape b = trunk_block(s, i);
        TrainGraph g{c, ps, b};
        Tensor t = lay.view(q.saved_out, 2 * i + 1), y = lay.view(q.saved_out, 2 * i + 2);
        if (g.forward_blocked(trunk_block_ptrs(q, i), x, t, y)) return g.rc;
        x = y;
        if (i == L - 1 && g.live()) {
            if (s.pool) g.check(launch_pool_to_dense(ps.stream, y.p, q.y, s.n, clast, pad_channels(clast), s.h, s.w), "pool_to_dense");
            else g.dense(y, q.y, clast, pad_channels(clast));
            if (g.rc) return g.rc;
        }
    }
    return PMP_OK;
}

int trunk_backward(pmp_ctx *c, Pass &ps, const pmp_trunk_shape &s, const TrunkPtrs &q)
{
    const TrunkLayout lay(s);
    const int L = s.nblocks, clast = s.cout[L - 1];
    Tensor gu{};                                 // the running gradient: g_out of block i behind its ReLU
    for (int i = L - 1; i >= 0; --i) {
        const pmp_rb_shape b = trunk_block(s, i);
        TrainGraph g{c, ps, b};
        const Tensor x = lay.view(q.saved_in, 2 * i), t = lay.view(q.saved_in, 2 * i + 1), out = lay.view(q.saved_in, 2 * i + 2);
        if (i == L - 1) {                        // the pool's backward and the last ReLU's in one pass over the dense g_y
            gu = g.act(g.cop());
            if (g.live())
                g.check(launch_grad_to_blocked(ps.stream, s.pool, q.g_y, out.p, gu.p, s.n, clast, g.cop(), s.h, s.w), "grad_to_blocked");
        } else if (g.live())                     // gu holds block i + 1's g_x: this block's g_out, masked in place
            g.check(launch_blocked_relu(ps.stream, 1, gu.p, out.p, gu.p, s.n, g.cop(), s.h, s.w), "blocked_relu");
        const bool want_dx = i > 0 || q.g_x;
        Tensor dx{};
        g.backward_blocked(trunk_block_ptrs(q, i), x, t, gu, want_dx ? &dx : nullptr);
        g.release(gu);
        if (i == 0 && want_dx) {
            g.dense(dx, q.g_x, s.cin, g.cip());
            g.release(dx);
        }
        if (g.rc) return g.rc;
        gu = dx;
    }
    return PMP_OK;
}

// Every check of pmp_trunk_forward_device (dir 0), _backward_device (1) and _unpack_device (2): nothing is launched before it passes
int trunk_check(pmp_ctx *c, const char *fn, const pmp_trunk_shape *s, const TrunkPtrs &q, int dir, int index, float *dense)
{
    const std::string f(fn);
    if (!trunk_shape_ok(s))
        return set_err(c, PMP_E_INVALID, f + ": null or unsupported shape (n 1..256, h and w multiples of 16 in 16..256, channels 1..64, k 3 or 5, "
                                             "1..8 blocks, pool 0 or 1)");
    const TrunkLayout lay(*s);
    const size_t px = (size_t)s->n * s->h * s->w * 4, py = s->pool ? px / 4 : px;
    const int L = s->nblocks;
    std::vector<Span> ins, outs;
    uintptr_t bits = 0;
    if (dir == 2) {
        if (!q.saved_in || !dense) return set_err(c, PMP_E_INVALID, f + ": null tensor");
        if (index < 0 || index >= lay.nt) return set_err(c, PMP_E_INVALID, f + ": index out of range (0 .. 2 * nblocks)");
        ins = {{q.saved_in, lay.off[lay.nt]}};
        outs = {{dense, px * lay.c[index]}};
    } else {
        if (!q.x && dir == 0) return set_err(c, PMP_E_INVALID, f + ": null tensor");
        if (!q.w || (dir ? !q.saved_in || !q.g_y || !q.g_w : !q.saved_out || !q.y)) return set_err(c, PMP_E_INVALID, f + ": null tensor");
        for (int i = 0; i < L; ++i) {
            const pmp_rb_shape b = trunk_block(*s, i);
            const size_t kk = (size_t)b.k * b.k * 4, bytes[3] = {kk * b.cout * b.cin, kk * b.cout * b.cout, (size_t)4 * b.cout * b.cin};
            for (int j = 0; j < 3; ++j) {
                const float *w = q.w[3 * i + j];
                const bool need = j < 2 || b.cin != b.cout;
                if (j < 2 && !w) return set_err(c, PMP_E_INVALID, f + ": null tensor");
                if ((w != nullptr) != need) return set_err(c, PMP_E_INVALID, f + ": a shortcut's tensors are passed exactly when its cin != cout");
                if (dir && (q.g_w[3 * i + j] != nullptr) != need)
                    return set_err(c, PMP_E_INVALID, f + ": d_g_w must be NULL exactly where d_w is");
                ins.push_back({w, bytes[j]});
                if (dir) outs.push_back({q.g_w[3 * i + j], bytes[j]});
            }
        }
        if (dir) {
            ins.insert(ins.end(), {{q.saved_in, lay.off[lay.nt]}, {q.g_y, py * s->cout[L - 1]}});
            outs.push_back({q.g_x, px * s->cin});
        } else {
            ins.push_back({q.x, px * s->cin});
            outs.insert(outs.end(), {{q.saved_out, lay.off[lay.nt]}, {q.y, py * s->cout[L - 1]}});
        }
    }
    for (size_t i = 0; i < outs.size(); ++i) {
        for (const Span &in : ins)
            if (overlaps(outs[i], in)) return set_err(c, PMP_E_INVALID, f + ": an output tensor overlaps an input");
        for (size_t j = 0; j < i; ++j)
            if (overlaps(outs[i], outs[j])) return set_err(c, PMP_E_INVALID, f + ": two output tensors overlap");
    }
    for (const Span &t : ins) bits |= (uintptr_t)t.p;
    for (const Span &t : outs) bits |= (uintptr_t)t.p;
    if (bits & 3) return set_err(c, PMP_E_INVALID, f + ": every tensor must be 4-byte aligned");
    if (((uintptr_t)q.saved_in | (uintptr_t)q.saved_out) & 15) return set_err(c, PMP_E_INVALID, f + ": d_saved must be 16-byte aligned");
    return PMP_OK;
}

int trunk_entry(pmp_ctx *c, const char *fn, const pmp_trunk_shape *s, const TrunkPtrs &q, int dir, int index = 0, float *dense = nullptr)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = trunk_check(c, fn, s, q, dir, index, dense))) return rc;
    if ((rc = settle_before_host_call(c))) return rc;
    if (dir == 2) {
        const TrunkLayout lay(*s);
        const hipError_t e = launch_blocked_to_dense(c->stream, lay.view(q.saved_in, index).p, dense, s->n, lay.c[index],
                                                     pad_channels(lay.c[index]), s->h, s->w);
        return e == hipSuccess ? PMP_OK : hip_fail(c, e, "blocked_to_dense");
    }
    Pass ps{c->stream, c->ws, PMP_PRECISION_F32, /*taps*/ false, /*cal*/ false, /*caller*/ true};
    return run_graph(c, ps, [&] { return dir ? trunk_backward(c, ps, *s, q) : trunk_forward(c, ps, *s, q); });
}

}  // namespace

extern "C" {

int64_t pmp_trunk_saved_bytes(const pmp_trunk_shape *s)
{
    if (!trunk_shape_ok(s)) return PMP_E_INVALID;
    const TrunkLayout lay(*s);
    return (int64_t)lay.off[lay.nt];
}

int pmp_trunk_forward_device(pmp_ctx *c, const pmp_trunk_shape *s, const float *x, const float *const *w, void *saved, float *y)
{
    TrunkPtrs q{};
    q.x = x; q.w = w; q.saved_out = (char *)saved; q.y = y;
    return trunk_entry(c, "pmp_trunk_forward_device", s, q, 0);
}

int pmp_trunk_backward_device(pmp_ctx *c, const pmp_trunk_shape *s, const void *saved, const float *const *w, const float *g_y, float *g_x,
                              float *const *g_w)
{
    TrunkPtrs q{};
    q.saved_in = (const char *)saved; q.w = w; q.g_y = g_y; q.g_x = g_x; q.g_w = g_w;
    return trunk_entry(c, "pmp_trunk_backward_device", s, q, 1);
}

int pmp_trunk_unpack_device(pmp_ctx *c, const pmp_trunk_shape *s, const void *saved, int index, float *dense)
{
    TrunkPtrs q{};
    q.saved_in = (const char *)saved;
    return trunk_entry(c, "pmp_trunk_unpack_device", s, q, 2, index, dense);
}

int pmp_resblock_forward_device(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *w0, const float *w2, const float *wsc,
                                float *t, float *out)
{
    RbPtrs q{};
    q.x = x; q.w0 = w0; q.w2 = w2; q.wsc = wsc; q.t = t; q.out = out;
    return rb_entry(c, "pmp_resblock_forward", s, q, false, true);
}

int pmp_resblock_forward(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *w0, const float *w2, const float *wsc, float *t,
                         float *out)
{
    RbPtrs q{};
    q.x = x; q.w0 = w0; q.w2 = w2; q.wsc = wsc; q.t = t; q.out = out;
    return rb_entry(c, "pmp_resblock_forward", s, q, false, false);
}

int pmp_resblock_backward_device(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *t, const float *out, const float *w0,
                                 const float *w2, const float *wsc, const float *g_out, float *g_x, float *g_w0, float *g_w2, float *g_wsc)
{
    RbPtrs q{};
    q.x = x; q.t_in = t; q.out_in = out; q.w0 = w0; q.w2 = w2; q.wsc = wsc; q.g_out = g_out;
    q.g_x = g_x; q.g_w0 = g_w0; q.g_w2 = g_w2; q.g_wsc = g_wsc;
    return rb_entry(c, "pmp_resblock_backward", s, q, true, true);
}

int pmp_resblock_backward(pmp_ctx *c, const pmp_rb_shape *s, const float *x, const float *t, const float *out, const float *w0,
                          const float *w2, const float *wsc, const float *g_out, float *g_x, float *g_w0, float *g_w2, float *g_wsc)
{
    RbPtrs q{};
    q.x = x; q.t_in = t; q.out_in = out; q.w0 = w0; q.w2 = w2; q.wsc = wsc; q.g_out = g_out;
    q.g_x = g_x; q.g_w0 = g_w0; q.g_w2 = g_w2; q.g_wsc = g_wsc;
    return rb_entry(c, "pmp_resblock_backward", s, q, true, false);
}

}  // extern "C"
