// api_debug.cpp — the measuring and test hooks of the C ABI (include/pmp.h): kernel-class timing, tensor taps, workspace poisoning,
// the fusion / winograd / variant switches, the convolution bench and the single ResidualBlock.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pmp_host.h"

namespace pmp {

// ---- kernel-class timing ---------------------------------------------------------------------------------
KScope::KScope(pmp_ctx *c_, hipStream_t stream_, int cls_, double flops_) : c(c_), stream(stream_), cls(cls_), on(false), a(nullptr), b(nullptr), flops(flops_)
{
    on = (c->kmask >> cls) & 1u;
    if (on) { a = c->event_pool.get(); b = c->event_pool.get(); hipEventRecord(a, stream); }
}

KScope::~KScope()
{
    if (on) { hipEventRecord(b, stream); c->krec[cls].push_back(KTimeRec{a, b, flops}); }
}

void ktime_drain(pmp_ctx *c)
{
    for (int k = 0; k < K_NCLASS; ++k) {
        for (auto &r : c->krec[k]) {
            float ms = 0.f;
            hipEventSynchronize(r.b);
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->kms[k] += ms; c->klaunch[k] += 1; c->kflops[k] += r.flops; }
            c->event_pool.put(r.a);
            c->event_pool.put(r.b);
        }
        c->krec[k].clear();
    }
}

// pmp_debug_set_taps: the tensor a kernel has just written, copied on the same stream right behind that launch - later launches
// (an identity-shortcut block writing its output in place, a tensor reusing freed arena bytes) cannot reach it before the copy.
int tap_record(pmp_ctx *c, hipStream_t stream, const std::string &name, const void *p, int n, int C, int H, int W, int c_real, int fmt, int exp)
{
    const size_t bytes = (size_t)n * C * H * W * (fmt == 1 ? 6 : 4);
    if (c->ntaps >= (int)c->taps.size()) c->taps.emplace_back();
    TapRec &t = c->taps[c->ntaps];
    int rc = ensure(c, t.buf, bytes);
    if (rc != PMP_OK) return rc;
    const hipError_t e = hipMemcpyAsync(t.buf.p, p, bytes, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return hip_fail(c, e, "tap copy");
    t.name = name; t.n = n; t.C = C; t.H = H; t.W = W; t.c_real = c_real; t.fmt = fmt; t.exp = exp;
    ++c->ntaps;
    return PMP_OK;
}

// pmp_debug_run_resblock: where the launchers' notes go while it runs (this thread only; nowhere otherwise)
static thread_local std::string *launch_log = nullptr;

void note_launch(const char *kernel, int t0, int t1, int t2, int t3, int t4)
{
    if (!launch_log) return;
    std::string s = std::string(kernel) + "<" + std::to_string(t0) + "," + std::to_string(t1) + "," + std::to_string(t2);
    for (int t : {t3, t4}) if (t >= 0) s += "," + std::to_string(t);
    *launch_log += s + ">\n";
}

}  // namespace pmp

using namespace pmp;

extern "C" {

int pmp_debug_set_conv_variant(int variant)
{
    int rc;
    if (abl_set_conv_variant(variant, &rc)) return rc;
    // the product library ships ONE form of every kernel (number 2): there is no process-wide selector in it.  The A/B forms
    // (bit-identical, measured slower or equal) and the timing-only builds live in tools/abl/libpmp_hip_abl.so (make -C tools/abl)
    if (variant != 2) return set_err(nullptr, PMP_E_INVALID, "pmp_debug_set_conv_variant: this library ships only the default form (2); the A/B and timing-only builds are in tools/abl/libpmp_hip_abl.so (make -C tools/abl)");
    return PMP_OK;
}

int pmp_debug_set_fusion(pmp_ctx *c, int on)
{
    CHECK_CTX(c);
    const int rc = settle(c);
    if (rc != PMP_OK) return rc;
    if (on < 0 || on > 3) return set_err(c, PMP_E_INVALID, "pmp_debug_set_fusion: 0 (none), 1 (all), 2 (16x16 tails only), 3 (32x32 ResidualBlocks only)");
    c->fuse16 = (on == 1 || on == 2) ? 1 : 0;
    c->fuse32 = (on == 1 || on == 3) ? 1 : 0;
    return PMP_OK;
}

int pmp_debug_set_winograd(pmp_ctx *c, int on)
{
    CHECK_CTX(c);
    int rc = settle(c);
    if (rc != PMP_OK) return rc;
    if (abl_set_winograd(c, on, &rc)) return rc;
    // the Winograd-x kernel did not beat the direct form (profiles/r03_notes.txt): it lives in tools/abl/libpmp_hip_abl.so (make -C tools/abl)
    if (on) return set_err(c, PMP_E_INVALID, "pmp_debug_set_winograd: the Winograd-x form is built into tools/abl/libpmp_hip_abl.so only (make -C tools/abl)");
    return PMP_OK;
}

int pmp_debug_conv_bench(pmp_ctx *c, int n, int h, int w, int cin, int cout, int k, int iters, double *ms_f32, double *ms_x6,
                         double *max_abs_diff, double *max_abs_ref)
{
    CHECK_CTX(c);
    if (n <= 0 || (h & 15) || (w & 15) || (cin & 15) || (cout & 15) || cout > 64 || (k != 1 && k != 3 && k != 5) || iters <= 0)
        return set_err(c, PMP_E_INVALID, "pmp_debug_conv_bench: bad shape");
    const size_t nx = (size_t)n * cin * h * w, ny = (size_t)n * cout * h * w;
    std::vector<float> hx(nx), hw((size_t)cout * cin * k * k);
    unsigned long long st = 0x1234567ull;
    auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) / 16777216.0) * 2.f - 1.f; };
    for (auto &v : hx) v = rnd() * 3.f;
    const float ws = 1.f / sqrtf((float)cin * k * k);
    for (auto &v : hw) v = rnd() * ws;
    std::vector<float> wp = pack_mfma(hw.data(), cout, cin, k, k, cout, cin);
    const bool h2 = c->precision == PMP_PRECISION_F16X3;   // the split leg follows the context's datapath
    const int kexp = h2_scale_exp(hw.data(), hw.size());
    std::vector<unsigned short> wx = h2 ? pack_h2(hw.data(), cout, cin, k, k, cout, cin, kexp) : pack_x6(hw.data(), cout, cin, k, k, cout, cin);
    AblBench ab;
    DevBuf bx, by, by2, bwp, bxs, bys, bwx;            // freed on every way out
    hipError_t e = hipSuccess;
    auto A = [&](DevBuf &b, size_t bytes) {            // not ensure(): a failure here is the bench's own PMP_E_HIP
        if (e != hipSuccess) return;
        if ((e = hipMalloc(&b.p, bytes)) == hipSuccess) b.cap = bytes;
        else b.p = nullptr;
    };
    A(bx, nx * 4); A(by, ny * 4); A(by2, ny * 4); A(bwp, wp.size() * 4);
    A(bxs, nx * 6); A(bys, ny * 6); A(bwx, wx.size() * 2);
    int rc = PMP_OK;
    if (e != hipSuccess) rc = hip_fail(c, e, "hipMalloc(conv bench)");
    if (rc == PMP_OK) {
        float *dx = (float *)bx.p, *dy = (float *)by.p, *dy2 = (float *)by2.p, *dwp = (float *)bwp.p;
        unsigned short *dxs = (unsigned short *)bxs.p, *dys = (unsigned short *)bys.p, *dwx = (unsigned short *)bwx.p;
        hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice);
        hipMemcpy(dwp, wp.data(), wp.size() * 4, hipMemcpyHostToDevice);
        hipMemcpy(dwx, wx.data(), wx.size() * 2, hipMemcpyHostToDevice);
        ConvMfmaArgs a{};
        a.x = dx; a.w = dwp; a.out = dy; a.N = n; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout; a.KH = a.KW = k; a.relu = 1;
        ConvX6Args b{};
        b.x = dxs; b.x_stride = nx; b.w = dwx; b.out = dys; b.out_stride = ny;
        b.N = n; b.H = h; b.W = w; b.Cin = cin; b.Cout = cout; b.KH = b.KW = k; b.relu = 1;
        b.out_scale = std::ldexp(1.f, -kexp);
        abl_bench_prepare(c, ab, hw.data(), k, cin, cout, h2, b);
        auto launch_split = [&]() { return h2 ? launch_conv_h2(c->stream, b) : launch_conv_x6(c->stream, b); };
        hipEvent_t e0 = c->event_pool.get(), e1 = c->event_pool.get();
        if (h2) launch_f32_to_split2(c->stream, dx, dxs, nx, nx);
        else launch_f32_to_split3(c->stream, dx, dxs, nx, nx);
        launch_conv_mfma(c->stream, a);
        e = launch_split();
        float ms = 0.f;
        hipEventRecord(e0, c->stream);
        for (int i = 0; i < iters; ++i) launch_conv_mfma(c->stream, a);
        hipEventRecord(e1, c->stream); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
        if (ms_f32) *ms_f32 = ms / iters;
        hipEventRecord(e0, c->stream);
        for (int i = 0; i < iters; ++i) launch_split();
        hipEventRecord(e1, c->stream); hipEventSynchronize(e1); hipEventElapsedTime(&ms, e0, e1);
        if (ms_x6) *ms_x6 = ms / iters;
        abl_bench_report(c, ab, h2, n, h, w, k, cout, b, launch_split);
        if (h2) launch_split2_to_f32(c->stream, dys, dy2, ny, ny);
        else launch_split3_to_f32(c->stream, dys, dy2, ny, ny);
        std::vector<float> y1(ny), y2(ny);
        hipMemcpyAsync(y1.data(), dy, ny * 4, hipMemcpyDeviceToHost, c->stream);
        hipMemcpyAsync(y2.data(), dy2, ny * 4, hipMemcpyDeviceToHost, c->stream);
        hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e == hipSuccess) e = hipGetLastError();
        double md = 0, mr = 0;
        for (size_t i = 0; i < ny; ++i) { md = fmax(md, fabs((double)y1[i] - y2[i])); mr = fmax(mr, fabs((double)y1[i])); }
        if (max_abs_diff) *max_abs_diff = md;
        if (max_abs_ref) *max_abs_ref = mr;
        c->event_pool.put(e0); c->event_pool.put(e1);
        if (e != hipSuccess) rc = hip_fail(c, e, "conv bench");
    }
    abl_bench_free(ab);
    return rc;
}

int pmp_debug_run_resblock(pmp_ctx *c, const pmp_rb_case *k, const float *x, const float *w0, const float *w2, const float *wsc,
                           const float *gate, int *saturated, char *kernels, int64_t cap)
{
    CHECK_CTX(c);
    if (!k || !x || !w0 || !w2) return set_err(c, PMP_E_INVALID, "pmp_debug_run_resblock: null argument");
    const int cin = k->cin, cout = k->cout;
    if (k->n < 1 || k->n > PMP_TAP_MAX_BLOCKS || k->h < 16 || k->h > 256 || (k->h & 15) || k->w < 16 || k->w > 256 || (k->w & 15) ||
        cin < 16 || cin > 256 || (cin & 15) || (cout != 16 && cout != 32 && cout != 64) || (k->k != 1 && k->k != 3 && k->k != 5))
        return set_err(c, PMP_E_INVALID, "pmp_debug_run_resblock: unsupported shape");
    if ((k->gate && k->pool) || (k->gate && !gate) || (cin != cout && !wsc))
        return set_err(c, PMP_E_INVALID, "pmp_debug_run_resblock: pool with a gate, or a missing gate / shortcut tensor");
    if (!c->taps_on) return set_err(c, PMP_E_INVALID, "pmp_debug_run_resblock: turn the taps on first (pmp_debug_set_taps)");
    int rc = settle(c);
    unsigned fired = 0;
    if (rc == PMP_OK) rc = sat_fetch(c, &fired);                 // the flag is this call's
    if (rc != PMP_OK) return rc;
    const bool h2 = c->precision == PMP_PRECISION_F16X3;
    NetWeights nw;
    nw.act_given = true;
    nw.act_exp[0] = k->gate ? k->exp_gate : k->exp_x;
    nw.act_exp[1] = k->exp_x;
    nw.act_exp[2] = k->exp_out;
    // the inputs in the graph's blocked layout at their stored scale (x 2^-e, exact: a power of two)
    auto blocked = [&](const float *src, int C, int e) {
        const int cp = (C + 15) & ~15;
        std::vector<float> b((size_t)k->n * cp * k->h * k->w, 0.f);
        const float s = h2 ? std::ldexp(1.f, -e) : 1.f;
        for (int n = 0; n < k->n; ++n)
            for (int ch = 0; ch < C; ++ch)
                for (int y = 0; y < k->h; ++y)
                    for (int xx = 0; xx < k->w; ++xx)
                        b[((((size_t)n * (cp / 16) + ch / 16) * k->h + y) * k->w + xx) * 16 + ch % 16] =
                            src[(((size_t)n * C + ch) * k->h + y) * k->w + xx] * s;
        return b;
    };
    const std::vector<float> xb = blocked(x, cin, k->exp_x), gb = k->gate ? blocked(gate, cout, k->exp_gate) : std::vector<float>();
    std::string log;
    rc = load_single_rb(c, nw, cin, cout, k->k, w0, w2, wsc, 1u << c->precision);
    if (rc == PMP_OK) {
        c->ntaps = 0;
        launch_log = &log;
        Pass ps{c->stream, c->ws, c->precision, /*taps*/ true, /*cal*/ false, /*caller*/ true};
        rc = run_graph(c, ps, [&] { return run_resblock(c, ps, nw, k->n, k->h, k->w, xb.data(), k->gate ? gb.data() : nullptr, k->pool != 0, k->out_f32 != 0); });
        launch_log = nullptr;
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess && rc == PMP_OK) rc = hip_fail(c, e, "pmp_debug_run_resblock");
    }
    if (rc == PMP_OK) rc = sat_fetch(c, &fired);
    free_net_weights(nw);
    if (rc != PMP_OK) return rc;
    if (saturated) *saturated = fired ? 1 : 0;
    if (kernels && cap > 0) {
        const size_t m = std::min(log.size(), (size_t)cap - 1);
        memcpy(kernels, log.data(), m);
        kernels[m] = 0;
    }
    return PMP_OK;
}

int pmp_debug_poison_workspace(pmp_ctx *c, int pattern)
{
    CHECK_CTX(c);
    if (pattern < 0 || pattern > 2) return set_err(c, PMP_E_INVALID, "pmp_debug_poison_workspace: 0 (off), 1 (0xFF bytes) or 2 (0x3C bytes)");
    const int rc = settle(c);
    if (rc != PMP_OK) return rc;
    c->poison = pattern;
    return PMP_OK;
}

int pmp_debug_set_taps(pmp_ctx *c, int on)
{
    CHECK_CTX(c);
    const int rc = settle(c);
    if (rc != PMP_OK) return rc;
    c->taps_on = on ? 1 : 0;
    c->ntaps = 0;
    if (!on) c->taps.clear();                   // ... and their device memory with them
    return PMP_OK;
}

static double f16_value(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 1023;
    const double v = e == 0 ? std::ldexp((double)m, -24) : e == 31 ? (m ? NAN : INFINITY) : std::ldexp((double)(m | 1024), e - 25);
    return (h & 0x8000) ? -v : v;
}

static double bf16_value(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int64_t pmp_debug_get_tap(pmp_ctx *c, const char *name, double *out, int64_t cap, int dims[4], int *c_real)
{
    CHECK_CTX(c);
    if (!name) return set_err(c, PMP_E_INVALID, "pmp_debug_get_tap: null name");
    int rc = settle(c);
    if (rc != PMP_OK) return rc;
    const TapRec *t = nullptr;
    for (int i = c->ntaps - 1; i >= 0 && !t; --i) if (c->taps[i].name == name) t = &c->taps[i];
    if (!t) return set_err(c, PMP_E_INVALID, std::string("pmp_debug_get_tap: no tensor ") + name + " in the last call");
    const size_t elems = (size_t)t->n * t->C * t->H * t->W;
    if (dims) { dims[0] = t->n; dims[1] = t->C; dims[2] = t->H; dims[3] = t->W; }
    if (c_real) *c_real = t->c_real;
    if (!out || (int64_t)elems > cap) return (int64_t)elems;
    std::vector<uint16_t> raw(elems * (t->fmt == 0 ? 2 : t->fmt == 1 ? 3 : 2));
    const hipError_t e = hipMemcpy(raw.data(), t->buf.p, raw.size() * 2, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(c, e, "pmp_debug_get_tap");
    const float *f = reinterpret_cast<const float *>(raw.data());
    const int G = t->C / 16;
    for (size_t i = 0; i < elems; ++i) {        // blocked [n][C/16][H][W][16] -> dense NCHW
        double v;
        if (t->fmt == 0) v = f[i];
        else if (t->fmt == 2) v = f16_value(raw[i]) + f16_value(raw[elems + i]);                                   // exact in float64
        else v = bf16_value(raw[i]) + bf16_value(raw[elems + i]) + bf16_value(raw[2 * elems + i]);
        const size_t cl = i & 15, x = (i >> 4) % t->W, y = (i >> 4) / t->W % t->H, g = (i >> 4) / ((size_t)t->W * t->H) % G,
                     b = (i >> 4) / ((size_t)t->W * t->H * G);
        out[((b * t->C + g * 16 + cl) * t->H + y) * t->W + x] = std::ldexp(v, t->exp);
    }
    return (int64_t)elems;
}

// ---- timing ------------------------------------------------------------------------------------------------
int pmp_ktime_classes(void) { return K_NCLASS; }

const char *pmp_ktime_name(int cls)
{
    static const char *names[K_NCLASS] = {"conv_mfma_3x3_c64", "conv_mfma_5x5_c64", "conv_mfma_other", "stem", "small", "postprocess"};
    return (cls >= 0 && cls < K_NCLASS) ? names[cls] : "";
}

int pmp_ktime_enable(pmp_ctx *c, uint32_t mask)
{
    CHECK_CTX(c);
    int rc = sync(c);
    if (rc != PMP_OK) return rc;
    ktime_drain(c);
    for (int k = 0; k < K_NCLASS; ++k) { c->klaunch[k] = 0; c->kms[k] = 0; c->kflops[k] = 0; }
    c->kmask = mask;
    return PMP_OK;
}

int pmp_ktime_get(pmp_ctx *c, int cls, int64_t *launches, double *ms, double *flops)
{
    CHECK_CTX(c);
    if (cls < 0 || cls >= K_NCLASS) return set_err(c, PMP_E_INVALID, "pmp_ktime_get: bad class");
    int rc = sync(c);
    if (rc != PMP_OK) return rc;
    ktime_drain(c);
    if (launches) *launches = c->klaunch[cls];
    if (ms) *ms = c->kms[cls];
    if (flops) *flops = c->kflops[cls];
    return PMP_OK;
}

}  // extern "C"
