// pmp_api.cpp — the C ABI declared in include/pmp.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "pmp_host.h"

namespace pmp {

int set_err(pmp_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return set_err_global(code, msg);   // host_emit.cpp: the calling thread's context-less error string
}

int hip_fail(pmp_ctx *c, hipError_t e, const char *what)
{
    return set_err(c, PMP_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// ---- parked workspaces.  On this pool a large hipMalloc that follows a hipFree of similar size stalls for 0.5-1.4 s now and then
// (tools/probe/malloc_probe.py: the freed VRAM is still being cleared); a host that destroys a context and creates the next one -
// one per sequence, one per encoder instance - would pay that for its 10 GB activation workspace every time.  pmp_destroy therefore
// PARKS the workspace (one buffer per device, the larger one wins) and the next context on that device takes it over; pmp_trim()
// gives parked memory back to the driver.  PMP_PARK_WORKSPACE=0 in the environment turns parking off (pmp_destroy then frees everything:
// for a host that destroys its context to hand the VRAM to another library and cannot call pmp_trim).
namespace {
std::mutex g_park_mutex;
constexpr int PARK_SLOTS = 2;     // a context in overlap mode owns two workspaces (ws, ws2): both are parked (round 5; one slot until then)
struct Parked { DevBuf b[PARK_SLOTS]; };
std::map<int, Parked> g_parked;   // device -> buffers
}  // namespace

static void park_workspace(int device, DevBuf &b)
{
    if (!b.p) return;
    const char *env = std::getenv("PMP_PARK_WORKSPACE");
    if (env && env[0] == '0' && !env[1]) { hipFree(b.p); b = DevBuf(); return; }
    std::lock_guard<std::mutex> lk(g_park_mutex);
    Parked &pk = g_parked[device];
    int victim = 0;                                   // an empty slot, else the smallest parked buffer
    for (int i = 0; i < PARK_SLOTS; ++i) {
        if (!pk.b[i].p) { victim = i; break; }
        if (pk.b[i].cap < pk.b[victim].cap) victim = i;
    }
    if (pk.b[victim].p && pk.b[victim].cap >= b.cap) { hipFree(b.p); }         // everything parked is at least as large: drop the newcomer
    else { if (pk.b[victim].p) hipFree(pk.b[victim].p); pk.b[victim] = b; }
    b = DevBuf();
}

static bool take_parked(int device, size_t bytes, DevBuf &out)
{
    std::lock_guard<std::mutex> lk(g_park_mutex);
    auto it = g_parked.find(device);
    if (it == g_parked.end()) return false;
    int best = -1;                                    // the smallest parked buffer that is large enough
    for (int i = 0; i < PARK_SLOTS; ++i)
        if (it->second.b[i].p && it->second.b[i].cap >= bytes && (best < 0 || it->second.b[i].cap < it->second.b[best].cap)) best = i;
    if (best < 0) return false;
    out = it->second.b[best];
    it->second.b[best] = DevBuf();
    return true;
}

int ensure(pmp_ctx *c, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return PMP_OK;
    if (b.p) { hipFree(b.p); b.p = nullptr; b.cap = 0; }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { b.p = nullptr; return set_err(c, PMP_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    b.cap = bytes;
    return PMP_OK;
}

// A pass's activation workspace: a large one takes a parked one of a destroyed context first (small ones are cheap to allocate and stay small)
static int ensure_workspace(pmp_ctx *c, DevBuf &b, size_t bytes)
{
    DevBuf got;
    if (bytes > b.cap && bytes >= ((size_t)64 << 20) && take_parked(c->device, bytes, got)) {
        if (b.p) hipFree(b.p);
        b = got;
        return PMP_OK;
    }
    return ensure(c, b, bytes);
}

// ---- kernel-class timing ---------------------------------------------------------------------------------
static hipEvent_t get_event(pmp_ctx *c)
{
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

KScope::KScope(pmp_ctx *c_, hipStream_t stream_, int cls_, double flops_) : c(c_), stream(stream_), cls(cls_), on(false), a(nullptr), b(nullptr), flops(flops_)
{
    on = (c->kmask >> cls) & 1u;
    if (on) { a = get_event(c); b = get_event(c); hipEventRecord(a, stream); }
}

KScope::~KScope()
{
    if (on) { hipEventRecord(b, stream); c->krec[cls].push_back(KTimeRec{a, b, flops}); }
}

static void ktime_drain(pmp_ctx *c)
{
    for (int k = 0; k < K_NCLASS; ++k) {
        for (auto &r : c->krec[k]) {
            float ms = 0.f;
            hipEventSynchronize(r.b);
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->kms[k] += ms; c->klaunch[k] += 1; c->kflops[k] += r.flops; }
            c->event_pool.push_back(r.a);
            c->event_pool.push_back(r.b);
        }
        c->krec[k].clear();
    }
}

NetWeights *find_net(pmp_ctx *c, int net_id, int qp)
{
    auto it = c->nets.find(net_id * 100 + qp);
    return (it == c->nets.end() || !it->second.loaded) ? nullptr : &it->second;
}

static int poison_byte(const pmp_ctx *c) { return c->poison == 1 ? 0xFF : 0x3C; }   // pmp_debug_poison_workspace: NaN bytes or finite garbage

// Runs forward (measure pass, then real) for n <= chunk blocks.
int run_graph(pmp_ctx *c, Pass &ps, const std::function<int()> &fwd)
{
    Arena &ar = ps.arena;
    ar.measuring = true;
    ar.reset();
    int rc = fwd();
    if (rc != PMP_OK) return rc;
    if ((rc = ensure_workspace(c, ps.ws, ar.peak)) != PMP_OK) return rc;
    if (ps.caller && ar.peak > c->ws_need) c->ws_need = ar.peak;
    ar.base = static_cast<char *>(ps.ws.p);
    ar.cap = ps.ws.cap;
    ar.measuring = false;
    ar.reset();
    if (c->poison && ps.ws.p) {   // pmp_debug_poison_workspace: the whole buffer (own, second or taken over), stream-ordered before the pass
        const hipError_t e = hipMemsetAsync(ps.ws.p, poison_byte(c), ps.ws.cap, ps.stream);
        if (e != hipSuccess) return hip_fail(c, e, "poison workspace");
    }
    return fwd();
}

// The passes of one inference call on datapath `precision`; taps: record its tensors (pmp_debug_set_taps).
static int infer_passes(pmp_ctx *c, int precision, bool taps, bool luma, NetWeights &wq, NetWeights &wb, const uint8_t *by, const uint8_t *bu,
                        const uint8_t *bv, int64_t n, float *qt, float *bt, float *dire, const float *qt_in = nullptr)
{
    // qt_in: teacher-forced MTT inference (pmp_infer_msbd) - the MTT net reads this map, the QT net does not run, qt is not written
    int rc0;     // weights are packed per datapath, on first use (the load packed the datapath that was current then)
    if ((rc0 = ensure_datapath(c, wq, precision)) != PMP_OK || (rc0 = ensure_datapath(c, wb, precision)) != PMP_OK) return rc0;
    // f16x3: the MTT net's activation scales, from one calibration pass when the net is first used on this datapath
    if (precision == PMP_PRECISION_F16X3 && c->act_scales && !wb.calibrated && (rc0 = calibrate_mtt(c, luma, wq, wb)) != PMP_OK) return rc0;
    if ((rc0 = abl_prepare_pass(c, precision, wq, wb)) != PMP_OK) return rc0;
    // Overlap mode: a call of at least 1024 blocks runs as (at least) two chunks, even ones on the context's stream and workspace, odd
    // ones on a second stream with a second workspace, so that one chunk's small launches (stems, 16x16 tails, HBM-bound 32x32 layers)
    // run beside the other's 64x64 convolutions.  Blocks are independent: the results do not depend on how a call is cut.
    const bool overlap = c->overlap && n >= 1024;
    int64_t chunk = c->chunk;
    if (overlap && (n + 1) / 2 < chunk) chunk = (n + 1) / 2;
    if (overlap) {
        hipError_t e = hipSuccess;
        if (!c->stream2) e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
        hipEvent_t ev = get_event(c);
        if (e == hipSuccess) e = hipEventRecord(ev, c->stream);              // fork: the second stream starts behind everything enqueued so far
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream2, ev, 0);
        c->event_pool.push_back(ev);
        if (e != hipSuccess) return hip_fail(c, e, "overlap: fork");
    }
    int rc = PMP_OK, k = 0;
    for (int64_t o = 0; o < n && rc == PMP_OK; o += chunk, ++k) {
        const int m = (int)((n - o) < chunk ? (n - o) : chunk);
        const uint8_t *y = by + o * 68 * 68;
        const uint8_t *u = bu ? bu + o * 34 * 34 : nullptr, *v = bv ? bv + o * 34 * 34 : nullptr;
        float *q = qt_in ? nullptr : qt + o * 64;
        const float *qi = qt_in ? qt_in + o * 64 : q;
        const bool side = overlap && (k & 1);
        Pass ps{side ? c->stream2 : c->stream, side ? c->ws2 : c->ws, precision, taps, /*cal*/ false, /*caller*/ true};
        if (!qt_in) rc = run_graph(c, ps, [&] { return forward_q(c, ps, luma, wq, y, u, v, m, q); });
        if (rc == PMP_OK) rc = run_graph(c, ps, [&] { return forward_msbd(c, ps, luma, wb, y, u, v, qi, m, bt + o * 768, dire + o * 768); });
    }
    if (overlap) {
        hipEvent_t ev = get_event(c);
        hipError_t e = hipEventRecord(ev, c->stream2);                       // join: the caller's stream continues behind both
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
        c->event_pool.push_back(ev);
        if (e != hipSuccess && rc == PMP_OK) rc = hip_fail(c, e, "overlap: join");
    }
    return rc;
}

// ---- f16x3 range guard (include/pmp.h) ----------------------------------------------------------------------------------
constexpr int PMP_SAT_SLOTS = 64;
constexpr int PMP_TAP_MAX_BLOCKS = 64;        // pmp_debug_set_taps: tap memory is one copy of every tensor of the call

// Reads and clears the device-side saturation word (synchronises the stream): PMP_SAT_IGNORE contexts, whose calls take no snapshots.
static int sat_fetch(pmp_ctx *c, unsigned *out)
{
    unsigned h = 0;
    hipError_t e = hipMemcpyAsync(&h, c->d_sat, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && h) e = hipMemsetAsync(c->d_sat, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "saturation flag");
    *out = h;
    return PMP_OK;
}

static void drop_pending(pmp_ctx *c)
{
    for (auto &p : c->pending) if (p.ev) c->event_pool.push_back(p.ev);
    c->pending.clear();
}

static int count_pending_infer(const pmp_ctx *c)
{
    int k = 0;
    for (const auto &p : c->pending) k += p.infer;
    return k;
}

// Looks at the flag snapshots of the calls in flight, oldest first.  wait = false: only those whose event has completed (a later
// call polling, no host stall); wait = true: all of them (pmp_synchronize, pmp_get_saturation, host-pointer calls).  The first
// fired flag drains the stream once - from then on every later snapshot is final - and from there on, in order: a fired inference
// call runs again on the exact fp32 MFMA datapath, a later inference call that keeps its logits in the context's own buffers runs
// again as it was (the re-run before it has overwritten them), a post-processing call behind a re-run is replayed.  Everything
// re-enqueued is ordered on the stream; the caller synchronises if it needs the results on the host.
static int resolve_pending(pmp_ctx *c, bool wait)
{
    bool dirty = false;
    while (!c->pending.empty()) {
        PendingCall &p = c->pending.front();
        int rc = PMP_OK;
        if (p.infer) {
            if (!dirty) {
                hipError_t e = wait ? hipEventSynchronize(p.ev) : hipEventQuery(p.ev);
                if (e == hipErrorNotReady) break;
                if (e != hipSuccess) { drop_pending(c); return hip_fail(c, e, "saturation flag event"); }
            }
            if (*p.slot) {
                c->sat_seen = 1;
                if (c->sat_policy == PMP_SAT_ERROR) {
                    drop_pending(c);
                    return set_err(c, PMP_E_RANGE, "pmp_infer: an activation exceeded the fp16 range of the f16x3 datapath (use bf16x6 or fp32)");
                }
                if (!dirty) {
                    hipError_t e = hipStreamSynchronize(c->stream);
                    if (e != hipSuccess) { drop_pending(c); return hip_fail(c, e, "hipStreamSynchronize"); }
                    dirty = true;
                }
                c->sat_reruns += 1;
                rc = p.rerun(true);
            } else if (dirty && p.ctx_logits) {
                rc = p.rerun(false);
            }
        } else if (dirty) {
            rc = p.rerun(false);
        }
        if (p.ev) c->event_pool.push_back(p.ev);
        c->pending.pop_front();
        if (rc != PMP_OK) { drop_pending(c); return rc; }
    }
    return PMP_OK;
}

static int infer_device_impl(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
                             int64_t n, float *qt, float *bt, float *dire, bool ctx_logits = false, const float *qt_in = nullptr)
{
    if (comp != PMP_LUMA && comp != PMP_CHROMA) return set_err(c, PMP_E_INVALID, "pmp_infer: comp must be PMP_LUMA or PMP_CHROMA");
    if (n < 0 || !by || (!qt && !qt_in) || !bt || !dire || (comp == PMP_CHROMA && (!bu || !bv)))
        return set_err(c, PMP_E_INVALID, "pmp_infer: null buffer or negative count");
    const bool luma = comp == PMP_LUMA;
    const int id_q = luma ? PMP_NET_LUMA_Q : PMP_NET_CHROMA_Q, id_b = luma ? PMP_NET_LUMA_MSBD : PMP_NET_CHROMA_MSBD;
    NetWeights *wq = find_net(c, id_q, qp);
    NetWeights *wb = find_net(c, id_b, qp);
    if (!wq || !wb) return set_err(c, PMP_E_NOWEIGHTS, "pmp_infer: weights for this (comp, qp) are not loaded");
    if (c->taps_on && (n > c->chunk || n > PMP_TAP_MAX_BLOCKS || c->overlap))
        return set_err(c, PMP_E_INVALID, "pmp_infer: with taps on, one pass of at most 64 blocks (n <= chunk) and overlap mode off");
    int rc = resolve_pending(c, false);          // earlier calls whose snapshot has landed by now: no wait
    if (rc != PMP_OK) return rc;
    if (c->taps_on) c->ntaps = 0;                // the taps are this call's (a re-run resolved above is recorded by nobody)
    const int precision = c->precision;          // the datapath at enqueue: a re-run that did not fire runs on it again
    rc = infer_passes(c, precision, c->taps_on != 0, luma, *wq, *wb, by, bu, bv, n, qt, bt, dire, qt_in);
    if (rc != PMP_OK || precision != PMP_PRECISION_F16X3 || c->sat_policy == PMP_SAT_IGNORE || n == 0) return rc;
    // f16x3 range guard: snapshot the flag behind this call's passes and reset it for the next call - all stream-ordered, the host
    // does not wait.  Whoever looks at the snapshot later (resolve_pending) re-runs the call on the fp32 MFMA datapath if it fired.
    if (count_pending_infer(c) >= PMP_SAT_SLOTS && (rc = resolve_pending(c, true)) != PMP_OK) return rc;
    unsigned *slot = c->h_sat + (c->sat_seq++ % PMP_SAT_SLOTS);
    *slot = 0;
    hipError_t e = hipMemcpyAsync(slot, c->d_sat, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_sat, 0, sizeof(unsigned), c->stream);
    hipEvent_t ev = get_event(c);
    if (e == hipSuccess) e = hipEventRecord(ev, c->stream);
    if (e != hipSuccess) { c->event_pool.push_back(ev); return hip_fail(c, e, "saturation flag snapshot"); }
    c->pending.push_back(PendingCall{true, ctx_logits, ev, slot, [=](bool fired) {
        NetWeights *rq = find_net(c, id_q, qp), *rb = find_net(c, id_b, qp);   // replacing a net settles first: still the same nets
        if (!rq || !rb) return set_err(c, PMP_E_NOWEIGHTS, "pmp_infer: weights vanished before the range-guard re-run");
        // fired: the exact fp32 MFMA datapath - fp32's range, a bit-exact fmaf chain, and on the full-size campaign the closest of the
        // three to the oracle (profiles/r03_parity_campaign.txt: 5.5e-4 against bf16x6's 8.9e-4 on the worst block); its speed does not
        // matter for a call that is this rare.  Not fired: the call's logits were in the context's buffers, which an earlier re-run has
        // overwritten - the same call again, on the datapath it ran on.  No taps: pmp_debug_set_taps records the call as it first ran.
        return infer_passes(c, fired ? PMP_PRECISION_F32 : precision, false, luma, *rq, *rb, by, bu, bv, n, qt, bt, dire, qt_in);   // teacher-forced: the MTT net only
    }});
    return PMP_OK;
}

static int post_launch(pmp_ctx *c, int comp, const M2PParams &prm, const float *qt, const float *bt, const float *dire, int64_t n,
                       uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8, int record_stride)
{
    KScope ks(c, c->stream, K_POST, 0.0);
    hipError_t e = launch_postprocess(c->stream, qt, bt, dire, n, comp == PMP_LUMA ? 1 : 2, prm, hor, ver, qt_u8, dire_i8, record_stride);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "postprocess");
}

static int post_device_impl(pmp_ctx *c, int comp, const float *qt, const float *bt, const float *dire, int64_t n,
                            uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8, int record_stride = 0)
{
    if (comp != PMP_LUMA && comp != PMP_CHROMA) return set_err(c, PMP_E_INVALID, "pmp_postprocess: bad comp");
    if (n < 0 || !qt || !bt || !dire || !hor || !ver || !qt_u8 || !dire_i8)
        return set_err(c, PMP_E_INVALID, "pmp_postprocess: null buffer or negative count");
    const M2PParams prm = c->m2p[comp];     // the thresholds current at ENQUEUE: the replay below runs with them too (include/pmp.h)
    const int rc = post_launch(c, comp, prm, qt, bt, dire, n, hor, ver, qt_u8, dire_i8, record_stride);
    // its logits may come from an inference call whose range flag has not been looked at yet: remember the call for the replay
    if (rc == PMP_OK && !c->pending.empty())
        c->pending.push_back(PendingCall{false, false, nullptr, nullptr, [=](bool) { return post_launch(c, comp, prm, qt, bt, dire, n, hor, ver, qt_u8, dire_i8, record_stride); }});
    return rc;
}


// The context's own logit buffers (fused entry points called without logit pointers, host-pointer entry points).  Calls still in
// flight may hold pointers into them for a range-guard re-run: they are settled BEFORE a buffer is regrown (and thereby freed).
static int ensure_logits(pmp_ctx *c, int64_t n)
{
    const size_t need[3] = {(size_t)(n ? n : 1) * 64 * 4, (size_t)(n ? n : 1) * 768 * 4, (size_t)(n ? n : 1) * 768 * 4};
    int rc;
    if ((need[0] > c->d_logit[0].cap || need[1] > c->d_logit[1].cap || need[2] > c->d_logit[2].cap) && !c->pending.empty() &&
        (rc = settle(c)) != PMP_OK)
        return rc;
    for (int i = 0; i < 3; ++i) {
        if ((rc = ensure(c, c->d_logit[i], need[i])) != PMP_OK) return rc;
        if (c->poison) {          // pmp_debug_poison_workspace: whoever uses them next must write every byte it later reads
            const hipError_t e = hipMemsetAsync(c->d_logit[i].p, poison_byte(c), need[i], c->stream);
            if (e != hipSuccess) return hip_fail(c, e, "poison logits");
        }
    }
    return PMP_OK;
}

static int sync(pmp_ctx *c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "hipStreamSynchronize");
}

// Everything this context has been asked to do is done and final: range flags looked at, re-runs finished.
int settle(pmp_ctx *c)
{
    int rc = resolve_pending(c, true);
    return rc != PMP_OK ? rc : sync(c);
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

// Host-pointer entry points stage through the context's own buffers (d_in, d_logit, d_out) and return final results.  A *_device call
// that is still in flight may re-run into those very buffers once its range flag is looked at (and a replayed post-processing call may
// read them), so everything pending is made final BEFORE the host call stages anything: afterwards the queue holds this call only.
static int settle_before_host_call(pmp_ctx *c) { return c->pending.empty() ? PMP_OK : settle(c); }

static int h2d(pmp_ctx *c, DevBuf &b, const void *src, size_t bytes)
{
    int rc = ensure(c, b, bytes ? bytes : 1);
    if (rc != PMP_OK) return rc;
    if (!bytes) return PMP_OK;
    hipError_t e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "hipMemcpyAsync(H2D)");
}

static int d2h(pmp_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!bytes || !dst) return PMP_OK;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "hipMemcpyAsync(D2H)");
}

}  // namespace pmp

using namespace pmp;

extern "C" {

const char *pmp_version(void)
{
    if (const char *v = abl_version()) return v;     // a measurement build says so
    return "pmp-hip 0.6 (gfx950; f16x3 default with calibrated activation scales, bf16x6 and fp32 MFMA datapaths)";
}

const char *pmp_last_error(const pmp_ctx *ctx) { return ctx ? ctx->err.c_str() : global_err(); }

int pmp_create(int device_id, pmp_ctx **out)
{
    if (!out) return set_err(nullptr, PMP_E_INVALID, "pmp_create: out is null");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return set_err(nullptr, PMP_E_NODEVICE, "pmp_create: no HIP device (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return set_err(nullptr, PMP_E_INVALID, "pmp_create: device_id out of range");
    if ((e = hipSetDevice(device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    abl_on_create();     // no-op in the product library (its own environment knobs: PMP_OVERLAP here, PMP_PARK_WORKSPACE at pmp_destroy)
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return set_err(nullptr, PMP_E_NODEVICE, std::string("pmp_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    pmp_ctx *c = new (std::nothrow) pmp_ctx();
    if (!c) return set_err(nullptr, PMP_E_NOMEM, "pmp_create: out of host memory");
    c->device = device_id;
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) { delete c; return hip_fail(nullptr, e, "hipStreamCreate"); }
    c->stream = c->own_stream;
    if (const char *ov = std::getenv("PMP_OVERLAP")) c->overlap = ov[0] == '1' && !ov[1];
    if ((e = hipMalloc((void **)&c->d_sat, 256)) != hipSuccess || (e = hipMemset(c->d_sat, 0, 256)) != hipSuccess) {
        if (c->d_sat) hipFree(c->d_sat);
        hipStreamDestroy(c->own_stream);
        delete c;
        return hip_fail(nullptr, e, "hipMalloc(saturation flag)");
    }
    if ((e = hipHostMalloc((void **)&c->h_sat, PMP_SAT_SLOTS * sizeof(unsigned), hipHostMallocDefault)) != hipSuccess) {
        hipFree(c->d_sat);
        hipStreamDestroy(c->own_stream);
        delete c;
        return hip_fail(nullptr, e, "hipHostMalloc(saturation snapshots)");
    }
    *out = c;
    return PMP_OK;
}

int pmp_destroy(pmp_ctx *c)
{
    if (!c) return PMP_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->stream2) hipStreamSynchronize(c->stream2);
    drop_pending(c);
    ktime_drain(c);
    for (auto &kv : c->nets) free_net_weights(kv.second);
    for (hipEvent_t e : c->event_pool) hipEventDestroy(e);
    park_workspace(c->device, c->ws);
    park_workspace(c->device, c->ws2);
    DevBuf *bufs[] = {&c->ws, &c->ws2, &c->d_in[0], &c->d_in[1], &c->d_in[2], &c->d_logit[0], &c->d_logit[1], &c->d_logit[2],
                      &c->d_out[0], &c->d_out[1], &c->d_out[2], &c->d_out[3], &c->d_frames[0], &c->d_frames[1], &c->d_frames[2],
                      &c->d_lab[0], &c->d_lab[1], &c->d_lab[2], &c->d_lab[3], &c->d_lab[4], &c->d_val[0], &c->d_val[1], &c->d_val[2],
                      &c->d_val[3], &c->d_val[4], &c->d_val[5], &c->d_valpart, &c->d_valout};
    for (DevBuf *b : bufs) if (b->p) hipFree(b->p);
    for (TapRec &t : c->taps) if (t.buf.p) hipFree(t.buf.p);
    if (c->d_sat) hipFree(c->d_sat);
    if (c->d_cal) hipFree(c->d_cal);
    if (c->d_calbuf.p) hipFree(c->d_calbuf.p);
    if (c->ws_cal.p) hipFree(c->ws_cal.p);
    if (c->cal_stream) hipStreamDestroy(c->cal_stream);
    if (c->h_sat) hipHostFree(c->h_sat);
    if (c->stream2) hipStreamDestroy(c->stream2);
    hipStreamDestroy(c->own_stream);
    delete c;
    return PMP_OK;
}

int pmp_trim(void)
{
    std::lock_guard<std::mutex> lk(g_park_mutex);
    for (auto &kv : g_parked)
        for (DevBuf &b : kv.second.b) if (b.p) hipFree(b.p);          // hipFree needs no current device: the caller's stays as it is
    g_parked.clear();
    return PMP_OK;
}

int pmp_set_stream(pmp_ctx *c, void *hip_stream)
{
    CHECK_CTX(c);
    if (!c->pending.empty()) { const int rc = settle(c); if (rc != PMP_OK) return rc; }   // calls in flight belong to the old stream
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    return PMP_OK;
}

int pmp_synchronize(pmp_ctx *c) { CHECK_CTX(c); return settle(c); }

int pmp_set_overlap(pmp_ctx *c, int on)
{
    CHECK_CTX(c);
    if (!c->pending.empty()) { const int rc = settle(c); if (rc != PMP_OK) return rc; }   // calls in flight keep the cut they were made with
    c->overlap = on ? 1 : 0;
    if (!c->overlap && c->ws2.p) { hipFree(c->ws2.p); c->ws2 = DevBuf(); }                // the second workspace exists only while the mode is on
    return PMP_OK;
}

int pmp_set_chunk(pmp_ctx *c, int blocks)
{
    CHECK_CTX(c);
    if (blocks < 1 || blocks > 4096) return set_err(c, PMP_E_INVALID, "pmp_set_chunk: 1..4096");   // 32-bit element offsets inside one activation tensor
    c->chunk = blocks;
    return PMP_OK;
}

int64_t pmp_get_workspace_bytes(const pmp_ctx *c) { return c ? (int64_t)(c->ws_need + c->ws2.cap) : PMP_E_INVALID; }   // + the second workspace while overlap mode holds one

int pmp_set_precision(pmp_ctx *c, int mode)
{
    CHECK_CTX(c);
    if (mode != PMP_PRECISION_F32 && mode != PMP_PRECISION_BF16X6 && mode != PMP_PRECISION_F16X3)
        return set_err(c, PMP_E_INVALID, "pmp_set_precision: 0 (fp32), 1 (bf16x6) or 2 (f16x3)");
    int rc = settle(c);
    if (rc != PMP_OK) return rc;
    c->precision = mode;
    return PMP_OK;
}

int pmp_get_precision(const pmp_ctx *c) { return c ? c->precision : PMP_E_INVALID; }

int pmp_set_saturation_policy(pmp_ctx *c, int policy)
{
    CHECK_CTX(c);
    if (policy != PMP_SAT_RERUN && policy != PMP_SAT_ERROR && policy != PMP_SAT_IGNORE)
        return set_err(c, PMP_E_INVALID, "pmp_set_saturation_policy: PMP_SAT_RERUN, PMP_SAT_ERROR or PMP_SAT_IGNORE");
    if (!c->pending.empty()) { const int rc = settle(c); if (rc != PMP_OK) return rc; }   // calls in flight keep the policy they were made under
    c->sat_policy = policy;
    return PMP_OK;
}

int pmp_get_saturation(pmp_ctx *c)
{
    CHECK_CTX(c);
    int rc = settle(c);          // flags of the calls in flight (re-runs included)
    if (rc != PMP_OK) return rc;
    unsigned fired = 0;          // under PMP_SAT_IGNORE no call takes a snapshot: read the device word itself
    if ((rc = sat_fetch(c, &fired)) != PMP_OK) return rc;
    if (fired) c->sat_seen = 1;
    return c->sat_seen;
}

int64_t pmp_get_saturation_reruns(const pmp_ctx *c) { return c ? c->sat_reruns : PMP_E_INVALID; }

int pmp_clear_saturation(pmp_ctx *c)
{
    CHECK_CTX(c);
    unsigned fired = 0;
    int rc = settle(c);
    if (rc == PMP_OK) rc = sat_fetch(c, &fired);
    c->sat_seen = 0;
    c->sat_reruns = 0;
    return rc;
}

// The two loaders' common end.  wf: the file the tensors came from (its manifest may carry the activation-scale exponents), or null.
static int load_weights(pmp_ctx *c, int net_id, int qp, const float *blob, const pmp_tensor_desc *descs, int ndesc, const WeightFile *wf)
{
    // REPLACING a net waits for the calls in flight (a range-guard re-run must still find the weights it ran with, and kernels may
    // be reading them); ADDING one does not - the upload runs next to whatever the stream is doing, so a driver can load the next
    // (component, QP) while the GPU works on this one
    int rc = find_net(c, net_id, qp) ? settle(c) : PMP_OK;
    if (rc != PMP_OK) return rc;
    if ((rc = load_net_weights(c, net_id, qp, blob, descs, ndesc)) != PMP_OK) return rc;
    if (net_id == PMP_NET_LUMA_Q || net_id == PMP_NET_CHROMA_Q) qt_partner_changed(c, net_id, qp);
    if (wf && wf->act_exp.size() == 5 && (net_id == PMP_NET_LUMA_MSBD || net_id == PMP_NET_CHROMA_MSBD)) {
        // The file carries its activation-scale exponents (tools/calibrate_pmpw.py calibrated once): nothing to run here - IF they belong
        // to these tensors.  The reader has bounded them (pmpw_file.cpp); "act_fp" says which tensors and which QT partner they were
        // calibrated on: a manifest whose fingerprints do not match (tensors edited, the QT net replaced since) is stale, and its
        // exponents are ignored in favour of a calibration pass.  A QT partner that is not loaded yet is checked when it arrives.
        NetWeights *nw = find_net(c, net_id, qp);
        NetWeights *wq = find_net(c, net_id == PMP_NET_LUMA_MSBD ? PMP_NET_LUMA_Q : PMP_NET_CHROMA_Q, qp);
        const bool stale = wf->have_fp && (wf->act_mtt_fp != nw->fp || (wq && wf->act_qt_fp != wq->fp));
        if (!stale) {
            if ((rc = set_activation_scales(c, *nw, wf->act_exp.data())) != PMP_OK) return rc;
            nw->calibrated = true;
            nw->act_from_file = true;
            nw->act_fp_known = wf->have_fp;
            nw->act_qt_fp = wf->act_qt_fp;
            nw->cal_names.clear(); nw->cal_seg.clear(); nw->cal_amax.clear();
            return PMP_OK;
        }
    }
    return calibrate_if_ready(c, net_id, qp);
}

int pmp_load_weights(pmp_ctx *c, int net_id, int qp, const float *blob, const pmp_tensor_desc *descs, int ndesc)
{
    CHECK_CTX(c);
    return load_weights(c, net_id, qp, blob, descs, ndesc, nullptr);
}

int pmp_weights_fingerprint(const pmp_ctx *c, int net_id, int qp, uint64_t *out)
{
    if (!c || !out) return set_err(nullptr, PMP_E_INVALID, "pmp_weights_fingerprint: null argument");
    const NetWeights *w = find_net(const_cast<pmp_ctx *>(c), net_id, qp);
    if (!w) return PMP_E_NOWEIGHTS;
    *out = w->fp;
    return PMP_OK;
}

int pmp_load_weights_file(pmp_ctx *c, int net_id, int qp, const char *path)
{
    CHECK_CTX(c);
    WeightFile wf;
    int rc = read_pmpw(path, wf);
    if (rc != PMP_OK) return set_err(c, rc, global_err());
    if (!wf.net.empty() && net_id_of(wf.net) != net_id)
        return set_err(c, PMP_E_INVALID, std::string(path) + ": holds net " + wf.net + ", not the net asked for");
    if (wf.qp >= 0 && wf.qp != qp) return set_err(c, PMP_E_INVALID, std::string(path) + ": holds QP " + std::to_string(wf.qp));
    std::vector<pmp_tensor_desc> descs(wf.tensors.size());
    for (size_t i = 0; i < wf.tensors.size(); ++i) {
        descs[i].name = wf.tensors[i].name.c_str();
        descs[i].ndim = wf.tensors[i].ndim;
        for (int j = 0; j < 4; ++j) descs[i].shape[j] = wf.tensors[i].shape[j];
        descs[i].offset = wf.tensors[i].offset;
    }
    return load_weights(c, net_id, qp, wf.payload.data(), descs.data(), (int)descs.size(), &wf);
}

int pmp_has_weights(const pmp_ctx *c, int net_id, int qp) { return c && find_net(const_cast<pmp_ctx *>(c), net_id, qp); }

int pmp_set_partition_params(pmp_ctx *c, int comp, const pmp_partition_params *p)
{
    CHECK_CTX(c);
    if (comp != PMP_LUMA && comp != PMP_CHROMA) return set_err(c, PMP_E_INVALID, "pmp_set_partition_params: comp must be PMP_LUMA or PMP_CHROMA");
    if (!p) { c->m2p[comp] = M2P_DEFAULT; return PMP_OK; }
    std::string why;
    if (!partition_params_valid(*p, why)) return set_err(c, PMP_E_INVALID, "pmp_set_partition_params: " + why);
    // no settling: calls already enqueued captured their set (post_device_impl), so nothing in flight can see this one
    for (int i = 0; i < 5; ++i) c->m2p[comp].lamb[i] = p->lamb[i];
    c->m2p[comp].thd = p->thd;
    return PMP_OK;
}

int pmp_get_partition_params(const pmp_ctx *c, int comp, pmp_partition_params *out)
{
    if (!c || !out) return set_err(nullptr, PMP_E_INVALID, "pmp_get_partition_params: null argument");
    if (comp != PMP_LUMA && comp != PMP_CHROMA) return set_err(nullptr, PMP_E_INVALID, "pmp_get_partition_params: comp must be PMP_LUMA or PMP_CHROMA");
    for (int i = 0; i < 5; ++i) out->lamb[i] = c->m2p[comp].lamb[i];
    out->thd = c->m2p[comp].thd;
    return PMP_OK;
}

int pmp_infer_device(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n,
                     float *qt, float *bt, float *dire)
{
    CHECK_CTX(c);
    return infer_device_impl(c, comp, qp, by, bu, bv, n, qt, bt, dire);
}

int pmp_postprocess_device(pmp_ctx *c, int comp, const float *qt, const float *bt, const float *dire, int64_t n,
                           uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8)
{
    CHECK_CTX(c);
    return post_device_impl(c, comp, qt, bt, dire, n, hor, ver, qt_u8, dire_i8);
}

int pmp_infer_postprocess_device(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
                                 int64_t n, uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8, float *qt,
                                 float *bt, float *dire)
{
    CHECK_CTX(c);
    int rc;
    const bool own = !qt || !bt || !dire;
    if (own && (rc = ensure_logits(c, n))) return rc;
    if (!qt) qt = (float *)c->d_logit[0].p;
    if (!bt) bt = (float *)c->d_logit[1].p;
    if (!dire) dire = (float *)c->d_logit[2].p;
    if ((rc = infer_device_impl(c, comp, qp, by, bu, bv, n, qt, bt, dire, own))) return rc;
    return post_device_impl(c, comp, qt, bt, dire, n, hor, ver, qt_u8, dire_i8);
}

// ---- packed records: hor[256] | ver[256] | qt[64] | dire[768] per block, the unit of the multi-GPU gather ------------
static int post_records(pmp_ctx *c, int comp, const float *qt, const float *bt, const float *dire, int64_t n, uint8_t *rec)
{
    if (n == 0) return PMP_OK;   // an empty shard: torch.empty((0, 1344)).data_ptr() is 0, as for the four-array entry points
    if (!rec || (reinterpret_cast<uintptr_t>(rec) & 3)) return set_err(c, PMP_E_INVALID, "records: null or unaligned (4 bytes) buffer");
    return post_device_impl(c, comp, qt, bt, dire, n, rec, rec + 256, rec + 512, reinterpret_cast<int8_t *>(rec + 576), PMP_RECORD_BYTES);
}

int pmp_postprocess_records_device(pmp_ctx *c, int comp, const float *qt, const float *bt, const float *dire, int64_t n, uint8_t *rec)
{
    CHECK_CTX(c);
    return post_records(c, comp, qt, bt, dire, n, rec);
}

int pmp_infer_postprocess_records_device(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
                                         int64_t n, uint8_t *rec)
{
    CHECK_CTX(c);
    if (n == 0) return PMP_OK;   // an empty shard has no buffers at all
    int rc;
    if ((rc = ensure_logits(c, n))) return rc;
    float *qt = (float *)c->d_logit[0].p, *bt = (float *)c->d_logit[1].p, *dire = (float *)c->d_logit[2].p;
    if ((rc = infer_device_impl(c, comp, qp, by, bu, bv, n, qt, bt, dire, true))) return rc;
    return post_records(c, comp, qt, bt, dire, n, rec);
}

// ---- host-pointer entry points: stage through device buffers owned by the context ------------------------
static int stage_blocks(pmp_ctx *c, int comp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n)
{
    int rc;
    if ((rc = h2d(c, c->d_in[0], by, (size_t)n * 68 * 68))) return rc;
    if (comp == PMP_CHROMA) {
        if ((rc = h2d(c, c->d_in[1], bu, (size_t)n * 34 * 34))) return rc;
        if ((rc = h2d(c, c->d_in[2], bv, (size_t)n * 34 * 34))) return rc;
    }
    return PMP_OK;
}

int pmp_infer(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n, float *qt,
              float *bt, float *dire)
{
    CHECK_CTX(c);
    if (n < 0 || !by || !qt || !bt || !dire || (comp == PMP_CHROMA && (!bu || !bv)))
        return set_err(c, PMP_E_INVALID, "pmp_infer: null buffer or negative count");
    if (n == 0) return PMP_OK;
    int rc;
    if ((rc = settle_before_host_call(c))) return rc;
    if ((rc = stage_blocks(c, comp, by, bu, bv, n))) return rc;
    if ((rc = ensure_logits(c, n))) return rc;
    float *dq = (float *)c->d_logit[0].p, *db = (float *)c->d_logit[1].p, *dd = (float *)c->d_logit[2].p;
    if ((rc = infer_device_impl(c, comp, qp, (const uint8_t *)c->d_in[0].p, (const uint8_t *)c->d_in[1].p,
                                (const uint8_t *)c->d_in[2].p, n, dq, db, dd, true)))
        return rc;
    if ((rc = resolve_pending(c, true))) return rc;      // range guard: a re-run is enqueued before the copies below
    if ((rc = d2h(c, qt, dq, (size_t)n * 64 * 4)) || (rc = d2h(c, bt, db, (size_t)n * 768 * 4)) ||
        (rc = d2h(c, dire, dd, (size_t)n * 768 * 4)))
        return rc;
    return sync(c);
}

static int alloc_out(pmp_ctx *c, int64_t n)
{
    int rc;
    if ((rc = ensure(c, c->d_out[0], (size_t)n * 256)) || (rc = ensure(c, c->d_out[1], (size_t)n * 256)) ||
        (rc = ensure(c, c->d_out[2], (size_t)n * 64)) || (rc = ensure(c, c->d_out[3], (size_t)n * 768)))
        return rc;
    return PMP_OK;
}

static int fetch_out(pmp_ctx *c, int64_t n, uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8)
{
    int rc;
    if ((rc = resolve_pending(c, true))) return rc;      // range guard: re-run and replay are enqueued before the copies below
    if ((rc = d2h(c, hor, c->d_out[0].p, (size_t)n * 256)) || (rc = d2h(c, ver, c->d_out[1].p, (size_t)n * 256)) ||
        (rc = d2h(c, qt_u8, c->d_out[2].p, (size_t)n * 64)) || (rc = d2h(c, dire_i8, c->d_out[3].p, (size_t)n * 768)))
        return rc;
    return sync(c);
}

int pmp_postprocess(pmp_ctx *c, int comp, const float *qt, const float *bt, const float *dire, int64_t n, uint8_t *hor,
                    uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8)
{
    CHECK_CTX(c);
    if (n < 0 || !qt || !bt || !dire || !hor || !ver || !qt_u8 || !dire_i8)
        return set_err(c, PMP_E_INVALID, "pmp_postprocess: null buffer or negative count");
    if (n == 0) return PMP_OK;
    int rc;
    if ((rc = settle_before_host_call(c))) return rc;
    if ((rc = ensure_logits(c, n))) return rc;
    if ((rc = h2d(c, c->d_logit[0], qt, (size_t)n * 64 * 4)) || (rc = h2d(c, c->d_logit[1], bt, (size_t)n * 768 * 4)) ||
        (rc = h2d(c, c->d_logit[2], dire, (size_t)n * 768 * 4)) || (rc = alloc_out(c, n)))
        return rc;
    if ((rc = post_device_impl(c, comp, (float *)c->d_logit[0].p, (float *)c->d_logit[1].p, (float *)c->d_logit[2].p, n,
                               (uint8_t *)c->d_out[0].p, (uint8_t *)c->d_out[1].p, (uint8_t *)c->d_out[2].p,
                               (int8_t *)c->d_out[3].p)))
        return rc;
    return fetch_out(c, n, hor, ver, qt_u8, dire_i8);
}

int pmp_infer_postprocess(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n,
                          uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8, float *qt, float *bt, float *dire)
{
    CHECK_CTX(c);
    if (n < 0 || !by || !hor || !ver || !qt_u8 || !dire_i8 || (comp == PMP_CHROMA && (!bu || !bv)))
        return set_err(c, PMP_E_INVALID, "pmp_infer_postprocess: null buffer or negative count");
    if (n == 0) return PMP_OK;
    int rc;
    if ((rc = settle_before_host_call(c))) return rc;
    if ((rc = stage_blocks(c, comp, by, bu, bv, n)) || (rc = alloc_out(c, n))) return rc;
    if ((rc = ensure_logits(c, n))) return rc;
    float *dq = (float *)c->d_logit[0].p, *db = (float *)c->d_logit[1].p, *dd = (float *)c->d_logit[2].p;
    if ((rc = infer_device_impl(c, comp, qp, (const uint8_t *)c->d_in[0].p, (const uint8_t *)c->d_in[1].p,
                                (const uint8_t *)c->d_in[2].p, n, dq, db, dd, true)))
        return rc;
    if ((rc = post_device_impl(c, comp, dq, db, dd, n, (uint8_t *)c->d_out[0].p, (uint8_t *)c->d_out[1].p,
                               (uint8_t *)c->d_out[2].p, (int8_t *)c->d_out[3].p)))
        return rc;
    if ((rc = resolve_pending(c, true))) return rc;
    if ((rc = d2h(c, qt, dq, (size_t)n * 64 * 4)) || (rc = d2h(c, bt, db, (size_t)n * 768 * 4)) ||
        (rc = d2h(c, dire, dd, (size_t)n * 768 * 4)))
        return rc;
    return fetch_out(c, n, hor, ver, qt_u8, dire_i8);
}

int pmp_cut_blocks_device(pmp_ctx *c, const void *y, const void *u, const void *v, int F, int H, int W, int bitdepth,
                          uint8_t *by, uint8_t *bu, uint8_t *bv)
{
    CHECK_CTX(c);
    if (!y || !u || !v || !by || !bu || !bv || F < 0 || H < 0 || W < 0 || (H & 1) || (W & 1) || (bitdepth != 8 && bitdepth != 10))
        return set_err(c, PMP_E_INVALID, "pmp_cut_blocks: bad arguments (bitdepth 8 or 10, even H/W)");
    hipError_t e = launch_cut_blocks(c->stream, y, u, v, F, H, W, bitdepth, by, bu, bv);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "cut_blocks");
}

int pmp_cut_blocks(pmp_ctx *c, const void *y, const void *u, const void *v, int F, int H, int W, int bitdepth, uint8_t *by,
                   uint8_t *bu, uint8_t *bv)
{
    CHECK_CTX(c);
    if (!y || !u || !v || !by || !bu || !bv || F < 0 || H < 0 || W < 0 || (H & 1) || (W & 1) || (bitdepth != 8 && bitdepth != 10))
        return set_err(c, PMP_E_INVALID, "pmp_cut_blocks: bad arguments (bitdepth 8 or 10, even H/W)");
    const size_t bps = bitdepth == 8 ? 1 : 2, ny = (size_t)F * H * W * bps, nc = (size_t)F * (H / 2) * (W / 2) * bps;
    const int64_t n = (int64_t)F * (H / 64) * (W / 64);
    if (n == 0) return PMP_OK;
    int rc;
    if ((rc = h2d(c, c->d_frames[0], y, ny)) || (rc = h2d(c, c->d_frames[1], u, nc)) || (rc = h2d(c, c->d_frames[2], v, nc)))
        return rc;
    if ((rc = ensure(c, c->d_in[0], (size_t)n * 68 * 68)) || (rc = ensure(c, c->d_in[1], (size_t)n * 34 * 34)) ||
        (rc = ensure(c, c->d_in[2], (size_t)n * 34 * 34)))
        return rc;
    hipError_t e = launch_cut_blocks(c->stream, c->d_frames[0].p, c->d_frames[1].p, c->d_frames[2].p, F, H, W, bitdepth,
                                     (uint8_t *)c->d_in[0].p, (uint8_t *)c->d_in[1].p, (uint8_t *)c->d_in[2].p);
    if (e != hipSuccess) return hip_fail(c, e, "cut_blocks");
    if ((rc = d2h(c, by, c->d_in[0].p, (size_t)n * 68 * 68)) || (rc = d2h(c, bu, c->d_in[1].p, (size_t)n * 34 * 34)) ||
        (rc = d2h(c, bv, c->d_in[2].p, (size_t)n * 34 * 34)))
        return rc;
    return sync(c);
}

// ---- training labels: GenMSBtMap (labels.hip) --------------------------------------------------------------------------
static int msbt_args(pmp_ctx *c, int cf, const void *qt, const void *bt, const void *dire, int64_t n, const void *msbt, const void *status)
{
    if (cf != 1 && cf != 2) return set_err(c, PMP_E_INVALID, "pmp_msbt_labels: cf must be 1 or 2");
    if (n < 0) return set_err(c, PMP_E_INVALID, "pmp_msbt_labels: negative count");
    if (n > 0 && (!qt || !bt || !dire || !msbt || !status)) return set_err(c, PMP_E_INVALID, "pmp_msbt_labels: null buffer");
    return PMP_OK;
}

int pmp_msbt_labels_device(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *msbt,
                           uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = msbt_args(c, cf, qt, bt, dire, n, msbt, status))) return rc;
    if (n == 0) return PMP_OK;
    if (((uintptr_t)qt | (uintptr_t)bt | (uintptr_t)dire | (uintptr_t)msbt) & 3)
        return set_err(c, PMP_E_INVALID, "pmp_msbt_labels_device: qt, bt, dire and msbt must be 4-byte aligned");
    const hipError_t e = launch_msbt_labels(c->stream, qt, bt, dire, n, cf, msbt, status);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "msbt_labels");
}

int pmp_msbt_labels(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *msbt,
                    uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = msbt_args(c, cf, qt, bt, dire, n, msbt, status))) return rc;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    // passes of at most `chunk` blocks through the context's own staging buffers (about 1.9 kB per block)
    const int64_t chunk = c->chunk;
    const int64_t m0 = n < chunk ? n : chunk;
    const size_t per[5] = {64, 256, 768, 768, 1};
    for (int i = 0; i < 5; ++i)
        if ((rc = ensure(c, c->d_lab[i], (size_t)m0 * per[i]))) return rc;
    for (int64_t o = 0; o < n; o += chunk) {
        const int64_t m = (n - o) < chunk ? (n - o) : chunk;
        if (c->poison) {          // pmp_debug_poison_workspace: the kernel must write every output byte it hands back
            for (int i = 3; i < 5; ++i) {
                const hipError_t e = hipMemsetAsync(c->d_lab[i].p, poison_byte(c), (size_t)m * per[i], c->stream);
                if (e != hipSuccess) return hip_fail(c, e, "poison label buffers");
            }
        }
        if ((rc = h2d(c, c->d_lab[0], qt + o * 64, (size_t)m * 64)) || (rc = h2d(c, c->d_lab[1], bt + o * 256, (size_t)m * 256)) ||
            (rc = h2d(c, c->d_lab[2], dire + o * 768, (size_t)m * 768)))
            return rc;
        const hipError_t e = launch_msbt_labels(c->stream, (const uint8_t *)c->d_lab[0].p, (const uint8_t *)c->d_lab[1].p,
                                                (const int8_t *)c->d_lab[2].p, m, cf, (uint8_t *)c->d_lab[3].p, (uint8_t *)c->d_lab[4].p);
        if (e != hipSuccess) return hip_fail(c, e, "msbt_labels");
        if ((rc = d2h(c, msbt + o * 768, c->d_lab[3].p, (size_t)m * 768)) || (rc = d2h(c, status + o, c->d_lab[4].p, (size_t)m)))
            return rc;
        if ((rc = sync(c))) return rc;   // the next pass reuses the staging buffers
    }
    return PMP_OK;
}

// ---- the labels' own partition: Map_to_SubMap.get_partition (labels.hip) -------------------------------------------------
static int lpart_args(pmp_ctx *c, int cf, const void *qt, const void *bt, const void *dire, int64_t n, const void *o0, const void *o1,
                      const void *status)
{
    if (cf != 1 && cf != 2) return set_err(c, PMP_E_INVALID, "pmp_label_partition: cf must be 1 or 2");
    if (n < 0) return set_err(c, PMP_E_INVALID, "pmp_label_partition: negative count");
    if (n > 0 && (!qt || !bt || !dire || !o0 || !o1 || !status)) return set_err(c, PMP_E_INVALID, "pmp_label_partition: null buffer");
    return PMP_OK;
}

int pmp_label_partition_device(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *hor,
                               uint8_t *ver, uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = lpart_args(c, cf, qt, bt, dire, n, hor, ver, status))) return rc;
    if (n == 0) return PMP_OK;
    if (((uintptr_t)qt | (uintptr_t)bt | (uintptr_t)dire | (uintptr_t)hor | (uintptr_t)ver) & 3)
        return set_err(c, PMP_E_INVALID, "pmp_label_partition_device: qt, bt, dire, hor and ver must be 4-byte aligned");
    const hipError_t e = launch_label_partition(c->stream, qt, bt, dire, n, cf, hor, ver, nullptr, status);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "label_partition");
}

int pmp_label_partition_records_device(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n,
                                       uint8_t *rec, uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = lpart_args(c, cf, qt, bt, dire, n, rec, rec, status))) return rc;
    if (n == 0) return PMP_OK;
    if (((uintptr_t)qt | (uintptr_t)bt | (uintptr_t)dire | (uintptr_t)rec) & 3)
        return set_err(c, PMP_E_INVALID, "pmp_label_partition_records_device: qt, bt, dire and rec must be 4-byte aligned");
    const hipError_t e = launch_label_partition(c->stream, qt, bt, dire, n, cf, nullptr, nullptr, rec, status);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "label_partition");
}

int pmp_label_partition(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *hor,
                        uint8_t *ver, uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = lpart_args(c, cf, qt, bt, dire, n, hor, ver, status))) return rc;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    // passes of at most `chunk` blocks through the staging buffers of pmp_msbt_labels; hor and ver share its 768-byte-per-block output
    const int64_t chunk = c->chunk;
    const int64_t m0 = n < chunk ? n : chunk;
    const size_t per[5] = {64, 256, 768, 768, 1};
    for (int i = 0; i < 5; ++i)
        if ((rc = ensure(c, c->d_lab[i], (size_t)m0 * per[i]))) return rc;
    for (int64_t o = 0; o < n; o += chunk) {
        const int64_t m = (n - o) < chunk ? (n - o) : chunk;
        uint8_t *d_hor = (uint8_t *)c->d_lab[3].p, *d_ver = d_hor + (size_t)m * 256;
        if (c->poison) {          // pmp_debug_poison_workspace: the kernel must write every output byte it hands back
            for (int i = 3; i < 5; ++i) {
                const hipError_t e = hipMemsetAsync(c->d_lab[i].p, poison_byte(c), (size_t)m * per[i], c->stream);
                if (e != hipSuccess) return hip_fail(c, e, "poison label buffers");
            }
        }
        if ((rc = h2d(c, c->d_lab[0], qt + o * 64, (size_t)m * 64)) || (rc = h2d(c, c->d_lab[1], bt + o * 256, (size_t)m * 256)) ||
            (rc = h2d(c, c->d_lab[2], dire + o * 768, (size_t)m * 768)))
            return rc;
        const hipError_t e = launch_label_partition(c->stream, (const uint8_t *)c->d_lab[0].p, (const uint8_t *)c->d_lab[1].p,
                                                    (const int8_t *)c->d_lab[2].p, m, cf, d_hor, d_ver, nullptr, (uint8_t *)c->d_lab[4].p);
        if (e != hipSuccess) return hip_fail(c, e, "label_partition");
        if ((rc = d2h(c, hor + o * 256, d_hor, (size_t)m * 256)) || (rc = d2h(c, ver + o * 256, d_ver, (size_t)m * 256)) ||
            (rc = d2h(c, status + o, c->d_lab[4].p, (size_t)m)))
            return rc;
        if ((rc = sync(c))) return rc;   // the next pass reuses the staging buffers
    }
    return PMP_OK;
}

// ---- validation statistics (valstats.hip) and teacher-forced MTT inference ------------------------------------------------
namespace {
struct ValArgs {
    const float *qt, *bt, *dire;
    const uint8_t *qt8, *msbt;
    const int8_t *msdire;
    int64_t n;
    float wm[3];
    int w0_one;
    double *stats, *block_stats;       // block_stats null: the context's scratch, looked up at launch (a replay may find it regrown)
};
}  // namespace

static int val_check(pmp_ctx *c, int qp, const void *qt, const void *bt, const void *dire, const void *qt8, const void *msbt,
                     const void *msdire, int64_t n, const void *stats, float wm[3], int *w0_one)
{
    // Metrics.py:148-151; the float64 entry becomes a float32 scalar when torch adds it to the float32 dl*dl
    static const double weight_mat[4][3] = {{0.5 * 1.0, 0.5 * 0.73, 0.5 * 0.15}, {0.5 * 2.43, 0.5 * 0.35, 0.5 * 0.10},
                                            {0.5 * 0.96, 0.5 * 0.23, 0.5 * 0.07}, {0.5 * 0.59, 0.5 * 0.16, 0.5 * 0.05}};
    if (qp < 22 || qp > 41) return set_err(c, PMP_E_INVALID, "pmp_val_stats: qp must be in 22..41 (rows 0..3 of weight_mat)");
    if (n < 0 || !stats) return set_err(c, PMP_E_INVALID, "pmp_val_stats: negative count or null stats");
    const bool q = qt && qt8, noq = !qt && !qt8, m = bt && dire && msbt && msdire, nom = !bt && !dire && !msbt && !msdire;
    if (n > 0 && !((q && m) || (q && nom) || (noq && m)))
        return set_err(c, PMP_E_INVALID, "pmp_val_stats: pass (qt, qt8), (bt, dire, msbt, msdire) or both; no other NULL mix");
    const int row = (qp - 22) / 5;
    for (int k = 0; k < 3; ++k) wm[k] = (float)weight_mat[row][k];
    *w0_one = qp == 22;
    return PMP_OK;
}

static int val_launch(pmp_ctx *c, const ValArgs &a)
{
    double *part = a.block_stats;
    if (!part) {
        const int rc = ensure(c, c->d_valpart, (size_t)a.n * PMP_VAL_NSTATS * sizeof(double));
        if (rc != PMP_OK) return rc;
        part = (double *)c->d_valpart.p;
    }
    const hipError_t e = launch_val_stats(c->stream, a.qt, a.bt, a.dire, a.qt8, a.msbt, a.msdire, a.n, a.wm, a.w0_one, part, a.stats);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "val_stats");
}

static int val_device_impl(pmp_ctx *c, const ValArgs &a)
{
    if (a.n == 0) {
        const hipError_t e = hipMemsetAsync(a.stats, 0, PMP_VAL_NSTATS * sizeof(double), c->stream);
        return e == hipSuccess ? PMP_OK : hip_fail(c, e, "val_stats");
    }
    const int rc = val_launch(c, a);
    // its logits may come from an inference call whose range flag has not been looked at yet: remember the call for the replay
    if (rc == PMP_OK && !c->pending.empty())
        c->pending.push_back(PendingCall{false, false, nullptr, nullptr, [=](bool) { return val_launch(c, a); }});
    return rc;
}

int pmp_val_stats_device(pmp_ctx *c, int qp, const float *qt, const float *bt, const float *dire, const uint8_t *qt8,
                         const uint8_t *msbt, const int8_t *msdire, int64_t n, double *stats, double *block_stats)
{
    CHECK_CTX(c);
    ValArgs a{qt, bt, dire, qt8, msbt, msdire, n, {0.f, 0.f, 0.f}, 0, stats, block_stats};
    int rc;
    if ((rc = val_check(c, qp, qt, bt, dire, qt8, msbt, msdire, n, stats, a.wm, &a.w0_one))) return rc;
    if (n > 0 && ((((uintptr_t)bt | (uintptr_t)dire) & 15) || (((uintptr_t)qt | (uintptr_t)msbt | (uintptr_t)msdire) & 3) ||
                  (((uintptr_t)stats | (uintptr_t)block_stats) & 7)))
        return set_err(c, PMP_E_INVALID, "pmp_val_stats_device: bt, dire must be 16-byte aligned, qt, msbt, msdire 4-byte, the outputs 8-byte");
    return val_device_impl(c, a);
}

int pmp_val_stats(pmp_ctx *c, int qp, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                  const int8_t *msdire, int64_t n, double stats[PMP_VAL_NSTATS])
{
    CHECK_CTX(c);
    ValArgs a{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, {0.f, 0.f, 0.f}, 0, nullptr, nullptr};
    int rc;
    if ((rc = val_check(c, qp, qt, bt, dire, qt8, msbt, msdire, n, stats, a.wm, &a.w0_one))) return rc;
    for (int i = 0; i < PMP_VAL_NSTATS; ++i) stats[i] = 0.0;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    // passes of at most `chunk` blocks through the context's own staging buffers (about 6.9 kB per block); one result row per pass
    const int64_t chunk = c->chunk, m0 = n < chunk ? n : chunk, passes = (n + chunk - 1) / chunk;
    const size_t per[6] = {64 * 4, 768 * 4, 768 * 4, 64, 768, 768};
    const void *src[6] = {qt, bt, dire, qt8, msbt, msdire};
    for (int i = 0; i < 6; ++i)
        if (src[i] && (rc = ensure(c, c->d_val[i], (size_t)m0 * per[i]))) return rc;
    if ((rc = ensure(c, c->d_valout, (size_t)passes * PMP_VAL_NSTATS * sizeof(double)))) return rc;
    for (int64_t o = 0, p = 0; o < n; o += chunk, ++p) {
        const int64_t m = (n - o) < chunk ? (n - o) : chunk;
        for (int i = 0; i < 6; ++i)
            if (src[i] && (rc = h2d(c, c->d_val[i], (const char *)src[i] + (size_t)o * per[i], (size_t)m * per[i]))) return rc;
        a.qt = qt ? (const float *)c->d_val[0].p : nullptr;
        a.bt = bt ? (const float *)c->d_val[1].p : nullptr;
        a.dire = bt ? (const float *)c->d_val[2].p : nullptr;
        a.qt8 = qt ? (const uint8_t *)c->d_val[3].p : nullptr;
        a.msbt = bt ? (const uint8_t *)c->d_val[4].p : nullptr;
        a.msdire = bt ? (const int8_t *)c->d_val[5].p : nullptr;
        a.n = m;
        a.stats = (double *)c->d_valout.p + p * PMP_VAL_NSTATS;
        if ((rc = val_launch(c, a))) return rc;
        if ((rc = sync(c))) return rc;   // the next pass reuses the staging buffers
    }
    std::vector<double> rows((size_t)passes * PMP_VAL_NSTATS);
    if ((rc = d2h(c, rows.data(), c->d_valout.p, rows.size() * sizeof(double))) || (rc = sync(c))) return rc;
    for (int64_t p = 0; p < passes; ++p)          // the whole call as one batch: pass results in pass order
        for (int i = 0; i < PMP_VAL_NSTATS; ++i) stats[i] += rows[(size_t)p * PMP_VAL_NSTATS + i];
    return PMP_OK;
}

int pmp_infer_msbd_device(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, const float *qt_in,
                          int64_t n, float *bt, float *dire)
{
    CHECK_CTX(c);
    if (!qt_in) return set_err(c, PMP_E_INVALID, "pmp_infer_msbd: qt_in is null");
    return infer_device_impl(c, comp, qp, by, bu, bv, n, nullptr, bt, dire, false, qt_in);
}

int pmp_infer_msbd(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, const float *qt_in, int64_t n,
                   float *bt, float *dire)
{
    CHECK_CTX(c);
    if (n < 0 || !by || !qt_in || !bt || !dire || (comp == PMP_CHROMA && (!bu || !bv)))
        return set_err(c, PMP_E_INVALID, "pmp_infer_msbd: null buffer or negative count");
    if (n == 0) return PMP_OK;
    int rc;
    if ((rc = settle_before_host_call(c))) return rc;
    if ((rc = stage_blocks(c, comp, by, bu, bv, n))) return rc;
    if ((rc = ensure_logits(c, n))) return rc;
    if ((rc = h2d(c, c->d_logit[0], qt_in, (size_t)n * 64 * 4))) return rc;
    float *db = (float *)c->d_logit[1].p, *dd = (float *)c->d_logit[2].p;
    if ((rc = infer_device_impl(c, comp, qp, (const uint8_t *)c->d_in[0].p, (const uint8_t *)c->d_in[1].p, (const uint8_t *)c->d_in[2].p,
                                n, nullptr, db, dd, true, (const float *)c->d_logit[0].p)))
        return rc;
    if ((rc = resolve_pending(c, true))) return rc;      // range guard: a re-run is enqueued before the copies below
    if ((rc = d2h(c, bt, db, (size_t)n * 768 * 4)) || (rc = d2h(c, dire, dd, (size_t)n * 768 * 4))) return rc;
    return sync(c);
}

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
    float *dx = nullptr, *dy = nullptr, *dy2 = nullptr, *dwp = nullptr;
    unsigned short *dxs = nullptr, *dys = nullptr, *dwx = nullptr;
    hipError_t e = hipSuccess;
    auto A = [&](void **p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    A((void **)&dx, nx * 4); A((void **)&dy, ny * 4); A((void **)&dy2, ny * 4); A((void **)&dwp, wp.size() * 4);
    A((void **)&dxs, nx * 6); A((void **)&dys, ny * 6); A((void **)&dwx, wx.size() * 2);
    int rc = PMP_OK;
    if (e != hipSuccess) rc = hip_fail(c, e, "hipMalloc(conv bench)");
    if (rc == PMP_OK) {
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
        hipEvent_t e0, e1;
        hipEventCreate(&e0); hipEventCreate(&e1);
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
        hipEventDestroy(e0); hipEventDestroy(e1);
        if (e != hipSuccess) rc = hip_fail(c, e, "conv bench");
    }
    abl_bench_free(ab);
    for (void *p : {(void *)dx, (void *)dy, (void *)dy2, (void *)dwp, (void *)dxs, (void *)dys, (void *)dwx}) if (p) hipFree(p);
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
    if (!on) {
        for (TapRec &t : c->taps) if (t.buf.p) hipFree(t.buf.p);
        c->taps.clear();
    }
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
