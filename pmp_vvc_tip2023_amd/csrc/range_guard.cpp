// range_guard.cpp — how an inference call runs and becomes final: workspaces (parked between contexts), the passes of a call, the
// f16x3 range guard's deferred flag snapshots with their re-runs and replays.
#include <cstdlib>
#include <mutex>

#include "pmp_host.h"

namespace pmp {

// ---- parked workspaces.  On this pool a large hipMalloc that follows a hipFree of similar size stalls for 0.5-1.4 s now and then
// (tools/probe/malloc_probe.py: the freed VRAM is still being cleared); a host that destroys a context and creates the next one -
// one per sequence, one per encoder instance - would pay that for its 10 GB activation workspace every time.  pmp_destroy therefore
// PARKS the workspace (two slots per device, the larger buffers win) and the next context on that device takes it over; pmp_trim()
// gives parked memory back to the driver.  PMP_PARK_WORKSPACE=0 in the environment turns parking off (pmp_destroy then frees everything:
// for a host that destroys its context to hand the VRAM to another library and cannot call pmp_trim).
// The registry lives in a heap object that is never destroyed: a buffer still parked at process exit is not freed, because a DevBuf
// destructor running during static destruction would call hipFree after the HIP runtime may already be gone.
namespace {
constexpr int PARK_SLOTS = 2;     // a context in overlap mode owns two workspaces (ws, ws2): both are parked (round 5; one slot until then)
struct Parked { DevBuf b[PARK_SLOTS]; };
struct ParkRegistry { std::mutex mutex; std::map<int, Parked> dev; };   // device -> buffers
ParkRegistry &parked() { static ParkRegistry *r = new ParkRegistry; return *r; }
}  // namespace

void park_workspace(int device, DevBuf &b)
{
    if (!b.p) return;
    const char *env = std::getenv("PMP_PARK_WORKSPACE");
    if (env && env[0] == '0' && !env[1]) { b.reset(); return; }
    std::lock_guard<std::mutex> lk(parked().mutex);
    Parked &pk = parked().dev[device];
    int victim = 0;                                   // an empty slot, else the smallest parked buffer
    for (int i = 0; i < PARK_SLOTS; ++i) {
        if (!pk.b[i].p) { victim = i; break; }
        if (pk.b[i].cap < pk.b[victim].cap) victim = i;
    }
    if (pk.b[victim].p && pk.b[victim].cap >= b.cap) b.reset();                 // everything parked is at least as large: drop the newcomer
    else pk.b[victim] = std::move(b);                                           // ... else the victim goes
}

static bool take_parked(int device, size_t bytes, DevBuf &out)
{
    std::lock_guard<std::mutex> lk(parked().mutex);
    auto it = parked().dev.find(device);
    if (it == parked().dev.end()) return false;
    int best = -1;                                    // the smallest parked buffer that is large enough
    for (int i = 0; i < PARK_SLOTS; ++i)
        if (it->second.b[i].p && it->second.b[i].cap >= bytes && (best < 0 || it->second.b[i].cap < it->second.b[best].cap)) best = i;
    if (best < 0) return false;
    out = std::move(it->second.b[best]);
    return true;
}

void trim_parked()
{
    std::lock_guard<std::mutex> lk(parked().mutex);
    parked().dev.clear();                             // hipFree needs no current device: the caller's stays as it is
}

// A pass's activation workspace: a large one takes a parked one of a destroyed context first (small ones are cheap to allocate and stay small)
static int ensure_workspace(pmp_ctx *c, DevBuf &b, size_t bytes)
{
    DevBuf got;
    if (bytes > b.cap && bytes >= ((size_t)64 << 20) && take_parked(c->device, bytes, got)) {
        b = std::move(got);
        return PMP_OK;
    }
    return ensure(c, b, bytes);
}

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
static int infer_passes(pmp_ctx *c, int precision, bool taps, bool luma, NetWeights &wq, NetWeights *wbp, const uint8_t *by, const uint8_t *bu,
                        const uint8_t *bv, int64_t n, float *qt, float *bt, float *dire, const float *qt_in = nullptr)
{
    // qt_in: teacher-forced MTT inference (pmp_infer_msbd) - the MTT net reads this map, the QT net does not run, qt is not written
    // wbp null: the QT net alone (pmp_infer_q) - no MTT net is looked at, packed, calibrated or run, bt and dire are not written
    int rc0;     // weights are packed per datapath, on first use (the load packed the datapath that was current then)
    if ((rc0 = ensure_datapath(c, wq, precision)) != PMP_OK || (wbp && (rc0 = ensure_datapath(c, *wbp, precision)) != PMP_OK)) return rc0;
    // f16x3: the MTT net's activation scales, from one calibration pass when the net is first used on this datapath
    if (wbp && precision == PMP_PRECISION_F16X3 && c->act_scales && !wbp->calibrated && (rc0 = calibrate_mtt(c, luma, wq, *wbp)) != PMP_OK) return rc0;
    if ((rc0 = abl_prepare_pass(c, precision, wq, wbp)) != PMP_OK) return rc0;
    // Overlap mode: a call of at least 1024 blocks runs as (at least) two chunks, even ones on the context's stream and workspace, odd
    // ones on a second stream with a second workspace, so that one chunk's small launches (stems, 16x16 tails, HBM-bound 32x32 layers)
    // run beside the other's 64x64 convolutions.  Blocks are independent: the results do not depend on how a call is cut.
    const bool overlap = c->overlap && n >= 1024;
    int64_t chunk = c->chunk;
    if (overlap && (n + 1) / 2 < chunk) chunk = (n + 1) / 2;
    if (overlap) {
        hipError_t e = hipSuccess;
        if (!c->stream2) e = hipStreamCreateWithFlags(&c->stream2.h, hipStreamNonBlocking);
        hipEvent_t ev = c->event_pool.get();
        if (e == hipSuccess) e = hipEventRecord(ev, c->stream);              // fork: the second stream starts behind everything enqueued so far
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream2, ev, 0);
        c->event_pool.put(ev);
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
        Pass ps{side ? c->stream2.h : c->stream, side ? c->ws2 : c->ws, precision, taps, /*cal*/ false, /*caller*/ true};
        if (!qt_in) rc = run_graph(c, ps, [&] { return forward_q(c, ps, luma, wq, y, u, v, m, q); });
        if (rc == PMP_OK && wbp) rc = run_graph(c, ps, [&] { return forward_msbd(c, ps, luma, *wbp, y, u, v, qi, m, bt + o * 768, dire + o * 768); });
    }
    if (overlap) {
        hipEvent_t ev = c->event_pool.get();
        hipError_t e = hipEventRecord(ev, c->stream2);                       // join: the caller's stream continues behind both
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
        c->event_pool.put(ev);
        if (e != hipSuccess && rc == PMP_OK) rc = hip_fail(c, e, "overlap: join");
    }
    return rc;
}

// ---- f16x3 range guard (include/pmp.h) ----------------------------------------------------------------------------------
// Reads and clears the device-side saturation word (synchronises the stream): PMP_SAT_IGNORE contexts, whose calls take no snapshots.
int sat_fetch(pmp_ctx *c, unsigned *out)
{
    unsigned h = 0;
    hipError_t e = hipMemcpyAsync(&h, c->d_sat, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && h) e = hipMemsetAsync(c->d_sat, 0, sizeof(unsigned), c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "saturation flag");
    *out = h;
    return PMP_OK;
}

void drop_pending(pmp_ctx *c)
{
    for (auto &p : c->pending) if (p.ev) c->event_pool.put(p.ev);
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
int resolve_pending(pmp_ctx *c, bool wait)
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
        if (p.ev) c->event_pool.put(p.ev);
        c->pending.pop_front();
        if (rc != PMP_OK) { drop_pending(c); return rc; }
    }
    return PMP_OK;
}

int infer_device_impl(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n, float *qt,
                      float *bt, float *dire, bool ctx_logits, const float *qt_in, bool q_only)
{
    const std::string fn = q_only ? "pmp_infer_q" : "pmp_infer";          // the entry point family the messages name
    if (comp != PMP_LUMA && comp != PMP_CHROMA) return set_err(c, PMP_E_INVALID, fn + ": comp must be PMP_LUMA or PMP_CHROMA");
    if (n < 0 || !by || (!qt && !qt_in) || (!q_only && (!bt || !dire)) || (comp == PMP_CHROMA && (!bu || !bv)))
        return set_err(c, PMP_E_INVALID, fn + ": null buffer or negative count");
    const bool luma = comp == PMP_LUMA;
    const int id_q = luma ? PMP_NET_LUMA_Q : PMP_NET_CHROMA_Q, id_b = luma ? PMP_NET_LUMA_MSBD : PMP_NET_CHROMA_MSBD;
    NetWeights *wq = find_net(c, id_q, qp);
    NetWeights *wb = q_only ? nullptr : find_net(c, id_b, qp);            // pmp_infer_q needs the QT net alone
    if (!wq || (!q_only && !wb))
        return set_err(c, PMP_E_NOWEIGHTS, fn + (q_only ? ": the QT net of this (comp, qp) is not loaded" : ": weights for this (comp, qp) are not loaded"));
    if (c->taps_on && (n > c->chunk || n > PMP_TAP_MAX_BLOCKS || c->overlap))
        return set_err(c, PMP_E_INVALID, fn + ": with taps on, one pass of at most 64 blocks (n <= chunk) and overlap mode off");
    int rc = resolve_pending(c, false);          // earlier calls whose snapshot has landed by now: no wait
    if (rc != PMP_OK) return rc;
    if (c->taps_on) c->ntaps = 0;                // the taps are this call's (a re-run resolved above is recorded by nobody)
    const int precision = c->precision;          // the datapath at enqueue: a re-run that did not fire runs on it again
    rc = infer_passes(c, precision, c->taps_on != 0, luma, *wq, wb, by, bu, bv, n, qt, bt, dire, qt_in);
    if (rc != PMP_OK || precision != PMP_PRECISION_F16X3 || c->sat_policy == PMP_SAT_IGNORE || n == 0) return rc;
    // f16x3 range guard: snapshot the flag behind this call's passes and reset it for the next call - all stream-ordered, the host
    // does not wait.  Whoever looks at the snapshot later (resolve_pending) re-runs the call on the fp32 MFMA datapath if it fired.
    if (count_pending_infer(c) >= PMP_SAT_SLOTS && (rc = resolve_pending(c, true)) != PMP_OK) return rc;
    unsigned *slot = c->h_sat + (c->sat_seq++ % PMP_SAT_SLOTS);
    *slot = 0;
    hipError_t e = hipMemcpyAsync(slot, c->d_sat, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_sat, 0, sizeof(unsigned), c->stream);
    hipEvent_t ev = c->event_pool.get();
    if (e == hipSuccess) e = hipEventRecord(ev, c->stream);
    if (e != hipSuccess) { c->event_pool.put(ev); return hip_fail(c, e, "saturation flag snapshot"); }
    c->pending.push_back(PendingCall{true, ctx_logits, ev, slot, [=](bool fired) {
        NetWeights *rq = find_net(c, id_q, qp), *rb = q_only ? nullptr : find_net(c, id_b, qp);   // replacing a net settles first: still the same nets
        if (!rq || (!q_only && !rb)) return set_err(c, PMP_E_NOWEIGHTS, fn + ": weights vanished before the range-guard re-run");
        // fired: the exact fp32 MFMA datapath - fp32's range, a bit-exact fmaf chain, and on the full-size campaign the closest of the
        // three to the oracle (profiles/r03_parity_campaign.txt: 5.5e-4 against bf16x6's 8.9e-4 on the worst block); its speed does not
        // matter for a call that is this rare.  Not fired: the call's logits were in the context's buffers, which an earlier re-run has
        // overwritten - the same call again, on the datapath it ran on.  No taps: pmp_debug_set_taps records the call as it first ran.
        return infer_passes(c, fired ? PMP_PRECISION_F32 : precision, false, luma, *rq, rb, by, bu, bv, n, qt, bt, dire, qt_in);   // teacher-forced: the MTT net only; q_only: the QT net only
    }});
    return PMP_OK;
}

int sync(pmp_ctx *c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "hipStreamSynchronize");
}

// sync() as the LAST thing an entry point does (pmp_synchronize, the host-pointer calls): the context is idle when it returns, so the
// next change of stream has nothing to order (pmp_set_stream).  With the stream everything it was ordered behind has finished: the
// second stream's join, and the streams the context was on before (the entry point made this one wait for their fence: CHECK_CTX).
// A sync() in the MIDDLE of a call - a training call that first settles a pending re-run - is followed by that call's own work, and
// leaves the flag alone.
int sync_idle(pmp_ctx *c)
{
    const int rc = sync(c);
    if (rc != PMP_OK) return rc;
    c->unsettled = false;
    c->fence_stream = nullptr;
    c->fence_due = false;
    return PMP_OK;
}

// Everything this context has been asked to do is done and final: range flags looked at, re-runs finished.
int settle(pmp_ctx *c)
{
    int rc = resolve_pending(c, true);
    return rc != PMP_OK ? rc : sync(c);
}

}  // namespace pmp
