// Host-side internals of libpmp_hip.so: context, packed weights, the four forward graphs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pmp.h"
#include "pmp_hostonly.h"
#include "pmp_kernels.h"

namespace pmp {

enum KClass { K_CONV3_64 = 0, K_CONV5_64, K_CONV_OTHER, K_STEM, K_SMALL, K_POST, K_NCLASS };

struct DevBuf {  // grow-only device buffer, owned: freed with whatever holds it; ensure() is the only place that grows one
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() { if (p) hipFree(p); p = nullptr; cap = 0; }
    void *release() { void *q = p; p = nullptr; cap = 0; return q; }   // the caller frees it
};

// The context's other owned handles: one stream, one allocation of device or pinned words.  Reads like the raw handle it holds.
template <class T, auto Free>
struct Owned {
    T h = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) { reset(); h = o.h; o.h = nullptr; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() { if (h) Free(h); h = nullptr; }
    operator T() const { return h; }
};
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using DevWords = Owned<unsigned *, hipFree>;
using PinnedWords = Owned<unsigned *, hipHostFree>;

// Events that are not in use: taken for a timing scope, a fork / join or a flag snapshot and handed back when that is over
struct EventPool {
    std::vector<hipEvent_t> idle;
    EventPool() = default;
    EventPool(const EventPool &) = delete;
    EventPool &operator=(const EventPool &) = delete;
    ~EventPool() { for (hipEvent_t e : idle) hipEventDestroy(e); }
    hipEvent_t get()
    {
        hipEvent_t e = nullptr;
        if (idle.empty()) hipEventCreate(&e);
        else { e = idle.back(); idle.pop_back(); }
        return e;
    }
    void put(hipEvent_t e) { idle.push_back(e); }
};

// ResidualBlock weights (Model_QBD.py:23-44), packed for the kernel that runs the block.
struct RBWeights {
    int cin = 0, cout = 0, k = 0;      // real dims
    int cin_pad = 0, cout_pad = 0;
    float *w0 = nullptr, *w2 = nullptr, *wsc = nullptr;  // fp32 MFMA packing (or direct packing when `direct`)
    unsigned short *w0x = nullptr, *w2x = nullptr, *wscx = nullptr;  // bf16x6 split packing (conv_bf16x6.hip)
    unsigned short *w0h = nullptr, *w2h = nullptr, *wsch = nullptr;  // f16x3 split packing (conv_f16x3.hip), scaled by
    int k0 = 0, k2 = 0;                                               // 2^k0 (first conv) / 2^k2 (second conv + shortcut)
    AblRB abl;                         // empty in the product library
    bool direct = false;               // 8x8 layers run on the direct kernel
    bool has_sc = false;               // 1x1 shortcut conv (cin != cout); the packed pointers exist per datapath, this flag always
};

struct NetWeights {
    bool loaded = false;
    int net_id = -1;
    unsigned packed = 0;                               // bit p: the formats of datapath p (PMP_PRECISION_*) are on the device
    std::vector<float> host;                           // the caller's fp32 tensors (OIHW), kept for the datapaths packed later
    std::vector<std::string> names;
    std::vector<pmp_tensor_desc> descs;                // offsets into `host`, names into `names`
    std::map<std::string, RBWeights> rb;
    float *stem_w = nullptr, *stem_b = nullptr;        // packed stem convs + 32 biases
    unsigned short *stem_wh = nullptr; int stem_k = 0; // f16x3 MFMA stem: fragment stream, scaled by 2^stem_k
    float *head_w[3] = {nullptr, nullptr, nullptr};    // [9][8][cout]
    float *head_b[3] = {nullptr, nullptr, nullptr};
    // f16x3 ACTIVATION SCALES (MTT nets; include/pmp.h).  The net is bias-free behind its stems and ReLU, max-pool and the gate product are
    // positively homogeneous, so a tensor may travel as true * 2^-e - exactly, a power of two commutes with every rounding - as long as
    // whoever consumes it knows e.  One exponent per SEGMENT of the graph (Model_QBD.py:127-155):
    //   0  stem .. trunk_M1 .. trunk_M2 .. trunk_B1          1  attention trunk 1 (input built from logits)
    //   2  x5 * att0 .. trunk_B2                              3  attention trunk 2                  4  x4 * att1 .. trunk_B3
    // and the changes of scale cost nothing at run time: 2^-e0 is folded into the stem's output scale and biases (stem_b_h), 2^-e1 / 2^-e3
    // into the attention inputs where they are built, the step at a gate product into the out_scale of the convolution whose epilogue
    // multiplies (nets.cpp), the way back into the head weights (head_w_h = head_w * 2^e).  The exponents come from a calibration pass on the library's own extreme-content blocks, run once when
    // the net is first used on the f16x3 datapath (calibrate.cpp: calibrate_mtt); all zero = the arithmetic of a net without scales, bit for bit.
    int act_exp[5] = {0, 0, 0, 0, 0};
    bool calibrated = false;
    uint64_t fp = 0;                                   // fingerprint_tensors() of `host` (pmp_weights_fingerprint)
    bool act_from_file = false;                        // the exponents came from a manifest ...
    bool act_fp_known = false; uint64_t act_qt_fp = 0; // ... that says which QT partner they were calibrated with
    bool act_given = false;                            // pmp_debug_run_resblock: act_exp set by the caller, for a net of one block
    float *stem_b_h = nullptr;                         // f16x3: stem biases * 2^-act_exp[0]
    float *head_w_h[3] = {nullptr, nullptr, nullptr};  // f16x3: head weights * 2^act_exp[{0, 2, 4}]
    std::vector<std::string> cal_names;                // calibration record: tensors in launch order ...
    std::vector<int> cal_seg;                          // ... their segment ...
    std::vector<float> cal_amax;                       // ... and their largest |value| (true scale) on the calibration blocks
    std::vector<void *> allocs;
};

// Activation workspace: a first-fit free-list allocator over one device buffer.  Every forward runs twice - a measuring
// pass (no launches) that replays the graph's alloc/release sequence to find the peak, then the real pass, which makes the
// same calls and therefore gets the same offsets.  All launches of a pass go to one stream in order, so a tensor's
// bytes may be handed out again as soon as its last consumer has been ENQUEUED (Graph::release).
struct Arena {
    char *base = nullptr;
    size_t cap = 0, top = 0, peak = 0;
    bool measuring = false;
    std::vector<std::pair<size_t, size_t>> holes;   // (offset, bytes), sorted by offset, coalesced
    void reset() { top = 0; peak = 0; holes.clear(); }
    size_t take(size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        size_t best = holes.size();
        for (size_t i = 0; i < holes.size(); ++i)      // best fit: the smallest hole that is large enough
            if (holes[i].second >= bytes && (best == holes.size() || holes[i].second < holes[best].second)) best = i;
        size_t off;
        if (best != holes.size()) {
            off = holes[best].first;
            if (holes[best].second == bytes) holes.erase(holes.begin() + best);
            else { holes[best].first += bytes; holes[best].second -= bytes; }
        } else {
            off = top;
            top += bytes;
            if (top > peak) peak = top;
        }
        return off;
    }
    void give(size_t off, size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        size_t i = 0;
        while (i < holes.size() && holes[i].first < off) ++i;
        holes.insert(holes.begin() + i, std::make_pair(off, bytes));
        if (i + 1 < holes.size() && holes[i].first + holes[i].second == holes[i + 1].first) { holes[i].second += holes[i + 1].second; holes.erase(holes.begin() + i + 1); }
        if (i > 0 && holes[i - 1].first + holes[i - 1].second == holes[i].first) { holes[i - 1].second += holes[i].second; holes.erase(holes.begin() + i); }
        if (!holes.empty() && holes.back().first + holes.back().second == top) { top = holes.back().first; holes.pop_back(); }
    }
    float *ptr(size_t off) const { return measuring ? nullptr : reinterpret_cast<float *>(base + off); }
};

// What one forward pass runs on and how: built on the stack by whoever starts the pass (infer_passes, calibrate_mtt,
// pmp_debug_run_resblock) and handed down to the graph, which reads its environment here and never from the context.
struct Pass {
    hipStream_t stream;                // every launch of the pass
    DevBuf &ws;                        // its activation workspace: c->ws, c->ws2 (odd chunks in overlap mode) or c->ws_cal
    int precision;                     // datapath, PMP_PRECISION_*
    bool taps;                         // pmp_debug_set_taps: record every tensor (a call's first run only: no re-run, no calibration)
    bool cal;                          // calibration of an MTT net: fold every tensor's largest |value| into c->d_cal
    bool caller;                       // a pass of the caller's own calls: its peak counts in c->ws_need
    Arena arena;                       // host bookkeeping of one graph run (run_graph)
};

struct KTimeRec { hipEvent_t a, b; double flops; };

// pmp_debug_set_taps: a stream-ordered copy of one tensor as the consuming kernel reads it (raw planes, blocked layout)
struct TapRec {
    std::string name;                  // "q/<tensor>" or "bd/<tensor>"
    DevBuf buf;                        // tap-owned device memory
    int n = 0, C = 0, H = 0, W = 0;    // C padded to 16; layout [n][C/16][H][W][16] per plane
    int c_real = 0;
    int fmt = 0;                       // 0 fp32, 1 split-3 (three bf16 planes), 2 split-2 (two fp16 planes)
    int exp = 0;                       // the stored value times 2^exp is the true value (f16x3 activation scales)
};

// f16x3 range guard, deferred (include/pmp.h): every inference call snapshots the device flag into a pinned host word behind its
// passes and records an event; the word is read when the event has completed - at a later call (polled), at pmp_synchronize /
// pmp_get_saturation or at the end of a host-pointer call (waited for).  A call whose flag fired is run again on the fp32 MFMA
// datapath and every post-processing call enqueued after it is replayed, in order, on the same buffers; later inference calls whose
// logits live in the context's own buffers (which the re-run has overwritten) run again too.
struct PendingCall {
    bool infer;                       // inference (has a flag snapshot) or a post-processing call recorded for replay
    bool ctx_logits;                  // infer: its logits are in c->d_logit, shared by every call that passes no logit pointers
    hipEvent_t ev;                    // infer: completes when the snapshot has landed
    unsigned *slot;                   // infer: pinned host word
    std::function<int(bool)> rerun;   // infer: the same call, on fp32 MFMA if its flag fired;  post: the same call again
};

}  // namespace pmp

namespace pmp {
void free_net_weights(NetWeights &w);   // weights_pack.cpp
constexpr int PMP_SAT_SLOTS = 64;             // flag snapshots in flight (pmp_ctx::h_sat)
constexpr int PMP_TAP_MAX_BLOCKS = 64;        // pmp_debug_set_taps: tap memory is one copy of every tensor of the call
}  // namespace pmp

// Every device resource below is owned by its member (DevBuf, Owned, EventPool) and goes with the context: nothing is freed by name.
// Members die in reverse order of declaration, so the streams, declared first, outlive every buffer and event.  That order only has to
// be valid, not careful: pmp_destroy has synchronised the streams and drained the events before it deletes the context.
struct pmp_ctx {
    ~pmp_ctx() { for (auto &kv : nets) pmp::free_net_weights(kv.second); }   // NetWeights keeps its own list of allocations
    int device = 0;
    pmp::OwnedStream own_stream;
    pmp::OwnedStream stream2;              // overlap mode: the passes of odd chunks; created on first use
    pmp::OwnedStream cal_stream;           // calibration runs on its own stream and workspace: it neither waits for the passes in flight on the
                                           // context's stream nor touches their workspace (created on first use)
    hipStream_t stream = nullptr;          // the caller's (pmp_set_stream) or own_stream; a pass runs on its Pass::stream
    // pmp_set_stream with work in flight (include/pmp.h): leaving a stream the context has used since it became current or was last
    // drained records a fence on it; the stream the context arrives on waits for the last fence before the next entry point's work
    bool unsettled = false;                // an entry point has run on `stream` since then (CHECK_CTX sets it, sync_idle() clears it)
    pmp::OwnedEvent fence[2];              // used in turn, created on first use without timing; [fence_at] holds the last record
    int fence_at = 0;
    hipStream_t fence_stream = nullptr;    // the stream of the last record; null: nothing outstanding
    bool fence_due = false;                // `stream` has yet to be made to wait for it (CHECK_CTX does, before anything is enqueued)
    int chunk = 4096;   // blocks per pass: the 16x16-resolution layers need >= 4096 tiles to fill 256 CUs x 3 workgroups evenly (+2.5 % over 1024)
    int precision = 2;                     // 0: fp32 MFMA, 1: bf16x6 split, 2: f16x3 split (default; both splits fp32-equivalent) - the caller's setting; a pass runs on its Pass::precision
    int fuse16 = 1;                        // f16x3: run the 16x16-resolution tails LDS-resident (chain16.hip: two / three launches per net); 0 = launch per layer (pmp_debug_set_fusion: A/B and the bit-identity tests)
    int act_scales = 1;                    // f16x3: use the MTT nets' calibrated activation scales (NetWeights::act_exp); 0 = exponents of zero (pmp_debug_set_activation_scales: the range-guard tests)
    int fuse32 = 1;                        // f16x3: trunk_B3.1 / B3.2 / Att2.0 (32x32, <= 32 output channels) as one launch per ResidualBlock (rbfuse32.hip); same hook
    pmp::M2PParams m2p[2] = {pmp::M2P_DEFAULT, pmp::M2P_DEFAULT};   // Map2Partition thresholds per component (pmp_set_partition_params); read at enqueue
    std::string err;
    // f16x3 range guard (include/pmp.h, pmp_set_saturation_policy): device word raised by every kernel that clamps a stored activation.
    // A 256-byte block: word 0 is the flag, bytes 64.. stay zero (the zero line of conv_f16x3_t32.hip's halo DMA)
    pmp::DevWords d_sat;
    pmp::PinnedWords h_sat;                // PMP_SAT_SLOTS pinned host words: flag snapshots of the calls still in flight
    uint64_t sat_seq = 0;
    std::deque<pmp::PendingCall> pending;  // calls whose flag has not been looked at yet (+ the post-processing calls after them)
    pmp::AblCtx abl;                       // empty in the product library
    int sat_policy = PMP_SAT_RERUN;
    int sat_seen = 0;                      // sticky: some inference call since pmp_clear_saturation saturated
    int64_t sat_reruns = 0;                // calls re-run on the fp32 MFMA datapath
    std::map<int, pmp::NetWeights> nets;  // key = net_id * 100 + qp
    pmp::DevBuf ws;                        // activation workspace (its own, or a larger one parked by a destroyed context)
    pmp::DevBuf ws2;                       // second workspace: the passes of odd chunks on `stream2` (overlap mode)
    int overlap = 0;                       // two chunks in flight on two streams (PMP_OVERLAP=1 in the environment at pmp_create)
    size_t ws_need = 0;                    // what the caller's largest pass so far needed of ws / ws2 (pmp_get_workspace_bytes)
    pmp::DevBuf d_in[3], d_logit[3], d_out[4], d_frames[3];  // staging for the host-pointer entry points
    pmp::DevBuf d_lab[5];                  // staging of pmp_msbt_labels: qt, bt, dire in; msbt, status out (pmp_label_partition: hor | ver in msbt's)
    pmp::DevBuf d_val[6];                  // staging of pmp_val_stats: qt, bt, dire, qt8, msbt, msdire
    pmp::DevBuf d_valpart;                 // validation statistics: per-block partials f64[n][20] of a call that passes no d_block_stats
    pmp::DevBuf d_valout;                  // pmp_val_stats: f64[passes][20]
    pmp::DevBuf d_confpart;                // confusion counts: per-block rows u16[n][175] of a call that passes no d_block_counts
    pmp::DevBuf d_confout;                 // pmp_val_confusion: i64[passes][175]
    pmp::DevBuf d_train[3];                // staging of pmp_train_loss's gradients: g_qt, g_bt, g_dire (its inputs go through d_val)
    pmp::DevBuf d_trainpart;               // training losses: per-block partials f64[n][13]
    pmp::DevBuf d_trainout;                // pmp_train_loss: f64[passes][13]
    pmp::DevBuf d_select;                  // pmp_select_rows_device: tile counts and segment tables (dataset.hip)
    pmp::DevBuf d_rb[11];                 // staging of pmp_resblock_forward / _backward: the inputs in RbCall's order (train_check.h), then the outputs
    // calibration of the f16x3 activation scales (NetWeights::act_exp): in a Pass with `cal`, the graph (nets.cpp, running on the fp32
    // datapath) folds the largest |value| of every tensor it produces into d_cal[slot] and logs (name, segment) per slot
    pmp::DevWords d_cal;                   // PMP_CAL_SLOTS device words
    std::vector<std::pair<std::string, int>> cal_log;
    pmp::DevBuf d_calbuf;                  // calibration blocks and their logits
    pmp::DevBuf ws_cal;                    // the workspace of the passes on cal_stream (created on first use; 44 MB for 16-block fp32 passes)
    // test hooks (include/pmp.h): tensor taps and workspace poisoning
    int taps_on = 0;
    std::vector<pmp::TapRec> taps;         // slots, reused call after call; the first ntaps hold the last inference call's tensors in launch order
    int ntaps = 0;
    int poison = 0;                        // 0 off, 1 0xFF bytes, 2 0x3C bytes into every activation workspace before each pass
    // kernel-class timing
    uint32_t kmask = 0;
    std::vector<pmp::KTimeRec> krec[pmp::K_NCLASS];
    pmp::EventPool event_pool;
    int64_t klaunch[pmp::K_NCLASS] = {0};
    double kms[pmp::K_NCLASS] = {0}, kflops[pmp::K_NCLASS] = {0};
};

namespace pmp {

int set_err(pmp_ctx *c, int code, const std::string &msg);
int hip_fail(pmp_ctx *c, hipError_t e, const char *what);

// weights_pack.cpp
int load_net_weights(pmp_ctx *c, int net_id, int qp, const float *blob, const pmp_tensor_desc *descs, int ndesc);
int ensure_datapath(pmp_ctx *c, NetWeights &w, int precision);   // packs the formats of `precision` if the net does not hold them yet
// f16x3 activation scales: stores exps in w.act_exp and (re)builds the scaled stem biases and head weights on the device
int set_activation_scales(pmp_ctx *c, NetWeights &w, const int exps[5]);
constexpr int PMP_CAL_SLOTS = 128;

// internals shared by the translation units of the C ABI (pmp_api.cpp, range_guard.cpp, api_labels.cpp, api_train.cpp, api_debug.cpp) and calibrate.cpp
// pmp_api.cpp
int ensure(pmp_ctx *c, DevBuf &b, size_t bytes);                    // grow-only device buffer
int fence_wait(pmp_ctx *c);                                         // c->stream waits, on the device, for the fence of the stream the context left
NetWeights *find_net(pmp_ctx *c, int net_id, int qp);               // loaded weights of (net, qp) or nullptr
int ensure_logits(pmp_ctx *c, int64_t n, bool qt_only = false);     // the context's own logit buffers (qt_only: the first alone), settled before one is regrown
int stage_blocks(pmp_ctx *c, int comp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n);   // host blocks -> c->d_in
int h2d(pmp_ctx *c, DevBuf &b, const void *src, size_t bytes);      // ensure + copy on c->stream
int d2h(pmp_ctx *c, void *dst, const void *src, size_t bytes);      // copy on c->stream; nothing for a null dst
inline int poison_byte(const pmp_ctx *c) { return c->poison == 1 ? 0xFF : 0x3C; }   // pmp_debug_poison_workspace: NaN bytes or finite garbage
// range_guard.cpp
int run_graph(pmp_ctx *c, Pass &ps, const std::function<int()> &fwd);   // a forward graph twice: measuring pass, then the real one in ps.ws
int infer_device_impl(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n, float *qt,
                      float *bt, float *dire, bool ctx_logits = false, const float *qt_in = nullptr, bool q_only = false);
int resolve_pending(pmp_ctx *c, bool wait);                         // looks at the flag snapshots in flight: re-runs and replays
void drop_pending(pmp_ctx *c);
int sat_fetch(pmp_ctx *c, unsigned *out);                           // reads and clears the device flag word (synchronises)
int sync(pmp_ctx *c);                                               // hipStreamSynchronize(c->stream)
int sync_idle(pmp_ctx *c);                                          // ... as the last thing an entry point does: the context is idle afterwards
int settle(pmp_ctx *c);                                             // everything asked of the context so far is done and final
// Host-pointer entry points stage through the context's own buffers (d_in, d_logit, d_out) and return final results.  A *_device call
// that is still in flight may re-run into those very buffers once its range flag is looked at (and a replayed post-processing call may
// read them), so everything pending is made final BEFORE the host call stages anything: afterwards the queue holds this call only.
inline int settle_before_host_call(pmp_ctx *c) { return c->pending.empty() ? PMP_OK : settle(c); }
void park_workspace(int device, DevBuf &b);                         // pmp_destroy: hands a workspace to the next context on the device
void trim_parked();                                                 // pmp_trim
// api_debug.cpp
void ktime_drain(pmp_ctx *c);                                       // folds the finished timing scopes into the class totals
// pmp_debug_set_taps: copies a tensor just produced on `stream` into tap-owned memory (stream-ordered, before anything can overwrite it)
int tap_record(pmp_ctx *c, hipStream_t stream, const std::string &name, const void *p, int n, int C, int H, int W, int c_real, int fmt, int exp);

// calibrate.cpp
int calibrate_mtt(pmp_ctx *c, bool luma, NetWeights &wq, NetWeights &wb);
void qt_partner_changed(pmp_ctx *c, int qt_net_id, int qp);         // a QT net was (re)loaded: its MTT partner's exponents may be stale
int calibrate_if_ready(pmp_ctx *c, int net_id, int qp);             // a (QT, MTT) pair that has just become complete, on the f16x3 datapath

// pmp_debug_run_resblock: one ResidualBlock "rb" packed by the loader's own load_rb into nw (the formats of `mask`); free_net_weights frees it
int load_single_rb(pmp_ctx *c, NetWeights &nw, int cin, int cout, int k, const float *w0, const float *w2, const float *wsc, unsigned mask);
// ... and run through the graph's rb() on n blocks; x, gate: blocked fp32 [n][C/16][h][w][16] at stored scale (host), gate may be null
int run_resblock(pmp_ctx *c, Pass &ps, const NetWeights &w, int n, int h, int wd, const float *x, const float *gate, bool pool, bool out_f32);

// nets.cpp: forward graphs on device pointers (n <= chunk); all launches go to ps.stream.
int forward_q(pmp_ctx *c, Pass &ps, bool luma, const NetWeights &w, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
              int n, float *qt);
int forward_msbd(pmp_ctx *c, Pass &ps, bool luma, const NetWeights &w, const uint8_t *by, const uint8_t *bu, const uint8_t *bv,
                 const float *qt, int n, float *bt, float *dire);

// timing hooks used by nets.cpp (api_debug.cpp)
struct KScope {
    pmp_ctx *c; hipStream_t stream; int cls; bool on; hipEvent_t a, b; double flops;
    KScope(pmp_ctx *c, hipStream_t stream, int cls, double flops);
    ~KScope();
};

}  // namespace pmp

#define CHECK_CTX(c) do { if (!(c)) return pmp::set_err(nullptr, PMP_E_INVALID, "null context"); hipSetDevice((c)->device); if ((c)->fence_due) { const int rc_ = pmp::fence_wait(c); if (rc_ != PMP_OK) return rc_; } (c)->unsettled = true; } while (0)

#include "abl_hooks.h"   // hooks/ in the product build (no-op inlines), abl/ in the measurement library
