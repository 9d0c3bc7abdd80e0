// pmp_api.cpp — the C ABI declared in include/pmp.h: errors, the context's life, settings, weights, and the inference, post-processing
// and block-cutting entry points.  How a call runs and becomes final: range_guard.cpp; labels and validation: api_labels.cpp; the
// measuring and test hooks: api_debug.cpp.
#include <cstdlib>
#include <memory>
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

int ensure(pmp_ctx *c, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return PMP_OK;
    b.reset();
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { b.p = nullptr; return set_err(c, PMP_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    b.cap = bytes;
    return PMP_OK;
}

NetWeights *find_net(pmp_ctx *c, int net_id, int qp)
{
    auto it = c->nets.find(net_id * 100 + qp);
    return (it == c->nets.end() || !it->second.loaded) ? nullptr : &it->second;
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
int ensure_logits(pmp_ctx *c, int64_t n, bool qt_only)
{
    const size_t rest = qt_only ? 0 : (size_t)(n ? n : 1) * 768 * 4;         // pmp_infer_q: no bt and dire buffers, 6 KB a block
    const size_t need[3] = {(size_t)(n ? n : 1) * 64 * 4, rest, rest};
    int rc;
    if ((need[0] > c->d_logit[0].cap || need[1] > c->d_logit[1].cap || need[2] > c->d_logit[2].cap) && !c->pending.empty() &&
        (rc = settle(c)) != PMP_OK)
        return rc;
    for (int i = 0; i < (qt_only ? 1 : 3); ++i) {
        if ((rc = ensure(c, c->d_logit[i], need[i])) != PMP_OK) return rc;
        if (c->poison) {          // pmp_debug_poison_workspace: whoever uses them next must write every byte it later reads
            const hipError_t e = hipMemsetAsync(c->d_logit[i].p, poison_byte(c), need[i], c->stream);
            if (e != hipSuccess) return hip_fail(c, e, "poison logits");
        }
    }
    return PMP_OK;
}

int h2d(pmp_ctx *c, DevBuf &b, const void *src, size_t bytes)
{
    int rc = ensure(c, b, bytes ? bytes : 1);
    if (rc != PMP_OK) return rc;
    if (!bytes) return PMP_OK;
    hipError_t e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "hipMemcpyAsync(H2D)");
}

int d2h(pmp_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!bytes || !dst) return PMP_OK;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "hipMemcpyAsync(D2H)");
}

int stage_blocks(pmp_ctx *c, int comp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n)
{
    int rc;
    if ((rc = h2d(c, c->d_in[0], by, (size_t)n * 68 * 68))) return rc;
    if (comp == PMP_CHROMA) {
        if ((rc = h2d(c, c->d_in[1], bu, (size_t)n * 34 * 34))) return rc;
        if ((rc = h2d(c, c->d_in[2], bv, (size_t)n * 34 * 34))) return rc;
    }
    return PMP_OK;
}

// c->stream waits, on the device, for the fence of the stream the context left with work on it (pmp_set_stream below)
int fence_wait(pmp_ctx *c)
{
    c->fence_due = false;
    const hipError_t e = hipStreamWaitEvent(c->stream, c->fence[c->fence_at], 0);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "ordering the stream behind the one the context was on before");
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
    std::unique_ptr<pmp_ctx> c(new (std::nothrow) pmp_ctx());      // a failure below gives back what exists so far
    if (!c) return set_err(nullptr, PMP_E_NOMEM, "pmp_create: out of host memory");
    c->device = device_id;
    if ((e = hipStreamCreateWithFlags(&c->own_stream.h, hipStreamNonBlocking)) != hipSuccess) return hip_fail(nullptr, e, "hipStreamCreate");
    c->stream = c->own_stream;
    if (const char *ov = std::getenv("PMP_OVERLAP")) c->overlap = ov[0] == '1' && !ov[1];
    if ((e = hipMalloc((void **)&c->d_sat.h, 256)) != hipSuccess || (e = hipMemset(c->d_sat, 0, 256)) != hipSuccess)
        return hip_fail(nullptr, e, "hipMalloc(saturation flag)");
    if ((e = hipHostMalloc((void **)&c->h_sat.h, PMP_SAT_SLOTS * sizeof(unsigned), hipHostMallocDefault)) != hipSuccess)
        return hip_fail(nullptr, e, "hipHostMalloc(saturation snapshots)");
    *out = c.release();
    return PMP_OK;
}

int pmp_destroy(pmp_ctx *c)
{
    if (!c) return PMP_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->fence_due) hipEventSynchronize(c->fence[c->fence_at]);   // work on the stream the context was on before, never waited for since
    if (c->stream2) hipStreamSynchronize(c->stream2);
    drop_pending(c);                                  // their events go back to the pool ...
    ktime_drain(c);                                   // ... and those of the timing scopes
    park_workspace(c->device, c->ws);
    park_workspace(c->device, c->ws2);
    delete c;                                         // everything else goes with its owner (pmp_host.h)
    return PMP_OK;
}

int pmp_trim(void)
{
    trim_parked();
    return PMP_OK;
}

// The context's hidden state - activation workspace, scratch and staging buffers, the logit buffers - is shared by every call, whatever
// stream it ran on, and the caller cannot order what it cannot see.  So a change of stream orders the NEW stream behind everything the
// context has enqueued on the OLD one.  The record happens here, while the old stream is still the caller's to use, and only if an
// entry point has run on it since it became current or was last drained (an idle context records nothing: its old stream may be gone).
// The wait is enqueued on the new stream when the next entry point runs on it (CHECK_CTX), not here: torch_call.run() goes to torch's
// stream and back around every call, and the stream it comes back to is mostly never used - so a training step pays one record per call
// and no wait at all (coming back to the stream of the last record needs none: stream order).  The host never waits.  A fence covers
// the streams before it, because a stream has waited for the previous fence before the context enqueued anything on it.
int pmp_set_stream(pmp_ctx *c, void *hip_stream)
{
    if (!c) return set_err(nullptr, PMP_E_INVALID, "null context");      // not CHECK_CTX: this call runs nothing on either stream
    hipSetDevice(c->device);
    if (!c->pending.empty()) { const int rc = settle(c); if (rc != PMP_OK) return rc; }   // calls in flight belong to the old stream
    const hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream.h;
    if (next == c->stream) return PMP_OK;
    if (c->unsettled) {
        const int k = c->fence_at ^ 1;
        hipError_t e = c->fence[k].h ? hipSuccess : hipEventCreateWithFlags(&c->fence[k].h, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(c->fence[k], c->stream);
        if (e != hipSuccess) return hip_fail(c, e, "pmp_set_stream: fence on the old stream");
        c->fence_at = k;
        c->fence_stream = c->stream;
    }
    c->stream = next;
    c->unsettled = false;
    c->fence_due = c->fence_stream && c->fence_stream != next;
    return PMP_OK;
}

int pmp_synchronize(pmp_ctx *c)
{
    CHECK_CTX(c);
    const int rc = resolve_pending(c, true);
    return rc != PMP_OK ? rc : sync_idle(c);
}

int pmp_set_overlap(pmp_ctx *c, int on)
{
    CHECK_CTX(c);
    if (!c->pending.empty()) { const int rc = settle(c); if (rc != PMP_OK) return rc; }   // calls in flight keep the cut they were made with
    c->overlap = on ? 1 : 0;
    if (!c->overlap) c->ws2.reset();                                                      // the second workspace exists only while the mode is on
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

int pmp_infer_q_device(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n, float *qt)
{
    CHECK_CTX(c);
    return infer_device_impl(c, comp, qp, by, bu, bv, n, qt, nullptr, nullptr, false, nullptr, true);
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

// ---- host-pointer entry points: stage through device buffers owned by the context (stage_blocks, h2d, d2h above) ------
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
    return sync_idle(c);
}

int pmp_infer_q(pmp_ctx *c, int comp, int qp, const uint8_t *by, const uint8_t *bu, const uint8_t *bv, int64_t n, float *qt)
{
    CHECK_CTX(c);
    if (n < 0 || !by || !qt || (comp == PMP_CHROMA && (!bu || !bv)))
        return set_err(c, PMP_E_INVALID, "pmp_infer_q: null buffer or negative count");
    if (n == 0) return PMP_OK;
    int rc;
    if ((rc = settle_before_host_call(c))) return rc;
    if ((rc = stage_blocks(c, comp, by, bu, bv, n))) return rc;
    if ((rc = ensure_logits(c, n, true))) return rc;
    float *dq = (float *)c->d_logit[0].p;
    if ((rc = infer_device_impl(c, comp, qp, (const uint8_t *)c->d_in[0].p, (const uint8_t *)c->d_in[1].p,
                                (const uint8_t *)c->d_in[2].p, n, dq, nullptr, nullptr, true, nullptr, true)))
        return rc;
    if ((rc = resolve_pending(c, true))) return rc;      // range guard: a re-run is enqueued before the copy below
    if ((rc = d2h(c, qt, dq, (size_t)n * 64 * 4))) return rc;
    return sync_idle(c);
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
    return sync_idle(c);
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

static int cut_args(pmp_ctx *c, const void *y, const void *u, const void *v, int F, int H, int W, int bitdepth, const void *by,
                    const void *bu, const void *bv)
{
    if (!y || !u || !v || !by || !bu || !bv || F < 0 || H < 0 || W < 0 || (H & 1) || (W & 1) || (bitdepth != 8 && bitdepth != 10))
        return set_err(c, PMP_E_INVALID, "pmp_cut_blocks: bad arguments (bitdepth 8 or 10, even H/W)");
    return PMP_OK;
}

int pmp_cut_blocks_device(pmp_ctx *c, const void *y, const void *u, const void *v, int F, int H, int W, int bitdepth,
                          uint8_t *by, uint8_t *bu, uint8_t *bv)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = cut_args(c, y, u, v, F, H, W, bitdepth, by, bu, bv))) return rc;
    hipError_t e = launch_cut_blocks(c->stream, y, u, v, F, H, W, bitdepth, by, bu, bv);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "cut_blocks");
}

int pmp_cut_blocks(pmp_ctx *c, const void *y, const void *u, const void *v, int F, int H, int W, int bitdepth, uint8_t *by,
                   uint8_t *bu, uint8_t *bv)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = cut_args(c, y, u, v, F, H, W, bitdepth, by, bu, bv))) return rc;
    const size_t bps = bitdepth == 8 ? 1 : 2, ny = (size_t)F * H * W * bps, nc = (size_t)F * (H / 2) * (W / 2) * bps;
    const int64_t n = (int64_t)F * (H / 64) * (W / 64);
    if (n == 0) return PMP_OK;
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
    return sync_idle(c);
}

}  // extern "C"
