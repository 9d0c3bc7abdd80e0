// api_labels.cpp — the entry points that work on VTM's labels (include/pmp.h): MSBT training labels, the labels' own partition,
// validation statistics, teacher-forced MTT inference and the training losses.
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "pmp_host.h"

using namespace pmp;

// ---- one staged pass loop for the host-pointer entry points below ----------------------------------------------------------
namespace {
struct StagedIn { const void *host; size_t per; DevBuf &buf; };          // per: bytes per block; host null: left out, nothing staged
struct StagedOut { void *host; size_t per; DevBuf &buf; size_t off; };   // starts `off` bytes per block into buf (hor | ver share one); host null: left out
}  // namespace

// n blocks in passes of at most `chunk` through the context's staging buffers, all on c->stream: H2D of every input, launch(blocks of
// the pass, its index), D2H of every per-block output, and a synchronise per pass, because the next pass reuses the staging buffers.
static int staged_passes(pmp_ctx *c, int64_t n, std::initializer_list<StagedIn> ins, std::initializer_list<StagedOut> outs,
                         const std::function<int(int64_t, int64_t)> &launch)
{
    const int64_t chunk = c->chunk, m0 = n < chunk ? n : chunk;
    int rc;
    for (const StagedIn &i : ins)
        if (i.host && (rc = ensure(c, i.buf, (size_t)m0 * i.per))) return rc;
    for (const StagedOut &o : outs) {
        if (!o.host) continue;
        size_t per = 0;                                // of the whole buffer: the outputs that share it lie plane behind plane
        for (const StagedOut &q : outs) if (q.host && &q.buf == &o.buf) per = std::max(per, q.off + q.per);
        if ((rc = ensure(c, o.buf, (size_t)m0 * per))) return rc;
    }
    for (int64_t at = 0, pass = 0; at < n; at += chunk, ++pass) {
        const int64_t m = (n - at) < chunk ? (n - at) : chunk;
        if (c->poison) {          // pmp_debug_poison_workspace: the kernel must write every output byte it hands back
            for (const StagedOut &o : outs) {
                if (!o.host) continue;
                const hipError_t e = hipMemsetAsync((char *)o.buf.p + (size_t)m * o.off, poison_byte(c), (size_t)m * o.per, c->stream);
                if (e != hipSuccess) return hip_fail(c, e, "poison label buffers");
            }
        }
        for (const StagedIn &i : ins)
            if (i.host && (rc = h2d(c, i.buf, (const char *)i.host + (size_t)at * i.per, (size_t)m * i.per))) return rc;
        if ((rc = launch(m, pass))) return rc;
        for (const StagedOut &o : outs)
            if (o.host && (rc = d2h(c, (char *)o.host + (size_t)at * o.per, (const char *)o.buf.p + (size_t)m * o.off, (size_t)m * o.per))) return rc;
        if ((rc = sync(c))) return rc;
    }
    return PMP_OK;
}

// The argument checks that pmp_msbt_labels*, pmp_label_partition* share; fn: the entry point family the message names
static int label_args(pmp_ctx *c, const char *fn, int cf, int64_t n, std::initializer_list<const void *> bufs)
{
    const std::string f(fn);
    if (cf != 1 && cf != 2) return set_err(c, PMP_E_INVALID, f + ": cf must be 1 or 2");
    if (n < 0) return set_err(c, PMP_E_INVALID, f + ": negative count");
    if (n > 0 && std::find(bufs.begin(), bufs.end(), nullptr) != bufs.end()) return set_err(c, PMP_E_INVALID, f + ": null buffer");
    return PMP_OK;
}

static int hip_rc(pmp_ctx *c, hipError_t e, const char *what) { return e == hipSuccess ? PMP_OK : hip_fail(c, e, what); }

static bool misaligned(std::initializer_list<const void *> ps, uintptr_t mask)
{
    uintptr_t bits = 0;
    for (const void *p : ps) bits |= (uintptr_t)p;
    return (bits & mask) != 0;
}

// The host forms of pmp_val_stats, pmp_train_loss and pmp_val_confusion, the whole call as one batch: the six inputs go through c->d_val
// in passes (about 6.9 kB per block), launch(the pass's inputs on the device, its blocks, its row of `rows` T[passes][ncols]) per pass,
// then the rows are copied back and added to sums[ncols] in pass order.  T: double, or int64_t for the counts.
template <class T, class F>
static int staged_logit_sums(pmp_ctx *c, const LogitLabels &h, int64_t n, std::initializer_list<StagedOut> outs, DevBuf &rows, int ncols,
                             T *sums, const F &launch)
{
    const int64_t passes = (n + c->chunk - 1) / c->chunk;
    int rc;
    if ((rc = ensure(c, rows, (size_t)passes * ncols * sizeof(T)))) return rc;
    DevBuf *d = c->d_val;
    rc = staged_passes(c, n, {{h.qt, 64 * 4, d[0]}, {h.bt, 768 * 4, d[1]}, {h.dire, 768 * 4, d[2]}, {h.qt8, 64, d[3]}, {h.msbt, 768, d[4]}, {h.msdire, 768, d[5]}},
                       outs, [&](int64_t m, int64_t pass) {
                           const auto on = [&](const void *host, int i) { return host ? d[i].p : nullptr; };   // left out stays left out
                           return launch(LogitLabels{(const float *)on(h.qt, 0), (const float *)on(h.bt, 1), (const float *)on(h.dire, 2),
                                                     (const uint8_t *)on(h.qt8, 3), (const uint8_t *)on(h.msbt, 4), (const int8_t *)on(h.msdire, 5)},
                                         m, (T *)rows.p + pass * ncols);
                       });
    if (rc != PMP_OK) return rc;
    std::vector<T> r((size_t)passes * ncols);
    if ((rc = d2h(c, r.data(), rows.p, r.size() * sizeof(T))) || (rc = sync_idle(c))) return rc;
    for (int64_t p = 0; p < passes; ++p)
        for (int i = 0; i < ncols; ++i) sums[i] += r[(size_t)p * ncols + i];
    return PMP_OK;
}

extern "C" {

// ---- training labels: GenMSBtMap (labels.hip) --------------------------------------------------------------------------
int pmp_msbt_labels_device(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *msbt,
                           uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = label_args(c, "pmp_msbt_labels", cf, n, {qt, bt, dire, msbt, status}))) return rc;
    if (n == 0) return PMP_OK;
    if (misaligned({qt, bt, dire, msbt}, 3))
        return set_err(c, PMP_E_INVALID, "pmp_msbt_labels_device: qt, bt, dire and msbt must be 4-byte aligned");
    return hip_rc(c, launch_msbt_labels(c->stream, qt, bt, dire, n, cf, msbt, status), "msbt_labels");
}

int pmp_msbt_labels(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *msbt,
                    uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = label_args(c, "pmp_msbt_labels", cf, n, {qt, bt, dire, msbt, status}))) return rc;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    DevBuf *d = c->d_lab;                              // about 1.9 kB per block
    return staged_passes(c, n, {{qt, 64, d[0]}, {bt, 256, d[1]}, {dire, 768, d[2]}}, {{msbt, 768, d[3], 0}, {status, 1, d[4], 0}},
                         [&](int64_t m, int64_t) {
                             return hip_rc(c, launch_msbt_labels(c->stream, (const uint8_t *)d[0].p, (const uint8_t *)d[1].p, (const int8_t *)d[2].p,
                                                                 m, cf, (uint8_t *)d[3].p, (uint8_t *)d[4].p), "msbt_labels");
                         });
}

// ---- the labels' own partition: Map_to_SubMap.get_partition (labels.hip) -------------------------------------------------
int pmp_label_partition_device(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *hor,
                               uint8_t *ver, uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = label_args(c, "pmp_label_partition", cf, n, {qt, bt, dire, hor, ver, status}))) return rc;
    if (n == 0) return PMP_OK;
    if (misaligned({qt, bt, dire, hor, ver}, 3))
        return set_err(c, PMP_E_INVALID, "pmp_label_partition_device: qt, bt, dire, hor and ver must be 4-byte aligned");
    return hip_rc(c, launch_label_partition(c->stream, qt, bt, dire, n, cf, hor, ver, nullptr, status), "label_partition");
}

int pmp_label_partition_records_device(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n,
                                       uint8_t *rec, uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = label_args(c, "pmp_label_partition", cf, n, {qt, bt, dire, rec, status}))) return rc;
    if (n == 0) return PMP_OK;
    if (misaligned({qt, bt, dire, rec}, 3))
        return set_err(c, PMP_E_INVALID, "pmp_label_partition_records_device: qt, bt, dire and rec must be 4-byte aligned");
    return hip_rc(c, launch_label_partition(c->stream, qt, bt, dire, n, cf, nullptr, nullptr, rec, status), "label_partition");
}

int pmp_label_partition(pmp_ctx *c, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *hor,
                        uint8_t *ver, uint8_t *status)
{
    CHECK_CTX(c);
    int rc;
    if ((rc = label_args(c, "pmp_label_partition", cf, n, {qt, bt, dire, hor, ver, status}))) return rc;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    DevBuf *d = c->d_lab;                              // the staging buffers of pmp_msbt_labels; hor and ver share its msbt output
    return staged_passes(c, n, {{qt, 64, d[0]}, {bt, 256, d[1]}, {dire, 768, d[2]}},
                         {{hor, 256, d[3], 0}, {ver, 256, d[3], 256}, {status, 1, d[4], 0}}, [&](int64_t m, int64_t) {
                             uint8_t *d_hor = (uint8_t *)d[3].p, *d_ver = d_hor + (size_t)m * 256;
                             return hip_rc(c, launch_label_partition(c->stream, (const uint8_t *)d[0].p, (const uint8_t *)d[1].p, (const int8_t *)d[2].p,
                                                                     m, cf, d_hor, d_ver, nullptr, (uint8_t *)d[4].p), "label_partition");
                         });
}

// ---- validation statistics, training losses (logitstats.hip) and teacher-forced MTT inference -----------------------------
// Metrics.py:148-151 = Train_QBD.py:35-38 (luma; validation is always luma) and Train_QBD.py:39-42 (chroma, training only); the float64
// entry becomes a float32 scalar when torch adds it to the float32 dl*dl
static const double weight_mat[4][3] = {{0.5 * 1.0, 0.5 * 0.73, 0.5 * 0.15}, {0.5 * 2.43, 0.5 * 0.35, 0.5 * 0.10},
                                        {0.5 * 0.96, 0.5 * 0.23, 0.5 * 0.07}, {0.5 * 0.59, 0.5 * 0.16, 0.5 * 0.05}};
static const double chroma_weight_mat[4][3] = {{0.5 * 17.83, 0.5 * 0.49, 0.5 * 0.11}, {0.5 * 1.20, 0.5 * 0.25, 0.5 * 0.07},
                                               {0.5 * 0.58, 0.5 * 0.17, 0.5 * 0.05}, {0.5 * 0.38, 0.5 * 0.12, 0.5 * 0.04}};

static LogitWeights logit_weights(int comp, int qp)     // qp in 22..41
{
    const double *row = (comp == PMP_LUMA ? weight_mat : chroma_weight_mat)[(qp - 22) / 5];
    return {{(float)row[0], (float)row[1], (float)row[2]}, qp == 22};
}

// The NULL forms that pmp_val_stats* and pmp_train_loss* take; fn: the entry point family the message names
static int logit_label_args(pmp_ctx *c, const char *fn, const LogitLabels &a, int64_t n)
{
    const bool q = a.qt && a.qt8, noq = !a.qt && !a.qt8, m = a.bt && a.dire && a.msbt && a.msdire,
               nom = !a.bt && !a.dire && !a.msbt && !a.msdire;
    if (n > 0 && !((q && m) || (q && nom) || (noq && m)))
        return set_err(c, PMP_E_INVALID, std::string(fn) + ": pass (qt, qt8), (bt, dire, msbt, msdire) or both; no other NULL mix");
    return PMP_OK;
}

namespace {
struct ValArgs {
    LogitLabels in;
    int64_t n;
    LogitWeights w;
    double *stats, *block_stats;       // block_stats null: the context's scratch, looked up at launch (a replay may find it regrown)
};
}  // namespace

static int val_check(pmp_ctx *c, int qp, const void *stats, ValArgs &a)      // fills a.w
{
    if (qp < 22 || qp > 41) return set_err(c, PMP_E_INVALID, "pmp_val_stats: qp must be in 22..41 (rows 0..3 of weight_mat)");
    if (a.n < 0 || !stats) return set_err(c, PMP_E_INVALID, "pmp_val_stats: negative count or null stats");
    const int rc = logit_label_args(c, "pmp_val_stats", a.in, a.n);
    if (rc != PMP_OK) return rc;
    a.w = logit_weights(PMP_LUMA, qp);
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
    return hip_rc(c, launch_val_stats(c->stream, a.in, a.n, a.w, part, a.stats), "val_stats");
}

static int val_device_impl(pmp_ctx *c, const ValArgs &a)
{
    if (a.n == 0) return hip_rc(c, hipMemsetAsync(a.stats, 0, PMP_VAL_NSTATS * sizeof(double), c->stream), "val_stats");
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
    ValArgs a{{qt, bt, dire, qt8, msbt, msdire}, n, {}, stats, block_stats};
    int rc;
    if ((rc = val_check(c, qp, stats, a))) return rc;
    if (n > 0 && (misaligned({bt, dire}, 15) || misaligned({qt, msbt, msdire}, 3) || misaligned({stats, block_stats}, 7)))
        return set_err(c, PMP_E_INVALID, "pmp_val_stats_device: bt, dire must be 16-byte aligned, qt, msbt, msdire 4-byte, the outputs 8-byte");
    return val_device_impl(c, a);
}

int pmp_val_stats(pmp_ctx *c, int qp, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                  const int8_t *msdire, int64_t n, double stats[PMP_VAL_NSTATS])
{
    CHECK_CTX(c);
    ValArgs a{{qt, bt, dire, qt8, msbt, msdire}, n, {}, stats, nullptr};
    int rc;
    if ((rc = val_check(c, qp, stats, a))) return rc;
    for (int i = 0; i < PMP_VAL_NSTATS; ++i) stats[i] = 0.0;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    return staged_logit_sums(c, a.in, n, {}, c->d_valout, PMP_VAL_NSTATS, stats, [&](const LogitLabels &dev, int64_t m, double *row) {
        return val_launch(c, ValArgs{dev, m, a.w, row, nullptr});
    });
}

// ---- confusion counts (logitstats.hip): per map the joint histogram of (label class, predicted class) ---------------------------
namespace {
struct ConfArgs {
    LogitLabels in;
    int64_t n;
    int64_t *counts;
    uint16_t *block_counts;            // null: the context's scratch, looked up at launch (a replay may find it regrown)
};
}  // namespace

// The forms pmp_val_confusion* take: a group is its labels with or without its logits, and at least one group's labels are there
static int conf_check(pmp_ctx *c, const ConfArgs &a)
{
    if (a.n < 0 || !a.counts) return set_err(c, PMP_E_INVALID, "pmp_val_confusion: negative count or null counts");
    if (a.n == 0) return PMP_OK;
    const LogitLabels &i = a.in;
    if ((i.qt && !i.qt8) || ((i.bt || i.dire) && !(i.msbt && i.msdire)))
        return set_err(c, PMP_E_INVALID, "pmp_val_confusion: logits without their labels");
    if (!i.bt != !i.dire || !i.msbt != !i.msdire)
        return set_err(c, PMP_E_INVALID, "pmp_val_confusion: bt goes with dire, msbt with msdire");
    if (!i.qt8 && !i.msbt) return set_err(c, PMP_E_INVALID, "pmp_val_confusion: no labels: pass qt8, (msbt, msdire) or both");
    return PMP_OK;
}

static int conf_launch(pmp_ctx *c, const ConfArgs &a)
{
    uint16_t *part = a.block_counts;
    if (!part) {
        const int rc = ensure(c, c->d_confpart, (size_t)a.n * PMP_CONF_NCOUNTS * sizeof(uint16_t));
        if (rc != PMP_OK) return rc;
        part = (uint16_t *)c->d_confpart.p;
    }
    return hip_rc(c, launch_val_confusion(c->stream, a.in, a.n, part, a.counts), "val_confusion");
}

int pmp_val_confusion_device(pmp_ctx *c, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                             const int8_t *msdire, int64_t n, int64_t *counts, uint16_t *block_counts)
{
    CHECK_CTX(c);
    const ConfArgs a{{qt, bt, dire, qt8, msbt, msdire}, n, counts, block_counts};
    int rc;
    if ((rc = conf_check(c, a))) return rc;
    if (misaligned({counts}, 7) || misaligned({block_counts}, 1) || (n > 0 && (misaligned({bt, dire}, 15) || misaligned({qt, msbt, msdire}, 3))))
        return set_err(c, PMP_E_INVALID, "pmp_val_confusion_device: bt, dire must be 16-byte aligned, qt, msbt, msdire 4-byte, d_counts 8-byte, d_block_counts 2-byte");
    if (n == 0) return hip_rc(c, hipMemsetAsync(counts, 0, PMP_CONF_NCOUNTS * sizeof(int64_t), c->stream), "val_confusion");
    rc = conf_launch(c, a);
    // as a statistics call: behind an inference call whose range flag has not been looked at yet, remembered for the replay
    if (rc == PMP_OK && !c->pending.empty())
        c->pending.push_back(PendingCall{false, false, nullptr, nullptr, [=](bool) { return conf_launch(c, a); }});
    return rc;
}

int pmp_val_confusion(pmp_ctx *c, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                      const int8_t *msdire, int64_t n, int64_t counts[PMP_CONF_NCOUNTS])
{
    CHECK_CTX(c);
    const ConfArgs a{{qt, bt, dire, qt8, msbt, msdire}, n, counts, nullptr};
    int rc;
    if ((rc = conf_check(c, a))) return rc;
    for (int i = 0; i < PMP_CONF_NCOUNTS; ++i) counts[i] = 0;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    return staged_logit_sums(c, a.in, n, {}, c->d_confout, PMP_CONF_NCOUNTS, counts, [&](const LogitLabels &dev, int64_t m, int64_t *row) {
        return conf_launch(c, ConfArgs{dev, m, row, nullptr});
    });
}

namespace {
struct TrainArgs {
    LogitLabels in;
    LogitGrads g;
    pmp_loss_params L;
    LogitWeights w;
};
const pmp_loss_params LOSS_DEFAULT = {1.0, {0.8, 1.0, 1.2}, {1.0, 1.0, 1.0}, {0.5, 0.5, 0.5}};   // Train_QBD.py:448-457

bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}
}  // namespace

// Every check of pmp_train_loss* that does not depend on where the pointers live; fills a.L, a.w.  Nothing is written before it passes.
static int train_check(pmp_ctx *c, int comp, int qp, const pmp_loss_params *p, int64_t n, const void *terms, const void *loss, TrainArgs &a)
{
    if (comp != PMP_LUMA && comp != PMP_CHROMA) return set_err(c, PMP_E_INVALID, "pmp_train_loss: comp must be PMP_LUMA or PMP_CHROMA");
    if (qp < 22 || qp > 41) return set_err(c, PMP_E_INVALID, "pmp_train_loss: qp must be in 22..41 (rows 0..3 of the weight matrices)");
    if (n < 0 || !terms || !loss) return set_err(c, PMP_E_INVALID, "pmp_train_loss: negative count, null terms or null loss");
    a.L = p ? *p : LOSS_DEFAULT;
    const double *lam = &a.L.lambq;
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(lam[i])) return set_err(c, PMP_E_INVALID, "pmp_train_loss: a loss weight is not finite");
    const int rc = logit_label_args(c, "pmp_train_loss", a.in, n);
    if (rc != PMP_OK) return rc;
    if (n > 0) {
        const bool none = !a.g.qt && !a.g.bt && !a.g.dire;
        if (!none && ((a.g.qt != nullptr) != a.in.has_q() || (a.g.bt != nullptr) != a.in.has_m() || (a.g.dire != nullptr) != a.in.has_m()))
            return set_err(c, PMP_E_INVALID, "pmp_train_loss: gradient pointers are all NULL or exactly those of the logits given");
        const struct { const void *p; size_t per; } in[6] = {{a.in.qt, 256}, {a.in.bt, 3072}, {a.in.dire, 3072}, {a.in.qt8, 64}, {a.in.msbt, 768}, {a.in.msdire, 768}},
                                                    g[3] = {{a.g.qt, 256}, {a.g.bt, 3072}, {a.g.dire, 3072}};
        for (const auto &o : g)
            for (const auto &i : in)
                if (overlaps(o.p, (size_t)n * o.per, i.p, (size_t)n * i.per))
                    return set_err(c, PMP_E_INVALID, "pmp_train_loss: a gradient tensor overlaps an input");
    }
    a.w = logit_weights(comp, qp);
    return PMP_OK;
}

// m blocks at the pointers of `a`, gradient divisors of an n_div-block call; block partials in the context's scratch
static int train_launch(pmp_ctx *c, const TrainArgs &a, int64_t m, int64_t n_div, double *terms, double *loss)
{
    const int rc = ensure(c, c->d_trainpart, (size_t)m * PMP_LOSS_NTERMS * sizeof(double));
    if (rc != PMP_OK) return rc;
    return hip_rc(c, launch_train_loss(c->stream, a.in, m, n_div, a.w, a.L, (double *)c->d_trainpart.p, terms, loss, a.g), "train_loss");
}

int pmp_train_loss_device(pmp_ctx *c, int comp, int qp, const pmp_loss_params *p, const float *qt, const float *bt, const float *dire,
                          const uint8_t *qt8, const uint8_t *msbt, const int8_t *msdire, int64_t n, double *terms, double *loss,
                          float *g_qt, float *g_bt, float *g_dire)
{
    CHECK_CTX(c);
    TrainArgs a{{qt, bt, dire, qt8, msbt, msdire}, {g_qt, g_bt, g_dire}, LOSS_DEFAULT, {}};
    int rc;
    if ((rc = train_check(c, comp, qp, p, n, terms, loss, a))) return rc;
    if (misaligned({terms, loss}, 7) || (n > 0 && (misaligned({bt, dire, g_bt, g_dire}, 15) || misaligned({qt, qt8, msbt, msdire, g_qt}, 3))))
        return set_err(c, PMP_E_INVALID, "pmp_train_loss_device: bt, dire, g_bt, g_dire must be 16-byte aligned, the other inputs and g_qt 4-byte, terms and loss 8-byte");
    // never queued for a range-guard replay: whatever is in flight on the context is made final first (nothing, for logits from elsewhere)
    if ((rc = settle_before_host_call(c))) return rc;
    if (n == 0) {
        hipError_t e = hipMemsetAsync(terms, 0, PMP_LOSS_NTERMS * sizeof(double), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(loss, 0, sizeof(double), c->stream);
        return hip_rc(c, e, "train_loss");
    }
    return train_launch(c, a, n, n, terms, loss);
}

int pmp_train_loss(pmp_ctx *c, int comp, int qp, const pmp_loss_params *p, const float *qt, const float *bt, const float *dire,
                   const uint8_t *qt8, const uint8_t *msbt, const int8_t *msdire, int64_t n, double terms[PMP_LOSS_NTERMS], double *loss,
                   float *g_qt, float *g_bt, float *g_dire)
{
    CHECK_CTX(c);
    TrainArgs a{{qt, bt, dire, qt8, msbt, msdire}, {g_qt, g_bt, g_dire}, LOSS_DEFAULT, {}};
    int rc;
    if ((rc = train_check(c, comp, qp, p, n, terms, loss, a))) return rc;
    for (int i = 0; i < PMP_LOSS_NTERMS; ++i) terms[i] = 0.0;
    *loss = 0.0;
    if (n == 0) return PMP_OK;
    if ((rc = settle_before_host_call(c))) return rc;
    DevBuf *g = c->d_train;                            // with gradients, 6.4 kB out per block
    rc = staged_logit_sums(c, a.in, n, {{g_qt, 64 * 4, g[0], 0}, {g_bt, 768 * 4, g[1], 0}, {g_dire, 768 * 4, g[2], 0}}, c->d_trainout,
                           PMP_LOSS_NTERMS, terms, [&](const LogitLabels &dev, int64_t m, double *row) {
                               const LogitGrads dg = {g_qt ? (float *)g[0].p : nullptr, g_bt ? (float *)g[1].p : nullptr,
                                                      g_dire ? (float *)g[2].p : nullptr};
                               return train_launch(c, TrainArgs{dev, dg, a.L, a.w}, m, n, row, nullptr);
                           });
    if (rc != PMP_OK) return rc;
    *loss = train_loss_value(terms, a.L, n);
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
    return sync_idle(c);
}

}  // extern "C"
