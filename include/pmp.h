/*
 * pmp.h — C ABI of libpmp_hip.so: the MI355X (gfx950) partition-map prediction path.
 *
 * The reference (AolinFeng/PMP-VVC-TIP2023) has no FFI; its hot path is plain Python.  This ABI replaces the
 * two function seams of that path and the helpers either side of them:
 *
 *   pmp_infer*              <- Metrics.py:387-419   inference_pre_QBD  (Net_Q + Net_BD forward, head regrouping)
 *                              Model_QBD.py:59-253  the four Down-Up-CNN nets
 *                              Inference_QBD.py:194-200 driver tensor prep (chroma = maxpool2(Y) ++ U ++ V)
 *   pmp_infer_q*            <- Metrics.py:198-212   pre_validation predID 0: Net_Q alone
 *   pmp_postprocess*        <- Metrics.py:764-774   seq_post_process   = eli_structual_error (Metrics.py:612-637)
 *                              + Map2Partition.py:98-373 Map_to_Partition (per-block search)
 *   pmp_infer_postprocess*  <- both, device-resident (no logits round trip): the throughput path
 *   pmp_cut_blocks*         <- Inference_QBD.py:104-149 output_block_yuv (+ :106-109 10-bit -> 8-bit)
 *   pmp_write_partition_file<- Map2Partition.py:385-412 frame tiling + text emission, parsed by
 *                              EncAppCfg::parsePartitionMatrix (codec/.../App/EncoderApp/EncAppCfg.cpp:4234-4404)
 *   pmp_load_weights        <- Inference_QBD.py:28-46 load_pretrain_model (state_dict tensors by name)
 *
 * Conventions
 *   - Every call returns 0 (PMP_OK) or a negative error class; pmp_last_error() gives the message.  Nothing
 *     aborts or throws across the ABI; HIP errors are mapped to PMP_E_HIP.
 *   - One context per GPU (several per GPU work too).  A context is not thread-safe: one host thread at a time per context.  Different
 *     contexts are independent and may be driven from different host threads CONCURRENTLY - everything a call touches hangs off its
 *     context (streams, workspaces, weights, calibration stream and workspace, range-guard queue, error string); the only
 *     process-wide state is the pool of parked workspaces behind pmp_destroy / pmp_trim (mutex-protected) and the calling thread's
 *     context-less error string (thread-local).  tests/test_gpu_threads.py: two contexts on two threads = the serial results, bit
 *     for bit.  (pmp_debug_set_conv_variant has no state in this library; in the measurement library it is process-wide.)
 *   - There is NO CPU fallback: every compute entry point needs a context on a gfx950 device.
 *   - "block" = one 64x64 luma region with its 4-pixel top/left context: u8[68][68] luma, u8[34][34] per chroma
 *     plane (Inference_QBD.py:190-191).  One VTM CTU (128x128) = 4 blocks.
 *   - Layouts (all dense, row-major):  qt f32[n][8][8]; bt, dire f32[n][3][16][16] (layer-major, as
 *     Metrics.py:399-402 regroups the heads); hor, ver u8[n][16][16]; qt_u8 u8[n][8][8]; dire_i8 i8[n][3][16][16].
 *   - *_device variants take device pointers and run asynchronously on the context's stream
 *     (pmp_set_stream lets the caller supply it); the others take host pointers and synchronise.  pmp_synchronize makes the
 *     outputs of every *_device call made so far final (see the range guard below).
 */
#ifndef PMP_H
#define PMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMP_OK 0
#define PMP_E_INVALID (-1)   /* bad argument / unknown net / shape mismatch */
#define PMP_E_HIP (-2)       /* HIP runtime error (message has hipGetErrorString) */
#define PMP_E_NOWEIGHTS (-3) /* weights for (comp, qp) not loaded */
#define PMP_E_IO (-4)        /* file could not be written */
#define PMP_E_NOMEM (-5)     /* device or host allocation failed */
#define PMP_E_NODEVICE (-6)  /* no gfx950 device: there is no CPU fallback */
#define PMP_E_RANGE (-7)     /* f16x3 datapath: an activation left the fp16 range and the policy is PMP_SAT_ERROR */

enum { PMP_LUMA = 0, PMP_CHROMA = 1 };
enum { PMP_NET_LUMA_Q = 0, PMP_NET_LUMA_MSBD = 1, PMP_NET_CHROMA_Q = 2, PMP_NET_CHROMA_MSBD = 3 };

typedef struct pmp_ctx pmp_ctx;

/* One state_dict entry (name without the DataParallel "module." prefix, Inference_QBD.py:23-25). */
typedef struct {
    const char *name;  /* e.g. "resblock_q1.left.0.weight" */
    int ndim;          /* 4 (OIHW conv weight) or 1 (bias) */
    int shape[4];
    int64_t offset;    /* in floats, into the blob */
} pmp_tensor_desc;

const char *pmp_version(void);

/* pmp_last_error(NULL) returns the calling thread's last context-less error (e.g. from pmp_create). */
const char *pmp_last_error(const pmp_ctx *ctx);

int pmp_create(int device_id, pmp_ctx **out);
int pmp_destroy(pmp_ctx *ctx);

/* pmp_destroy parks the context's activation workspace (up to 10 GB) for the next context created on the same device instead of
 * freeing it: a large hipMalloc right after a hipFree of that size stalls for 0.5-1.4 s now and then on MI355X (the freed memory is
 * still being cleared).  Up to two parked buffers per device (a context in overlap mode owns two workspaces); pmp_trim() returns parked memory to the driver - a host that destroys its
 * context to hand the VRAM to another library calls it right after pmp_destroy (or runs with PMP_PARK_WORKSPACE=0 in the
 * environment: nothing is parked then).  pmp_trim leaves the calling thread's current device as it is. */
int pmp_trim(void);

/* Use the caller's hipStream_t (e.g. torch's current stream); NULL restores the context's own stream.
 *
 * Who orders what across a change of stream.  Every call of a context, whatever stream it runs on, works in memory the caller never
 * sees: the activation workspace, the scratch of the loss, statistics and gradient kernels, the staging and logit buffers of the
 * host-pointer forms.  THE LIBRARY orders that memory: when the stream changes and a call has run on the old stream since it became
 * the context's or was last drained (by pmp_synchronize, or by a host-pointer call that ends with its wait), pmp_set_stream records an event on
 * the old stream, and the context's next call makes the stream it runs on wait for that event, on the device, before it enqueues
 * anything (no wait where that is the stream of the record itself).  Everything the context enqueues after the change therefore
 * starts behind everything it enqueued before; the host does not wait, and no call synchronises because of it.  The old stream must
 * still be the caller's to use when pmp_set_stream is called (an idle context records nothing: the old stream may be destroyed after
 * pmp_synchronize), and pmp_destroy waits for an old stream's work that nothing has waited for since.
 * THE CALLER orders its own tensors, as with any stream: an input written on stream A and read by a call on stream B, an output read
 * on another stream than the one its call ran on, need the caller's own event or synchronisation - except that calls of ONE context
 * are ordered among themselves by the rule above, so one call's output may feed the context's next call on any stream.
 *
 * pmp_synchronize waits for the context's CURRENT stream and resolves the range guard; it first makes that stream wait for the event
 * of the stream before it, as every call does, so it makes the outputs of every *_device call made so far final, on whichever stream
 * each was enqueued. */
int pmp_set_stream(pmp_ctx *ctx, void *hip_stream);
int pmp_synchronize(pmp_ctx *ctx);

/* Blocks processed per pass; n > chunk is looped.  1..4096 (32-bit element offsets inside one activation tensor), default
 * 4096.  The activation workspace is sized for the blocks a pass actually runs, min(n, chunk), and tensors share memory once
 * their last consumer is enqueued: 2.5 MB per luma block on the default datapath (10 GB for a full 4096-block pass, 10 MB
 * for a 4-block call; bf16x6 3.75 MB, chroma 1.1 MB per block); it only grows, to what the largest pass so far needed.
 * pmp_get_workspace_bytes reports that need (the buffer behind it may be a larger one taken over from a destroyed context, see pmp_trim),
 * plus the second workspace overlap mode holds while it is on (sized for its half-call chunks; freed by pmp_set_overlap(ctx, 0)). */
int pmp_set_chunk(pmp_ctx *ctx, int blocks);
int64_t pmp_get_workspace_bytes(const pmp_ctx *ctx);

/* Overlap mode (off by default; PMP_OVERLAP=1 in the environment turns it on at pmp_create).  A call of at least 1024 blocks is cut into
 * (at least) two chunks; even chunks run on the context's stream and workspace, odd ones on a second, internal stream with a second
 * workspace, forked from and joined to the context's stream by events - one chunk's small launches (stems, 16x16 tails, HBM-bound 32x32
 * layers) then run beside the other's 64x64 convolutions.  Blocks are independent, so results do not depend on how a call is cut (bit-
 * identical records; tests/test_gpu_parity.py).  Measured -0.2 ... -1.2 % (luma) / -0.7 ... -1.7 % (chroma) on the 4096-block step.  Two launches share
 * the device then, so the per-launch durations of pmp_ktime_* (and of a profiler) no longer describe a kernel running alone: bench.py
 * keeps the mode off for its timed region and reports its effect beside it.  At JOB level (the CLI driver on 8 x 4K frames, all eight
 * files) the mode bought nothing - 1.702 s on, 1.701 s off (profiles/r05e_driver_bench.txt): the driver's pipeline already hides the
 * small launches' gaps - so the driver leaves it off too (its --overlap turns it on; round 5 had it on by default). */
int pmp_set_overlap(pmp_ctx *ctx, int on);

/* Convolution datapath.  All three are fp32-accurate (EXPERIMENTS.md, precision study); results differ in the last bits only.
 *   PMP_PRECISION_F32    v_mfma_f32_16x16x4_f32, exact fp32 fmaf chain
 *   PMP_PRECISION_BF16X6 every fp32 operand carried as 3 bf16 terms, 6 bf16 MFMA products, fp32 accumulate
 *   PMP_PRECISION_F16X3  (default) every fp32 operand carried as 2 fp16 terms (weights pre-scaled by a power of two),
 *                        3 fp16 MFMA products, fp32 accumulate; activations beyond +-65504 would saturate: guarded, see below */
#define PMP_PRECISION_F32 0
#define PMP_PRECISION_BF16X6 1
#define PMP_PRECISION_F16X3 2
int pmp_set_precision(pmp_ctx *ctx, int mode);
int pmp_get_precision(const pmp_ctx *ctx);

/* Range guard of the f16x3 datapath.  Its activations travel as two fp16 terms, so a value beyond +-65504 is clamped when it
 * is stored (the reference's nets stay below 3e3 on 8-bit content with the trained QT weights; trained MTT weights are not
 * in the reference checkout).  Every kernel that stores such a tensor raises a per-context device flag when the clamp fires
 * (a NaN raises it too), and never otherwise; it compares the value as stored, true x 2^-e of its segment.  Evidence:
 * tests/test_gpu_range_sites.py over-drives one tensor at a time, fused and unfused, by the weight gains of oracle/range_cases.py.
 * Every pmp_infer* call snapshots the flag behind its passes - stream-ordered, into pinned host memory - and the snapshot is
 * LOOKED AT LATER, so that the *_device entry points never stall the host: by the next call of the context
 * (polled: only snapshots that have landed), and by pmp_synchronize / pmp_get_saturation / any host-pointer call (waited for).
 *   PMP_SAT_RERUN (default)  a call whose flag fired is run AGAIN on the exact fp32 MFMA datapath (fp32 range and arithmetic) into
 *                            the same output buffers, and every post-processing call that was enqueued after it is replayed in
 *                            order (a later call whose logits are in the context's own buffers - no logit pointers passed - runs again too).
 *                            Consequence for *_device callers: outputs are FINAL once pmp_synchronize (or
 *                            pmp_get_saturation) has returned - synchronising the stream yourself is enough only if you also
 *                            know the flag stayed down; inputs and outputs must stay untouched until then.  Host-pointer entry
 *                            points return final results, as before.
 *   PMP_SAT_ERROR            the call that looks at a fired snapshot returns PMP_E_RANGE (for *_device calls that may be the
 *                            NEXT call or pmp_synchronize) and forgets the calls in flight; nothing is re-run
 *   PMP_SAT_IGNORE           no snapshots, no re-runs; the caller polls
 * pmp_get_saturation settles the calls in flight and returns 1 if any inference call of this context saturated since the last
 * pmp_clear_saturation (0 otherwise, negative on error); pmp_get_saturation_reruns counts the calls that were re-run. */
/* Activation scales of the f16x3 datapath (MTT nets).  The range guard above is a safety net; what keeps a net with large activations
 * ON the default datapath is this: the MTT nets are bias-free behind their stems, and ReLU, max-pool and the two gate products
 * (Model_QBD.py:143,150) are positively homogeneous, so a tensor can travel as true * 2^-e - exactly: a power of two commutes with
 * every rounding - if its consumer knows e.  The graph has five segments (stem..trunk_M1..trunk_M2..trunk_B1 | attention 1 | x5*att0..
 * trunk_B2 | attention 2 | x4*att1..trunk_B3) with one exponent each; the changes of scale are folded into numbers the kernels multiply
 * by anyway (the stem's output scale and biases, the out_scale of the convolution whose epilogue applies a gate, the head weights), so
 * they cost nothing per call.  The exponents are chosen when a (QT, MTT) pair is first used on the f16x3 datapath: one pass of both nets
 * over 32 built-in calibration blocks (flat, checkerboards, stripes, edges, white noise, smooth random content) on the fp32 MFMA
 * datapath records the largest |value| of every MTT tensor, and a segment whose maximum exceeds 2^12 gets the exponent that brings it
 * there (16x headroom below 65504 for content harsher than the calibration set; the attention trunks take theirs where their input is
 * built from the logits, capped at 2^-6: that input is O(1) and must stay out of fp16's subnormals - an attention trunk that needs more
 * falls to the range guard).
 * Deterministic: same weights, same exponents, on every context and rank.  Exponents of zero - the synthetic uniform MTT weights, any
 * net whose activations stay below 4096 - leave the arithmetic exactly as it was.
 * WHEN: as soon as both nets of a (component, QP) are loaded while the context is on the f16x3 datapath - inside the pmp_load_weights*
 * call that completes the pair (≈ 20 ms of host time; the pass runs on a private stream and a private 44 MB workspace, beside whatever the
 * context's stream is doing) - or, for a pair loaded under another datapath, at its first f16x3 inference call.  NOT AT ALL for an MTT
 * file whose .pmpw manifest carries "act_exp": [e0..e4] (tools/calibrate_pmpw.py writes them once per model directory): those exponents
 * are taken as they are - bounded by the reader (0..30 for the trunk segments, 0..6 for the attention segments: PMP_E_INVALID beyond), and
 * only if the manifest's "act_fp" fingerprints match the tensors of the file and of the QT partner that is (or later gets) loaded; a stale
 * manifest falls back to the calibration pass, and (re)loading a QT net drops exponents that were derived with another one.
 * pmp_debug_activation_report (below) returns the exponents and the recorded maxima. */
#define PMP_SAT_RERUN 0
#define PMP_SAT_ERROR 1
#define PMP_SAT_IGNORE 2
int pmp_set_saturation_policy(pmp_ctx *ctx, int policy);
int pmp_get_saturation(pmp_ctx *ctx);
int64_t pmp_get_saturation_reruns(const pmp_ctx *ctx);
int pmp_clear_saturation(pmp_ctx *ctx);

/* Caller keeps ownership of blob/descs; the library re-packs into its kernel layouts in device memory.
 * Every tensor the net needs must be present with the reference's shape (else PMP_E_INVALID). */
int pmp_load_weights(pmp_ctx *ctx, int net_id, int qp, const float *blob, const pmp_tensor_desc *descs,
                     int ndesc);
/* The same from the product's weight container (<Comp>_{Q,BD}_<qp>.pmpw, pmp_vvc_tip2023_amd/weights.py; tools/convert_weights.py
 * makes one from a reference .pkl): for hosts without Python, e.g. the in-process VTM hook (tools/vtm_build/pmp_hook.cpp).
 * The manifest's net and QP must match the arguments. */
int pmp_load_weights_file(pmp_ctx *ctx, int net_id, int qp, const char *path);
int pmp_has_weights(const pmp_ctx *ctx, int net_id, int qp);
/* Fingerprint of a loaded net's tensors / of a tensor set (names, shapes, float bit patterns; independent of the order and layout they
 * are handed over in; weights.fingerprint() computes the same number with numpy).  What ties a manifest's "act_exp" to the tensors it
 * was calibrated on: tools/calibrate_pmpw.py stores "act_fp": [this net's, its QT partner's] beside the exponents, and
 * pmp_load_weights_file ignores exponents whose fingerprints do not match what is loaded (stale file: the QT net or the tensors changed
 * since) in favour of a calibration pass.  Host-only arithmetic; pmp_fingerprint_tensors needs no context and no GPU. */
int pmp_weights_fingerprint(const pmp_ctx *ctx, int net_id, int qp, uint64_t *out);
int pmp_fingerprint_tensors(const float *blob, const pmp_tensor_desc *descs, int ndesc, uint64_t *out);

/* ---- inference: inference_pre_QBD (Metrics.py:387-419).  block_u/block_v are ignored for PMP_LUMA. --- */
int pmp_infer(pmp_ctx *ctx, int comp, int qp, const uint8_t *block_y, const uint8_t *block_u,
              const uint8_t *block_v, int64_t n, float *qt, float *bt, float *dire);
int pmp_infer_device(pmp_ctx *ctx, int comp, int qp, const uint8_t *d_block_y, const uint8_t *d_block_u,
                     const uint8_t *d_block_v, int64_t n, float *d_qt, float *d_bt, float *d_dire);

/* ---- the QT net alone: what Metrics.pre_validation(val_loader, Net, 0) runs (Metrics.py:198-212), which never touches an MTT net.
 *      pmp_infer's arguments without bt and dire.  Only the QT net of (comp, qp) has to be loaded (PMP_E_NOWEIGHTS otherwise); only its
 *      forward graph runs.  Everything else is pmp_infer's: the context's datapath, chunking, overlap mode, the taps rules, and on the
 *      f16x3 datapath the flag snapshot behind the call with the re-run - of the QT net alone - on the fp32 MFMA datapath.  No
 *      calibration pass runs and no MTT partner's calibration state changes.  qt equals the qt of pmp_infer on the same blocks, bit for
 *      bit, on all three datapaths and however the call is cut. ---- */
int pmp_infer_q(pmp_ctx *ctx, int comp, int qp, const uint8_t *block_y, const uint8_t *block_u, const uint8_t *block_v, int64_t n,
                float *qt);
int pmp_infer_q_device(pmp_ctx *ctx, int comp, int qp, const uint8_t *d_block_y, const uint8_t *d_block_u, const uint8_t *d_block_v,
                       int64_t n, float *d_qt);

/* ---- post-processing: seq_post_process minus the file (Metrics.py:764-774).  qt = RAW QT logits. -------
 *      Value domain: EVERY float32 bit pattern, with the reference's results (tests/golden/g3b_m2p_range.npz, made by the reference):
 *      - depth logits of any magnitude: np.round has no clamp (Map2Partition.py:104) and neither has this in effect - the rounded
 *        depth is only compared with candidate depths 0..6, so the kernel's integer copy saturates at +-100 without a difference;
 *        the float32 error sums (:307-312) run on the raw values in numpy's summation order, overflow to inf included;
 *      - non-finite logits (a saturated datapath under PMP_SAT_IGNORE can hand them over): a NaN / +inf depth is "deeper than any
 *        candidate" (numpy's `== 0` and `< 0` are False), -inf "shallower"; a NaN direction counts as 0, +-inf as +-1; a QT leaf
 *        holding one takes the FIRST candidate leaf (Python's min() over inf / NaN errors); a NaN QT logit survives max-pool, round
 *        and clamp (Metrics.py:632), no check_square_unity rule fires on its quadrant, its region gets no edges and directions 0
 *        (set_partition_vector, :348-362: neither == nor > holds) and qt_u8 carries 0 (numpy's .astype(uint8) of NaN on x86-64). */
int pmp_postprocess(pmp_ctx *ctx, int comp, const float *qt, const float *bt, const float *dire, int64_t n,
                    uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8);

/* ---- Map2Partition thresholds, per context and per component (PMP_LUMA / PMP_CHROMA).  Map_to_Partition takes them as constructor
 *      parameters (Map2Partition.py:100) and th_round as its `thd` (:30-35, called with 0.5 at :105).  Every post-processing entry point
 *      uses the set of its component (pmp_postprocess*, pmp_infer_postprocess*, the *_records_device forms).
 *        lamb[0] lamb1  a CU stops splitting when count_zero >= (lamb1*h)*w                    default 0.7
 *        lamb[1] lamb2  the direction map decides when (count_ver+count_hor) >= (lamb2*h)*w  default 0.7
 *        lamb[2] lamb3  ... horizontal if count_hor >= lamb3*count_ver, else vertical if
 *                       count_ver >= lamb3*count_hor                                           default 1.5
 *        lamb[3] lamb4  a split part qualifies if count_minus < num_pixel*lamb4 ...           default 0.3
 *        lamb[4] lamb5  ... and count_zero > num_pixel*lamb5                                  default 0.7
 *        thd            th_round: dire >= thd -> 1, dire <= -thd -> -1, else 0                 default 0.5
 *      Semantics are the reference's at every accepted value, ties included: the counts are compared with the DOUBLE products above in
 *      Python's evaluation order, and th_round compares the float32 logits with float32(thd) as numpy does.  th_round's third step zeroes
 *      (-thd, thd) after the first two have written +-1, so for thd > 1 every direction becomes 0: reproduced, not "fixed".  NaN and
 *      +-inf logits keep the meaning described above.
 *      Accepted domain (anything else, NaN and +-inf included, is PMP_E_INVALID and leaves the current set in force):
 *        0 <= lamb1 <= 1,  lamb2 >= 0,  lamb3 >= 0,  0 <= lamb4 <= 1,  0.67 <= lamb5 <= 1,  0 < thd <= 2  (thd as stored, a float).
 *      Why lamb5 >= 0.67: a BT and a TT split in the same direction can then never both be candidates - each would need more than
 *      lamb5 of its parts' cells at its target depth, and the TT's outer quarter is half of the BT's half with a target one level
 *      deeper, impossible for lamb5 >= 2/3 (0.67 keeps the argument clear of how 2/3 rounds).  So a CU has at most three candidates
 *      - no split, one horizontal and one vertical split - as with the defaults, and the search's worst case (the number of leaves
 *      of the depth-3 candidate tree) is no larger than with the defaults.
 *      CAPTURE AT ENQUEUE: a call uses the set that was current when it was made - a *_device call still running, every chunk of an
 *      overlap-mode call, and a post-processing call that the range guard replays at pmp_synchronize all keep their set, whatever
 *      pmp_set_partition_params does in between.
 *      pmp_set_partition_params(ctx, comp, NULL) restores the defaults.  pmp_parse_partition_params is host-only (no context, no GPU):
 *      it reads "lamb1=0.6,thd=0.45" (keys lamb1..lamb5 and thd, comma-separated, any subset, the last of a repeated key wins) on top
 *      of *inout and writes *inout only if the text parses and the result lies in the domain; "" leaves *inout as it is. ---- */
typedef struct {
    double lamb[5];    /* lamb1..lamb5 */
    float thd;
} pmp_partition_params;
int pmp_set_partition_params(pmp_ctx *ctx, int comp, const pmp_partition_params *p);
int pmp_get_partition_params(const pmp_ctx *ctx, int comp, pmp_partition_params *out);
int pmp_parse_partition_params(const char *spec, pmp_partition_params *inout);
int pmp_postprocess_device(pmp_ctx *ctx, int comp, const float *d_qt, const float *d_bt, const float *d_dire,
                           int64_t n, uint8_t *d_hor, uint8_t *d_ver, uint8_t *d_qt_u8, int8_t *d_dire_i8);

/* ---- fused: blocks in, split flags out; logits stay in HBM (qt/bt/dire may be NULL). ------------------- */
int pmp_infer_postprocess(pmp_ctx *ctx, int comp, int qp, const uint8_t *block_y, const uint8_t *block_u,
                          const uint8_t *block_v, int64_t n, uint8_t *hor, uint8_t *ver, uint8_t *qt_u8,
                          int8_t *dire_i8, float *qt, float *bt, float *dire);
int pmp_infer_postprocess_device(pmp_ctx *ctx, int comp, int qp, const uint8_t *d_block_y,
                                 const uint8_t *d_block_u, const uint8_t *d_block_v, int64_t n, uint8_t *d_hor,
                                 uint8_t *d_ver, uint8_t *d_qt_u8, int8_t *d_dire_i8, float *d_qt, float *d_bt,
                                 float *d_dire);

/* ---- the same with one packed RECORD per block, the unit the multi-GPU path gathers to the rank that writes the file
 *      (counterpart of nn.DataParallel's gather, Inference_QBD.py:223-224):
 *        u8 rec[n][PMP_RECORD_BYTES] = hor[256] | ver[256] | qt_u8[64] | dire_i8[768]
 *      written directly by the post-processing kernel (no repacking pass); d_rec must be 4-byte aligned. ---- */
#define PMP_RECORD_BYTES 1344
int pmp_postprocess_records_device(pmp_ctx *ctx, int comp, const float *d_qt, const float *d_bt, const float *d_dire,
                                   int64_t n, uint8_t *d_rec);
int pmp_infer_postprocess_records_device(pmp_ctx *ctx, int comp, int qp, const uint8_t *d_block_y, const uint8_t *d_block_u,
                                         const uint8_t *d_block_v, int64_t n, uint8_t *d_rec);

/* ---- block cutter: output_block_yuv (Inference_QBD.py:104-149).  Planes y[F][H][W], u,v[F][H/2][W/2];
 *      bitdepth 8 -> uint8 samples, 10 -> uint16 samples reduced with round-half-even(x/4), clipped to 255.
 *      Writes F*(H/64)*(W/64) blocks, frame-major then row-major; right/bottom remainders are dropped. ---- */
int pmp_cut_blocks(pmp_ctx *ctx, const void *y, const void *u, const void *v, int frames, int height, int width,
                   int bitdepth, uint8_t *block_y, uint8_t *block_u, uint8_t *block_v);
int pmp_cut_blocks_device(pmp_ctx *ctx, const void *d_y, const void *d_u, const void *d_v, int frames,
                          int height, int width, int bitdepth, uint8_t *d_block_y, uint8_t *d_block_u,
                          uint8_t *d_block_v);

/* ---- training labels: GenMSBtMap.gen_seq_sub_map (GenMSBtMap.py:434-449) = Map_to_SubMap(qt, bt, dire, cf).get_sub_map() per block
 *      (:89-368), the per-layer MTT depth maps (MSBT) that Train_QBD fits the MSBD net to.  The candidate-tree search of Map2Partition
 *      with other rules; one workgroup per block (labels.hip).  Inputs in CreateDataSet's dtypes, on which the reference's result
 *      depends:
 *        qt   u8[n][8][8]      VTM qtDepth - 1 as GenMSBtMap.main_process passes it (:477; a u8 subtraction, so 0 becomes 255);
 *                              read at each QT node's top-left cell only (set_sub_map, :314-324)
 *        bt   u8[n][16][16]    final MTT depth of each 4x4 cell
 *        dire i8[n][3][16][16] per-layer direction, 1 horizontal, -1 vertical (other values count as neither)
 *      Outputs: msbt u8[n][3][16][16] (the maps of the best leaf's depth-1 and depth-2 ancestors and of the leaf, :341-363) and
 *      status u8[n].  cf = the chroma factor, 1 or 2 (the reference's main_process passes is_luma=True, i.e. cf 1, for BOTH components).
 *      Rules (GenMSBtMap.py), reproduced bit for bit: lamb1..lamb5 = 0.8, 1.0, 1.2, 0.2, 0.2, counts compared with the float64 products
 *      in Python's order ((lamb1*h)*w, num_pixel*(1 - lamb5) with 1 - 0.2 formed in float64); "no partition" compares the label bt with
 *      the node's map; a direction map that does not dominate gives [0]; the candidate list starts empty and a CU with an empty list
 *      leaves its node without children, so leaves can sit above depth 3; the leaf error np.sum(np.abs(leaf - bt)) subtracts two u8
 *      maps and WRAPS: a leaf one level shallower than the label costs 255 per cell, not 1 (a root leaf's map is i8: it costs sum(bt));
 *      the first minimum in DFS leaf order wins.  With bt held in a wider integer type the reference picks other labels for some
 *      blocks: these results are the u8 ones.
 *      Where the reference gives no usable answer, status bits (OR-ed over the block's QT regions; other regions are unaffected):
 *        PMP_MSBT_INCONSISTENT  the best leaf of a region is shallower than depth 3 (the reference raises AttributeError, :342-349,
 *                               ending the whole dataset run).  Carry-down: msbt[k] = the map of the ancestor at depth min(k+1, d),
 *                               all zeros for d = 0.
 *        PMP_MSBT_QT_DEEP       a qt value above 3 was reached at a depth-3 node: its region stays zero, which is what the reference
 *                               produces for 4..~10 (it recurses on empty regions; for larger values practically forever).
 *        PMP_MSBT_BUDGET        a region's candidate tree has more than PMP_MSBT_LEAF_BUDGET leaves: scoring stops at the first leaf
 *                               beyond the budget and the best of the leaves scored so far, in the reference's order, is kept.  Valid
 *                               partitions need at most a few dozen leaves; labels that admit every legal split give up to 2.7 M for a
 *                               64x64 luma region.  A 1024-block launch of such blocks: profiles/msbt_labels.txt.
 *      pmp_msbt_labels takes host pointers and runs in passes of at most pmp_set_chunk blocks; pmp_msbt_labels_device takes device
 *      pointers (qt, bt, dire, msbt 4-byte aligned) and runs stream-ordered on the context's stream.  n = 0 does nothing. ---- */
#define PMP_MSBT_LEAF_BUDGET 4096
#define PMP_MSBT_INCONSISTENT 1
#define PMP_MSBT_QT_DEEP 2
#define PMP_MSBT_BUDGET 4
int pmp_msbt_labels(pmp_ctx *ctx, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *msbt,
                    uint8_t *status);
int pmp_msbt_labels_device(pmp_ctx *ctx, int cf, const uint8_t *d_qt, const uint8_t *d_bt, const int8_t *d_dire, int64_t n,
                           uint8_t *d_msbt, uint8_t *d_status);

/* ---- the labels' own partition: GenMSBtMap.map_to_parititon (GenMSBtMap.py:377-382) = Map_to_SubMap(qt, bt, dire, cf).get_partition()
 *      (:262-312) per block, cropped to [:16, :16] - the split flags that GenMSBtMap.get_sequence_partition_for_VTM (:384-432) writes
 *      into a PartitionMat file.  Such a file is a perfect predictor's: fed to the patched VTM it gives the ceiling of speed-up and
 *      BD-rate that the map representation allows, and it needs no trained net.  Same kernel family (labels.hip), same inputs, dtypes,
 *      thresholds, u8-wrapping leaf error, first-minimum rule and leaf budget as pmp_msbt_labels above.  What is painted, bit for bit
 *      as the reference paints it:
 *        - the QT walk of set_partition_vector (:294-309): a node at depth d whose qt (read at its top-left cell) exceeds d paints the
 *          cross of its region [2qx, 2qy, 2sms, 2sms], sms = 8 >> d: hor row 2qx+sms over columns 2qy..2qy+2sms-1 and ver column 2qy+sms
 *          over rows 2qx..2qx+2sms-1 - at d = 3 as well, where the reference then recurses on empty regions and paints nothing more
 *          (PMP_MSBT_QT_DEEP is set); a node with qt < d paints nothing;
 *        - a node with qt == d searches its region (set_bt_partition_vector, :262-292) and paints every CU [x, y, h, w] of the best
 *          leaf: hor[x][y..y+w-1], hor[x+h][y..y+w-1], ver[x..x+h-1][y], ver[x..x+h-1][y+w]; row and column 16 of the reference's
 *          u8[2][17][17] par_vec are cropped away (:382).
 *      A best leaf above depth 3 is legal here (set_bt_partition_vector never walks a leaf's parents, so the reference does not raise):
 *      status bit 1 (PMP_MSBT_INCONSISTENT) is NEVER set by these calls.  Status bits, OR-ed over the block's QT nodes:
 *        PMP_MSBT_QT_DEEP  a qt value above 3 was reached at a depth-3 node: its cross is painted and nothing else (the reference's result
 *                          for 4..~10; beyond that it recurses practically forever).
 *        PMP_MSBT_BUDGET   a region has more than PMP_MSBT_LEAF_BUDGET leaves: the CUs of the best of the first PMP_MSBT_LEAF_BUDGET leaves,
 *                          in the reference's order, are painted (the reference scores them all and may choose another).
 *      Outputs: hor, ver u8[n][16][16] (0 / 1) and status u8[n]; every byte is written.  The _records form writes one packed record
 *      u8[n][PMP_RECORD_BYTES] = hor | ver | qt | dire per block instead, qt and dire being byte copies of the inputs - what the reference
 *      puts into the file's qt and direction sections (:407-408) - so that pmp_format_partition_rows_records and
 *      pmp_tile_partition_rows_records take it as they take the post-processing kernel's records.  NOTE on the file: the reference casts
 *      the direction section to u8 before printing (:413), so -1 appears as "255"; VTM reads it with stoi into an int8_t (Rom.h:247), where
 *      255 is -1 again.  The writers of this library print "-1", as in every other PartitionMat file they write.
 *      The same inputs give the same bits on every run (per-wave row masks combined in a fixed order, no atomics).
 *      pmp_label_partition takes host pointers and runs in passes of at most pmp_set_chunk blocks; the _device forms take device pointers
 *      (qt, bt, dire, hor, ver, rec 4-byte aligned: PMP_E_INVALID otherwise) and run stream-ordered on the context's stream.  n = 0 does
 *      nothing and touches no buffer.  cf other than 1 or 2, n < 0 or a NULL pointer with n > 0: PMP_E_INVALID. ---- */
int pmp_label_partition(pmp_ctx *ctx, int cf, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t n, uint8_t *hor,
                        uint8_t *ver, uint8_t *status);
int pmp_label_partition_device(pmp_ctx *ctx, int cf, const uint8_t *d_qt, const uint8_t *d_bt, const int8_t *d_dire, int64_t n,
                               uint8_t *d_hor, uint8_t *d_ver, uint8_t *d_status);
int pmp_label_partition_records_device(pmp_ctx *ctx, int cf, const uint8_t *d_qt, const uint8_t *d_bt, const int8_t *d_dire, int64_t n,
                                       uint8_t *d_rec, uint8_t *d_status);

/* ---- validation: how well does a pair of nets predict what VTM decided.  The arithmetic of Metrics.validation_QBD (Metrics.py:313-385),
 *      Metrics.pre_validation predID 0 / 1 (:196-274) and the losses under them (loss_func_QBD_val, loss_func_MSBD_val, weight_mat,
 *      :148-194) for ONE batch of n blocks (valstats.hip).  Logits in the library's layouts - qt f32[n][8][8], bt, dire f32[n][3][16][16]
 *      (layer k = the reference's bd_out_batchK[:, 0] / [:, 1]) - against labels in the dtypes of the label files (gen_labels):
 *        qt8    u8[n][8][8]       RAW qtDepth as saved (<..>_QTdepth_Block8.npy)
 *        msbt   u8[n][3][16][16]  (<..>_MSBTdepth_Block16.npy)
 *        msdire i8[n][3][16][16]  (<..>_MSdirection_Block16.npy)
 *      converted as the reference's loader converts them (Metrics.py:127-135): bl = float(msbt), dl = float(msdire) and
 *      ql = float(qt8 - 1) where the subtraction is numpy's ON THE u8 ARRAY: a raw qtDepth of 0 becomes 255.0, not -1.0 (the quirk
 *      pmp_msbt_labels documents for its qt input).  Reproduced, not "fixed".
 *      The twenty numbers (elements = how many terms a sum or count runs over):
 *        S[0]       sum |qt - ql|                                                        64 n
 *        S[1..3]    sum |bt_k - bl_k|,  k = 0..2                                         256 n each
 *        S[4..6]    sum |dire_k - dl_k|                                                  256 n each
 *        S[7..9]    sum |w_k*dire_k - w_k*dl_k|                                          256 n each
 *        S[10]      sum |w_0*bt_0 - w_0*bl_0|                                            256 n
 *        S[11,12]   sum |w_k*(bt_k - bt_{k-1}) - w_k*(bl_k - bl_{k-1})|,  k = 1, 2        256 n each
 *        S[13]      #(round(qt) == ql)                                                   64 n
 *        S[14..16]  #(round(bt_k) == bl_k)                                               256 n each
 *        S[17..19]  #(round(dire_k) == dl_k)                                             256 n each
 *      with w_k = dl_k*dl_k + float32(weight_mat[int((qp - 22) / 5)][k]), weight_mat = 0.5 * {{1.0, 0.73, 0.15}, {2.43, 0.35, 0.10},
 *      {0.96, 0.23, 0.07}, {0.59, 0.16, 0.05}} (Metrics.py:148-151), and w_0 = 1.0 when qp == 22 (:180-181).  22 <= qp <= 41 (rows 0..3),
 *      PMP_E_INVALID otherwise.  From them, per batch: an L1 loss is S / elements, an accuracy hits / elements, and
 *        loss_func_QBD_val  = S0/(64n) + (0.8 S1 + 1.0 S2 + 1.2 S3 + S7 + S8 + S9 + 0.5 (S10 + S11 + S12)) / (256n)
 *        loss_func_MSBD_val = the same without S0/(64n).
 *      TERMS: every per-element term is computed as torch computes it - float32 operations in the reference's order (w*out, w*label,
 *      the subtraction, abs; for S[11], S[12] the two differences first), no fused multiply-add, the float64 weight_mat entry rounded
 *      to float32 before the add.  round is torch.round: half to even.  A NaN logit is never a hit; NaN / inf logits give NaN / inf sums
 *      as torch does; nothing is clamped.
 *      DETERMINISM: the sums are float64, added in a fixed order that depends on n only - one wavefront per block (lane partials in cell
 *      order, a fixed butterfly over the 64 lanes), per-block partials f64[n][20], then one workgroup that adds them in a fixed order.
 *      No atomics.  The same inputs give the same bits on every run, stream, context and chunk setting of pmp_val_stats_device; the seven
 *      counts are integers and exact (stored as float64).  Against the reference's float32 batch means the sums differ by the reference's
 *      own float32 summation error (about 1e-7 relative on 200-block batches; tests/golden/g12_val.npz records the measured distance).
 *      FORMS: bt, dire, msbt, msdire all NULL = QT only (pre_validation predID 0): S[0] and S[13] filled, the rest 0.  qt and qt8 both
 *      NULL = MTT only: S[0] = S[13] = 0.  Any other NULL mix, n < 0 or a NULL stats: PMP_E_INVALID.  n = 0: twenty zeros, no launch.
 *      pmp_val_stats_device: device pointers (bt, dire 16-byte aligned, msbt, msdire 4-byte aligned: PMP_E_INVALID otherwise), stream-ordered
 *      on the context's stream, the host does not wait.  d_block_stats (may be NULL): the per-block partials f64[n][20] as an OUTPUT - the
 *      twenty numbers of each block on its own (hit counts as float64), which is where one looks for the blocks a net gets wrong; d_stats
 *      is their fixed-order sum.  RANGE GUARD: the logits may come from a pmp_infer*_device call whose range flag has not been looked at
 *      yet.  Like a post-processing call, a statistics call enqueued behind such a call is REPLAYED, in order, if that call is re-run: once
 *      pmp_synchronize has returned, d_stats and d_block_stats are those of the FINAL logits (and equal, bit for bit, what a second call
 *      made after the synchronize gives).  Synchronising the stream yourself is enough only if you know the flag stayed down; logits,
 *      labels and outputs must stay untouched until then.
 *      pmp_val_stats: host pointers; runs in passes of at most pmp_set_chunk blocks through staging buffers and returns the statistics of
 *      the WHOLE call as one batch: the pass results added in pass order in float64.  Its bits therefore depend on the chunk setting (the
 *      order of the float64 additions does); the counts never do. ---- */
#define PMP_VAL_NSTATS 20
int pmp_val_stats(pmp_ctx *ctx, int qp, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                  const int8_t *msdire, int64_t n, double stats[PMP_VAL_NSTATS]);
int pmp_val_stats_device(pmp_ctx *ctx, int qp, const float *d_qt, const float *d_bt, const float *d_dire, const uint8_t *d_qt8,
                         const uint8_t *d_msbt, const int8_t *d_msdire, int64_t n, double *d_stats, double *d_block_stats);

/* ---- validation: WHICH WAY the nets err, and how the labels are distributed.  S[13..19] above add two different errors together: a
 *      predicted depth below the label cuts off splits the encoder can no longer try, one above it forces splits it did not want
 *      (EncModeCtrl.cpp:2005-2015).  counts[m][l][p] is the number of cells of map m (0 qt, 1..3 bt_k, 4..6 dire_k) whose label has class
 *      l and whose prediction has class p: the joint histogram per map.  Its diagonal over the valid classes is S[13 + m], its row sums
 *      are the census of the labels.  Layouts, dtypes and label conversion are pmp_val_stats' (ql = float(u8(qt8 - 1)): a raw qtDepth of 0
 *      is the label 255); there is no qp, nothing is weighted.  A prediction is r = rintf(logit): torch.round, half to even.
 *      CLASS of a value v, label or r alike:
 *        depth maps (qt, bt_k)   v if v is one of 0, 1, 2, 3, else 4 ("other")
 *        direction maps          v + 1 if v is one of -1, 0, 1, else 3 ("other"); class 4 stays zero there
 *      so -0.0 is class 0 and, on a depth map, the label 255, a label of 4 or more, a negative r, an r of 4 or more, NaN and +-inf are
 *      all class 4.  Counts are integers: no floating-point value is added anywhere, the result is exact and depends on no order.
 *      FORMS, the QT group (qt, qt8) and the MTT group (bt and dire, msbt and msdire) independently: logits and labels given = the
 *      group's confusion; labels only = their CENSUS, every prediction counted as "other" (class 4, 3 on direction maps), so that the row
 *      sums are the label counts; neither = the group's cells are zero.  PMP_E_INVALID, before any launch and with nothing written: logits
 *      without their labels, bt without dire or msbt without msdire, no labels at all, n < 0, NULL counts, a misaligned pointer
 *      (pmp_val_stats_device's alignments; d_counts 8-byte, d_block_counts 2-byte).  n = 0: 175 zeros, no launch.  Every element of
 *      d_counts, and of d_block_counts if given, is written by every call; nothing is accumulated across calls.
 *      pmp_val_confusion_device: stream-ordered, the host does not wait.  d_block_counts (may be NULL): the counts of each block on its
 *      own, u16[n][175] (a block's cell is at most 256); d_counts is their column sum in int64.  RANGE GUARD: replayed behind a re-run
 *      exactly as a pmp_val_stats_device call is - after pmp_synchronize the counts are those of the FINAL logits.
 *      pmp_val_confusion: host pointers, in passes of at most pmp_set_chunk blocks; the passes' counts are added. ---- */
#define PMP_CONF_MAPS 7        /* qt, bt0, bt1, bt2, dire0, dire1, dire2 */
#define PMP_CONF_CLASSES 5
#define PMP_CONF_NCOUNTS (7*5*5)
int pmp_val_confusion(pmp_ctx *ctx, const float *qt, const float *bt, const float *dire, const uint8_t *qt8, const uint8_t *msbt,
                      const int8_t *msdire, int64_t n, int64_t counts[PMP_CONF_NCOUNTS]);
int pmp_val_confusion_device(pmp_ctx *ctx, const float *d_qt, const float *d_bt, const float *d_dire, const uint8_t *d_qt8,
                             const uint8_t *d_msbt, const int8_t *d_msdire, int64_t n, int64_t *d_counts, uint16_t *d_block_counts);

/* ---- training: the objective the nets are trained on and its gradient with respect to the logits, in one pass (trainloss.hip).
 *      The arithmetic of Train_QBD.loss_func_QBD (Train_QBD.py:68-90), Train_QBD.loss_func_MSBD (:44-66) and the plain L1_Loss of
 *      pre_train_Q (:161), and of torch's backward pass through them, for ONE batch of n blocks.  These are NOT the validation losses
 *      above: they take ten weights (Train_QBD's --lambq, --lambb0..2, --lambd0..2, --lambresb0..2, :448-457) and chroma nets use a
 *      second weight matrix.  Logits and labels in the layouts and dtypes of pmp_val_stats, converted the same way (ql = float(u8(qt8 - 1)):
 *      a raw qtDepth of 0 becomes 255.0; bl = float(msbt); dl = float(msdire)).
 *      WEIGHTS: w_k = dl_k*dl_k + float32(M[int((qp - 22) / 5)][k]), 22 <= qp <= 41, M = luma_weight_mat (= weight_mat above) for PMP_LUMA and
 *      chroma_weight_mat = 0.5 * {{17.83, 0.49, 0.11}, {1.20, 0.25, 0.07}, {0.58, 0.17, 0.05}, {0.38, 0.12, 0.04}} for PMP_CHROMA
 *      (Train_QBD.py:35-42); w_0 = 1.0 when qp == 22, for both components (:53-54, :76-77).
 *      SUMS: T[0..12] are, term for term and in the same order of additions, S[0..12] of pmp_val_stats with the component's matrix in w -
 *      for PMP_LUMA they equal pmp_val_stats_device's, bit for bit.  T[4..6], the unweighted direction L1 sums, are not part of the loss;
 *      the training loops print them (Train_QBD.py:249-251).
 *      LOSS, a float64 formed in this written order:
 *        loss = lambq*T0/(64n) + (lambb0*T1 + lambb1*T2 + lambb2*T3 + lambd0*T7 + lambd1*T8 + lambd2*T9
 *                                 + lambresb0*T10 + lambresb1*T11 + lambresb2*T12)/(256n)
 *      GRADIENTS of that loss (optional).  sgn(x) is torch.sign, by which torch's backward of abs multiplies: +1, -1, and 0 for x == 0
 *      AND for a NaN x (measured on the reference: a NaN term, an inf - inf layer difference included, gives a ZERO gradient, while the
 *      loss is NaN; +-inf terms give -+1).  Every sign is taken of the float32 term exactly as the sums form it, so a term that is exactly
 *      zero in float32 contributes zero:
 *        a_k = sgn(bt_k - bl_k)      c_k = sgn(w_k*dire_k - w_k*dl_k)      e_0 = sgn(w_0*bt_0 - w_0*bl_0)
 *        e_k = sgn(w_k*(bt_k - bt_{k-1}) - w_k*(bl_k - bl_{k-1})),  k = 1, 2
 *        g_qt     = lambq*sgn(qt - ql) / (64n)
 *        g_dire_k = lambd_k*w_k*c_k / (256n)
 *        g_bt_k   = (lambb_k*a_k + lambresb_k*w_k*e_k - [k < 2] lambresb_{k+1}*w_{k+1}*e_{k+1}) / (256n)
 *      each computed in float64 from the float32 w and the double weights, left to right as written, and rounded ONCE to float32.  Every
 *      byte of a requested gradient tensor is written.  Against torch's float32 backward they differ by float32 rounding only
 *      (tests/golden/g14_train_loss.npz records the measured distance); their zero pattern is torch's.
 *      DETERMINISM: as pmp_val_stats - float64 sums in a fixed order that depends on n only, no atomics, the same bits on every run,
 *      stream, context and chunk setting of pmp_train_loss_device.
 *      FORMS (the NULL rules of pmp_val_stats): all inputs = loss_func_QBD; qt, qt8 NULL = loss_func_MSBD (T[0] = 0); bt, dire, msbt,
 *      msdire NULL = pre_train_Q's L1 (T[1..12] = 0; pass lambq = 1).  p NULL = Train_QBD's defaults.  terms and loss are required.
 *      Gradient pointers: all NULL (value only, nothing else is written) or exactly those of the form's logits.  PMP_E_INVALID before
 *      any launch, nothing written: any other mix, comp not PMP_LUMA / PMP_CHROMA, n < 0, qp outside 22..41, a weight that is not
 *      finite, NULL terms or loss, a gradient tensor that overlaps an input.  n = 0: thirteen zeros, loss 0, no launch.
 *      pmp_train_loss_device: device pointers - bt, dire, g_bt, g_dire 16-byte aligned, the other inputs and g_qt 4-byte, terms and loss
 *      8-byte (PMP_E_INVALID otherwise) - stream-ordered on the context's stream; the host does not wait for the kernel.  RANGE GUARD:
 *      unlike a statistics call it is never queued for a replay: it first SETTLES the context's calls in flight, as the pmp_debug_set_*
 *      calls do, so a caller whose logits come from a pending pmp_infer*_device call gets the loss of the FINAL logits (and waits for
 *      them).  Logits that come from elsewhere (a torch forward pass) find nothing in flight and pay nothing.
 *      pmp_train_loss: host pointers; runs in passes of at most pmp_set_chunk blocks through staging buffers.  The sums are the pass
 *      sums added in pass order (so their bits depend on the chunk setting), the loss is formed from them on the host in the same
 *      float64 order, and every pass divides by the WHOLE call's n: the gradients do not depend on the chunk setting.
 *      pmp_parse_loss_params is host-only (no context, no GPU): it reads "lambb0=0.8,lambresb2=0" (keys lambq, lambb0..2, lambd0..2,
 *      lambresb0..2, comma-separated, any subset, the last of a repeated key wins) on top of *inout and writes *inout only if the
 *      whole text parses to finite numbers; "" leaves *inout as it is. ---- */
typedef struct {
    double lambq, lambb[3], lambd[3], lambresb[3];   /* defaults 1.0 | 0.8, 1.0, 1.2 | 1, 1, 1 | 0.5, 0.5, 0.5 (Train_QBD.py:448-457) */
} pmp_loss_params;
#define PMP_LOSS_NTERMS 13
int pmp_parse_loss_params(const char *spec, pmp_loss_params *inout);
int pmp_train_loss(pmp_ctx *ctx, int comp, int qp, const pmp_loss_params *p, const float *qt, const float *bt, const float *dire,
                   const uint8_t *qt8, const uint8_t *msbt, const int8_t *msdire, int64_t n, double terms[PMP_LOSS_NTERMS], double *loss,
                   float *g_qt, float *g_bt, float *g_dire);
int pmp_train_loss_device(pmp_ctx *ctx, int comp, int qp, const pmp_loss_params *p, const float *d_qt, const float *d_bt,
                          const float *d_dire, const uint8_t *d_qt8, const uint8_t *d_msbt, const int8_t *d_msdire, int64_t n,
                          double *d_terms, double *d_loss, float *d_g_qt, float *d_g_bt, float *d_g_dire);

/* ---- training: ONE Model_QBD.ResidualBlock (Model_QBD.py:23-44), forward and backward, on this library's kernels - about 97 % of the
 *      nets' FLOPs in training as in inference.  t = relu(conv0(x)), out = relu(conv2(t) + sc(x)); both convolutions k x k, stride 1,
 *      zero padding k/2, no bias; sc is the identity when cin == cout and a 1x1 convolution otherwise.  Backward, from the saved x, t,
 *      out and the upstream gradient g_out, in this order:
 *        gu    = g_out where out > 0, else 0
 *        g_w2  = wgrad(t, gu)                         wgrad(a, g)[co][ci][dy][dx] = sum over (n, y, x) of g[n][co][y][x] *
 *        g_wsc = wgrad_1x1(x, gu)   (cin != cout)                                    a[n][ci][y + dy - k/2][x + dx - k/2]
 *        gt    = conv(gu, flipT(w2)) where t > 0, else 0        flipT: taps mirrored, cin and cout swapped
 *        g_w0  = wgrad(x, gt)
 *        g_x   = conv(gt, flipT(w0)) + gu             (cin == cout)
 *              = conv(gt, flipT(w0)) + conv1x1(gu, wsc transposed)   (cin != cout)
 *      The masks are exactly `> 0` of the t and out the CALLER passes - and open where t or out is NaN, torch's ReLU backward - so a
 *      trainer may hand in the tensors the forward call returned or its own.
 *      ARITHMETIC: always the fp32 MFMA datapath (v_mfma_f32_16x16x4_f32, a chain of fused multiply-adds in float32), whatever
 *      pmp_set_precision says.  The forward is the launches of the inference graph on PMP_PRECISION_F32, bit for bit.  The weight
 *      gradients are reduced over (n, 16x16 tile) in two stages in an order that depends on the shape only, without atomics: the same
 *      bits on every run, stream, context and device.  On values whose every product and sum is exactly representable in float32 every
 *      result is exact.  NaN and +-inf in any tensor: NON-FINITE VALUES IN THE TRAINING CALLS, below.
 *      TENSORS: dense fp32 in torch's layouts at true scale - x, g_x [n][cin][h][w]; t, out, g_out [n][cout][h][w]; w0, g_w0
 *      [cout][cin][k][k]; w2, g_w2 [cout][cout][k][k]; wsc, g_wsc [cout][cin].  wsc (and, backward, g_wsc) are passed exactly when
 *      cin != cout and NULL otherwise.  g_x may be NULL: it is then not computed and nothing is written for it (a first block whose
 *      input needs no gradient).  Every byte of every requested output is written.
 *      SHAPES: n in 1..256; h and w multiples of 16 in 16..256; cin and cout in 1..64 (padded to 16, 32 or 64 internally); k 3 or 5.
 *      PMP_E_INVALID before any launch, nothing written: a NULL shape, any other shape, a missing tensor or a shortcut tensor that
 *      should not be there, an output that overlaps an input or another output, and for the _device forms a pointer that is not
 *      4-byte aligned.
 *      pmp_resblock_*_device: device pointers, stream-ordered on the context's stream; the host does not wait and the weights - which
 *      change every optimiser step - are packed on the device, never copied to the host.  Like pmp_train_loss_device the call first
 *      SETTLES the context's calls in flight.  Intermediates live in the context's activation workspace (pmp_get_workspace_bytes).
 *      pmp_resblock_forward / _backward: host pointers, staged through the context's buffers; they return final results. ---- */
typedef struct pmp_rb_shape {
    int n, h, w, cin, cout, k;
} pmp_rb_shape;
int pmp_resblock_forward(pmp_ctx *ctx, const pmp_rb_shape *shape, const float *x, const float *w0, const float *w2, const float *wsc,
                         float *t, float *out);
int pmp_resblock_forward_device(pmp_ctx *ctx, const pmp_rb_shape *shape, const float *d_x, const float *d_w0, const float *d_w2,
                                const float *d_wsc, float *d_t, float *d_out);
int pmp_resblock_backward(pmp_ctx *ctx, const pmp_rb_shape *shape, const float *x, const float *t, const float *out, const float *w0,
                          const float *w2, const float *wsc, const float *g_out, float *g_x, float *g_w0, float *g_w2, float *g_wsc);
int pmp_resblock_backward_device(pmp_ctx *ctx, const pmp_rb_shape *shape, const float *d_x, const float *d_t, const float *d_out,
                                 const float *d_w0, const float *d_w2, const float *d_wsc, const float *d_g_out, float *d_g_x,
                                 float *d_g_w0, float *d_g_w2, float *d_g_wsc);

/* ---- NON-FINITE VALUES IN THE TRAINING CALLS (pmp_resblock_*, pmp_trunk_*, pmp_qtail_*, pmp_stem_*, pmp_head_* / pmp_gate_*).  A trainer
 *      notices a diverged run by a NaN or inf loss, so NaN and +-inf are ordinary data here and travel as they do in torch (what to DO
 *      about a gradient that is not finite is the caller's: THE DIVERGENCE GUARD under TRAINING STEP counts them on the device).  For every
 *      tensor a call writes let R be the elements that are not finite when torch computes the same call on the CPU under autograd
 *      (F.conv2d, F.relu, F.max_pool2d, F.interpolate as Model_QBD.py uses them), L those that are not finite in this library's result,
 *      and S the REACH of the non-finite inputs: what the same net reaches with every weight non-zero (a split stem: with its three
 *      kernels zero-padded to the one k x k kernel the library runs), every ReLU open and the pools kept - forward from the non-finite
 *      input elements; backward from the non-finite gradient elements and from whatever the forward pass reached in a tensor that a
 *      gradient is masked or routed by.  Weight and bias gradients are reachable as a whole, and a non-finite weight reaches everything.
 *        1. DETECT   R is inside L.  Whether an element is NaN or inf, and its sign, is not specified.
 *        2. CONTAIN  L is inside S.
 *        3. Outside S every element is what the call gives without the non-finite inputs: the same bits.
 *      How: relu(NaN) = NaN, relu(-inf) = +0; the maximum of a window that holds a NaN is NaN (2x2 pools, the QT tail's 2/4/8 windows);
 *      a ReLU's backward passes g where the output is > 0 OR NaN (`out <= 0 ? 0 : g`, torch's threshold_backward); a pool's backward
 *      gives the window's gradient to its LAST NaN if it holds one, else to its first maximum.  On finite values every result has the
 *      bits it had before this was specified.
 *      Where L is larger than R (all inside S):
 *        - zero times non-finite is NaN.  Padded channel lanes and a split stem's zero taps have zero weights; the QT tail's q6 runs on
 *          a map padded to 16 with a 0/1 region product; gt is the transposed convolution TIMES the 0/1 mask of t.  So an inf in a real
 *          channel makes its pixel's padded lanes NaN, the next convolution spreads that over its window in every channel, and an inf
 *          may come out as NaN.  The invariant "padded channels are zero" holds for FINITE inputs only.
 *        - a pool window with several NaNs: which of them gets the gradient is torch's rule here, but a caller should not rely on it.
 *      Where a result need not be non-finite on either side: a sum that overflows float32 in one order of summation and not in another
 *      (a * 3e38 - b * 3e38: an MFMA's four-term inner product does not round in between, a chain of float32 additions does).
 *      INFERENCE is not part of this: conv_mfma is also the fp32 inference datapath (PMP_PRECISION_F32, the range guard's fallback),
 *      and there its ReLU and pool stay max(v, 0) and max(a, b), which map a NaN to 0 or to the other operand - one kernel, the
 *      NaN's way through the ReLU behind a flag that only the training calls set.  Inference results do not move, on finite data or
 *      any other.  The
 *      f16x3 and bf16x6 datapaths and the fused 16x16 / 32x32 kernels are unchanged as well: a NaN raises their range flag.
 *      tests/nonfinite_cases.py, tests/test_gpu_nonfinite.py. ---- */

/* ---- training: a TRUNK - an nn.Sequential of 1..8 ResidualBlocks, optionally followed by F.max_pool2d(., 2) (Model_QBD.py:112-125,
 *      :136-137, :151: trunk_M1 = 6 blocks + pool, trunk_M2 = 4 + pool, trunk_B1..B3 = 3, trunk_Att1/2 = 2, resblock_q1/q2 = 1 + pool):
 *        y = [max_pool2d(., 2)] (block_{L-1} o ... o block_0)(x)
 *      Every block is exactly pmp_resblock_forward's block - the same formulas, the same fp32 MFMA datapath, the same bits - but the
 *      activations stay in the kernels' blocked layout between the blocks and between forward and backward: x goes dense -> blocked
 *      once, y (and g_x) blocked -> dense once, where a chain of pmp_resblock_* calls converts eight tensors per block.
 *      SHAPE: block i is cin_i -> cout[i] with k[i] (3 or 5), cin_0 = cin and cin_i = cout[i-1]; n 1..256; h and w multiples of 16 in
 *      16..256; every channel count 1..64; nblocks 1..PMP_TRUNK_MAX_BLOCKS; pool 0 or 1.
 *      TENSORS (device pointers, dense fp32 in torch's layouts): x, g_x [n][cin][h][w]; y, g_y [n][cout_last][h][w], with pool
 *      [n][cout_last][h/2][w/2]; d_w and d_g_w are HOST arrays of 3 * nblocks device pointers - w0, w2, wsc of block 0, then of block
 *      1, ... - in pmp_resblock_*'s layouts, the wsc entry NULL exactly where cin_i == cout[i], and d_g_w NULL exactly where d_w is.
 *      d_saved: pmp_trunk_saved_bytes(shape) bytes the caller owns, 16-byte aligned, OPAQUE: the blocked x, every t_i and every out_i
 *      (the last one un-pooled).  Forward writes every byte of it that backward or unpack reads; backward and unpack only read it.
 *      pmp_trunk_unpack_device copies one saved tensor out in torch's dense layout: index 0 = x, 2i + 1 = t_i, 2i + 2 = out_i.
 *      BACKWARD walks the blocks from the last to the first with pmp_resblock_backward's six steps per block, in that order; the g_x of
 *      block i + 1 becomes the g_out of block i without leaving the blocked layout.  d_g_x may be NULL: the first block's data gradient
 *      is then not computed and nothing is written for it.  Every byte of every requested output is written.
 *      POOL BACKWARD: the gradient of a 2x2 window goes to its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1) - torch's
 *      max_pool2d rule (`val > maxval` replaces, so ties keep the earlier element) - recomputed from the saved un-pooled out; no index
 *      tensor is stored.  With a NaN in the window the gradient goes to the window's LAST NaN, as torch's (`|| isnan(val)`); non-finite
 *      values otherwise as in pmp_resblock_* (NON-FINITE VALUES IN THE TRAINING CALLS, above).
 *      PMP_E_INVALID before any launch, nothing written: a NULL or unsupported shape; a missing tensor; a shortcut pointer present
 *      where cin_i == cout[i] or absent where they differ; a d_g_w whose NULL pattern differs from d_w's; an output that overlaps an
 *      input or another output (d_saved is an output of forward and an input of backward and unpack); a pointer that is not 4-byte
 *      aligned (d_saved: 16-byte); an index out of range.  pmp_trunk_saved_bytes returns PMP_E_INVALID (< 0) for such a shape; it
 *      needs no context and no GPU.
 *      Like pmp_resblock_*_device the calls first SETTLE the context's calls in flight and run stream-ordered on its stream; the
 *      intermediates (one block's working set and the running gradient) live in the activation workspace.
 *      There are NO host-pointer forms: the saved activations are device-resident by design (trunk_M1 at n = 200 saves 2.6 GB), and a
 *      host form would copy them out and back between the two calls. ---- */
#define PMP_TRUNK_MAX_BLOCKS 8
typedef struct pmp_trunk_shape {
    int n, h, w, cin, nblocks;
    int cout[PMP_TRUNK_MAX_BLOCKS], k[PMP_TRUNK_MAX_BLOCKS];
    int pool;
} pmp_trunk_shape;
int64_t pmp_trunk_saved_bytes(const pmp_trunk_shape *shape);
int pmp_trunk_forward_device(pmp_ctx *ctx, const pmp_trunk_shape *shape, const float *d_x, const float *const *d_w, void *d_saved,
                             float *d_y);
int pmp_trunk_backward_device(pmp_ctx *ctx, const pmp_trunk_shape *shape, const void *d_saved, const float *const *d_w,
                              const float *d_g_y, float *d_g_x, float *const *d_g_w);
int pmp_trunk_unpack_device(pmp_ctx *ctx, const pmp_trunk_shape *shape, const void *d_saved, int index, float *d_dense);

/* ---- training: a net's STEM - its first layer, a bias convolution with 1..4 input channels, 32 outputs and a ReLU, at full resolution
 *      (Model_QBD.py:79-80, :132-135, :177-178, :230-233).  With p = k / 2, x is f32 [n][cin][h + p][w + p], dense; everything to the
 *      right of and below x is zero (the nets' padding_rb, padding_r and padding_b, folded into index arithmetic), and
 *        split = 0 (QT nets):   y = relu(conv_kxk(x, w[0]) + b[0]),                       w[0] [32][cin][k][k], b[0] [32]
 *        split = 1 (MTT nets):  y = relu(cat[conv(x, w[0]) + b[0], conv(x, w[1]) + b[1], conv(x, w[2]) + b[2]]),
 *                               w[0] [16][cin][k][k], w[1] [8][cin][p+1][k] (rows 0..p of the k x k window), w[2] [8][cin][k][p+1]
 *                               (columns 0..p), b of 16, 8 and 8 values
 *      In both forms y[n][co][yy][xx] reads x[n][ci][yy + dy][xx + dx]; y and g_y are f32 [n][32][h][w], dense.  The split form is
 *      ONE k x k convolution with 32 outputs whose smaller kernels are zero-padded (stem_train.hip); taps outside a kernel's support
 *      are not part of g_w.
 *      BACKWARD: gm = g_y where y > 0, else 0 (torch's mask rule); g_w[j], g_b[j] have the shapes of w[j], b[j]; g_x [n][cin][h+p][w+p]
 *      is optional: NULL = not computed, nothing written.  Every element of every requested output is written.  The weight and bias
 *      gradients are a two-stage reduction whose order depends on the shape only, the input gradient a fixed chain per element: no
 *      atomics, the same bits on every run, stream and context.  Non-finite values: NON-FINITE VALUES IN THE TRAINING CALLS, above.
 *      SHAPES: n 1..256; h and w multiples of 16 in 16..256; cin 1..4; k 5 or 9; split 0 or 1.  d_w, d_b, d_g_w, d_g_b are HOST arrays
 *      of three device pointers; entries 1 and 2 are non-NULL exactly when split = 1.
 *      PMP_E_INVALID before any launch, nothing written: a NULL or unsupported shape, a missing tensor or array, entries 1 and 2
 *      against the rule, an output that overlaps an input or another output, a pointer that is not 4-byte aligned.
 *      Like pmp_trunk_*_device the calls first SETTLE the context's calls in flight and run stream-ordered on its stream, always on
 *      the exact fp32 MFMA datapath; packed weights and partial sums live in the activation workspace. ---- */
typedef struct pmp_stem_shape {
    int n, h, w, cin, k, split;
} pmp_stem_shape;
int pmp_stem_forward_device(pmp_ctx *ctx, const pmp_stem_shape *shape, const float *d_x, const float *const d_w[3],
                            const float *const d_b[3], float *d_y);
int pmp_stem_backward_device(pmp_ctx *ctx, const pmp_stem_shape *shape, const float *d_x, const float *d_y, const float *const d_w[3],
                             const float *d_g_y, float *d_g_x /* may be NULL */, float *const d_g_w[3], float *const d_g_b[3]);

/* ---- training: an MTT net's HEAD - conv_B1..3 (8 -> 2, 3x3, padding 1, bias), the carry out_k[:,0] += out_{k-1}[:,0] and the next
 *      attention trunk's input cat[interpolate(x1), interpolate(out)] (Model_QBD.py:139-153, :237-251) - forward and backward
 *      (head_train.hip).  All tensors dense NCHW f32.
 *      FORWARD.  x [n][cin][h][w], w [cout][cin][3][3], b [cout]; one element of y [n][cout][h][w]:
 *        acc = +0; acc = fma(w[co][ci][dy][dx], x[n][ci][yy+dy-1][xx+dx-1], acc) for ci = 0..cin-1, inside that dy = 0..2, inside that
 *        dx = 0..2 (an x outside the map enters as +0); y = acc + b[co]; then, if d_prev [n][cout][h][w] is given and co = 0,
 *        y = y + prev[n][0][yy][xx] - the carry, added behind the bias as the reference adds it.  Channels 1.. of prev are not read.
 *        If up_y != 0, att [n][1+cout][up_y h][up_y w] is written in the same pass from the CARRIED y:
 *        att[n][0][Y][X] = q[n][0][Y / up_q][X / up_q], att[n][1+co][Y][X] = y[n][co][Y / up_y][X / up_y]  (nearest, the reference's
 *        F.interpolate), q [n][1][up_y h / up_q][up_y w / up_q].  d_q and d_att are passed exactly when up_y != 0.
 *      BACKWARD.  g_y [n][cout][h][w] is the gradient that reaches the carried y from everywhere but att (the loss, and the next
 *        head's carry); g_att [n][1+cout][up_y h][up_y w] is passed exactly when up_y != 0.  The effective gradient of the carried y:
 *        gy = g_y, then gy = gy + g_att[n][1+co][up_y yy + i][up_y xx + j] for (i, j) = (0,0), (0,1), (1,0), (1,1) in that order
 *        (up_y = 1: the one element).
 *        g_x [n][cin][h][w] (optional): acc = +0; acc = fma(w[co][ci][dy][dx], gy[n][co][yy+1-dy][xx+1-dx], acc) for co, inside that
 *        dy, inside that dx (a gy outside the map enters as +0).
 *        g_w [cout][cin][3][3] and g_b [cout], two stages: the ITEMS are the 8x8 tiles of the maps, item = (n * h/8 + ty) * w/8 + tx;
 *        NP = min(ceil(items / 2), 128) partitions, a function of the shape only; partition p starts from +0 and adds the items p,
 *        p + NP, ... in that order, each pixel by pixel in row order, acc = fma(gy, x, acc) (g_b: acc = acc + gy); then
 *        s = partial 0, s = s + partial p for p = 1 .. NP-1.  No atomics: the same bits on every run, stream and context.
 *        g_q [n][1][up_y h / up_q][up_y w / up_q] (optional, only with g_att): s = +0, then s = s + g_att[n][0][up_q Y + i][up_q X + j]
 *        over the window in row-major order.
 *        g_prev [n][cout][h][w] (optional): the carry's gradient, g_prev[:,0] = gy[:,0] and +0 in the other channels.  Where up_y = 0
 *        that is g_y[:,0] and a caller needs no copy of it; with an attention input (conv_B2) the window sums of g_att belong to it.
 *      SHAPES: n 1..256; h and w multiples of 8 in 8..256; cin 1..16; cout 1 or 2 (conv_q2 has 1); (up_q, up_y) = (0,0): no attention
 *      input, or (2,1) or (4,2), the two pairs the nets use.
 *      PMP_E_INVALID before any launch, nothing written: a NULL or unsupported shape, a missing tensor, q / att / g_att against the
 *      rule, g_q without g_att, an output that overlaps an input or another output, a pointer that is not 4-byte aligned.  Every
 *      element of every requested output is written.  Settles the context's calls in flight, then runs stream-ordered on its stream;
 *      the partial sums live in the activation workspace.  Non-finite values: NON-FINITE VALUES IN THE TRAINING CALLS, above - a
 *      head is a convolution, a carry, copies and window sums, a gate a product: no ReLU, no maximum, nothing masked or routed. ---- */
typedef struct pmp_head_shape {
    int n, h, w, cin, cout, up_q, up_y;
} pmp_head_shape;
int pmp_head_forward_device(pmp_ctx *ctx, const pmp_head_shape *shape, const float *d_x, const float *d_w, const float *d_b,
                            const float *d_prev /* may be NULL */, const float *d_q, float *d_y, float *d_att);
int pmp_head_backward_device(pmp_ctx *ctx, const pmp_head_shape *shape, const float *d_x, const float *d_w, const float *d_g_y,
                             const float *d_g_att, float *d_g_x /* may be NULL */, float *d_g_w, float *d_g_b,
                             float *d_g_q /* may be NULL */, float *d_g_prev /* may be NULL */);

/* ---- training: the GATE product of an attention trunk, xb = x * a (Model_QBD.py:143, :150), over count floats (1 .. 2^31 - 1).
 *      forward:  y = x * a
 *      backward: g_a = g_y * x;  g_x = g_y * a, or with d_g_acc (the gradient x already has from its other reader, trunk_M2 or
 *                trunk_B1) g_x = g_acc + g_y * a: the product rounded, then the sum rounded - torch's mul and add, bit for bit.
 *      16-byte accesses when every pointer of the call is 16-byte aligned, scalar ones otherwise.  PMP_E_INVALID before any launch
 *      as above (count out of range, a missing tensor, an output over an input or another output, a misaligned pointer). ---- */
int pmp_gate_forward_device(pmp_ctx *ctx, int64_t count, const float *d_x, const float *d_a, float *d_y);
int pmp_gate_backward_device(pmp_ctx *ctx, int64_t count, const float *d_x, const float *d_a, const float *d_g_y,
                             const float *d_g_acc /* may be NULL */, float *d_g_x, float *d_g_a);

/* ---- training: a QT net's TAIL - everything of Luma_Q_Net / Chroma_Q_Net behind its second pool except the head conv_q2
 *      (Model_QBD.py:83-90, :181-188), forward and backward, as one call (qtail_train.hip, api_train.cpp):
 *        x5 = resblock_q3(x4)                                     64 -> 32, 3x3, 1x1 shortcut
 *        x6 = cat[x5, up2(mp2(x5)), up4(mp4(x5)), up8(mp8(x5))]   32 -> 128: x6[:, 0:32] = x5 and, for s = 2, 4, 8,
 *                                                                 x6[:, 32 log2(s) + c][y][x] = max of x5[c] over the s x s window, aligned
 *                                                                 to multiples of s, that holds (y, x)
 *        x7 = resblock_q4(x6)                                     128 -> 32, 3x3, 1x1 shortcut
 *        x8 = max_pool2d(resblock_q5(x7), 2)                      32 -> 32, identity shortcut, then h/2 x w/2
 *        x9 = resblock_q6(x8)                                     32 -> 8, 3x3, 1x1 shortcut, on the h/2 x w/2 map
 *      TENSORS (device pointers, dense NCHW fp32): x4, g_x4 [n][64][h][w]; x9, g_x9 [n][8][h/2][w/2]; d_w and d_g_w are HOST arrays of
 *      12 device pointers - w0, w2, wsc of q3, q4, q5, q6 in pmp_trunk_*'s layouts ([32][64][3][3], [32][32][3][3], [32][64]; [32][128][3][3],
 *      [32][32][3][3], [32][128]; [32][32][3][3] twice, NULL; [8][32][3][3], [8][8][3][3], [8][32]) - with the trunk's NULL rule: q5's wsc
 *      and g_wsc NULL, the other three present.  SHAPES: n 1..256; h and w multiples of 16 in 16..256 (the nets: 16 x 16).
 *      d_saved: pmp_qtail_saved_bytes(shape) bytes the caller owns, 16-byte aligned, OPAQUE: the blocked x4 and t, out of q3, q4, q5 and
 *      q6.  x6 and x8 are NOT saved: backward rebuilds them from x5 and q5's out, bit for bit (a maximum has no rounding).  At n = 200,
 *      16 x 16: 58 982 400 bytes (x6 would add 26 214 400).  Forward writes every byte backward or unpack reads; they only read it.
 *      pmp_qtail_unpack_device: index 0 = x4; 1, 2 = t, out of q3 (out = x5); 3, 4 = of q4; 5, 6 = of q5 (un-pooled); 7, 8 = of q6
 *      ([n][8][h/2][w/2]; out = x9), in torch's dense layout.
 *      ARITHMETIC: always the exact fp32 MFMA datapath.  q3, q4 and q5 are pmp_resblock_forward's block - its formulas, and backward its
 *      six steps in its order; the forward results of q3 and q5 are pmp_resblock_forward_device's bit for bit.  q4 reads its 128 inputs
 *      as eight channel groups through the same convolution kernel; its weight gradients g_w0 and g_wsc follow conv_wgrad.hip's
 *      two-stage order with Ca = 128: eight channel groups, NP = min(ceil(items / 2), 32) partitions of the items (n, 16x16 tile).  Its
 *      data gradient g6 [n][128][h][w] is two convolutions of 64 outputs each (channels 0..63 and 64..127), every element the chain
 *      pmp_resblock_backward's g_x has.
 *      q6: the h/2 x w/2 map lies in the top-left corner of a map of h2 x w2 = the sides rounded up to multiples of 16 whose other
 *      pixels are +0, and the block runs on that map through the SAME kernels as the other three: a pixel outside the h/2 x w/2
 *      region enters every convolution as the zero that torch's padding is.  Forward, t and out are multiplied by the region's 0/1
 *      mask behind their ReLU; backward needs no mask (gu and gt are zero outside the region through `out > 0` and `t > 0`).  Per
 *      element inside the region the chains are therefore pmp_resblock_*'s chains of an h/2 x w/2 map; the weight gradients are
 *      reduced over the items (n, 16x16 tile of the h2 x w2 map) with the order above (NP from those items), the added products
 *      being exact zeros.
 *      q5's POOL and its backward follow pmp_trunk_*'s rule: the gradient of a 2x2 window goes to its first maximum in the order (0,0),
 *      (0,1), (1,0), (1,1) where q5's out > 0, recomputed from the saved un-pooled out, no index tensor.
 *      MULTI-SCALE POOL, BACKWARD.  One element of g_x5 [n][32][h][w], from g6:  g = g6[c], then g = g + r2, g = g + r4, g = g + r8 in
 *      that order.  r_s = +0 unless (y, x) is the FIRST maximum of x5[c] over its whole s x s window in row-major order (torch's
 *      max_pool2d rule, `val > maxval` replaces - not the argmax of a hierarchy of 2x2 maxima, which differs on ties); for that pixel
 *      r_s starts from +0 and adds g6[32 log2(s) + c] over the window in row-major order.  q3's upstream gradient is g where
 *      x5 > 0, else +0.
 *      BACKWARD walks q6, the pool, q5, q4, the multi-scale pool, q3.  d_g_x4 may be NULL: q3's data gradient is then not computed
 *      and nothing is written for it.  Every byte of every requested output is written.  No atomics anywhere: the same bits on every
 *      run, stream and context.  Non-finite values: NON-FINITE VALUES IN THE TRAINING CALLS, above.
 *      PMP_E_INVALID before any launch, nothing written: a NULL or unsupported shape; a missing tensor or array; a NULL pattern of d_w
 *      or d_g_w against the rule; an output that overlaps an input or another output (d_saved is an output of forward and an input of
 *      backward and unpack); a pointer that is not 4-byte aligned (d_saved: 16-byte); an unpack index outside 0..8.
 *      pmp_qtail_saved_bytes returns PMP_E_INVALID (< 0) for such a shape; it needs no context and no GPU.
 *      Like pmp_trunk_*_device the calls first SETTLE the context's calls in flight and run stream-ordered on its stream; x6, x8, the
 *      running gradient and one block's working set live in the activation workspace. ---- */
typedef struct pmp_qtail_shape {
    int n, h, w;
} pmp_qtail_shape;
int64_t pmp_qtail_saved_bytes(const pmp_qtail_shape *shape);
int pmp_qtail_forward_device(pmp_ctx *ctx, const pmp_qtail_shape *shape, const float *d_x4, const float *const *d_w, void *d_saved,
                             float *d_x9);
int pmp_qtail_backward_device(pmp_ctx *ctx, const pmp_qtail_shape *shape, const void *d_saved, const float *const *d_w,
                              const float *d_g_x9, float *d_g_x4 /* may be NULL */, float *const *d_g_w);
int pmp_qtail_unpack_device(pmp_ctx *ctx, const pmp_qtail_shape *shape, const void *d_saved, int index, float *d_dense);

/* ---- TRAINING STEP: what a training loop runs around the nets and the loss - a batch assembled on the device from a data set that
 *      stays there as the label files hold it, and Adam over every parameter of a step (train_step.hip).  One launch each.
 *
 *      pmp_batch_gather_device.  src: the WHOLE set, device pointers to the bytes of Load_Pre_VP_Dataset's .npy files (Metrics.py:64-146)
 *      and count = N >= 1 blocks: y u8[N][68][68]; u, v u8[N][34][34], both given = a chroma set, both NULL = luma; qt8 u8[N][8][8] (raw
 *      qtDepth), msbt u8[N][3][16][16], msdire i8[N][3][16][16], each of the three NULL where the set has none.  d_index i64[n]: the rows
 *      of the batch, in the batch's order; a row may repeat.  dst: the batch, each NULL where it is not asked for:
 *        x      luma   f32[n][1][68][68] = float(y)
 *               chroma f32[n][3][34][34]: channel 0 [r][c] = float(max(y[2r][2c], y[2r][2c+1], y[2r+1][2c], y[2r+1][2c+1])) - F.max_pool2d(y, 2),
 *                      Metrics.py:85 - channel 1 = float(u), channel 2 = float(v)
 *        qt_f   f32[n][1][8][8] = float((uint8)(qt8 - 1)): the loader's `np.load(...) - 1` in uint8, a raw 0 becoming 255.0 as in pmp_val_stats
 *        qt8, msbt, msdire     the raw label rows (u8[n][8][8], u8[n][3][16][16], i8[n][3][16][16]), as pmp_train_loss_device reads them
 *      Every value is an integer of at most 255: exact.  Every byte of every requested output row is written.
 *      INDICES OUTSIDE [0, N) are never dereferenced: the rows of such an index are written as zeros (+0.0, 0) in every requested output and
 *      bit 0 of *d_status is set with an atomic OR.  Nothing else ever writes *d_status: the caller zeroes it once and reads it when
 *      it likes (once an epoch, say).
 *      ALIGNMENT: every pointer of src and dst and d_status 4-byte aligned, d_index 8-byte; no more is assumed (rows of 4624 and 1156
 *      bytes keep 4-byte alignment and nothing better): 4-byte loads, and 16-byte stores only where a call's output rows happen to allow them.
 *      ORDER: no atomics but the status bit, no sums: the same bits on every run, stream and context.
 *      PMP_E_INVALID before any launch, nothing written: NULL src, dst, d_index or d_status; count < 1; n outside 1..65536; y NULL; one of
 *      u, v without the other; no output asked for; an output whose source is NULL; a pointer not aligned as above; an output that
 *      overlaps the set, the index, the status word or another output.
 *      Stream-ordered on the context's stream, the host does not wait; like the other training calls it first SETTLES the context's
 *      calls in flight.
 *
 *      pmp_adam_step_device.  torch.optim.Adam without weight decay and without amsgrad, step number `step` >= 1, over ntensors tensors
 *      in one launch.  param, grad, m, v and count are HOST arrays [ntensors] of device pointers (float32, 4-byte aligned) and of element
 *      counts, like d_w of pmp_stem_*.  On the host, in double:
 *        c1 = 1 - beta1^step      c2 = 1 - beta2^step      a = lr / c1      r = sqrt(c2)
 *      and d1 = float(1 - beta1), b2 = float(beta2), d2 = float(1 - beta2), af = float(a), rf = float(r), ef = float(eps).
 *      Per element in float32, fma(a, b, c) = a*b + c rounded once, every other operation rounded on its own, sqrt and the divisions
 *      correctly rounded, in this order:
 *        m = fma(d1, g - m, m)          v = fma(d2*g, g, b2*v)          param = param + ((-af)*m) / (sqrt(v)/rf + ef)
 *      which is  m = beta1*m + (1-beta1)*g;  v = beta2*v + (1-beta2)*g*g;  param -= (lr/(1-beta1^step)) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)
 *      in the order of operations of torch's float32 CPU kernels (lerp_, mul_ and addcmul_, addcdiv_): on an x86 host with FMA it gave
 *      their bits on all but a few elements in a million (those kernels' own bits differ from one CPU to another).
 *      Elements are independent: a NaN or an inf in g makes that element's m, v and param what the formula gives (NaN g: all three NaN;
 *      +-inf g: m = +-inf, v = +inf, param NaN - torch's float32 CPU Adam gives the same) and touches no other element.
 *      LAUNCHES: the tensors' pointers travel in the kernel's argument block, PMP_ADAM_TABLE entries to a launch - the 92 tensors of the luma
 *      joint step are one launch; more tensors (and tensors of 2^30 elements or more, which take an entry per 2^30) go in the fewest
 *      launches that hold them, in the order given.  Nothing is staged, allocated or waited for: a call costs its launches.
 *      PMP_E_INVALID before anything is launched or written, with a message in pmp_last_error: ntensors < 1; a NULL p or array; a NULL
 *      entry or one not 4-byte aligned; a count < 1; step < 1; lr, beta1, beta2 or eps not finite; a beta outside [0, 1); eps <= 0; two
 *      tensors of the call (any two of the 4*ntensors) overlapping in memory.
 *      ORDER: no atomics, no sums: the same bits on every run, stream and context.  Stream-ordered, settles first, as above.
 *
 *      GRADIENT BUCKETS, for data-parallel training whose result is defined bit for bit (grad_sync.py): every rank packs its gradients
 *      into one bucket, the buckets are gathered, and every rank adds them IN RANK ORDER with a kernel of this library - not with an
 *      all-reduce, whose order of additions belongs to the communication library.
 *      pmp_grad_bucket_floats.  Host only, no context, no GPU.  The bucket of ntensors tensors of count[i] floats: the tensors in the
 *      order given, tensor i at offset[i] floats, every offset a multiple of 4 (16 bytes), offset[0] = 0, offset[i+1] = offset[i] +
 *      count[i] rounded up to a multiple of 4.  Returns the bucket's floats, a multiple of 4, and, where offset is not NULL, the
 *      offsets; -1 for ntensors < 1, a NULL count, a count < 1 or a count >= 2^30.
 *      pmp_grad_pack_device.  grad and count are HOST arrays [ntensors], as Adam's: device pointers (float32, 4-byte aligned) and element
 *      counts.  d_bucket (16-byte aligned, pmp_grad_bucket_floats floats) receives tensor i at offset[i]; a NULL grad[i] stands for a
 *      parameter without a gradient, whose slice is written as +0.0, and so are the padding floats: EVERY float of the bucket is
 *      written.  The pointers travel in the kernel's argument block, PMP_ADAM_TABLE entries to a launch, in the fewest launches that
 *      hold them; nothing is staged or allocated.  16-byte stores, 16-byte loads where a gradient's pointer allows them.
 *      PMP_E_INVALID: a bad table (as above), a NULL array or bucket, a gradient not 4-byte or a bucket not 16-byte aligned, a gradient
 *      that overlaps the bucket.
 *      pmp_grad_sum_device.  d_src is a HOST array of nsrc in 1..PMP_GRAD_SUM_MAX device pointers, each to count floats; count >= 4 and
 *      a multiple of 4, every pointer 16-byte aligned.  d_dst[i] = ((d_src[0][i] + d_src[1][i]) + d_src[2][i]) + ...: float32
 *      additions, each rounded on its own, in the order of d_src; no atomics, nothing the compiler may reassociate (no fast-math flag in
 *      this library's build).  nsrc = 1 is a copy, or nothing at all where d_dst == d_src[0].  d_dst may be EXACTLY d_src[0] (the
 *      sum in place); otherwise it overlaps no source.  The sources may alias one another.  x + 0.0 is not x for x = -0.0: a caller
 *      leaves out what it does not mean to add.  NaN and inf propagate as float32 addition propagates them.
 *      PMP_E_INVALID: nsrc outside 1..64, a NULL array, entry or d_dst, count < 4 or no multiple of 4, a pointer not 16-byte aligned,
 *      d_dst over a source other than as d_src[0] itself.
 *      Both device calls: PMP_E_INVALID before any launch, with a message; stream-ordered on the context's stream, settle first; the
 *      same bits on every run, stream and context.
 *
 *      THE DIVERGENCE GUARD: the global norm and the non-finite census of a step's gradients, and an Adam step that takes its orders
 *      from that result in device memory - clipping by global norm and skipping a step with a NaN or inf gradient, the host out of the loop.
 *      pmp_grad_guard_scratch_bytes.  Host only, no context, no GPU: the bytes of d_scratch for this table, 16 per tile (below); -1 for
 *      ntensors < 1, a NULL count, a count < 1 or a count >= 2^30.
 *      pmp_grad_guard_device.  grad and count are HOST arrays [ntensors], as Adam's: device pointers (float32, 4-byte aligned; 16-byte
 *      loads where a pointer allows them) and element counts in 1 .. 2^30 - 1.  PMP_ADAM_TABLE entries to a launch, in the fewest launches
 *      that hold them, in the order given, then ONE more launch of one workgroup: two launches for a step of up to 96 tensors.  No
 *      atomics.  The gradients are read only.  THE CENSUS:
 *        sumsq      the float64 sum of double(g) * double(g) over every FINITE element; each square is exact in double
 *        nonfinite  the int64 count of the elements that are NaN or +-inf; these add nothing to sumsq
 *      THE ORDER OF THE CENSUS is part of the interface (the same bits whatever wrote the gradients, on every run, stream and context,
 *      on one rank and on many):  tensor i is cut into tiles of 4096 elements; tiles are numbered through the tensors in the order given,
 *      on across the launches.  In a tile, lane l of 256 adds the squares of its elements l, l + 256, ... , l + 256*15 that exist, in
 *      ascending order, from +0.0.  Then a[l] += a[l + h] for l < h, with h = 128, 64, ... , 1; a[0] is the tile's partial and goes to
 *      d_scratch, of which every word is written before it is read (what it held before does not matter).  The last launch is one
 *      workgroup: lane l adds the partials l, l + 256, ... in ascending order from +0.0, and the same tree follows.  Any implementation
 *      that gives exactly these bits is this interface; the pairing is what is fixed.
 *      THE RECORD, finished in double by that last launch and written to d_record by one lane with ordinary stores:
 *        norm = sqrt(sumsq), correctly rounded          c = max_norm / (norm + 1e-6)
 *        coef = max_norm > 0 && c < 1 ? (float)c : 1.0f         (torch.nn.utils.clip_grad_norm_'s rule; max_norm 0: no clipping)
 *        action bit 1 (clip) is set when coef < 1;  action bit 0 (skip) is set when skip_nonfinite && nonfinite > 0
 *      THE RUNNING COUNTERS, d_state, optional (NULL: none).  Only this call writes them, in stream order; the caller zeroes them once.
 *      Per call: steps += 1;  with the skip bit: skipped += 1, run += 1, max_run = max(max_run, run);  otherwise run = 0 and, with the
 *      clip bit, clipped += 1.  run is the number of skipped steps in a row.  max_norm = max(max_norm, norm) at every call: the norm of the
 *      finite part, which is finite.
 *      PMP_E_INVALID before any launch, nothing written: NULL p, grad, count, d_scratch or d_record; a bad table (as
 *      pmp_grad_guard_scratch_bytes); a NULL entry or one not 4-byte aligned; max_norm negative or not finite; d_scratch, d_record or
 *      d_state not 8-byte aligned; d_scratch, d_record or d_state overlapping a gradient or one another.
 *      pmp_adam_step_guarded_device.  pmp_adam_step_device's arithmetic to the letter and its launches, but every thread reads coef
 *      and action from d_record (device memory, as pmp_grad_guard_device wrote it earlier on the stream).  With the skip bit set it
 *      writes NOTHING: param, m and v keep their bits.  Otherwise g' = g * coef stands where g stood: one rounded float32 multiply, and
 *      no multiply at all where coef == 1.0f.  The caller's gradients are not modified.  The host computes af, rf and the rest from
 *      `step` as above.  A SKIPPED STEP STILL COUNTS AS A STEP: the caller passes the next step number at the next call, whatever the
 *      record said.  torch's GradScaler, which skips optimizer.step() and leaves the step number alone, does otherwise; counting keeps the
 *      host out of the loop (it never has to read the record) and keeps a torch.optim.Adam state's host-side `step` interchangeable.
 *      PMP_E_INVALID: what pmp_adam_step_device refuses; a NULL d_record or one not 8-byte aligned; d_record overlapping any of the
 *      4*ntensors tensors.
 *      Both device calls: stream-ordered on the context's stream, settle first; the same bits on every run, stream and context. ---- */
typedef struct pmp_guard_params {
    double max_norm;                   /* 0: no clipping */
    int skip_nonfinite;
} pmp_guard_params;
typedef struct pmp_guard_record {
    double sumsq, norm;
    int64_t nonfinite;
    float coef;
    uint32_t action;                   /* bit 0: skip, bit 1: clip */
} pmp_guard_record;
typedef struct pmp_guard_state {
    int64_t steps, skipped, clipped, run, max_run;
    double max_norm;
} pmp_guard_state;
typedef struct pmp_batch_src {
    const uint8_t *y, *u, *v, *qt8, *msbt;
    const int8_t *msdire;
    int64_t count;
} pmp_batch_src;
typedef struct pmp_batch_dst {
    float *x, *qt_f;
    uint8_t *qt8, *msbt;
    int8_t *msdire;
} pmp_batch_dst;
typedef struct pmp_adam_params {
    double lr, beta1, beta2, eps;      /* torch.optim.Adam's defaults: 1e-3, 0.9, 0.999, 1e-8 */
} pmp_adam_params;
#define PMP_BATCH_MAX 65536
#define PMP_ADAM_TABLE 96
int pmp_batch_gather_device(pmp_ctx *ctx, const pmp_batch_src *src, const int64_t *d_index, int64_t n, const pmp_batch_dst *dst,
                            int32_t *d_status);
int pmp_adam_step_device(pmp_ctx *ctx, const pmp_adam_params *p, int ntensors, float *const *param, const float *const *grad,
                         float *const *m, float *const *v, const int64_t *count, int64_t step);
int64_t pmp_grad_guard_scratch_bytes(int ntensors, const int64_t *count);
int pmp_grad_guard_device(pmp_ctx *ctx, const pmp_guard_params *p, int ntensors, const float *const *grad, const int64_t *count,
                          void *d_scratch, pmp_guard_record *d_record, pmp_guard_state *d_state /* may be NULL */);
int pmp_adam_step_guarded_device(pmp_ctx *ctx, const pmp_adam_params *p, int ntensors, float *const *param, const float *const *grad,
                                 float *const *m, float *const *v, const int64_t *count, int64_t step, const pmp_guard_record *d_record);
#define PMP_GRAD_SUM_MAX 64
int64_t pmp_grad_bucket_floats(int ntensors, const int64_t *count, int64_t *offset /* [ntensors], may be NULL */);
int pmp_grad_pack_device(pmp_ctx *ctx, int ntensors, const float *const *grad, const int64_t *count, float *d_bucket);
int pmp_grad_sum_device(pmp_ctx *ctx, int nsrc, const float *const *d_src, int64_t count, float *d_dst);

/* ---- DATA SET ASSEMBLY: a training set put together on the device (dataset.hip; python -m pmp_vvc_tip2023_amd.make_dataset).  Behind
 *      pmp_cut_blocks_device and pmp_msbt_labels_device every array of a set is on the device, row i of each belonging to block i.  The
 *      rows the set keeps are chosen ONCE, as one index, and every array is gathered by that index: blocks and labels cannot disagree.
 *
 *      pmp_select_rows_device.  d_flags: a HOST array of nflags device pointers, each u8[n] (the status arrays of pmp_msbt_labels, one
 *      per (component, QP)).  Row i is a CANDIDATE iff (d_flags[k][i] & mask) == 0 for every k; nflags = 0 (d_flags may be NULL then)
 *      makes every row one.  d_seg_end i64[nseg] cuts the rows into segments, one sequence each: segment s is rows
 *      [d_seg_end[s-1], d_seg_end[s]) (from 0 for s = 0); ascending, the last entry n, empty segments allowed.  A candidate is KEPT iff
 *      cap == 0 or fewer than cap candidates precede it in its segment.
 *        d_index i64[n]        [0, m) the kept rows in ascending order, [m, n) = -1; every element is written
 *        d_count i64[nseg+1]   [s] the rows kept of segment s, [nseg] = m
 *      The entries of d_seg_end live on the device and are not looked at by the host: an entry is used as clamped into 0..n and never
 *      below an earlier one, and the last as n, so no entry, whatever it holds, makes an access leave the arrays (d_count then counts
 *      the segments so clamped).
 *      LIMITS: n in 1..2^30, nseg in 1..65536, nflags in 0..PMP_SELECT_MAX_FLAGS, mask in 1..255, cap >= 0.  d_seg_end, d_index and
 *      d_count 8-byte aligned.
 *      ORDER: a prefix sum of fixed shape (candidates per 1024 rows, one workgroup's scan of those counts, a scatter) - no atomics, no
 *      workgroup waits for another: the same bits on every run, stream and context.  Scratch of n/256 + 12 nseg bytes is the context's.
 *
 *      pmp_gather_rows_device.  Row j of d_dst is row d_index[j] of d_src (nsrc rows), row_bytes bytes each, for j in [0, m); a row may
 *      repeat.  An index outside [0, nsrc) - the -1 tail of d_index included - is never dereferenced: its row is written as zeros and bit
 *      0 of *d_status is set with an atomic OR, the call's only atomic; nothing else writes *d_status (the caller zeroes it once).
 *      LIMITS: row_bytes a multiple of 4 in 4..65536 (a set's rows: 64, 256, 768, 1156, 4624), m in 1..2^30, nsrc >= 1.  d_src, d_dst
 *      and d_status 4-byte aligned, d_index 8-byte; no more is assumed, and 16-byte accesses are used only where d_src, d_dst and
 *      row_bytes are all multiples of 16.
 *
 *      BOTH: PMP_E_INVALID before any launch, nothing written, with a message in pmp_last_error: a NULL pointer (d_flags with nflags > 0,
 *      or one of its entries, included), a limit broken, a pointer not aligned as above, an output that overlaps an input or the other
 *      output.  Stream-ordered on the context's stream, the host does not wait; like the training calls they first SETTLE the context's
 *      calls in flight. ---- */
#define PMP_SELECT_MAX_FLAGS 64
int pmp_select_rows_device(pmp_ctx *ctx, const uint8_t *const *d_flags, int nflags, int mask, const int64_t *d_seg_end, int nseg,
                           int64_t cap, int64_t n, int64_t *d_index, int64_t *d_count);
int pmp_gather_rows_device(pmp_ctx *ctx, const void *d_src, int64_t nsrc, int64_t row_bytes, const int64_t *d_index, int64_t m,
                           void *d_dst, int32_t *d_status);

/* ---- teacher-forced MTT inference: the MTT net of (comp, qp) on the blocks with a GIVEN QT map instead of the QT net's output, what
 *      pre_validation predID 1 runs (Net(input_batch, qt_label_batch), Metrics.py:226).  qt_in f32[n][8][8] is read, never written
 *      (for the reference's validation: float(qt8 - 1) with the u8 wrap above).  Everything else is pmp_infer's: the context's datapath,
 *      overlap mode, chunking, the range guard (a re-run repeats the MTT net only, on the fp32 MFMA datapath) and the f16x3 activation
 *      scales - which belong to the (QT, MTT) PAIR, so both nets of (comp, qp) must be loaded (PMP_E_NOWEIGHTS otherwise).  With qt_in =
 *      the QT logits pmp_infer returns, bt and dire are pmp_infer's, bit for bit. ---- */
int pmp_infer_msbd(pmp_ctx *ctx, int comp, int qp, const uint8_t *block_y, const uint8_t *block_u, const uint8_t *block_v,
                   const float *qt_in, int64_t n, float *bt, float *dire);
int pmp_infer_msbd_device(pmp_ctx *ctx, int comp, int qp, const uint8_t *d_block_y, const uint8_t *d_block_u, const uint8_t *d_block_v,
                          const float *d_qt_in, int64_t n, float *d_bt, float *d_dire);

/* ---- partition dump of the patched VTM decoder (Save_Depth_fal, Lib/DecoderLib/DecLib.cpp:998-1050) -> CreateDataSet's label blocks
 *      (CreateDataSet.output_block_partition_map, CreateDataSet.py:188-264).  Host only: no context, no GPU.
 *      Lines "x y h w depth qtDepth btDepth mtDepth s0 .. s7" (non-negative decimal integers separated by single spaces, trailing
 *      whitespace allowed), and a line containing "frame" before each frame.  Split codes (UnitPartitioner.h): 2 BT-H, 3 BT-V, 4 TT-H,
 *      5 TT-V, 2000 none.  is_chroma multiplies the coordinates by 2.  Each CU paints qtDepth, btDepth and, per layer i = 0..2, the
 *      direction of s[qtDepth + i] into frame matrices of 4x4-pixel cells [frames][height/4][width/4], with numpy's clipping slices; an
 *      unknown split code keeps the PREVIOUS layer's direction (0 for layer 0) and is counted in *n_unknown (the reference prints
 *      "Error!!").  The QT matrix is down-sampled [::2, ::2].  Blocks are cut frame-major, row-major, right and bottom remainders dropped:
 *      n = frames * (height/64) * (width/64) blocks of qt8 u8[n][8][8] (raw qtDepth), bt16 u8[n][16][16], dire16 i8[n][3][16][16].
 *      PMP_E_INVALID, nothing written, where the reference would index wrongly or crash: more "frame" lines than frames, a CU line before
 *      the first one, a malformed line (wrong field count, a non-integer or negative field, qtDepth > 5: s[qtDepth + 2] must exist),
 *      a qtDepth or btDepth outside u8.  PMP_E_IO if the file cannot be read. ---- */
int pmp_read_depth_dump(const char *path, int frames, int height, int width, int is_chroma, uint8_t *qt8, uint8_t *bt16,
                        int8_t *dire16, int64_t *n_unknown);

/* ---- PartitionMat text file (Map2Partition.py:385-412): per frame hor, ver, qt, dire[3]; one decimal
 *      integer per line.  Host-side (file I/O); inputs are per-block arrays in block order. ---------------- */
int pmp_write_partition_file(const char *path, int frames, int height, int width, const uint8_t *hor,
                             const uint8_t *ver, const uint8_t *qt_u8, const int8_t *dire_i8);
/* Same bytes into memory: returns the byte count (or a negative error).  buf == NULL returns the exact size; a buffer of
 * exactly that size is enough (cap < size: PMP_E_INVALID, nothing beyond buf[cap-1] is ever written). */
int64_t pmp_format_partition_text(int frames, int height, int width, const uint8_t *hor, const uint8_t *ver,
                                  const uint8_t *qt_u8, const int8_t *dire_i8, char *buf, int64_t cap);

/* ---- sharded emission (the reference's serial tail is the per-value text emission, Map2Partition.py:401-412).
 *      Frames are self-contained in the file (Map2Partition.py:389-412) and inside a frame every section (hor, ver, qt, dire 0..2) is
 *      row-major, so a writer that holds `block_rows` consecutive BLOCK ROWS of one frame (block_rows * (width/64) blocks, row-major)
 *      owns six contiguous byte ranges of the file.  These two calls produce them back to back - section-major, i.e. exactly the
 *      text of a frame of height 64*block_rows - and report the exact size of every (block row, section) pair in
 *      row_section_bytes[block_rows][6] (may be NULL), from which the ranks derive their file offsets with one exclusive scan
 *      (pmp_vvc_tip2023_amd/parallel.py: section_offsets) and write concurrently with pwrite.  buf == NULL: sizes only; the return
 *      value is the total byte count.  The _records form reads packed PMP_RECORD_BYTES records, what the device path produces. ---- */
int64_t pmp_format_partition_rows(int width, int block_rows, const uint8_t *hor, const uint8_t *ver, const uint8_t *qt_u8,
                                  const int8_t *dire_i8, char *buf, int64_t cap, int64_t *row_section_bytes);
int64_t pmp_format_partition_rows_records(int width, int block_rows, const uint8_t *rec, char *buf, int64_t cap,
                                          int64_t *row_section_bytes);
/* The same rows as matrices (binary side channel / in-process hand-over): hor, ver u8[16*block_rows][cols], qt u8[8*block_rows][cols/2],
 * dire i8[3][16*block_rows][cols], cols = 16*(width>>6). */
int pmp_tile_partition_rows_records(int width, int block_rows, const uint8_t *rec, uint8_t *out_hor, uint8_t *out_ver, uint8_t *out_qt,
                                    int8_t *out_dire);

/* ---- binary side channel.  Same content as the text file, laid out as the arrays the patched VTM keeps
 *      after parsing (Lib/CommonLib/Rom.h:240-248), so a consumer can mmap it instead of 645 k getline+stoi calls per frame:
 *        char magic[8] = "PMPB1\0\0\0"; int32 frames, height, width, rows (= 16*(H>>6)), cols (= 16*(W>>6)), reserved[3];
 *        then per frame:  u8 hor[rows][cols] | u8 ver[rows][cols] | u8 qt[rows/2][cols/2] | i8 dire[3][rows][cols]
 *      (frame matrices, already tiled from the per-block arrays; little-endian; 40-byte header). ---- */
int pmp_write_partition_binary(const char *path, int frames, int height, int width, const uint8_t *hor, const uint8_t *ver,
                               const uint8_t *qt_u8, const int8_t *dire_i8);

/* ---- in-process hand-over: the same frame matrices straight into caller memory, in the shapes the
 *      patched VTM allocates in EncAppCfg::parsePartitionMatrix (EncAppCfg.cpp:4270-4298; Rom.h:240-248), one component:
 *        hor, ver: u8[frames][rows][cols]   qt: u8[frames][rows/2][cols/2]   dire: i8[frames][3][rows][cols]
 *      with rows = 16*(height>>6), cols = 16*(width>>6) (4x4 luma units of the picture cropped to multiples of 64).
 *      A hook that replaces the text parser copies (or points) partitionHorMat[f][comp] etc. at these rows. ---- */
int pmp_tile_partition_maps(int frames, int height, int width, const uint8_t *hor, const uint8_t *ver, const uint8_t *qt_u8,
                            const int8_t *dire_i8, uint8_t *out_hor, uint8_t *out_ver, uint8_t *out_qt, int8_t *out_dire);

/* ---- per-kernel-class timing with hipEvents on the launch stream (bench.py roofline leg). -------------- */
/* mask: bit i enables kernel class i (see pmp_ktime_name); 0 disables.  Resets the accumulators. */
int pmp_ktime_enable(pmp_ctx *ctx, uint32_t mask);
int pmp_ktime_classes(void);
const char *pmp_ktime_name(int cls);
/* Synchronises, then returns launches / total milliseconds / algorithmic FLOPs accumulated for the class. */
int pmp_ktime_get(pmp_ctx *ctx, int cls, int64_t *launches, double *ms, double *flops);

/* ---- measurement hook.  The product library ships ONE form of every convolution kernel - number 2 - and accepts nothing else
 *      here (PMP_E_INVALID): it has no process-wide kernel selector.  The forms that were built, parity-tested and measured slower
 *      than or equal to the shipped ones (1, 3..9; bit-identical results) and the timing-only builds (10 and above; WRONG results)
 *      exist only in the measurement library tools/abl/libpmp_hip_abl.so (`make -C tools/abl`), where this call selects them process-wide for
 *      in-process A/B timing (tools/conv_ab.py, tools/variants_agree.py; the list is in tools/abl/conv_f16x3.hip, the numbers in EXPERIMENTS.md). ---- */
int pmp_debug_set_conv_variant(int variant);

/* ---- measurement hook (f16x3 datapath): run the 3x3 64->64 convolutions - 55 % of the luma step - in the Winograd F(2,3)-along-x
 *      form (conv_f16x3_wx.hip: 1.5x fewer MFMAs, fp32-equivalent logits within the 1e-3 tolerance, not bit-identical to the direct
 *      form).  It did not beat the direct kernels (EXPERIMENTS.md, profiles/r03_notes.txt), so like the other forms that lost their
 *      A/B it exists in the measurement library tools/abl/libpmp_hip_abl.so only (`make -C tools/abl`; tools/wx_probe.py, tools/wx_ablate.py): the
 *      product library accepts on = 0 and answers PMP_E_INVALID to anything else. ---- */
int pmp_debug_set_winograd(pmp_ctx *ctx, int on);

/* ---- test / A-B hook (f16x3 datapath, per context): launch fusion.  on = 1 (default): (a) the 16x16-resolution tails of the nets - trunk_B1/B2 +
 *      heads + attention 1 of the MTT nets, resblock_q3 .. conv_q2 of the QT nets - run as two (QT) / three (MTT) launches per net with the activations of
 *      a ResidualBlock resident in LDS, two blocks per CU (chain16.hip), and (b) the ResidualBlocks with <= 32 output channels at 32x32 - trunk_B3.1, trunk_B3.2 (+ pool),
 *      trunk_Att2.0 of the MTT nets - as one launch per block with the intermediate in LDS (rbfuse32.hip).  on = 0: launch per layer, as the
 *      other two datapaths always do; on = 2: (a) only; on = 3: (b) only.  Results are BIT-IDENTICAL in all four settings
 *      (tests/test_gpu_parity.py::test_fused_16x16_tails_are_bit_identical); only the launch count (68 -> 40 per luma pass) and the time
 *      differ.  Settles the calls in flight first. ---- */
int pmp_debug_set_fusion(pmp_ctx *ctx, int on);

/* ---- test / diagnosis hook: the f16x3 activation scales of the MTT net of (comp, qp) (see "Activation scales" above) and the calibration
 *      record behind them.  Runs the calibration now if the pair has not been used on the f16x3 datapath yet (both nets must be loaded).
 *      exps[5]: the segment exponents; seg_amax[5]: the largest |value| seen in each segment on the calibration blocks (true scale);
 *      buf (may be NULL): one text line per recorded tensor, "<name> <segment> <max |value|>\n", in launch order ("<block>.t" is the
 *      intermediate of a ResidualBlock).  Returns the number of recorded tensors or a negative error. ---- */
int pmp_debug_activation_report(pmp_ctx *ctx, int comp, int qp, int exps[5], float seg_amax[5], char *buf, int64_t cap);
/* ---- test hook: on = 0 runs the f16x3 datapath with exponents of zero whatever the calibration chose (how the range-guard tests still
 *      drive activations out of the fp16 range: with the scales on, their power-of-two stress weights simply get larger exponents);
 *      on = 1 (default) uses the calibrated exponents.  Settles the calls in flight first. ---- */
int pmp_debug_set_activation_scales(pmp_ctx *ctx, int on);

/* ---- test hook: every intermediate tensor of an inference call, for layer-local checks against a float64 reference
 *      (oracle/layers64.py, tests/test_gpu_layers.py).  While taps are on (pmp_debug_set_taps(ctx, 1); 0 turns them off and frees
 *      their memory), every inference call records each tensor the graph produces, by a device-to-device copy on the context's stream
 *      right behind the launch that wrote it (so an identity-shortcut block that later overwrites its input in place cannot reach the
 *      copy).  Names carry the net: "q/stem", "q/resblock_q1.t" (a ResidualBlock's intermediate), "q/resblock_q1", "q/x6" (the
 *      multi-scale pool), "q/resblock_q3" (also inside the fused 16x16 tail), "bd/trunk_M1.3", "bd/att_input1", "bd/trunk_Att1.1"
 *      (also inside the fused tail), ...; a tensor that a fused kernel keeps in LDS has no tap.  Not recorded: the calibration pass of
 *      the activation scales, the arena's measuring pass, and the fp32 re-run of the range guard - a test that reads taps runs with the
 *      saturation policy at PMP_SAT_ERROR or PMP_SAT_IGNORE and checks that nothing saturated.  With taps on, an inference call must
 *      run as one pass of at most 64 blocks (n <= chunk) with overlap mode off: PMP_E_INVALID otherwise.
 *      pmp_debug_get_tap (settles the calls in flight) returns the tensor `name` of the last call as dense NCHW float64, padded channels
 *      included (dims = {n, C padded to 16, H, W}, *c_real = the real channel count), at true scale (the stored value times 2^e of its
 *      segment on f16x3 with activation scales) and exactly as the consuming kernel reads it: h0 + h1 (split-2), b0 + b1 + b2
 *      (split-3), the fp32 value - float64 holds these sums exactly.  Returns the element count (out == NULL or cap too small: nothing
 *      written) or a negative error (PMP_E_INVALID: no such tensor). ---- */
int pmp_debug_set_taps(pmp_ctx *ctx, int on);
int64_t pmp_debug_get_tap(pmp_ctx *ctx, const char *name, double *out, int64_t cap, int dims[4], int *c_real);

/* ---- test hook: poisoned workspaces.  pattern 1: before every pass, fill every activation workspace the context uses (its own, the
 *      second one of overlap mode, one taken over from a destroyed context - the whole buffer) with 0xFF bytes, a NaN in fp32, bf16 and
 *      fp16; pattern 2: with 0x3C bytes, a finite value (0.0115 in fp32, 1.06 in fp16): in the inference graph a ReLU is a hardware
 *      maximum, which returns 0 for a NaN, so in an inference pass a NaN that was read can vanish before it shows.  (The training calls
 *      carry a NaN through ReLU and pool - NON-FINITE VALUES IN THE TRAINING CALLS - so there pattern 1 shows it too.)
 *      The context's own logit buffers (fused entry points called without logit pointers, host-pointer entry points) are filled too
 *      before each call that uses them.  hipMemsetAsync on the context's streams, nothing else; 0 (default) turns it off.  A kernel that
 *      reads a byte it did not write shows up as a difference from an unpoisoned run (tests/test_gpu_layers.py).  Settles first. ---- */
int pmp_debug_poison_workspace(pmp_ctx *ctx, int pattern);

/* ---- test hook (host only, no GPU needed): the f16x3 weight packing of one OIHW conv tensor (conv_f16x3.hip).
 *      Writes the power-of-two exponent k of the scale S = 2^k to *scale_exp and, if out != NULL, the packed stream
 *      [K-step][2 splits][cout_pad/16][64 lanes][8] of fp16 bit patterns (h0, h1 with h0 + h1 ~= S*w) to out.
 *      Returns the number of uint16 elements of the stream (> cap: nothing written), or a negative error. ---- */
int64_t pmp_debug_pack_f16x3(const float *w, int cout, int cin, int k, uint16_t *out, int64_t cap, int *scale_exp);

/* ---- test hook (host only): parse a .pmpw container; reports its net id (-1 if unknown), QP, tensor count, payload floats
 *      and the sum of all tensor elements. ---- */
int pmp_debug_read_weights_file(const char *path, int *net_id, int *qp, int *ntensors, int64_t *nfloats, double *checksum);

/* ---- measurement hook: one convolution layer on random data, both datapaths.  Runs conv KxK Cin->Cout (+ReLU) on
 *      n blocks of HxW with the fp32-MFMA kernel and with the context's split kernel (f16x3 or bf16x6; bf16x6 if the
 *      context is in fp32 mode), `iters` timed launches each.
 *      Outputs: average milliseconds per launch and max |fp32 - split| / max |fp32| over the whole output. ---- */
int pmp_debug_conv_bench(pmp_ctx *ctx, int n, int h, int w, int cin, int cout, int k, int iters, double *ms_f32,
                         double *ms_x6, double *max_abs_diff, double *max_abs_ref);

/* ---- test hook: ONE ResidualBlock (Model_QBD.py:23-44) at any shape the convolution kernels support, through the product's own code:
 *      the loader's packing of its weights (the f16x3 scales, the second convolution and the 1x1 shortcut sharing one), the graph's
 *      conversion of the input to the datapath's split format, its dispatch, out_scale and exponent composition, its in-place store of
 *      an identity-shortcut block and its routing to the fused 32x32 kernel (pmp_debug_set_fusion) - on the context's datapath, in its
 *      poisoned workspace if pmp_debug_poison_workspace is on (oracle/conv_cases.py, tests/test_gpu_conv_sweep.py).
 *      The shortcut follows the loader: identity when cin == cout, a 1x1 convolution of the input otherwise.  exp_x / exp_gate / exp_out
 *      (f16x3 only, ignored elsewhere): the activation-scale exponents of the input (and of .t and an ungated output, which the graph
 *      keeps in the input's segment), of the gate and of a gated output.  Needs taps on (pmp_debug_set_taps); the call's taps are
 *      "x" and "gate" (as the kernels read them), "rb.t" (absent when a fused kernel keeps it in LDS) and "rb", read with pmp_debug_get_tap.
 *      x: [n][cin][h][w], w0: [cout][cin][k][k], w2: [cout][cout][k][k], wsc: [cout][cin] (cin != cout), gate: [n][cout][h][w] (gate
 *      != 0), host fp32 at true scale.  *saturated (may be NULL): the f16x3 range flag of this call (read and cleared).  kernels (may be
 *      NULL): the kernel instantiations the call launched, "name\n" each, e.g. "conv_h2_kernel<5,5,4,0,1>" (template arguments as
 *      integers).  PMP_E_INVALID before any launch for a shape the kernels do not support: cout not 16, 32 or 64, cin not a multiple
 *      of 16 in 16..256, k not 1, 3 or 5, h or w not a multiple of 16 in 16..256, n not in 1..64, pool together with a gate. ---- */
typedef struct pmp_rb_case {
    int n, h, w, cin, cout, k;
    int gate, pool, out_f32;                /* 0 / 1 */
    int exp_x, exp_gate, exp_out;
} pmp_rb_case;
int pmp_debug_run_resblock(pmp_ctx *ctx, const pmp_rb_case *cs, const float *x, const float *w0, const float *w2, const float *wsc,
                           const float *gate, int *saturated, char *kernels, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PMP_H */
