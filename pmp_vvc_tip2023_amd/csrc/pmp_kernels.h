// Internal launch interface between the host-side graph (nets.cpp and the C ABI: pmp_api.cpp, range_guard.cpp, api_labels.cpp, api_train.cpp, api_debug.cpp) and the HIP kernels.
//
// Activation layout in HBM ("blocked channels-last"):  act[n][c/16][y][x][c%16]  float32, channels padded to a
// multiple of 16 with zeros.  A 16-channel group of one tile row is contiguous (16 px * 64 B = 1 KiB), which is
// exactly what one wave loads or stores per instruction in the MFMA conv kernel (16 B per lane, 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pmp.h"         // pmp_loss_params (include/)
#include "abl_types.h"   // hooks/ in the product build (empty structs), abl/ in the measurement library

namespace pmp {

// pmp_debug_run_resblock: the convolution launchers name the instantiation they launch ("kernel<a,b,...>", template arguments as integers,
// -1 = absent) - host side, and a no-op unless that hook is collecting on this thread (api_debug.cpp).
void note_launch(const char *kernel, int t0, int t1, int t2, int t3 = -1, int t4 = -1);

// ReLU and maximum that CARRY a NaN, as torch's relu and max_pool2d do (include/pmp.h: NON-FINITE VALUES): the hardware maximum
// behind fmaxf returns the operand that is a number.  On numbers (infinities and signed zeros included) the result is fmaxf's, bit for
// bit; the compare and the select are what a NaN costs.  relu_nan(-inf) = +0, as torch's.
__device__ __forceinline__ float relu_nan(float v) { const float m = fmaxf(v, 0.f); return v != v ? v : m; }
// A ReLU's output lets its gradient through: out > 0, or out is NaN - torch's threshold_backward is `out <= 0 ? 0 : g`.  And the element
// of a pooled window that gets the gradient: torch's max_pool2d replaces its maximum on `val > max || isnan(val)`, so the LAST NaN of a
// window wins, and without a NaN the first maximum.
__device__ __forceinline__ bool relu_on(float out) { return !(out <= 0.f); }
__device__ __forceinline__ bool pool_takes(float v, float best) { return v > best || v != v; }
__device__ __forceinline__ float max_nan(float a, float b) { const float m = fmaxf(a, b); return __builtin_isunordered(a, b) ? __builtin_nanf("") : m; }

// ------------------------------------------------------------------------------------------------ conv (MFMA)
// out = epilogue( conv_KHxKW(x, w) [+ conv_1x1(x_sc, w_sc)] [+ res] ), stride 1, zero padding K/2.
// epilogue: optional ReLU, optional multiply by `gate`, optional 2x2 max-pool.  H, W multiples of 16;
// Cin, Csc, Cout multiples of 16 (Cout <= 64).  Weight packing: pack_conv_mfma() in weights_pack.cpp.
struct ConvMfmaArgs {
    const float *x;     // [N][Cin/16][H][W][16]
    const float *w;     // packed [Cin/16][KH*KW][Cout/16][64 lanes][4]
    const float *x_sc;  // optional second source for the 1x1 shortcut conv, [N][Csc/16][H][W][16]
    const float *w_sc;  // packed [Csc/16][1][Cout/16][64][4]
    const float *res;   // optional identity residual [N][Cout/16][H][W][16]
    const float *gate;  // optional gate (attention multiply), same shape as the un-pooled output
    float *out;         // [N][Cout/16][H(/2)][W(/2)][16]
    int N, H, W, Cin, Csc, Cout, KH, KW;
    int relu, pool;
    int nan;            // the ReLU carries a NaN (relu_nan): the training calls.  0, the inference graph: max(v, 0), which maps a NaN to 0
};
hipError_t launch_conv_mfma(hipStream_t s, const ConvMfmaArgs &a);

// ------------------------------------------------------------------------------------------------ conv (bf16 x 6)
// Same operation on "split-3" activations (three bf16 planes per tensor, conv_bf16x6.hip).  *_stride = elements between
// the planes of the respective tensor.  Output goes to split-3 planes (`out`) or, if out_f32 != nullptr, to a plain
// fp32 blocked tensor (for consumers that are not MFMA convs).
struct ConvX6Args {
    const unsigned short *x; size_t x_stride;
    const unsigned short *w;                 // packed [Cin/16][ceil(taps/2)][3 splits][Cout/16][64 lanes][8 bf16]
    const unsigned short *x_sc; size_t sc_stride; const unsigned short *w_sc;
    const unsigned short *res; size_t res_stride;
    const unsigned short *gate; size_t gate_stride;
    unsigned short *out; size_t out_stride;
    float *out_f32;
    int N, H, W, Cin, Csc, Cout, KH, KW;
    int relu, pool;
    float out_scale;           // f16x3 only: 1/S of the power-of-two weight scaling (conv_f16x3.hip)
    unsigned *sat;             // f16x3 only: sticky flag raised when a stored activation exceeded the fp16 range (may be nullptr)
    AblConvArgs abl;           // empty in the product library
};
hipError_t launch_conv_x6(hipStream_t s, const ConvX6Args &a);
hipError_t launch_f32_to_split3(hipStream_t s, const float *x, unsigned short *out, size_t n, size_t plane_stride);
hipError_t launch_split3_to_f32(hipStream_t s, const unsigned short *x, float *out, size_t n, size_t plane_stride);
// Same operation on "split-2" activations (two fp16 planes) with three fp16 MFMA products per term (conv_f16x3.hip).
// Weights packed [K-step][2 splits][Cout/16][64 lanes][8 fp16], pre-multiplied by 1/out_scale.
hipError_t launch_conv_h2(hipStream_t s, const ConvX6Args &a);
hipError_t launch_f32_to_split2(hipStream_t s, const float *x, unsigned short *out, size_t n, size_t plane_stride, unsigned *sat = nullptr);
hipError_t launch_split2_to_f32(hipStream_t s, const unsigned short *x, float *out, size_t n, size_t plane_stride);

// ------------------------------------------------------------------------------------------------ 16x16 tails, LDS-resident
// chain16.hip (f16x3 datapath): the layers of a net that run at 16x16 resolution - where a block is a single tile - with
// every activation of a ResidualBlock resident in LDS, two blocks per CU (round 6: three / two kernels per tail, tail16_dev.h); bit-identical to the launch-per-layer path.  Weights: a ResidualBlock's pack_h2 streams
// (RBWeights::w0h / w2h / wsch) with 1/S of its two passes (s0 = 2^-k0, s2 = 2^-k2).
struct Chain16RB { const unsigned short *w0, *w2, *wsc; float s0, s2; };
// MTT nets: trunk_B1 + conv_B1 -> out0; cat[up2(q), out0] -> trunk_Att1, x x5 -> trunk_B2 + conv_B2 -> out1 (accumulated)
struct Chain16MsbdArgs {
    const unsigned short *x5; size_t x5_stride;     // [N][4][16][16][16] split-2
    unsigned short *xb; size_t xb_stride;           // scratch, same layout: x5 * att0, handed from the attention kernel to trunk_B2's through L2
    const float *qt; float *bt, *dire;              // raw QT logits [N][64]; outputs [N][3][256], layers 0 and 1
    Chain16RB b1[3], att[2], b2[3];
    const float *head_w[2], *head_b[2];             // conv_B1, conv_B2: [9][8][2] + [2]
    unsigned *sat;
    int N;
    float att_scale;                                // f16x3 activation scale of attention segment 1 (2^-e1; the attention input is built in the kernel)
};
hipError_t launch_msbd_branch16(hipStream_t s, const Chain16MsbdArgs &a);
// QT nets: resblock_q3 -> multi-scale pool -> resblock_q4 -> resblock_q5 + max_pool2d(2) -> resblock_q6 (8x8, fp32 direct) -> conv_q2
struct Chain16QtArgs {
    const unsigned short *x4; size_t x4_stride;     // [N][4][16][16][16] split-2: resblock_q2's pooled output
    float *x5;                                      // scratch [N][2][16][16][16] fp32: resblock_q3's output (the multi-scale pool reads fp32)
    float *qt;                                      // [N][64]
    Chain16RB q3, q4, q5;
    const float *d_w0, *d_w2, *d_wsc;               // resblock_q6, plain fp32 packing (pack_plain)
    const float *head_w, *head_b;                   // conv_q2: [9][8][1] + [1]
    unsigned *sat;
    int N;
};
hipError_t launch_qt_tail16(hipStream_t s, const Chain16QtArgs &a);

// ------------------------------------------------------------------------------------------------ a ResidualBlock at 32x32, one launch
// rbfuse32.hip (f16x3 datapath): conv3x3 + ReLU, conv3x3 + 1x1 shortcut + ReLU [+ 2x2 max-pool] of a block with <= 32 output channels,
// the intermediate resident in LDS; bit-identical to two launches of conv_f16x3.hip.  Shapes: (cin_groups, cout_groups, pool_f32) =
// (2, 1, 0) trunk_B3.1, (1, 1, 1) trunk_B3.2, (1, 2, 0) trunk_Att2.0.
struct RbFuse32Args {
    const unsigned short *x; size_t x_stride;        // [N][cin_groups][H][W][16] split-2
    const unsigned short *w0, *w2, *wsc;             // the block's pack_h2 streams (RBWeights::w0h / w2h / wsch)
    float s0, s2;                                    // 1/S of the two passes
    unsigned short *out; size_t out_stride;          // [N][cout_groups][H][W][16] split-2 ...
    float *out_f32;                                  // ... or, with pool_f32, [N][cout_groups][H/2][W/2][16] plain fp32
    unsigned *sat;
    int N, H, W, cin_groups, cout_groups, pool_f32;
    // x == nullptr (trunk_Att2.0 only): the block's input is the attention input cat[up(q), up(bt[att_layer]), up(dire[att_layer])], built in
    // the kernel from the logits q [N][64], bt / dire [N][3][256] (launch_att_input's arithmetic)
    const float *q, *bt, *dire; int att_layer;
    float att_scale;                                 // ... times the f16x3 activation scale of its segment (2^-e3)
};
hipError_t launch_rbfuse32(hipStream_t s, const RbFuse32Args &a);

// ------------------------------------------------------------------------------------------------ stems
// First layers straight from the u8 blocks (Model_QBD.py:79-80, :130-135, :177-178, :228-233).
// luma: block_y u8[N][68][68];  chroma: + block_u/v u8[N][34][34], plane 0 = 2x2 max-pool of block_y
// (Inference_QBD.py:196-200).  msbd: adds the plane built from the raw QT logits q f32[N][8][8]
// (nearest x8 / x4 upsample, zero pad top/left by 4 / 2).  Output: 32 channels, [N][2][S][S][16], S = 64 / 32.
struct StemArgs {
    const uint8_t *by, *bu, *bv;
    const float *q;      // msbd only
    const float *w;      // packed per conv: [conv][tap][cin][cout], see pack_stem()
    const float *bias;   // [32]
    float *out;
    int N;
    unsigned short *out_s3; size_t s3_stride;   // if out_s3 != nullptr the 32 channels are written as split planes ...
    int fmt;                                    // ... of format 1 (three bf16) or 2 (two fp16), see split3.h
    const unsigned short *wh; float out_scale;  // fmt 2: fp16 fragment stream (pack_stem_h2) and 1/scale -> the MFMA stem
    unsigned *sat;                              // fmt 2: saturation flag (see ConvX6Args)
};
hipError_t launch_stem(hipStream_t s, bool luma, bool msbd, const StemArgs &a);

// ------------------------------------------------------------------------------------------------ small direct conv
// Generic direct convolution for the tiny tail layers (8x8 maps, 8-channel trunks):
// out = [relu]( conv(x, w) [+ conv1x1(x_sc, w_sc)] [+ res] [+ bias] ).  Weights plain [tap][cin][cout_real].
struct ConvDirectArgs {
    const float *x; const float *w;
    const float *x_sc; const float *w_sc;
    const float *res; const float *bias;
    float *out;
    int N, H, W, Cin, CinPad, Csc, CscPad, Cout, CoutPad, KH, KW, relu;
};
hipError_t launch_conv_direct(hipStream_t s, const ConvDirectArgs &a);

// Heads (Model_QBD.py:91,:139,:145-146,:152-153): 3x3, 8 -> 1 (QT) or 8 -> 2 (MTT layer k), bias, no activation.
// QT: qt[n][y][x].  MTT layer k: bt[n][k][y][x] = ch0 (+ bt[n][k-1][y][x] if k > 0), dire[n][k][y][x] = ch1.
struct HeadArgs {
    const float *x;   // [N][1][S][S][16], channels 0..7 used
    const float *w;   // [9][8][cout]
    const float *bias;
    float *qt, *bt, *dire;
    int N, S, layer;  // layer < 0: QT head
};
hipError_t launch_head(hipStream_t s, const HeadArgs &a);

// x5 [N][2][16][16][16] -> cat[x5, up2(mp2), up4(mp4), up8(mp8)] [N][8][16][16][16]  (Model_QBD.py:84-87)
hipError_t launch_multipool_concat(hipStream_t s, const float *x5, float *x6, int N, unsigned short *x6_s3 = nullptr,
                                   size_t s3_stride = 0, int fmt = 1, unsigned *sat = nullptr);

// Attention trunk input (Model_QBD.py:140, :147): [N][1][S][S][16] with ch0 = up(q) (S/8 nearest), ch1 = bt[n][layer],
// ch2 = dire[n][layer] (both 16x16, nearest-upsampled to S), channels 3..15 zero.
hipError_t launch_att_input(hipStream_t s, const float *q, const float *bt, const float *dire, int layer, float *out,
                            int N, int S, unsigned short *out_s3 = nullptr, size_t s3_stride = 0, int fmt = 1, unsigned *sat = nullptr,
                            float scale = 1.f);     // scale: the f16x3 activation scale of the attention segment (a power of two)

// Largest |value| of an fp32 tensor (n a multiple of 4), atomicMax'ed into *slot as the bit pattern of the magnitude: the calibration
// pass of the f16x3 activation scales (calibrate.cpp: calibrate_mtt).
hipError_t launch_amax_f32(hipStream_t s, const float *x, size_t n, unsigned *slot);

// ------------------------------------------------------------------------------------------------ post-processing
// Map_to_Partition's thresholds (include/pmp.h: pmp_partition_params; validated by the caller): lamb1..lamb5 and th_round's thd.
struct M2PParams {
    double lamb[5];
    float thd;
};
constexpr M2PParams M2P_DEFAULT = {{0.7, 0.7, 1.5, 0.3, 0.7}, 0.5f};   // Map2Partition.py:100,105
inline bool m2p_is_default(const M2PParams &p)
{
    for (int i = 0; i < 5; ++i) if (p.lamb[i] != M2P_DEFAULT.lamb[i]) return false;
    return p.thd == M2P_DEFAULT.thd;
}
// eli_structual_error + Map_to_Partition, one wavefront per block.  qt raw logits [N][64]; bt, dire [N][3][256].
// record_stride != 0: the four outputs are fields of one packed record per block (bytes between blocks), else dense arrays.
hipError_t launch_postprocess(hipStream_t s, const float *qt, const float *bt, const float *dire, int64_t N, int chroma_factor,
                              const M2PParams &prm, uint8_t *hor, uint8_t *ver, uint8_t *qt_u8, int8_t *dire_i8, int record_stride = 0);

// GenMSBtMap (labels.hip): qt u8[N][64], bt u8[N][256], dire i8[N][3][256] -> msbt u8[N][3][256], status u8[N] (include/pmp.h: pmp_msbt_labels).
hipError_t launch_msbt_labels(hipStream_t s, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t N, int chroma_factor,
                              uint8_t *msbt, uint8_t *status);
// The labels' own partition (labels.hip; include/pmp.h: pmp_label_partition): the same inputs -> hor, ver u8[N][256] and status u8[N], or
// with rec != null (hor, ver ignored) one packed record u8[N][PMP_RECORD_BYTES] = hor | ver | qt | dire per block.  All 4-byte aligned.
hipError_t launch_label_partition(hipStream_t s, const uint8_t *qt, const uint8_t *bt, const int8_t *dire, int64_t N, int chroma_factor,
                                  uint8_t *hor, uint8_t *ver, uint8_t *rec, uint8_t *status);

// Logits against labels (logitstats.hip): what pmp_val_stats and pmp_train_loss read.  qt f32[N][64] with qt8 u8[N][64] (RAW qtDepth),
// bt, dire f32[N][3][256] with msbt u8 / msdire i8 [N][3][256].  qt/qt8 null: MTT only; bt/dire/msbt/msdire null: QT only.
// bt, dire 16-byte aligned, the others 4-byte aligned.
struct LogitLabels {
    const float *qt, *bt, *dire;
    const uint8_t *qt8, *msbt;
    const int8_t *msdire;
    __host__ __device__ bool has_q() const { return qt != nullptr; }
    __host__ __device__ bool has_m() const { return bt != nullptr; }
    LogitLabels from(int64_t o) const                   // the same arrays from block o on; what is left out stays left out
    {
        return {qt ? qt + o * 64 : nullptr,    bt ? bt + o * 768 : nullptr,     dire ? dire + o * 768 : nullptr,
                qt8 ? qt8 + o * 64 : nullptr,  msbt ? msbt + o * 768 : nullptr, msdire ? msdire + o * 768 : nullptr};
    }
};
// The gradients of pmp_train_loss: qt f32[N][64], bt, dire f32[N][3][256] (16-byte aligned); all null = value only, else those of
// the logits given.
struct LogitGrads {
    float *qt, *bt, *dire;
    LogitGrads from(int64_t o) const { return {qt ? qt + o * 64 : nullptr, bt ? bt + o * 768 : nullptr, dire ? dire + o * 768 : nullptr}; }
};
// w_k = dl_k * dl_k + wm[k], wm = float32(weight matrix[row][0..2]) of the component; w0_one: qp == 22 (weight_d0 = 1.0)
struct LogitWeights {
    float wm[3];
    int w0_one;
};

// Validation statistics (include/pmp.h: pmp_val_stats): block_stats f64[N][20] (always written: the caller's buffer or scratch) and
// their fixed-order sum stats f64[20].  lw: the luma matrix.  N >= 1.
hipError_t launch_val_stats(hipStream_t s, const LogitLabels &in, int64_t N, const LogitWeights &lw, double *block_stats, double *stats);

// Confusion counts (include/pmp.h: pmp_val_confusion): block_counts u16[N][175] (always written: the caller's buffer or scratch) and
// their column sums counts i64[175].  A group is counted if its LABELS are given (in.qt8; in.msbt, in.msdire); without its logits it is
// the labels' census.  N >= 1.
hipError_t launch_val_confusion(hipStream_t s, const LogitLabels &in, int64_t N, uint16_t *block_counts, int64_t *counts);

// Training losses and their logit gradients (include/pmp.h: pmp_train_loss): block_terms f64[N][13] (scratch, always written), their
// fixed-order sum terms f64[13] and, if loss != null, train_loss_value(terms, L, n_div).  Every cell of the gradients given is
// written.  n_div: the block count in the gradients' divisors 64 n and 256 n (the whole call's, where N is one pass of it).  N >= 1.
hipError_t launch_train_loss(hipStream_t s, const LogitLabels &in, int64_t N, int64_t n_div, const LogitWeights &lw, const pmp_loss_params &L,
                             double *block_terms, double *terms, double *loss, const LogitGrads &g);
// lambq T0 / (64 n) + (lambb0 T1 + .. + lambresb2 T12) / (256 n) in float64, in that order, on either side (no FMA)
__host__ __device__ double train_loss_value(const double T[PMP_LOSS_NTERMS], const pmp_loss_params &L, int64_t n);

// ------------------------------------------------------------------------------------------------ training (conv_wgrad.hip)
// Weight gradient of a stride-1 KxK convolution (K = 1, 3, 5): dw[cout][cin][K][K] (torch's dense layout, real channels only) =
// sum over (n, y, x) of g[n][co][y][x] * a[n][ci][y + dy - K/2][x + dx - K/2].  a [N][Ca/16][H][W][16] and g [N][Cg/16][H][W][16] are
// blocked, Ca = 16, 32, 64 or 128, Cg = 16, 32 or 64; cin <= Ca, cout <= Cg.  part: scratch of wgrad_partial_floats() floats, every one written.  Two
// launches, a fixed order of additions that depends on the shape only, no atomics.
size_t wgrad_partial_floats(int N, int H, int W, int Ca, int Cg, int K);
hipError_t launch_wgrad(hipStream_t s, const float *a, const float *g, int N, int H, int W, int Ca, int Cg, int K, float *part,
                        float *dw, int cout, int cin);
// torch's dense [N][C][H][W] <-> blocked [N][Cp/16][H][W][16] (channels C .. Cp-1 zero / dropped).  mode 0: the values; 1: src where
// m > 0, else 0 (m dense, src's shape) - a ReLU's backward.
hipError_t launch_dense_to_blocked(hipStream_t s, const float *src, const float *m, int mode, float *dst, int N, int C, int Cp, int H, int W);
hipError_t launch_blocked_to_dense(hipStream_t s, const float *src, float *dst, int N, int C, int Cp, int H, int W);
// pack_mfma() on the device, from w [cout][cin][K][K] into [CB][K*K][NT][64][4].  flip_t = 0: as is (16 NT >= cout, 16 CB >= cin);
// flip_t = 1: taps mirrored, cin and cout swapped - the data gradient's weights (16 CB >= cout; its first 16 NT output channels where
// cin is larger: w + 16 NT K K then packs the next ones).
hipError_t launch_pack_mfma(hipStream_t s, const float *w, float *out, int cout, int cin, int K, int NT, int CB, int flip_t);

// ------------------------------------------------------------------------------------------------ training, blocked in and out (trunk_glue.hip)
// A trunk of ResidualBlocks keeps its activations blocked [N][Cp/16][H][W][16] (H, W multiples of 16): these are the steps between
// its convolutions.  Padded channels are zero on the way in and on the way out.
// mode 1: dst = a where m > 0, else 0 - launch_dense_to_blocked's mode 1;  2: dst = 1.0 where a > 0, else 0.0 (m unused) - a ReLU's mask
// as the conv kernel's `gate`.  In both dst may be a.
hipError_t launch_blocked_relu(hipStream_t s, int mode, const float *a, const float *m, float *dst, int N, int Cp, int H, int W);
// 2x2 max-pool of blocked src into dense dst [N][C][H/2][W/2]: the bits of conv_mfma's `pool` epilogue
hipError_t launch_pool_to_dense(hipStream_t s, const float *src, float *dst, int N, int C, int Cp, int H, int W);
// dense upstream gradient g -> blocked dst, behind the ReLU of blocked `out` (un-pooled).  pool = 0: g [N][C][H][W], dst = g where
// out > 0.  pool = 1: g [N][C][H/2][W/2], dst[y][x] = g[y/2][x/2] where out[y][x] > 0 and is the FIRST maximum of its 2x2 window in
// the order (0,0), (0,1), (1,0), (1,1).  Everything else, the padded channels included, is written as +0.
hipError_t launch_grad_to_blocked(hipStream_t s, int pool, const float *g, const float *out, float *dst, int N, int C, int Cp, int H, int W);

// ------------------------------------------------------------------------------------------------ training, a net's stem (stem_train.hip)
// pmp_stem_*'s convolution: x [N][cin][H+K/2][W+K/2], zeros to its right and below; y, g_y [N][32][H][W]; w, b and their gradients the
// caller's one (split 0) or three (split 1) dense tensors, read and written through the unified K x K kernel.  cin 1..4, K 5 or 9.
struct StemTrainArgs {
    int N, H, W, cin, K, split;
    const float *x, *y, *g_y;          // y: the forward's output, read by the gradients
    const float *w[3], *b[3];
    float *y_out;                      // forward
    float *g_x, *g_w[3], *g_b[3];      // backward; g_x only for launch_stem_dgrad
};
size_t stem_packed_floats(int cin, int K);                            // launch_stem_forward's scratch, every word written
size_t stem_partial_floats(int N, int H, int W, int cin, int K);      // launch_stem_wgrad's
hipError_t launch_stem_forward(hipStream_t s, const StemTrainArgs &a, float *packed);     // y_out = relu(conv(x, w) + b)
hipError_t launch_stem_wgrad(hipStream_t s, const StemTrainArgs &a, float *part);         // g_w, g_b: two launches, a fixed order
hipError_t launch_stem_dgrad(hipStream_t s, const StemTrainArgs &a);                      // g_x, every element

// ------------------------------------------------------------------------------------------------ training, a head and the gate (head_train.hip)
// pmp_head_*'s 3x3 bias convolution with cin 1..16 inputs and cout 1..2 outputs on dense NCHW, its carry and its attention input;
// the formulas and the orders of summation are include/pmp.h's.  H, W multiples of 8.
struct HeadTrainArgs {
    int N, H, W, cin, cout, up_q, up_y;
    const float *x, *w, *b, *prev, *q;           // forward; x and w backward too
    float *y, *att;
    const float *g_y, *g_att;                    // backward
    float *g_x, *g_w, *g_b, *g_q, *g_prev;       // g_x, g_q, g_prev may be null
};
size_t head_partial_floats(int N, int H, int W, int cin, int cout);       // launch_head_backward's scratch, every word written
hipError_t launch_head_forward(hipStream_t s, const HeadTrainArgs &a);
hipError_t launch_head_backward(hipStream_t s, const HeadTrainArgs &a, float *part);
// y = x * a;  g_a = g_y * x, g_x = (g_acc ? g_acc + : ) g_y * a: product and sum each rounded once.  count >= 1
hipError_t launch_gate_forward(hipStream_t s, size_t count, const float *x, const float *a, float *y);
hipError_t launch_gate_backward(hipStream_t s, size_t count, const float *x, const float *a, const float *g_y, const float *g_acc, float *g_x,
                                float *g_a);

// ------------------------------------------------------------------------------------------------ training, a QT net's tail (qtail_train.hip)
// The steps of pmp_qtail_* between its ResidualBlocks, all on blocked tensors of an H x W map (multiples of 16) and of q6's map
// H2 x W2 = (H/2, W/2) rounded up to 16, which holds the H/2 x W/2 pixels top-left and +0 elsewhere.  One launcher: step, then
//   QT_MULTIPOOL       a = x5 [N][2][H][W][16]                              -> out = x6 [N][8][H][W][16]
//   QT_MULTIPOOL_BACK  a, b = g6's channels 0..63, 64..127 [N][4][H][W][16], c = x5 -> out = q3's upstream gradient [N][2][H][W][16]
//   QT_POOL_EMBED      a = q5's out [N][2][H][W][16]                        -> out = x8 [N][2][H2][W2][16], out2 (may be null) = the
//                                                                              region's 0/1 mask [N][1][H2][W2][16]
//   QT_POOL_BACK       a = q6's data gradient [N][2][H2][W2][16], b = q5's out -> out = q5's upstream gradient [N][2][H][W][16]
//   QT_EMBED_GRAD      a = g_x9 dense [N][8][H/2][W/2], b = q6's out [N][1][H2][W2][16] -> out = q6's upstream gradient, same shape
//   QT_CROP_DENSE      a = a tensor of q6's map [N][1][H2][W2][16]          -> out = dense [N][8][H/2][W/2]
// Every element of every output is written; the arithmetic is include/pmp.h's.
enum { QT_MULTIPOOL, QT_MULTIPOOL_BACK, QT_POOL_EMBED, QT_POOL_BACK, QT_EMBED_GRAD, QT_CROP_DENSE };
hipError_t launch_qtail_step(hipStream_t s, int step, const float *a, const float *b, const float *c, float *out, float *out2, int N, int H, int W);

// ------------------------------------------------------------------------------------------------ training, a step's ends (train_step.hip)
// pmp_batch_gather_device: one workgroup per row of the batch; every pointer 4-byte aligned, n in 1..PMP_BATCH_MAX, src.count >= 1
hipError_t launch_batch_gather(hipStream_t s, const pmp_batch_src &src, const int64_t *index, int n, const pmp_batch_dst &dst, int32_t *status);
// pmp_adam_step_device: one launch over the first nt <= PMP_ADAM_TABLE entries of t, an entry being a tensor (or a part of one) of
// 1 .. 2^30 floats.  The float32 constants are include/pmp.h's.  The table travels in the kernel's argument block.
struct AdamConsts { float d1, b2, d2, neg_af, rf, ef; };
struct AdamTable {
    float *param[PMP_ADAM_TABLE];
    const float *grad[PMP_ADAM_TABLE];
    float *m[PMP_ADAM_TABLE], *v[PMP_ADAM_TABLE];
    unsigned count[PMP_ADAM_TABLE];
    unsigned first[PMP_ADAM_TABLE];     // the entry's first workgroup: filled by the launcher
};
// rec: NULL, or pmp_adam_step_guarded_device's record in device memory, which the kernel reads coef and the skip bit from
hipError_t launch_adam_step(hipStream_t s, AdamTable &t, int nt, const AdamConsts &k, const pmp_guard_record *rec = nullptr);
// pmp_grad_guard_device: one census launch over the first nt <= PMP_ADAM_TABLE entries of t, count[i] in 1 .. 2^30 - 1, a workgroup to a
// tile of 4096 elements; the launch's first tile is tile0 of the call's tiles_all.  scratch: 16 bytes a tile, the partial sums
// (float64) in front of the counts (uint64), each written by its tile.  Then one finish launch over all tiles writes rec and steps st
// (may be NULL)
struct GuardTable {
    const float *grad[PMP_ADAM_TABLE];
    unsigned count[PMP_ADAM_TABLE];
    unsigned first[PMP_ADAM_TABLE];     // the entry's first workgroup: filled by the launcher
};
hipError_t launch_grad_census(hipStream_t s, GuardTable &t, int nt, int64_t tile0, void *scratch, int64_t tiles_all);
hipError_t launch_grad_guard_finish(hipStream_t s, const void *scratch, int64_t tiles, const pmp_guard_params &p, pmp_guard_record *rec,
                                    pmp_guard_state *st);
// pmp_grad_pack_device: one launch over the first nt <= PMP_ADAM_TABLE entries of t: grad[i] (NULL: zeros), count[i] in 1 .. 2^30 - 1
// floats, to bucket + at[i], both 16-byte aligned; the padding behind a tensor, up to a multiple of 4 floats, is written as zeros
struct GradPackTable {
    const float *grad[PMP_ADAM_TABLE];
    int64_t at[PMP_ADAM_TABLE];
    unsigned count[PMP_ADAM_TABLE];
    unsigned first[PMP_ADAM_TABLE];     // the entry's first workgroup: filled by the launcher
};
hipError_t launch_grad_pack(hipStream_t s, GradPackTable &t, int nt, float *bucket);
// pmp_grad_sum_device: dst = ((src[0] + src[1]) + ...) over quads float4s; nsrc in 1..PMP_GRAD_SUM_MAX, every pointer 16-byte aligned
struct GradSumTable { const float *src[PMP_GRAD_SUM_MAX]; };
hipError_t launch_grad_sum(hipStream_t s, const GradSumTable &t, int nsrc, int64_t quads, float *dst);

// ------------------------------------------------------------------------------------------------ data set assembly (dataset.hip)
// pmp_select_rows_device: the flag arrays travel in the kernel's argument block.  scratch: select_scratch_words(n, nseg) 32-bit words,
// every one written before it is read.  n in 1..2^30, nseg in 1..65536, nflags in 0..PMP_SELECT_MAX_FLAGS, cap >= 0; five launches.
constexpr int SELECT_TILE = 1024;
struct SelectFlags { const uint8_t *p[PMP_SELECT_MAX_FLAGS]; };
size_t select_scratch_words(int64_t n, int nseg);
hipError_t launch_select_rows(hipStream_t s, const SelectFlags &f, int nflags, int mask, const int64_t *seg_end, int nseg, int64_t cap, int64_t n,
                              uint32_t *scratch, int64_t *index, int64_t *count);
// pmp_gather_rows_device: src, dst 4-byte aligned, row_bytes a multiple of 4 in 4..65536, m in 1..2^30, nsrc >= 1
hipError_t launch_gather_rows(hipStream_t s, const void *src, int64_t nsrc, int64_t row_bytes, const int64_t *index, int64_t m, void *dst, int32_t *status);

// Block cutter (Inference_QBD.py:104-149).
hipError_t launch_cut_blocks(hipStream_t s, const void *y, const void *u, const void *v, int F, int H, int W,
                             int bitdepth, uint8_t *by, uint8_t *bu, uint8_t *bv);

}  // namespace pmp
