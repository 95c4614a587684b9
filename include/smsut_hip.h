/* smsut_hip.h -- C ABI of the MI355X (gfx950) kernels behind the SMSUT conv hot path.
 *
 * The reference (Sue1347/SMSUT-MedicalImgSegmentation) has no native code and no FFI: its boundary is the Python
 * module API (network.unet / network.ugan / network.networks constructors, trainer.uganConsisTrainer), whose
 * arithmetic it delegates to torch operators.  Each entry point below replaces the torch operator(s) named in
 * its comment at the cited reference call site(s); `smsut-medicalimgsegmentation_amd/ops.py` binds them behind
 * torch.autograd.Function objects and INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every pointer is DEVICE memory (fp32 unless typed otherwise), allocated and owned by the caller; the
 *     library never allocates, frees or synchronises; `workspace` sizes come from the matching `*_ws` query;
 *   - activations are dense NHWC: [N][H][W][C]; conv weights are [KH][KW][Cin][Cout]; ConvTranspose2x2 weights
 *     are [kh][kw][Cin][Cout]; Linear weights are [in][out];
 *   - `stream` is a hipStream_t passed as void*; every kernel is enqueued on it (graph-capture safe);
 *   - return value: 0 = enqueued, -1 = invalid argument, > 0 = hipError_t of the launch; nothing throws;
 *   - no global mutable state; safe to call from several host threads on different streams;
 *   - the library's only environment input is SMSUT_WINOGRAD, read once per process: "0" runs the direct forms of
 *     the 3x3 convs where the Winograd F(2x2,3x3) forms would run (the reference those forms are tested against);
 *     every other kernel choice follows from the arguments of the call.
 */
#ifndef SMSUT_HIP_H
#define SMSUT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------- convolution
 * nn.Conv2d as used at network/blocks.py:10-16 (conv3x3 / conv1x1), blocks.py:123 + ugan.py:26 (5x5 stems),
 * ugan.py:70 (1x1 heads with bias), ugan.py:202 (D stem k4 s2 p1 + bias), ugan.py:214-215 (conv_src / conv_cls).
 * *_generic: any kernel size / stride / zero padding (direct convolution).
 * *_mfma   : stride-1 "same" 1x1 / 3x3 on the matrix cores (v_mfma_f32_16x16x4_f32), the > 97 %-of-FLOPs path. */
int smsut_conv2d_fwd_generic(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H,
                             int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                             void* stream);
int smsut_conv2d_dgrad_generic(const float* gy, const float* w, float* gx, int N, int H, int W, int Cin, int Ho, int Wo,
                               int Cout, int KH, int KW, int stride, int pad, void* stream);
int64_t smsut_conv2d_wgrad_generic_ws(int N, int Ho, int Wo, int Cin, int Cout, int KH, int KW);
int smsut_conv2d_wgrad_generic(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W,
                               int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, void* stream);

int smsut_conv2d_mfma_supported(int KS, int stride, int pad, int Kdim, int Ndim);
/* transposed = 0: y[N,H,W,Ndim] = conv(x[N,H,W,Kdim], w[KS*KS][Kdim][Ndim]);
 * transposed = 1: data-gradient, x = gy[N,H,W,Kdim=Cout], w = forward weights [KS*KS][Ndim=Cin][Kdim=Cout];
 * transposed | 2: the result is ADDED to what y already holds (second gradient path into a block input,
 *                 reference autograd's accumulation for x used by conv1 and the shortcut, network/blocks.py:66-78). */
int smsut_conv2d_fwd_mfma(const float* x, const float* w, float* y, int N, int H, int W, int Kdim, int Ndim, int KS,
                          int transposed, void* stream);
/* forward conv that also emits the InstanceNorm {sum, sum^2} partials of its output (fused statistics pass):
 * stats = float[N * smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, KS, f16) * Ndim * 2], consumed by smsut_instnorm_fwd_partials
 * (the tile shape is chosen per layer shape AND operand dtype -- f16 = 1 for the *_f16 entry points: the fp32 forms of a shape may
 * run a Winograd kernel on 16-row items where the fp16-operand ones keep the direct kernel's -- so both are part of the query). */
int smsut_conv2d_mfma_tiles(int N, int H, int W, int Kdim, int Ndim, int KS, int f16);
/* 1 when this shape runs one of the persistent kernels that carry the fused forms (statistics / input-side IN / BST epilogues):
 * conv_mfma_fwd_p (direct or Winograd F(2x2,3x3), resident weights, Kdim <= 64) or, fp32 only, conv_wino_l (Winograd, streamed
 * weights, Kdim >= 64); else 0 (per-tile kernel). */
int smsut_conv2d_mfma_persistent(int N, int H, int W, int Kdim, int Ndim, int KS, int f16);
/* data-gradient of conv2 inside a BasicBlock (its input was LeakyReLU(IN(y1)), blocks.py:66-72) with the InstanceNorm backward
 * folded into the epilogue: gz = g * mask(y1) is written instead of g, plus the per-tile partials {sum gz, sum gz*xhat}
 * [N][smsut_conv2d_mfma_tiles(N,H,W,Kdim,Ndim,3)][Ndim][2].  Persistent-kernel shapes only (-1 otherwise). */
int smsut_conv2d_dgrad_mfma_bwdstats(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                     const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     float slope, int N, int H, int W, int Kdim, int Ndim, void* stream);
int smsut_conv2d_fwd_mfma_stats(const float* x, const float* w, float* y, float* stats, int N, int H, int W, int Kdim,
                                int Ndim, int KS, void* stream);
/* tuning hook: same as smsut_conv2d_fwd_mfma with a forced tile configuration (returns -1 for an unknown cfg) */
int smsut_conv2d_fwd_mfma_cfg(const float* x, const float* w, float* y, int N, int H, int W, int Kdim, int Ndim, int KS,
                              int transposed, int cfg, void* stream);
/* Prepared Winograd weights (optional; replaces nothing in the reference -- it is the cuDNN-internal filter transform of the
 * nn.Conv2d sites above made explicit, network/blocks.py:10-16): the large-reduction Winograd kernel (Kdim >= 64) transforms its
 * weights U = G g G^T per workgroup and chunk unless the caller hands it a prepared image.
 *   smsut_wino_image_floats(Kdim, Ndim)  floats of one image (16 * Kdim * Ndim; 0 when the shape has none);
 *   smsut_wino_prepare                  writes the images of `count` weight tensors in ONE launch.  w[i]: a 3x3 weight tensor in
 *                                       this library's layout [3][3][Cin][Cout]; transposed[i] = 0: image of the forward conv
 *                                       (Kdim[i] = Cin, Ndim[i] = Cout), 1: of its data-gradient (Kdim[i] = Cout, Ndim[i] = Cin);
 *                                       u[i]: device float[smsut_wino_image_floats(Kdim[i], Ndim[i])].  The five arrays are HOST arrays;
 *   *_pre entry points (below)         the conv entry points that may run that kernel, with one more argument: wu = the image the
 *                                       CALLER prepared for this weight tensor and form (same Kdim, Ndim, same bit 0 of `transposed`),
 *                                       or NULL = transform on the fly.  The caller keeps wu in step with w (re-prepare after every
 *                                       change of w).  The library holds NO table of images and no other process-wide mutable state
 *                                       (r03's smsut_wino_bind* registry is gone): an image is an argument like any other.
 * Results are bit-identical with and without an image (same arithmetic, done once instead of per workgroup). */
int64_t smsut_wino_image_floats(int Kdim, int Ndim);
int smsut_wino_prepare(const float* const* w, float* const* u, const int* Kdim, const int* Ndim, const int* transposed, int count,
                       void* stream);
int smsut_conv2d_fwd_mfma_pre(const float* x, const float* w, float* y, int N, int H, int W, int Kdim, int Ndim, int KS,
                              int transposed, const float* wu, void* stream);
int smsut_conv2d_fwd_mfma_stats_pre(const float* x, const float* w, float* y, float* stats, int N, int H, int W, int Kdim,
                                    int Ndim, int KS, const float* wu, void* stream);
int smsut_conv2d_dgrad_mfma_bwdstats_pre(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta,
                                         float slope, int N, int H, int W, int Kdim, int Ndim, const float* wu, void* stream);
int smsut_conv2d_fwd_mfma_stats_inaff_pre(const float* x, const float* w, float* y, float* stats, const float* mean,
                                          const float* rstd, const float* gamma, const float* beta, float slope, int N, int H,
                                          int W, int Kdim, int Ndim, const float* wu, void* stream);
int smsut_conv2d_fwd_mfma_stats_cat_pre(const float* xa, const float* xb, const float* w, float* y, float* stats, int N, int H,
                                        int W, int Kdim, int Ndim, const float* wu, void* stream);
int smsut_conv2d_fwd_mfma_split_pre(const float* x, const float* w, float* ya, float* yb, int split, int N, int H, int W,
                                    int Kdim, int Ndim, int transposed, const float* wu, void* stream);
int smsut_conv2d_fwd_mfma_stats_sc_pre(const float* x, const float* xb, const float* w, const float* wsc, float* y, float* ysc,
                                       float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim, const float* wu,
                                       void* stream);
int smsut_conv2d_wgrad_mfma_supported(int KS, int stride, int pad, int Cin, int Cout);
int64_t smsut_conv2d_wgrad_mfma_ws(int N, int H, int W, int Cin, int Cout, int KS);
int smsut_conv2d_wgrad_mfma(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin,
                            int Cout, int KS, void* stream);

/* 1x1 convolutions as streaming GEMMs (shortcuts blocks.py:63,95-97; up-path blocks.py:45; nn.Linear ugan.py:295): the
 * activation operand goes global -> registers (no LDS, no barrier in the loop), only the weights are staged.
 * transposed = 1 is the data-gradient.  stats (nullable): InstanceNorm partials [N][smsut_conv1x1_tiles][Ndim][2].
 * The weight gradients (smsut_conv1x1_wgrad, smsut_conv1x1_wgrad_cat) take any Cin, Cout with (Cin * Cout) % 4 == 0 -- their
 * split slabs are summed as float4s -- and refuse every other pair with an invalid-argument status before anything is launched. */
int smsut_conv1x1_supported(int Kdim, int Ndim);
int smsut_conv1x1_tiles(int N, int HW, int Ndim);
int smsut_conv1x1_fwd(const float* x, const float* w, float* y, float* stats /*nullable*/, int N, int HW, int Kdim,
                      int Ndim, int transposed, void* stream);
int64_t smsut_conv1x1_wgrad_ws(int N, int HW, int Cin, int Cout);
int smsut_conv1x1_wgrad(const float* x, const float* gy, float* gw, float* workspace, int N, int HW, int Cin, int Cout,
                        void* stream);

/* input-side InstanceNorm + LeakyReLU: the operand is a = lrelu(IN(x; mean[N,C], rstd[N,C], gamma[C], beta[C])) of the tensor
   passed, normalised while the tiles are staged -- conv2 of a BasicBlock (network/blocks.py:70-72) and its weight gradient
   read the raw conv1 output, so the activation a1 is never written to or read from HBM.  Same in_affine() fma as the IN
   kernels: results equal the two-pass path bit for bit.  Forward: persistent-kernel shapes (smsut_conv2d_mfma_persistent). */
int smsut_conv2d_fwd_mfma_stats_inaff(const float* x, const float* w, float* y, float* stats, const float* mean,
                                      const float* rstd, const float* gamma, const float* beta, float slope, int N, int H,
                                      int W, int Kdim, int Ndim, void* stream);
int smsut_conv2d_wgrad_mfma_inaff(const float* x, const float* gy, float* gw, float* workspace, const float* mean,
                                  const float* rstd, const float* gamma, const float* beta, float slope, int N, int H, int W,
                                  int Cin, int Cout, void* stream);
/* measurement entry point (bench.py's roofline leg): the first of the two launches of smsut_conv2d_wgrad_mfma[_inaff] alone -- the
   register-row weight-gradient kernel (csrc/conv_wgrad_rr.hip) writing its per-split slabs, without the reduction; returns the
   number of slabs (> 0) or a negative value when the shape is not one that kernel takes.  mean == NULL: plain form. */
int smsut_conv2d_wgrad_mfma_slabs(const float* x, const float* gy, float* workspace, const float* mean, const float* rstd,
                                  const float* gamma, const float* beta, float slope, int N, int H, int W, int Cin, int Cout,
                                  void* stream);
/* which arithmetic a 3x3 stride-1 fp32 conv call of this shape runs: 0 direct, 1 Winograd F(2x2,3x3) resident weights, 2 Winograd
   streamed weights (16 instead of 36 products per 2x2 output tile); sc_dgrad: the fused shortcut data-gradient (Kdim = 2 Cout) */
int smsut_conv2d_mfma_form(int N, int H, int W, int Kdim, int Ndim, int sc_dgrad);

/* virtual-cat input forms: the logical input is cat([xa, xb], channel) (UpSampleAndConcat, network/blocks.py:49-50) read
   from the two tensors in place -- same chunk order and arithmetic as on a materialised cat, so results are bit-identical.
   ca % 16 == 0.  conv2d forward: persistent kernel, Kdim in {32, 64}, xa and xb of Kdim/2 channels each (ask _cat_supported). */
int smsut_conv2d_mfma_cat_supported(int N, int H, int W, int Kdim, int Ndim);
int smsut_conv2d_fwd_mfma_stats_cat(const float* xa, const float* xb, const float* w, float* y, float* stats, int N, int H,
                                    int W, int Kdim, int Ndim, void* stream);
/* conv1 of a BasicBlock fused with the block's 1x1 shortcut conv (reference network/blocks.py:66-80: `self.conv1(x)` and
 * `self.shortcut(x)` read the same x): y = conv3x3(x, w), ysc = conv1x1(x, wsc) and the InstanceNorm partials of both in one
 * pass.  xb nullable: non-null = x is the virtual cat([x, xb]) of two [N,H,W,Kdim/2] tensors.  _supported(..., cat) first. */
int smsut_conv2d_fwd_sc_supported(int N, int H, int W, int Kdim, int Ndim, int cat);
int smsut_conv2d_fwd_mfma_stats_sc(const float* x, const float* xb /*nullable*/, const float* w, const float* wsc, float* y,
                                   float* ysc, float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim,
                                   void* stream);
/* the same with fp16 operands (config 5): persistent kernel's direct form, Kdim in {16, 32, 64}; tiles with f16 = 1 */
int smsut_conv2d_fwd_sc_f16_supported(int N, int H, int W, int Kdim, int Ndim, int cat);
int smsut_conv2d_fwd_mfma_stats_sc_f16(const float* x, const float* xb, const float* w, const float* wsc, float* y, float* ysc,
                                       float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim, void* stream);
/* ... and the data-gradient of that pair in one pass: gx = dgrad3x3(gy, w) + dgrad1x1(gs, wsc) (the backward of
 * `out = conv1(x) ... + shortcut(x)` w.r.t. x, blocks.py:66-80).  gxb nullable: non-null = channels [0, split) of gx go to
 * gxa, the rest to gxb (the block input was cat([up, skip])).  _supported(..., split or 0) first. */
int smsut_conv2d_dgrad_sc_supported(int N, int H, int W, int Cout, int Cin, int split);
int smsut_conv2d_dgrad_mfma_sc(const float* gy, const float* gs, const float* w, const float* wsc, float* gxa,
                               float* gxb /*nullable*/, int split, int N, int H, int W, int Cout, int Cin, void* stream);
/* ... and both weight gradients in one pass: gw10 [10][Cin][Cout], rows 0..8 = conv1's 3x3 gradient (HWIO), row 9 = the 1x1
 * shortcut's; gs = gradient of the shortcut's output.  xb nullable (virtual cat, ca channels in xa). */
int smsut_conv2d_wgrad_sc_supported(int N, int H, int W, int Cin, int Cout);
int64_t smsut_conv2d_wgrad_sc_ws(int N, int H, int W, int Cin, int Cout);
int smsut_conv2d_wgrad_mfma_sc(const float* xa, const float* xb /*nullable*/, int ca, const float* gy, const float* gs,
                               float* gw10, float* workspace, int N, int H, int W, int Cin, int Cout, void* stream);
int smsut_conv2d_wgrad_mfma_cat(const float* xa, const float* xb, int ca, const float* gy, float* gw, float* workspace,
                                int N, int H, int W, int Cin, int Cout, int KS, void* stream);
/* `_fin` forms (r05) of the three statistics-producing convs of a fused BasicBlock: the same launch, with the InstanceNorm statistics
 * FINALISED INSIDE IT by the workgroup whose partials complete an image (fixed-order fp64 combine, the bits smsut_in_finalize_fwd /
 * _fwd2 / _bwd produce) -- the separate finalize launch behind each of them disappears (reference: conv -> nn.InstanceNorm2d,
 * network/blocks.py:70-79, and its backward).  tickets: int [N], ZERO on entry and zero again when the launch is over (the caller
 * keeps one zero-initialised pool and hands out slices; slices of launches that may run concurrently must not overlap).
 * wu: nullable prepared Winograd image (the `_pre` argument).  Partials are still written (stats / stats_sc), outputs [N][Ndim]. */
int smsut_conv2d_fwd_mfma_stats_sc_fin(const float* x, const float* xb /*nullable*/, const float* w, const float* wsc, float* y,
                                       float* ysc, float* stats, float* stats_sc, int* tickets, float* mean, float* rstd,
                                       float* mean_sc, float* rstd_sc, float eps, int N, int H, int W, int Kdim, int Ndim,
                                       const float* wu /*nullable*/, void* stream);
int smsut_conv2d_fwd_mfma_stats_inaff_fin(const float* x, const float* w, float* y, float* stats, const float* mean,
                                          const float* rstd, const float* gamma, const float* beta, float slope, int* tickets,
                                          float* mean_out, float* rstd_out, float eps, int N, int H, int W, int Kdim, int Ndim,
                                          const float* wu /*nullable*/, void* stream);
int smsut_conv2d_dgrad_mfma_bwdstats_fin(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta, float slope,
                                         int* tickets, float* a_mean, float* b_mean, int N, int H, int W, int Kdim, int Ndim,
                                         const float* wu /*nullable*/, void* stream);
/* PAIRED 3x3 weight gradient: gw = wgrad(set A) + wgrad(set B) in ONE launch, for two image sets that went through the same conv
 * (the reference differentiates every generator layer twice per iteration: G(x_real) and the cycle pass G(x_fake),
 * trainer/uganConsisTrainer.py:152,159,179 -- autograd sums the two weight gradients; here they are summed in the kernel's
 * accumulators).  Forms as the single-set entry points, present in both sets or in neither: x2 (virtual cat, ca channels in x),
 * mean / rstd [N, Cin] (x is the raw conv output, lrelu(IN(.)) applied in flight; gamma, beta, slope of the shared layer), gs (fused
 * 1x1 shortcut: gw holds 10 rows).  cat / aff / sc in the queries: 0 / 1 for those forms.  workspace: _ws floats. */
int smsut_conv2d_wgrad_pair_supported(int NA, int NB, int H, int W, int Cin, int Cout, int cat, int aff, int sc);
int64_t smsut_conv2d_wgrad_pair_ws(int NA, int NB, int H, int W, int Cin, int Cout, int cat, int aff, int sc);
int smsut_conv2d_wgrad_pair(const float* xA, const float* x2A /*nullable*/, const float* gyA, const float* gsA /*nullable*/,
                            const float* meanA /*nullable*/, const float* rstdA /*nullable*/, int NA, const float* xB,
                            const float* x2B /*nullable*/, const float* gyB, const float* gsB /*nullable*/,
                            const float* meanB /*nullable*/, const float* rstdB /*nullable*/, int NB, int ca,
                            const float* gamma /*nullable*/, const float* beta /*nullable*/, float slope, float* gw, float* workspace,
                            int H, int W, int Cin, int Cout, void* stream);
/* measurement twin of smsut_conv2d_wgrad_mfma_slabs for the paired launch (plain / input-side-IN form): the kernel alone, slabs left in
 * the workspace; returns the slab count (> 0) or a negative value */
int smsut_conv2d_wgrad_pair_slabs(const float* xA, const float* gyA, const float* meanA /*nullable*/, const float* rstdA /*nullable*/,
                                  int NA, const float* xB, const float* gyB, const float* meanB /*nullable*/,
                                  const float* rstdB /*nullable*/, int NB, const float* gamma /*nullable*/, const float* beta /*nullable*/,
                                  float slope, float* workspace, int H, int W, int Cin, int Cout, void* stream);
int smsut_conv1x1_fwd_cat(const float* xa, const float* xb, int ca, const float* w, float* y, float* stats /*nullable*/,
                          int N, int HW, int Kdim, int Ndim, void* stream);
int smsut_conv1x1_wgrad_cat(const float* xa, const float* xb, int ca, const float* gy, float* gw, float* workspace, int N,
                            int HW, int Cin, int Cout, void* stream);

/* split-output forms: result channels [0, split) -> ya (pixel stride split), [split, Ndim) -> yb (stride Ndim - split).
   They write the data-gradient of a block whose input was cat([up, skip]) (network/blocks.py:49) straight into the two
   gradient tensors.  conv2d form: persistent kernel shapes only (ask _split_supported), any `transposed` form of
   smsut_conv2d_fwd_mfma; conv1x1 form: split % 16 == 0. */
int smsut_conv2d_mfma_split_supported(int N, int H, int W, int Kdim, int Ndim, int split);
int smsut_conv2d_fwd_mfma_split(const float* x, const float* w, float* ya, float* yb, int split, int N, int H, int W,
                                int Kdim, int Ndim, int transposed, void* stream);
int smsut_conv1x1_fwd_split(const float* x, const float* w, float* ya, float* yb, int split, int N, int HW, int Kdim,
                            int Ndim, int transposed, void* stream);

/* fp16-operand convolutions (BASELINE config 5: 512x512 slices, "fp16 MFMA conv path with fp32 IN / loss accumulators"; the
 * reference has no AMP -- SURVEY.md 2.2 -- so these replace the same nn.Conv2d sites as the fp32 entry points: network/blocks.py:10-16,
 * 53-80 at the shapes of network/ugan.py:205-215, config.py:50).  Tensors stay fp32 in HBM; operands are converted to fp16 while a tile
 * is staged into LDS, products accumulate in fp32 (v_mfma_f32_16x16x16_f16), statistics / epilogues / outputs are the fp32 ones.
 * gsc (nullable): device float[2] = {s, 1/s} from smsut_absmax_scale -- a per-tensor power-of-two scale for a GRADIENT input operand
 * (it would underflow fp16 otherwise); the operand is multiplied by s before the conversion, the fp32 result by 1/s.
 * Statistics layout as the fp32 entry points with the tiles of smsut_conv2d_mfma_tiles(..., f16 = 1); `transposed` flags alike. */
int smsut_conv2d_f16_supported(int KS, int Kdim, int Ndim);
int smsut_conv2d_fwd_mfma_f16(const float* x, const float* w, float* y, const float* gsc /*nullable*/, int N, int H, int W,
                              int Kdim, int Ndim, int KS, int transposed, void* stream);
int smsut_conv2d_fwd_mfma_stats_f16(const float* x, const float* w, float* y, float* stats, int N, int H, int W, int Kdim,
                                    int Ndim, int KS, void* stream);
int smsut_conv2d_fwd_mfma_stats_cat_f16(const float* xa, const float* xb, const float* w, float* y, float* stats, int N, int H,
                                        int W, int Kdim, int Ndim, void* stream);
int smsut_conv2d_fwd_mfma_split_f16(const float* x, const float* w, float* ya, float* yb, const float* gsc /*nullable*/,
                                    int split, int N, int H, int W, int Kdim, int Ndim, int transposed, void* stream);
/* fp16 STORAGE of a BasicBlock's internal raw conv outputs y1, y2, s (config 5, "_hs" = half storage): the conv epilogues store
 * fp16 [N,H,W,Ndim] (InstanceNorm partials still from the fp32 accumulators), the consumers below and in the InstanceNorm section
 * read fp16 and compute in fp32.  Persistent-kernel shapes, Kdim in {16, 32, 64}; xb nullable (virtual cat).  Kdim == 8 (first
 * block after the stem): the fused-shortcut entry only, on fp32 operands (the 8-channel form has no fp16 twin), same storage. */
int smsut_conv2d_f16_hs_supported(int N, int H, int W, int Kdim, int Ndim, int cat);
int smsut_conv2d_fwd_mfma_stats_f16_hs(const float* x, const float* xb /*nullable*/, const float* w, void* y16, float* stats, int N,
                                       int H, int W, int Kdim, int Ndim, void* stream);
/* ... whose input is fp16 too (conv2 of the block reading the a1 that smsut_instnorm_fwd_partials_hs2 stored): same operand bits */
int smsut_conv2d_fwd_mfma_stats_f16_hsx(const void* x16, const float* w, void* y16, float* stats, int N, int H, int W, int Kdim,
                                        int Ndim, void* stream);
/* ... reading the RAW fp16 conv1 output and applying lrelu(IN(.)) while staging (half-storage twin of ..._stats_inaff) */
int smsut_conv2d_fwd_mfma_stats_inaff_f16_hsx(const void* y1_16, const float* w, void* y16, float* stats, const float* mean,
                                              const float* rstd, const float* gamma, const float* beta, float slope, int N, int H,
                                              int W, int Kdim, int Ndim, void* stream);
int smsut_conv2d_fwd_mfma_stats_sc_f16_hs(const float* x, const float* xb /*nullable*/, const float* w, const float* wsc, void* y16,
                                          void* ysc16, float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim,
                                          void* stream);
int smsut_conv2d_dgrad_mfma_bwdstats_f16_hs(const float* gy, const float* w, float* gz, float* stats, const void* y1_16,
                                            const float* mean, const float* rstd, const float* gamma, const float* beta,
                                            const float* gsc /*nullable*/, float slope, int N, int H, int W, int Kdim, int Ndim,
                                            void* stream);
/* the fused-shortcut data-gradient with fp16 operands (config 5): gsc = {s, 1/s} of smsut_absmax_scale2(gy, gs) (the two gradients
 * share accumulators, hence ONE scale); Cout in {16, 32}, Cin >= 16, persistent-kernel shapes */
int smsut_conv2d_dgrad_sc_f16_supported(int N, int H, int W, int Cout, int Cin, int split);
int smsut_conv2d_dgrad_mfma_sc_f16(const float* gy, const float* gs, const float* w, const float* wsc, float* gxa,
                                   float* gxb /*nullable*/, const float* gsc, int split, int N, int H, int W, int Cout, int Cin,
                                   void* stream);
int smsut_conv2d_dgrad_mfma_bwdstats_f16(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta,
                                         const float* gsc /*nullable*/, float slope, int N, int H, int W, int Kdim, int Ndim,
                                         void* stream);
/* 3x3 weight gradient, fp16 operands read transposed from LDS (ds_read_b64_tr_b16): H % 8 == 0, W % 16 == 0, Cin % 16 == 0,
 * Cout % 16 == 0.  x2 (nullable): x is the virtual cat([x, x2]) with ca channels in x.  workspace: _ws floats. */
int smsut_conv2d_wgrad_f16_supported(int N, int H, int W, int Cin, int Cout);
int64_t smsut_conv2d_wgrad_f16_ws(int N, int H, int W, int Cin, int Cout);
int smsut_conv2d_wgrad_f16(const float* x, const float* x2 /*nullable*/, int ca, const float* gy, float* gw, float* workspace,
                           const float* gsc /*nullable*/, int N, int H, int W, int Cin, int Cout, void* stream);
/* ... with x stored as fp16 (half storage: conv2's weight gradient reads the activated a1): same operand bits, same result */
int smsut_conv2d_wgrad_f16_xh(const void* x16, const float* gy, float* gw, float* workspace, const float* gsc /*nullable*/, int N,
                              int H, int W, int Cin, int Cout, void* stream);
/* ... with x the RAW fp16 conv1 output, lrelu(IN(.)) applied while staging (half-storage twin of smsut_conv2d_wgrad_mfma_inaff) */
int smsut_conv2d_wgrad_f16_xh_inaff(const void* y1_16, const float* gy, float* gw, float* workspace, const float* gsc /*nullable*/,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta, float slope, int N,
                                    int H, int W, int Cin, int Cout, void* stream);
/* ... plus the 1x1 shortcut's weight gradient in the same pass (fp16 twin of smsut_conv2d_wgrad_mfma_sc): gw10 [10][Cin][Cout],
 * rows 0..8 the 3x3 taps, row 9 the shortcut; gsc from smsut_absmax_scale2(gy, gs) */
int smsut_conv2d_wgrad_sc_f16_supported(int N, int H, int W, int Cin, int Cout);
int64_t smsut_conv2d_wgrad_sc_f16_ws(int N, int H, int W, int Cin, int Cout);
int smsut_conv2d_wgrad_sc_f16(const float* x, const float* x2 /*nullable*/, int ca, const float* gy, const float* gs, float* gw10,
                              float* workspace, const float* gsc, int N, int H, int W, int Cin, int Cout, void* stream);
/* out2[2] = {s, 1/s}, s = 2^k with max|x| * s in [2^13, 2^14] (s = 1 for an all-zero tensor); workspace: _ws floats.
 * _scale2: one scale for two tensors (max over both; the same workspace size serves it) */
int64_t smsut_absmax_scale_ws(int64_t n);
int smsut_absmax_scale(const float* x, int64_t n, float* out2, float* workspace, void* stream);
int smsut_absmax_scale2(const float* x, int64_t n, const float* x2, int64_t n2, float* out2, float* workspace, void* stream);
/* the same scale from maxima the PRODUCING kernels handed over (smsut_restail_bwd_amax, smsut_in_apply_bwd_amax: one slot per
 * workgroup and output tensor): out2 = scale of max(amax[0..n)) -- no pass over the gradient tensor */
int smsut_absmax_finish(const float* amax, int n, float* out2, void* stream);

/* 4x4 stride-1 pad-1 convolutions on the matrix cores: networks.NLayerDiscriminator / PatchDiscriminator (reference
 * network/networks.py:977-1032, 64 -> 128 -> 256 -> 512 channels).  (H, W) = extents of the conv's forward input; the output
 * is (H-1) x (W-1).  transposed = 0: x [N,H,W,Cin] -> y [N,H-1,W-1,Cout]; transposed = 1 (data-gradient): x = gy
 * [N,H-1,W-1,Cout] -> y = gx [N,H,W,Cin].  Weights [4][4][Cin][Cout]; Cin, Cout multiples of 4. */
int smsut_conv2d_k4_supported(int Cin, int Cout);
int smsut_conv2d_k4_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, int transposed,
                        void* stream);
int64_t smsut_conv2d_k4_wgrad_ws(int N, int H, int W, int Cin, int Cout);
int smsut_conv2d_k4_wgrad(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin, int Cout,
                          void* stream);

/* thin 1x1 layers (Cout <= 8, Cin in {8,16,32,64}; reference: the nn.Conv2d heads at network/blocks.py:123-125 and
   network/ugan.py:70): data-gradient gx[P][Cin] = gy[P][Cout] W^T and weight-gradient gw[Cin][Cout], both streaming. */
int smsut_conv1x1_thin_supported(int Cin, int Cout);
int smsut_conv1x1_thin_dgrad(const float* gy, const float* w, float* gx, int N, int HW, int Cin, int Cout, void* stream);
int64_t smsut_conv1x1_thin_wgrad_ws(int Cin);
int smsut_conv1x1_thin_wgrad(const float* x, const float* gy, float* gw, float* workspace, int N, int HW, int Cin,
                             int Cout, void* stream);

/* Tiny-channel convolutions (HBM-bound): 5x5 stems (blocks.py:123, ugan.py:26), D's k4 s2 stem (ugan.py:202), 1x1 heads
 * (blocks.py:166, ugan.py:70).  fwd/dgrad: direct, Cin <= 8, Cout in {4,8,12,16}; wgrad: MFMA with the flattened
 * (tap, ci) index as M, KS*KS*Cin <= 128, Cout <= 16. */
int smsut_conv2d_small_supported(int KS, int Cin, int Cout);
int smsut_conv2d_small_fwd(const float* x, const float* w, const float* bias /*nullable*/, float* y, int N, int H, int W,
                           int Cin, int Ho, int Wo, int Cout, int KS, int stride, int pad, void* stream);
int smsut_conv2d_small_dgrad(const float* gy, const float* w, float* gx, int N, int H, int W, int Cin, int Ho, int Wo,
                             int Cout, int KS, int stride, int pad, void* stream);
int smsut_conv2d_flat_wgrad_supported(int KS, int stride, int Cin, int Cout);
int64_t smsut_conv2d_flat_wgrad_ws(int N, int Ho, int Wo, int Cin, int Cout, int KS);
int smsut_conv2d_flat_wgrad(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin,
                            int Ho, int Wo, int Cout, int KS, int stride, int pad, void* stream);

/* nn.ConvTranspose2d(in, out, kernel_size=2, stride=2, bias=False) -- network/blocks.py:41 (U-Net / seg decoder up path). */
int smsut_convT2x2_mfma_supported(int Cin, int Cout);
int smsut_convT2x2_fwd_mfma(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, void* stream);
int smsut_convT2x2_dgrad_mfma(const float* gy, const float* w, float* gx, int N, int H, int W, int Cin, int Cout,
                              void* stream);
int64_t smsut_convT2x2_wgrad_mfma_ws(int N, int H, int W, int Cin, int Cout);
int smsut_convT2x2_wgrad_mfma(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin,
                              int Cout, void* stream);
/* The same transposed conv through the 1x1 kernels' pixel-shuffle forms (x read once per 64-column slab of the 4 * Cout tap-major
 * columns instead of once per tap; Cout % 16 == 0): forward and weight gradient; the data gradient is already one pass.
 * smsut_convT2x2_ps_supported: Cout == 16 and Cin <= 256 (the forward's weight image of one 64-column slab is 256 B per input
 * channel and stays within 64 KiB of LDS); every other pair belongs to the per-tap kernels above. */
int smsut_convT2x2_ps_supported(int Cin, int Cout);
int smsut_convT2x2_fwd_ps(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, void* stream);
int64_t smsut_convT2x2_wgrad_ps_ws(int N, int H, int W, int Cin, int Cout);
int smsut_convT2x2_wgrad_ps(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin,
                            int Cout, void* stream);

/* bias gradient: out[c] = sum over rows of x[rows][C] */
int64_t smsut_colsum_ws(int64_t rows, int C);
int smsut_colsum(const float* x, float* out, float* workspace, int64_t rows, int C, void* stream);

/* ---------------------------------------------------------------------------------------------- instance norm
 * nn.InstanceNorm2d(C, affine=True) (+ the following LeakyReLU/ReLU) -- network/blocks.py:19-32,57-60,64.
 * _bwd2 is the backward of _bwd, needed because WGAN-GP differentiates D's backward
 * (trainer/uganShp0Trainer.py:127-134, create_graph=True). */
int smsut_in_chunks(int N, int HW, int C); /* workspace = N * chunks * C * 3 floats */
int smsut_in_slabs(int N, int HW, int C);  /* channel slabs of the partial-sum launches (host-only query) */
int smsut_instnorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                       float* workspace, int N, int HW, int C, float eps, float slope, int has_act, void* stream);
int smsut_instnorm_fwd_partials(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                float* rstd, const float* partials, int chunks, int N, int HW, int C, float eps,
                                float slope, int has_act, void* stream);
/* ... reading an fp16 x (half storage, see smsut_conv2d_f16_hs_supported); y stays fp32; C % 4 == 0 */
int smsut_instnorm_fwd_partials_hs(const void* x16, const float* gamma, const float* beta, float* y, float* mean,
                                   float* rstd, const float* partials, int chunks, int N, int HW, int C, float eps,
                                   float slope, int has_act, void* stream);
/* ... and y stored as fp16 as well (consumers: smsut_conv2d_fwd_mfma_stats_f16_hsx, smsut_conv2d_wgrad_f16_xh) */
int smsut_instnorm_fwd_partials_hs2(const void* x16, const float* gamma, const float* beta, void* y16, float* mean,
                                    float* rstd, const float* partials, int chunks, int N, int HW, int C, float eps,
                                    float slope, int has_act, void* stream);
int smsut_in_finalize_fwd(const float* partials, int chunks, float* mean, float* rstd, int N, int HW, int C, float eps,
                          void* stream);
/* the same for TWO partial sets of one (N, HW, C) in one launch (conv2's and the shortcut's statistics of a BasicBlock,
   network/blocks.py:66-80, are both due when the residual tail starts) */
int smsut_in_finalize_fwd2(const float* pa, int chunks_a, float* mean_a, float* rstd_a, const float* pb, int chunks_b, float* mean_b,
                           float* rstd_b, int N, int HW, int C, float eps, void* stream);
/* InstanceNorm backward fed by the dgrad epilogue (smsut_conv2d_dgrad_mfma_bwdstats): finalise the {sum gz, sum gz*xhat}
 * partials into a / b, then gx = gamma*rstd*(gz - a - xhat*b) on the ALREADY masked gz (+ affine gradients, nullable). */
int smsut_in_finalize_bwd(const float* partials, int chunks, float* a_mean, float* b_mean, int N, int HW, int C, void* stream);
int smsut_in_apply_bwd(const float* gz, const float* x, const float* mean, const float* rstd, const float* gamma,
                       const float* a_mean, const float* b_mean, float* gx, float* ggamma /*nullable*/,
                       float* gbeta /*nullable*/, int N, int HW, int C, void* stream);
/* ... that also hands over max|gx|: every workgroup writes the maximum of what it stored into its own slot, amax[0 .. B),
 * B = smsut_amax_blocks(N, HW, C) (no atomics, no zeroing); fp16-operand consumers reduce the slots with smsut_absmax_finish */
int smsut_amax_blocks(int N, int HW, int C);
int smsut_in_apply_bwd_amax(const float* gz, const float* x, const float* mean, const float* rstd, const float* gamma,
                            const float* a_mean, const float* b_mean, float* gx, float* ggamma /*nullable*/,
                            float* gbeta /*nullable*/, float* amax, int N, int HW, int C, void* stream);
/* ... reading an fp16 x (half storage, see smsut_conv2d_f16_hs_supported); amax nullable; C % 4 == 0 */
int smsut_in_apply_bwd_hs(const float* gz, const void* x16, const float* mean, const float* rstd, const float* gamma,
                          const float* a_mean, const float* b_mean, float* gx, float* ggamma /*nullable*/,
                          float* gbeta /*nullable*/, float* amax /*nullable*/, int N, int HW, int C, void* stream);
/* residual tail of BasicBlock (blocks.py:60-79): out = act(IN(y2) + (IN(s) | s)), forward and backward in one pass each */
int smsut_restail_fwd(const float* y2, const float* m2, const float* r2, const float* g2, const float* b2, const float* s,
                      const float* ms /*nullable: identity*/, const float* rs, const float* gs, const float* bs, float* out,
                      int N, int HW, int C, float slope, void* stream);
int smsut_restail_bwd(const float* gout, const float* out, const float* y2, const float* m2, const float* r2,
                      const float* g2, const float* b2 /*nullable*/, const float* s, const float* ms /*nullable*/,
                      const float* rs, const float* gs_, const float* bs /*nullable*/, float* gy2, float* gs, float* a_mean, float* b2_mean, float* bs_mean, float* gg2, float* gb2,
                      float* ggs /*nullable*/, float* gbs /*nullable*/, float* workspace, int N, int HW, int C,
                      float slope, void* stream);
/* ... with the per-image means finalised inside the partial-sum launch (r05; tickets: int [N], zero on entry and on exit): two
 * launches instead of three, same bits */
int smsut_restail_bwd_fin(const float* gout, const float* out, const float* y2, const float* m2, const float* r2,
                      const float* g2, const float* b2 /*nullable*/, const float* s, const float* ms /*nullable*/,
                      const float* rs, const float* gs_, const float* bs /*nullable*/, float* gy2, float* gs, float* a_mean, float* b2_mean, float* bs_mean, float* gg2, float* gb2,
                      float* ggs /*nullable*/, float* gbs /*nullable*/, float* workspace, int* tickets, int N, int HW, int C,
                      float slope, void* stream);
/* half storage: y2 and s are fp16 [N,HW,C]; conv shortcut with both betas (ms, b2, bs non-null); C % 4 == 0; amax nullable */
int smsut_restail_fwd_hs(const void* y2_16, const float* m2, const float* r2, const float* g2, const float* b2, const void* s16,
                         const float* ms, const float* rs, const float* gs, const float* bs, float* out, int N, int HW, int C,
                         float slope, void* stream);
int smsut_restail_bwd_hs(const float* gout, const float* out, const void* y2_16, const float* m2, const float* r2,
                         const float* g2, const float* b2, const void* s16, const float* ms, const float* rs, const float* gs_,
                         const float* bs, float* gy2, float* gs, float* a_mean, float* b2_mean, float* bs_mean, float* gg2,
                         float* gb2, float* ggs, float* gbs, float* workspace, float* amax /*nullable*/, int N, int HW, int C,
                         float slope, void* stream);
/* ... that also hands over max|gy2| in amax[0 .. B) and max|gs| in amax[B .. 2B), B = smsut_amax_blocks(N, HW, C) */
int smsut_restail_bwd_amax(const float* gout, const float* out, const float* y2, const float* m2, const float* r2,
                           const float* g2, const float* b2 /*nullable*/, const float* s, const float* ms /*nullable*/,
                           const float* rs, const float* gs_, const float* bs /*nullable*/, float* gy2, float* gs, float* a_mean, float* b2_mean, float* bs_mean, float* gg2, float* gb2,
                           float* ggs /*nullable*/, float* gbs /*nullable*/, float* workspace, float* amax, int N, int HW,
                           int C, float slope, void* stream);
/* The tail of an ENCODER level's block together with the level's MaxPool2d(2, 2) (r05; /root/reference/network/blocks.py:74-79 +
 * 131-133, network/ugan.py:36-39).  Forward: out [N,H,W,C] (the skip connection), pooled [N,H/2,W/2,C] and idx (one byte per pooled
 * element: where the maximum sat in its window) in ONE pass -- bit-identical to smsut_restail_fwd + smsut_maxpool2_fwd.  Backward:
 * gout = gradient of out through the skip connection, gp = gradient of pooled; the block output's total gradient (what
 * smsut_maxpool2_bwd_add writes) is formed while loading -- bit-identical to that call followed by smsut_restail_bwd / _fin (tickets
 * non-null) / _amax (amax non-null) / _hs (hs != 0: y2, s are _Float16).  Conv shortcut only (ms, b2, bs non-null), C % 4 == 0, H, W even.
 * idx == NULL in both calls: AVERAGE pooling instead (a stride-2 BottleBlock feeding the next one, blocks.py:99-107: its output goes to
 * conv1 and to F.avg_pool2d) -- smsut_avgpool2_fwd's arithmetic forward, gout + 0.25 gp per window pixel backward. */
int smsut_restail_fwd_pool(const void* y2, const float* m2, const float* r2, const float* g2, const float* b2, const void* s,
                           const float* ms, const float* rs, const float* gs, const float* bs, float* out, float* pooled,
                           void* idx /*nullable*/, int N, int H, int W, int C, float slope, int hs, void* stream);
int smsut_restail_bwd_pool(const float* gout, const float* gp, const void* idx /*nullable*/, const void* y2, const float* m2, const float* r2,
                           const float* g2, const float* b2, const void* s, const float* ms, const float* rs, const float* gs_,
                           const float* bs, float* gy2, float* gs, float* a_mean, float* b2_mean, float* bs_mean, float* gg2,
                           float* gb2, float* ggs, float* gbs, float* workspace, int* tickets /*nullable*/, float* amax /*nullable*/,
                           int N, int H, int W, int C, float slope, int hs, void* stream);
int smsut_instnorm_bwd(const float* gy, const float* x, const float* beta /*nullable: no activation*/, const float* mean,
                       const float* rstd, const float* gamma, float* gx, float* a_mean, float* b_mean,
                       float* ggamma /*nullable*/, float* gbeta /*nullable*/, float* workspace, int N, int HW, int C,
                       float slope, void* stream);
/* InstanceNorm + LeakyReLU + AvgPool2d(2) as ONE op (r05): bn1 -> relu -> avgpool of a stride-2 BottleBlock
 * (/root/reference/network/blocks.py:99-107), for passes differentiated once.  Forward from a conv epilogue's statistics partials
 * (as smsut_instnorm_fwd_partials): x [N,H,W,C] raw conv output -> y [N,H/2,W/2,C]; mean / rstd [N,C] are outputs; H, W even.
 * Backward: gyp [N,H/2,W/2,C] = gradient of the POOLED output; other arguments as smsut_instnorm_bwd.  Both are bit-identical to
 * the two-op compositions (instnorm + avgpool2; avgpool2_bwd + instnorm_bwd) without the full-resolution intermediate. */
int smsut_instnorm_pool_fwd_partials(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                                     const float* partials, int chunks, int N, int H, int W, int C, float eps, float slope,
                                     void* stream);
int smsut_instnorm_pool_bwd(const float* gyp, const float* x, const float* beta, const float* mean, const float* rstd,
                            const float* gamma, float* gx, float* a_mean, float* b_mean, float* ggamma /*nullable*/,
                            float* gbeta /*nullable*/, float* workspace, int N, int H, int W, int C, float slope, void* stream);
int smsut_instnorm_bwd2(const float* v, const float* ug /*nullable*/, const float* ub /*nullable*/, const float* gy,
                        const float* x, const float* beta /*nullable: no activation*/, const float* mean, const float* rstd,
                        const float* gamma, const float* a_mean, const float* b_mean, float* d_gy, float* d_x,
                        float* d_gamma, float* workspace, float* scratch /*3*N*C*/, int N, int HW, int C, float slope,
                        void* stream);

/* ---------------------------------------------------------------------------------------------- pointwise / resampling
 * LeakyReLU + residual add (blocks.py:78-79,115-116), nn.Tanh (ugan.py:72-73), conv bias, F.avg_pool2d(x,2)
 * (blocks.py:101,107), nn.MaxPool2d(2,2) (blocks.py:128-134), nn.Upsample(x2, bilinear, align_corners=False)
 * (blocks.py:44), torch.cat (blocks.py:50, ugan.py:159), modality planes (ugan.py:156-157), x_hat (uganConsisTrainer.py:139). */
int smsut_add_act(const float* a, const float* b /*nullable*/, float* y, int64_t n, float slope, void* stream);
int smsut_act_bwd(const float* gy, const float* y, float* gx, int64_t n, float slope, void* stream);
int smsut_tanh_fwd(const float* x, float* y, int64_t n, void* stream);
int smsut_tanh_bwd(const float* gy, const float* y, float* gx, int64_t n, void* stream);
int smsut_bias_add(const float* x, const float* bias, float* y, int64_t rows, int C, void* stream);
int smsut_row_lerp(const float* a, const float* b, const float* alpha, float* out, int64_t rows, int64_t row_len,
                   void* stream);
int smsut_fill(float* out, float v, int64_t n, void* stream);
int smsut_scale(const float* x, const float* scale_dev /*nullable*/, float mul, float* out, int64_t n, void* stream);
/* SGD with momentum + weight decay over many tensors in ONE launch (r05): torch.optim.SGD's rule (dampening 0, no Nesterov; the
 * reference's optimizer, /root/reference/trainer/baseTrainer.py) -- g' = g + wd p; buf = momentum buf + g'; p -= lr buf.  ents: device
 * array of {float* p; const float* g; float* buf; long long n;} (parameter, gradient, momentum buffer: same dense layout); blk_ent /
 * blk_chunk: per block its entry and its chunk (of smsut_sgd_chunk() elements) inside that tensor.  Not for the first step (the buffers
 * must exist). */
int smsut_sgd_momentum_multi(const void* ents, const int* blk_ent, const int* blk_chunk, int nblocks, float lr, float momentum, float wd,
                             void* stream);
int smsut_sgd_chunk(void);
int smsut_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int smsut_maxpool2_bwd(const float* gy, const float* x, float* gx, int N, int H, int W, int C, void* stream);
/* gx = maxpool2_bwd(gy; x) + add: pooled-path and skip-connection gradients of an encoder level (blocks.py:131-133) in one pass */
int smsut_maxpool2_bwd_add(const float* gy, const float* x, const float* add, float* gx, int N, int H, int W, int C,
                           void* stream);
int smsut_avgpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int smsut_avgpool2_bwd(const float* gy, float* gx, int N, int H, int W, int C, void* stream);
/* Device-side joint augmentation (rotate + elastic + random-resized-crop of data_loader/externalTransforms.py:45-90 as one
 * resampling pass): source position = aff[n] * (xo, yo, 1) + bilinear(ctrl[n][2][P][P]); image bilinear, labels nearest,
 * zeros outside.  img [N,H,W], msk [N,H,W] (nullable), aff [N][6], ctrl nullable when P == 0. */
int smsut_warp_joint(const float* img, const int64_t* msk, const float* aff, const float* ctrl, float* oimg,
                     int64_t* omsk, int N, int H, int W, int Ho, int Wo, int P, void* stream);
/* JointElasticDeform's resampling (reference data_loader/externalTransforms.py:69-90 -> elasticdeform.deform_random_grid(order = [0, 0])):
   coef [N][2][P][P] = cubic B-spline coefficients (mirror boundary) of the P x P control displacements (dy, dx), first / last control
   point on the first / last pixel; image and label map sampled at (y + dy, x + dx) with order 0, constant 0 outside. */
int smsut_elastic_deform(const float* img, const int64_t* msk, const float* coef, float* oimg, int64_t* omsk, int N, int H,
                         int W, int P, void* stream);
/* Photometric augmentation (reference data_loader/baseLoader.py:102-109: ColorJitter(0.4, 0.4, 0.4, 0.125), then
 * RandomGammaCorrection, on mode-L 8-bit slices; saturation and hue are the identity there).  img / out: [N][HW] fp32, img on the
 * [0, 1] scale; a pixel is first quantised to the level PIL would hold, floor(x * 255 + 0.5) clamped to 0..255.  Per slice the chain
 * brightness = blend(0, v, b), contrast = blend(m, v, c) (m = int(mean + 0.5) of the slice as it is when that step runs; blend =
 * PIL's ImagingBlend: fp32 multiply, fp32 add, truncation, clipped when the factor leaves [0, 1]) and the gamma table collapses into
 * one 256-entry table built from the slice's histogram; the output is out_tab[final level] (out_tab: 256 floats chosen by the
 * caller -- level / 255, or the normalised values).  Bit-reproducible (integer adds, fixed-order fp32); pinned to Pillow's outputs.
 *   smsut_photo_parts(HW) = G, the histogram kernel's workgroups per slice (at most 16).
 *   smsut_photo_hist: part [N][G][256] int32, every row written by its own workgroup (no zeroing needed), summed by the next call.
 *   smsut_photo_apply: params [N][4] = {order (0: brightness first, 1: contrast first), b, c, gamma drawn (0 / 1)};
 *     part == NULL: no jitter (gamma only, no histogram launch needed); gtab: uint8 [N][256] gamma tables, read for the slices whose
 *     flag is set, NULL: no gamma.  out must not alias img.  N <= 65535. */
int smsut_photo_parts(int HW);
int smsut_photo_hist(const float* img, int* part, int N, int HW, void* stream);
int smsut_photo_apply(const float* img, const int* part /*nullable*/, const float* params, const uint8_t* gtab /*nullable*/,
                      const float* out_tab, float* out, int N, int HW, void* stream);
int smsut_bilinear2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int smsut_bilinear2_bwd(const float* gy, float* gx, int N, int H, int W, int C, void* stream);
/* networks.py building blocks of ResnetGenerator / NLayerDiscriminator: reflection / replication /
 * zero padding and cropping (mode 0 zero, 1 reflect, 2 replicate; (oy, ox) = (top, left) pad, negative = crop) and the
 * anti-aliased Downsample(filt 3, stride 2, reflect) -- networks.py:37-60,95-105.  Upsample(filt 4, 'repl', stride 2)
 * (networks.py:73-93) is arithmetically the x2 bilinear kernel above. */
int smsut_window_fwd(const float* src, float* dst, int N, int Hs, int Ws, int Hd, int Wd, int C, int oy, int ox, int mode,
                     void* stream);
int smsut_window_bwd(const float* gdst, float* gsrc, int N, int Hs, int Ws, int Hd, int Wd, int C, int oy, int ox, int mode,
                     void* stream);
int smsut_blurdown_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int smsut_blurdown_bwd(const float* gy, float* gx, int N, int H, int W, int C, void* stream);
/* torch.cat([a, b], 1) (dir 0) and its backward split (dir 1; a / b nullable) in one pass over the wide tensor. */
int smsut_concat2(float* a, int Ca, float* b, int Cb, float* y, int64_t P, int dir, void* stream);
int smsut_copy_channels(const float* src, int Cs, int src_off, float* dst, int Cd, int dst_off, int Cc, int64_t P,
                        void* stream);
int smsut_modal_planes(const float* x, const float* m, float* out, int N, int64_t HW, int Cx, int M, void* stream);

/* ---------------------------------------------------------------------------------------------- losses
 * DiceAndCrossEntropyLoss / SoftDiceLoss (misc/loss.py:8-63): stage 1 = per-class {tp, sum_p, count} + CE sum,
 * (optional all-reduce by the caller under data parallelism), stage 2 = scalar; G = 1 batch dice, G = N per sample. */
int64_t smsut_dicece_ws(int N, int64_t HW, int C, int G);
int smsut_dicece_stats(const float* logits, const int64_t* labels, float* stats, float* ce_sum, float* workspace, int N,
                       int64_t HW, int C, int G, void* stream);
int smsut_dicece_final(const float* stats, const float* ce_sum, float* out /*3*/, int G, int C, double npix_total,
                       float w_dc, float w_ce, void* stream);
int smsut_dicece_bwd(const float* logits, const int64_t* labels, const float* stats, const float* gout, float* glogits,
                     int N, int64_t HW, int C, int G, double npix_total, float w_dc, float w_ce, void* stream);
/* -/+ mean(out_src) (uganConsisTrainer.py:130,136,154), mean|a-b| (:162), F.cross_entropy on [B,n_modal] (:131,155),
 * gradient penalty norm term (uganShp0Trainer.py:131-134). */
int64_t smsut_sum_ws(int64_t n, int rows);
int smsut_sum(const float* a, float* out, float* workspace, int64_t n, double scale, void* stream);
int smsut_l1_fwd(const float* a, const float* b, float* out, float* workspace, int64_t n, void* stream);
int smsut_l1_bwd(const float* a, const float* b, const float* gout, float* ga /*nullable*/, float* gb /*nullable*/,
                 int64_t n, void* stream);
/* mean((softmax(a) - softmax(b))^2) over [P pixels][C] NHWC logits, gradient to a only: the mean-teacher consistency
 * term (trainer/meanTeacherTrainer.py:113-131).  workspace: smsut_sum_ws(P, 1) floats. */
int smsut_softmax_mse_fwd(const float* a, const float* b, float* out, float* workspace, int64_t P, int C, void* stream);
int smsut_softmax_mse_bwd(const float* a, const float* b, const float* gout, float* ga, int64_t P, int C, void* stream);
/* labels[p] = argmax_c logits[p][c] (first maximum): pseudo labels (uganConsisTrainer.py:45-53, crossPseTrainer.py:122-127)
 * and the prediction map of validate_epoch (uganShp0Trainer.py:262-266). */
int smsut_argmax_channels(const float* logits, int64_t* labels, int64_t P, int C, void* stream);
int smsut_gp_fwd(const float* dydx, float* out, float* norms, float* workspace, int rows, int64_t n, void* stream);
int smsut_gp_bwd(const float* dydx, const float* norms, const float* gout, float* g, int rows, int64_t n, void* stream);
int smsut_ce_rows_fwd(const float* z, const int64_t* tgt, float* out, int B, int C, void* stream);
int smsut_ce_rows_bwd(const float* z, const int64_t* tgt, const float* gout, float* gz, int B, int C, void* stream);
/* PatchSampleF gather (ugan.py:318-327), networks.Normalize (networks.py:234-243), PatchNCELoss (patchnce.py:13-51). */
int smsut_gather_rows(const float* feat, const int64_t* ids, float* out, int B, int64_t HW, int C, int P, void* stream);
int smsut_scatter_rows(const float* gout, const int64_t* ids, float* gfeat, int B, int64_t HW, int C, int P,
                       void* stream);
int smsut_l2norm_fwd(const float* x, float* y, float* norms, int rows, int C, void* stream);
int smsut_l2norm_bwd(const float* gy, const float* x, const float* norms, float* gx, int rows, int C, void* stream);
int smsut_patchnce_fwd(const float* q, const float* k, float* loss, float* probs, int rows, int np, int dim, float T,
                       void* stream);
int smsut_patchnce_bwd(const float* gloss, const float* probs, const float* k, float* gq, int rows, int np, int dim,
                       float T, void* stream);

/* ---------------------------------------------------------------------------------------------- CoraNet heads
 * trainer/coraNetTrainer.py after the logits.  The 3L+1 channels of the U-Net output [N][HW][3L+1] are three (L+1)-class heads
 * h0, h1, h2 that share the background logit (channel 0; head k owns channels 1+kL .. (k+1)L), 1 <= L <= 10.  No head is ever
 * materialised: every pass reads a pixel's logits once and the backward passes write its 3L+1 gradients once.
 * workspace (both statistics passes): smsut_cora_ws(N, HW, L) floats.
 *
 * Supervised loss (:288-301), two stages like smsut_dicece_*:
 *   S = ([w_dc Dice_batch(h0, y) + w_ce CE(h0, y)] + CE_{w_con}(h1, y) + CE_{w_rad}(h2, y)) / 4,
 *   CE_w = sum_p w[y_p] nll_p / sum_p w[y_p] (torch CrossEntropyLoss(weight=w)); w_con, w_rad: device arrays of L+1 floats.
 *   stats[3(L+1)+3] = head-0 {tp, sum_p, count}[L+1], sum nll(h0), sum w_con[y] nll(h1), sum w_rad[y] nll(h2): sums over the batch, so
 *   under data parallelism the caller all-reduces them between the stages and passes the global pixel count.
 *   final: out[4] = [S, w_dc dice + w_ce ce of head 0, CE_con, CE_rad];  bwd: glogits = gout[0] * dS/dlogits.
 * Pseudo-labelled loss (:304-347) of student logits z against pseudo labels q, mask m in {0,1} and teacher logits e:
 *   certain   = (sum_p m_p nll_p(h0, q) / (sum_p m_p + 1e-16) + Dice_per_sample(h0, q)) / 2
 *   uncertain = (cw / 3) sum_k [sum_p (1 - m_p) |softmax(h_k(z)) - softmax(h_k(e))|^2 / (sum_p (1 - m_p) + 1e-16)]
 *   stats[N][3(L+1)+4] per sample = head-0 {tp, sum_p, count}[L+1] against q, sum m nll, sum m, the masked squared-difference sum over
 *   the three heads, sum (1 - m).  final: out[2] = [certain, uncertain];  bwd: gz = gout[0] d certain/dz + gout[1] d uncertain/dz
 *   (no gradient to e).
 * smsut_cora_pseudo: q[p] = argmax(h0) (int64), m[p] = (argmax(h1) == argmax(h2)) (0/1), first maximum wins (:189-208). */
int64_t smsut_cora_ws(int N, int64_t HW, int L);
int smsut_cora_sup_stats(const float* logits, const int64_t* labels, const float* w_con, const float* w_rad, float* stats,
                         float* workspace, int N, int64_t HW, int L, void* stream);
int smsut_cora_sup_final(const float* stats, const float* w_con, const float* w_rad, float* out /*4*/, int L, double npix_total,
                         float w_dc, float w_ce, void* stream);
int smsut_cora_sup_bwd(const float* logits, const int64_t* labels, const float* stats, const float* w_con, const float* w_rad,
                       const float* gout, float* glogits, int N, int64_t HW, int L, double npix_total, float w_dc, float w_ce,
                       void* stream);
int smsut_cora_semi_stats(const float* z, const float* e, const int64_t* q, const float* m, float* stats, float* workspace, int N,
                          int64_t HW, int L, void* stream);
int smsut_cora_semi_final(const float* stats, float* out /*2*/, int N, int L, float cw, void* stream);
int smsut_cora_semi_bwd(const float* z, const float* e, const int64_t* q, const float* m, const float* stats, const float* gout /*2*/,
                        float* gz, int N, int64_t HW, int L, float cw, void* stream);
int smsut_cora_pseudo(const float* z, int64_t* q, float* m, int64_t P, int L, void* stream);
/* ema = alpha * ema + beta * p over many tensors in one launch (:168-174; beta = 1 - alpha).  ents: device array of
 * {float* ema, const float* p, int64 n}; blk_ent / blk_chunk: for every block its entry and its chunk of smsut_ema_chunk() elements
 * inside that entry's tensor, as smsut_sgd_momentum_multi. */
int smsut_ema_multi(const void* ents, const int* blk_ent, const int* blk_chunk, int nblocks, float alpha, float beta, void* stream);
int smsut_ema_chunk(void);

/* ---------------------------------------------------------------------------------------------- dual-task consistency (DTC)
 * network/dtc.py's two heads (tanh level-set regression t, segmentation logits z) need, per iteration, the normalised signed distance
 * map of every class of every labelled slice, and a two-term loss.  csrc/dtc.hip.
 *
 * smsut_edt_sq: labels int64 [B][H][W] -> d2 int32 [B][C][H][W].  With P = (label == c): d2 = the exact squared Euclidean distance from
 *   the pixel to the nearest pixel whose membership in P differs from its own (members: nearest non-member = scipy's
 *   distance_transform_edt(P)^2; non-members: nearest member = distance_transform_edt(~P)^2).  Outside the image is nothing; d2 = 0
 *   everywhere where P is empty or full.  1 <= H, W <= 512, 1 <= C <= 16, B * C <= 65535; otherwise SMSUT_EINVAL (smsut_sdf_ws: -1).
 *   workspace: smsut_sdf_ws(B, C, H, W) floats; it keeps the two per-image maxima for smsut_sdf_final.  status: one device int that a
 *   label outside [0, C) sets to 1 (such a pixel is a member of no class); it is never cleared or read here.
 * smsut_sdf_final: sdf fp32 [B][H][W][C] (NHWC) = +sqrt(d2 / max of d2 over the non-members) on non-members,
 *   -sqrt(d2 / max over the members) on members, exactly 0 on the inner boundary (members with d2 == 1), exactly +1 everywhere where P is
 *   empty and -1 where P is full.  One fp64 division and square root, rounded to fp32 once.
 * smsut_dtc_loss_fwd: t, z fp32 [N][HW][C], sdf [B][HW][C] pairing with the first B slices (1 <= B <= N), 1 <= C <= 16:
 *   out[2] = [mean over B C HW of (t - sdf)^2, mean over N C HW of (sigmoid(-k t) - softmax(z)_c)^2]; workgroup partials in double,
 *   summed in a fixed order (bitwise reproducible); finite for every t in [-1, 1] and any k.
 *   workspace: the memory of smsut_dtc_ws(N, HW) floats, 8-byte aligned; the kernels keep doubles in it (hence void*).
 * smsut_dtc_loss_bwd: gt = gout[0] d out[0]/dt + gout[1] d out[1]/dt and gz = gout[1] d out[1]/dz in one launch (no gradient to sdf). */
int64_t smsut_sdf_ws(int B, int C, int H, int W);
int smsut_edt_sq(const int64_t* labels, int* d2, float* workspace, int* status, int B, int C, int H, int W, void* stream);
int smsut_sdf_final(const int64_t* labels, const int* d2, const float* workspace, float* sdf, int B, int C, int H, int W, void* stream);
int64_t smsut_dtc_ws(int N, int64_t HW);
int smsut_dtc_loss_fwd(const float* t, const float* z, const float* sdf, float* out /*2*/, void* workspace, int N, int B, int64_t HW,
                       int C, float k, void* stream);
int smsut_dtc_loss_bwd(const float* t, const float* z, const float* sdf, const float* gout /*2*/, float* gt, float* gz, int N, int B,
                       int64_t HW, int C, float k, void* stream);

/* ---------------------------------------------------------------------------------------------- test-phase metrics
 * The `-p test` table of trainer/baseTrainer.py:254-318: get_all_matrix (misc/utils.py:206-283) cleans every predicted volume
 * with connected_components (misc/utils.py:18-36, skimage measure.label connectivity=2) in 3-D and then slice by slice, and
 * scores each organ with medpy's dc and assd (erosion connectivity 1; in voxels, or with the _sp forms under a voxel
 * spacing).  Volumes are dense uint8 [D][H][W]; a 2-D image is D = 1.  Workspaces are BYTES, from the matching *_ws query (-1 there: invalid arguments).
 *
 * smsut_cc_filter: out[v] = c where v lies in a component of class c in 1..n_cls (label value c; different classes never merge)
 *   whose size S satisfies (double)S > 0.1 * (double)F, F = the class's voxel count (per_slice = 1: in that slice), else 0 --
 *   values above n_cls become 0.  per_slice = 0: 3-D 18-neighbourhood; 1: each z slice alone, 8-neighbourhood.  out may alias in.
 *   The first int of the workspace is an error word: 0 after a good run, non-zero if a union-find loop hit its bound of D*H*W
 *   iterations (a bug, reported instead of hanging; out is then undefined).  D*H*W < 2^31, 1 <= n_cls <= 255.
 * smsut_surface_stats: out = double[n_cls][7], per label l = 1..n_cls of P = (pred == l), G = (gt == l):
 *   {|P & G|, |P|, |G|, border voxels of P, sum over them of the distance to the nearest border voxel of G,
 *    border voxels of G, sum over them of the distance to the nearest border voxel of P}
 *   border = mask XOR erosion(mask) with the 6-neighbour cross (4-neighbour when planar = 1, which needs D = 1) and the array
 *   faces outside the mask; distances are exact Euclidean in voxels (fp64 sqrt of integer squared distances), reduced in a
 *   fixed order: the result is bitwise reproducible.  A distance sum is meaningless when the other mask is empty.
 *   D, H, W <= 4096.
 * smsut_surface_hd: out = double[n_cls][6], per label, every entry an integer (medpy's hd / hd95 ingredients):
 *   {border voxels of P, border voxels of G, largest squared distance from a border voxel of P to G's border, the same from G
 *    to P, lo2, hi2}: with the squared distances of both directions pooled into one multiset of n values, lo2 is the one at
 *   sorted rank lo = floor((double)(n - 1) * quantile) (one fp64 product) and hi2 the one at rank min(lo + 1, n - 1).  The four
 *   distance entries are -1 when either mask is empty.  Borders, planar, limits and exactness as smsut_surface_stats; selected
 *   through integer histograms (bitwise reproducible); 0 < quantile <= 1.  Its own workspace query.
 * smsut_surface_stats_sp, smsut_surface_hd_sp (workspaces from smsut_surface_sp_ws, smsut_surface_hd_sp_ws): the two above with
 *   a voxel spacing (sz, sy, sx), ordered like the array axes, in any unit; sz is ignored when planar = 1.  Each spacing must lie
 *   in [1e-100, 1e100] (so every squared distance, up to 3 * 4095^2 * s^2, is a normal finite double); otherwise the status is
 *   SMSUT_EINVAL and nothing is launched.  Squared distances are fp64: min over the border voxels of
 *   (sx*sx) * dx^2 + (sy*sy) * dy^2 + (sz*sz) * dz^2, the weights formed once, every product rounded before it is added (no
 *   fma), the sums in x, y, z order.  At spacing (1, 1, 1) every output equals the unit entry point's bit for bit; scaling all
 *   spacings by a power of two scales the distances by exactly it.  smsut_surface_stats_sp: the [n_cls][7] layout, distances in
 *   the spacing's unit, the same fixed-order reduction (bitwise reproducible).  smsut_surface_hd_sp: the [n_cls][6] layout; the
 *   four distance entries are fp64 SQUARED physical distances, each exactly one of the computed values (an exact five-level
 *   radix select over the doubles' bit patterns, integer atomics only), -1 when either mask is empty. */
int64_t smsut_cc_ws(int D, int H, int W, int n_cls, int per_slice);
int smsut_cc_filter(const uint8_t* in, uint8_t* out, void* workspace, int D, int H, int W, int n_cls, int per_slice,
                    void* stream);
int64_t smsut_surface_ws(int D, int H, int W, int n_cls, int planar);
int smsut_surface_stats(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                        int planar, void* stream);
int64_t smsut_surface_hd_ws(int D, int H, int W, int n_cls, int planar);
int smsut_surface_hd(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                     int planar, double quantile, void* stream);
int64_t smsut_surface_sp_ws(int D, int H, int W, int n_cls, int planar);
int smsut_surface_stats_sp(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                           int planar, double sz, double sy, double sx, void* stream);
int64_t smsut_surface_hd_sp_ws(int D, int H, int W, int n_cls, int planar);
int smsut_surface_hd_sp(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                        int planar, double quantile, double sz, double sy, double sx, void* stream);
/* Validation on the device (csrc/evaluate.hip): the prediction map of a batch of logits and the Dice overlap counts of its slices in
 * one pass.  logits: NHWC [N][HW][C] fp32; labels: int64 [N][HW]; vol: int [N], the volume slot of each slice.
 *   prediction p = the first maximum of channels 0 .. K-1 of the pixel's C-float row (K < C: head 0 of CoraNet's 3L+1 channels),
 *     by smsut_argmax_channels' comparison: the first maximum wins, a NaN wins.  pred: uint8 [N][HW], nullable.
 *   counts: int64 [V][K][3] = {|P & G|, |P|, |G|} per (volume, class), ACCUMULATED and never zeroed here: counts[vol][p][1] += 1;
 *     a label g in 0 .. K-1 adds to counts[vol][g][2] and, when p == g, to counts[vol][p][0]; any other label counts nowhere.
 *   A slice with vol[n] < 0 or vol[n] >= V is skipped: no count, its pred bytes untouched.
 * Integer arithmetic only (register counters, a block reduction, one 64-bit integer atomic add per non-zero (class, statistic) and
 * workgroup): bitwise reproducible.  Needs 1 <= K <= C, K <= 32, HW >= 1, V >= 1, N <= 65535, otherwise SMSUT_EINVAL and nothing
 * is launched; N == 0 returns SMSUT_OK without a launch. */
int smsut_eval_overlap(const float* logits, const int64_t* labels, const int* vol, int64_t* counts, uint8_t* pred /*nullable*/, int N,
                       int64_t HW, int C, int K, int V, void* stream);
/* Translation metrics of the test phase (csrc/similarity.hip): SSIM, squared and absolute error of two image batches in one pass.
 * a, b: fp32 [n][h][w], dense.  out: double [n][3], WRITTEN (not accumulated), per slice
 *   {sum of SSIM over its (h-10)(w-10) window centres, SE = sum over all h w pixels of (a-b)^2, AE = sum of |a-b|}.
 *   SSIM (Wang et al. 2004): the 11x11 window w (x) w, w[k] = exp(-k^2 / (2 1.5^2)), k = -5 .. 5, normalised to sum 1; population
 *   moments mu_a, mu_b, s_a^2 = E[a^2] - mu_a^2, s_b^2, s_ab = E[ab] - mu_a mu_b at every centre at least 5 pixels from each edge;
 *   ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)), C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2.
 *   Window sums (11 fp32 weights, fixed tap order) and the per-centre value are fp32; SE and AE convert each pixel to fp64 before
 *   the subtraction; every sum over centres or pixels is fp64 in a fixed order, without atomics: bitwise reproducible.
 *   A NaN or Inf in one slice stays in that slice's three outputs.
 * workspace: smsut_image_similarity_ws(n, h, w) bytes (per-workgroup partials), -1 for arguments outside the limits.
 * Limits: 1 <= n <= 65535, 11 <= h, w <= 4096, data_range finite and positive; otherwise SMSUT_EINVAL and nothing is launched. */
int64_t smsut_image_similarity_ws(int n, int h, int w);
int smsut_image_similarity(const float* a, const float* b, double* out, void* workspace, int n, int h, int w, double data_range,
                           void* stream);

/* Volume preparation (csrc/volume.hip): raw scanner volume -> the processed grid the package trains and tests on.  Arrays are dense
 * [D][H][W] = [z][y][x]; every axis 1 .. 4096, at most 2^31 - 1 voxels; otherwise SMSUT_EINVAL (the `_ws` queries: -1) and nothing
 * is launched.  Nothing reads back to the host; every kernel runs on `stream`.
 *
 * Index map, shared by both resamplers: output index i of an axis reads the source at the continuous index
 *   x = ((i + start) * num) / den - offset      (fp64: an exact integer product, one division, one subtraction)
 * and the point is inside iff -0.5 <= x < n - 0.5 on every axis (n = the source's length); outside points are written as 0.
 * num, den in 1 .. 4096; start, offset in 0 .. 4096.
 *
 * smsut_bspline_coefficients: the cubic B-spline interpolation coefficients of vol under whole-sample mirror boundaries (index
 *   -1 -> 1, n -> n - 2) on every axis: per axis the solution of A c = v, A[i][mirror(i + k)] += (1/6, 4/6, 1/6), k = -1, 0, 1; an
 *   axis of length 1 is copied.  Computed as the symmetric FIR h[k] = -6 z / (1 - z^2) z^|k|, z = sqrt(3) - 2, |k| <= 15, over the
 *   mirrored line, each output one fixed-order fp64 sum rounded once to fp32 per axis.  out must not alias vol.
 *   workspace: smsut_bspline_ws(d, h, w) bytes (one intermediate volume).
 * smsut_resample_volume: out[od][oh][ow] = the cubic B-spline with coefficients coef[sd][sh][sw] at the mapped points: four weights
 *   per axis on the mirror-folded indices floor(x) - 1 .. floor(x) + 2, fp64 accumulation in the order z (y (x)), rounded once.
 * smsut_resample_labels: nearest neighbour, source index floor(x + 0.5) (halves round up); lut: 256 bytes applied to the SOURCE
 *   value, or null.
 *   workspace of both: smsut_resample_ws(od, oh, ow) bytes (the per-axis index / weight tables). */
int64_t smsut_bspline_ws(int d, int h, int w);
int smsut_bspline_coefficients(const float* vol, float* out, void* workspace, int d, int h, int w, void* stream);
int64_t smsut_resample_ws(int od, int oh, int ow);
int smsut_resample_volume(const float* coef, float* out, void* workspace, int sd, int sh, int sw, int od, int oh, int ow, int num_z,
                          int num_y, int num_x, int den_z, int den_y, int den_x, int start_z, int start_y, int start_x, int off_z,
                          int off_y, int off_x, void* stream);
int smsut_resample_labels(const uint8_t* lab, uint8_t* out, void* workspace, const uint8_t* lut /*nullable*/, int sd, int sh, int sw,
                          int od, int oh, int ow, int num_z, int num_y, int num_x, int den_z, int den_y, int den_x, int start_z,
                          int start_y, int start_x, int off_z, int off_y, int off_x, void* stream);
/* Exact order statistics: out[k] = the value at sorted rank r_k (0-based, ascending) of the n FINITE floats v, k < nr, 1 <= nr <= 8,
 * 0 <= r_k < n <= 2^31 - 1 (ranks past nr are ignored).  MSD radix select over order-preserving 32-bit keys (-0.0 sorts below
 * +0.0), four 8-bit levels, integer atomics only: exact and independent of the order of arrival.  NaN / Inf: outside the contract.
 * workspace: smsut_order_statistics_ws(n, nr) bytes, zeroed by the call. */
int64_t smsut_order_statistics_ws(int64_t n, int nr);
int smsut_order_statistics(const float* v, float* out, void* workspace, int64_t n, int nr, int64_t r0, int64_t r1, int64_t r2,
                           int64_t r3, int64_t r4, int64_t r5, int64_t r6, int64_t r7, void* stream);
/* out[i] = (uint8)((min(max(v[i], lo), hi) - lo) / (hi - lo) * 255.0f), (lo, hi) = bounds[0..1] read on the device; fp32 in this
 * order with IEEE division, converted by truncation; all zeros when hi == lo.  1 <= n <= 2^31 - 1. */
int smsut_window_u8(const float* v, const float* bounds, uint8_t* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------- test-time augmentation
 * Inference with flipped / rotated copies of a slice and with ensembles (csrc/tta.hip; predict.py).  The reference has no inference
 * entry point: this replaces the flip / rot90 / softmax / stack / mean / max chain an inference script would build from torch.
 * Transform g = r + 4 f, r in 0..3, f in 0..1, on the last two axes of a slice x [H][W]:
 *   F_g(x) = torch.rot90(f ? torch.flip(x, [-1]) : x, k = r, dims = (-2, -1));  odd r needs H == W.
 * `transforms` (T ints in 0..7) and `members` (T device pointers) are HOST arrays, read before the call returns.
 *
 * smsut_tta_expand: img uint8 [N][H][W] -> out fp32 [T][N][1][H][W]; member t = F_{g_t}(slice), converted as the loader converts a
 *   slice on the device (data_loader/inTurnLoader.py:166,173: `.float().div_(255.0).sub_(0.5).div_(0.5)`, where torch divides a
 *   device tensor by a host scalar as a product with the scalar's reciprocal): ((float)u * (float)(1.0 / 255.0) - 0.5f) * 2.0f,
 *   in fp32, each of the three steps rounded on its own, in this order -- bitwise what that torch expression gives.
 * smsut_tta_merge: members[t]: logits fp32 [N][H][W][C] (NHWC) of the network run on member t of smsut_tta_expand (repeats of a
 *   g are allowed: several networks), 4-byte aligned, read in place, each logit once.  Classes = channels 0 .. K-1.  Per output
 *   pixel q, member by member in list order, all in fp32: p = the position of q in F_{g_t}; m = max_k z[p][k];
 *   e_k = expf(z[p][k] - m); s = e_0 + e_1 + ... in channel order; acc_k += e_k / s.  Then mean_k = acc_k / (float)T;
 *   pred uint8 [N][H][W] = the first maximum of mean_k by smsut_argmax_channels' comparison (the first maximum wins, a NaN wins);
 *   conf (nullable) fp32 [N][H][W] = mean_pred; prob (nullable) fp32 [N][H][W][K] = mean_k.  No atomics, no cross-thread sums:
 *   bitwise reproducible.
 * Limits (otherwise SMSUT_EINVAL and nothing is launched; N == 0 returns SMSUT_OK without a launch): */
#define SMSUT_TTA_MAX_MEMBERS 16   /* 1 <= T <= 16 */
#define SMSUT_TTA_MAX_CLASSES 32   /* 1 <= K <= min(C, 32) */
#define SMSUT_TTA_MAX_SLICES 65535 /* N <= 65535 */
#define SMSUT_TTA_MAX_DIM 16384    /* 1 <= H, W <= 16384 */
int smsut_tta_expand(const uint8_t* img, float* out, const int* transforms, int T, int N, int H, int W, void* stream);
int smsut_tta_merge(const float* const* members, const int* transforms, uint8_t* pred, float* conf /*nullable*/,
                    float* prob /*nullable*/, int T, int N, int H, int W, int C, int K, void* stream);
/* smsut_tta_uncertain (csrc/uncertainty.hip): the merge's pass with the uncertainty of the prediction.  Inputs, limits, tiles and
 *   staging are smsut_tta_merge's (C <= 8 and K in 2..5: 32 x 32 tiles staged through LDS; other C <= 32: 16 x 16 staged; C > 32:
 *   16 x 16, rows read in place); pred and conf are bitwise what smsut_tta_merge writes.  Per output pixel, all fp32, member by
 *   member in list order: z = member[F_g(q)][0..K-1]; a_t = the first maximum of z (smsut_argmax_channels' comparison);
 *   m = max_k z_k; e_k = expf(z_k - m); s = e_0 + e_1 + ... in channel order; q_k = e_k / s; acc_k += q_k;
 *   h_t = -(q_0 logf(q_0 + 1e-6f) + q_1 logf(q_1 + 1e-6f) + ...), terms added in channel order; hs += h_t.  Then
 *   mean_k = acc_k / (float)T; pred = the first maximum of mean; conf = mean_pred;
 *   entropy = H = -(mean_0 logf(mean_0 + 1e-6f) + ...) in channel order; EH = hs / (float)T; mutual = fmaxf(H - EH, 0.f);
 *   votes = #{t : a_t == pred}.  pred uint8, conf / entropy / mutual fp32, votes uint8, all [N][H][W]; all nullable but pred.
 *   counts (nullable) int64 [K][2 T + 4], contiguous, ADDED into (the caller zeroes it once per volume); row k =
 *   {V, ALL, ANY, HSUM, V_0 .. V_{T-1}, I_0 .. I_{T-1}}: V pixels with pred == k; ALL pixels where every a_t == k; ANY pixels where
 *   some a_t == k; V_t pixels with a_t == k; I_t pixels with a_t == k and pred == k; HSUM the sum over pixels with pred == k of
 *   (int64)rintf(H * 1048576.f), a pixel whose H is not finite adding nothing (it still counts in the other slots).  Integer
 *   atomics only: bitwise reproducible. */
int smsut_tta_uncertain(const float* const* members, const int* transforms, uint8_t* pred, float* conf /*nullable*/,
                        float* entropy /*nullable*/, float* mutual /*nullable*/, uint8_t* votes /*nullable*/,
                        int64_t* counts /*nullable*/, int T, int N, int H, int W, int C, int K, void* stream);

/* ---------------------------------------------------------------------------------------------- sliding-window inference
 * A slice larger than the window the network was trained on is predicted window by window, and the windows' class probabilities are
 * blended on the slice's grid (csrc/window.hip; predict.py: Predictor.predict_windows).  The reference has no inference entry
 * point: this replaces the zeros / strided multiply-add per window / division / argmax chain one would build from torch.
 * smsut_window_blend: tiles[iy * nx + ix]: mean class probabilities fp32 [N][wh][ww][K] (the `prob` of smsut_tta_merge), 4-byte
 *   aligned (a view that starts anywhere in its allocation), read in place; the tile covers rows ys[iy] .. ys[iy] + wh - 1 and
 *   columns xs[ix] .. xs[ix] + ww - 1 of the grid [N][H][W].  `tiles` (ny * nx device pointers), `ys` (ny ints) and `xs` (nx ints)
 *   are HOST arrays, read before the call returns; wy [wh] and wx [ww] are DEVICE tables of positive weights (the blend's
 *   importance map is wy[i] * wx[j]).  Per output pixel (n, y, x), all in fp32, the tiles that cover it in row-major (iy, ix) order:
 *     w_t = wy[y - ys[iy]] * wx[x - xs[ix]], rounded on its own;   s = w_0 + w_1 + ... in that order;   v_t = w_t / s (IEEE);
 *     acc_k = v_0 p_0[k] + v_1 p_1[k] + ... in that order from 0.0f (the product of a term may be fused into its addition).
 *   pred uint8 [N][H][W] = the first maximum of acc_k by smsut_argmax_channels' comparison (the first maximum wins, a NaN wins);
 *   conf (nullable) fp32 [N][H][W] = acc_pred; prob (nullable) fp32 [N][H][W][K] = acc_k.  The weights are normalised before the
 *   sum: under ONE tile v = w / w = 1.0f and the tile's probabilities pass through bit for bit.  A pixel under no tile gets
 *   acc = 0 and pred 0 (the Python wrapper refuses a plan that leaves one).  No atomics, no cross-thread sums: bitwise reproducible.
 * Limits (otherwise SMSUT_EINVAL and nothing is launched; N == 0 returns SMSUT_OK without a launch): 1 <= ny * nx <= 64,
 *   1 <= K <= SMSUT_TTA_MAX_CLASSES, N <= SMSUT_TTA_MAX_SLICES, 1 <= wh <= H <= SMSUT_TTA_MAX_DIM, 1 <= ww <= W <= SMSUT_TTA_MAX_DIM,
 *   every tile inside the grid: 0 <= ys[iy] <= H - wh, 0 <= xs[ix] <= W - ww. */
#define SMSUT_WINDOW_MAX_TILES 64  /* 1 <= ny * nx <= 64 */
int smsut_window_blend(const float* const* tiles, const int* ys, const int* xs, const float* wy, const float* wx, uint8_t* pred,
                       float* conf /*nullable*/, float* prob /*nullable*/, int ny, int nx, int N, int H, int W, int wh, int ww, int K,
                       void* stream);

/* ---------------------------------------------------------------------------------------------- calibration
 * How far the predicted probabilities of a batch can be trusted (csrc/calibration.hip; misc/utils.py: CalibrationMeter,
 * fit_temperature): the reliability table, negative log-likelihood, Brier score and the derivatives of the NLL by the inverse
 * temperature, in one pass.  The reference has no calibration code: this replaces the softmax / max / gather / bucketize /
 * bincount / log / sum chain one would build from torch.
 * logits fp32 [N][H][W][C] (NHWC), 4-byte aligned, read in place, each logit once; labels int64 [N][H][W]; classes = channels
 * 0 .. K-1; B confidence bins; beta = 1 / temperature.  Per pixel with label y, all in fp32, in this order (z = the pixel's logits):
 *   u_k = beta * z_k, rounded on its own (beta == 1.0f: u_k is z_k);   m = max_k u_k;   e_k = expf(u_k - m);
 *   s = e_0 + e_1 + ... in channel order;   p_k = e_k / s;
 *   pred = the first maximum of p_k by smsut_argmax_channels' comparison (the first maximum wins, a NaN wins);   conf = p_pred;
 *   correct = (pred == y);   bin = min(B - 1, (int)(conf * (float)B));
 *   nll = logf(s) - (u_y - m);
 *   brier = sum_k (p_k - [k == y])^2,   ez = sum_k p_k z_k,   ezz = sum_k p_k (z_k z_k),   each in channel order from 0.0f (the
 *     product of a term may be fused into its addition: one rounding less);   vz = max(ezz - ez ez, 0.0f).
 * A pixel whose label lies outside 0 .. K-1 counts in `skipped` and nowhere else (smsut_eval_overlap's rule; its logits are not
 * looked at); otherwise a pixel whose conf is NaN or Inf counts in `nonfinite` and nowhere else.
 * out: double [3 B + 4 K + 4], ADDED to and never zeroed here (the caller zeroes it once per evaluation):
 *   out[3 b + 0..2]          bin b:        {pixels, sum of conf, correct pixels}
 *   out[3 B + 4 k + 0..3]    true class k: {pixels, correct pixels, sum of nll, sum of brier}
 *   out[3 B + 4 K + 0..3]    {g = sum of (ez - z_y), h = sum of vz, skipped, nonfinite}
 *   (ez - z_y is one fp32 subtraction; g and h are the first and second derivative of the summed NLL by beta).
 * Counts are integers summed as integers; so is the sum of conf, as conf * 2^28 (an fp32 conf in [2^-5, 1] is a multiple of
 * 2^-28), converted once: exact while it stays below 2^53 * 2^-28.  (A workgroup keeps pixels and correct pixels as the 32-bit
 * halves of one word and the batch's sum of conf * 2^28 is one int64: both hold for any batch of fewer than 2^35 pixels, and a
 * larger one -- more than 2^38 bytes of labels alone -- fits no device this library runs on; the limits below are per axis.)  nll, brier, ez - z_y and vz are converted to fp64 per pixel and
 * summed in fp64 in an order that depends on (N H W, K) alone: per-workgroup partial vectors in `workspace`, added in workgroup
 * order by a finishing launch.  No float atomics: two calls on the same input give the same bits.  Two launches, no memset.
 * workspace: smsut_calibration_ws(N, H, W, C, K, B) bytes, written before it is read; -1 for arguments outside the limits.
 * Limits (otherwise SMSUT_EINVAL and nothing is launched; N == 0 returns SMSUT_OK without a launch); beta finite and positive: */
#define SMSUT_CALIB_MAX_CLASSES 32   /* 1 <= K <= min(C, 32) */
#define SMSUT_CALIB_MAX_BINS 64      /* 1 <= B <= 64 */
#define SMSUT_CALIB_MAX_SLICES 65535 /* N <= 65535 */
#define SMSUT_CALIB_MAX_DIM 16384    /* 1 <= H, W <= 16384 */
int64_t smsut_calibration_ws(int N, int H, int W, int C, int K, int B);
int smsut_calibration_stats(const float* logits, const int64_t* labels, double* out, void* workspace, int N, int H, int W, int C,
                            int K, int B, float beta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMSUT_HIP_H */
