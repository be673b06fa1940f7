/*
 * medfusion_hip.h -- C-ABI of libmedfusion_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the latent-diffusion SAMPLING path of mueller-franzes/medfusion
 * (DiffusionPipeline.sample -> UNet denoise loop -> VAE.decode; VAE.encode as API surface).
 * The reference is pure PyTorch: its "FFI" for this path is the set of ATen ops each Python
 * method dispatches.  Every entry point below names the reference call site(s) it replaces
 * (paths relative to the reference repo root).  The Python host (medfusion_amd/) binds these
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers + sizes, no torch types.  All pointers are DEVICE pointers
 *    owned by the caller (torch allocations); the library never allocates, frees or retains
 *    device memory.  Scratch is caller-provided (`*_workspace_bytes`).
 *  - fp32 everywhere.  Activations are NHWC ("channels-last") inside the path; the API edge
 *    tensors of the reference (latents, images) are NCHW and are read/written directly by the
 *    edge convolutions (MF_LAYOUT_NCHW) -- no separate transpose pass.
 *  - Every call is an asynchronous launch on `stream` (a hipStream_t passed as void*);
 *    no host sync, no allocation, no host reads: hipGraph-capture-safe.
 *  - Return 0 on success, negative MF_E* on failure; message via mf_last_error() (thread-local).
 */
#ifndef MEDFUSION_HIP_H
#define MEDFUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_VERSION 250 /* 0.2.5 */

enum { MF_OK = 0, MF_EINVAL = -1, MF_EUNSUPPORTED = -2, MF_ELAUNCH = -3, MF_EWORKSPACE = -4 };
enum { MF_LAYOUT_NHWC = 0, MF_LAYOUT_NCHW = 1 };

int mf_version(void);
const char* mf_last_error(void);

/* ------------------------------------------------------------------ convolution
 * Replaces torch.nn.Conv2d.forward at: conv_blocks.py:185 (BasicBlock.conv), :238 (conv_res 1x1),
 * :66 (BasicDown 3x3 stride 2), :123-125 (BasicUp: F.interpolate nearest-exact x2 + 3x3 conv, fused:
 * upsample=1 gathers from the low-res tensor), unet2.py:259 (torch.cat([h, skip]) fused: x2/C2),
 * unet2.py:267 / latent_embedders.py:768 (1x1 out convs).
 * Weights are pre-packed once by mf_pack_conv_weight_f32 (OIHW -> [Cout][KH][KW][Cin]).
 */
typedef struct MfConvDesc {
  int32_t N, Hin, Win;     /* batch, input spatial size (BEFORE the fused x2 upsample) */
  int32_t C1, C2;          /* channels read from x1 and x2 (C2 = 0: single source); Cin = C1 + C2 */
  int32_t Cout;
  int32_t KH, KW;          /* 1x1 or 3x3 */
  int32_t stride;          /* 1 or 2 */
  int32_t pad;             /* MONAI get_padding(k, s) = int((k - s + 1) / 2) */
  int32_t upsample;        /* 1: nearest x2 of the input fused into the gather; 2: the same op in its SUB-PIXEL form (4 phase-specific
                              2x2 convs on the low-res tensor, 4/9 of the MACs; weights from mf_pack_upconv_weight_f32) */
  int32_t in_layout;       /* layout of x1 (NCHW only with C2 == 0) */
  int32_t out_layout;      /* layout of y */
  int32_t tile_hint;       /* 0 = auto; else forces an implicit-GEMM tile config (tuning/tests) */
  int32_t splitk_hint;     /* 0 = auto; else forces split-K factor */
  int32_t precision;       /* arithmetic of the implicit-GEMM path (MF_CONV_*, below); the small/direct kernels are always plain fp32 */
} MfConvDesc;
/* MF_CONV_FP32: v_mfma_f32_32x32x2_f32, products and sums exactly those of an fp32 fma chain.
 * MF_CONV_FP32_SPLIT3_W3: every fp32 operand is split EXACTLY into three bf16 terms (x = h + m + l, 8 significant bits each) and
 *   a*b is accumulated in fp32 on the bf16 matrix cores as the six terms of order <= 2 (hh, hm, mh, mm, hl, lh); the dropped terms
 *   are < 2^-23 |a*b|.  16x the MFMA rate / 6 terms = 3/8 of the matrix time.  `w_packed` points to the weights ALREADY split:
 *   mf_split_conv_weight_bf16x3 turns either fp32 packing ([rows][K]) into [rows][K/8][3 pieces][8] bf16 (6 bytes per weight) once
 *   at load time; the activations are split in the kernel.  Measured against fp64 its error is at or below the fp32-MFMA kernel's on
 *   every shape of the path (the planner keeps one accumulation chain <= 96 chunks via split-K).  Implicit-GEMM path only.
 *   (Values 1 and 2 -- the same arithmetic with the weights split in the kernel, and its chunk-sum variant -- were retired in ABI 200.)
 * MF_CONV_BF16 (opt-in, REDUCED precision): operands rounded to bf16 (round to nearest even), one MFMA term, fp32
 *   accumulate; `w_packed` points to weights converted by mf_convert_conv_weight_bf16 ([rows][K] bf16).  Error vs fp64 ~3e-3 per
 *   convolution (2^-9 per operand); never selected by default, has its own tolerance in the tests.  Implicit-GEMM path only.
 * MF_CONV_FP32_F16X2: fp32 through PAIRS of fp16 on the fp16 matrix cores.  Every operand -- activations and weights -- lives in HBM
 *   as x ~ hi + lo/2048 with hi = RN16(x), lo = RN16((x - hi) * 2048): 23 of the 24 significand bits (error <= 2^-23 |x|, one fp32
 *   ulp at most, zero for 3 values of 4; the format is 4 bytes per element like fp32, groups of 8 channels as [hi x 8][lo x 8]).  a*b is accumulated in
 *   fp32 as wh*xh + (wh*xl + wl*xh)/2048 -- 3 matrix instructions per product instead of 6, dropped term < 2^-22 |a*b|.  Because the
 *   operands need no arithmetic in the kernel, both go HBM -> LDS by LDS-DMA.  Entry point mf_conv2d_f16x2 (operands produced by
 *   mf_split_f16x2 or by the split output of mf_gn_apply_split_f32); every operand tensor carries a per-sample power-of-two scale, so
 *   there is no range limit (mf_gn_apply_split_f32 below has the details).
 * MF_CONV_F16 (opt-in, REDUCED precision; SURVEY 8f row 4, ABI 210): the fp16-pair operands and the LDS-DMA kernel of MF_CONV_FP32_F16X2 with
 *   ONE product term -- main += wh * xh only, i.e. both operands rounded to fp16 (11 significant bits, the per-sample power-of-two
 *   scales keep the range), fp32 accumulate.  Same entry point (mf_conv2d_f16x2 with desc.precision = MF_CONV_F16), same operand
 *   images; a third of the matrix instructions, half of the LDS fragment reads.  Error vs fp64 ~3e-4 per convolution (2^-12 per
 *   operand); never selected by default, own tolerance in the tests, never the headline. */
enum { MF_CONV_FP32 = 0, MF_CONV_FP32_SPLIT3_W3 = 3, MF_CONV_BF16 = 4, MF_CONV_FP32_F16X2 = 5, MF_CONV_F16 = 6 };

int mf_pack_conv_weight_f32(const float* w_oihw, float* w_packed, int Cout, int Cin, int KH, int KW, void* stream);
/* nearest-x2 + 3x3 (conv_blocks.py:123-125) as the transposed-conv-equivalent sub-pixel form: OIHW 3x3 -> [4][Cout][2][2][Cin],
 * each phase kernel = sum of the 3x3 taps that land on the same source pixel.  mf_conv2d_subpixel_ok: can `d` (upsample = 2) run so? */
int mf_pack_upconv_weight_f32(const float* w_oihw, float* w_packed, int Cout, int Cin, void* stream);
int mf_conv2d_subpixel_ok(const MfConvDesc* d);
/* 1 if `d` runs on the implicit-GEMM kernel (the only one that looks at `precision`), 0 for the small-Cin / direct kernels */
int mf_conv2d_is_igemm(const MfConvDesc* d);
/* rows = Cout (x4 for the sub-pixel packing); out: rows * K * 6 bytes */
int mf_split_conv_weight_bf16x3(const float* w_packed, void* w_split, long rows, int K, void* stream);
/* out: rows * K * 2 bytes (MF_CONV_BF16) */
int mf_convert_conv_weight_bf16(const float* w_packed, void* w_bf16, long rows, int K, void* stream);
size_t mf_conv2d_workspace_bytes(const MfConvDesc* d);
/* y = conv(x1 (++ x2 on channels), w) + bias.  bias may be NULL.  workspace >= mf_conv2d_workspace_bytes. */
int mf_conv2d_f32(const float* x1, const float* x2, const float* w_packed, const float* bias, float* y,
                  void* workspace, size_t workspace_bytes, const MfConvDesc* d, void* stream);

/* --- MF_CONV_FP32_F16X2 (same reference call sites as mf_conv2d_f32: conv_blocks.py:185,238,66,123-125, unet2.py:259)
 * mf_split_f16x2: fp32 [rows][per_row] (per_row % 8 == 0) -> the fp16-pair form (4 bytes per element), row r scaled by
 *   2^-(floor(log2 bound[r]) - 14) (bound NULL: no scaling).  Used for packed weights (rows = 1, bound = max|w|) once at load time and for
 *   activations no producer kernel has split (rows = N samples).
 * mf_conv2d_f16x2: x1s / x2s / ws in fp16-pair form with their bounds (x*_bound: [N] floats or NULL = unscaled; w_bound: the scalar the
 *   weights were split with, 0 = unscaled); y fp32 NHWC.  gn_partial optional: statistics of the following GroupNorm(G), [N][parts][G][2]
 *   doubles, parts = mf_conv2d_gn_parts(d, G) > 0.  y_bound optional ([N][slots] floats, slots = mf_conv2d_f16x2_bound_slots(d) > 0,
 *   not together with gn_partial): every (tile, wave) -- or reducer wave -- stores the max |y| of its share of a sample; reduce with
 *   mf_bound_finalize_f32 to the operand bound of y for consumers that take it un-normalised.  Split-K plans reduce through `workspace`
 *   (mf_conv2d_workspace_bytes).  A power-of-two split meets INSIDE the launch: the partial tiles of a pair are handed over through
 *   `workspace` with write-through stores, a counter per pair in `sync` tells the workgroup that arrives second to add its partner's tile
 *   (a + b does not depend on who adds: deterministic), the last one runs the ordinary epilogue -- no reducer launch.  `sync`:
 *   mf_conv2d_f16x2_sync_words(d) 32-bit words, zero before the FIRST launch and left zero by every launch (caller keeps them; one array
 *   per stream is enough).  Other splits (or GroupNorm statistics the epilogue cannot emit; or MF_CONV_TREE=0 in the environment, read once)
 *   take the slab + reducer pass, the reducer emitting y, the statistics and y_bound; it sums the slabs in the same pairwise order, so the
 *   two paths give the same bits.
 * mf_conv2d_plan_query: the tile id and split-K factor the planner picks for `d` (any precision; 0, 0 = not on the implicit-GEMM path). */
int mf_conv2d_f16x2_ok(const MfConvDesc* d);
int mf_conv2d_f16x2_bound_slots(const MfConvDesc* d);
int mf_split_f16x2(const float* x, void* xs, const float* bound, int rows, int64_t per_row, void* stream);
/* The same split when the bound of every row still lies as slot maxima -- slots [rows][nslots]: the y_bound array of mf_conv2d_f16x2 or
 * the `partial` array of mf_maxabs_rows_f32 (bound = NULL there) -- reduced inside the pass, which also publishes bound_out[rows]: one
 * launch instead of mf_bound_finalize_f32 + mf_split_f16x2 (7 launches fewer per denoise iteration of the published UNet). */
int mf_split_f16x2_slots(const float* x, void* xs, const float* slots, int nslots, float* bound_out, int rows, int64_t per_row, void* stream);
int mf_conv2d_f16x2_sync_words(const MfConvDesc* d);
int mf_conv2d_f16x2(const void* x1s, const void* x2s, const void* ws, const float* bias, float* y, const float* x1_bound,
                    const float* x2_bound, float w_bound, float* y_bound, void* workspace, size_t workspace_bytes, uint32_t* sync,
                    double* gn_partial, int G, const MfConvDesc* d, void* stream);
int mf_conv2d_plan_query(const MfConvDesc* d, int32_t* tile_id, int32_t* splitk);
/* A run-time override of the planner's choice for the shape of `d` (ABI 220; tile = 0 removes it): consulted before the built-in table when the
 * descriptor carries no hints.  For tuning inside the real pipeline (scripts/plan_tune.py) -- the table is what ships. */
/* (a caller that caches plan-derived sizes -- workspace bytes, sync words, bound slots, which pairs share a launch -- drops them when it installs an
 * override: the Python host's per-module caches are cleared by the tuning scripts that use this entry, scripts/plan_tune.py:clear_caches) */
int mf_conv2d_plan_override(const MfConvDesc* d, int tile, int splitk);

/* TWO independent fp16-pair convolutions in ONE launch (ABI 220; BasicResBlock.forward, conv_blocks.py:194-240: `conv_res(x)` (:238) and the 3x3
 * convolution of the block (:185) read the same x and neither reads the other's result).  The grid is a's workgroups followed by b's: a -- the
 * large one -- fills the device as it does alone, b's workgroups take the CUs a's workgroups leave; no kernel boundary between the two, b's ramp
 * under a's drain.  Every workgroup runs the unchanged code of its own convolution, so both results are bit-identical to two mf_conv2d_f16x2
 * calls with the same arguments (each call struct holds exactly those arguments).  mf_conv2d_f16x2_group_ok(a, Ga, b, Gb): can these two plans
 * share a launch (Ga / Gb: groups of the GroupNorm statistics asked of a / b, 0 = none) -- both MF_CONV_FP32_F16X2, both finishing inside their
 * launch (no slab + reducer pass), equal workgroup sizes, a tile pair that is instantiated (the pairs cfg2's channel-changing ResBlocks use;
 * descriptor hints choose b's tile).  When both meet their split-K slices inside the launch, their workspaces and sync arrays must not overlap. */
typedef struct MfConvF16x2Call {
  const void* x1s; const void* x2s; const void* ws; const float* bias; float* y;
  const float* x1_bound; const float* x2_bound; float w_bound; float* y_bound;
  void* workspace; size_t workspace_bytes; uint32_t* sync;
  double* gn_partial; int G;
  const MfConvDesc* d;
} MfConvF16x2Call;
int mf_conv2d_f16x2_group_ok(const MfConvDesc* a, int Ga, const MfConvDesc* b, int Gb);
int mf_conv2d_f16x2_group(const MfConvF16x2Call* a, const MfConvF16x2Call* b, void* stream);

/* Convolution + GroupNorm + Swish + residual + embedding in ONE launch (ABI 220; BasicBlock.forward / BasicResBlock.forward,
 * conv_blocks.py:185-191,236-240, with the `x += emb` of :360-363): the fp16-pair convolution whose workgroups keep their final tile in
 * registers, publish the tile's partial GroupNorm sums (gn_partial, as in mf_conv2d_f16x2), meet the other tiles of their SAMPLE at a
 * counter, finalize mean / rstd from the sample's records and apply act(gn(y) gamma + beta) + residual + emb[n][c] on the way out -- what
 * mf_conv2d_f16x2 + mf_gn_apply_from_partials_pairs_f32 compute in two launches, bit for bit (same records, same summation order, same
 * per-element operations); the un-normalised y is never written.  Workgroups WAIT for each other, so the form exists only for plans whose
 * whole grid is resident on the device at once: mf_conv2d_f16x2_fuse_words(d, G) = the zero-initialised 32-bit words `rendezvous` needs
 * (2 per sample; every launch leaves them zero; one array per stream), 0 = this convolution cannot (use the two-launch form).
 * `error_flag`: one zero-initialised word; a wait that does not complete within 50 ms (another process's waiting workgroups filling the
 * device) sets it, later launches stop waiting, and the results since are INVALID: the caller checks it at the end of its loop, zeroes
 * flag and rendezvous words, and re-runs on the two-launch form.  Arguments as in the two calls it replaces; out may be NULL (fp16 pairs
 * only), out_split / out_bound are required.  MEASURED (round 4, profiles/r04_fused_gn_apply_ab.txt, r04_conv_timeline_fused.txt): not
 * faster than the two launches on MI355X -- the tail (records, rendezvous, finalize, apply at one wave per SIMD) costs what the kernel
 * boundary plus the stand-alone pass cost -- so the Python host keeps it opt-in (MEDFUSION_FUSED_APPLY=1). */
typedef struct MfGnFuse {
  const float* gamma;            /* [Cout] or NULL (both) */
  const float* beta;
  const float* residual;         /* fp32 NHWC [N][Ho][Wo][Cout], or NULL */
  const void* residual_pairs;    /* the residual as fp16 pairs scaled by res_bound, or NULL */
  const float* res_bound;        /* [N], or NULL with res_bound_slots */
  const float* res_bound_slots;  /* [N][res_nslots] slot maxima (y_bound of the convolution that made the residual) */
  const float* emb;              /* emb[n * emb_stride + c] or NULL */
  const float* emb_bound;        /* [N] */
  float* out;                    /* fp32 result or NULL */
  void* out_split;               /* fp16-pair result */
  float* out_bound;              /* [N] written */
  uint32_t* rendezvous;
  uint32_t* error_flag;
  int64_t emb_stride;
  int32_t res_nslots;
  int32_t act;                   /* 1: Swish */
  float bconst;                  /* >= max |act(gn(y) gamma + beta)| (mf_gn_apply_from_partials_f32) */
  float eps;
} MfGnFuse;
int mf_conv2d_f16x2_fuse_words(const MfConvDesc* d, int G);
int mf_conv2d_f16x2_gn_apply(const void* x1s, const void* x2s, const void* ws, const float* bias, const float* x1_bound, const float* x2_bound,
                             float w_bound, void* workspace, size_t workspace_bytes, uint32_t* sync, double* gn_partial, int G,
                             const MfGnFuse* f, const MfConvDesc* d, void* stream);

/* The network input as an fp16-pair operand (ABI 220; the NCHW latent of unet2.py:246 / the image of latent_embedders.py:757): x NCHW
 * [N][C][HW], C <= CP -> the pair form of the NHWC tensor [N][HW][CP] (CP % 32 == 0, channels C .. CP-1 zero) scaled per sample by its own
 * max |x|, which the launch measures and publishes (bound_out[N]); one workgroup per sample (C * HW <= 2^18).  With the convolution's
 * weights zero-padded to CP input channels (host, once) the input convolution runs on mf_conv2d_f16x2 like the rest of the network. */
int mf_pack_nchw_pairs_f32(const float* x, void* out_pairs, float* bound_out, int N, int C, int HW, int CP, void* stream);
/* The same convolution writing its output ALSO as fp16 pairs (ABI 220), for outputs that feed convolutions un-normalised (BasicDown /
 * BasicUp, conv_blocks.py:66,123-125): the per-sample scale comes from a bound DERIVED from the operands, |y[n]| <= x1_bound[n] w_l1_1 +
 * x2_bound[n] w_l1_2 + bias_max with w_l1 = max over the output channels of the L1 norm of the filter over that source's channels (host,
 * once per weight tensor) -- rigorous, a few binades above the true maximum (the pair format keeps its 23 bits down to 2^-28 of the bound),
 * so no measuring epilogue, no mf_split_f16x2_slots launch behind the convolution.  y_bound_out[N] receives the bound.  Only for plans
 * whose final values exist inside the launch: mf_conv2d_f16x2_pairs_out_ok(d). */
int mf_conv2d_f16x2_pairs_out_ok(const MfConvDesc* d);
int mf_conv2d_f16x2_pairs_out(const void* x1s, const void* x2s, const void* ws, const float* bias, float* y, void* y_split, float* y_bound_out,
                              const float* x1_bound, const float* x2_bound, float w_bound, float w_l1_1, float w_l1_2, float bias_max,
                              void* workspace, size_t workspace_bytes, uint32_t* sync, const MfConvDesc* d, void* stream);

/* --- Winograd F(2x2, 3x3) form of the 3x3 stride-1 pad-1 convolutions on the fp16-pair arithmetic (ABI 230; conv_blocks.py:185 as reached
 * from unet2.py:250-264 -- the 3x3 convolutions of the UnetResBlocks, 94.4 % of the UNet's FLOPs).
 *   y = A^T [ sum_c (G g G^T) . (B^T d B) ] A   per 2x2 output tile: 16 products per (tile, channel pair) instead of 36 (2.25x fewer matrix
 * instructions).  The 16 element-wise products summed over the input channels are 16 independent GEMMs; they run on the kernel of
 * mf_conv2d_f16x2 (fp16-pair operands, three product terms, fp32 accumulate, in-launch split-K tree), each row block with the weight slab of
 * its component.  Same values as the direct form to fp32 rounding -- a DIFFERENT summation, not the same bits (error vs fp64 in
 * profiles/r05_winograd_ab.txt).  The exact arithmetics (MF_CONV_FP32 / MF_CONV_FP32_SPLIT3_W3) have their own entry points for this form since
 * ABI 250 (mf_wino_f32_ok and below).
 *  mf_wino_ok(d): can `d` (3x3, stride 1, pad 1, upsample 0, NHWC, precision MF_CONV_FP32_F16X2, H and W even, C1 % 32 == C2 % 32 == 0,
 *    Cout in {64, 128, 256, 512, 1024}) run so?  mf_wino_preferred(d): ... AND is it the faster form on MI355X?  ABI 240: answered for ANY batch by
 *    a rule in (Cin, Cout, H W, N) fitted to the sweeps at B = 4 ... 69 (Cin Cout >= 190 (Cin + Cout), csrc/conv_f16x2_wino.inc) instead of the
 *    exact-shape table of ABI 230 (csrc/wino_plan_table.inc, kept as the record: mf_wino_in_table(d) says whether `d` is one of its rows).
 *  mf_wino_pack_weight_f32: OIHW 3x3 -> U = G g G^T, [16 components][Cout][Cin] fp32 (fp64 arithmetic, one rounding); split it with
 *    mf_split_f16x2(rows = 1, bound = max |U|) like any packed weight.
 *  mf_wino_input_f16x2: the fp16-pair form xs of an NHWC activation (scaled per sample by x_bound[N]) -> V = B^T d B as fp16 pairs
 *    [16][N][(H/2)(W/2)][C], component k of sample n scaled by v_bound[k N + n] = 4 x_bound[n] (v_bound: 16 N floats, written).
 *  mf_conv2d_wino_f16x2: v1s / v2s (the second source of a fused channel concat, or NULL) with their v*_bound arrays, us = the split U with the
 *    scalar u_bound it was split with; y fp32 NHWC [N][H][W][Cout] = conv3x3(x1 ++ x2) + bias.  gn_partial optional: [N][parts][G][2] doubles,
 *    parts = mf_wino_gn_parts(d, G) > 0 -- the records mf_gn_apply_from_partials_* reads.  workspace >= mf_wino_workspace_bytes(d) (the GEMM's
 *    output in the transform domain + its split-K hand-off region), sync = mf_wino_sync_words(d) zero-initialised words as for mf_conv2d_f16x2.
 *    d->tile_hint / splitk_hint address the component GEMM.  Two launches: the GEMM, then A^T M A + bias + statistics. */
int mf_wino_ok(const MfConvDesc* d);
int mf_wino_preferred(const MfConvDesc* d);
int mf_wino_in_table(const MfConvDesc* d);
int mf_wino_pack_weight_f32(const float* w_oihw, float* u, int Cout, int Cin, void* stream);
int mf_wino_input_f16x2(const void* xs, const float* x_bound, void* vs, float* v_bound, int N, int H, int W, int C, void* stream);
size_t mf_wino_workspace_bytes(const MfConvDesc* d);
int mf_wino_sync_words(const MfConvDesc* d);
int mf_wino_gn_parts(const MfConvDesc* d, int G);
int mf_wino_plan_query(const MfConvDesc* d, int32_t* tile_id, int32_t* splitk);
/* --- the Winograd form on the EXACT arithmetics (ABI 250): MF_CONV_FP32_SPLIT3_W3 and MF_CONV_FP32 take plain fp32 operands, so the three pieces are
 * separate calls on fp32 tensors (same reference call sites as above: conv_blocks.py:185-191,236-240,360-363 via unet2.py:250-264):
 *   mf_wino_f32_ok(d, G): can the 3x3 `d` (precision 0 or 3, stride 1, pad 1, NHWC, H and W even, n T % 64 == 0) with the G-group GroupNorm behind it run so?
 *   mf_wino_input_f32: x fp32 NHWC -> V = B^T d B fp32 [16][N][(H/2)(W/2)][C]
 *   the 16 component GEMMs: mf_conv2d_f32 with the descriptor {N = 16 n, Hin = 1, Win = T, C1, C2, Cout, KH = KW = 1, stride 1, pad 0, upsample = 3, NHWC,
 *     precision 0 | 3}: x1 / x2 = V of the two sources, w = U = G g G^T [16][Cout][Cin] from mf_wino_pack_weight_f32 (precision 3: split by
 *     mf_split_conv_weight_bf16x3 over rows = 16 Cout), bias NULL, y = M fp32 [16][n T][Cout]; rows [k n T, (k + 1) n T) use weight slab k
 *   mf_wino_tail_f32: M -> y = A^T M A + bias -> GroupNorm over the whole (sample, group) -> Swish (act = 1) -> + residual (fp32 NHWC or NULL) -> + emb row;
 *     out fp32 NHWC and, if out_wino != NULL, V of the result for the next Winograd convolution.  The kernel is the tail of the fp16-pair form. */
int mf_wino_f32_ok(const MfConvDesc* d, int G);
int mf_wino_input_f32(const float* x, float* v, int N, int H, int W, int C, void* stream);
int mf_wino_tail_f32(const float* m, const float* bias, const float* gamma, const float* beta, const float* residual, const float* emb, int64_t emb_stride,
                     float* out, float* out_wino, int N, int H, int W, int C, int G, int act, float eps, void* stream);
int mf_conv2d_wino_f16x2(const void* v1s, const void* v2s, const void* us, const float* bias, float* y, const float* v1_bound, const float* v2_bound,
                         float u_bound, void* workspace, size_t workspace_bytes, uint32_t* sync, double* gn_partial, int G, const MfConvDesc* d,
                         void* stream);
/* The Winograd convolution WITH what follows it in a ResBlock (BasicBlock.forward / BasicResBlock.forward, conv_blocks.py:185-191,236-240, and
 * the `x += emb` of :360-363): GroupNorm(G) + Swish + residual + embedding row -- and, optionally, the INPUT TRANSFORM of the next Winograd
 * convolution -- in the launch behind the GEMM: one workgroup per (sample, group) holds all pixels of the sample x the group's channels in LDS,
 * so the statistics are complete inside the workgroup (no records, no apply pass, no un-normalised y in memory).  Outputs, each optional: `out`
 * fp32 NHWC, `out_split` its fp16-pair form scaled per sample by out_bound[n] = bconst + bound(residual) + bound(embedding row) (as
 * mf_gn_apply_from_partials_pairs_f32 derives it), `out_wino` = B^T d B of the result as mf_wino_input_f16x2 would make it from out_split (bit
 * for bit; [16][N][(H/2)(W/2)][Cout], wino_bound: 16 N floats).  mf_wino_tail_ok(d, G): mf_wino_ok(d), whole 8-channel groups per GroupNorm
 * group and H W (Cout / G) floats <= 64 KB.  The per-element arithmetic is that of the apply pass; the statistics are summed in another order
 * than the records of mf_conv2d_wino_f16x2 (same values to fp64 rounding). */
typedef struct MfWinoTail {
  const float* gamma; const float* beta;                    /* [Cout], both or neither */
  const float* residual; const void* residual_pairs;         /* fp32 NHWC, or fp16 pairs scaled by res_bound, or neither */
  const float* res_bound; const float* res_bound_slots;      /* [N], or [N][res_nslots] slot maxima (mf_conv2d_f16x2 y_bound) */
  const float* emb; const float* emb_bound;                  /* [N][emb_stride] rows added per (n, c) + their bounds [N], or NULL */
  float* out; void* out_split; float* out_bound;
  void* out_wino; float* wino_bound;
  int64_t emb_stride;
  int32_t res_nslots, act;                                   /* act 1: Swish */
  float bconst, eps;                                         /* bconst >= max |act(gn(y) gamma + beta)| (host constant), GroupNorm eps */
} MfWinoTail;
int mf_wino_tail_ok(const MfConvDesc* d, int G);
/* `guest` (optional): a second, independent fp16-pair convolution -- conv_res of the same ResBlock (conv_blocks.py:238), an ordinary
 * MfConvF16x2Call as for mf_conv2d_f16x2_group -- whose workgroups share the component GEMM's launch (the GEMM's first, the guest's on the CUs
 * they leave); bit-identical to its own mf_conv2d_f16x2 call; its output may be the tail's residual (the tail launches behind both).  Ask
 * mf_wino_group_ok(d, guest->d) first; workspaces and sync arrays of the two must not overlap. */
int mf_wino_group_ok(const MfConvDesc* d, const MfConvDesc* guest);
int mf_conv2d_wino_gn_apply_f16x2(const void* v1s, const void* v2s, const void* us, const float* bias, const float* v1_bound, const float* v2_bound,
                                  float u_bound, void* workspace, size_t workspace_bytes, uint32_t* sync, int G, const MfWinoTail* t,
                                  const MfConvF16x2Call* guest, const MfConvDesc* d, void* stream);

/* Convolution with the statistics of the FOLLOWING GroupNorm (G groups over Cout) fused in: per-tile sums from the
 * epilogue, or from the split-K reducer when the plan splits K.  gn_partial: [N][parts][G][2] doubles {sum, sumsq},
 * parts = mf_conv2d_gn_parts(d, G); 0 means this convolution cannot emit them (use mf_gn_stats_partial_f32). */
int mf_conv2d_gn_parts(const MfConvDesc* d, int G);
int mf_conv2d_gn_f32(const float* x1, const float* x2, const float* w_packed, const float* bias, float* y, void* workspace,
                     size_t workspace_bytes, double* gn_partial, int G, const MfConvDesc* d, void* stream);

/* ------------------------------------------------------------------ GroupNorm + Swish + residual + embedding
 * Replaces nn.GroupNorm + MONAI Swish + `out + residual` + `x += emb` at conv_blocks.py:186-191,
 * :236-240, :360-363 (UnetResBlock) / :298-301 (UnetBasicBlock).  NHWC.
 * stats[n][g] = {mean, rstd} (biased variance, eps inside the sqrt).
 */
size_t mf_gn_stats_workspace_bytes(int N, int HW, int C, int G);
int mf_gn_stats_f32(const float* x, float* stats, void* workspace, size_t workspace_bytes, int N, int HW, int C, int G,
                    float eps, void* stream);
/* Form used on the hot path: partial sums [N][parts][G][2] (doubles; parts = mf_gn_partial_parts(HW), or emitted by
 * mf_conv2d_gn_f32 / mf_conv2d_f16x2), a tiny finalize kernel, then the apply pass. */
int mf_gn_partial_parts(int HW);
int mf_gn_stats_partial_f32(const float* x, double* partial, int N, int HW, int C, int G, void* stream);
/* partial sums -> stats[n][g] = {mean, rstd} (tiny kernel; mf_gn_apply_from_partials_f32 below folds it into the apply pass) */
int mf_gn_finalize_f32(const double* partial, int parts, float* stats, int N, int HW, int C, int G, float eps, void* stream);
/* out = act(gn(x) * gamma + beta) + residual + emb[n*emb_stride + c]; act: 0 none, 1 Swish x*sigmoid(x).
 * gamma/beta NULL => no affine; stats NULL => no normalisation; residual / emb NULL => skipped.
 * out may alias x. */
int mf_gn_apply_f32(const float* x, const float* stats, const float* gamma, const float* beta, const float* residual,
                    const float* emb, int64_t emb_stride, float* out, int N, int HW, int C, int G, int act, void* stream);
/* The same pass, also writing the fp16-pair form of `out` (operand of a following MF_CONV_FP32_F16X2 convolution; C % 8 == 0).
 * A fp16-pair tensor carries a per-sample power-of-two scale derived from an UPPER BOUND of |value| over the sample (fp16 stops at
 * 65504, an un-normalised residual stream does not): the pass derives the bound of its output from its inputs --
 *   bound[n] = (stats ? bconst : x_bound[n]) + res_bound[n] + emb_bound[n],  bconst >= max|act(gn(x) gamma + beta)| =
 *   max|gamma| sqrt(group size) + max|beta| -- scales sample n by 2^-(floor(log2 bound[n]) - 14) and publishes bound[n] in out_bound.
 *   The bounds handed in must BE bounds: the from-partials passes no longer clamp to the fp16 range (round 4: 4 VALU instructions per element in
 *   a VALU-bound pass) -- a value above its sample's bound by more than 2x overflows its pair to Inf instead of saturating at 65504 2^s. */
int mf_gn_apply_split_f32(const float* x, const float* stats, const float* gamma, const float* beta, const float* residual,
                          const float* emb, int64_t emb_stride, float* out, void* out_split, const float* x_bound, const float* res_bound,
                          const float* emb_bound, float bconst, float* out_bound, int N, int HW, int C, int G, int act, void* stream);
/* mf_gn_finalize_f32 + mf_gn_apply_split_f32 in ONE launch: mean / rstd are reduced from the partial records of the producing convolution
 * ([N][parts][G][2], mf_conv2d_gn_f32 / mf_conv2d_f16x2) by the first G threads of every workgroup while its first loads are in flight.
 * out_split NULL => fp32 output only (then the bound arguments are ignored).  The residual's bound is res_bound[N], or -- res_bound NULL --
 * the [N][res_nslots] slot maxima a convolution wrote (y_bound of mf_conv2d_f16x2), reduced inside the pass: no mf_bound_finalize_f32 launch. */
int mf_gn_apply_from_partials_f32(const float* x, const double* gn_partial, int parts, float eps, const float* gamma, const float* beta,
                                  const float* residual, const float* emb, int64_t emb_stride, float* out, void* out_split,
                                  const float* res_bound, const float* res_bound_slots, int res_nslots, const float* emb_bound, float bconst,
                                  float* out_bound, int N, int HW, int C, int G, int act, void* stream);
/* The same pass for tensors that exist ONLY as fp16 pairs between two convolutions (ABI 210; conv_blocks.py:236-240 where the block output
 * feeds convolutions and residual adds alone): `out` may be NULL -- only the pair form out_split is written, 12 instead of 16 bytes per
 * element -- and the residual may be given as pairs (`residual_pairs`, scaled by `res_bound`; `residual` must then be NULL): it is read back
 * as hi + lo/2048 times its scale, i.e. the fp32 value with its last significand bit cleared at most (<= 2^-23 relative, the order of the
 * rounding of the add itself). */
int mf_gn_apply_from_partials_pairs_f32(const float* x, const double* gn_partial, int parts, float eps, const float* gamma, const float* beta,
                                        const float* residual, const void* residual_pairs, const float* emb, int64_t emb_stride, float* out,
                                        void* out_split, const float* res_bound, const float* res_bound_slots, int res_nslots,
                                        const float* emb_bound, float bconst, float* out_bound, int N, int HW, int C, int G, int act, void* stream);
/* bound[n] = max |x[n][:]| over the FINITE values of per_row elements (NaN and +-Inf do not count: an Inf bound would store every finite
 * value of the row as zero): the measured operand bound of tensors no producer bounded analytically (network
 * input convolutions, embedding rows).  Two launches, no atomics: every wave stores the max of its share into its own slot of
 * `partial` (N * mf_maxabs_rows_slots(per_row) floats of caller scratch), then one wave per row reduces the slots.
 * mf_bound_finalize_f32 is that second pass on its own: it turns the slot array a convolution filled (y_bound of mf_conv2d_f16x2)
 * into bound[n]. */
int mf_maxabs_rows_slots(int64_t per_row);
int mf_maxabs_rows_f32(const float* x, float* partial, float* bound, int N, int64_t per_row, void* stream);
int mf_bound_finalize_f32(const float* partial, float* bound, int N, int slots, void* stream);

/* ------------------------------------------------------------------ small dense ops
 * mf_linear_f32: y[b*y_stride + o] = sum_i f(x[b*x_stride + i]) * w[o*In + i] + bias[o] (+ y if accumulate);
 * f = Swish if act_in else identity.  Replaces nn.Linear at time_embedder.py:66-71 and the
 * local_embedder Swish->Linear at conv_blocks.py:340-344,349-353 (all 17 batched into one call by the host).
 */
int mf_linear_f32(const float* x, int64_t x_stride, const float* w, const float* bias, float* y, int64_t y_stride,
                  int B, int In, int Out, int act_in, int act_out, int accumulate, void* stream);
/* SinusoidalPosEmb (time_embedder.py:15-28): out[b][0:half] = sin(t f_k), [half:2half] = cos(t f_k),
 * f_k = exp(-(ln(max_period)/(half - shift)) k); flip swaps halves; odd dim zero-padded.
 * freqs: optional device table f_k[half] precomputed by the host exactly like the reference (a 1-ulp difference
 * in f_k is amplified by t ~ 1000); NULL = compute with device expf. */
int mf_sinusoidal_f32(const float* t, const float* freqs, float* out, int B, int dim, float max_period, float shift, int flip, void* stream);
/* LearnedSinusoidalPosEmb (ABI 220; time_embedder.py:31-49): out[b] = [t_b | sin(2 pi t_b w_k) | cos(2 pi t_b w_k) | 0 if emb_dim is odd],
 * k < emb_dim / 2, row length 1 + 2 (emb_dim / 2) + (emb_dim & 1); the angle is formed in the reference's order ((t w) 2) pi in fp32.
 * (The reference's TimeEmbbeding cannot hold this embedder -- its first Linear takes emb_dim features, this returns emb_dim + 1 -- so it
 * is a stand-alone module there and here.) */
int mf_learned_sinusoidal_f32(const float* t, const float* weights, float* out, int B, int emb_dim, void* stream);
/* LabelEmbedder lookup + save_add (cond_embedders.py:19-24, conv_blocks.py:16-18): io[b][:] += table[idx[b]][:] */
int mf_embedding_add_f32(const float* table, const int64_t* idx, float* io, int B, int D, int num_rows, void* stream);

/* ------------------------------------------------------------------ scheduler step (one fused elementwise pass)
 * Replaces the ~49 ATen ops/step of DiffusionPipeline.forward :240-273 (CFG combine, objective switch),
 * GaussianNoiseScheduler.estimate_x_0 :119-124, estimate_x_T :127-131, estimate_mean_t :104-107,
 * estimate_variance_t :110-116, estimate_x_t_prior_from_x_0 :85-101 and the DDIM update
 * diffusion_pipeline.py:297-304.  Per-step scalars are computed on the host in fp32 exactly as the
 * reference computes them and live in a device table; the step index may come from device memory so a
 * captured hipGraph replays unchanged (no host sync, unlike the reference's `alphas_cumprod[t]`).
 * Products are rounded separately (no FMA contraction) to mirror ATen's elementwise chain.
 */
typedef struct MfSchedStep {
  float sqrt_recip_ac;    /* sqrt_recip_alphas_cumprod[t] */
  float sqrt_recipm1_ac;  /* sqrt_recipm1_alphas_cumprod[t] */
  float coef1, coef2;     /* posterior_mean_coef1/2[t] */
  float std_fixed;        /* exp(0.5*log(clamp(posterior_variance[t],1e-20))), 0 when t == 0 (var_scale == 0 path) */
  float log_var_min;      /* log(clamp(posterior_variance[t])) -- learned-variance path */
  float log_var_max;      /* log(clamp(betas[t])) */
  float ddim_sqrt_an;     /* sqrt(alphas_cumprod[t_next]) */
  float ddim_c;           /* sqrt(1 - alpha_next - sigma^2) */
  float ddim_sigma;       /* eta * sqrt((1 - a/a_next)(1 - a_next)/(1 - a)), eta == 1 */
  int32_t t;              /* timestep value (for t == 0 test) */
  int32_t mode;           /* 0: x_t <- x_t_prior (DDPM / last DDIM iteration); 1: DDIM update */
} MfSchedStep;

typedef struct MfSchedArgs {
  const float* x_t;          /* [n] current latent */
  const float* pred;         /* [n] estimator output (conditional pass when CFG) */
  const float* pred_uncond;  /* [n] or NULL: CFG pred = pu + g*(pred - pu) */
  const float* pred_var;     /* [n] or NULL: learned variance head (estimate_variance=True, g == 1 only) */
  const float* noise_post;   /* base of posterior-noise bank */
  const float* noise_ddim;   /* base of DDIM-noise bank (unused when mode == 0) */
  int64_t noise_step_stride; /* elements between consecutive steps in the banks (0: same buffer each step) */
  float* x_t_out;            /* [n] next latent (may alias x_t) */
  float* x0_out;             /* [n] or NULL: x_0 estimate of this step */
  float* xT_out;             /* [n] or NULL: x_T estimate of this step */
  const MfSchedStep* table;  /* device table, one entry per loop iteration */
  const int32_t* step_dev;   /* device step counter or NULL (then `step` is used) */
  int32_t step;
  int32_t objective;         /* 0: 'x_T', 1: 'x_0' */
  int32_t clip_x0;           /* clamp x_0 to [-1, 1] */
  float guidance_scale;
  int64_t n;                 /* elements */
} MfSchedArgs;
int mf_sched_step_f32(const MfSchedArgs* a, void* stream);
/* The tail of a denoise iteration in ONE launch (ABI 220): the posterior draw and the DDIM draw of mf_philox_normal_f32 (draw indices
 * draw_base + draw_stride * step and + 1, rows sample_offset .. + B) are generated in registers, mf_sched_step_f32's arithmetic runs on
 * them -- bit for bit what the three launches produce -- and *step_counter (read as the step; a->step_dev / a->step are ignored) is
 * incremented by the workgroup that finishes last (`ticket`: one zero-initialised word the launch leaves zero).  a->noise_post / noise_ddim
 * must be NULL.  Replaces torch.randn_like x 2 + the ~49 elementwise ATen ops + the host loop counter of diffusion_pipeline.py:294-304. */
int mf_sched_step_philox_f32(const MfSchedArgs* a, uint64_t seed, int32_t draw_base, int32_t draw_stride, int64_t sample_offset, int B,
                             int32_t* step_counter, uint32_t* ticket, void* stream);
/* Inpainting inside the step's launch (img2img / masked sampling; additive to ABI 250).  After the step has produced the next latent, the cells
 * the caller KEEPS take the known latent at the next timestep, built from the same draw every time:
 *   x_t_out[i] = mask[sample][cell] ? x_t_out[i] : coef[step].a * z0[i] + coef[step].c * eps0[i]
 * with the two products rounded separately and then the sum (mf_rows_axpby_f32's chain = GaussianNoiseScheduler.estimate_x_t,
 * gaussian_scheduler.py:61-77, at t_next; (1, 0) after the last iteration: the kept cells end as z0).  x0_out / xT_out stay the estimator's
 * estimates.  `step` is the index mf_sched_step_f32 uses for its MfSchedStep table (a->step / *a->step_dev, or *step_counter of the Philox form). */
typedef struct MfSchedBlend {
  const float* z0;       /* [n] the known latent (same layout as x_t: [B][channels][cells]) */
  const float* eps0;     /* [n] the draw that diffused z0 to the loop's first timestep */
  const uint8_t* mask;   /* [B][cells] one byte per latent cell: != 0 regenerate, 0 keep */
  const float* coef;     /* device table of (a, c) pairs, one per loop iteration */
  int64_t cells;         /* spatial cells per sample (h * w, or d * h * w) */
  int32_t channels;      /* latent channels (the mask is broadcast over them) */
  int32_t reserved;      /* 0 */
} MfSchedBlend;
int mf_sched_step_blend_f32(const MfSchedArgs* a, const MfSchedBlend* blend, void* stream);
/* mf_sched_step_philox_f32 with the select above on its x_t_out, still ONE launch: cells % 4 == 0, z0 / eps0 16-byte and mask 4-byte aligned. */
int mf_sched_step_philox_blend_f32(const MfSchedArgs* a, uint64_t seed, int32_t draw_base, int32_t draw_stride, int64_t sample_offset, int B,
                                   int32_t* step_counter, uint32_t* ticket, const MfSchedBlend* blend, void* stream);
/* The deterministic solver step (few-step sampling; additive to ABI 250): DDIM with eta = 0 and DPM-Solver++(2M) in data-prediction form.
 * Front half = mf_sched_step_f32's (CFG combine, x_0 / x_T estimates by objective, clip_x0: x0_out / xT_out are bit-equal to what that entry
 * point writes for the same inputs); back half = one MfSolverStep row, every product rounded on its own, sums left to right:
 *   MF_SOLVER_FINAL   x_t_out = x_0                               (the loop's last iteration)
 *   MF_SOLVER_DDIM0   x_t_out = B * x_0 + A * x_T                 (diffusion_pipeline.py:297-304 at sigma = 0: B = sqrt(a_next), A = sqrt(1 - a_next))
 *   MF_SOLVER_ORDER1  x_t_out = A * x_t + B * x_0                 (2M, first executed transition: no history yet)
 *   MF_SOLVER_ORDER2  x_t_out = A * x_t + B * x_0 + C * x_0_prev  (2M; x_0_prev = the previous iteration's x_0)
 * x0_hist: caller-owned [2][n]; every launch writes its x_0 to slot (step & 1), MF_SOLVER_ORDER2 reads slot ((step + 1) & 1); no other mode
 * loads it (it may be uninitialised).  It may be NULL when no row is MF_SOLVER_ORDER2 (such a row then yields NaN).  The step comes from
 * *step_counter when given -- then the workgroup that finishes last advances it, with `ticket` one zero-initialised word the launch leaves
 * zero, as in mf_sched_step_philox_f32 -- else from *step_dev, else from `step`.  No noise is drawn.  16-byte vectors when every tensor
 * is 16-byte aligned, element by element otherwise; any n. */
enum { MF_SOLVER_FINAL = 0, MF_SOLVER_DDIM0 = 1, MF_SOLVER_ORDER1 = 2, MF_SOLVER_ORDER2 = 3 };
typedef struct MfSolverStep {
  float sqrt_recip_ac;    /* sqrt_recip_alphas_cumprod[t] */
  float sqrt_recipm1_ac;  /* sqrt_recipm1_alphas_cumprod[t] */
  float A, B, C;          /* see the modes above; unused ones 0 */
  int32_t t;              /* timestep value */
  int32_t mode;           /* MF_SOLVER_* */
  int32_t reserved;       /* 0 */
} MfSolverStep;
typedef struct MfSolverArgs {
  const float* x_t;          /* [n] current latent */
  const float* pred;         /* [n] estimator output (conditional pass when CFG) */
  const float* pred_uncond;  /* [n] or NULL: CFG pred = pu + g*(pred - pu) */
  float* x_t_out;            /* [n] next latent (may alias x_t) */
  float* x0_out;             /* [n] or NULL: x_0 estimate of this step */
  float* xT_out;             /* [n] or NULL: x_T estimate of this step */
  float* x0_hist;            /* [2][n] or NULL: the x_0 history */
  const MfSolverStep* table; /* device table, one entry per executed iteration */
  int32_t* step_counter;     /* device step counter the launch advances, or NULL */
  uint32_t* ticket;          /* with step_counter: one zero-initialised word */
  const int32_t* step_dev;   /* device step index (read only) or NULL (then `step` is used) */
  int32_t step;
  int32_t objective;         /* 0: 'x_T', 1: 'x_0' */
  int32_t clip_x0;           /* clamp x_0 to [-1, 1] */
  float guidance_scale;
  int64_t n;                 /* elements */
} MfSolverArgs;
int mf_solver_step_f32(const MfSolverArgs* a, void* stream);
/* the same with mf_sched_step_blend_f32's select on x_t_out (coef[step] of the executed grid); x0_out / xT_out / x0_hist stay the estimates */
int mf_solver_step_blend_f32(const MfSolverArgs* a, const MfSchedBlend* blend, void* stream);
/* The stochastic solver step (few-step stochastic sampling; additive to ABI 250): DDIM at eta = 1 on any grid and SDE-DPM-Solver++(2M) in
 * data-prediction form.  Front half and deterministic back half are mf_solver_step_f32's exactly (same rounding, same history slots, same three
 * sources of the step index, same ticket); then
 *   x_t_out = det + scale[step] * eps      (the product rounded on its own, then one add; an MF_SOLVER_FINAL row draws and adds nothing)
 * and, with `blend`, mf_solver_step_blend_f32's select AFTER the noise.  eps is either
 *   noise != NULL  the caller's draw: element i of the launch reads noise[step * noise_step_stride + i] (stride 0: one [n] buffer; n: a bank); any n,
 *                  16-byte vectors when everything is aligned (noise and a stride that is a multiple of 4 included), element by element otherwise;
 *   noise == NULL  generated in registers: the values mf_philox_normal_f32 writes for (seed, draw = draw_base + draw_stride * step, rows
 *                  sample_offset .. + B).  Refused (MF_EUNSUPPORTED) where that function refuses -- elements per sample not a multiple of 4 -- and
 *                  where the launch could not run on 16-byte vectors (an unaligned tensor; a blend whose cells are not a multiple of 4).
 * `step` is the index the deterministic part resolves, so a replayed command list or graph needs no per-iteration argument.  No host
 * synchronisation, no allocation, capture-safe, one launch. */
typedef struct MfSolverNoise {
  const float* scale;        /* device table of fp32 noise scales, one per executed iteration */
  const float* noise;        /* the caller's draw, or NULL: Philox inside the launch */
  int64_t noise_step_stride; /* elements between consecutive steps in `noise` (0: the same buffer each step) */
  uint64_t seed;             /* Philox form: the key of mf_philox_normal_f32 */
  int64_t sample_offset;     /* Philox form: global index of row 0 */
  int32_t draw_base;
  int32_t draw_stride;       /* draw = draw_base + draw_stride * step */
  int32_t B;                 /* Philox form: samples in the launch (n / B elements each) */
  int32_t reserved;          /* 0 */
} MfSolverNoise;
int mf_solver_step_noise_f32(const MfSolverArgs* a, const MfSolverNoise* nz, const MfSchedBlend* blend_or_null, void* stream);
/* The trajectory of an inversion inside the solver step's launch (DDIM inversion / counterfactual editing; additive to ABI 250).  `traj` is a
 * caller-owned [slots][n] buffer; the launch touches slot = slot0 + slot_stride * step, `step` being the index mf_solver_step_f32 resolves
 * (*step_counter, *step_dev or a->step), so a replayed loop walks the buffer up (record) or down (keep) with no per-iteration pointer:
 *   MF_TRAJ_RECORD  x_t_out[i] and traj[slot][i] receive the same value (mf_solver_step_f32's x_t_out, bit for bit);
 *   MF_TRAJ_KEEP    x_t_out[i] = mask[sample][cell] ? mf_solver_step_f32's value : traj[slot][i]  (the mask of MfSchedBlend: != 0 regenerate).
 * x0_out / xT_out / x0_hist stay the estimates.  A slot outside [0, slots) is refused with MF_EINVAL when the step is known on the host; a
 * device-resolved step that lands outside touches no slot (nothing recorded; the kept cells become NaN).  traj must not overlap another tensor
 * of the launch.  16-byte vectors when every tensor is 16-byte aligned, n % 4 == 0 and (KEEP) cells % 4 == 0 with a 4-byte aligned mask;
 * element by element otherwise; any n. */
enum { MF_TRAJ_RECORD = 0, MF_TRAJ_KEEP = 1 };
typedef struct MfSolverTraj {
  float* traj;          /* [slots][n], caller-owned */
  const uint8_t* mask;  /* KEEP: [B][cells], != 0 regenerate, 0 keep; RECORD: NULL */
  int64_t cells;        /* KEEP: spatial cells per sample */
  int32_t channels;     /* KEEP: latent channels (the mask is broadcast over them) */
  int32_t mode;         /* MF_TRAJ_* */
  int32_t slot0;
  int32_t slot_stride;  /* slot = slot0 + slot_stride * step */
  int32_t slots;
  int32_t reserved;     /* 0 */
} MfSolverTraj;
int mf_solver_step_traj_f32(const MfSolverArgs* a, const MfSolverTraj* tr, void* stream);
/* out[n][cell] = (1 / C) * sum_c |a[n][c][cell] - b[n][c][cell]| on NCHW / NCDHW fp32, the channels summed in index order: the change map of
 * an edit (out is [N][1][cells]). */
int mf_absdiff_mean_c_f32(const float* a, const float* b, float* out, int N, int C, int64_t cells, void* stream);
/* out[n][c][cell] = mask[n][cell] ? a[n][c][cell] : b[n][c][cell] on NCHW / NCDHW fp32, the per-cell mask broadcast over the C channels: the
 * pixel-space composite of inpainting and the un-fused form of the select above. */
int mf_select_cells_f32(const uint8_t* mask, const float* a, const float* b, float* out, int N, int C, int64_t cells, void* stream);
/* [N][1][D][H][W] mask (uint8: != 0; mask_is_f32 = 1: fp32 > 0.5; D = 1 in 2-D) -> [N][1][D/fd][H/fh][W/fw] uint8 0 / 1 by max over fd x fh x fw
 * blocks: an image-resolution mask reduced to the latent's cells (a cell is regenerated if any of its pixels is). */
int mf_mask_maxpool_u8(const void* mask, int mask_is_f32, uint8_t* out, int N, int D, int H, int W, int fd, int fh, int fw, void* stream);
/* Windowed denoising of a canvas larger than the trained size (MultiDiffusion; additive to ABI 250).  A canvas [B][C][D][H][W] fp32 (D = 1 and
 * dims = 2 for images) is covered by M = count[0] * count[1] * count[2] windows of extent window[0..2], window m = (k0 * count[1] + k1) * count[2]
 * + k2 (last axis fastest) starting at (origin[0][k0], origin[1][k1], origin[2][k2]).  Origins ascend strictly on every axis, start at 0, end at
 * canvas - window and never leave a gap (origin[a][k + 1] - origin[a][k] <= window[a]), so every cell is covered.  The window tensor is
 * [B * M][C][d][h][w], row b * M + m = window m of canvas row b (sample-major).
 *   mf_window_gather_f32  windows[b * M + m] = the crop of canvas[b]: a copy, bit for bit.
 *   mf_window_merge_f32   canvas_out[cell] = sum_m w_m p_m / sum_m w_m over the windows m that cover the cell, visited in ASCENDING m:
 *                         acc = fmaf(w_m, p_m, acc), den += w_m, then one division.  A cell that exactly ONE window covers takes that window's
 *                         value bit for bit (no multiply, no divide).  w_m is the product over the axes of the profile at the cell's offset i
 *                         inside the window: MF_WINDOW_UNIFORM 1; MF_WINDOW_TENT min(i + 1, extent - i) (small integers: exact in fp32).
 *                         No atomics, a fixed order: the same bits on every launch.
 * B is the number of canvas rows of the launch (2 B' for the classifier-free-guidance pair).  Both are plain stream launches that allocate
 * nothing and read nothing on the host (command list / graph capture).  16-byte vectors along the last axis when canvas[2], window[2] and every
 * origin[2][k] are multiples of 4 and both tensors are 16-byte aligned; element by element otherwise.  The tensors must not overlap. */
enum { MF_WINDOW_UNIFORM = 0, MF_WINDOW_TENT = 1 };
#define MF_WINDOW_MAX_PER_AXIS 32
typedef struct MfWindowDesc {
  int32_t dims;                                 /* 2 or 3 (2: canvas[0] = window[0] = count[0] = 1, origin[0][0] = 0) */
  int32_t canvas[3];                            /* D, H, W of the canvas */
  int32_t window[3];                            /* d, h, w of a window (<= canvas) */
  int32_t count[3];                             /* origins per axis, 1 .. MF_WINDOW_MAX_PER_AXIS */
  int32_t origin[3][MF_WINDOW_MAX_PER_AXIS];    /* ascending; entries past count[a] are ignored */
  int32_t weight;                               /* MF_WINDOW_* */
  int32_t B;                                    /* canvas rows */
  int32_t C;                                    /* channels */
  int32_t reserved;                             /* 0 */
} MfWindowDesc;
int mf_window_gather_f32(const float* canvas, float* windows, const MfWindowDesc* desc, void* stream);
int mf_window_merge_f32(const float* windows, float* canvas_out, const MfWindowDesc* desc, void* stream);
/* out[0..n) = table[step] with step = *step_dev (or `step`): `t.expand(B)` of diffusion_pipeline.py:294 inside a captured graph */
int mf_broadcast_from_table_f32(const float* table, const int32_t* step_dev, int32_t step, float* out, int n, void* stream);
/* out[b][:] = table[step][cols[b]][:] for a [S][ncol][row_len] table, step = *step_dev (or `step`): the per-iteration gather of the
 * embedding rows UNet.precompute_embeddings hoisted out of the loop (unet2.py:229-241, conv_blocks.py:340-353), usable inside a captured graph. */
int mf_gather_step_rows_f32(const float* table, const int64_t* cols, const int32_t* step_dev, int32_t step, int ncol, int64_t row_len,
                            float* out, int B, void* stream);
/* Up to three such gathers in ONE launch (ABI 220): the embedding rows, the local-embedder rows and their bounds share `cols` and the step. */
int mf_gather_step_rows3_f32(const float* const* tables, const int64_t* row_lens, float* const* outs, int n_tables, const int64_t* cols,
                             const int32_t* step_dev, int32_t step, int ncol, int B, void* stream);
/* *counter += inc (one thread); lets a captured graph advance its own step index. */
int mf_counter_add_i32(int32_t* counter, int32_t inc, void* stream);

/* Per-row scaled combination: out[b][:] = clamp?((a[b]*x[b][:] + c[b]*y[b][:]) / d[b]); y, a, c, d optional (NULL).
 * The scheduler's tensor-level API with a timestep PER ROW (gaussian_scheduler.py:61-77 estimate_x_t, :104-107, :119-131)
 * and the lerp of DiffusionPipeline.interpolate (diffusion_pipeline.py:329); coefficient rows are gathered on the host like
 * `extract()` (scheduler_base.py:43-46).  Bit-exact vs ATen's elementwise chain.  Every clamp of the library that restates a torch.clamp (this one,
 * clip_x0 of the scheduler / solver steps, the logvar of mf_diag_gaussian_*) keeps a NaN like torch.clamp does; +-Inf go to the nearer limit. */
int mf_rows_axpby_f32(const float* x, const float* y, const float* a, const float* c, const float* d, float* out, int B,
                      int64_t per_row, int do_clamp, float lo, float hi, void* stream);

/* ------------------------------------------------------------------ noise
 * Counter-based standard normals (Philox-4x32-10 + Box-Muller), shard-invariant: element quad q of sample
 * (sample_offset + b) in draw `draw` depends only on (seed, draw, sample index, q).  Stands in for
 * torch.randn_like at diffusion_pipeline.py:315(x_final), gaussian_scheduler.py:99, diffusion_pipeline.py:303.
 * draw index = draw_base + draw_stride * step where step = *step_dev (or `step`).
 * The sample index is one 32-bit word of the Philox counter: sample_offset + b is taken mod 2^32 (row 2^32 draws what row 0 draws), here
 * and in every launch that regenerates these values.  A uniform whose 24 bits are all ones is exactly 1.0 in fp32: where it is the radius
 * word, the pair of normals is (+-0, +-0), finite.
 */
int mf_philox_normal_f32(float* out, uint64_t seed, int32_t draw_base, int32_t draw_stride, const int32_t* step_dev,
                         int32_t step, int64_t sample_offset, int B, int64_t per_sample, void* stream);

/* ------------------------------------------------------------------ attention family (use_attention = 'linear'|'spatial')
 * mf_attention_f32: compute_attention (attention_blocks.py:35-43) on NHWC-token tensors:
 * q [B][Nq][H*d], k,v [B][Nk][H*d] -> out [B][Nq][H*d]; softmax((q s)(k s)^T) v per head, s = d^-0.25.
 */
int mf_attention_f32(const float* q, const float* k, const float* v, float* out, int B, int H, int Nq, int Nk, int d,
                     float scale, void* stream);
/* LayerNorm over the last dim (attention_blocks.py:22), rows x C */
int mf_layernorm_f32(const float* x, const float* gamma, const float* beta, float* out, int64_t rows, int C, float eps,
                     void* stream);
/* GEGLU gate (attention_blocks.py:23-24): out[r][c] = h[r][c] * gelu(h[r][C + c]), h is rows x 2C */
int mf_geglu_f32(const float* h, float* out, int64_t rows, int C, void* stream);
/* out = a + b (elementwise, n floats) -- the `x + out` skips of attention_blocks.py:124,193,230,287 */
int mf_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------ layout + egress
 * NCHW <-> NHWC for API-edge tensors and tests. */
int mf_nchw_to_nhwc_f32(const float* x, float* y, int N, int C, int H, int W, void* stream);
int mf_nhwc_to_nchw_f32(const float* x, float* y, int N, int C, int H, int W, void* stream);
/* DiagonalGaussianDistribution (latent_embedders.py:22-27): z = mean + exp(0.5*clamp(logvar,-30,20)) * noise,
 * moments NCHW [N][2C][HW] -> z [N][C][HW] */
int mf_diag_gaussian_sample_f32(const float* moments, const float* noise, float* z, int N, int C, int HW, void* stream);
/* its KL term (latent_embedders.py:29-31; ABI 220): kl[0] = 0.5 * sum(mean^2 + exp(logvar) - 1 - logvar) / N, logvar clamped like above, fp64
 * accumulation -- the `emb_loss` VAE.forward returns (:778), evaluation-time only */
int mf_diag_gaussian_kl_f32(const float* moments, float* kl, int N, int C, int HW, void* stream);

/* VectorQuantizer.forward of VQVAE / VQGAN (latent_embedders.py:40-71; additive to ABI 250): nearest-codebook search, gather and loss term.
 * z NCHW [N][C][HW] fp32 (what the sampler hands to decode), codebook [K][C] fp32 (nn.Embedding weight, key quantizer.embedder.weight) ->
 *   z_q NCHW [N][C][HW] = z + (e_idx - z) in fp32 (the reference's straight-through value :67, which can differ from the code row by an ulp),
 *   idx[N*HW] int32 (optional, NULL: not written), pixel order n * HW + hw,
 *   sqerr[0] = sum over all elements of (e_idx - z)^2, each square in fp32, summed in fp64 (optional, NULL) -- the reference's
 *   emb_loss = (1 + beta) * sqerr / (N * C * HW) (:62).
 * Distance: the reference's cancelling formula d_k = (sum_c z_c^2 + sum_c e_kc^2) - 2 * sum_c z_c e_kc (:51-54), every sum in fp32 in index
 * order, no contraction; d may be negative.  argmin (:56): equal distances resolve to the LOWEST index; a NaN distance beats every number and
 * the first NaN wins (torch.argmin).  The result does not depend on launch order (the codebook slices combine through a commutative 64-bit
 * minimum; the loss partials are summed in a fixed order): two calls give bit-identical outputs.
 * 1 <= C <= 16 (larger: MF_EUNSUPPORTED), K >= 1, N = 0 returns at once.  workspace: mf_vq_workspace_bytes(N * HW) bytes of caller scratch.
 * 3 launches, a 4th with sqerr. */
size_t mf_vq_workspace_bytes(int64_t pixels);
int mf_vector_quantize_f32(const float* z, const float* codebook, float* z_q, int32_t* idx, double* sqerr, void* workspace,
                           size_t workspace_bytes, int N, int C, int HW, int K, void* stream);

/* --- 3-D convolution (spatial_dims=3; additive to ABI 250): MONAI Convolution with Conv[CONV, 3] at conv_blocks.py:48,169,229 -- BasicBlock /
 * BasicResBlock / UnetBasicBlock / UnetResBlock convolutions, BasicDown (stride 2 or (1, 2, 2)), BasicUp (nearest x2 per axis, then 3x3x3), the
 * fused torch.cat([h, skip]) of unet2.py:259 -- on the MF_CONV_FP32_F16X2 arithmetic (the only one built in 3-D).
 * Operands: x1 / x2 NDHWC fp16 pairs, i.e. what mf_split_f16x2 / mf_gn_apply_*_pairs / mf_pack_nchw_pairs_f32 write for the [N, D*H, W, C] view
 * of an NDHWC tensor, with per-sample bounds [N] (or NULL: unscaled); C1 and C2 whole 32-channel chunks (a network input with fewer channels is
 * zero-padded: mf_pack_nchw_pairs_f32 with HW = D*H*W, CP = 32).  Weights: mf_pack_conv3d_weight_f32 (OIDHW -> [Cout][KD][KH][KW][cin_pad],
 * input channels Cin.. zero), then split into pairs once by mf_split_f16x2 under their max |w| (= w_bound).  y: fp32 NDHWC [N][Do][Ho][Wo][Cout]
 * plus bias.  Any Cout >= 1 (masked on store).  Split-K slices go to `workspace` (mf_conv3d_workspace_bytes) and are summed in slice order by a
 * second launch: bit-identical from run to run.  mf_conv3d_ok(d) == 1 guarantees that mf_conv3d_f16x2 accepts d (with that workspace). */
typedef struct MfConv3dDesc {
  int32_t N, D, H, W;      /* batch, input size per axis (BEFORE a fused upsample) */
  int32_t C1, C2;          /* channels of x1 and x2 (C2 = 0: single source), multiples of 32 */
  int32_t Cout;
  int32_t k;               /* 1 or 3 on every axis */
  int32_t stride[3];       /* per axis (d, h, w): 1 or 2 */
  int32_t pad[3];          /* per axis: MONAI get_padding(k, stride) */
  int32_t upsample[3];     /* per axis: 1 = nearest x2 of the input folded into the gather (source voxel u >> 1) */
  int32_t tile_hint;       /* 0 = planner; 1..4 = 64x64, 128x64, 64x128, 128x128 voxels x channels */
  int32_t splitk_hint;     /* 0 = planner; else 1..16 slices of the (chunk, tap) loop */
  int32_t precision;       /* must be MF_CONV_FP32_F16X2 */
} MfConv3dDesc;
int mf_conv3d_ok(const MfConv3dDesc* d);
int mf_conv3d_out_dims(const MfConv3dDesc* d, int32_t* out3);
int mf_conv3d_plan_query(const MfConv3dDesc* d, int32_t* tile, int32_t* splitk);
size_t mf_conv3d_workspace_bytes(const MfConv3dDesc* d);
int mf_pack_conv3d_weight_f32(const float* w_oidhw, float* out, int Cout, int Cin, int k, int cin_pad, void* stream);
int mf_conv3d_f16x2(const void* x1_pairs, const void* x2_pairs, const void* w_pairs, const float* bias, float* y, const float* x1_bound,
                    const float* x2_bound, float w_bound, void* workspace, size_t workspace_bytes, const MfConv3dDesc* d, void* stream);

/* learnable_interpolation=False (ABI 210): BasicDown = nn.AvgPool2d(k, stride, get_padding(k, stride)) (conv_blocks.py:57-63; count_include_pad
 * like torch's default: the divisor counts the padding), BasicUp = F.interpolate(nearest-exact) to twice the size (conv_blocks.py:128-130).
 * NHWC fp32, C % 4 == 0. */
int mf_avgpool2d_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int k, int stride, int pad, void* stream);
int mf_upsample_nearest2x_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* The `use_res` skips of BasicDown / BasicUp (conv_blocks.py:54-55,68-69 and :114-115,125-126), added in place to the convolution's output:
 * y [N][H/2][W/2][4C] += PixelUnshuffle(2)(x [N][H][W][C])   (channel c * 4 + dy * 2 + dx <- pixel (2h + dy, 2w + dx), torch's order), H, W even;
 * y [N][2H][2W][C/4]  += PixelShuffle(2)(x [N][H][W][C]),    C % 4 == 0. */
int mf_pixel_unshuffle2_add_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
int mf_pixel_shuffle2_add_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* Image egress on the device: NCHW float -> NHWC uint8.
 * mode 0: scripts/helpers/sample_dataset.py:44-53  clip(-1,1) -> (x+1)/2*255 -> astype(uint8)   (bit-exact vs numpy)
 * mode 1: scripts/sample.py:49-51 + torchvision save_image(normalize=True, scale_each=True): (x+1)/2, clamp(0,1), per-image
 *         min-max, mul(255).add(0.5).clamp(0,255).to(uint8); minmax_ws = 2*N floats of caller scratch. */
int mf_image_egress_u8(const float* x_nchw, uint8_t* out_nhwc, float* minmax_ws, int N, int C, int H, int W, int mode, void* stream);
/* Image ingress, the inverse (additive to ABI 250): NHWC uint8 -> NCHW float in [-1, 1] by (x / 255 - 0.5) / 0.5, bit-exact against
 * tF.normalize(x / 255, 0.5, 0.5) (scripts/evaluate_latent_embedder.py:77). */
int mf_image_ingress_u8(const uint8_t* x_nhwc, float* out_nchw, int N, int C, int H, int W, void* stream);

/* Image-quality metrics on the device (additive to ABI 250): SSIM / MS-SSIM / MSE of image PAIRS taken from two banks of fp32 NCHW images,
 * xbank [Nx][C][H][W] and ybank [Ny][C][H][W] (the same pointer twice for the pairwise diversity of one set).  Pair p compares xbank[ix[p]] with
 * ybank[iy[p]]; a null index array is the identity (then P <= the bank's rows).  Nothing is gathered into per-pair copies.  An index outside
 * its bank makes that pair's results NaN and reads nothing.
 *   mf_ssim_pairs_f32   ONE scale of all P pairs in one launch.  The window is taps (x) taps (k taps by value in the descriptor, the caller
 *                       normalises them), VALID positions only: (H - k + 1) x (W - k + 1) windows per channel.  Per window mu_x, mu_y, E[x^2],
 *                       E[y^2], E[xy]; c1 = (k1 L)^2, c2 = (k2 L)^2; cs = (2 s_xy + c2) / (s_x^2 + s_y^2 + c2), ssim = (2 mu_x mu_y + c1) /
 *                       (mu_x^2 + mu_y^2 + c1) * cs.  L is data_range, or with range_on_device = 1 max(max x - min x, max y - min y) of the
 *                       pair, formed in the kernel from minmax_x [Nx][2] / minmax_y [Ny][2] (mf_rows_minmax_f32 of the scale-0 banks): no host
 *                       sync.  The second moments are taken about a per-tile pivot, so a near-constant region does not cancel.  A workgroup owns
 *                       32 x 32 window origins of one (pair, channel) and writes three fp64 partial sums (ssim, cs, and with want_mse (x - y)^2
 *                       over the pixels it owns) to the workspace: mf_ssim_workspace_bytes(desc) bytes, 8-byte aligned.  16-byte loads when
 *                       W % 4 == 0 and both banks are 16-byte aligned, element by element otherwise: the same bits either way, in sim, cs and mse (a thread
 *                       takes the same pixels in the same order on both).
 *   mf_ssim_finish_f32  adds each pair's partials in ascending (channel, tile) order in fp64 and writes sim[p * out_stride], cs[p * out_stride]
 *                       (the means over all channels and valid positions) and mse[p] (the mean over C H W; want_mse only) as fp32; any of the
 *                       three may be null.  out_stride lets a caller fill one column of a [P][S] table per scale.
 * No floating-point atomics: the same inputs give the same bits on every launch, and a pair's result depends neither on P nor on its place
 * among the pairs.  mf_ssim_ok / mf_ssim_workspace_bytes are host-only (the descriptor's rules: k odd in 3 .. MF_SSIM_MAX_K, H, W >= k,
 * 0 < P, C <= 65535, banks non-empty, P within an un-indexed bank); every entry point refuses a bad descriptor with MF_EINVAL before any launch.
 *   mf_avgpool2_planes_f32  y[pl][oy][ox] = ((x[2oy][2ox] + x[2oy][2ox+1]) + (x[2oy+1][2ox] + x[2oy+1][2ox+1])) / 4 on [planes][H][W] ->
 *                       [planes][H/2][W/2] (an odd trailing row or column is dropped): the next level of a bank's pyramid, built once per bank.
 *   mf_rows_minmax_f32  out[row] = {min, max} of x[row][0 .. n), both NaN when the row holds a NaN; one workgroup per row. */
#define MF_SSIM_MAX_K 11
typedef struct MfSsimDesc {
  int32_t P, C, H, W;             /* pairs, channels, extents of THIS scale */
  int32_t Nx, Ny;                 /* rows of the two banks */
  int32_t k;                      /* taps: odd, 3 .. MF_SSIM_MAX_K */
  int32_t indexed;                /* bit 0: ix is given, bit 1: iy is given */
  int32_t want_mse;               /* 1: also sum (x - y)^2 (scale 0) */
  int32_t range_on_device;        /* 1: L from minmax_x / minmax_y; 0: data_range */
  float taps[MF_SSIM_MAX_K];      /* the 1-D window, entries past k ignored */
  float k1, k2, data_range;
} MfSsimDesc;
int mf_ssim_ok(const MfSsimDesc* desc);
size_t mf_ssim_workspace_bytes(const MfSsimDesc* desc);
int mf_ssim_pairs_f32(const float* xbank, const float* ybank, const int32_t* ix, const int32_t* iy, const float* minmax_x, const float* minmax_y,
                      void* workspace, size_t workspace_bytes, const MfSsimDesc* desc, void* stream);
int mf_ssim_finish_f32(const void* workspace, float* sim, float* cs, float* mse, int out_stride, const MfSsimDesc* desc, void* stream);
int mf_avgpool2_planes_f32(const float* x, float* y, int64_t planes, int H, int W, void* stream);
int mf_rows_minmax_f32(const float* x, float* out, int N, int64_t n, void* stream);

/* The same metrics of VOLUMES (additive to ABI 250): SSIM / MS-SSIM / MSE of pairs taken from two banks of fp32 NCDHW volumes, xbank
 * [Nx][C][D][H][W] and ybank [Ny][C][D][H][W], under the index rules of the 2-D block above (a null index array is the identity; an index outside
 * its bank makes that pair NaN and reads nothing).
 *   mf_ssim3d_pairs_f32   ONE scale of all P pairs in one launch.  The window is taps (x) taps (x) taps, VALID positions only: (D - k + 1) x
 *                         (H - k + 1) x (W - k + 1) windows per channel; per window the cs and ssim of the 2-D block, c1 = (k1 L)^2, c2 = (k2 L)^2,
 *                         L = data_range or (range_on_device = 1) max(max x - min x, max y - min y) of the pair over the whole volume, from
 *                         minmax_x [Nx][2] / minmax_y [Ny][2] (mf_rows_minmax_f32 of the scale-0 banks).  A workgroup owns 16 x 16 in-plane
 *                         window origins over a chunk of 16 origins in depth and marches over the planes under them: each plane is filtered
 *                         in-plane through LDS, the depth pass keeps a ring of k partial sums per field in registers (fmaf chains in ascending
 *                         depth).  Second moments are taken about a per-workgroup pivot (its first voxel of x, of y), so a near-constant volume
 *                         does not cancel.  No intermediate field goes through global memory: the launch stores three fp64 partial sums per
 *                         workgroup (ssim, cs, and with want_mse (x - y)^2 over the voxels it owns) to the workspace:
 *                         mf_ssim3d_workspace_bytes(desc) = P C tiles 3 8 bytes, 8-byte aligned.  16-byte loads when W % 4 == 0 and both banks
 *                         are 16-byte aligned, element by element otherwise: the same bits either way, in sim, cs and mse.
 *   mf_ssim3d_finish_f32  adds each pair's partials in ascending (channel, tile) order in fp64 and writes sim[p * out_stride], cs[p * out_stride]
 *                         (the means over all channels and valid positions) and mse[p] (the mean over C D H W; want_mse only) as fp32; any of
 *                         the three may be null.
 * No floating-point atomics: the same inputs give the same bits on every launch, and a pair's result depends neither on P nor on its place
 * among the pairs.  mf_ssim3d_ok / mf_ssim3d_workspace_bytes are host-only (the rules: k odd in 3 .. MF_SSIM_MAX_K, D, H, W >= k,
 * 0 < P, C <= 65535, banks non-empty, P within an un-indexed bank); every entry point refuses a bad descriptor with MF_EINVAL before any launch.
 *   mf_avgpool2_volumes_f32  y[pl][oz][oy][ox] = the mean of the 2 x 2 x 2 block at (2 oz, 2 oy, 2 ox) on [planes][D][H][W] -> [planes][D/2][H/2][W/2]
 *                         (an odd trailing plane, row or column is dropped).  The eight are added one after the other in (depth, row, column)
 *                         order, ((((((v000 + v001) + v010) + v011) + v100) + v101) + v110) + v111, then multiplied by 1/8. */
typedef struct MfSsim3dDesc {
  int32_t P, C, D, H, W;          /* pairs, channels, extents of THIS scale */
  int32_t Nx, Ny;                 /* rows of the two banks */
  int32_t k;                      /* taps per axis: odd, 3 .. MF_SSIM_MAX_K */
  int32_t indexed;                /* bit 0: ix is given, bit 1: iy is given */
  int32_t want_mse;               /* 1: also sum (x - y)^2 (scale 0) */
  int32_t range_on_device;        /* 1: L from minmax_x / minmax_y; 0: data_range */
  float taps[MF_SSIM_MAX_K];      /* the 1-D window, entries past k ignored */
  float k1, k2, data_range;
} MfSsim3dDesc;
int mf_ssim3d_ok(const MfSsim3dDesc* desc);
size_t mf_ssim3d_workspace_bytes(const MfSsim3dDesc* desc);
int mf_ssim3d_pairs_f32(const float* xbank, const float* ybank, const int32_t* ix, const int32_t* iy, const float* minmax_x, const float* minmax_y,
                        void* workspace, size_t workspace_bytes, const MfSsim3dDesc* desc, void* stream);
int mf_ssim3d_finish_f32(const void* workspace, float* sim, float* cs, float* mse, int out_stride, const MfSsim3dDesc* desc, void* stream);
int mf_avgpool2_volumes_f32(const float* x, float* y, int64_t planes, int D, int H, int W, void* stream);

/* Improved precision / recall of two feature sets on the device (additive to ABI 250): squared distances between the rows of two contiguous fp32
 * feature banks [rows][D] on the fp32 matrix cores, the k-NN radius of every row of a bank, and the membership of query rows in a bank's manifold
 * -- the last two WITHOUT the rows x rows matrix ever being written.  The definition: xt = fl32(x - pivot), n(x) = the fp64 sum of xt_k^2 rounded
 * to fp32, d2(x, y) = max(0, fl32(fl32(n(x) + n(y)) - 2 dot(xt, yt))) with dot ONE fp32 fmaf chain over k ascending (v_mfma_f32_32x32x2_f32; no
 * split-K).  The bits of d2(i, j) depend on the two rows and the pivot only: not on N, M, the tile, the grid or the rows' places in their banks,
 * and d2(i, j) of (x, y) equals d2(j, i) of (y, x).  Sixteen-byte loads when D % 4 == 0 and the banks and the pivot are 16-byte aligned, element
 * loads otherwise: the same bits.  Every global access is masked: N, M and D are arbitrary.
 *   mf_feat_colmean_f32      pivot[k] = the fp64 mean of column k of x [N][D], rows added in a fixed order, rounded to fp32.
 *   mf_feat_norms_f32        norms[i] = n(x_i), one wave per row, fp64, a fixed order.
 *   mf_feat_sqdist_f32       out [N][M] = d2(x_i, y_j); with same_bank (x == y, nx == ny) the diagonal is stored as exactly 0.
 *   mf_knn_partial_f32       grid (row tiles of 128, `splits` column splits): every row's MF_FIDELITY_LIST smallest d2(x_i, x_j) over the split's column
 *                            tiles, ascending, the j == i entry counted as exactly 0, +inf where a split holds fewer; [splits][N][MF_FIDELITY_LIST]
 *                            floats to the workspace.  desc->N rows; desc->M is not read.
 *   mf_knn_finish_f32        merges the splits in ascending order: radii_sq[i] = the (knn + 1)-th smallest (the reference's topk(knn + 1), self included).
 *   mf_manifold_partial_f32  grid (query tiles of 128, `splits` splits of the reference rows): flag[s][j] = any_i [d2(ref_i, query_j) < radii_sq[i]]
 *                            (strict, on squared values) over the split's rows, as bytes [splits][M] to the workspace.  desc->N reference rows,
 *                            desc->M queries.
 *   mf_manifold_finish_f32   ORs the splits in ascending order: hit[j] (0 / 1) and count = the number of hits, by a fixed tree in one workgroup;
 *                            either output may be null.
 * No atomics: the same bits on every launch and for every `splits`.  Launches are asynchronous on `stream`; nothing is allocated, retained or
 * read back.  mf_fidelity_ok / mf_fidelity_workspace_bytes are host-only (the rules: 1 <= knn <= 15, knn < N, 1 <= N, M < 2^24, 1 <= D <= 65536,
 * 1 <= splits <= MF_FIDELITY_MAX_SPLITS, same_bank only with M == N); the workspace (16-byte aligned) serves either pair of launches:
 * max(splits N MF_FIDELITY_LIST 4, splits M rounded up to 16) bytes.  Every entry point refuses a bad descriptor with MF_EINVAL before any launch. */
#define MF_FIDELITY_LIST 16
#define MF_FIDELITY_MAX_SPLITS 16
typedef struct MfFidelityDesc {
  int32_t N, M, D;                /* rows of the first bank (the reference rows), rows of the second (the queries), features per row */
  int32_t knn;                    /* 1 .. 15, < N */
  int32_t splits;                 /* 1 .. MF_FIDELITY_MAX_SPLITS */
  int32_t same_bank;              /* 1: both banks are one (mf_feat_sqdist_f32: the diagonal is exactly 0) */
  int32_t reserved[2];
} MfFidelityDesc;
int mf_fidelity_ok(const MfFidelityDesc* desc);
size_t mf_fidelity_workspace_bytes(const MfFidelityDesc* desc);
int mf_feat_colmean_f32(const float* x, float* pivot, int N, int D, void* stream);
int mf_feat_norms_f32(const float* x, const float* pivot, float* norms, int N, int D, void* stream);
int mf_feat_sqdist_f32(const float* x, const float* nx, const float* y, const float* ny, const float* pivot, float* out, const MfFidelityDesc* desc,
                       void* stream);
int mf_knn_partial_f32(const float* x, const float* nx, const float* pivot, void* workspace, size_t workspace_bytes, const MfFidelityDesc* desc,
                       void* stream);
int mf_knn_finish_f32(const void* workspace, float* radii_sq, const MfFidelityDesc* desc, void* stream);
int mf_manifold_partial_f32(const float* ref, const float* nref, const float* radii_sq, const float* query, const float* nquery, const float* pivot,
                            void* workspace, size_t workspace_bytes, const MfFidelityDesc* desc, void* stream);
int mf_manifold_finish_f32(const void* workspace, uint8_t* hit, int32_t* count, const MfFidelityDesc* desc, void* stream);

/* Nearest neighbours with indices across two banks, the exact distance of listed pairs, and the counting form of the manifold launch (additive to
 * ABI 250; the same d2, tile and load paths as above).  MfFidelityDesc carries them: N = reference rows, M = query rows, knn = k, same_bank =
 * the query bank IS the reference bank and every row's own entry is left out (by index: another row with the same features stays a neighbour at 0).
 *   mf_nn_partial_f32              grid (query tiles of 128, `splits` splits of the reference rows): every query's MF_FIDELITY_LIST smallest pairs
 *                                  (d2(query_j, ref_i), i) over the split's reference tiles in ascending LEXICOGRAPHIC order -- d2 compared as a
 *                                  float (-0 counted as +0), then the smaller index i -- as 64-bit keys (the bits of d2 high, i low), (+inf, -1)
 *                                  where a split holds fewer; [splits][M][MF_FIDELITY_LIST] keys to the workspace.  The indices are unique, so the
 *                                  order is total: the result cannot depend on the tile, on `splits` or on the order of merging.
 *   mf_nn_finish_f32               merges the splits in ascending order: d2 [M][k] (fp32, the bits of mf_feat_sqdist_f32(query, ref)) and
 *                                  index [M][k] (int32), ascending by (d2, index).
 *   mf_pair_sqdist_f32             out [M][k] = fl32(sum over c of fl32(query[j][c] - ref[index[j][p]][c])^2), the sum in fp64 in a fixed order, one
 *                                  wave per pair, no pivot: equal rows give exactly 0, the relative error is at most 4 2^-24.  The index is
 *                                  clamped into the bank before any load; a pair whose index is outside 0 .. N - 1 is stored as +inf.
 *   mf_manifold_count_partial_f32  as mf_manifold_partial_f32, counting: part[s][j] = #{ i in split s : d2(ref_i, query_j) < radii_sq[i] } (strict),
 *                                  int32 [splits][M] to the workspace.
 *   mf_manifold_count_finish_f32   count[j] = the sum over the splits (int32), total = the sum of count[] (int64) by a fixed tree in one
 *                                  workgroup; either output may be null.  Integer sums: the same bits in any order.
 * No atomics on global memory.  mf_nn_ok / mf_nn_workspace_bytes are host-only.  The rules of these calls (MF_EINVAL before any launch):
 * 1 <= k <= MF_FIDELITY_LIST, k <= N (k <= N - 1 with same_bank), same_bank only with M == N (and, for mf_nn_partial_f32, query == ref), 1 <= N, M
 * < 2^24, 1 <= D <= 65536, 1 <= splits <= MF_FIDELITY_MAX_SPLITS.  The workspace (16-byte aligned) is splits M MF_FIDELITY_LIST 8 bytes; the
 * counting launches need splits M 4 bytes of it, rounded up to 16.  mf_fidelity_workspace_bytes keeps its meaning. */
int mf_nn_ok(const MfFidelityDesc* desc);
size_t mf_nn_workspace_bytes(const MfFidelityDesc* desc);
int mf_nn_partial_f32(const float* query, const float* nquery, const float* ref, const float* nref, const float* pivot, void* workspace,
                      size_t workspace_bytes, const MfFidelityDesc* desc, void* stream);
int mf_nn_finish_f32(const void* workspace, float* d2, int32_t* index, const MfFidelityDesc* desc, void* stream);
int mf_pair_sqdist_f32(const float* query, const float* ref, const int32_t* index, float* out, const MfFidelityDesc* desc, void* stream);
int mf_manifold_count_partial_f32(const float* ref, const float* nref, const float* radii_sq, const float* query, const float* nquery,
                                  const float* pivot, void* workspace, size_t workspace_bytes, const MfFidelityDesc* desc, void* stream);
int mf_manifold_count_finish_f32(const void* workspace, int32_t* count, int64_t* total, const MfFidelityDesc* desc, void* stream);

/* Kernel distances: the sum of a kernel k(x, y) over pairs of rows of two feature banks, for the Kernel Inception Distance and the unbiased MMD^2
 * (additive to ABI 250; the tile and the load paths of the calls above).  The definition:
 *   MF_KERNEL_POLY  v = fmaf(gamma, dot(x, y), coef0) in fp32, k = v, v v, (v v) v, (v v)(v v) for degree 1 .. 4, every product rounded to fp32; dot is
 *                   the ONE fp32 fmaf chain over k ascending of the distances, run on xt = fl32(x - pivot) with a pivot of ZEROS passed by the caller
 *                   (x - 0 is x bit for bit);
 *   MF_KERNEL_RBF   k = expf(fl32(-gamma d2)) with d2 exactly as above (pivot, norms of mf_feat_norms_f32).
 * The bits of k(i, j) depend on the two rows, the pivot and the scalars only -- not on the tile, the grid, N, M, the rows' places, the load path or
 * the subset -- and k(i, j) = k(j, i).
 *   mf_ksum_partial_f32  grid (the tiles of one subset pair, S subsets): subset s takes rows ia[s][0 .. sa) of bank a [N][D] and ib[s][0 .. sb) of bank
 *                        b [M][D] (int32 [S][sa], [S][sb]; null: the identity 0 .. sa - 1; an index is clamped into its bank before any load).  The
 *                        sum of k over each 128 x 128 tile of the sa x sb pairs, in fp64 in a fixed order, goes to the workspace as one double per
 *                        tile, [S][tiles].  same_bank = 1 or 2 (a == b, na == nb, ia == ib, sb == sa): only the tiles on or above the diagonal are
 *                        visited, an off-diagonal tile counts twice (exact in fp64); 1 leaves the pairs p == q out, by position, 2 counts them.
 *                        na, nb: the banks' norms, needed by MF_KERNEL_RBF only (else they may be null).
 *   mf_ksum_finish_f64   out[s] = the sum of subset s's tile sums in ascending tile order (256 consecutive runs, each ascending, added ascending).
 *   mf_feat_kernel_f32   out [N][M] = k(x_i, y_j) as fp32, the counterpart of mf_feat_sqdist_f32 (S, sa, sb and same_bank are checked, not used).
 * No atomics: the same bits on every launch, and a gathered subset gives the bits of the same call on its materialised rows.  mf_ksum_ok and
 * mf_ksum_workspace_bytes are host-only.  The rules (MF_EINVAL before any launch): 1 <= N, M < 2^24, 1 <= D <= 65536, 1 <= S <= 65535, 1 <= sa <= N,
 * 1 <= sb <= M, degree 1 .. 4 (poly), gamma finite and positive, coef0 finite, same_bank only with M == N and sb == sa, reserved 0, at most 2^31 - 1
 * tiles per subset pair.  The workspace (16-byte aligned) is 8 bytes per visited tile -- S ceil(sa / 128) ceil(sb / 128), or S T (T + 1) / 2 with
 * T = ceil(sa / 128) for same_bank -- rounded up to 16. */
#define MF_KERNEL_POLY 0
#define MF_KERNEL_RBF 1
typedef struct MfKernelSumDesc {
  int32_t N, M, D;                /* rows of bank a, rows of bank b, features per row */
  int32_t S;                      /* subsets, 1 .. 65535 */
  int32_t sa, sb;                 /* rows of a subset in bank a (<= N) and in bank b (<= M) */
  int32_t kernel;                 /* MF_KERNEL_POLY, MF_KERNEL_RBF */
  int32_t degree;                 /* 1 .. 4 (MF_KERNEL_POLY) */
  float gamma, coef0;
  int32_t same_bank;              /* 0: two banks; 1: one bank, the pairs p == q left out; 2: one bank, all pairs */
  int32_t reserved;               /* 0 */
} MfKernelSumDesc;
int mf_ksum_ok(const MfKernelSumDesc* desc);
size_t mf_ksum_workspace_bytes(const MfKernelSumDesc* desc);
int mf_ksum_partial_f32(const float* a, const float* na, const int32_t* ia, const float* b, const float* nb, const int32_t* ib, const float* pivot,
                        void* workspace, size_t workspace_bytes, const MfKernelSumDesc* desc, void* stream);
int mf_ksum_finish_f64(const void* workspace, double* out, const MfKernelSumDesc* desc, void* stream);
int mf_feat_kernel_f32(const float* x, const float* nx, const float* y, const float* ny, const float* pivot, float* out, const MfKernelSumDesc* desc,
                       void* stream);

/* Held-out denoising loss (the validation step of diffusion_pipeline.py:78-201 on the device; additive to ABI 250).  All tensors fp32, NCHW / NCDHW
 * contiguous, B rows of per_row elements; t is a device int32 [B]; the scheduler tables are device fp32 [T].  No host synchronisation, no allocation,
 * no atomics, capture-safe.
 *
 * mf_diffuse_rows_f32: the forward process with t PER ROW, GaussianNoiseScheduler.estimate_x_t (gaussian_scheduler.py:61-77):
 *   x_t[b] = sqrt_ac[t_b] x_0[b] + sqrt_1m_ac[t_b] eps[b], the two products rounded separately, then the sum (mf_rows_axpby_f32's chain on the
 *   gathered coefficients, bit for bit); a row with t_b < 0 returns x_0[b], one with t_b >= T returns eps[b], as the reference's clipper does.
 *   eps != NULL  the caller's draw; any per_row, 16-byte vectors when every tensor is 16-byte aligned and per_row % 4 == 0, else element by element;
 *   eps == NULL  generated in registers: the values mf_philox_normal_f32 writes for (seed, draw, rows sample_offset .. + B); eps_out (optional)
 *                receives them.  Refused (MF_EUNSUPPORTED) where mf_solver_step_noise_f32 refuses: per_row not a multiple of 4, an unaligned tensor. */
typedef struct MfDiffuseArgs {
  const float* x_0;
  const float* eps;          /* the caller's draw, or NULL: Philox inside the launch */
  float* x_t;
  float* eps_out;            /* Philox form only, optional: the draw */
  const int32_t* t;          /* [B], device */
  const float* sqrt_ac;      /* [T] sqrt_alphas_cumprod */
  const float* sqrt_1m_ac;   /* [T] sqrt_one_minus_alphas_cumprod */
  int64_t per_row;
  uint64_t seed;             /* Philox form: the key of mf_philox_normal_f32 */
  int64_t sample_offset;     /* Philox form: global index of row 0 */
  int32_t draw;
  int32_t T, B;
  int32_t reserved;          /* 0 */
} MfDiffuseArgs;
int mf_diffuse_rows_f32(const MfDiffuseArgs* a, void* stream);
/* mf_denoise_loss_f32 / mf_denoise_loss_finish_f32: per-row error sums of one prediction against its target.
 *   pred [B][C][D][H][W] (D = 1 and dims = 2 for images).  The target has extents (D f, H f, W f) -- (H f, W f) in 2-D -- for an integer pooling
 *   factor f >= 1 and is average-pooled on the fly: the pooled value is the fp32 sum of the f^dims block, added in (depth, row, column) order, divided
 *   by f^dims -- F.interpolate(mode='area') for a side that is a multiple of f (anything else cannot be described here).
 *   target != NULL  read from the tensor;
 *   target == NULL  regenerated in registers: the values mf_philox_normal_f32 writes for (seed, draw, rows sample_offset .. + B) of target shape
 *                   (MF_EUNSUPPORTED unless the target's elements per row are a multiple of 4): the draw is never stored.
 *   Per element d = fl32(pred - target); every lane adds |d| and d d in fp64 over its elements in ascending order, the 256 lanes of a workgroup meet
 *   in LDS by a fixed tree, and each workgroup writes two doubles: workspace [B][parts][2], parts = mf_loss_parts(per_row), 16 bytes per partial --
 *   mf_loss_workspace_bytes(B, per_row, 2) in all (parts <= 256; one partial covers at least 8192 elements).  The finish launch adds a row's partials
 *   in ascending order: out [B][2] fp64 = (sum |d|, sum d d).  A workgroup takes whole quads of 4 consecutive elements of a row; 16-byte loads of pred
 *   (and of an un-pooled target) when they are 16-byte aligned and per_row % 4 == 0, element by element otherwise -- the same elements in the same
 *   lanes in the same order.  The bits of a row's sums depend on that row's data only: not on B, the row's place, the load path, or whether the
 *   target was stored or regenerated. */
typedef struct MfLossDesc {
  int32_t B, C;
  int32_t dims;        /* 2 or 3 */
  int32_t size[3];     /* pred's D, H, W (D = 1 in 2-D) */
  int32_t f;           /* pooling factor of the target per axis, >= 1 */
  int32_t draw;        /* Philox target */
  uint64_t seed;
  int64_t sample_offset;
} MfLossDesc;
int mf_loss_parts(int64_t per_row);
size_t mf_loss_workspace_bytes(int B, int64_t per_row, int values);
int mf_denoise_loss_f32(const float* pred, const float* target_or_null, const MfLossDesc* d, void* workspace, size_t workspace_bytes, void* stream);
int mf_denoise_loss_finish_f32(const void* workspace, double* out, int B, int64_t per_row, void* stream);
/* mf_variance_loss_f32 / mf_variance_loss_finish_f32: the learned-variance terms of the validation step (diffusion_pipeline.py:152-173) per row, with
 * the same partial / finish scheme (three doubles per partial: mf_loss_workspace_bytes(B, per_row, 3)).  Per element, evaluated in fp64 on the fp32
 * data (inputs, tables, and the two clamp constants as an fp32 run holds them, 1e-20f and 1e-6f): at t = 0 exp(-pred_logvar) reaches e^46 and the
 * two terms of nll cancel, so one fp32 evaluation of an element is only good to ~2e-6 of it:
 *   vs = (pred_var + 1) / 2;  lmax = log(max(betas[t], 1e-20)), lmin = log(max(posterior_variance[t], 1e-20));
 *   pred_logvar = vs lmax + (1 - vs) lmin;  true_logvar = lmin;
 *   pred_x_0 = objective 0 ('x_T'): clip?(sqrt_recip_ac[t] x_t - sqrt_recipm1_ac[t] x_T) with the TRUE x_T (the reference's line 159, mirrored);
 *              objective 1 ('x_0'): pred;
 *   pred_mean = coef1[t] pred_x_0 + coef2[t] x_t,  true_mean = coef1[t] x_0 + coef2[t] x_t;
 *   kl  = 0.5 (pred_logvar - true_logvar + exp(true_logvar - pred_logvar) + (true_mean - pred_mean)^2 exp(-pred_logvar) - 1)   (math_utils.py);
 *   nll = 0.5 (log(v) + (pred_x_0 - x_0)^2 / v), v = max(exp(pred_logvar), 1e-6)                                           (F.gaussian_nll_loss).
 * out [B][3] fp64 = (sum kl, sum nll, sum vs).  The select t == 0 ? nll : kl belongs to the caller.  A row whose t is outside [0, T) reads no
 * table and gives NaN. */
typedef struct MfVarianceLossArgs {
  const float* x_0;
  const float* x_t;
  const float* x_T;
  const float* pred;
  const float* pred_var;
  const int32_t* t;                 /* [B], device */
  const float* betas;               /* the [T] tables of the scheduler */
  const float* posterior_variance;
  const float* coef1;               /* posterior_mean_coef1 */
  const float* coef2;               /* posterior_mean_coef2 */
  const float* sqrt_recip_ac;
  const float* sqrt_recipm1_ac;
  int64_t per_row;
  int32_t T, B;
  int32_t objective;                /* 0: 'x_T', 1: 'x_0' */
  int32_t clip_x0;
} MfVarianceLossArgs;
int mf_variance_loss_f32(const MfVarianceLossArgs* a, void* workspace, size_t workspace_bytes, void* stream);
int mf_variance_loss_finish_f32(const void* workspace, double* out, int B, int64_t per_row, void* stream);

/* Guidance stage (additive to ABI 250): what stands between the estimator and the scheduler / solver step of a denoise iteration when the guidance
 * scale follows a schedule, the guided prediction is rescaled (Lin et al. 2024, section 3.4) or the x_0 estimate is thresholded dynamically (Saharia
 * et al. 2022).  All tensors fp32, B rows of n contiguous elements.  No host synchronisation, no allocation, capture-safe; the launch sequence is
 * fixed by (B, n, stages).  Per row b, with the table row S = table[step_dev ? *step_dev : step]:
 *   1. p = fl(pu + fl(S.g fl(pc - pu))) -- the chain of the step launches; pred_uncond == NULL: p = pred.
 *   2. MF_GUIDE_RESCALE: sigma_pos, sigma_cfg = the unbiased standard deviations of pc and p over the row, from fp64 sums of the fp32 values about a
 *      pivot (an element of the row), added in a fixed order; k = fl32(S.phi sigma_pos / sigma_cfg + (1 - S.phi)) evaluated in fp64 and rounded once,
 *      k = 1 when sigma_cfg == 0 or n < 2; p <- fl(k p).
 *   3. MF_GUIDE_THRESHOLD: x0 = fl(fl(a x_t) - fl(b p)) for objective 0 ('x_T'; a = S.sqrt_recip_ac, b = S.sqrt_recipm1_ac), x0 = p for objective 1.
 *      v = the row's |x0| in ascending order of their bit patterns (torch.sort's order on finite values; a NaN sorts above +inf and is one more large
 *      magnitude, it does not poison the row as it does torch.quantile); pos = S.q (n - 1) in fp64 (S.q as the table's fp32 holds it), lo = floor(pos),
 *      hi = ceil(pos); s = fl32(v[lo] + (v[hi] - v[lo]) (pos - lo)) in fp64 (v[lo] itself when hi == lo); s <- max(s, 1) (a NaN s gives 1), and
 *      min(s, S.s_max) when S.s_max > 0.  x0' = clamp_keep_nan(x0, -s, s) / s; p <- x0' for objective 1, fl(fl(fl(a x_t) - x0') / b) for objective 0:
 *      the prediction that the step turns back into x0'.  v[lo] and v[hi] are EXACT: a most-significant-digit-first radix select (8-bit digits, four
 *      passes, integer counts through LDS atomics) on the non-negative bit patterns, both ranks at once.
 *   pred_out = p (it may be `pred` itself, nothing else); scale_out[b] = k (1 without the stage), limit_out[b] = s (0 without the stage), optional.
 * A caller then runs its step launch on pred_out with pred_uncond = NULL.
 * n <= MF_GUIDE_ROW_ONE_WG: ONE launch of B workgroups, the row held in registers.  Longer rows: workgroups of mf_guide_workspace_bytes' geometry
 * (at most 64 per row) in a fixed sequence -- combine (+ partial sums), then with the threshold four counting passes, then the apply pass: 1 launch
 * without a stage, 2 with the rescale alone, 6 with the threshold -- through a caller-owned workspace that no launch expects zeroed.  16-byte vectors
 * when every tensor is 16-byte aligned and n % 4 == 0, element by element otherwise: the same elements in the same lanes.  A row's bits depend on
 * its data and its table row only: not on B, the row's place, the load path or the launch.  No floating-point atomics, no global atomics. */
#define MF_GUIDE_ROW_ONE_WG 8192
#define MF_GUIDE_RESCALE 1
#define MF_GUIDE_THRESHOLD 2
typedef struct MfGuideStep {
  float g;                   /* guidance scale of this executed iteration */
  float phi;                 /* rescale weight in [0, 1] (read with MF_GUIDE_RESCALE) */
  float q;                   /* quantile in (0, 1] (read with MF_GUIDE_THRESHOLD) */
  float s_max;               /* cap of the limit, > 1; <= 0: none */
  float sqrt_recip_ac;       /* of the iteration's timestep, as in its MfSchedStep / MfSolverStep row */
  float sqrt_recipm1_ac;
  int32_t t;
  int32_t reserved;          /* 0 */
} MfGuideStep;
typedef struct MfGuideArgs {
  const float* x_t;          /* read with MF_GUIDE_THRESHOLD and objective 0; else may be NULL */
  const float* pred;         /* the conditional prediction (the only one without a pair) */
  const float* pred_uncond;  /* or NULL: no pair */
  float* pred_out;           /* may be `pred` */
  float* scale_out;          /* [B] or NULL */
  float* limit_out;          /* [B] or NULL */
  const MfGuideStep* table;  /* device, one row per executed iteration */
  const int32_t* step_dev;   /* device step counter, or NULL: `step` */
  void* workspace;           /* mf_guide_workspace_bytes(B, n) bytes, 8-byte aligned; may be NULL when that is 0 or stages == 0 */
  uint64_t workspace_bytes;
  int64_t n;                 /* elements per row, <= 2^31 - 1 */
  int32_t step;
  int32_t objective;         /* 0: 'x_T', 1: 'x_0' */
  int32_t B;                 /* <= 65535 */
  int32_t stages;            /* MF_GUIDE_RESCALE | MF_GUIDE_THRESHOLD */
  int32_t reserved;          /* 0 */
  int32_t reserved2;         /* 0 */
} MfGuideArgs;
size_t mf_guide_workspace_bytes(int B, int64_t n);
int mf_guide_f32(const MfGuideArgs* a, void* stream);

/* ------------------------------------------------------------------ dataset transform (additive to ABI 250): resize, crop, normalise on the device
 * Replaces the loader's transform, medical_diffusion/data/datasets/dataset_simple_2d.py:34-45: T.Resize (PIL, bilinear, antialiased when reducing) ->
 * T.CenterCrop -> T.ToTensor -> T.Normalize(0.5, 0.5), and augmentations_2d.py:14-19 (Normalize: (v - min) / (max - min)), for a RAGGED batch: N
 * images of any sizes back to back in one byte buffer, one pair of launches, no launch per image, no host sync, nothing allocated.
 *
 * The definition is PIL's ImagingResample restated (tests/ingest_cases.py; 0 mismatching pixels / bits against Pillow on the test list).
 * Coefficient table of one axis, in -> out samples, fp64 on the host (mf_resample_table): scale = in / out, fs = max(scale, 1), support = fs,
 * ksize = 2 ceil(support) + 1; for output xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support
 * + 0.5), in), n = xmax - xmin (int() truncates), w_x = max(0, 1 - |(x + xmin - center + 0.5) (1 / fs)|) for x < n -- the product with the rounded
 * reciprocal, as PIL forms it --, summed ascending to ww, each divided by ww when ww != 0; entries n .. ksize are 0.
 *   uint8 (1 or 3 interleaved channels): k_x = int(0.5 + w_x 2^22) (int(-0.5 + ...) for a negative one); a sample is
 *     clamp((2^21 + sum_x pix[xmin + x] k_x) >> 22, 0, 255) in 32-bit integers.
 *   float32 (1 channel): ss = 0; ss = ss + double(pix) w_x, x ascending, product and sum rounded separately; the sample is (float)ss.
 *   uint16 (1 channel): the same chain; the sample is clamp(floor(ss + 0.5), 0, 65535).
 * The horizontal pass comes first and its result is rounded to the element type; the vertical pass runs on that.  An axis whose size does not
 * change is skipped (its elements pass through: nothing is rounded twice).  The crop box (top, left, h, w) of the resized image is applied inside the
 * kernels: only the surviving columns, and only the source rows the surviving rows reach, are computed -- the same bits as resize-then-crop.
 * out_mode: MF_INGEST_RAW -> out [N][C][h][w] fp32, the resampled values; MF_INGEST_CENTERED (uint8 / uint16) -> fl(fl(fl(v / full) - 0.5) / 0.5),
 * full = 255 / 65535 (mf_image_ingress_u8's chain: an image that needs no pass gives that call's bits); MF_INGEST_BYTES (uint8) -> out [N][h][w][C]
 * uint8.  mf_minmax_apply_f32: x [N][n] in place, v = fl(fl(v - min) / fl(max - min)), then fl(fl(v - 0.5) / 0.5) with center != 0; minmax [N][2] is
 * mf_rows_minmax_f32's.
 *
 * The caller concatenates the tables of the distinct (in, out) pairs of the batch: weights_f64 / weights_i32 ([out][ksize] rows, the same entry
 * offsets in both; uint8 reads the integers, the others the doubles -- the unused one may be NULL) and bounds ((xmin, n) pairs), on the device, with
 * a HOST copy of the bounds and of the descriptors: every rule is checked on the host copies before any launch (the device copies must equal them).
 * mf_resample_plan (host only) checks the descriptors and fills their derived fields: the source rows an image's surviving rows reach, its offset
 * in the workspace, its first workgroup in the horizontal pass.  Refused before any launch, MF_EINVAL unless stated: a null pointer, C not 1 or 3,
 * C = 3 with uint16 / float32 (MF_EUNSUPPORTED), a side < 1, a crop outside the resized image, bytes or table rows outside what was given, a ksize
 * that is not the pair's, derived fields that are not the plan's, a workspace too small (MF_EWORKSPACE). */
#define MF_INGEST_U8 0
#define MF_INGEST_U16 1
#define MF_INGEST_F32 2
#define MF_INGEST_RAW 0
#define MF_INGEST_CENTERED 1
#define MF_INGEST_BYTES 2
typedef struct MfResampleImage {
  int64_t src_off;           /* byte offset of the image ([H][W][C] elements) in src; a multiple of the element size, else any alignment */
  int64_t ws_off;            /* (plan) ELEMENT offset of its intermediate [rows][w][C] in the workspace */
  int64_t tw_h, tw_v;        /* first entry of its horizontal / vertical table in weights_* (read when that axis changes size) */
  int64_t tb_h, tb_v;        /* first (xmin, n) pair of its horizontal / vertical table in bounds */
  int32_t H, W;              /* source size */
  int32_t Hr, Wr;            /* resized size */
  int32_t top, left;         /* crop box's corner in the resized image; its size is the batch's (h, w) */
  int32_t ksize_h, ksize_v;  /* row length of the two tables */
  int32_t row0, rows;        /* (plan) source rows [row0, row0 + rows) the surviving output rows reach */
  int32_t wg_h;              /* (plan) its first workgroup in the horizontal pass */
  int32_t reserved;          /* 0 */
} MfResampleImage;
typedef struct MfResamplePlan {
  int64_t workspace_bytes;   /* of the horizontal pass's intermediates */
  int32_t wg_h, wg_v;        /* workgroups of the two passes (wg_h = 0: no image changes width, one launch) */
  int32_t launches;          /* 1 or 2 */
  int32_t reserved;
} MfResamplePlan;
typedef struct MfResampleArgs {
  const void* src;                     /* device: the images back to back */
  const MfResampleImage* images;       /* device [N] */
  const MfResampleImage* images_host;  /* host [N], equal */
  const double* weights_f64;           /* device */
  const int32_t* weights_i32;          /* device */
  const int32_t* bounds;               /* device, (xmin, n) pairs */
  const int32_t* bounds_host;          /* host, equal */
  void* workspace;                     /* device, 16-byte aligned; may be NULL when no image changes width */
  void* out;                           /* device: fp32 [N][C][h][w], or uint8 [N][h][w][C] with MF_INGEST_BYTES */
  int64_t bounds_count;                /* pairs in bounds */
  int64_t weights_count;               /* entries in weights_* */
  int64_t src_bytes;
  uint64_t workspace_bytes;
  int32_t N, C, dtype, h, w, out_mode;
  int32_t reserved;                    /* 0 */
  int32_t reserved2;
} MfResampleArgs;
/* host only, no device needed: -> ksize (negative: MF_E*); fills weights [out][ksize] fp64, fixed [out][ksize] (the 22-bit integers) and bounds
 * [out][2], each of which may be NULL (all NULL: only ksize) */
int mf_resample_table(int in, int out, double* weights, int32_t* fixed, int32_t* bounds);
int mf_resample_plan(MfResampleImage* images, int N, int C, int dtype, int h, int w, const int32_t* bounds_host, int64_t bounds_count,
                     int64_t weights_count, int64_t src_bytes, MfResamplePlan* plan);
int mf_image_resample(const MfResampleArgs* a, void* stream);
int mf_minmax_apply_f32(float* x, const float* minmax, int N, int64_t n, int center, void* stream);

/* ------------------------------------------------------------------ LPIPS (additive to ABI 250): a pretrained-CNN trunk's plain layers and the distance
 * Replaces lpips.LPIPS(net='vgg').forward at medical_diffusion/loss/perceivers.py (the embedders' perception_loss: per slice, the mean over depth for
 * volumes) and torchmetrics' LearnedPerceptualImagePatchSimilarity (AlexNet trunk) at scripts/evaluate_latent_embedder.py ("LPIPS Score: 1 - mean").
 * Nothing pretrained is shipped or fetched: the caller loads the torchvision trunk state dict and the lpips package's linear-layer file.
 *
 * Definition (lpips v0.1).  Inputs x, y: fp32 NCHW, C in {1, 3}, in [-1, 1]; with normalize they are in [0, 1] and fl(2 x - 1) is taken first.
 *   Scaling layer: h_c = fl(fl(x_c' - shift_c) / scale_c), c = 0, 1, 2, c' = c for 3 channels and 0 for one; shift = (-.030, -.088, -.188),
 *     scale = (.458, .448, .450).
 *   Trunks: every convolution has a bias and is followed by ReLU.
 *     vgg: thirteen 3x3 pad 1 convolutions of widths 64, 64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512; a 2x2 stride-2 max-pool
 *       (floor mode) at each |; taps after relu1_2, 2_2, 3_3, 4_3, 5_3; keys features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}.
 *     alex: conv1 3 -> 64, 11x11, stride 4, pad 2; conv2 64 -> 192, 5x5, pad 2; conv3-5 3x3 pad 1, 192 -> 384 -> 256 -> 256; a 3x3 stride-2 max-pool
 *       (no padding, floor mode) after relu1 and after relu2; taps after each of the five ReLUs; keys features.{0,3,6,8,10}.{weight,bias}.
 *   Distance: per tap l, pixel p, feature vectors a, b: a^ = a / (sqrt(sum_c a_c^2) + 1e-10), b^ likewise; d_p = sum_c w_{l,c} (a^_c - b^_c)^2;
 *     term_l = mean_p d_p; lpips = sum_l term_l.  w_l: key lin{l}.model.1.weight, [1, C_l, 1, 1].
 *   Volumes [B, C, D, H, W]: the mean over d of the 2-D value of slice d.  Minimum side (host-checked): 16 for vgg, 31 for alex.
 *
 * mf_lpips_prepare_f32: x, y NCHW [B][C][H][W] -> out NHWC [2B][H][W][3], the scaled operand: rows [0, B) from x, rows [B, 2B) from y, so that the
 *   trunk runs once over both.
 * mf_conv2d_direct_f32: y = conv(x, w) + bias (bias may be NULL), ReLU with desc.relu, NHWC in and out, for the layers mf_conv2d_f32's implicit-GEMM
 *   path does not take (Cin = 3, 11x11 stride 4, 5x5): any Cin and Cout, KH, KW <= 11, stride 1 .. 4, any pad >= 0.  DEFINED as mf_conv2d_gemm_f32
 *   ("Inception" below; one kernel runs both) with pad_h = pad_w = pad, chain = 0, tile = 0 and a dense output: one fp32 fma chain per output value
 *   from +0 in (kh, kw, cin) order, padding taps as zeros, then + bias.  A padding tap is a term 0 w: it leaves no trace on finite weights, and makes a
 *   NaN of a non-finite weight under it (the one-thread-per-output kernel this entry ran before skipped those taps).  Its launches are timed as
 *   MF_FAM_CONV_IGEMM.  Weights [KH][KW][Cin][Cout] (OIHW permuted once at load time).
 * mf_relu_f32: in place, x < 0 -> 0 (a NaN stays).  mf_maxpool_nhwc_f32: (k, stride) = (2, 2) or (3, 2), floor mode, no padding; a NaN wins; the max
 *   of mf_pool2d_nhwc_f32's kernel without padding, which also has the window 2.
 * mf_lpips_layer_f32: fx, fy [B][P][C] (the two halves of a tap's feature map), w [C] -> per-workgroup partial sums of d_p in `workspace`
 *   (mf_lpips_workspace_bytes(B, P)); evaluated in fp64 on the fp32 features, channel and pixel sums in a fixed order, no atomics.  A pair's bits depend
 *   on its own feature values only: not on B, its place in the batch, or the load path (16-byte loads when both operands are 16-byte aligned and
 *   C % 4 == 0, else element-wise).  An all-zero vector gives a^ = 0; identical maps give exactly 0.
 * mf_lpips_finish_f32: terms[b][layer] (fp64, [B][layers]) = the pair's partials added in ascending order / P; with total != NULL also
 *   total[b] = (float)(terms[b][0] + ... + terms[b][layers - 1]) in ascending order (pass it with the last layer).
 * Refused before any launch, MF_EINVAL unless stated: a null pointer, a side below the minimum, C not 1 or 3, a (k, stride) pair other than the two, sizes
 * outside the ranges above, a workspace too small (MF_EWORKSPACE). */
#define MF_LPIPS_VGG 0
#define MF_LPIPS_ALEX 1
typedef struct MfDirectConvDesc {
  int32_t N, Hin, Win;
  int32_t Cin, Cout;
  int32_t KH, KW;          /* 1 .. 11 */
  int32_t stride;          /* 1 .. 4 */
  int32_t pad;             /* >= 0 */
  int32_t relu;            /* != 0: y = max(y, 0) after the bias */
  int32_t reserved;        /* 0 */
  int32_t reserved2;
} MfDirectConvDesc;
int mf_lpips_min_side(int net);
int mf_lpips_prepare_f32(const float* x, const float* y, float* out, int B, int C, int H, int W, int normalize, int net, void* stream);
int mf_conv2d_direct_out_dims(const MfDirectConvDesc* d, int32_t* out2);
int mf_conv2d_direct_f32(const float* x, const float* w_hwio, const float* bias, float* y, const MfDirectConvDesc* d, void* stream);
int mf_relu_f32(float* x, int64_t n, void* stream);
int mf_maxpool_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int k, int stride, void* stream);
int mf_lpips_layer_parts(int64_t P);
size_t mf_lpips_workspace_bytes(int B, int64_t P);
int mf_lpips_layer_f32(const float* fx, const float* fy, const float* w, void* workspace, size_t workspace_bytes, int B, int64_t P, int C, void* stream);
int mf_lpips_finish_f32(const void* workspace, double* terms, float* total, int B, int64_t P, int layer, int layers, void* stream);

/* ------------------------------------------------------------------ Inception (additive to ABI 250): the FID variant of Inception-v3 and its layers
 * Replaces the feature extractor behind torchmetrics' FrechetInceptionDistance and torch-fidelity's precision / recall at scripts/evaluate_images.py
 * ("FID Score", "Precision", "Recall"): torch-fidelity's `inception-v3-compat`, read from pt_inception-2015-12-05-6726825d.pth.  Nothing pretrained is
 * shipped or fetched: the caller loads the file a reference run has in its torch hub cache.
 *
 * Definition.  Input: uint8 [B][C][H][W], C in {1, 3}; one channel is replicated to three.
 *   Resize: TF1-style bilinear to S x S (299 is the metric; any S >= 75 runs).  Per axis, s = fl32(in / S): g = fl32(i s), lo = int(g), hi = min(lo + 1,
 *     in - 1), d = fl32(g - lo) -- no half-pixel offset.  top = fl32(a00 + fl32(fl32(a01 - a00) dx)), bottom likewise, v = fl32(top + fl32(fl32(bottom -
 *     top) dy)), out = fl32(fl32(v - 128) / 128), written NHWC.  The resize always runs; with in = S it is the identity on the values.
 *   BasicConv: a convolution without bias, BatchNorm (eps = 0.001, eval mode), ReLU.  The BatchNorm is folded once on the host in fp64:
 *     s = gamma / sqrt(var + eps), w' = fl32(w s), b' = fl32(beta - mean s); the network is DEFINED as the convolution with w', b' and ReLU.
 *   Trunk (k square unless (kh, kw); padding (k - 1) / 2 per axis only where marked p; output side at 299 in brackets):
 *     Conv2d_1a_3x3 3 -> 32 k3 s2 [149]; Conv2d_2a_3x3 32 -> 32 k3 [147]; Conv2d_2b_3x3 32 -> 64 k3 p [147]; max-pool 3 s2 [73] (tap "64");
 *     Conv2d_3b_1x1 64 -> 80 [73]; Conv2d_4a_3x3 80 -> 192 k3 [71]; max-pool 3 s2 [35] (tap "192");
 *     Mixed_5b / 5c / 5d = A(in 192 / 256 / 288, pool 32 / 64 / 64) [35]; Mixed_6a = B(288) [17]; Mixed_6b .. 6e = C(768, c7 128 / 160 / 160 / 192) [17]
 *     (tap "768"); Mixed_7a = D(768) [8]; Mixed_7b = E(1280, avg) [8]; Mixed_7c = E(2048, max) [8]; the mean over the pixels [B][2048] (tap "2048");
 *     fc 2048 -> F rows (1008 in the FID file): logits_unbiased without the bias, logits with it.
 *   Blocks, concatenated in the order written:
 *     A: branch1x1 in -> 64 | branch5x5_1 in -> 48, _2 48 -> 64 k5 p | branch3x3dbl_1 in -> 64, _2 64 -> 96 k3 p, _3 96 -> 96 k3 p | avg-pool(3, s1,
 *        pad 1, divisor = the number of valid taps), branch_pool in -> pool k1.
 *     B: branch3x3 in -> 384 k3 s2 | branch3x3dbl_1 in -> 64, _2 64 -> 96 k3 p, _3 96 -> 96 k3 s2 | max-pool(3, s2) of the input.
 *     C: branch1x1 in -> 192 | branch7x7_1 in -> c7, _2 c7 -> c7 (1,7) p, _3 c7 -> 192 (7,1) p | branch7x7dbl_1 in -> c7, _2 (7,1) p, _3 (1,7) p,
 *        _4 (7,1) p (all c7 -> c7), _5 c7 -> 192 (1,7) p | the avg-pool of A, branch_pool in -> 192.
 *     D: branch3x3_1 in -> 192, _2 192 -> 320 k3 s2 | branch7x7x3_1 in -> 192, _2 (1,7) p, _3 (7,1) p (192 -> 192), _4 192 -> 192 k3 s2 | max-pool(3, s2).
 *     E: branch1x1 in -> 320 | branch3x3_1 in -> 384, then [_2a 384 -> 384 (1,3) p, _2b 384 -> 384 (3,1) p] both of _1 | branch3x3dbl_1 in -> 448,
 *        _2 448 -> 384 k3 p, then [_3a (1,3) p, _3b (3,1) p] both of _2 | the avg-pool of A (Mixed_7b) or max-pool(3, s1, pad 1) (Mixed_7c), branch_pool
 *        in -> 192.
 *   Keys: {layer}.conv.weight, {layer}.bn.{weight, bias, running_mean, running_var}, fc.weight, fc.bias; AuxLogits.* and *.num_batches_tracked ignored.
 *   Pools: max = the largest valid tap, a NaN wins; avg = the fp32 sum of the valid taps in ascending (kh, kw) order, divided once by their number.
 *   Mean over the pixels: the fp64 sum in ascending order, divided by the number, rounded once to fp32.
 *
 * mf_conv2d_gemm_f32: y = conv(x, w) + bias (bias may be NULL), ReLU with desc.relu; NHWC in, weights [KH][KW][Cin][Cout], KH, KW 1 .. 11 independently,
 *   stride 1 .. 4, pad_h, pad_w >= 0, any Cin, any Cout >= 1.  The value of output channel co of pixel m lands at y[m ldy + y_offset + co]: a branch
 *   writes straight into its block's concatenated tensor (ldy = 0: dense, ldy = Cout).  An implicit GEMM on v_mfma_f32_32x32x2_f32 with exact fp32
 *   operands staged through LDS: M = the output pixels of the whole batch, N = Cout, K = (kh, kw, cin) flattened, k = (kh KW + kw) Cin + cin, never split
 *   across workgroups; padding taps and every tail are staged as zeros.
 *     chain = 0: one fmaf chain per output value over all of K ascending from +0, then + bias.  This is what mf_conv2d_direct_f32 ("LPIPS" above)
 *       runs; on finite data a padding tap, staged as a zero, leaves the chain's bits as if it were skipped.
 *     chain = L > 0: with L' = 32 ceil(L / 32), the K axis is cut at k = L', 2 L', ... (< K): piece j = [j L', min((j + 1) L', K)) is its own fmaf chain
 *       from +0, t_0 = piece 0, t_j = fl32(t_{j-1} + piece j) in ascending order in registers, then + bias.  The cuts depend on (KH, KW, Cin, L) only.
 *     tile = 0: the planner picks (from M and Cout); 1: 128 x 128, 2: 128 x 64, 3: 64 x 64 (pixels x channels per workgroup).  No bit of the output
 *       depends on the tile, the batch, the pixel's place in it, ldy / y_offset, or the load path (16-byte loads when Cin % 4 == 0, Cout % 4 == 0 and both
 *       operands are 16-byte aligned, else element by element).
 *   mf_conv2d_gemm_out_dims -> (Hout, Wout); mf_conv2d_gemm_plan -> (tile, workgroups).  Both host-only.
 * mf_pool2d_nhwc_f32: window 3, stride 1 or 2, pad 0 or 1, floor mode, mode MF_POOL_MAX or MF_POOL_AVG_VALID as defined above; ldy / y_offset as above.
 * mf_inception_prepare_u8: x uint8 NCHW [B][C][H][W] -> out fp32 NHWC [B][S][S][3]: the resize, the value map and the replication of the definition.
 * mf_mean_pixels_f32: x [B][P][C] -> out [B][C], the mean over the pixels of the definition; a row's bits do not depend on B or its place.
 * Refused before any launch, MF_EINVAL unless stated: a null pointer, C not 1 or 3, S < 75 or > 4096, a side above 16384, sizes outside the ranges above,
 * a slice outside ldy, a non-zero reserved field; a problem too large for the index arithmetic (MF_EUNSUPPORTED). */
#define MF_POOL_MAX 0
#define MF_POOL_AVG_VALID 1
#define MF_INCEPTION_MIN_SIZE 75
typedef struct MfGemmConvDesc {
  int32_t N, Hin, Win;
  int32_t Cin, Cout;
  int32_t KH, KW;          /* 1 .. 11, independently */
  int32_t stride;          /* 1 .. 4 */
  int32_t pad_h, pad_w;    /* >= 0 */
  int32_t relu;            /* != 0: y = max(y, 0) after the bias */
  int32_t ldy, y_offset;   /* channels of an output pixel (0: Cout) and the first one written */
  int32_t chain;           /* 0: one chain over K; L > 0: pieces of 32 ceil(L / 32) */
  int32_t tile;            /* 0: planned; 1 .. 3: forced */
  int32_t reserved;        /* 0 */
} MfGemmConvDesc;
int mf_conv2d_gemm_out_dims(const MfGemmConvDesc* d, int32_t* out2);
int mf_conv2d_gemm_plan(const MfGemmConvDesc* d, int32_t* out2);
int mf_conv2d_gemm_f32(const float* x, const float* w_hwio, const float* bias, float* y, const MfGemmConvDesc* d, void* stream);
int mf_pool2d_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int stride, int pad, int mode, int ldy, int y_offset, void* stream);
int mf_inception_prepare_u8(const uint8_t* x, float* out, int B, int C, int H, int W, int S, void* stream);
int mf_mean_pixels_f32(const float* x, float* out, int B, int64_t P, int C, void* stream);

/* ------------------------------------------------------------------ built-in launch timing (bench / roofline)
 * When enabled every launch is bracketed by hipEvents on its own stream and attributed to a kernel family.
 * NOT capture-safe; off by default. */
enum { MF_FAM_CONV_IGEMM = 0, MF_FAM_CONV_DIRECT, MF_FAM_SPLITK_REDUCE, MF_FAM_GN_STATS, MF_FAM_GN_APPLY, MF_FAM_LINEAR,
       MF_FAM_SCHED, MF_FAM_NOISE, MF_FAM_ATTENTION, MF_FAM_MISC, MF_FAM_CONV_GN_FUSED, MF_FAM_WINO_XFORM, MF_FAM_COUNT };
int mf_prof_enable(int on);
int mf_prof_reset(void);
/* synchronises outstanding events; returns summed ms, launch count, algorithmic flops and bytes of a family */
int mf_prof_query(int family, double* ms, int64_t* launches, double* flops, double* bytes);
/* the same plus the flops the hardware EXECUTES for those launches (matrix terms per product x the MACs actually done) */
int mf_prof_query2(int family, double* ms, int64_t* launches, double* flops, double* bytes, double* exec_flops);
const char* mf_prof_family_name(int family);
/* The same records grouped by KERNEL INSTANTIATION (ABI 230): `tag` identifies the instantiation -- for the fp16-pair convolution family its tile id
 * (a grouped launch: 1000 + 100 host tile + guest tile; the single-term mode: + 100000) --, `variant` 1 marks the component GEMMs of the Winograd
 * form (same kernel, same name in a profiler).  mf_prof_rows fills up to max_rows rows and returns how many; mf_prof_tag_name writes the kernel's
 * name as rocprofv3 --kernel-trace prints it, so that a row can be checked against the committed kernel_stats.csv. */
typedef struct MfProfRow { int32_t tag, variant; int64_t launches; double ms, flops, bytes, exec_flops; } MfProfRow;
int mf_prof_rows(int family, MfProfRow* rows, int max_rows);
int mf_prof_tag_name(int family, int tag, char* buf, int n);
/* Measurement aid: what the fp16 matrix pipe SUSTAINS on this device for given operand data.  Launches `workgroups` x 512 threads running
 * nothing but v_mfma_f32_32x32x16_f16 from registers (4 independent chains per wave, `iters` instructions per chain; operands = the first
 * workgroups * 512 * 8 sixteen-byte groups of fp16 at `operands`, loaded once; `out`: workgroups * 512 floats) and reports the flops of the
 * launch; the caller times it.  On MI355X random operands sustain ~60-65 % of the nominal 2516.8 TF, zeros ~97 % (profiles/): the matrix
 * pipe is power-limited by the data it multiplies, and bench.py reports the conv kernel against both numbers. */
int mf_mfma_rate_probe_f16(const void* operands, float* out, int workgroups, int iters, double* flops, void* stream);

/* ------------------------------------------------------------------ command lists (ABI 210): the loop body of denoise() replayed from C
 * Replaces the Python loop of diffusion_pipeline.py:290-305 for every iteration after the second: the host side of one iteration is ~160
 * launches through this ABI (2.0 ms of Python -> ctypes work, profiles/r02_host_enqueue_time.txt), all of whose per-iteration values -- t,
 * the scheduler record, the Philox draw indices, the rows of the hoisted embedding table -- come from a DEVICE step counter that the
 * iteration advances itself.  mf_cmdlist_begin() makes the calling thread record every launch it issues through this library (the
 * launches still execute): kernel, grid, block, LDS size and a copy of the kernarg bytes, in issue order.  mf_cmdlist_end() returns the
 * list; mf_cmdlist_replay(list, times, stream) re-issues it `times` times on `stream` -- plain stream-ordered launches (no graph node
 * latency), ~1 us of host time each.  The caller guarantees what a graph capture would: every pointer recorded stays valid and means the
 * same buffer during the replays (pipeline.py records inside a private torch memory pool), and nothing but launches of this library makes
 * up the iteration.  Not recorded: hipFuncSetAttribute (done by the eager warm-up iteration), launch timing (begin refuses while
 * mf_prof_enable is on).  Lists are immutable after end(), replay is thread-safe, free() releases. */
int mf_cmdlist_begin(void);
int mf_cmdlist_end(void** list);
int mf_cmdlist_count(const void* list);
int mf_cmdlist_replay(const void* list, int times, void* stream);
int mf_cmdlist_free(void* list);

#ifdef __cplusplus
}
#endif
#endif /* MEDFUSION_HIP_H */
