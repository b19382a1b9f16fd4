/* somi_hip.h - C ABI of libsomi_hip.so, the MI355X (gfx950) hot path of YOLO-SOMI.
 *
 * Drop-in boundary.  The reference's only native boundary is the pybind
 * module `DCNv3` (models/ops_dcnv3/src/vision.cpp:14-17, src/dcnv3.h:20-59); everything else on
 * the path is reached through Python call signatures (models/yolo.py, utils/loss.py,
 * utils/general.py).  This header declares one plain-C entry point per device operation on
 * that path; the Python host layer in yolo-somi_amd/somi_amd/ mirrors the reference's
 * Python signatures on top of it (see INTEGRATION.md for the reference-side binding).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the name ends in _host; the library never
 *    allocates, frees, copies or synchronises: outputs and workspaces are caller-owned;
 *  - tensors are fp32, activations are NHWC with an explicit channel stride (`*_cs`, in floats)
 *    and channel offset (`*_coff`) so that channel slices / concatenations need no copy;
 *  - THE SLICE RULE, checked the same way at every entry point that takes a slice (pointer, `*_cs`,
 *    `*_coff`): the pointer is non-NULL and 16-byte aligned; `*_cs` > 0 and `*_cs % 4 == 0`;
 *    `*_coff` >= 0 and `*_coff % 4 == 0`; and the channels the entry point touches,
 *    [coff, coff + width), lie inside the stride: width > 0, coff + width <= cs.  width is C unless
 *    the entry point's comment names more (4 * C for SPPF, heads * 128 for attention's qkv, ...).
 *    An optional slice (residual, accumulate, ...) is checked when its pointer is given.  A slice
 *    that breaks the rule is SOMI_EINVAL, and somi_last_error() names the parameter and the reason:
 *    "add: out = [12, 20) of 16 channels: runs past the channel stride";
 *  - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the call returns;
 *  - return value: 0 on success, a negative SOMI_E* code on a rejected argument (nothing was
 *    launched), or a positive hipError_t from the launch.  somi_last_error() gives the text.
 *    Argument errors mirror the reference's AT_ASSERTM checks (dcnv3_cuda.cu:29-53).
 */
#ifndef SOMI_HIP_H
#define SOMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOMI_ABI_VERSION 15

#define SOMI_EINVAL   (-1) /* bad shape / stride / alignment */
#define SOMI_ENOTIMPL (-2) /* configuration outside the SOMI path */
#define SOMI_EWORKSPACE (-3) /* workspace too small */

typedef void *somi_stream_t;

int somi_abi_version(void);
const char *somi_last_error(void);
/* sizeof of a descriptor struct as the library was compiled (0: somi_conv_desc, 1: somi_loss_desc, 2: somi_loss_box_rule): lets a binding check its mirror */
size_t somi_sizeof_desc(int which);

/* ------------------------------------------------------------------------------------------
 * Activations used in fused epilogues.
 */
enum somi_act { SOMI_ACT_NONE = 0, SOMI_ACT_SILU = 1, SOMI_ACT_GELU = 2, SOMI_ACT_RELU = 3, SOMI_ACT_SIGMOID = 4,
                SOMI_ACT_LEAKY = 5 /* LeakyReLU(0.1), add_conv of models/common.py:5322-5343: the dense conv epilogue, somi_chan_affine_act_* and the
                                      somi_bn_act_backward_* family take it; somi_linear_f32 keeps reading 5 as its softmax */,
                SOMI_ACT_HSWISH = 6 /* h_swish, x * relu6(x + 3) / 6 (models/common.py:1381-1398), the activation between bn1 and conv_h / conv_w of
                                       coordinate attention: taken wherever SOMI_ACT_LEAKY is */ };

/* A channel slice as one argument (the slice rule above: p 16-byte aligned, cs and coff multiples of 4), for the entry points that take their
 * slices by value or in a descriptor (somi_maxpool3s2_*, somi_asff_desc, somi_coordatt_desc, somi_ema_desc, somi_acmix_desc, somi_simam_desc, the asf.hip descriptors).  An input slice is only read. */
typedef struct somi_slice {
    float *p;
    int32_t cs, coff;
} somi_slice;

/* ------------------------------------------------------------------------------------------
 * Dense convolution as NHWC implicit GEMM on MFMA with a fused epilogue.
 * Replaces: nn.Conv2d + BatchNorm2d(eval, folded) + SiLU inside `Conv.forward`
 * (models/common.py:64-70, utils/torch_utils.py:202-222), the grouped conv of ODConv2d_3rd
 * (models/common.py:4602-4605, per-sample weights), SEAM's 1x1 (+GELU+BN, models/common.py:8463-8465),
 * Decouple's b3/c3 1x1 (+bias, models/yolo.py:1057,1063) and nn.Linear projections of DCNv3
 * (models/ops_dcnv3/modules/dcnv3.py:324,330-331,377) which are 1x1 convs in NHWC.
 *
 *   y[b,ho,wo,n] = post( act( sum_{r,q,c} x'[b, ho*s-p+r*d, wo*s-p+q*d, c] * w[wset][n][(r*kw+q)*Cin+c] + bias[wset][n] ) )
 *   post(v) = v*post_scale[n] + post_shift[n]  (if given), then + residual[b,ho,wo,n] (if given)
 *   x' = x * a_chan_scale[b][c] * a_pix_scale[b][h][w]   (each factor optional; CBAM fused on the operand load)
 *   wset = b if per_sample_w else 0.
 */
typedef struct somi_conv_desc {
    const float *x;
    const float *w;
    const float *bias;        /* [n_wsets][Cout] or NULL */
    const float *post_scale;  /* [Cout] or NULL */
    const float *post_shift;  /* [Cout] or NULL (required iff post_scale) */
    const float *residual;    /* NHWC (B,Ho,Wo,*) or NULL */
    const float *a_chan_scale;/* [B][Cin] or NULL */
    const float *a_pix_scale; /* [B][H][W] or NULL */
    float *y;
    int32_t B, H, W, Cin, x_cs, x_coff;
    int32_t Ho, Wo, Cout, y_cs, y_coff;
    int32_t kh, kw, stride, pad, dil;
    int32_t res_cs, res_coff;
    int32_t act;              /* enum somi_act */
    int32_t per_sample_w;
    int32_t res2_cs, res2_coff; /* channel stride / offset of residual2 */
    void *workspace;          /* optional scratch (16 B aligned, somi_conv2d_workspace_bytes()); with it, layers whose tile
                               * count leaves workgroup slots idle in the last round are scheduled stream-K: the K range of
                               * some tiles is cut between workgroups and the pieces are added in a fixed order (results
                               * then differ from the unsplit sum by fp32 rounding only).  NULL: one workgroup per tile. */
    uint64_t workspace_bytes;
    const float *residual2;   /* optional second tensor added after the activation (NHWC (B,Ho,Wo,*)), or NULL */
    /* Optional per-channel statistics of the stored output for a following BatchNorm in training mode (the conv epilogue
     * has every value in registers: this saves the separate read of y).  stat_sum / stat_sumsq: [somi_conv2d_stat_rows(d)][Cout]
     * partial sums of (y - pivot) and (y - pivot)^2 - one row per (row tile, wave row), each written exactly once; stat_pivot:
     * [Cout] or NULL (= 0).  Reduce them with somi_bn_stats_partials_f32.  Needs Cout % 4 == 0 and per_sample_w == 0. */
    float *stat_sum;
    float *stat_sumsq;
    const float *stat_pivot;
    /* Opt-in reduced precision of the products (train.py:263 `amp.autocast`; the default 0 is the exact fp32 path every parity claim is
     * made on): 1 = operands rounded to bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulate - autocast's arithmetic), 2 = "bf16x3": each
     * operand split into two bf16 values and hi*hi + hi*lo + lo*hi accumulated in fp32 (~1e-5 relative error).  Tensors stay fp32 in
     * HBM either way.  Honoured by the launches that have a bf16 form: of somi_conv2d_nhwc_f32 / _dgrad_, the plain channel-aligned ones
     * (operand channels % 32 == 0, at most 32 taps, no operand modulation; shared or per-sample weights) that plan an 8-wave tile, 128 x 128
     * or 128 x 64 (somi_conv2d_kernel_name tells) - not the 4-wave tiles, 64 x 128 (more than 64 output channels on fewer than 32768 rows and 512
     * tiles without the stream-K schedule: no workspace, per-sample weights, a data gradient at stride > 1) and 128 x 32 (at most 32 output
     * channels); of somi_conv2d_wgrad_nhwc_f32, the shared-weight ones with kh * kw * Cin > 64 (a 128-column tile), at any Cin % 4 == 0.
     * Every other launch computes in exact fp32, bit for bit what prec = 0 gives - among them the forward and the data gradient of a
     * patch-embedding conv of more than 32 taps (kh == kw == stride >= 6, pad 0, dil 1: see somi_conv2d_nhwc_f32), whose instantiation has
     * no reduced-precision form; its weight gradient honours `prec` like any other.  tests/test_conv_amp_gpu.py pins both halves. */
    int32_t prec;
} somi_conv_desc;

/* Any kh, kw, stride, pad, dil.  Which code a launch runs: Cin % 32 == 0 with kh*kw <= 32 taps takes the wave-uniform tap walk with a
 * per-row tap mask (LDS-DMA staging, stream-K with a workspace, `prec`) - that includes the patch-embedding geometry kh == kw == stride
 * == p, pad 0 (MultiSEAM's stems, models/common.py:8510) at p = 3 and 5.  The same geometry at p*p > 32 (p = 7: 49 taps) with Cin % 32
 * == 0 takes instantiations of its own, here and in somi_conv2d_dgrad_nhwc_f32: no tap of an in-range output pixel leaves the image, so
 * there is no tap mask; the data gradient runs p*p parity classes of ONE tap each (dx pixel (h, w) has the tap (h % p, w % p) and the
 * source pixel (h / p, w / p)), and the dx pixels with h >= Ho*p or w >= Wo*p, which no tap reaches, are written as exact zeros (plus
 * `accumulate` / residual2, if given).  Exact fp32 whatever `prec` asks for.  Everything else - Cin % 32 != 0, more than 32 taps at
 * another geometry, modulated operands beyond 32 taps - takes the generic register-staged path: correct, not fast. */
int somi_conv2d_nhwc_f32(const somi_conv_desc *d, somi_stream_t stream);
/* Scratch size that enables the stream-K schedule for every shape (64 MiB). */
size_t somi_conv2d_workspace_bytes(void);
/* Rows of the stat_sum / stat_sumsq partial arrays somi_conv2d_nhwc_f32 would write for this descriptor. */
int somi_conv2d_stat_rows(const somi_conv_desc *d);

/* Data gradient of the convolution whose FORWARD geometry `fwd` describes (x (B,H,W,Cin) -> y (B,Ho,Wo,Cout); the pointer
 * fields of `fwd` are ignored):  dx[b,h,w,ci] = sum_{r,q,co} dy[b,(h+p-r)/s,(w+p-q)/s,co] * W[co][ci][r][q]
 * over the taps for which the divisions are exact and in range (autograd of F.conv2d, train.py:270 `backward()`); a pixel no tap
 * reaches (kh == stride, h >= Ho*stride) is written as 0 (+ accumulate).
 * With fwd->dil = d > 1 (stride 1 only):  dx[b,h,w,ci] = sum_{r,q,co} dy[b, h+p-r*d, w+p-q*d, co] * W[co][ci][r][q];
 * fwd->Ho / Wo must be the dilated output size (H + 2p - (d*(kh-1)+1))/s + 1.  d > 1 together with s > 1 returns
 * SOMI_ENOTIMPL: the taps that reach a pixel would then depend on (h+p-r*d) % s, which the parity classes do not model.
 * Runs the same MFMA implicit-GEMM kernel with rows = forward-input pixels.  `w_dgrad` is packed [Cin][kh*kw*Cout],
 * k = (r*kw+q)*Cout + co.  `accumulate` (optional, may alias dx) is added to the result (skip connections).
 * fwd->workspace / workspace_bytes are honoured as in somi_conv2d_nhwc_f32; fwd->residual2 (with res2_cs / res2_coff), if set,
 * is a second tensor of dx's shape added to the result (a shortcut branch's gradient).
 * per_sample_w in `fwd` selects per-image weight sets [B][Cin][kh*kw*Cout]. */
int somi_conv2d_dgrad_nhwc_f32(const somi_conv_desc *fwd, const float *dy, int dy_cs, int dy_coff, const float *w_dgrad,
                               float *dx, int dx_cs, int dx_coff, const float *accumulate, int acc_cs, int acc_coff,
                               somi_stream_t stream);

/* Weight gradient of the convolution whose FORWARD geometry `fwd` describes:
 *   dw[co][(r*kw+q)*Cin + ci] = sum_{b,ho,wo} dy[b,ho,wo,co] * x[b, ho*s-p+r*d, wo*s-p+q*d, ci]  (same packing as the forward weights)
 * with d = fwd->dil >= 1 at any stride; fwd->Ho / Wo (and the workspace size) follow the dilated extent d*(kh-1)+1.  Any tap count: a
 * thread's column quad has one fixed tap, so the patch-embedding geometry (kh == kw == stride, 9 / 25 / 49 taps) runs the code every conv runs.
 * MFMA GEMM with the reduction over pixels, split over workgroups; the split partials live in `workspace`
 * (somi_conv2d_wgrad_workspace_bytes) and are summed in a fixed order, on top of `accumulate` if given (may alias dw).
 * per_sample_w: one gradient per image, dw is [B][Cout][K]. Cin, Cout multiples of 4. */
size_t somi_conv2d_wgrad_workspace_bytes(const somi_conv_desc *fwd);
int somi_conv2d_wgrad_nhwc_f32(const somi_conv_desc *fwd, const float *x, int x_cs, int x_coff, const float *dy, int dy_cs,
                               int dy_coff, float *dw, const float *accumulate, void *workspace, size_t workspace_bytes,
                               somi_stream_t stream);

/* Name of the kernel instantiation somi_conv2d_nhwc_f32 would launch for this descriptor (for profiling: matches the
 * kernel name rocprofv3 reports), or NULL for an invalid descriptor. */
const char *somi_conv2d_kernel_name(const somi_conv_desc *d);
/* The same for the kernel somi_conv2d_wgrad_nhwc_f32 would launch for this forward geometry (the fp32 instantiation's name), or NULL. */
const char *somi_conv2d_wgrad_kernel_name(const somi_conv_desc *fwd);

/* ------------------------------------------------------------------------------------------
 * DCNv3 operator.  Replaces `dcnv3_forward` / `dcnv3_backward` of the reference extension
 * (models/ops_dcnv3/src/dcnv3.h:20-59, src/cuda/dcnv3_cuda.cu:21-174, kernels
 * src/cuda/dcnv3_im2col_cuda.cuh:216-275 fwd and :278-839 bwd).
 * input (N,H,W,G*Gc); offset (N,Ho,Wo,G*K*2) x,y interleaved, points ordered kernel_w-outer /
 * kernel_h-inner; mask (N,Ho,Wo,G*K); output (N,Ho,Wo,G*Gc).  All contiguous.
 * Backward: grad_input must be ZEROED by the caller (the reference allocates it with at::zeros,
 * dcnv3_cuda.cu:126-133); grad_offset / grad_mask are fully overwritten.
 * workspace (optional, may be NULL / 0): somi_dcnv3_backward_workspace_bytes(...) bytes, 16-byte aligned, enable the windowed
 * form of the fp32 backward (grad_input summed per tile in LDS in exact arithmetic, combined in a fixed order: no float atomics,
 * run-to-run bit-identical, while every sampling tap stays within SOMI_DCN_SLACK = 2 pixels of the kernel footprint; taps
 * beyond go through fp32 atomics and are counted in the uint32 at workspace + size - 256).  Without it - or for group widths other than 8/16/32/64 (then the size is 0) - one kernel
 * scatters with fp32 atomics like the reference.  The _f16 / _f64 entries take the two arguments for a uniform signature and
 * ignore them.
 * im2col_step is validated like the reference (batch % min(batch, im2col_step) == 0) and otherwise
 * unused: the whole batch is one launch.
 */
int somi_dcnv3_forward_f32(const float *input, const float *offset, const float *mask, float *output,
                           int N, int H, int W, int G, int Gc, int kernel_h, int kernel_w, int stride_h,
                           int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                           float offset_scale, int im2col_step, somi_stream_t stream);

int somi_dcnv3_backward_f32(const float *input, const float *offset, const float *mask, const float *grad_output,
                            float *grad_input, float *grad_offset, float *grad_mask,
                            int N, int H, int W, int G, int Gc, int kernel_h, int kernel_w, int stride_h,
                            int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                            float offset_scale, int im2col_step, void *workspace, size_t workspace_bytes, somi_stream_t stream);
size_t somi_dcnv3_backward_workspace_bytes(int N, int H, int W, int G, int Gc, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                           int pad_h, int pad_w, int dilation_h, int dilation_w, float offset_scale);

/* The same operator over offset / mask tensors that are column ranges of wider rows: the module (modules/dcnv3.py:330-334) computes both from
 * the same activations, so ONE 1x1 GEMM with the two Linear weights stacked produces [pixel][2*G*K offsets | G*K mask logits] and the operator
 * reads (and, backward, writes grad_offset / grad_mask) in place there.  offset_stride / mask_stride = floats between consecutive pixels
 * (0 = packed, i.e. the entries above); offset_stride must be even and offset 8-byte aligned.  grad_offset / grad_mask use the same
 * strides.  Arithmetic identical to the packed entries. */
int somi_dcnv3_forward_strided_f32(const float *input, const float *offset, const float *mask, long offset_stride, long mask_stride,
                                   float *output, int N, int H, int W, int G, int Gc, int kernel_h, int kernel_w, int stride_h,
                                   int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, float offset_scale,
                                   int im2col_step, somi_stream_t stream);
int somi_dcnv3_backward_strided_f32(const float *input, const float *offset, const float *mask, long offset_stride, long mask_stride,
                                    const float *grad_output, float *grad_input, float *grad_offset, float *grad_mask, int N, int H,
                                    int W, int G, int Gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                    int pad_w, int dilation_h, int dilation_w, float offset_scale, int im2col_step,
                                    void *workspace, size_t workspace_bytes, somi_stream_t stream);

/* The other two dtypes the reference extension dispatches (AT_DISPATCH_FLOATING_TYPES_AND_HALF, dcnv3_cuda.cu:69,136), same argument
 * meaning as the _f32 pair.  _f16: tensors are IEEE half (the AMP path of train.py:263), arithmetic fp32 (the reference's opmath_t),
 * and the three gradient outputs are FP32 buffers exactly like the reference's (dcnv3_cuda.cu:126-133: the caller casts them back,
 * :168-170).  _f64: everything double (the exact-parity mode of models/ops_dcnv3/test.py:55).  grad_input must be zeroed by the
 * caller (at::zeros in the reference); grad_offset / grad_mask are fully overwritten. */
int somi_dcnv3_forward_f16(const void *input, const void *offset, const void *mask, void *output, int N, int H, int W, int G, int Gc,
                           int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                           float offset_scale, int im2col_step, somi_stream_t stream);
int somi_dcnv3_backward_f16(const void *input, const void *offset, const void *mask, const void *grad_output, float *grad_input,
                            float *grad_offset, float *grad_mask, int N, int H, int W, int G, int Gc, int kernel_h, int kernel_w,
                            int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, float offset_scale,
                            int im2col_step, void *workspace, size_t workspace_bytes, somi_stream_t stream);
int somi_dcnv3_forward_f64(const double *input, const double *offset, const double *mask, double *output, int N, int H, int W, int G,
                           int Gc, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h,
                           int dilation_w, float offset_scale, int im2col_step, somi_stream_t stream);
int somi_dcnv3_backward_f64(const double *input, const double *offset, const double *mask, const double *grad_output, double *grad_input,
                            double *grad_offset, double *grad_mask, int N, int H, int W, int G, int Gc, int kernel_h, int kernel_w,
                            int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, float offset_scale,
                            int im2col_step, void *workspace, size_t workspace_bytes, somi_stream_t stream);

/* Pieces of the DCNv3 nn.Module around the operator (models/ops_dcnv3/modules/dcnv3.py:283-291,334,370-376):
 *  LayerNorm over C (biased variance, eps inside the sqrt) + activation on contiguous NHWC;
 *  softmax over the K points of each (pixel, group): x, y are (n_groups, K) contiguous;
 *  centre-feature-scale blend y = x*(1-s) + xproj*s with s = sigmoid(logit[p*logit_cs + g]). */
int somi_layernorm_act_nhwc_f32(const float *x, const float *gamma, const float *beta, float eps, int act, float *y,
                                long npix, int C, somi_stream_t stream);
/* depthwise 3x3 conv (+bias) -> LayerNorm over C -> activation in ONE pass (the DCNv3 block's dw_conv chain, modules/dcnv3.py:283-291), C == 256:
 * u = the conv output (the LayerNorm backward reads it), y = act(LN(u)); bit-identical to somi_dwconv3x3_nhwc_f32 + somi_layernorm_act_nhwc_f32. */
int somi_dwconv3x3_ln_nhwc_f32(const float *x, const float *w, const float *bias, const float *gamma, const float *beta, float eps, int act,
                               float *u, float *y, int B, int H, int W, int C, somi_stream_t stream);
int somi_group_softmax_f32(const float *x, float *y, long n_groups, int K, somi_stream_t stream);
/* group g of pixel p at x + p*x_stride + g*K (y likewise); x == y allowed */
int somi_group_softmax_strided_f32(const float *x, long x_stride, float *y, long y_stride, long npix, int G, int K, somi_stream_t stream);
int somi_dcnv3_cfs_blend_f32(const float *x, const float *xproj, const float *logit, int logit_cs, float *y, long npix,
                             int G, int Gc, somi_stream_t stream);

/* Backward of those pieces (training through the DCNv3 module).  LayerNorm->GELU: z = gelu(LN(u)), du from dz; dgamma / dbeta
 * are ACCUMULATED; workspace: somi_layernorm_act_bwd_workspace_floats(npix, C) floats.  Softmax: dx = y*(dy - sum dy*y).
 * Blend: dx = dout*(1-s), dxproj = dout*s, dlogit[p][g] = s(1-s) * sum_c dout*(xproj - x)  (dlogit row stride dlogit_cs). */
size_t somi_layernorm_act_bwd_workspace_floats(long npix, int C);
int somi_layernorm_gelu_bwd_nhwc_f32(const float *u, const float *gamma, const float *beta, float eps, const float *dz, float *du,
                                     float *dgamma_accumulate, float *dbeta_accumulate, float *workspace, long npix, int C,
                                     somi_stream_t stream);
int somi_group_softmax_bwd_f32(const float *y, const float *dy, float *dx, long n_groups, int K, somi_stream_t stream);
/* y rows of y_stride floats, dy / dx rows of d_stride floats; dx == dy allowed */
int somi_group_softmax_bwd_strided_f32(const float *y, long y_stride, const float *dy, float *dx, long d_stride, long npix, int G, int K,
                                       somi_stream_t stream);
int somi_dcnv3_cfs_blend_bwd_f32(const float *x, const float *xproj, const float *logit, int logit_cs, const float *dout, float *dx,
                                 float *dxproj, float *dlogit, int dlogit_cs, long npix, int G, int Gc, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bandwidth-bound layer kernels of Model._forward_once (models/yolo.py:1269-1290).
 */

/* uint8 NCHW image batch -> fp32 NHWC with 4 channels (4th = 0), scaled by 1/255
 * (train.py:249 `imgs.float()/255`, val.py:150-152).  Also accepts fp32 NCHW input via the _f32 form. */
int somi_image_u8_to_nhwc4(const uint8_t *img, float *y, int B, int C, int H, int W, somi_stream_t stream);
int somi_image_f32_to_nhwc4(const float *img, float *y, int B, int C, int H, int W, float scale, somi_stream_t stream);

/* Depthwise 3x3, stride 1, pad 1, + bias, then act, then per-channel affine, then optional residual.
 * Replaces SEAM's `Conv2d(groups=c) -> GELU -> BatchNorm2d` stages (+Residual) (models/common.py:8454-8466, 7183-7189).
 * w is [3][3][C] (tap-major), C % 4 == 0. */
int somi_dwconv3x3_nhwc_f32(const float *x, const float *w, const float *bias, const float *post_scale,
                            const float *post_shift, const float *residual, float *y, int B, int H, int W, int C,
                            int act, somi_stream_t stream);

/* SPPF pooling: from x = slice [x_coff, x_coff+C) of a (B,H,W,cs) tensor write the three chained 5x5/s1/p2
 * max-pools (== 5x5, 9x9, 13x13 windows) to the slices at y_coff + {1,2,3}*C of the same tensor
 * (models/common.py:1856-1861).  In-place on one concat buffer: the pooled slices never alias the source slice. */
int somi_sppf_pool_nhwc_f32(float *buf, int B, int H, int W, int C, int cs, int x_coff, somi_stream_t stream);
/* The same for a training forward, level by level (three launches), leaving for every (element, level) the position r*5 + q of the first maximum
 * (row-major) in its 5x5 window of the previous slice: `codes` = 3*B*H*W*C bytes, handed to somi_sppf_pool_bwd_nhwc_f32 as its workspace with buf = NULL. */
int somi_sppf_pool_codes_nhwc_f32(float *buf, void *codes, int B, int H, int W, int C, int cs, int x_coff, somi_stream_t stream);

/* Max-pooling outside SPPF's chained 5x5 (pool.hip).  NHWC fp32 channel slices (the slice rule above); C is a multiple of 4.
 * Routing rule of every entry: a pooled value's gradient goes to the FIRST maximum of its full window in row-major order (torch's max_pool2d
 * autograd on the CPU); the forward leaves that position as one byte r * k + q per pooled element (`codes`, NULL in eval), the backward gathers by
 * it: owner-computes, a fixed order of terms, no float atomics.
 *
 * maxpool2: nn.MaxPool2d(2, stride, 0), stride 1 or 2, floor mode, over x zero-padded by (pad_l, pad_r, pad_t, pad_b), each 0 or 1 - with
 *   (0, 1, 0, 1) and stride 1 it is yolov3-tiny's nn.ZeroPad2d([0, 1, 0, 1]) + nn.MaxPool2d(2, 1, 0) in one pass.  The pad VALUE is 0 (not -inf): it wins
 *   over negative activations, and the gradient of an output it won is dropped.  x (B,H,W,x_cs) -> y (B,Ho,Wo,y_cs), Ho = (H + pad_t + pad_b - 2) / stride + 1;
 *   codes: B*Ho*Wo*C bytes.  The backward WRITES dx (B,H,W,dx_cs) - elements no window covers get 0; at stride 2 windows do not overlap and no sums form.
 * spp_pool: the nk (1..3) PARALLEL stride-1 windows k0 < k1 < k2 of SPP (models/common.py:1806-1826), each odd and 3 <= k <= 13, implicit -inf pad of k / 2:
 *   from x = slice [x_coff, x_coff + C) of buf (B,H,W,cs) the slices at x_coff + (i + 1) * C = pool_k[i](x), in place, in one walk over the largest window.
 *   codes: nk*B*H*W*C bytes, window-major.  The backward ADDS the routed gradients of dbuf's slices 1..nk into its slice 0 (which holds x's direct
 *   gradient from the concat's consumer). */
/* maxpool3s2: F.max_pool2d(x, 3, stride=2, padding=1) (ASFF level 0, models/common.py:5536).  The pad is an implicit -inf (it never wins; maxpool2's
 *   pad value is 0).  x (B,H,W,.) -> y (B,Ho,Wo,.), Ho = (H + 2 - 3) / 2 + 1, any H, W >= 1; codes: B*Ho*Wo*C bytes, r * 3 + q each.  The backward
 *   WRITES dx (B,H,W,.): an element gathers from the up to four windows that cover it, nothing else writes it. */
int somi_maxpool3s2_nhwc_f32(const somi_slice *x, const somi_slice *y, void *codes, int B, int H, int W, int C, somi_stream_t stream);
int somi_maxpool3s2_bwd_nhwc_f32(const somi_slice *dy, const void *codes, const somi_slice *dx, int B, int H, int W, int C, somi_stream_t stream);
int somi_maxpool2_nhwc_f32(const float *x, float *y, void *codes, int B, int H, int W, int C, int x_cs, int x_coff, int y_cs, int y_coff, int stride,
                           int pad_l, int pad_r, int pad_t, int pad_b, somi_stream_t stream);
int somi_maxpool2_bwd_nhwc_f32(const float *dy, const void *codes, float *dx, int B, int H, int W, int C, int dy_cs, int dy_coff, int dx_cs, int dx_coff,
                               int stride, int pad_l, int pad_r, int pad_t, int pad_b, somi_stream_t stream);
int somi_spp_pool_nhwc_f32(float *buf, void *codes, int B, int H, int W, int C, int cs, int x_coff, int nk, int k0, int k1, int k2,
                           somi_stream_t stream);
int somi_spp_pool_bwd_nhwc_f32(const void *codes, float *dbuf, int B, int H, int W, int C, int cs, int x_coff, int nk, int k0, int k1, int k2,
                               somi_stream_t stream);

/* The learned 2x upsamplers of the neck (upsample.hip).  NHWC fp32 channel slices (the slice rule above); C is a multiple of 4.  New symbols only: the ABI
 * version does not move.
 *
 * carafe: out[c, 2h+dy, 2w+dx] = sum_{a,b} softmax_t(logits[t*4 + dy*2 + dx, h, w])[a*k+b] * x[c, h+a-r, w+b-r], k = k_up (3 or 5), r = k / 2, x zero outside
 *   the map (models/common.py:4476-4490 without the unfolded tensor).  x (B,H,W,x_cs), logits (B,H,W,l_cs) = the 4*k*k channels of the encoder conv,
 *   out (B,2H,2W,o_cs).  weights: NULL (eval) or B*2H*2W*k*k floats that receive the softmax weights per OUTPUT pixel - the only tensor backward needs.
 *   No workspace.  The backward WRITES dx (B,H,W,dx_cs) - owner-computes, a fixed order of terms - and dlogits (B,H,W,dl_cs) in the logits' channel
 *   layout: p * (dp - sum p * dp), dp[a*k+b] = sum_c dout * x.  No float atomics.
 * dysample (style 'lp', no dyscope): offset (B,H,W,f_cs) is the raw output of the 1x1 offset conv, 8 * groups channels (x in the first half, y in the
 *   second), init_pos 8 * groups floats.  For j = g*4 + dy*2 + dx: sx = w + 0.25 * offset[j] + init_pos[j], sy = h + 0.25 * offset[4*groups + j] +
 *   init_pos[4*groups + j], clamped to the map; out[2h+dy, 2w+dx] = the bilinear sample of x's channels of group g there.  C % groups == 0 and
 *   (C / groups) % 4 == 0.  The backward WRITES dx (owner-computes over the output pixels whose source pixel lies within 2 pixels; a bilinear corner
 *   farther than that from its source pixel is added with an fp32 atomic and counted into *far_count, a device uint32 the caller zeroes: 0 <=> the launch
 *   was bit-reproducible) and doffset (B,H,W,df_cs) in offset's layout, the 0.25 included, 0 where the coordinate was clamped. */
int somi_carafe_nhwc_f32(const float *x, const float *logits, float *out, float *weights, int B, int H, int W, int C, int k_up, int x_cs, int x_coff,
                         int l_cs, int l_coff, int o_cs, int o_coff, somi_stream_t stream);
int somi_carafe_bwd_nhwc_f32(const float *dout, const float *x, const float *weights, float *dx, float *dlogits, int B, int H, int W, int C, int k_up,
                             int d_cs, int d_coff, int x_cs, int x_coff, int dx_cs, int dx_coff, int dl_cs, int dl_coff, somi_stream_t stream);
int somi_dysample_nhwc_f32(const float *x, const float *offset, const float *init_pos, float *out, int B, int H, int W, int C, int groups, int x_cs,
                           int x_coff, int f_cs, int f_coff, int o_cs, int o_coff, somi_stream_t stream);
int somi_dysample_bwd_nhwc_f32(const float *dout, const float *x, const float *offset, const float *init_pos, float *dx, float *doffset, void *far_count,
                               int B, int H, int W, int C, int groups, int d_cs, int d_coff, int x_cs, int x_coff, int f_cs, int f_coff, int dx_cs,
                               int dx_coff, int df_cs, int df_coff, somi_stream_t stream);

/* Adaptive spatial feature fusion (ASFF.forward, models/common.py:5551-5560; asff.hip), the data-dependent cousin of the BiFPN fusion below.
 * Per pixel of the (B,H,W) output:  L = w . cat(v_0, v_1, v_2) + bias (the 48 -> 3 1x1 `weight_levels` conv),  p = softmax(L) with the maximum
 * subtracted,  fused = sum_i p_i * r_i.  Source r_i (C channels) and weight map v_i (16 channels) are each read at (h >> up, w >> up) with their own
 * up in {0, 1, 2}: r_i is a (B, H >> r_up[i], W >> r_up[i], .) slice, v_i a (B, H >> v_up[i], W >> v_up[i], .) slice; H and W are multiples of the
 * largest factor.  No upsampled, concatenated or per-source product tensor is formed.
 * forward  (somi_asff_fuse_nhwc_f32): writes `out` = fused and, when p is given (training), p (B,H,W,3) contiguous - all backward needs beyond its inputs.
 * backward (somi_asff_fuse_bwd_nhwc_f32): `out` holds dfused (read).  dL_i = p_i (<dfused, r_i> - sum_j p_j <dfused, r_j>);
 *   dr[i] = p_i * dfused in r_i's layout - the owner of a low-resolution element sums its 4 or 16 children in row-major order; dr[i].p NULL skips it,
 *   dr_accumulate[i] adds to what dr[i] holds;  dv[i] = w^T dL in v_i's layout, summed over the children likewise (written);  dw[3][48] and db[3]
 *   ACCUMULATED: one partial per workgroup in `workspace` (somi_asff_fuse_bwd_workspace_floats(B, H, W) floats, 16-byte aligned), then one
 *   fixed-order reduce.  No float atomics: two launches are bit-identical. */
typedef struct somi_asff_desc {
    somi_slice r[3], v[3];     /* the sources (width C) and the weight maps (width 16) */
    int32_t r_up[3], v_up[3];
    const float *w;            /* [3][48], 16-byte aligned */
    const float *bias;         /* [3] */
    somi_slice out;            /* forward: fused, written; backward: dfused, read (B,H,W,.) */
    float *p;                  /* (B,H,W,3): forward writes it when non-NULL, backward reads it */
    somi_slice dr[3], dv[3];   /* backward only */
    int32_t dr_accumulate[3];
    int32_t B, H, W, C;
    float *dw, *db;            /* backward only, accumulated */
    float *workspace;
    uint64_t workspace_floats;
} somi_asff_desc;
size_t somi_asff_desc_bytes(void);   /* sizeof(somi_asff_desc) as the library was compiled: lets a binding check its mirror */
size_t somi_asff_fuse_bwd_workspace_floats(int B, int H, int W);
int somi_asff_fuse_nhwc_f32(const somi_asff_desc *d, somi_stream_t stream);
int somi_asff_fuse_bwd_nhwc_f32(const somi_asff_desc *d, somi_stream_t stream);

/* Coordinate attention (CoorAttention, models/common.py:1399-1450; CABottleneck, :4884-4922; coordatt.hip): the four passes over the map
 * x (B,H,W,.) that the attention makes; the small tensors between them (conv1, bn1, h-swish, conv_h / conv_w, sigmoid, B * (H + W) rows) run on
 * the conv and BatchNorm entries.  Every tensor is a channel slice of width C (a multiple of 4).  A "row tensor" (a_h, a_w, r_h, r_w) is a
 * (B, rows, .) tensor with `*_rows` rows per image: [b][h] is read or written for h < H (a_h, r_h), [b][w] for w < W (a_w, r_w).  With rows = H
 * and W they are the plain (B,H,C) and (B,W,C) tensors; with rows = H + W and the second pointer advanced by H rows they are the two halves of
 * one tensor in `pool`'s layout - how the blocks run conv_h and conv_w as one 1x1 conv over conv1's output.
 * means     (somi_coordatt_means_nhwc_f32):     pool (B, H + W, .): rows [0,H) = the mean over W per (b,h,c), rows [H,H+W) = the mean over H per
 *           (b,w,c) - the reference's cat([x_h, x_w.permute], dim=2), so conv1 runs on it as a (B, H + W, 1, C) map.  One pass over x.
 * apply     (somi_coordatt_apply_nhwc_f32):     y = [res +] x * a_h[b,h,c] * a_w[b,w,c], the gates already sigmoided; res (optional) is the
 *           bottleneck's shortcut.  No expanded gate and no x * a_w product reaches memory.
 * bwd gates (somi_coordatt_bwd_gates_nhwc_f32): y holds dout (read).  r_h[b,h,c] = sum_w dout x a_w, r_w[b,w,c] = sum_h dout x a_h, WRITTEN;
 *           dout and x are read once for both.
 * bwd input (somi_coordatt_bwd_input_nhwc_f32): y holds dout (read), r_h / r_w the gradients of the two means (read: the two halves of conv1's
 *           input gradient).  dx = dout a_h a_w + r_h[b,h,c] / W + r_w[b,w,c] / H, written, or added to what dx holds with `accumulate`; x is
 *           not read.
 * So forward and backward each make two passes over the (B,H,W,C) tensors.  means and bwd gates sum through per-workgroup partials in
 * `workspace` (somi_coordatt_workspace_floats(B, H, W, C) floats, 16-byte aligned) and a fixed-order second stage.  No float atomics: two
 * launches are bit-identical. */
typedef struct somi_coordatt_desc {
    somi_slice x;              /* the attended map x1 (B,H,W,.), read (unused by bwd input) */
    somi_slice y;              /* apply: the output, written; both backward passes: dout, read; unused by means */
    somi_slice res;            /* apply only; res.p NULL: no shortcut */
    somi_slice pool;           /* means only: (B, H + W, .), written */
    somi_slice a_h, a_w;       /* the gates, read (all but means) */
    int32_t a_h_rows, a_w_rows;
    somi_slice r_h, r_w;       /* bwd gates: da_h, da_w, written; bwd input: gh, gw, read */
    int32_t r_h_rows, r_w_rows;
    somi_slice dx;             /* bwd input only */
    int32_t accumulate;        /* bwd input: add to what dx holds */
    int32_t B, H, W, C;
    float *workspace;          /* means and bwd gates */
    uint64_t workspace_floats;
} somi_coordatt_desc;
size_t somi_coordatt_desc_bytes(void);   /* sizeof(somi_coordatt_desc) as the library was compiled: lets a binding check its mirror */
size_t somi_coordatt_workspace_floats(int B, int H, int W, int C);
int somi_coordatt_means_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream);
int somi_coordatt_apply_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream);
int somi_coordatt_bwd_gates_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream);
int somi_coordatt_bwd_input_nhwc_f32(const somi_coordatt_desc *d, somi_stream_t stream);

/* Efficient multi-scale attention (EMA, models/common.py:5263-5292; ema.hip): the passes over the map x (B,H,W,.) that are EMA's own.  With
 * g = factor, cg = C / g, channel c = gi * cg + j and N = H * W: the means pass is somi_coordatt_means_nhwc_f32, conv1x1 (cg -> cg, shared by
 * the groups, with bias and a sigmoid epilogue) runs on the conv entry over the (B, H + W, g, cg) view and leaves sg = sigmoid(hw)
 * (B, H + W, .) in pool's layout, conv3x3 (cg -> cg, shared) leaves x2 (B,H,W,.).  Every slice is C wide.  gamma, beta: gn's affine, cg floats.
 * stats    (somi_ema_stats_nhwc_f32):    reads x, sg and x2 (optional) once.  stats (B, 3, C): the mean of t = x * sg_h * sg_w per (b, c), its sum
 *          of squared deviations (around a pivot, t at pixel (0, 0); never sum t^2 - (sum t)^2 / N) and the mean of x2.  vec (B, 4, C): mean,
 *          rstd = 1 / sqrt(M2 / N + eps), x21 = softmax over the group of the x2 means, x11 = softmax over cg of beta (the mean of the normalised
 *          map is its shift); both softmaxes subtract the maximum.
 * gate     (somi_ema_gate_nhwc_f32):     y = [res +] x * sigmoid(wgt), wgt[b,gi,h,w] = sum_j x11[j] x2[..j] + x21[b,gi,j] x1[..j],
 *          x1 = gamma * (t - mean) * rstd + beta rebuilt in registers.  x1, the expanded gates and wgt never reach memory.
 * bwd gate (somi_ema_bwd_gate_nhwc_f32): y holds dout (read).  dx = dout * sigmoid(wgt), written or added with `accumulate`; dw = dwgt =
 *          s (1 - s) sum_j dout x, the same value over the cg channels of a group; sums (B, 3, C) = sum dwgt * that, sum dwgt, sum dwgt * x2 per
 *          (b, c) (that = (t - mean) * rstd); bvec (B, 3, C): what the next pass needs per (b, c); dgamma, dbeta (cg floats) ADDED to, (b, gi) in order.
 * bwd norm (somi_ema_bwd_norm_nhwc_f32): reads x, sg, dw.  y = dt, the gradient of t (the instance-norm backward), written; dw becomes
 *          dx2 = dwgt * x11 + the softmax term / N in place; dsg (B, H + W, .) = the gradient of hw (in front of the sigmoid): the row and
 *          column sums of dt * t, times 1 - sg.  The input gradient is then finished by the conv backward of conv3x3 (accumulating into dx),
 *          of conv1x1 and by somi_coordatt_bwd_input_nhwc_f32(y = dt, a_h / a_w = sg, r_h / r_w = d means, accumulate).
 * Two passes of EMA's own forward (stats, gate) and two backward.  Reductions go through per-workgroup partials in `workspace`
 * (somi_ema_workspace_floats(B, H, W, C) floats, 16-byte aligned), somi_ema_partials(B, H, W, C) per (b, c), and a fixed-order second stage.  No
 * float atomics: two launches are bit-identical.  SOMI_ENOTIMPL before any launch: C % factor != 0, cg % 4 != 0, cg > 64 (what a group
 * reduction holds), C > 1024 with a cg / 4 that does not divide 256, a tensor of more than 2^30 floats. */
typedef struct somi_ema_desc {
    somi_slice x;              /* the map (B,H,W,.), read by all four */
    somi_slice x2;             /* conv3x3(x) + bias, read: stats (x2.p NULL: no mean of x2), gate, bwd gate */
    somi_slice sg;             /* sigmoid(conv1x1(means)) (B, H + W, .), read by all four */
    somi_slice y;              /* gate: the output, written; bwd gate: dout, read; bwd norm: dt, written */
    somi_slice res;            /* gate only; res.p NULL: no residual */
    somi_slice dx;             /* bwd gate only */
    somi_slice dw;             /* bwd gate: dwgt, written; bwd norm: dwgt read, dx2 written */
    somi_slice dsg;            /* bwd norm only: (B, H + W, .), written */
    const float *gamma, *beta;
    float *stats, *vec;        /* stats: written; the others read vec */
    float *sums, *bvec;        /* bwd gate: written; bwd norm reads bvec */
    float *dgamma, *dbeta;     /* bwd gate: added to */
    float eps;
    int32_t factor;
    int32_t accumulate;        /* bwd gate: add to what dx holds */
    int32_t B, H, W, C;
    float *workspace;          /* all but gate */
    uint64_t workspace_floats;
} somi_ema_desc;
size_t somi_ema_desc_bytes(void);        /* sizeof(somi_ema_desc) as the library was compiled */
size_t somi_ema_workspace_floats(int B, int H, int W, int C);
int somi_ema_partials(int B, int H, int W, int C);      /* host arithmetic: partials per (b, c) of the reductions over the map (0: bad sizes) */
int somi_ema_stats_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream);
int somi_ema_gate_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream);
int somi_ema_bwd_gate_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream);
int somi_ema_bwd_norm_nhwc_f32(const somi_ema_desc *d, somi_stream_t stream);

/* ACmix (models/common.py:7281-7365; acmix.hip): a 7x7 sliding-window attention over 4 heads with reflection padding 3 and a linear position
 * term, mixed with a grouped 3x3 conv over the same q, k, v.  C = out_planes, D = C / 4, channel (head h, dim d) = h * D + d, s = D ** -0.5; q, k, v
 * are slices C wide (in the block: thirds of the stacked 1x1 projection).  wp: conv_p.weight, (D, 2) floats, column 0 for x; rate1, rate2: one
 * float each, read on the device.  r(.) reflects an index, lx(x) = -1 + 2 x / (W - 1), ly(y) likewise.
 * attn    (somi_acmix_attn_nhwc_f32):        score_j = s * (q_p . k_r(p+j) + (q_p . wp[:, 0]) (lx(p) - lx(r(p+j))) + (q_p . wp[:, 1]) (ly(p) - ly(r(p+j))))
 *         over the 49 taps j, a = softmax (maximum subtracted), out = rate1 * sum_j a_j v_r(p+j) [+ rate2 * mix].  lse (optional, 4 wide): the
 *         log-sum-exp per (pixel, head), written.  conv_p.bias cancels and the position map is never built.
 * bwd q   (somi_acmix_attn_bwd_q_nhwc_f32):  out holds dout (read).  dq written (added with `accumulate`); aux (24 wide) written per (pixel, head):
 *         delta = sum_j a_j (rate1 dout_p . v_j), q . wp[:, 0], q . wp[:, 1], sum_j dS_j dx_j, sum_j dS_j dy_j, 1 / sum_j exp(score_j - lse) (the fp32 lse leaves that sum off 1); dwp (D, 2) and
 *         drates = (sum dout . att, sum dout . mix (0 without mix)) WRITTEN, from partials in `workspace` folded in a fixed order.
 * bwd kv  (somi_acmix_attn_bwd_kv_nhwc_f32): reads q, k, v, dout, lse and the aux bwd q wrote.  dk, dv written (added with `accumulate`) by the
 *         owner pixel: each query of the clipped window around it counts once per tap that reflects onto the owner.
 * conv    (somi_acmix_conv_nhwc_f32):        mix[., 4 d + o] = bias[4 d + o] + sum_(t, tap) weff[t][tap][d][o] * src_t[p + tap][d] with zero padding,
 *         the 12 sources t = 4 * (q, k, v) + head: dep_conv(fc(.)) as ONE grouped conv, the 9 D-channel fc output never exists.
 *         weff: (12, 9, D, 4) floats from somi_acmix_fold_weff_f32(fc.weight (9, 12), dep_conv.weight (C, 9, 3, 3)).
 * conv bwd data / weight: out holds dout.  data: dq, dk, dv = rate2 * the transposed conv of dout, written (added with `accumulate`).  weight:
 *         dweff (weff's layout) and dbias (C) = rate2 * the sums over the map, WRITTEN, partials in `workspace` folded in order;
 *         somi_acmix_split_dweff_f32 turns dweff into the gradients of fc.weight and dep_conv.weight (written).
 * Workspace: somi_acmix_workspace_floats(B, H, W, C) floats, 16-byte aligned (bwd q, conv bwd weight).  The reductions use partials folded in
 * a fixed order: two launches are bit-identical.  SOMI_ENOTIMPL before any launch: C % 16 != 0, C > 1024, a tensor of more than 2^30
 * floats; SOMI_EINVAL: H < 4 or W < 4 (the reflection pad of 3), a broken slice, a missing pointer or workspace. */
typedef struct somi_acmix_desc {
    somi_slice q, k, v;        /* (B,H,W,.), read (conv bwd data: unused) */
    somi_slice mix;            /* conv: written; attn, bwd q: read, optional */
    somi_slice out;            /* attn: the output, written; every backward pass: dout, read */
    somi_slice lse;            /* 4 wide; attn: written (optional); bwd q, bwd kv: read */
    somi_slice aux;            /* 24 wide; bwd q: written; bwd kv: read */
    somi_slice dq, dk, dv;     /* bwd q: dq; bwd kv: dk, dv; conv bwd data: all three */
    const float *wp, *rate1, *rate2;
    const float *weff, *bias;  /* conv, conv bwd data (weff) */
    float *dwp, *drates;       /* bwd q: written */
    float *dweff, *dbias;      /* conv bwd weight: written */
    int32_t accumulate;        /* bwd q, bwd kv, conv bwd data: add to what dq / dk / dv hold */
    int32_t B, H, W, C;
    float *workspace;          /* bwd q, conv bwd weight */
    uint64_t workspace_floats;
} somi_acmix_desc;
size_t somi_acmix_desc_bytes(void);      /* sizeof(somi_acmix_desc) as the library was compiled */
size_t somi_acmix_workspace_floats(int B, int H, int W, int C);    /* 0: sizes outside the path */
int somi_acmix_plan(int H, int W, int *tile, int *tiles_y, int *tiles_x);   /* host arithmetic: the square pixel tile of a workgroup and their count per image */
int somi_acmix_attn_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream);
int somi_acmix_attn_bwd_q_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream);
int somi_acmix_attn_bwd_kv_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream);
int somi_acmix_conv_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream);
int somi_acmix_conv_bwd_data_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream);
int somi_acmix_conv_bwd_weight_nhwc_f32(const somi_acmix_desc *d, somi_stream_t stream);
int somi_acmix_fold_weff_f32(const float *fc, const float *dep, float *weff, int C, somi_stream_t stream);
int somi_acmix_split_dweff_f32(const float *dweff, const float *fc, const float *dep, float *dfc, float *ddep, int C, somi_stream_t stream);

/* Channel prior convolutional attention (CPCA, CPCABottleneck: models/common.py:5753-5859; cpca.hip): the strip part
 *   s = u + V7(H7(u)) + V11(H11(u)) + V21(H21(u)),  H_k the depthwise (1,k) conv along W, V_k the depthwise (k,1) conv along H, zero padding k / 2,
 * and the element-wise passes of the block; its 1x1 conv, GELU, depthwise 5x5, global pools and channel scale run on the existing entries.
 * Every tensor is a channel slice of width C (a multiple of 4) of a (B,H,W,.) tensor.  Tap tensors w[k] are (C, taps[k]) floats - how
 * nn.Conv2d stores (C,1,1,k) and (C,1,k,1) -, biases (C) floats; neither needs any alignment beyond a float's.  taps must be (7, 11, 21).
 * fan-out (somi_cpca_fanout_nhwc_f32): dst[k] = S_k(src[0]) [+ bias[k]] for the three tap sets; src[0] is read once.
 * fan-in  (somi_cpca_fanin_nhwc_f32):  dst[0] = [dst[0] +] src[3] + sum_k (S_k(src[k]) [+ bias[k]]); `accumulate` adds to what dst[0] holds.
 * axis 0: S_k runs along W, 1: along H.  flip: the taps are walked backwards (the transposed conv of the data gradient).  bias[k] NULL: none.
 * Training forward: fan-out along W, fan-in along H (9 tensor passes, the three t_k = dst of the fan-out kept); data gradient: fan-out along H
 * of ds, flipped, no bias -> dt_k; fan-in along W of dt_k, flipped, no bias, src[3] = ds -> du.
 * wgrad (somi_cpca_wgrad_nhwc_f32): from u, t_k, ds, dt_k all 78 tap gradients, dw_h[k] (C, taps[k]) and dw_v[k] likewise, and the six bias
 * gradients db_h[k] = sum dt_k, db_v[k] = sum ds (C each), written, or added to what they hold with `accumulate`; a NULL target is skipped.
 * Per-workgroup rows of partials in `workspace` (somi_cpca_wgrad_workspace_floats floats, 16-byte aligned), then a fixed-order tree.
 * No float atomics anywhere: two launches are bit-identical. */
typedef struct somi_cpca_strip_desc {
    somi_slice src[4];         /* fan-out: src[0]; fan-in: src[0..2] the three branch tensors, src[3] the pass-through */
    somi_slice dst[3];         /* fan-out: the three results; fan-in: dst[0] */
    const float *w[3];
    const float *bias[3];
    int32_t taps[3];           /* 7, 11, 21 */
    int32_t axis, flip, accumulate;
    int32_t B, H, W, C;
} somi_cpca_strip_desc;
typedef struct somi_cpca_wgrad_desc {
    somi_slice u, t[3], ds, dt[3];
    float *dw_h[3], *dw_v[3], *db_h[3], *db_v[3];
    int32_t taps[3];
    int32_t accumulate;
    int32_t B, H, W, C;
    float *workspace;
    uint64_t workspace_floats;
} somi_cpca_wgrad_desc;
size_t somi_cpca_strip_desc_bytes(void);
size_t somi_cpca_wgrad_desc_bytes(void);
int somi_cpca_fanout_nhwc_f32(const somi_cpca_strip_desc *d, somi_stream_t stream);
int somi_cpca_fanin_nhwc_f32(const somi_cpca_strip_desc *d, somi_stream_t stream);
size_t somi_cpca_wgrad_workspace_floats(int B, int H, int W, int C);
/* How many tiles in a row a workgroup of the strip kernels (wgrad = 0) or of the weight gradient's first stage (wgrad = 1) walks along
 * `axis` at this shape - host arithmetic: 4 (32) halved while fewer than 1024 (512) workgroups exist.  0 for sizes the kernels refuse. */
int somi_cpca_tiles_per_workgroup(int B, int H, int W, int C, int axis, int wgrad);
int somi_cpca_wgrad_nhwc_f32(const somi_cpca_wgrad_desc *d, somi_stream_t stream);
/* out = x * y (the gate product conv(s) * a), and its backward dx = dout * y, dy = dout * x; npix pixels, slices of width C */
int somi_cpca_gate_nhwc_f32(somi_slice x, somi_slice y, somi_slice out, long npix, int C, somi_stream_t stream);
int somi_cpca_gate_bwd_nhwc_f32(somi_slice dout, somi_slice x, somi_slice y, somi_slice dx, somi_slice dy, long npix, int C, somi_stream_t stream);
/* CPCA_ChannelAttention's sum of two sigmoids: z (2B, C) = the shared MLP on the B average rows, then on the B maximum rows;
 * g[b][c] = sigmoid(z[b][c]) + sigmoid(z[B + b][c]);  backward: dz (2B, C) from dg (B, C). */
int somi_cpca_sigmoid2_f32(const float *z, float *g, int B, int C, somi_stream_t stream);
int somi_cpca_sigmoid2_bwd_f32(const float *z, const float *dg, float *dz, int B, int C, somi_stream_t stream);
/* amaxp[b][c] = the first pixel p with x[b,p,c] == mx[b][c], mx the spatial maximum somi_global_pool_nhwc_f32 took of the same tensor: what
 * somi_pool_bwd_add_nhwc_f32 needs.  An integer minimum over the matching pixels, independent of the order. */
int somi_cpca_argmax_pixel_nhwc_f32(somi_slice x, const float *mx, int32_t *amaxp, int B, int HW, int C, somi_stream_t stream);

/* Tail attention of the CBAM C3 family (SCBAMBottleneck, models/common.py:975-995; the bare C3CBAM row, :494-504; cbam_c3.hip): a map t
 * (B,H,W,.) combined with its channel gate ca (B, C) and its spatial gate sa (B, H, W) into a channel slice, plus an optional shortcut:
 *   SOMI_GATE_PRODUCT      out = t * ca * sa [+ residual]
 *   SOMI_GATE_SIGMOID_SUM  out = sigmoid(t * (ca + sa)) [+ residual]
 * residual.p NULL: none.  out may be t or residual themselves.  B <= 65535, B * HW < 2^31, C % 4 == 0; ca 16-byte aligned.
 * Backward in two passes with the spatial gate's own backward between them:
 *  pixel: dsa[p] = sum_c g * t * ca (product, g = dout) or sum_c g * t (sigmoid-sum, g = dout * o * (1 - o), o the forward's sigmoid), written
 *         raw (logit = 0) or times sa * (1 - sa) (logit = 1: what somi_spatial_attn_bwd_f32 takes); amaxc[p] = the first channel of the
 *         pixel's maximum of t * ca; with t_max (B, C) = the spatial maxima of t the forward pooled, amaxp[b][c] = the first pixel that
 *         holds it (an integer minimum, order-independent).  t_max and amaxp are given together or not at all.  A channel none of whose
 *         values equals its t_max (a NaN in t, or a t_max from elsewhere) keeps 0x7f7f7f7f, which is no pixel: somi_pool_bwd_add_nhwc_f32
 *         compares against amaxp and never indexes with it, so the maximum's gradient then goes nowhere.  B * C < 2^31.
 *  chan:  with dstats (B,H,W,2) the gradient of [mean_c, max_c] of t * ca,  dt1 = dstats0 / C + [c == amaxc] * dstats1 (+ dout * sa, product);
 *         product: dca = sum_p dt1 * t, dt = dt1 * ca;  sigmoid-sum: dca = sum_p (g + dt1) * t, dt = g * (ca + sa) + dt1 * ca.
 *         dt is written, or added to with `accumulate`; it may be dout itself.  dca (B, C) is written.  workspace:
 *         somi_gate_combine_bwd_workspace_floats floats, 16-byte aligned: per-workgroup partials, finished in ascending order in fp64.
 * No float atomics: two launches are bit-identical. */
#define SOMI_GATE_PRODUCT 0
#define SOMI_GATE_SIGMOID_SUM 1
int somi_gate_combine_nhwc_f32(somi_slice t, const float *ca, const float *sa, somi_slice residual, somi_slice out, int B, int HW, int C, int mode,
                               somi_stream_t stream);
int somi_gate_combine_bwd_pixel_f32(somi_slice dout, somi_slice t, const float *ca, const float *sa, const float *t_max, float *dsa,
                                    int32_t *amaxc, int32_t *amaxp, int B, int HW, int C, int mode, int logit, somi_stream_t stream);
/* How many trips of its grid-stride loop the busiest wave of the per-pixel pass makes at this shape - host arithmetic: at most 2048 workgroups
 * of four waves, a wave taking 64 / lanes pixels a trip, lanes = the smallest power of two covering C / 4.  0 for sizes the pass refuses. */
int somi_gate_combine_pixel_trips(int B, int HW, int C);
size_t somi_gate_combine_bwd_workspace_floats(int B, int HW, int C);
/* The depthwise-separable spatial gate of CBAMBottleneckDWC (SpatialAttentionModuleDWC, models/common.py:361-389, 425-438) on stats (B,H,W,2):
 *   u = depthwise k x k conv (bias, pad k / 2);  v = relu(BN(u));  p = 1x1 conv 2 -> 1 (bias);  q = relu(BN1(p));  sa = sigmoid(q);  k = 3 or 7.
 * params, 2 k k + 11 floats: depth_conv.weight (2,1,k,k), depth_conv.bias (2), bn.weight (2), bn.bias (2), point_conv.weight (2),
 * point_conv.bias, bn1.weight, bn1.bias.  run, 6 floats: bn.running_mean (2), bn.running_var (2), bn1.running_mean, bn1.running_var.
 * eval: running statistics, one launch.  train: batch statistics over the B H W > 1 values of a channel (biased variance), run (if given)
 * moved by `momentum` with the unbiased variance; keeps u (B,H,W,2), p (B,H,W) and st (8 floats: mean (2) and rstd (2) of u, mean and
 * rstd of p); three launches - the two BatchNorms are grid-wide reductions that follow one another.  bwd: from the RAW gradient of sa
 * (somi_gate_combine_bwd_pixel_f32 with logit = 0) dstats (B,H,W,2), and every parameter gradient ADDED to dparams_accumulate in the layout
 * of params.  workspace: somi_dwc_gate_workspace_floats floats, 16-byte aligned (fp64 partial rows, finished in a fixed order: bit-identical
 * launches).  somi_dwc_gate_trips: the trips of the kernels' grid-stride loops at this size (host arithmetic; at most 128 workgroups). */
size_t somi_dwc_gate_workspace_floats(int B, int H, int W, int k);
int somi_dwc_gate_trips(int B, int H, int W);
int somi_dwc_gate_eval_f32(const float *stats, const float *params, const float *run, float *sa, int B, int H, int W, int k, float eps,
                           somi_stream_t stream);
int somi_dwc_gate_train_f32(const float *stats, const float *params, float *u, float *p, float *st, float *run, float momentum, float eps,
                            float *sa, float *workspace, size_t workspace_floats, int B, int H, int W, int k, somi_stream_t stream);
int somi_dwc_gate_bwd_f32(const float *dsa, const float *stats, const float *u, const float *p, const float *st, const float *params,
                          float *dstats, float *dparams_accumulate, float *workspace, size_t workspace_floats, int B, int H, int W, int k,
                          somi_stream_t stream);
int somi_gate_combine_bwd_chan_f32(somi_slice dout, somi_slice t, const float *ca, const float *sa, const float *dstats, const int32_t *amaxc,
                                   somi_slice dt, float *dca, float *workspace, size_t workspace_floats, int B, int HW, int C, int mode,
                                   int accumulate, somi_stream_t stream);

/* SimAM attention (SimAM, models/common.py:2915-2939; SimAMWithSlicing, :9374-9408; SimAMWithFlexibleSlicing, :9411-9480; simam.hip): the
 * parameter-free energy gate as ONE operator over a grid of ny x nx regions of the map x (B,H,W,.).  Region (i, j) spans rows
 * [i * step_y, i * step_y + len_y) and columns [j * step_x, j * step_x + len_x); with stretch_last the last region of an axis runs to the map
 * edge (needs step == len).  Per (image, region r, channel), over the region's own N_r pixels:
 *   mu_r = mean x,  d = x - mu_r,  S_r = sum d^2,  D_r = 4 (S_r / n + lambda),  s = sigmoid(d^2 / D_r + 0.5),
 * the divisor n GIVEN, not derived from N_r.  The three modules are
 *   whole map  ny = nx = 1, len = step = (H, W), n = H W - 1;
 *   quadrants  ny = nx = 2, len = step = (H / 2, W / 2), stretch_last, n = (H / 2)(W / 2) - 1 for all four, the larger ones included;
 *   windows    len = t, step = st, ny = (H - t) / st + 1, nx = (W - t) / st + 1, n = t t - 1.
 * A pixel's weight in a region that covers it is w = 1 / k, k its 1-based rank among the regions covering the pixel in row-major order (the
 * reference divides a window's contribution by the coverage count at the time it is added, not by the final count); at most 4 regions may
 * cover a pixel along one axis (ceil(len / step) <= 4, else SOMI_ENOTIMPL).  A region has at least two pixels; lambda > 0.
 * Every tensor is a channel slice of width C (a multiple of 4).  stats and sums are plain (B, ny * nx, 2, C) tensors, 16-byte aligned.
 * stats     (somi_simam_stats_nhwc_f32):     stats[b][r][0] = mu_r, [1] = S_r, the sum of squared deviations about that mean (count, mean, M2
 *           partials merged by the pairwise update in a fixed order - not sum x^2 - N mu^2).  One pass over x.
 * apply     (somi_simam_apply_nhwc_f32):     y = [x +] sum_{r covers the pixel} w x s, written; a pixel no region covers gets 0 [+ x].
 *           add_input: the [x +] (PSSimAM's b + attn(b)).
 * bwd sums  (somi_simam_bwd_sums_nhwc_f32):  y holds dout = g (read).  sums[b][r][0] = A_r = sum T d, [1] = B_r = sum T d^2, T = w g x s (1 - s).
 * bwd input (somi_simam_bwd_input_nhwc_f32): dx = [g +] sum_{r covers} ( w g s + 2 T d / D_r - 2 A_r / (N_r D_r) - (8 / n) d B_r / D_r^2 ),
 *           written, or added to what dx holds with `accumulate`; the gate is recomputed from x and stats, [g +] with add_input.
 * stats and bwd sums split a region larger than one chunk over workgroups through `workspace` (somi_simam_workspace_floats(d) floats,
 * 16-byte aligned; 0: not needed, the pointer may be NULL) and a fixed-order second stage.  No float atomics: two launches are bit-identical. */
typedef struct somi_simam_desc {
    somi_slice x;              /* the map, read by all four */
    somi_slice y;              /* apply: the output, written; both backward passes: dout, read; unused by stats */
    somi_slice dx;             /* bwd input only */
    float *stats;              /* stats: written; the other three: read */
    float *sums;               /* bwd sums: written; bwd input: read */
    int32_t B, H, W, C;
    int32_t ny, nx, step_y, step_x, len_y, len_x, stretch_last;
    int32_t add_input;         /* apply: out = x + ...; bwd input: dx = g + ... */
    int32_t accumulate;        /* bwd input: add to what dx holds */
    float n, lambda;
    float *workspace;          /* stats and bwd sums */
    uint64_t workspace_floats;
} somi_simam_desc;
size_t somi_simam_desc_bytes(void);   /* sizeof(somi_simam_desc) as the library was compiled: lets a binding check its mirror */
size_t somi_simam_workspace_floats(const somi_simam_desc *d);   /* from B, H, W, C and the region grid; 0 for a grid the kernels refuse too */
int somi_simam_stats_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream);
int somi_simam_apply_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream);
int somi_simam_bwd_sums_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream);
int somi_simam_bwd_input_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream);

/* ASF-YOLO neck (Zoom_cat, models/common.py:4312-4327; ScalSeq, :4330-4355; attention_model, :4358-4424; asf.hip).  fp32, NHWC, every map a
 * channel slice whose width is a multiple of 4, one channel quad per lane.  Every reduction has a fixed order, no float atomics: two launches
 * on the same input are bit-identical.
 *
 * Zoom_cat.  l (B,2H,2W,.) Cl wide, m (B,H,W,.) Cm wide, s (B,(H+1)/2,(W+1)/2,.) Cs wide; out (B,H,W,.) Cl + Cm + Cs wide from out.coff.
 * forward (somi_zoomcat_nhwc_f32), one launch: out[..., 0:Cl] = max2x2(l) + mean2x2(l), out[..., Cl:Cl+Cm] = m (skipped when m.p is NULL: the
 *   producer wrote it in place), out[..., Cl+Cm:] = s at (h >> 1, w >> 1).  codes non-NULL (training): one byte per (pixel, quad of l's part),
 *   (B,H,W,Cl/4) bytes, two bits per channel (bits 2j, 2j+1 of channel 4q + j): the window position 2i + j of the maximum, the first one in
 *   row-major order on a tie.
 * backward (somi_zoomcat_bwd_nhwc_f32), one launch, owner-computes: `out` holds dout (read);
 *   dl[2h+i, 2w+j] = dout_l[h, w] * (1/4 + [code == 2i + j]),  dm = dout_m,  ds[hs, ws] = the sum of dout_s over the (up to) 2x2 pixels it fed;
 *   the gradients go to the slices l, m, s, each written, or added to what it holds with accumulate[k]; a NULL p skips that gradient. */
typedef struct somi_zoomcat_desc {
    somi_slice l, m, s;        /* forward: the inputs, read; backward: dl, dm, ds */
    somi_slice out;            /* forward: written; backward: dout, read */
    uint8_t *codes;            /* (B,H,W,Cl/4) bytes */
    int32_t B, H, W;           /* of m and out */
    int32_t Cl, Cm, Cs;
    int32_t accumulate[3];     /* backward: dl, dm, ds are added to */
} somi_zoomcat_desc;
size_t somi_zoomcat_desc_bytes(void);
int somi_zoomcat_nhwc_f32(const somi_zoomcat_desc *d, somi_stream_t stream);
int somi_zoomcat_bwd_nhwc_f32(const somi_zoomcat_desc *d, somi_stream_t stream);

/* ScalSeq's tail behind the three maps u_i = conv3d(.) kept at their own resolution: u3 (B,H,W,.), u4 (B,H/2,W/2,.),
 * u5 (B,H/4,W/4,.), H and W multiples of 4, all C wide.  The reference's (B,C,3,H,W) stack holds u3 once, every u4 pixel 4 times and every
 * u5 pixel 16 times: weights w = 1, 4, 16, N = 3 B H W elements per channel.
 * stats  (somi_scalseq_stats_f32):           mean and biased variance of the weighted union per channel (per-workgroup partial sums about the
 *        pivot running_mean - 0 when NULL - then one workgroup per channel quad adds them in a fixed order, in double) -> mean, rstd = 1 / sqrt(var + eps),
 *        scale = gamma rstd, shift = beta - mean scale (C floats each); running_mean / running_var, when given, move by `momentum` towards
 *        mean and var N / (N - 1), as nn.BatchNorm3d moves them.
 * fuse   (somi_scalseq_fuse_nhwc_f32):       out = max_i leaky0.1(scale u_i + shift), u4 read at (h / 2, w / 2), u5 at (h / 4, w / 4); the
 *        maximum is taken AFTER the affine (a negative gamma reverses the order), ties go to the first i.  scale / shift NULL: 1 and 0 (eval,
 *        the BatchNorm folded into the producing conv).  codes non-NULL: (B,H,W,C/4) bytes, two bits per channel, the winning i.
 * route  (somi_scalseq_route_bwd_nhwc_f32):  `out` holds dout.  One lane per (4x4-aligned tile of P3, quad) reads dout and codes once and
 *        writes g3, g4, g5: the gradient routed to branch i times the LeakyReLU slope there, the 2x2 / 4x4 children summed inside the tile;
 *        per-workgroup partials of sum g and sum g xhat over all three maps go to `workspace`, a second kernel of the launch adds them in
 *        a fixed order into sums (2, C) and ADDS dgamma += sum g xhat, dbeta += sum g (NULL: skipped).
 * apply  (somi_scalseq_apply_bwd_f32):       in place on g3, g4, g5: du_i = scale (g_i - w_i (m1 + xhat_i m2)), m1 = sum g / N,
 *        m2 = sum g xhat / N, xhat_i = (u_i - mean) rstd. */
typedef struct somi_scalseq_desc {
    somi_slice u3, u4, u5;     /* read by all four */
    somi_slice out;            /* fuse: written; route: dout, read */
    somi_slice g3, g4, g5;     /* route: written; apply: read and overwritten */
    uint8_t *codes;            /* fuse: written when given; route: read */
    const float *gamma, *beta; /* stats */
    float *mean, *rstd, *scale, *shift;      /* stats: written; route and apply: read (fuse: scale, shift, may be NULL) */
    float *running_mean, *running_var;       /* stats: updated when given */
    float *sums;               /* (2, C): route: written; apply: read */
    float *dgamma, *dbeta;     /* route: added to */
    int32_t B, H, W, C;        /* of u3 */
    float eps, momentum;
    float *workspace;          /* stats and route */
    uint64_t workspace_floats;
} somi_scalseq_desc;
size_t somi_scalseq_desc_bytes(void);
size_t somi_scalseq_workspace_floats(int B, int H, int W, int C);
int somi_scalseq_stats_f32(const somi_scalseq_desc *d, somi_stream_t stream);
int somi_scalseq_fuse_nhwc_f32(const somi_scalseq_desc *d, somi_stream_t stream);
int somi_scalseq_route_bwd_nhwc_f32(const somi_scalseq_desc *d, somi_stream_t stream);
int somi_scalseq_apply_bwd_f32(const somi_scalseq_desc *d, somi_stream_t stream);

/* attention_model: the ECA gate on (B, C) vectors and the mix t = x1 gate + x2 in front of the coordinate-attention passes.
 * somi_eca_gate_f32:      gate[b,c] = sigmoid(sum_j w[j] avg[b, c + j - k / 2]), zero-padded; k odd, at most 9.
 * somi_eca_gate_bwd_f32:  dz = dgate gate (1 - gate);  davg[b,c] = sum_j w[j] dz[b, c - j + k / 2];  dw[j] = sum_{b,c} dz[b,c] avg[b, c + j - k / 2],
 *                         written, one workgroup in a fixed order.
 * mix + means (somi_asf_mix_means_nhwc_f32):   t = x1 gate[b,c] + x2 written, and pool (B, H + W, .) = the row means (rows [0, H)) and column
 *                         means (rows [H, H + W)) of t in the same pass (somi_coordatt_means with the mix in front; same partial layout).
 * mix bwd sums (somi_asf_mix_bwd_sums_nhwc_f32):  `t` holds dt (read): ds[b,c] = sum over the pixels of dt x1, partials in `workspace`, then in order.
 * mix bwd input (somi_asf_mix_bwd_input_nhwc_f32): dx1 = dt gate + davg / (H W), written, or added with `accumulate`.  dx2 is dt itself. */
typedef struct somi_asfatt_desc {
    somi_slice x1, x2;         /* mix: read; bwd sums: x1 read */
    somi_slice t;              /* mix: written; both backward passes: dt, read */
    somi_slice pool;           /* mix: (B, H + W, .) written */
    somi_slice dx1;            /* bwd input */
    const float *gate;         /* (B, C): mix and bwd input */
    float *ds;                 /* (B, C): bwd sums, written */
    const float *davg;         /* (B, C): bwd input */
    int32_t B, H, W, C;
    int32_t accumulate;        /* bwd input: add to what dx1 holds */
    float *workspace;          /* mix and bwd sums */
    uint64_t workspace_floats;
} somi_asfatt_desc;
size_t somi_asfatt_desc_bytes(void);
size_t somi_asfatt_workspace_floats(int B, int H, int W, int C);
int somi_eca_gate_f32(const float *avg, const float *w, int k, float *gate, int B, int C, somi_stream_t stream);
int somi_eca_gate_bwd_f32(const float *avg, const float *w, int k, const float *gate, const float *dgate, float *davg, float *dw, int B, int C,
                          somi_stream_t stream);
int somi_asf_mix_means_nhwc_f32(const somi_asfatt_desc *d, somi_stream_t stream);
int somi_asf_mix_bwd_sums_nhwc_f32(const somi_asfatt_desc *d, somi_stream_t stream);
int somi_asf_mix_bwd_input_nhwc_f32(const somi_asfatt_desc *d, somi_stream_t stream);

/* Slim-neck GSConv (models/common.py:9586-9610; gsconv.hip).  With Ch = c2 / 2 (a multiple of 4), x1 = cv1(x) and x_2 = cv2_2(cv2_1(x1)), two
 * stacked depthwise 3x3 Conv blocks, the module returns the fixed channel de-interleave of s = cat(x1, x_2): out[o] = s[2 o] for o < Ch and
 * s[2 (o - Ch) + 1] otherwise (not channel_shuffle(groups=2), which interleaves).  A source quad J of s (channels [4 J, 4 J + 4), J < Ch / 2)
 * therefore lands as two float2: its even channels at out[2 J, 2 J + 2), its odd ones at out[Ch + 2 J, Ch + 2 J + 2).  All three entries walk
 * source quads that way, so no width has a special case.  `out` / `dout` / `residual` are slices of width 2 Ch, the others of width Ch.  fp32,
 * deterministic (no atomics), no workspace.
 *
 * tail (somi_gs_tail_nhwc_f32), inference: reads x1 once per tile and writes the whole module output,
 *   t = act(dw1(x1) + b1) inside the image and ZERO outside it (cv2_2 pads its input with zeros; evaluating dw1 on the padded x1 there would give
 *   act(b1)), x_2 = act(dw2(t) + b2), out = shuffle(x1, x_2) [+ residual].  w1 / w2: the depthwise weights with BatchNorm folded, [9][w_cs]
 *   (pack_gconv_weight), w_cs % 4 == 0, w_cs >= Ch; b1 / b2: Ch floats; all 16-byte aligned.  One workgroup owns 16 x 16 pixels x 4 quads (8 x 16
 *   pixels x 8 quads from Ch = 32 up): x1 with a 2-pixel halo and t with a 1-pixel halo live in LDS, nothing between x1 and out reaches memory.
 *   out must not overlap x1.
 * shuffle (somi_gs_shuffle_affine_act_nhwc_f32), training forward: out = shuffle(z1, act(y2 * scale + shift)) [+ residual]; z1 = cv1's activated
 *   output, y2 = cv2_2's raw conv output, scale / shift its BatchNorm's (Ch floats each, 16-byte aligned; both NULL: the identity).
 * unshuffle (somi_gs_unshuffle_nhwc_f32), training backward: d1[s] / d2[s] = dout[where s went], the exact inverse permutation.
 * The two streaming entries walk somi_gs_tiles_per_workgroup(npix, Ch) pixel tiles per workgroup (host arithmetic; 0 for sizes they refuse). */
int somi_gs_tiles_per_workgroup(long npix, int Ch);
int somi_gs_tail_nhwc_f32(somi_slice x1, const float *w1, const float *b1, const float *w2, const float *b2, int w_cs, int act, somi_slice out,
                          somi_slice residual, int B, int H, int W, int Ch, somi_stream_t stream);
int somi_gs_shuffle_affine_act_nhwc_f32(somi_slice z1, somi_slice y2, const float *scale, const float *shift, int act, somi_slice out,
                                        somi_slice residual, long npix, int Ch, somi_stream_t stream);
int somi_gs_unshuffle_nhwc_f32(somi_slice dout, somi_slice d1, somi_slice d2, long npix, int Ch, somi_stream_t stream);

/* BiFPN fusion (models/common.py:3695-3704) with the preceding nn.Upsample(2,'nearest') folded in:
 * y = sum_i wn[i] * src_i, where source i is read at (h>>up[i], w>>up[i]).  wn = w / (sum swish(w) + eps) is computed
 * inside the kernel from the raw parameter w_dev (n_in floats on the device; no host copy of it is needed).
 * n_in in {2,3}; all sources C channels, contiguous NHWC.  src_host / up_host are host arrays of n_in entries. */
int somi_bifpn_nhwc_f32(const float *const *src_host, const int *up_host, const float *w_dev, float eps, int n_in, float *y,
                        int B, int H, int W, int C, somi_stream_t stream);

/* Global average + max pool over H*W of a channel slice: out_avg[b][c], out_max[b][c]
 * (ChannelAttentionModule models/common.py:355-357; also GAP for ODConv :4558 and SEAM :8483).
 * partial workspace: 2*B*nchunk*C floats with nchunk = somi_pool_nchunk(H*W). out_max may be NULL. */
int somi_pool_nchunk(int HW);
int somi_global_pool_nhwc_f32(const float *x, int x_cs, int x_coff, int B, int HW, int C, float *out_avg,
                              float *out_max, float *workspace, somi_stream_t stream);
/* The average pool of act(x), optionally followed by a per-channel affine map: out_avg[b][c] = post_scale[c] * mean_p act(x[b,p,c]) + post_shift[c]
 * (post_scale / post_shift NULL: the plain mean).  SEAM's squeeze (models/common.py:8483) reads BatchNorm(GELU(u)) only through its global average,
 * which is that expression with the BatchNorm's scale / shift: the normalised tensor is never written.  Same workspace. */
int somi_global_pool_act_nhwc_f32(const float *x, int x_cs, int x_coff, int B, int HW, int C, int act, const float *post_scale,
                                  const float *post_shift, float *out_avg, float *workspace, somi_stream_t stream);
/* z = silu(x * scale + shift) (the Conv block's BatchNorm + SiLU, as somi_chan_affine_act_nhwc_f32 with act = SILU, order = 0) AND the global
 * average / max pools of z per (image, channel) in the same pass - what a channel attention right behind the block would otherwise re-read z for
 * (models/common.py:339-358).  C / 4 must divide 256 or be a multiple of it (somi_affine_silu_pool_rows returns 0 otherwise: use the two
 * separate entries).  workspace: 2 * B * somi_affine_silu_pool_rows(B, HW, C) * C floats. */
int somi_affine_silu_pool_rows(int B, int HW, int C);
int somi_affine_silu_pool_nhwc_f32(const float *x, int x_cs, int x_coff, const float *scale, const float *shift, float *z, int z_cs, int z_coff,
                                   int B, int HW, int C, float *out_avg, float *out_max, float *workspace, somi_stream_t stream);

/* Tiny per-sample MLP heads (host picks the recipe):
 *  mode 0 (CBAM channel attention, models/common.py:355-358):
 *        out[b] = sigmoid( W2 relu(W1 avg[b] + b1) + b2 + W2 relu(W1 max[b] + b1) + b2 )
 *  mode 1 (SEAM, models/common.py:8484-8487): out[b] = exp( sigmoid( W2 relu(W1 avg[b]) ) )   (no biases)
 * W1 [mid][C], W2 [C][mid]. */
int somi_attn_mlp_f32(int mode, const float *avg, const float *mx, const float *W1, const float *b1, const float *W2,
                      const float *b2, float *out, int B, int C, int mid, somi_stream_t stream);

/* Per-pixel channel statistics of x*ca: stats[b,h,w,0] = mean_c(x*ca), stats[...,1] = max_c(x*ca)
 * (SpatialAttentionModule models/common.py:400-402 applied to `channel_attention(x)*x`, :686-688). */
int somi_chan_stats_nhwc_f32(const float *x, int x_cs, int x_coff, const float *ca, float *stats, int B, int HW, int C,
                             somi_stream_t stream);

/* k x k conv 2->1 channels + bias + sigmoid on the stats map -> sa[b,h,w] (models/common.py:396,403). w is [k][k][2]. */
int somi_spatial_attn_f32(const float *stats, const float *w, const float *bias /* device, 1 value */, float *sa, int B, int H, int W, int k,
                          somi_stream_t stream);

/* CBAM apply in one pass: sa = sigmoid(conv_kxk(stats) + bias); y = x * ca[b][c] * sa[b,h,w] (models/common.py:686-688:
 * `out = channel_attention(x2) * x2; out = spatial_attention(out) * out`).  x / y are channel slices; in place allowed. */
int somi_cbam_apply_nhwc_f32(const float *x, int x_cs, int x_coff, const float *ca, const float *stats, const float *w,
                             const float *bias /* device, 1 value */, float *y, int y_cs, int y_coff, int B, int H, int W, int C, int k,
                             somi_stream_t stream);

/* y = x * s[b][c] (SEAM output x*exp(fc), models/common.py:8489-8490; also materialised CBAM scaling). In place allowed. */
int somi_scale_channels_nhwc_f32(const float *x, const float *s, const float *pix, float *y, int B, int HW, int C,
                                 somi_stream_t stream);

/* ODConv attention + per-sample weight synthesis (models/common.py:4557-4590):
 *  z = relu(bn(fc(gap)))  [bn folded into fc_w/fc_b by the host; skipped when B==1 as the reference does]
 *  a_f = sigmoid(Wf z + bf) [Cout], a_s = sigmoid(Ws z + bs) [kk], a_c = sigmoid(Wc z + bc) [Cin], a_w = softmax(Ww z + bw) [K]
 *  wout[b][n][(t)*Cin_pad + c] = a_f[n] a_s[t] a_c[c] sum_K a_w[K] Wk[K][n][t][c]   (zero in padded c)
 *  bout[b][n] = sum_K a_w[K] bias[K][n]
 * then conv BN (eval) is folded: wout *= bn_scale[n]; bout = bout*bn_scale[n] + bn_shift[n].
 * Wk is [K][Cout][kk][Cin_pad]. attn workspace: B*(hid + Cout + kk + Cin + K) floats. */
int somi_odconv_weights_f32(const float *gap, const float *fc_w, const float *fc_b, const float *Wf, const float *bf,
                            const float *Ws, const float *bs, const float *Wc, const float *bc, const float *Ww,
                            const float *bw, const float *Wk, const float *biask, const float *bn_scale,
                            const float *bn_shift, float *wout, float *bout, float *workspace, int B, int Cin,
                            int Cin_pad, int Cout, int kk, int K, int hid, somi_stream_t stream);

/* Detection decode (DecoupledDetect.forward eval branch, models/yolo.py:943-961 + Decouple interleave :1073):
 * box (B,ny,nx,box_cs>=na*5) and cls (B,ny,nx,cls_cs>=na*nc) head outputs ->
 *   raw (B,na,ny,nx,no)            [x[i] of the reference, always written if non-NULL]
 *   z   (B,total,no) rows [row_off, row_off+na*ny*nx): sigmoid, xy=(s*2-0.5+grid)*stride, wh=(s*2)^2*anchor_px. */
int somi_detect_decode_f32(const float *box, int box_cs, const float *cls, int cls_cs, const float *anchors_px_host,
                           float stride, float *raw, float *z, int B, int ny, int nx, int na, int nc, int total,
                           int row_off, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode normalisation / activation (nn.BatchNorm2d with batch statistics: models/common.py:64-66 under model.train(),
 * eps 1e-3 / momentum 0.03 from utils/torch_utils.py:165-174; SEAM's act-then-norm stages models/common.py:8454-8466).
 * Tensors are channel slices (cs, coff) of NHWC buffers with npix = B*H*W rows.  order 0: z = act(x*scale+shift) (norm then
 * act); order 1: z = act(x)*scale+shift (act then norm).  Workspaces: bn_stats 2*nchunk*C floats,
 * bn_act_backward 2*nchunk*C + 3*C(+pad to 4) floats, chan_sum 2*nchunk*C floats, nchunk = somi_red_nchunk(npix).
 */
int somi_red_nchunk(long npix);
/* batch mean / biased variance of x per channel -> mean, rstd = 1/sqrt(var+eps), scale = gamma*rstd, shift = beta - mean*scale;
 * running_mean / running_var (optional) updated with `momentum` and the unbiased variance like nn.BatchNorm2d. */
int somi_bn_stats_nhwc_f32(const float *x, int x_cs, int x_coff, long npix, int C, float eps, float momentum,
                           const float *gamma, const float *beta, float *mean, float *rstd, float *scale, float *shift,
                           float *running_mean, float *running_var, float *workspace, somi_stream_t stream);
/* The same statistics of act(x) (enum somi_act) without act(x) ever being stored: SEAM's act-then-norm stages (models/common.py:8455-8457)
 * then are two passes - this one, and somi_chan_affine_act_nhwc_f32 with order 1 - instead of act, statistics, affine. */
int somi_bn_stats_act_nhwc_f32(const float *x, int x_cs, int x_coff, int act, long npix, int C, float eps, float momentum,
                               const float *gamma, const float *beta, float *mean, float *rstd, float *scale, float *shift,
                               float *running_mean, float *running_var, float *workspace, somi_stream_t stream);
/* The same from the partial sums a convolution left behind (somi_conv_desc.stat_sum / stat_sumsq, `rows` rows, taken around
 * running_mean as the pivot when running_mean is given - pass the same pointer as stat_pivot).  workspace: 2*1024*C floats. */
int somi_bn_stats_partials_f32(const float *part_sum, const float *part_sumsq, int rows, long npix, int C, float eps, float momentum,
                               const float *gamma, const float *beta, float *mean, float *rstd, float *scale, float *shift,
                               float *running_mean, float *running_var, float *workspace, somi_stream_t stream);
/* SyncBatchNorm (reference train.py:165-167, torch.nn.SyncBatchNorm.convert_sync_batchnorm under --sync-bn): the statistics of a
 * BatchNorm layer over the batches of ALL ranks.  The library has no communicator: the caller exchanges one small record per layer.
 *   forward   somi_bn_local_sums_f64 -> record [2*C + 1] doubles {mean_r, M2_r = sum (x - mean_r)^2, pixel count} of this rank, from x
 *             or (part_sum != NULL) from a convolution's partial rows (taken around `pivot` there); the record itself is pivot-free,
 *             so ranks whose running means have drifted apart still combine correctly.
 *             all-gather the records ([nranks][2*C + 1]); somi_bn_stats_from_sums_f64 combines them in rank order (parallel-variance
 *             formula in double; identical results on every rank) -> mean / rstd / scale / shift and the running statistics
 *             (unbiased variance over the global count).
 *   backward  somi_bn_act_backward_sums_f64 -> record {sum d, sum d*(v - mean), count}; all-gather; ..._apply_sync_f32 builds the
 *             input gradient from the global sums and ACCUMULATES dgamma / dbeta from the LOCAL ones (the gradient exchange sums them).
 * workspace: max(2*1024*C, 2*somi_red_nchunk(npix)*C) floats (sums), 3*C floats (apply). */
int somi_bn_local_sums_f64(const float *x, int x_cs, int x_coff, long npix, int C, const float *pivot /* or NULL */, const float *part_sum,
                           const float *part_sumsq, int rows, double *sums, float *workspace, somi_stream_t stream);
int somi_bn_stats_from_sums_f64(const double *all_sums, int nranks, int C, float eps, float momentum, const float *gamma, const float *beta,
                                float *mean, float *rstd, float *scale, float *shift, float *running_mean, float *running_var,
                                somi_stream_t stream);
int somi_bn_act_backward_sums_f64(const float *dz, int dz_cs, int dz_coff, const float *x, int x_cs, int x_coff, const float *mean,
                                  const float *scale, const float *shift, int act, int order, long npix, int C, double *sums, float *workspace,
                                  somi_stream_t stream);
int somi_bn_act_backward_apply_sync_f32(const float *dz, int dz_cs, int dz_coff, const float *x, int x_cs, int x_coff, const float *mean,
                                        const float *rstd, const float *scale, const float *shift, int act, int order,
                                        const double *local_sums, const double *all_sums, int nranks, float *dx, int dx_cs, int dx_coff,
                                        float *dgamma, float *dbeta, long npix, int C, float *workspace, somi_stream_t stream);
int somi_chan_affine_act_nhwc_f32(const float *x, int x_cs, int x_coff, const float *scale, const float *shift, int act,
                                  int order, float *z, int z_cs, int z_coff, long npix, int C, const float *residual /* or NULL: added last */,
                                  int res_cs, int res_coff, somi_stream_t stream);
/* gradient of z = [order 0] act(norm(x)) / [order 1] norm(act(x)) w.r.t. x (written to dx, may alias dz), and dgamma / dbeta
 * ACCUMULATED into the given arrays (may be NULL).  batch_stats = 1: statistics were computed from this batch (train);
 * 0: frozen statistics (the norm is a per-channel affine map). */
int somi_bn_act_backward_nhwc_f32(const float *dz, int dz_cs, int dz_coff, const float *x, int x_cs, int x_coff, const float *mean,
                                  const float *rstd, const float *scale, const float *shift, int act, int order,
                                  int batch_stats, float *dx, int dx_cs, int dx_coff, float *dgamma, float *dbeta, long npix,
                                  int C, float *workspace, somi_stream_t stream);
/* The same backward (batch statistics) for the conv in front of a CBAM attention pair (models/common.py:339-358, 671-691), with the gradient of
 * the channel attention's global pools folded in instead of added by a pass of its own (somi_pool_bwd_add_nhwc_f32):
 *   dz_eff[b,p,c] = dz[b,p,c] + davg[b,c] / HW + [p == amaxp[b,c]] * dmax[b,c];   dz is only read.
 * davg, dmax (B,C) float, amaxp (B,C) int32 - the first pixel of each channel's spatial maximum.  dmax and amaxp may both be NULL (no max-pool:
 * SEAM's squeeze, models/common.py:8483-8490), and dz may be NULL when the pooled part is the WHOLE incoming gradient (the tensor is read by a
 * global average pool only: no zero tensor is materialised and read).  workspace: 2 * somi_bn_pooled_rows(B, HW) * C + 3 * round_up(C, 4) floats. */
int somi_bn_pooled_rows(int B, int HW);
int somi_bn_act_backward_pooled_nhwc_f32(const float *dz, int dz_cs, int dz_coff, const float *x, int x_cs, int x_coff, const float *mean,
                                         const float *rstd, const float *scale, const float *shift, int act, int order, const float *davg,
                                         const float *dmax, const int32_t *amaxp, float *dx, int dx_cs, int dx_coff, float *dgamma,
                                         float *dbeta, int B, int HW, int C, float *workspace, somi_stream_t stream);
/* out = a + b on channel slices (residual connections, gradient accumulation); out may alias a or b */
int somi_add_nhwc_f32(const float *a, int a_cs, int a_coff, const float *b, int b_cs, int b_coff, float *out, int o_cs,
                      int o_coff, long npix, int C, somi_stream_t stream);
/* out[c] += sum over pixels of x[p,c] (bias gradients) */
int somi_chan_sum_nhwc_f32(const float *x, int x_cs, int x_coff, long npix, int C, float *out_accumulate, float *workspace,
                           somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the attention pieces (autograd of models/common.py:339-405, 671-691 CBAM; :8483-8490 SEAM squeeze).
 * See yolo-somi_amd/csrc/train_blocks.hip for the derivation.  Per-image reductions use nchunk = somi_img_nchunk(H*W).
 */
int somi_img_nchunk(int HW);
/* A + D: dlogit[p] = (sum_c dt2*t*ca) * sa*(1-sa), amaxc[p] = argmax_c(t*ca), and amaxp[b,c] = first pixel index p with t[b,p,c] == t_max[b,c],
 * where t_max (B,C) is the spatial maximum the forward pooled from the same tensor (somi_global_pool_nhwc_f32's out_max) - the arg-max of the
 * channel attention's max-pool without a pass of its own over t (integer min over the matching pixels: order-independent). */
int somi_cbam_bwd_pixel_argmax_f32(const float *dt2, int d_cs, int d_coff, const float *t, int t_cs, int t_coff, const float *ca,
                                   const float *sa, const float *t_max, float *dlogit, int32_t *amaxc, int32_t *amaxp, int B, int HW, int C,
                                   somi_stream_t stream);
/* B: gradient of sigmoid's argument through the k x k conv: dstats (B,H,W,2); dw and dbias ACCUMULATED; dw_chw = 0: dw laid out [k][k][2] like
 * the forward's packed weight, 1: (2,k,k) - nn.Conv2d(2, 1, k).weight's own layout, so that the parameter's .grad can be the target.
 * workspace: ceil(B*H*W/512) * (2*k*k+1) floats */
int somi_spatial_attn_bwd_f32(const float *dlogit, const float *stats, const float *w, float *dstats, float *dw_accumulate,
                              float *dbias_accumulate, float *workspace, int B, int H, int W, int k, int dw_chw, somi_stream_t stream);
/* Step C INSIDE the BatchNorm + SiLU backward of the bottleneck's first conv (models/common.py:671-691: cv1 = Conv -> BN -> SiLU, then t*ca*sa):
 * d = gradient w.r.t. t*ca*sa, y = cv1's convolution output, t = silu(scale*y + shift) is rebuilt in registers, dt never exists in memory.
 *   reduce: dca[b,c] = sum_p dt1*t (as step C) and, per (image chunk, channel), the separable batch sums of dt*silu'(u) - kept in `workspace`;
 *   (the caller then runs somi_attn_mlp_bwd_f32 on dca -> davg, dmax)
 *   apply:  the BatchNorm backward (batch statistics) of dz = dt + davg/HW + [p == amaxp]*dmax: dx, dgamma / dbeta ACCUMULATED.
 * Same tensors and `workspace` (somi_cbam_bn_bwd_workspace_floats(B,HW,C) floats) for both calls.  amaxp (B,C): first pixel of each channel's spatial
 * maximum (somi_cbam_bwd_pixel_argmax_f32); amaxc, dstats: steps A / B. */
size_t somi_cbam_bn_bwd_workspace_floats(int B, int HW, int C);
int somi_cbam_bn_bwd_reduce_f32(const float *d, int d_cs, int d_coff, const float *y, int y_cs, int y_coff, const float *scale, const float *shift,
                                const float *mean, const float *ca, const float *sa, const float *dstats, const int32_t *amaxc,
                                const int32_t *amaxp, float *dca, float *workspace, int B, int HW, int C, somi_stream_t stream);
int somi_cbam_bn_bwd_apply_f32(const float *d, int d_cs, int d_coff, const float *y, int y_cs, int y_coff, const float *scale, const float *shift,
                               const float *mean, const float *rstd, const float *ca, const float *sa, const float *dstats, const int32_t *amaxc,
                               const int32_t *amaxp, const float *davg, const float *dmax, float *dx, int dx_cs, int dx_coff, float *dgamma,
                               float *dbeta, float *workspace, int B, int HW, int C, somi_stream_t stream);
/* C: dt1 = dt2*sa + dstats0/C + [c==amaxc]*dstats1; dca[b,c] = sum_p dt1*t; dt2 <- dt1*ca (in place).
 * workspace: B*nchunk*C floats */
int somi_cbam_bwd_chan_f32(float *dt2_inout, int d_cs, int d_coff, const float *t, int t_cs, int t_coff, const float *ca,
                           const float *sa, const float *dstats, const int32_t *amaxc, float *dca, float *workspace, int B, int HW,
                           int C, somi_stream_t stream);
/* E: backward of somi_attn_mlp_f32 (same modes); dW1/db1/dW2/db2 ACCUMULATED (db* may be NULL), davg / dmax overwritten.
 *    The sum over samples runs in ascending order (no atomics).  workspace: somi_attn_mlp_bwd_workspace_floats(B, C, mid) floats. */
size_t somi_attn_mlp_bwd_workspace_floats(int B, int C, int mid);
int somi_attn_mlp_bwd_f32(int mode, const float *dout, const float *out, const float *avg, const float *mx, const float *W1,
                          const float *b1, const float *W2, float *dW1, float *db1, float *dW2, float *db2, float *davg,
                          float *dmax, float *workspace, int B, int C, int mid, somi_stream_t stream);
/* F: dt[p,c] += davg[b,c]/HW + [p==amaxp[b,c]]*dmax[b,c]  (dmax / amaxp may be NULL: average pool only) */
int somi_pool_bwd_add_nhwc_f32(float *dt_inout, int d_cs, int d_coff, const float *davg, const float *dmax, const int32_t *amaxp,
                               int B, int HW, int C, somi_stream_t stream);

/* Backward of the remaining layer kernels (train_blocks.hip).
 * detect: d raw (B,na,ny,nx,no) -> d box (B,ny,nx,box_cs), d cls (B,ny,nx,cls_cs) (inverse of the interleave; pads zeroed).
 * sppf:   dbuf slices 1..3 (the gradients of the three chained 5x5 pools y1 = m(x), y2 = m(y1), y3 = m(y2)) are routed back through the chain - each
 *         pool's gradient to the arg-max of its 5x5 window of the previous slice, first maximum in row-major order - and ADDED into slice 0 of dbuf
 *         (gather form, fixed summation order).  Slices 1 and 2 of dbuf hold the chain's intermediate gradients afterwards.  workspace: 3*B*H*W*C bytes;
 *         with buf = NULL it already holds the codes of somi_sppf_pool_codes_nhwc_f32 and no search runs.  SPP's parallel 5 / 9 / 13
 *         pools (models/common.py:1806-1826) give the same values and the same routing except at exact ties inside a window.
 * bifpn:  dsrc_i = wn_i*dout (2x2 sum for an upsampled source, dsrc_i low-res); dw ACCUMULATED incl. the normalisation's chain
 *         rule.  workspace: 3*2048 floats.
 * dwconv: dx (+dx_accumulate), dw [3][3][C] and dbias ACCUMULATED.  workspace: ceil(B*H*W/512)*10*C floats.
 * scale:  y = x*s[b][c]: dx = dout*s, ds[b,c] = sum_p dout*x.  workspace: B*nchunk*C floats. */
int somi_detect_raw_bwd_f32(const float *draw, float *dbox, int box_cs, float *dcls, int cls_cs, int B, int ny, int nx, int na,
                            int nc, somi_stream_t stream);
int somi_sppf_pool_bwd_nhwc_f32(const float *buf, float *dbuf, void *workspace, int B, int H, int W, int C, int cs, int x_coff,
                                somi_stream_t stream);   /* workspace: 3*B*H*W*C bytes (arg-max codes) */
int somi_bifpn_bwd_nhwc_f32(const float *const *src_host, float *const *dsrc_host, const int *up_host, const float *w_dev,
                            float eps, int n_in, const float *dout, float *dw_accumulate, float *workspace, int B, int H,
                            int W, int C, somi_stream_t stream);
size_t somi_dwconv3x3_bwd_workspace_floats(int B, int W, int C);   /* floats of `workspace` below; C/4 must divide 256 */
int somi_dwconv3x3_bwd_nhwc_f32(const float *dy, const float *x, const float *w, float *dx, const float *dx_accumulate,
                                float *dw_accumulate, float *dbias_accumulate, float *workspace, int B, int H, int W, int C,
                                somi_stream_t stream);
int somi_scale_channels_bwd_nhwc_f32(const float *dout, const float *x, const float *s, float *dx, float *ds, float *workspace, int B,
                                     int HW, int C, somi_stream_t stream);

/* Training path of ODConv (models/common.py:4495-4624), see train_odconv.hip.
 * linear:     y[b][y_off+o] = act(x[b] . W[o] + bias[o]); act = enum somi_act or 5 = softmax over the nout outputs (<= 64).
 * linear_bwd: (dy, y) are slices (ld, off) of one buffer pair; computes d(pre-activation) through `act`, then dW, db ACCUMULATED,
 *             dx (B,nin) written or accumulated.  workspace: B*nout floats.
 * synth:      per-sample weights / biases from an attention buffer laid out [a_f(Cout) | a_s(kk) | a_c(Cin) | a_w(K)] per sample.
 * synth_bwd:  from dW_b (B,Cout,kk*Cin_pad) and dbias_b (B,Cout): dWk, dbiask ACCUMULATED (float atomics), dattn (same layout) written. */
int somi_linear_f32(const float *x, int ldx, const float *W, const float *bias, int act, float *y, int ldy, int y_off, int B, int nin,
                    int nout, somi_stream_t stream);
int somi_linear_bwd_f32(const float *x, int ldx, const float *W, const float *dy, const float *y, int ld, int off, int act, float *dW,
                        float *db, float *dx, int ldx_out, int dx_accumulate, float *workspace, int B, int nin, int nout,
                        somi_stream_t stream);
int somi_odconv_synth_f32(const float *attn, const float *Wk, const float *biask, float *wout, float *bout, int B, int Cin, int Cin_pad,
                          int Cout, int kk, int K, somi_stream_t stream);
/* dWk / dbiask ACCUMULATED, dattn overwritten; fixed summation orders (no atomics).
 * workspace: somi_odconv_synth_bwd_workspace_floats(B, Cin, Cout, kk, K) floats. */
size_t somi_odconv_synth_bwd_workspace_floats(int B, int Cin, int Cout, int kk, int K);
int somi_odconv_synth_bwd_f32(const float *dWb, const float *attn, const float *Wk, const float *biask, const float *dbias_b, float *dWk,
                              float *dbiask, float *dattn, float *workspace, int B, int Cin, int Cin_pad, int Cout, int kk, int K,
                              somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam step (train.py:134-140,271) fused with the ModelEMA update
 * (utils/torch_utils.py:335-345) over one flat, 16 B-aligned parameter segment:
 *   g' = grad + weight_decay*param; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 *   param -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps);   ema = d*ema + (1-d)*param  (ema may be NULL)
 * axpby: y = a*y + b*x (EMA of the BN running statistics). */
int somi_adam_ema_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema, long n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int step, float ema_decay, somi_stream_t stream);
/* The other optimizer branch of train.py:136-138: torch.optim.SGD(momentum, nesterov=True) + the same EMA update in one pass
 * (g' = g + weight_decay*p; buf = step == 1 ? g' : momentum*buf + g'; p -= lr*(g' + momentum*buf)).  momentum_buf plays exp_avg's role. */
int somi_sgd_ema_step_f32(float *param, const float *grad, float *momentum_buf, float *ema, long n, float lr, float momentum,
                          float weight_decay, int step, float ema_decay, somi_stream_t stream);
int somi_axpby_f32(float *y, const float *x, long n, float a, float b, somi_stream_t stream);
/* Forward-packed conv weights [Cout][taps][Cin] -> the packing somi_conv2d_dgrad_nhwc_f32 reads, [Cin][taps][Cout].  Run once
 * per optimizer step on the master weights (which the training path keeps in the forward packing). */
int somi_pack_dgrad_weights_f32(const float *w_packed, float *w_dgrad, int Cout, int taps, int Cin, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Grouped / depthwise convolution (Conv with g > 1, DWConv, the GhostConv cheap operation; models/common.py:53-70, 9580-9583, 2001-2011).
 * NHWC fp32; C1 input and C2 output channels in `groups` groups of cin_g = C1/groups and cout_g = C2/groups; k in {1, 3, 5},
 * stride 1 or 2, pad k/2, dilation 1; cin_g <= 16.  Depthwise (cin_g = cout_g = 1) reads float4 quads of channels.
 * Weights are packed [k*k][cin_g][w_cs] (tap-major, output channel fastest, columns >= C2 zero).  Channel slices follow the slice
 * rule above (x and dy are read to their width rounded up to 4).  Deterministic: fixed-order reductions, no float atomics.  fp32 only (the conv precision switch does not apply).
 *
 * Forward: y[.., y_coff + co] = act(conv + bias) [+ residual] for co < Cw (Cw >= C2, a multiple of 4; channels C2..Cw come out zero
 * when their weights and bias are).  stat_sum / stat_sumsq (optional, [somi_gconv2d_stat_rows][Cw] each): per-channel partial sums of
 * (y - stat_pivot) and its square, the format of the dense conv epilogue's (somi_conv_desc.stat_sum), for somi_bn_stats_partials_f32. */
int somi_gconv2d_stat_rows(int B, int Ho, int Wo, int Cw);
int somi_gconv2d_nhwc_f32(const float *x, int x_cs, int x_coff, int B, int H, int W, int C1, const float *w, int w_cs, const float *bias,
                          int groups, int k, int stride, float *y, int y_cs, int y_coff, int C2, int Cw, int act, const float *residual,
                          int res_cs, int res_coff, float *stat_sum, float *stat_sumsq, const float *stat_pivot, somi_stream_t stream);
/* Data gradient: dx[.., dx_coff + ci] = conv^T(dy) [+ acc1] [+ acc2] for ci < Cx (Cx >= C1, a multiple of 4); acc1 may be dx itself
 * (accumulate in place).  w is the forward packing. */
int somi_gconv2d_dgrad_nhwc_f32(const float *dy, int dy_cs, int dy_coff, int B, int Ho, int Wo, int C2, const float *w, int w_cs, int groups,
                                int k, int stride, float *dx, int dx_cs, int dx_coff, int H, int W, int C1, int Cx, const float *acc1,
                                int acc1_cs, int acc1_coff, const float *acc2, int acc2_cs, int acc2_coff, somi_stream_t stream);
/* Weight gradient into dw (C2, cin_g, k, k) - the nn.Conv2d layout - written, or added to when accumulate != 0. */
size_t somi_gconv2d_wgrad_workspace_floats(int B, int Ho, int Wo, int C2, int cin_g, int k);
int somi_gconv2d_wgrad_nhwc_f32(const float *x, int x_cs, int x_coff, int B, int H, int W, int C1, const float *dy, int dy_cs, int dy_coff,
                                int Ho, int Wo, int C2, int groups, int k, int stride, float *dw, int accumulate, float *workspace,
                                size_t workspace_floats, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Large-kernel depthwise convolution (ConvNextBlock's 7x7, models/common.py:6755; ConvMix's 9x9, :7153; dwlk.hip).  NHWC fp32, C channels
 * (any multiple of 4) in and out, k in {7, 9}, stride 1, pad k/2, dilation 1.  Weights are tap-major [k*k][w_cs] (pack_gconv_weight's layout
 * at cin_g = 1; w_cs % 4 == 0, w_cs >= C).  Slices are taken by value (somi_slice) and follow the slice rule above, every slice C wide; an
 * optional slice is absent when its p is NULL.  A lane owns a channel quad of a
 * strip of somi_dwlk_strip_length() adjacent outputs of one image row and holds one row of k taps at a time; a workgroup walks
 * somi_dwlk_strips_per_workgroup(B, H, W, C, wgrad) rows of strips (host arithmetic; wgrad != 0: the weight gradient's plan; 0 for sizes the
 * family refuses).  Deterministic: fixed-order reductions, no float atomics.  fp32 only.  Refused before any launch: SOMI_ENOTIMPL for another
 * k, C % 4 != 0, an activation other than none / gelu, a tensor of more than 2^30 floats (B * H * W * its channel stride); SOMI_EINVAL for
 * null or misaligned pointers and slices that break the slice rule; SOMI_EWORKSPACE for a short workspace.
 *
 * Forward: y = post_scale * act(conv + bias) + post_shift [+ residual], act in {SOMI_ACT_NONE, SOMI_ACT_GELU}; bias, post_scale, post_shift
 * (C floats each, 16-byte aligned) and residual are optional, each on its own.  y must not overlap x.
 * stat_sum / stat_sumsq (optional, [somi_dwlk_stat_rows][C] each): per-channel partial sums of (act(conv + bias) - stat_pivot) and its
 * square - what a BatchNorm behind the activation normalises -, in the format somi_bn_stats_partials_f32 reads.  When statistics are asked for,
 * the tensor WRITTEN is the pre-activation conv + bias: the GELU backward needs it, and the BatchNorm pass applies the activation.
 * post_scale, post_shift and residual must then be NULL. */
int somi_dwlk_strip_length(void);
int somi_dwlk_strips_per_workgroup(int B, int H, int W, int C, int wgrad);
int somi_dwlk_stat_rows(int B, int H, int W, int C);
int somi_dwlk_nhwc_f32(somi_slice x, const float *w, int w_cs, const float *bias, int k, int act, const float *post_scale, const float *post_shift,
                       somi_slice y, somi_slice residual, int B, int H, int W, int C, float *stat_sum, float *stat_sumsq, const float *stat_pivot,
                       somi_stream_t stream);
/* Data gradient: dx = conv^T(dy) [+ acc1] [+ acc2], the forward's stencil with the taps mirrored; acc1 may be dx itself (accumulate in
 * place).  w is the forward packing. */
int somi_dwlk_dgrad_nhwc_f32(somi_slice dy, const float *w, int w_cs, int k, somi_slice dx, somi_slice acc1, somi_slice acc2, int B, int H, int W,
                             int C, somi_stream_t stream);
/* Weight and bias gradient from one pass over x and dy: dw (C, 1, k, k) - the nn.Conv2d layout - and db (C; NULL: not wanted) = the
 * per-channel sum of dy, both written, or added to when accumulate != 0.  A lane keeps k accumulators, one tap row at a time; one partial row
 * per workgroup goes to the workspace (somi_dwlk_wgrad_workspace_floats, 16-byte aligned) and a second kernel adds the rows in a fixed order. */
size_t somi_dwlk_wgrad_workspace_floats(int B, int H, int W, int C, int k);
int somi_dwlk_wgrad_nhwc_f32(somi_slice x, somi_slice dy, int B, int H, int W, int C, int k, float *dw, float *db, int accumulate, float *workspace,
                             size_t workspace_floats, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PSA multi-head spatial self-attention (AttentionPSA, models/common.py:7203-7230; yolov10.yaml).  NHWC fp32, key_dim 32 and head_dim
 * 64 fixed (scale 32^-0.5).  q, k and v are read in place from the qkv Conv's output: per pixel (row stride qkv_cs), head h's channels
 * qkv_coff + h*128 + [0,32) are q, + [32,64) k and + [64,128) v.  N = H*W tokens per image, any N >= 1.  Slices of heads*128 (qkv, dqkv)
 * and heads*64 (o, dout) channels under the slice rule above.  The N x N matrix never reaches memory.  Deterministic: fixed-order sums, no float atomics.  fp32 only.
 *
 * Forward: o[.., o_coff + h*64 + d] = sum_j softmax_j(q.k_j * scale) v_j[d].  lse (optional, (B, heads, N)): the natural-log
 * log-sum-exp of each row's scaled scores, for the backward pass.  v_out (optional): v written contiguously as (B, N, heads*64),
 * channel h*64 + d - the input of the depthwise pe Conv. */
int somi_psa_attention_f32(const float *qkv, int qkv_cs, int qkv_coff, int B, int N, int heads, float *o, int o_cs, int o_coff,
                           float *lse, float *v_out, somi_stream_t stream);
/* Backward: dq, dk, dv written into dqkv's slice (the qkv layout above; every channel of the heads' slice is written).  dv_add
 * (optional, contiguous (B, N, heads*64)) is added to dv.  o and lse are the forward's; workspace holds B*heads*N floats. */
int somi_psa_attention_backward_f32(const float *qkv, int qkv_cs, int qkv_coff, const float *o, int o_cs, int o_coff, const float *dout,
                                    int do_cs, int do_coff, const float *lse, int B, int N, int heads, float *dqkv, int g_cs, int g_coff,
                                    const float *dv_add, float *workspace, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Swin window attention (WindowAttention inside SwinTransformerLayer, models/common.py:1184-1358; C3STR :1632-1637).  fp32, window 8 x 8 and
 * head_dim 32 fixed (scale 32^-0.5): C != heads * 32 is SOMI_ENOTIMPL.  Whole contiguous tensors: qkv and dqkv (B,H,W,3C) as the bias-free qkv
 * Linear wrote it (channel = which * C + head * 32 + d, which = 0 q / 1 k / 2 v), o and dout (B,H,W,C); 16-byte aligned.
 * table: the relative_position_bias_table parameter as stored, (225, heads).  shift: 0 or 4.  region_ids: int32 (Wp, Hp) with Wp, Hp = W, H
 * rounded up to 8 - the reference's img_mask (its frame is transposed: rows run along W), required when shift > 0; scores of token pairs with
 * different ids get -100.  The cyclic shift, the zero padding to the window grid (padding tokens have q = k = v = 0 and still are keys), the
 * window partition and the crop are index arithmetic; neither a rolled / padded / partitioned tensor nor a score matrix reaches memory.
 * Deterministic: fixed-order sums, no float atomics.
 *
 * Forward: lse (optional, somi_swin_attention_lse_floats floats) receives each score row's log-sum-exp for the backward.
 * Backward: dq, dk, dv of every pixel written into dqkv; the table's gradient is ACCUMULATED into dtable_accumulate (225, heads) from
 * per-workgroup partial sums in workspace (somi_swin_attention_bwd_workspace_floats floats), added in a fixed order. */
size_t somi_swin_attention_lse_floats(int B, int H, int W, int heads);
int somi_swin_attention_f32(const float *qkv, const float *table, const int32_t *region_ids, int B, int H, int W, int C, int heads, int shift,
                            float *o, float *lse, somi_stream_t stream);
size_t somi_swin_attention_bwd_workspace_floats(int B, int H, int W, int heads);
int somi_swin_attention_backward_f32(const float *qkv, const float *table, const int32_t *region_ids, const float *dout, const float *lse,
                                     int B, int H, int W, int C, int heads, int shift, float *dqkv, float *dtable_accumulate,
                                     float *workspace, somi_stream_t stream);
/* Backward of a plain LayerNorm over C (no activation behind it: norm1 / norm2 of SwinTransformerLayer), contiguous (npix, C): du from dy,
 * `add` (optional, (npix, C)) added to du - the gradient of the residual branch around the norm; dgamma / dbeta are ACCUMULATED, in a fixed
 * order.  workspace: somi_layernorm_bwd_workspace_floats(npix, C) floats.  And the backward of an exact GELU over n = 4k contiguous floats:
 * du = dy * gelu'(u) (Mlp's activation, :1157; du may alias dy). */
size_t somi_layernorm_bwd_workspace_floats(long npix, int C);
int somi_layernorm_bwd_nhwc_f32(const float *u, const float *gamma, float eps, const float *dy, const float *add, float *du,
                                float *dgamma_accumulate, float *dbeta_accumulate, float *workspace, long npix, int C, somi_stream_t stream);
int somi_gelu_bwd_f32(const float *u, const float *dy, float *du, long n, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Stock YOLOv5 module set (north_star "CSP/Darknet backbone, PANet/FPN neck, anchor-based detection head"; BASELINE configs[0]).
 * Bottleneck / C3 / SPP (models/common.py:1494-1509,1541-1565,1806-1826) are compositions of the convolution entry points above
 * (C3's torch.cat never materialises: cv2 and the last bottleneck write the two halves of cv3's input; SPP's parallel 5/9/13
 * pools equal SPPF's chained 5x5 pools exactly and share somi_sppf_pool_nhwc_f32).  What needs kernels of its own:
 *
 * somi_resample_slice_nhwc_f32 - `Concat` (models/common.py:2085-2097) of inputs that cannot be produced in place, with
 *   `nn.Upsample(None, 2, 'nearest')` folded into the copy.
 *     reduce = 0:  dst[b, h, w, dst_coff + c] = src[b, h >> up, w >> up, src_coff + c]      src (B,Hs,Ws,src_cs) -> dst (B,Hs<<up,Ws<<up,dst_cs)
 *     reduce = 1:  dst[b, h, w, dst_coff + c] (+)= sum_{i,j < 2^up} src[b, (h<<up)+i, (w<<up)+j, src_coff + c]   (the adjoint; fixed order)
 *   C is a multiple of 4; both slices follow the slice rule above.
 * somi_space_to_depth_nhwc_f32 - `Focus` (models/common.py:1996): y[b,h,w,q*C+c] = x[b, 2h+(q&1), 2w+(q>>1), c], q = 0..3;
 *   inverse = 1: x is the gradient in y's layout (B,Ho,Wo,x_cs), y receives the gradient in the image layout (B,2Ho,2Wo,y_cs).
 * somi_detect_plain_decode_f32 - `Detect.forward` (models/yolo.py:66-98): t (B,ny,nx,t_cs >= na*no) = the level's 1x1 conv output ->
 *   raw (B,na,ny,nx,no) and, if z != NULL, rows [row_off, row_off + na*ny*nx) of z (B,total,no):
 *   xy = (2*sigmoid - 0.5 + cell)*stride (that operation order), wh = (2*sigmoid)^2 * anchors_px, rest sigmoid.
 * somi_detect_plain_raw_bwd_f32 - the adjoint of the view/permute: d raw -> d t (pad channels zeroed). */
int somi_resample_slice_nhwc_f32(const float *src, int src_cs, int src_coff, float *dst, int dst_cs, int dst_coff, int B, int Hs,
                                 int Ws, int C, int up, int reduce, int accumulate, somi_stream_t stream);
int somi_space_to_depth_nhwc_f32(const float *x, int x_cs, int x_coff, float *y, int y_cs, int y_coff, int B, int Ho, int Wo, int C,
                                 int inverse, somi_stream_t stream);
int somi_detect_plain_decode_f32(const float *t, int t_cs, const float *anchors_px_host, float stride, float *raw, float *z, int B,
                                 int ny, int nx, int na, int nc, int total, int row_off, somi_stream_t stream);
int somi_detect_plain_raw_bwd_f32(const float *draw, float *dt, int t_cs, int B, int ny, int nx, int na, int nc, somi_stream_t stream);

/* Test-time augmentation, `Model._forward_augment` (models/yolo.py:1253-1267).
 * somi_tta_resample_nhwc4_f32: `scale_img(x.flip(3) if flip_lr else x, ratio, gs)` (utils/torch_utils.py:270-282) on the ingested image
 *   x (B,H,W,4) -> y (B,Hp,Wp,4): bilinear resize to (Hs,Ws) = (int(H*ratio), int(W*ratio)) with torch's align_corners=False arithmetic,
 *   the rest up to (Hp,Wp) = the next stride multiples filled with `pad` (0.447); channels >= `channels` stay zero.
 * somi_tta_descale_f32: `_descale_pred` (:1292-1308) in place on z (rows, no): xywh /= scale, x = img_w - x after a left-right flip. */
int somi_tta_resample_nhwc4_f32(const float *x, float *y, int B, int H, int W, int Hs, int Ws, int Hp, int Wp, int flip_lr, float pad,
                                int channels, somi_stream_t stream);
int somi_tta_descale_f32(float *z, long rows, int no, float scale, int flip_lr, float img_w, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Post-processing: batched NMS (utils/general.py:629-711 incl. the torchvision.ops.nms core at :694).
 * pred (B,n,5+nc) decoded.  Output: det (B,max_det,6) [x1,y1,x2,y2,conf,cls], count (B) int32.
 * Selection is bit-exact with the oracle: candidates in prediction order (row-major over (box, class) for
 * multi_label), stable sort by descending score, greedy suppression with IoU > iou_thres, class offset 4096.
 * classes_mask: HOST pointer to ceil(nc/64) 64-bit words, bit (c % 64) of word c/64 set = keep class c (the `classes` argument,
 * general.py:676-677); NULL = no filter.  nc <= 1024.
 * workspace bytes: somi_nms_workspace_bytes(B, n, nc, multi_label).
 */
size_t somi_nms_workspace_bytes(int B, int n, int nc, int multi_label);
int somi_nms_f32(const float *pred, int B, int n, int nc, float conf_thres, float iou_thres, int multi_label,
                 int agnostic, const uint64_t *classes_mask, int max_det, float *det, int32_t *count, void *workspace,
                 size_t workspace_bytes, somi_stream_t stream);

/* The reference's other selection rules (utils/general.py).  Candidate generation, the top-30000 cut and the stable descending sort are
 * those of somi_nms_f32; `mode` picks what runs on the sorted candidates:
 *   SOMI_NMS_IOU                   the torchvision rule; with merge = 0 the call is somi_nms_f32, bit for bit.
 *   SOMI_NMS_GIOU .. SOMI_NMS_SIOU `NMS(boxes, scores, iou_thres, class_nms)` (:925-951): greedy, candidate j is suppressed by an earlier
 *                                  kept box i iff !(bbox_iou(box_i, box_j, <mode>=True) <= iou_thres) (utils/metrics.py:490-579, alpha = 1,
 *                                  eps = 1e-7; a NaN suppresses).  GIoU / DIoU / EIoU reproduce the CPU's fp32 bits; CIoU / SIoU go
 *                                  through atan / asin / cos / exp and agree to a few roundings of the metric.
 *   SOMI_NMS_SOFT                  `soft_nms` (:834-862, the alternative at :695) on the sorted candidates: keep the current box with its
 *                                  score as it stands, multiply every live score whose box_iou_for_nms(cur, j, CIoU=True) (:868-892)
 *                                  exceeds iou_thres by exp(-m*m/sigma), drop what is not > score_threshold, go on with the highest live
 *                                  score (an exact tie: the lowest index), at most max_det picks.  det rows carry the decayed scores.
 *                                  Unlike the reference, whose loop leaves with one candidate in hand, the last candidate is kept.
 *   merge != 0                     merge-NMS (:698-704) after the max_det cut, for images with 1 < candidates < 3000: each kept box
 *                                  becomes the score-weighted mean of the candidates whose plain IoU with it exceeds iou_thres (summed in
 *                                  a fixed order), and rows whose cluster is the box alone are dropped (`redundant`).  Not with SOFT.
 * sigma and score_threshold are read by SOMI_NMS_SOFT only (the reference's defaults: 0.5, 0.25).
 * somi_nms_boxes_f32 is the standalone form, `NMS()` / `soft_nms()` on boxes (n,4) xyxy (16-byte aligned) and scores (n), n <= 30000:
 * keep (n) int64 receives the kept indices (greedy modes: descending score, ties in index order; SOFT: pick order, candidates taken in
 * the given order with index 0 first, scores decayed in place), count (1) int32 how many.
 * workspace bytes: somi_nms_ex_workspace_bytes(B, n, nc, multi_label, mode, merge), somi_nms_boxes_workspace_bytes(n). */
enum { SOMI_NMS_IOU = 0, SOMI_NMS_GIOU = 1, SOMI_NMS_DIOU = 2, SOMI_NMS_CIOU = 3, SOMI_NMS_EIOU = 4, SOMI_NMS_SIOU = 5, SOMI_NMS_SOFT = 6 };
size_t somi_nms_ex_workspace_bytes(int B, int n, int nc, int multi_label, int mode, int merge);
int somi_nms_ex_f32(const float *pred, int B, int n, int nc, float conf_thres, float iou_thres, int multi_label, int agnostic,
                    const uint64_t *classes_mask, int max_det, int mode, int merge, float sigma, float score_threshold, float *det,
                    int32_t *count, void *workspace, size_t workspace_bytes, somi_stream_t stream);
size_t somi_nms_boxes_workspace_bytes(int n);
int somi_nms_boxes_f32(const float *boxes, float *scores, int n, int mode, float iou_thres, float sigma, float score_threshold,
                       int64_t *keep, int32_t *count, void *workspace, size_t workspace_bytes, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss: ComputeLoss.__call__ + build_targets (utils/loss.py:142-262) with CIoU (utils/metrics.py:476-518).
 * p[l] (B,na,ny_l,nx_l,no) for l < nl<=4; targets (nt,6) [img,cls,x,y,w,h]; anchors (nl,na,2) in grid units.
 * out[0..3] = total*bs, lbox, lobj, lcls (already multiplied by the hyp gains, like loss_items).
 * grad[l] (optional, may be NULL): d(out[0])/d p[l], fully overwritten.  Cells hit by several targets sum their entries in
 * ascending (level, anchor, target, offset) order: value and gradient are run-to-run bit-identical.
 * workspace bytes: somi_loss_workspace_bytes(B, na, nl, ny[], nx[], nt).
 */
typedef struct somi_loss_desc {
    const float *p[4];
    float *grad[4];
    int32_t ny[4], nx[4];
    int32_t nl, na, nc, B, nt;
    const float *targets;
    const float *anchors;
    float balance[4];
    float box_gain, obj_gain, cls_gain, cls_pw, obj_pw, anchor_t, cp, cn, gr;
    float fl_gamma;     /* hyp['fl_gamma']: > 0 wraps both BCE terms in FocalLoss(gamma, alpha 0.25) (utils/loss.py:125-127,35-60) */
    int32_t slide;      /* hyp['slide_ratio'] > 0: SlideLoss around them (:129-131,378-402), weighted by the level's mean IoU */
    float nwd_ratio;    /* 0, or iou_ratio = 0.5 when hyp['nwdloss'] > 0: box term (1-r)(1-CIoU) + r(1-NWD) (:148,162-169) */
    float nwd_constant; /* 12.8 = wasserstein_loss (utils/metrics.py:341); 2.5 = wasserstein under hyp['shapeloss'] > 0 (:373, its shape
                         * weights are 1 at the scale1 = 0 the loss calls it with) */
} somi_loss_desc;

size_t somi_loss_workspace_bytes(const somi_loss_desc *d);
/* out8: 8 device floats = {loss * B, lbox, lobj, lcls, obji[0..3]}; obji[l] = the level's mean objectness BCE before `balance`, the value
 * ComputeLoss(autobalance=True) updates its balance with after the call (utils/loss.py:197-201; host state, the kernel only reports). */
int somi_yolo_loss_f32(const somi_loss_desc *d, float *out8, void *workspace, size_t workspace_bytes,
                       somi_stream_t stream);
/* Five detection levels (models/hub/yolov5-p7.yaml, Detect over P3..P7): d->nl = 5, levels 0..3 in the descriptor (whose layout stays as it is) and the
 * fifth in `l5`.  out9 = out8 + obji[4].  Same kernels and the same order of sums as somi_yolo_loss_f32, which keeps serving 1 to 4 levels. */
typedef struct somi_loss_level {
    const float *p;
    float *grad;
    int32_t ny, nx;
    float balance;
} somi_loss_level;
size_t somi_loss5_workspace_bytes(const somi_loss_desc *d, const somi_loss_level *l5);
int somi_yolo_loss5_f32(const somi_loss_desc *d, const somi_loss_level *l5, float *out9, void *workspace, size_t workspace_bytes,
                        somi_stream_t stream);

/* The box-regression rule of the loss: which reference call stands where utils/loss.py:161 hard-codes bbox_iou(..., CIoU=True).
 * kind IOU..WIOU: bbox_iou(pbox.T, tbox, x1y1x2y2=False, <flag>, Focal, alpha, gamma, scale) (utils/metrics.py:476-583); SHAPE: shape_iou
 * (:397-439); inner != 0: bbox_inner_iou(pbox, tbox, xywh=True, <flag>, ratio) (:604-702, its xywh branch as written).  A tensor result r
 * enters the loss as mean(1 - r) with similarity s = r; a pair (r0, r1) as mean(r1.detach() * (1 - r0)), s = r0 (Focal, unscaled WIoU); the
 * triple of scaled WIoU as mean(r0 * r1), s = r2.  s takes the place of the CIoU in the NWD blend, the objectness target and the SlideLoss mean.
 * Which combinations mean something is the caller's business (somi_amd.loss.ComputeLoss refuses the rest); the library checks ranges only. */
enum somi_loss_iou_kind { SOMI_LOSS_IOU = 0, SOMI_LOSS_GIOU = 1, SOMI_LOSS_DIOU = 2, SOMI_LOSS_CIOU = 3, SOMI_LOSS_EIOU = 4, SOMI_LOSS_SIOU = 5,
                          SOMI_LOSS_EFFICICIOU = 6, SOMI_LOSS_WIOU = 7, SOMI_LOSS_SHAPE = 8 };
typedef struct somi_loss_box_rule {
    int32_t kind;        /* enum somi_loss_iou_kind */
    int32_t focal;       /* Focal=True: the pair form, weight (inter / (union + eps)) ** gamma */
    int32_t inner;       /* bbox_inner_iou with `inner_ratio` instead of bbox_iou */
    int32_t wiou_scaled; /* WIoU with scale=True: the non-monotonic focusing factor of WIoU_Scale (v3) */
    float alpha;         /* >= 1; 1 leaves every pow out */
    float gamma;         /* Focal exponent */
    float inner_ratio;
    float shape_scale;   /* shape_iou's scale1 */
    double *wiou_mean;   /* device, one element: WIoU_Scale.iou_mean.  Read and (with wiou_train) updated by every call with wiou_scaled, level by
                          * level in level order before that level's factor is formed, with momentum 1 - 0.5 ** (1 / 7000); no host round trip */
    int32_t wiou_train;  /* WIoU_Scale._is_train */
} somi_loss_box_rule;
/* `l5` NULL: up to four levels; else d->nl = 5.  CIoU without focal / inner and alpha = 1 - the default rule - runs the very kernels of
 * somi_yolo_loss_f32 / somi_yolo_loss5_f32 and gives their bits.  out9: as there (eight floats are written for up to four levels). */
size_t somi_loss_rule_workspace_bytes(const somi_loss_desc *d, const somi_loss_level *l5, const somi_loss_box_rule *rule);
int somi_yolo_loss_rule_f32(const somi_loss_desc *d, const somi_loss_level *l5, const somi_loss_box_rule *rule, float *out9, void *workspace,
                            size_t workspace_bytes, somi_stream_t stream);

/* Repulsion loss, RepGT + RepBox (utils/RepulsionLoss.py:47-95; imported by utils/loss.py:8 but never called by ComputeLoss,
 * so it is an optional term and off by default).  pbox, gtbox: (B,A,4) xyxy; fg_mask: (B,A) bytes (non-zero = foreground).
 * Value only - the reference detaches both box sets.  out2 = {rep_gt, rep_box}, each the mean over the images that have
 * foreground anchors (0/0 = NaN when none has, like the reference). */
size_t somi_repulsion_workspace_bytes(int B, int A);
int somi_repulsion_loss_f32(const float *pbox, const float *gtbox, const uint8_t *fg_mask, int B, int A, float sigma_repgt,
                            float sigma_repbox, float pnms, float gtnms, float *out2, void *workspace, size_t workspace_bytes,
                            somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weighted boxes fusion (wbf.py:68 -> ensemble_boxes.weighted_boxes_fusion, conf_type 'avg').
 * boxes (n,4) xyxy in [0,1], scores (n), labels (n) int32, model (n) int32, already concatenated over models
 * in model order; out_* sized n; out_count 1 int32.  One launch per image; sequential per label by design.
 *
 * Float32 contract: weights, iou_thr and skip_box_thr are float32 values.  The kernel widens them exactly and from there on compares and
 * multiplies in float64 as the package does, so the result equals the package's called with those float32 values (a weight such as 0.7
 * is the float32 nearest to 0.7, not the double; callers that hold doubles round them first - somi_amd.wbf does).  `score < skip_box_thr`
 * drops a box and `iou > iou_thr` joins a cluster, both strict, at the float32 values.
 *
 * Labels: integers in [0, SOMI_WBF_MAX_LABELS).  A label outside that range is never dropped silently: if any of an image's n member rows
 * carries one (whether or not the row would pass the score and area filters), the image is not fused, its out_count is SOMI_WBF_BAD_LABEL
 * and its out_boxes / out_scores / out_labels rows are not written.  Rows at and beyond out_count are never written either.
 */
#define SOMI_WBF_MAX_LABELS 128  /* label capacity of one image (static LDS tables); the largest nc the repository's configs build is 80 */
#define SOMI_WBF_BAD_LABEL  (-1) /* out_count of an image that holds a label outside [0, SOMI_WBF_MAX_LABELS) */
size_t somi_wbf_workspace_bytes(int n);
int somi_wbf_f32(const float *boxes, const float *scores, const int32_t *labels, const int32_t *model, int n,
                 int n_models, const float *weights_host, float iou_thr, float skip_box_thr, float *out_boxes,
                 float *out_scores, int32_t *out_labels, int32_t *out_count, void *workspace, size_t workspace_bytes,
                 somi_stream_t stream);
/* Batched form (BASELINE configs[4]: val.py's NMS followed by wbf.py over the detections of several models): one workgroup per image.
 * det[t] (B,max_det,6) [x1,y1,x2,y2,conf,cls] in pixels and count[t] (B) are somi_nms_f32's outputs for model t (host arrays of
 * n_models device pointers).  Image b's members are model 0's rows, then model 1's, ... (the order wbf.py:44-59 appends them in),
 * boxes divided by (img_w, img_h) and clipped to [0,1].  Outputs are strided per image by N = n_models * max_det:
 * out_boxes (B,N,4), out_scores (B,N), out_labels (B,N), out_count (B).  Same arithmetic as somi_wbf_f32, image by image, under the same
 * float32 contract (img_w and img_h are float32 too; the division is a true float32 division).  count[t][b] is clamped to [0, max_det].
 * The class column is truncated to int32; an image with a class outside [0, SOMI_WBF_MAX_LABELS) among its counted rows gets
 * out_count[b] = SOMI_WBF_BAD_LABEL and unwritten output rows, the other images of the batch are fused as usual.  No host synchronisation.
 */
size_t somi_wbf_batch_workspace_bytes(int B, int max_det, int n_models);
int somi_wbf_batch_f32(const float *const *det, const int32_t *const *count, int B, int max_det, int n_models,
                       const float *weights_host, float img_w, float img_h, float iou_thr, float skip_box_thr, float *out_boxes,
                       float *out_scores, int32_t *out_labels, int32_t *out_count, void *workspace, size_t workspace_bytes,
                       somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Validation metrics after NMS.
 * somi_val_match_f32 = val.py:50-71 `process_batch` for a batch of images: det (sum N_b, 6) x1,y1,x2,y2,conf,cls and
 * labels (sum M_b, 5) cls,x1,y1,x2,y2 are concatenated per image, det_off / lab_off (B+1 ints, device) delimit the images;
 * iouv: T <= 16 ascending IoU levels (device); correct: (sum N_b, T) bytes.  max_det / max_labels: largest per-image counts
 * (host values; they size the LDS tables).  Exact IoU ties are broken by lowest label index (the reference's sort is
 * unstable there).
 * somi_ap_per_class_f64 = utils/metrics.py:21-95 `ap_per_class`: tp (N,T) bytes, conf / pred_cls (N), target_cls (M) with
 * integer-valued class ids in [0, ncap).  Outputs for the classes present among the targets, ascending: out_classes,
 * *out_n, ap (n,T), and p / r / f1 at the confidence of best mean F1 - all in fp64 like numpy.  Equal confidences keep
 * their input order. */
int somi_val_match_f32(const float *det, const int *det_off, const float *labels, const int *lab_off, const float *iouv, int T,
                       int B, int max_det, int max_labels, uint8_t *correct, somi_stream_t stream);
/* somi_confusion_matrix_f32 = utils/metrics.py:98-142 `ConfusionMatrix.process_batch` (val.py:141,186) for a batch of images in
 * the layout of somi_val_match_f32: detections above `conf` are matched to labels regardless of class (best label per detection,
 * then best detection per label, IoU > iou_thres) and counted into matrix[(nc+1) x (nc+1)] int32, row = predicted class, column =
 * true class, index nc = background; counts are ADDED (zero the matrix once).  An image's unmatched detections count only if the
 * image has at least one match, as in the reference.  Classes outside [0, nc] are ignored. */
int somi_confusion_matrix_f32(const float *det, const int *det_off, const float *labels, const int *lab_off, int B, int max_det,
                              int max_labels, int nc, float conf, float iou_thres, int32_t *matrix, somi_stream_t stream);
size_t somi_ap_per_class_workspace_bytes(long N, int T, int ncap);
int somi_ap_per_class_f64(const uint8_t *tp, const float *conf, const float *pred_cls, const float *target_cls, long N, long M,
                          int T, int ncap, int *out_classes, int *out_n, double *out_ap, double *out_p, double *out_r,
                          double *out_f1, void *workspace, size_t workspace_bytes, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline on device: what `LoadImagesAndLabels.__getitem__` does to the pixels of one
 * sample once the source images are cached at the training size - mosaic composition (utils/datasets.py:732-777), the
 * affine crop (`random_perspective` -> cv2.warpAffine, utils/augmentations.py:126-169), mixup (:305-310), HSV jitter
 * (`augment_hsv` :47-61), flips and the HWC BGR -> CHW RGB transpose (datasets.py:648-671) - fused into one pass per output
 * pixel: the 2s x 2s mosaic canvas is never materialised.  Random draws, matrices and label boxes stay with the caller
 * (they are a few hundred scalars per sample); it passes one `somi_aug_sample` per output image, in device memory.
 *
 * canvas(x, y) = the LAST source whose rectangle [x1,x2) x [y1,y2) holds (x, y), read at pixels[y - dy][x - dx], else `fill`.
 * warp == 0: out(x, y) = canvas(x, y) (letterbox: one source placed at (left, top)).
 * warp == 1: out(x, y) = bilinear sample of the canvas at minv * (x, y, 1), taps outside the canvas = `fill`, in the fixed
 *            point of OpenCV 4.9 warpAffine (coordinates to 1/32 pixel from round(m*1024) terms, 15-bit weights).
 * mix:  out = (uint8) trunc(canvas[0] * mix_r + canvas[1] * (1 - mix_r)) in fp64.
 * hsv:  BGR -> HSV (OpenCV 8-bit, hue range 180), channel-wise through lut[0..2], HSV -> BGR.
 * flips move the pixel, then it is stored as out[b][2 - c][y][x] (RGB planes).
 * Sources and output are at most 16384 px a side.  The caller guarantees that every rectangle maps inside its source
 * (0 <= x1 - dx, x2 - dx <= w, same for y): the records live in device memory, so the library cannot check them. */
typedef struct somi_aug_source {
    const uint8_t *pixels;       /* device, (h, w, 3) BGR, tightly packed */
    int32_t h, w;
    int32_t x1, y1, x2, y2;
    int32_t dx, dy;
} somi_aug_source;

typedef struct somi_aug_canvas {
    somi_aug_source src[4];
    int32_t nsrc, height, width, warp;
    double minv[6];              /* dst -> src, row-major 2x3 (the inverse of the matrix cv2.warpAffine is given) */
} somi_aug_canvas;

typedef struct somi_aug_sample {
    somi_aug_canvas canvas[2];
    int32_t mix, hsv, flipud, fliplr;
    double mix_r;
    uint8_t lut[3][256];
} somi_aug_sample;

int somi_augment_u8(const somi_aug_sample *samples, int B, int H, int W, int fill, uint8_t *out, somi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AutoAnchor (utils/autoanchor.py): anchor metric, genetic evolution and the Lloyd step of scipy.cluster.vq.kmeans.
 * wh: (n, 2) fp32 label sizes in pixels; anchors: (na, 2) fp32, na <= 64; thr is the reference's 1 / anchor_t.
 * metric: x = min(w/kw, kw/w, h/kh, kh/h) in fp32 with IEEE division, best = max over the anchors (written to `best`
 *   when it is not NULL); out[0] = labels with best > thr, out[1] = (label, anchor) pairs with x > thr, out[2] = sum of
 *   best over the labels with best > thr.  The sums are fp64 and EXACT for thr >= 1/8 and n < 2^27 (every term is a
 *   multiple of 2^-26), hence independent of the launch shape.
 * evolve: generations 0..gen-1 one after the other, all enqueued by one call and with no host round trip: candidate
 *   kg = max(k * v[g], 2.0) in fp64 (v: (gen, na, 2) fp64 mutation factors), rounded to fp32 for the metric; if its
 *   fitness sum (out[2] above) is > *fitness then k <- kg, *fitness <- that sum and g is appended to `accepted`
 *   (int32, gen + 1 entries: [0] = count - zero it before the first call - then the generations).  *fitness holds the sum
 *   of the start k on entry.
 * kmeans lloyd step: one iteration of _kmeans for `restarts` independent code books at once, fp64.  book (restarts, k, 2),
 *   alive (restarts, k) int32 (1 = the code is still in the book; codes that end an iteration without members leave it),
 *   dist (restarts) = mean Euclidean distance of the assignment before the move (set it to +inf before the first step),
 *   done (restarts) int32 is raised when |previous dist - dist| <= thresh and freezes that restart, iters counts the
 *   steps a restart took.  k <= 32.  The caller reads `done` between steps; nothing else leaves the device.
 * Workspaces hold per-block partial sums; every fold has a fixed order, no float atomics. */
size_t somi_anchor_metric_workspace_bytes(long n);
int somi_anchor_metric_f32(const float *wh, long n, const float *anchors, int na, float thr, float *best, double *out,
                           void *workspace, size_t workspace_bytes, somi_stream_t stream);
int somi_anchor_evolve_f32(const float *wh, long n, double *k, int na, const double *v, int gen, float thr, double *fitness,
                           int32_t *accepted, void *workspace, size_t workspace_bytes, somi_stream_t stream);
size_t somi_kmeans_workspace_bytes(long n, int k, int restarts);
int somi_kmeans_lloyd_step_f64(const double *obs, long n, double *book, int32_t *alive, int k, int restarts, double thresh,
                               double *dist, int32_t *done, int32_t *iters, void *workspace, size_t workspace_bytes,
                               somi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SOMI_HIP_H */
