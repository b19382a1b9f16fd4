"""Torch-tensor wrappers over the C ABI (device pointers + current HIP stream).

PyTorch is plumbing here: it owns the HBM allocations and the stream; all arithmetic happens in
libsomi_hip.so.  Tensors must live on the GPU; anything else raises.
"""
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import ConvDesc, check

DCN_DIRECT = os.environ.get('SOMI_DCN_DIRECT', '0') == '1'          # 1: DCNv3 backward scatters with fp32 atomics (the reference's form)
PROFILE = None   # bench.py sets this to a list: every conv launch appends (kernel name, algorithmic FLOPs, ev0, ev1)



class _timed:
    """`with _timed(info):` around a launch: while bench.py profiles (PROFILE is a list) an event pair brackets the body on torch's current
    stream - the stream the kernel runs on - and info() -> (kernel name, algorithmic work, shape key) completes the entry
    (name, work, ev0, ev1, key).  Otherwise nothing happens: no events, info is never called."""
    __slots__ = ('info', 'ev')

    def __init__(self, info):
        self.info, self.ev = info, None

    def __enter__(self):
        if PROFILE is not None:
            self.ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.ev[0].record()

    def __exit__(self, etype, *exc):
        if self.ev is not None and etype is None:
            self.ev[1].record()
            name, work, key = self.info()
            PROFILE.append((name, work, *self.ev, key))
        return False


ACT = {'none': 0, None: 0, 'silu': 1, 'gelu': 2, 'relu': 3, 'sigmoid': 4, 'leaky': 5,       # enum somi_act; leaky = LeakyReLU(0.1)
       'hswish': 6,                 # x * relu6(x + 3) / 6
       'softmax': 5}                # somi_linear_f32 only, which reads 5 as a softmax over its outputs


_CONV_WS = {}
# Opt-in reduced precision of the conv family's products (train.py:263 `amp.autocast`): 0 exact fp32 (the default, what every parity
# claim is made on), 1 bf16 operands, 2 bf16x3 split (somi_conv_desc.prec).  train.TrainStep(amp=...) / bench.py --amp set it.
CONV_PREC = 0
PREC = {None: 0, 'f32': 0, 'bf16': 1, 'bf16x3': 2}


def _conv_workspace(d, dev):
    """Attach the stream-K scratch of the current stream to a conv descriptor (launches on one stream are ordered, so they
    can share it).  A descriptor without it runs the one-workgroup-per-tile schedule."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _CONV_WS.get(key)
    if ws is None:
        ws = _CONV_WS[key] = torch.empty(_lib.lib().somi_conv2d_workspace_bytes(), dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('somi_amd ops need GPU tensors (no CPU fallback)')
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t, name='tensor'):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f'{name} tensor has to be contiguous float32')
    return t


def _map(t, shape, what):
    """t, once its leading (B, H, W) is known to be `shape`: a tuple, or a map whose sizes t must share."""
    want = tuple(shape.shape[:3]) if torch.is_tensor(shape) else tuple(shape)
    if tuple(t.shape[:3]) != want:
        raise RuntimeError(f'{what} must be {want} + (channels,), got {tuple(t.shape)}')
    return t


def _check_impl(rc, what):
    """check() for the entry points that refuse a configuration before any launch: that refusal is a NotImplementedError."""
    if rc == -2:                                                  # SOMI_ENOTIMPL
        raise NotImplementedError(f'{what}: {_lib.lib().somi_last_error().decode(errors="replace")}')
    check(rc, what)


def _scratch(d, floats, dev):
    """A fresh float workspace of at least `floats` on descriptor d -> the tensor, which the caller keeps alive until the launch is enqueued."""
    ws = torch.empty(max(floats, 4), device=dev, dtype=torch.float32)
    d.workspace, d.workspace_floats = _ptr(ws), ws.numel()
    return ws


def conv_out_size(size, k, s, p, d=1):
    return (size + 2 * p - (d * (k - 1) + 1)) // s + 1


def conv2d_nhwc(x, w, bias=None, *, kh, kw, stride=1, pad=0, dil=1, act='none', cin=None, x_coff=0, out=None,
                cout=None, y_coff=0, post_scale=None, post_shift=None, residual=None, res_coff=0, a_chan_scale=None,
                a_pix_scale=None, per_sample_w=False, alg_cin=None, alg_cout=None, bn_stats=None):
    """x (B,H,W,x_cs) NHWC; w packed [n_sets][Cout][kh*kw*Cin]; returns / fills out (B,Ho,Wo,y_cs)."""
    B, H, W, x_cs = x.shape
    cin = x_cs - x_coff if cin is None else cin
    cout = w.shape[-2] if cout is None else cout
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    if out is None:
        out = torch.empty(B, Ho, Wo, cout, device=x.device, dtype=torch.float32)
    d = ConvDesc()
    d.prec = CONV_PREC
    d.x, d.w, d.bias, d.y = _ptr(_f32c(x, 'input')), _ptr(_f32c(w, 'weight')), _ptr(bias), _ptr(_f32c(out, 'output'))
    d.post_scale, d.post_shift, d.residual = _ptr(post_scale), _ptr(post_shift), _ptr(residual)
    d.a_chan_scale, d.a_pix_scale = _ptr(a_chan_scale), _ptr(a_pix_scale)
    d.B, d.H, d.W, d.Cin, d.x_cs, d.x_coff = B, H, W, cin, x_cs, x_coff
    d.Ho, d.Wo, d.Cout, d.y_cs, d.y_coff = Ho, Wo, cout, out.shape[3], y_coff
    d.kh, d.kw, d.stride, d.pad, d.dil = kh, kw, stride, pad, dil
    _conv_workspace(d, x.device)
    d.res_cs, d.res_coff = (residual.shape[3] if residual is not None else 0), res_coff
    d.act, d.per_sample_w = ACT[act], int(per_sample_w)
    if w.numel() != (B if per_sample_w else 1) * cout * kh * kw * cin:
        raise RuntimeError(f'weight has {w.numel()} elements, expected {(B if per_sample_w else 1) * cout * kh * kw * cin}')
    if bn_stats is not None:                                      # dict filled in place: the epilogue leaves partial channel sums
        rows = _lib.lib().somi_conv2d_stat_rows(C.byref(d))
        part = torch.empty(2, rows, cout, device=x.device, dtype=torch.float32)
        d.stat_sum, d.stat_sumsq, d.stat_pivot = part[0].data_ptr(), part[1].data_ptr(), _ptr(bn_stats.get('pivot'))
        bn_stats['part'], bn_stats['rows'] = part, rows
    with _timed(lambda: (_lib.lib().somi_conv2d_kernel_name(C.byref(d)).decode(), 2.0 * B * Ho * Wo * (alg_cout or cout) * (alg_cin or cin) * kh * kw,
                         (B, H, W, cin, cout, kh, stride, int(per_sample_w)))):
        check(_lib.lib().somi_conv2d_nhwc_f32(C.byref(d), _stream()), 'conv2d_nhwc')
    return out


_DCN_SUFFIX = {torch.float32: 'f32', torch.float16: 'f16', torch.float64: 'f64'}


def dcnv3_forward_raw(input, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels, offset_scale,
                      im2col_step):
    N, H, W, _ = input.shape
    Ho, Wo = conv_out_size(H, kh, sh, ph, dh), conv_out_size(W, kw, sw, pw, dw)
    if input.dtype != torch.float32:                              # half / double: the reference's other two dispatch types
        out = torch.empty(N, Ho, Wo, group * group_channels, device=input.device, dtype=input.dtype)
        fn = getattr(_lib.lib(), 'somi_dcnv3_forward_' + _DCN_SUFFIX[input.dtype])
        check(fn(_ptr(input), _ptr(offset), _ptr(mask), _ptr(out), N, H, W, group, group_channels, kh, kw, sh, sw, ph, pw, dh, dw,
                 float(offset_scale), int(im2col_step), _stream()), 'dcnv3_forward')
        return out
    out = torch.empty(N, Ho, Wo, group * group_channels, device=input.device, dtype=torch.float32)
    C_, GK = group * group_channels, group * kh * kw             # algorithmic bytes: 4 (2C + 3GK) per output pixel
    with _timed(lambda: ('dcnv3_fwd_kernel', 4.0 * N * Ho * Wo * (2 * C_ + 3 * GK), (N, H, W, C_, group, kh, sh, 10))):
        check(_lib.lib().somi_dcnv3_forward_f32(_ptr(input), _ptr(offset), _ptr(mask), _ptr(out), N, H, W, group,
                                                group_channels, kh, kw, sh, sw, ph, pw, dh, dw, float(offset_scale),
                                                int(im2col_step), _stream()), 'dcnv3_forward')
    return out


DCN_LAST_WORKSPACE = None
_DCN_WS = {}                                                     # device -> the windowed backward's workspace (grow-only: the staging slab, <= SOMI_DCN_SLAB_MB = 1 GiB by default, + near masks)
_DCN_FAR = {}                                                    # device -> int64 device counter: far taps of EVERY windowed backward since the last reset


def dcn_overflow_taps(total=False):
    """FAR sampling taps of the windowed DCNv3 backward - those that went to grad_input as fp32 atomics because they landed more than
    two tiles from their own (0 <=> bit-reproducible).  Default: the last call only.  total=True: summed over every call on every device
    since reset_dcn_overflow_taps() - a graph has several DCNv3 sites sharing one workspace whose counter word each call zeroes again, so
    "no float atomic ran in this step" is a statement about the total.  Host sync; diagnostics / tests."""
    if total:
        return int(sum(int(t.item()) for t in _DCN_FAR.values()))
    ws = DCN_LAST_WORKSPACE
    return None if ws is None else int(ws[-256:-252].view(torch.int32).item())


def reset_dcn_overflow_taps():
    for t in _DCN_FAR.values():
        t.zero_()


def _dcn_count_far(ws):
    """Adds the call's far-tap word to the device's running total (one tiny stream-ordered add, no sync)."""
    tot = _DCN_FAR.get(ws.device)
    if tot is None:
        tot = _DCN_FAR[ws.device] = torch.zeros(1, dtype=torch.int64, device=ws.device)
    tot.add_(ws[-256:-252].view(torch.int32))


def free_workspaces():
    """Releases the per-device DCNv3 backward workspace (up to SOMI_DCN_SLAB_MB + near masks; it is otherwise kept for the life of the
    process and only grows).  The next windowed backward allocates it again."""
    global DCN_LAST_WORKSPACE
    DCN_LAST_WORKSPACE = None
    _DCN_WS.clear()


def _dcn_workspace(nbytes, dev):
    """One buffer per device serves every windowed backward: the library caps the staging slab (SOMI_DCN_SLAB_MB, 1024 by default - a memory
    bound, see dcnv3.hip) and walks the batch through it in chunks of images (round 2 allocated up to 2.95 GB per call and kept it in a global)."""
    ws = _DCN_WS.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = _DCN_WS[dev] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws[:nbytes]


def dcnv3_backward_raw(input, offset, mask, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels,
                       offset_scale, im2col_step):
    N, H, W, _ = input.shape
    if input.dtype != torch.float32:
        # half: fp32 gradient buffers cast back to half afterwards, exactly as dcnv3_cuda.cu:126-133,168-170; double: double
        gdt = torch.float64 if input.dtype == torch.float64 else torch.float32
        gi = torch.zeros(input.shape, device=input.device, dtype=gdt)
        go = torch.empty(offset.shape, device=input.device, dtype=gdt)
        gm = torch.empty(mask.shape, device=input.device, dtype=gdt)
        fn = getattr(_lib.lib(), 'somi_dcnv3_backward_' + _DCN_SUFFIX[input.dtype])
        check(fn(_ptr(input), _ptr(offset), _ptr(mask), _ptr(grad_output), _ptr(gi), _ptr(go), _ptr(gm), N, H, W, group, group_channels, kh, kw,
                 sh, sw, ph, pw, dh, dw, float(offset_scale), int(im2col_step), None, 0, _stream()), 'dcnv3_backward')
        return gi.to(input.dtype), go.to(input.dtype), gm.to(input.dtype)
    gi = torch.zeros_like(input)
    go = torch.empty_like(offset)
    gm = torch.empty_like(mask)
    C_, GK, (Ho, Wo) = group * group_channels, group * kh * kw, grad_output.shape[1:3]          # 4 (4C + 6GK) bytes per output pixel
    global DCN_LAST_WORKSPACE
    with _timed(lambda: ('dcnv3_bwd_kernel', 4.0 * N * Ho * Wo * (4 * C_ + 6 * GK), (N, H, W, C_, group, kh, sh, 11))):
        L = _lib.lib()
        nbytes = 0 if DCN_DIRECT else L.somi_dcnv3_backward_workspace_bytes(N, H, W, group, group_channels, kh, kw, sh, sw, ph, pw, dh, dw, float(offset_scale))
        ws = _dcn_workspace(nbytes, input.device) if nbytes else None   # staging slab + near masks + overflow word of the windowed form
        DCN_LAST_WORKSPACE = ws                                  # tests read the overflow-tap counter at its end (dcn_overflow_taps)
        check(L.somi_dcnv3_backward_f32(_ptr(input), _ptr(offset), _ptr(mask), _ptr(grad_output), _ptr(gi), _ptr(go),
                                        _ptr(gm), N, H, W, group, group_channels, kh, kw, sh, sw, ph, pw, dh, dw,
                                        float(offset_scale), int(im2col_step), _ptr(ws), nbytes, _stream()), 'dcnv3_backward')
    if ws is not None:
        _dcn_count_far(ws)
    return gi, go, gm


def dcnv3_forward_merged(input, om, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels, offset_scale, im2col_step):
    """The fp32 operator over ONE tensor om (N,Ho,Wo,R >= 3*G*K) holding [2*G*K offsets | G*K masks (already soft-maxed) | pad] per pixel -
    the output of a single 1x1 GEMM with the two Linear weights stacked (modules/dcnv3.py:330-334).  Same arithmetic as dcnv3_forward_raw."""
    N, H, W, _ = input.shape
    Ho, Wo = conv_out_size(H, kh, sh, ph, dh), conv_out_size(W, kw, sw, pw, dw)
    R, GK = om.shape[-1], group * kh * kw
    if om.shape[:3] != (N, Ho, Wo) or R < 3 * GK or not om.is_contiguous() or om.dtype != torch.float32:
        raise RuntimeError(f'dcnv3 (merged offset/mask): om must be contiguous float32 ({N},{Ho},{Wo},>={3 * GK}), got {tuple(om.shape)}')
    out = torch.empty(N, Ho, Wo, group * group_channels, device=input.device, dtype=torch.float32)
    C_ = group * group_channels
    with _timed(lambda: ('dcnv3_fwd_kernel', 4.0 * N * Ho * Wo * (2 * C_ + 3 * GK), (N, H, W, C_, group, kh, sh, 10))):
        check(_lib.lib().somi_dcnv3_forward_strided_f32(_ptr(input), om.data_ptr(), om.data_ptr() + 8 * GK, R, R, _ptr(out), N, H, W, group,
                                                        group_channels, kh, kw, sh, sw, ph, pw, dh, dw, float(offset_scale), int(im2col_step),
                                                        _stream()), 'dcnv3_forward')
    return out


def dcnv3_backward_merged(input, om, grad_output, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels, offset_scale, im2col_step):
    """-> (grad_input, d_om): d_om has om's layout - grad_offset in the first 2*G*K columns, grad_mask (w.r.t. the soft-maxed mask) in the
    next G*K, zeros in the pad."""
    N, H, W, _ = input.shape
    R, GK = om.shape[-1], group * kh * kw
    gi = torch.zeros_like(input)
    d_om = torch.empty_like(om)
    if R != 3 * GK:
        d_om[..., 3 * GK:].zero_()                                # the operator writes the first 3GK columns of every row; the pad stays zero
    C_, (Ho, Wo) = group * group_channels, grad_output.shape[1:3]
    global DCN_LAST_WORKSPACE
    with _timed(lambda: ('dcnv3_bwd_kernel', 4.0 * N * Ho * Wo * (4 * C_ + 6 * GK), (N, H, W, C_, group, kh, sh, 11))):
        L = _lib.lib()
        nbytes = 0 if DCN_DIRECT else L.somi_dcnv3_backward_workspace_bytes(N, H, W, group, group_channels, kh, kw, sh, sw, ph, pw, dh, dw, float(offset_scale))
        ws = _dcn_workspace(nbytes, input.device) if nbytes else None
        DCN_LAST_WORKSPACE = ws
        check(L.somi_dcnv3_backward_strided_f32(_ptr(input), om.data_ptr(), om.data_ptr() + 8 * GK, R, R, _ptr(grad_output), _ptr(gi),
                                                d_om.data_ptr(), d_om.data_ptr() + 8 * GK, N, H, W, group, group_channels, kh, kw, sh, sw, ph, pw,
                                                dh, dw, float(offset_scale), int(im2col_step), _ptr(ws), nbytes, _stream()), 'dcnv3_backward')
    if ws is not None:
        _dcn_count_far(ws)
    return gi, d_om


def group_softmax_cols_(om, G, K, col):
    """In place: softmax over each of the G groups of K columns starting at column `col` of every row of om (..., R)."""
    R = om.shape[-1]
    p = om.data_ptr() + 4 * col
    check(_lib.lib().somi_group_softmax_strided_f32(p, R, p, R, om.numel() // R, G, K, _stream()), 'group_softmax')
    return om


def group_softmax_backward_cols_(om, d_om, G, K, col):
    """In place on d_om's columns [col, col + G*K): dmask -> dlogits, with the soft-maxed masks read from the same columns of om."""
    R = om.shape[-1]
    check(_lib.lib().somi_group_softmax_bwd_strided_f32(om.data_ptr() + 4 * col, R, d_om.data_ptr() + 4 * col, d_om.data_ptr() + 4 * col, R,
                                                        om.numel() // R, G, K, _stream()), 'group_softmax_bwd')
    return d_om


def image_to_nhwc4(img, scale=1.0 / 255.0):
    """(B,C<=4,H,W) uint8 or float32 NCHW -> (B,H,W,4) float32 (train.py:249 `/255`)."""
    B, Cc, H, W = img.shape
    if not img.is_contiguous():
        raise RuntimeError('image batch has to be contiguous NCHW')
    y = torch.empty(B, H, W, 4, device=img.device, dtype=torch.float32)
    L = _lib.lib()
    if img.dtype == torch.uint8:
        if abs(scale - 1.0 / 255.0) > 1e-12:
            raise RuntimeError('uint8 images are always scaled by 1/255')
        check(L.somi_image_u8_to_nhwc4(_ptr(img), _ptr(y), B, Cc, H, W, _stream()), 'image_u8_to_nhwc4')
    elif img.dtype == torch.float32:
        check(L.somi_image_f32_to_nhwc4(_ptr(img), _ptr(y), B, Cc, H, W, float(scale), _stream()), 'image_f32_to_nhwc4')
    else:
        raise RuntimeError('images must be uint8 or float32')
    return y


def dwconv3x3(x, w, bias=None, post_scale=None, post_shift=None, residual=None, act='none', out=None):
    B, H, W, Cc = x.shape
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().somi_dwconv3x3_nhwc_f32(_ptr(_f32c(x)), _ptr(w), _ptr(bias), _ptr(post_scale), _ptr(post_shift),
                                             _ptr(residual), _ptr(out), B, H, W, Cc, ACT[act], _stream()), 'dwconv3x3')
    return out


def dwconv3x3_ln(x, w, bias, gamma, beta, eps, act='gelu'):
    """(u, y): u = depthwise 3x3 conv of x (+bias), y = act(LayerNorm_C(u)) - one pass (256 channels; somi_dwconv3x3_ln_nhwc_f32)."""
    B, H, W, Cc = x.shape
    u, y = torch.empty_like(x), torch.empty_like(x)
    check(_lib.lib().somi_dwconv3x3_ln_nhwc_f32(_ptr(_f32c(x)), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), float(eps), ACT[act], _ptr(u), _ptr(y),
                                                B, H, W, Cc, _stream()), 'dwconv3x3_ln')
    return u, y


def sppf_pool_(buf, c, x_coff=0, codes=False):
    """The three chained 5x5 pools of slice [x_coff, x_coff + c) into the next three slices of `buf`.  codes=True (training): level by level, and
    -> (buf, codes): where each window's first maximum sits, for sppf_pool_backward_(codes=...)."""
    B, H, W, cs = buf.shape
    if codes:
        arg = torch.empty(3 * B * H * W * c, device=buf.device, dtype=torch.uint8)
        check(_lib.lib().somi_sppf_pool_codes_nhwc_f32(_ptr(_f32c(buf)), _ptr(arg), B, H, W, c, cs, x_coff, _stream()), 'sppf_pool_codes')
        return buf, arg
    check(_lib.lib().somi_sppf_pool_nhwc_f32(_ptr(_f32c(buf)), B, H, W, c, cs, x_coff, _stream()), 'sppf_pool')
    return buf


def maxpool2_out_size(size, stride, pad0, pad1):
    """Floor-mode output size of a 2-wide window over a map padded by (pad0, pad1)."""
    return (size + pad0 + pad1 - 2) // stride + 1


def maxpool2(x, c, x_coff=0, *, stride=2, pad=(0, 0, 0, 0), out=None, y_coff=0, codes=False):
    """nn.MaxPool2d(2, stride, 0) of slice [x_coff, x_coff + c) of x (B,H,W,cs) over a ZERO pad (left, right, top, bottom) folded into the read
    -> out (B,Ho,Wo,*) slice at y_coff.  codes=True (training): -> (out, codes), one byte per pooled element for maxpool2_backward."""
    B, H, W, _ = x.shape
    pl, pr, pt, pb = (int(v) for v in pad)
    Ho, Wo = maxpool2_out_size(H, stride, pt, pb), maxpool2_out_size(W, stride, pl, pr)
    if out is None:
        out = torch.empty(B, max(Ho, 0), max(Wo, 0), c, device=x.device, dtype=torch.float32)
    if Ho < 1 or Wo < 1 or tuple(out.shape[:3]) != (B, Ho, Wo):
        raise RuntimeError(f'maxpool2: output must be ({B}, {Ho}, {Wo}, .) with both sizes >= 1, got {tuple(out.shape)}')
    arg = torch.empty(B * Ho * Wo * c, device=x.device, dtype=torch.uint8) if codes else None
    check(_lib.lib().somi_maxpool2_nhwc_f32(_ptr(_f32c(x)), _ptr(_f32c(out)), _ptr(arg), B, H, W, c, x.shape[3], x_coff, out.shape[3], y_coff,
                                            int(stride), pl, pr, pt, pb, _stream()), 'maxpool2')
    return (out, arg) if codes else out


def maxpool2_backward(dy, codes, c, H, W, dy_coff=0, *, stride=2, pad=(0, 0, 0, 0), out=None, dx_coff=0):
    """dx (B,H,W,*) slice at dx_coff = the gradient of maxpool2's input, written (not added): every element gathers the outputs whose code points at it."""
    B = dy.shape[0]
    pl, pr, pt, pb = (int(v) for v in pad)
    if out is None:
        out = torch.empty(B, H, W, c, device=dy.device, dtype=torch.float32)
    Ho, Wo = maxpool2_out_size(H, stride, pt, pb), maxpool2_out_size(W, stride, pl, pr)
    if tuple(dy.shape[:3]) != (B, Ho, Wo) or tuple(out.shape[:3]) != (B, H, W) or codes.dtype != torch.uint8 or codes.numel() != B * Ho * Wo * c:
        raise RuntimeError(f'maxpool2_backward: dy must be ({B}, {Ho}, {Wo}, .), dx ({B}, {H}, {W}, .), codes {B * Ho * Wo * c} bytes')
    check(_lib.lib().somi_maxpool2_bwd_nhwc_f32(_ptr(_f32c(dy)), _ptr(codes), _ptr(_f32c(out)), B, H, W, c, dy.shape[3], dy_coff, out.shape[3], dx_coff,
                                                int(stride), pl, pr, pt, pb, _stream()), 'maxpool2_backward')
    return out


def _slice(t, coff):
    return _lib.Slice(_ptr(_f32c(t)), t.shape[3], coff)


_NO_SLICE = _lib.Slice(None, 0, 0)                              # an optional slice that is absent


def maxpool3s2_out_size(size):
    """Output size of F.max_pool2d(., 3, stride=2, padding=1), floor mode."""
    return (size - 1) // 2 + 1


def maxpool3s2(x, c, x_coff=0, *, out=None, y_coff=0, codes=False):
    """F.max_pool2d(., 3, stride=2, padding=1) of slice [x_coff, x_coff + c) of x (B,H,W,cs), the pad an implicit -inf -> out (B,Ho,Wo,*) slice at
    y_coff.  codes=True (training): -> (out, codes), one byte per pooled element for maxpool3s2_backward."""
    B, H, W, _ = x.shape
    Ho, Wo = maxpool3s2_out_size(H), maxpool3s2_out_size(W)
    if out is None:
        out = torch.empty(B, Ho, Wo, c, device=x.device, dtype=torch.float32)
    _map(out, (B, Ho, Wo), 'maxpool3s2: output')
    arg = torch.empty(B * Ho * Wo * c, device=x.device, dtype=torch.uint8) if codes else None
    check(_lib.lib().somi_maxpool3s2_nhwc_f32(C.byref(_slice(x, x_coff)), C.byref(_slice(out, y_coff)), _ptr(arg), B, H, W, c, _stream()), 'maxpool3s2')
    return (out, arg) if codes else out


def maxpool3s2_backward(dy, codes, c, H, W, dy_coff=0, *, out=None, dx_coff=0):
    """dx (B,H,W,*) slice at dx_coff = the gradient of maxpool3s2's input, written (not added): every element gathers the windows whose code points at it."""
    B = dy.shape[0]
    Ho, Wo = maxpool3s2_out_size(H), maxpool3s2_out_size(W)
    if out is None:
        out = torch.empty(B, H, W, c, device=dy.device, dtype=torch.float32)
    if tuple(dy.shape[:3]) != (B, Ho, Wo) or tuple(out.shape[:3]) != (B, H, W) or codes.dtype != torch.uint8 or codes.numel() != B * Ho * Wo * c:
        raise RuntimeError(f'maxpool3s2_backward: dy must be ({B}, {Ho}, {Wo}, .), dx ({B}, {H}, {W}, .), codes {B * Ho * Wo * c} bytes')
    check(_lib.lib().somi_maxpool3s2_bwd_nhwc_f32(C.byref(_slice(dy, dy_coff)), _ptr(codes), C.byref(_slice(out, dx_coff)), B, H, W, c, _stream()),
          'maxpool3s2_backward')
    return out


def _asff_desc(rs, vs, r_ups, v_ups, w, bias, c, what):
    """The descriptor of both fusion launches.  rs / vs: three (tensor, channel offset) each; -> (descriptor, (B, H, W))."""
    if tuple(w.shape) != (3, 48) or tuple(bias.shape) != (3,):
        raise RuntimeError(f'{what}: the weight_levels conv is (3, 48) with 3 biases, got {tuple(w.shape)} and {tuple(bias.shape)}')
    B = rs[0][0].shape[0]
    H, W = rs[0][0].shape[1] << r_ups[0], rs[0][0].shape[2] << r_ups[0]
    for (t, _), up in list(zip(rs, r_ups)) + list(zip(vs, v_ups)):
        if up not in (0, 1, 2) or H % (1 << up) or W % (1 << up) or tuple(t.shape[:3]) != (B, H >> up, W >> up):
            raise RuntimeError(f'{what}: an input read at up={up} must be ({B}, {H >> up}, {W >> up}, .), got {tuple(t.shape)}')
    d = _lib.AsffDesc()
    for i in range(3):
        d.r[i], d.v[i] = _slice(*rs[i]), _slice(*vs[i])
        d.r_up[i], d.v_up[i] = r_ups[i], v_ups[i]
    d.w, d.bias = _ptr(_f32c(w)), _ptr(_f32c(bias))
    d.B, d.H, d.W, d.C = B, H, W, c
    return d, (B, H, W)


def asff_fuse(rs, vs, r_ups, v_ups, w, bias, c, *, out=None, o_coff=0, weights=False):
    """ASFF's fusion: fused = sum_i softmax(w . cat(v) + bias)_i * r_i per output pixel; source r_i = rs[i] = (tensor, channel offset), c channels, and
    weight map v_i = vs[i], 16 channels, are read at (h >> up, w >> up) with their own up.  -> out (B,H,W,*) slice at o_coff; weights=True (training):
    -> (out, p) with p (B,H,W,3) the softmax, all asff_fuse_backward needs beyond the inputs."""
    d, (B, H, W) = _asff_desc(rs, vs, r_ups, v_ups, w, bias, c, 'asff_fuse')
    if out is None:
        out = torch.empty(B, H, W, c, device=w.device, dtype=torch.float32)
    _map(out, (B, H, W), 'asff_fuse: output')
    p = torch.empty(B, H, W, 3, device=w.device, dtype=torch.float32) if weights else None
    d.out, d.p = _slice(out, o_coff), _ptr(p)
    check(_lib.lib().somi_asff_fuse_nhwc_f32(C.byref(d), _stream()), 'asff_fuse')
    return (out, p) if weights else out


def asff_fuse_backward(dout, rs, vs, r_ups, v_ups, w, bias, p, c, dw, db, *, do_coff=0, drs=(None, None, None), accumulate=(False, False, False),
                       dvs=None):
    """From dout = d fused (slice at do_coff) and the forward's inputs and p: the source gradients dr_i in the sources' own (low-resolution)
    layouts - drs[i] = (tensor, channel offset) to write into, or add to with accumulate[i]; a tensor of its own when None -, the weight maps'
    gradients dv_i likewise (written), and dw (3, 48) / db (3) ACCUMULATED.  -> ([dr_i tensors], [dv_i tensors])."""
    d, (B, H, W) = _asff_desc(rs, vs, r_ups, v_ups, w, bias, c, 'asff_fuse_backward')
    if tuple(dout.shape[:3]) != (B, H, W) or tuple(p.shape) != (B, H, W, 3):
        raise RuntimeError(f'asff_fuse_backward: dout must be ({B}, {H}, {W}, .) and p ({B}, {H}, {W}, 3)')
    dev = dout.device
    drs = [(torch.empty(*rs[i][0].shape[:3], c, device=dev, dtype=torch.float32), 0) if drs[i] is None else drs[i] for i in range(3)]
    dvs = [(torch.empty(*vs[i][0].shape[:3], 16, device=dev, dtype=torch.float32), 0) for i in range(3)] if dvs is None else dvs
    for i in range(3):
        if tuple(drs[i][0].shape[:3]) != tuple(rs[i][0].shape[:3]) or tuple(dvs[i][0].shape[:3]) != tuple(vs[i][0].shape[:3]):
            raise RuntimeError('asff_fuse_backward: a gradient tensor does not have its input\'s map size')
        d.dr[i], d.dv[i], d.dr_accumulate[i] = _slice(*drs[i]), _slice(*dvs[i]), int(accumulate[i])
    ws = torch.empty(_lib.lib().somi_asff_fuse_bwd_workspace_floats(B, H, W), device=dev, dtype=torch.float32)
    d.out, d.p, d.dw, d.db, d.workspace, d.workspace_floats = _slice(dout, do_coff), _ptr(_f32c(p)), _ptr(_f32c(dw)), _ptr(_f32c(db)), _ptr(ws), ws.numel()
    check(_lib.lib().somi_asff_fuse_bwd_nhwc_f32(C.byref(d), _stream()), 'asff_fuse_backward')
    return [t for t, _ in drs], [t for t, _ in dvs]


def _row_tensor(spec, B, n, what):
    """A row tensor of the coordinate-attention kernels -> (Slice, rows per image).  spec: a (B, rows, cs) or (B, rows, 1, cs) tensor, or
    (tensor, channel offset[, first row]): rows [first row, first row + n) of every image are the ones addressed."""
    t, coff, row0 = (tuple(spec) + (0, 0))[:3] if isinstance(spec, (tuple, list)) else (spec, 0, 0)
    if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[2] != 1) or t.shape[0] != B or row0 < 0 or row0 + n > t.shape[1]:
        raise RuntimeError(f'{what}: a ({B}, >= {row0 + n}, cs) row tensor is expected, got {tuple(t.shape)}')
    cs = t.shape[-1]
    return _lib.Slice(_ptr(_f32c(t)) + 4 * row0 * cs, cs, coff), t.shape[1]


def _coordatt_desc(B, H, W, c, a_h=None, a_w=None, what='coordatt'):
    d = _lib.CoordAttDesc()
    d.B, d.H, d.W, d.C = B, H, W, c
    if a_h is not None:
        d.a_h, d.a_h_rows = _row_tensor(a_h, B, H, what + ': a_h')
        d.a_w, d.a_w_rows = _row_tensor(a_w, B, W, what + ': a_w')
    return d


def coordatt_means(x, c, x_coff=0, *, out=None, o_coff=0):
    """The two directional means of slice [x_coff, x_coff + c) of x (B,H,W,cs) -> out (B, H + W, 1, *) slice at o_coff: rows [0, H) the mean over W
    per (b, h, channel), rows [H, H + W) the mean over H per (b, w, channel) - the map coordinate attention's conv1 reads."""
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, H + W, 1, c, device=x.device, dtype=torch.float32)
    _map(out, (B, H + W, 1), 'coordatt_means: output')
    d = _coordatt_desc(B, H, W, c)
    d.x, d.pool = _slice(x, x_coff), _slice(out, o_coff)
    ws = _scratch(d, _lib.lib().somi_coordatt_workspace_floats(d.B, d.H, d.W, d.C), x.device)    # noqa: F841  (alive until the launch is enqueued)
    check(_lib.lib().somi_coordatt_means_nhwc_f32(C.byref(d), _stream()), 'coordatt_means')
    return out


def coordatt_apply(x, a_h, a_w, c, x_coff=0, *, res=None, res_coff=0, out=None, o_coff=0):
    """out = [res +] x * a_h[b,h,:] * a_w[b,w,:] over c channels; a_h / a_w: sigmoided gates as row tensors (_row_tensor)."""
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    _map(out, (B, H, W), 'coordatt_apply: output')
    if res is not None:
        _map(res, (B, H, W), 'coordatt_apply: shortcut')
    d = _coordatt_desc(B, H, W, c, a_h, a_w, 'coordatt_apply')
    d.x, d.y = _slice(x, x_coff), _slice(out, o_coff)
    if res is not None:
        d.res = _slice(res, res_coff)
    check(_lib.lib().somi_coordatt_apply_nhwc_f32(C.byref(d), _stream()), 'coordatt_apply')
    return out


def coordatt_backward_gates(dout, x, a_h, a_w, c, do_coff=0, x_coff=0, *, da_h=None, da_w=None):
    """da_h[b,h,:] = sum_w dout x a_w and da_w[b,w,:] = sum_h dout x a_h, written into the row tensors da_h / da_w ((B,H,c) and (B,W,c) tensors
    of their own when None).  -> (da_h tensor, da_w tensor)."""
    B, H, W, _ = x.shape
    _map(dout, (B, H, W), 'coordatt_backward_gates: dout')
    da_h = torch.empty(B, H, c, device=x.device, dtype=torch.float32) if da_h is None else da_h
    da_w = torch.empty(B, W, c, device=x.device, dtype=torch.float32) if da_w is None else da_w
    d = _coordatt_desc(B, H, W, c, a_h, a_w, 'coordatt_backward_gates')
    d.x, d.y = _slice(x, x_coff), _slice(dout, do_coff)
    d.r_h, d.r_h_rows = _row_tensor(da_h, B, H, 'coordatt_backward_gates: da_h')
    d.r_w, d.r_w_rows = _row_tensor(da_w, B, W, 'coordatt_backward_gates: da_w')
    ws = _scratch(d, _lib.lib().somi_coordatt_workspace_floats(d.B, d.H, d.W, d.C), x.device)    # noqa: F841
    check(_lib.lib().somi_coordatt_bwd_gates_nhwc_f32(C.byref(d), _stream()), 'coordatt_backward_gates')
    first = lambda s: s[0] if isinstance(s, (tuple, list)) else s    # noqa: E731
    return first(da_h), first(da_w)


def coordatt_backward_input(dout, a_h, a_w, gh, gw, c, do_coff=0, *, out=None, dx_coff=0, accumulate=False):
    """dx = dout * a_h * a_w + gh[b,h,:] / W + gw[b,w,:] / H over c channels (gh / gw: the gradients of the two means, row tensors), written into
    out's slice at dx_coff, or added to it with `accumulate`."""
    B, H, W, _ = dout.shape
    if out is None:
        if accumulate:
            raise RuntimeError('coordatt_backward_input: accumulate needs the tensor to add to')
        out = torch.empty(B, H, W, c, device=dout.device, dtype=torch.float32)
    _map(out, (B, H, W), 'coordatt_backward_input: dx')
    d = _coordatt_desc(B, H, W, c, a_h, a_w, 'coordatt_backward_input')
    d.y, d.dx, d.accumulate = _slice(dout, do_coff), _slice(out, dx_coff), int(accumulate)
    d.r_h, d.r_h_rows = _row_tensor(gh, B, H, 'coordatt_backward_input: gh')
    d.r_w, d.r_w_rows = _row_tensor(gw, B, W, 'coordatt_backward_input: gw')
    check(_lib.lib().somi_coordatt_bwd_input_nhwc_f32(C.byref(d), _stream()), 'coordatt_backward_input')
    return out


# ---------------------------------------------------------------------------------------------- EMA (ema.hip)
def ema_partials(B, H, W, c):
    """Partials per (image, channel) of the EMA kernels' reductions over the map at this size (host arithmetic; 0 for bad sizes)."""
    return _lib.lib().somi_ema_partials(int(B), int(H), int(W), int(c))


def _ema_rows(t, B, n, coff, what):
    """sg / dsg: a contiguous (B, H + W, cs) or (B, H + W, 1, cs) tensor -> Slice."""
    if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[2] != 1) or t.shape[0] != B or t.shape[1] != n:
        raise RuntimeError(f'{what}: a ({B}, {n}, cs) tensor is expected, got {tuple(t.shape)}')
    return _lib.Slice(_ptr(_f32c(t)), t.shape[-1], coff)


def _ema_desc(x, c, factor, x_coff, sg, sg_coff, gamma, beta, vec, what, workspace=True):
    B, H, W, _ = x.shape
    cg = c // max(factor, 1)
    if gamma.numel() != cg or beta.numel() != cg:
        raise RuntimeError(f'{what}: gamma and beta hold {gamma.numel()} and {beta.numel()} values, a group has {cg} channels')
    d = _lib.EmaDesc()
    d.B, d.H, d.W, d.C, d.factor = B, H, W, c, factor
    d.x, d.sg = _slice(x, x_coff), _ema_rows(sg, B, H + W, sg_coff, what + ': sg')
    d.gamma, d.beta, d.vec = _ptr(_f32c(gamma)), _ptr(_f32c(beta)), _ptr(_f32c(vec))
    ws = None
    if workspace:
        ws = _scratch(d, _lib.lib().somi_ema_workspace_floats(B, H, W, c), x.device)
    return d, ws


def ema_stats(x, sg, c, factor, gamma, beta, eps, x_coff=0, *, sg_coff=0, x2=None, x2_coff=0):
    """Per (image, channel) of t = x * sg_h[b,h,:] * sg_w[b,w,:]: -> (stats (B, 3, c): mean of t, its sum of squared deviations, the mean of
    x2 (zero without x2); vec (B, 4, c): mean, rstd, x21 = the softmax of the x2 means over each group of c / factor channels, x11 = the
    softmax of beta).  sg (B, H + W, .): the sigmoided gates, rows [0, H) by row and [H, H + W) by column."""
    B = x.shape[0]
    stats = torch.empty(B, 3, c, device=x.device, dtype=torch.float32)
    vec = torch.empty(B, 4, c, device=x.device, dtype=torch.float32)
    d, ws = _ema_desc(x, c, factor, x_coff, sg, sg_coff, gamma, beta, vec, 'ema_stats')     # noqa: F841  (ws alive until the launch is enqueued)
    d.stats, d.eps = _ptr(stats), float(eps)
    if x2 is not None:
        d.x2 = _slice(_map(x2, x, 'ema_stats: a map'), x2_coff)
    _check_impl(_lib.lib().somi_ema_stats_nhwc_f32(C.byref(d), _stream()), 'ema_stats')
    return stats, vec


def ema_gate(x, x2, sg, vec, c, factor, gamma, beta, x_coff=0, *, x2_coff=0, sg_coff=0, res=None, res_coff=0, out=None, o_coff=0):
    """out = [res +] x * sigmoid(wgt), wgt per (image, group, pixel) = sum_j x11[j] x2[j] + x21[j] x1[j] with x1 = gamma * (t - mean) * rstd + beta
    rebuilt from x, sg and vec (ema_stats)."""
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    d, _ = _ema_desc(x, c, factor, x_coff, sg, sg_coff, gamma, beta, vec, 'ema_gate', workspace=False)
    d.x2, d.y = _slice(_map(x2, x, 'ema_gate: a map'), x2_coff), _slice(_map(out, x, 'ema_gate: a map'), o_coff)
    if res is not None:
        d.res = _slice(_map(res, x, 'ema_gate: a map'), res_coff)
    _check_impl(_lib.lib().somi_ema_gate_nhwc_f32(C.byref(d), _stream()), 'ema_gate')
    return out


def ema_backward_gate(dout, x, x2, sg, vec, c, factor, gamma, beta, dgamma, dbeta, do_coff=0, x_coff=0, *, x2_coff=0, sg_coff=0, dx=None,
                      dx_coff=0, accumulate=False, dw=None, dw_coff=0):
    """From dout = d(x * sigmoid(wgt)): dx = dout * sigmoid(wgt) (written, or added with `accumulate`), dw = dwgt over the channels of each group,
    sums (B, 3, c) = sum dwgt * that, sum dwgt, sum dwgt * x2, bvec (B, 3, c) for ema_backward_norm; dgamma / dbeta (c / factor) are ADDED to.
    -> (dx, dw, sums, bvec)."""
    B, H, W, _ = x.shape
    if dx is None:
        if accumulate:
            raise RuntimeError('ema_backward_gate: accumulate needs the tensor to add to')
        dx = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    dw = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32) if dw is None else dw
    sums = torch.empty(B, 3, c, device=x.device, dtype=torch.float32)
    bvec = torch.empty(B, 3, c, device=x.device, dtype=torch.float32)
    d, ws = _ema_desc(x, c, factor, x_coff, sg, sg_coff, gamma, beta, vec, 'ema_backward_gate')     # noqa: F841
    d.x2, d.y = _slice(_map(x2, x, 'ema_backward_gate: a map'), x2_coff), _slice(_map(dout, x, 'ema_backward_gate: a map'), do_coff)
    d.dx, d.dw = _slice(_map(dx, x, 'ema_backward_gate: a map'), dx_coff), _slice(_map(dw, x, 'ema_backward_gate: a map'), dw_coff)
    d.sums, d.bvec, d.dgamma, d.dbeta, d.accumulate = _ptr(sums), _ptr(bvec), _ptr(_f32c(dgamma)), _ptr(_f32c(dbeta)), int(accumulate)
    if dgamma.numel() != gamma.numel() or dbeta.numel() != beta.numel():
        raise RuntimeError('ema_backward_gate: dgamma / dbeta must have gamma\'s / beta\'s size')
    _check_impl(_lib.lib().somi_ema_bwd_gate_nhwc_f32(C.byref(d), _stream()), 'ema_backward_gate')
    return dx, dw, sums, bvec


def ema_backward_norm(x, sg, dw, vec, bvec, c, factor, gamma, beta, x_coff=0, *, sg_coff=0, dw_coff=0, dt=None, dt_coff=0, dsg=None, dsg_coff=0):
    """The instance-norm backward: dt = the gradient of t (written), dw: dwgt -> dx2 = the gradient of conv3x3's output IN PLACE,
    dsg (B, H + W, .) = the gradient of conv1x1's output in front of its sigmoid.  -> (dt, dw, dsg)."""
    B, H, W, _ = x.shape
    dt = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32) if dt is None else dt
    dsg = torch.empty(B, H + W, c, device=x.device, dtype=torch.float32) if dsg is None else dsg
    d, ws = _ema_desc(x, c, factor, x_coff, sg, sg_coff, gamma, beta, vec, 'ema_backward_norm')     # noqa: F841
    d.dw, d.y = _slice(_map(dw, x, 'ema_backward_norm: a map'), dw_coff), _slice(_map(dt, x, 'ema_backward_norm: a map'), dt_coff)
    d.dsg, d.bvec = _ema_rows(dsg, B, H + W, dsg_coff, 'ema_backward_norm: dsg'), _ptr(_f32c(bvec))
    _check_impl(_lib.lib().somi_ema_bwd_norm_nhwc_f32(C.byref(d), _stream()), 'ema_backward_norm')
    return dt, dw, dsg


# ---------------------------------------------------------------------------------------------- ACmix (acmix.hip)
ACMIX_AUX = 24          # floats per pixel acmix_attn_backward_q leaves for acmix_attn_backward_kv (AC_AUX of acmix.hip)


def acmix_plan(H, W):
    """-> (tile, tiles_y, tiles_x): the square pixel tile a workgroup of the attention kernels owns and their count per image (host arithmetic)."""
    t, ny, nx = C.c_int(), C.c_int(), C.c_int()
    check(_lib.lib().somi_acmix_plan(int(H), int(W), C.byref(t), C.byref(ny), C.byref(nx)), 'acmix_plan')
    return t.value, ny.value, nx.value


def _acmix_desc(qkv, c, what, workspace=False):
    """qkv: (tensor, q_coff, k_coff, v_coff) or None.  -> (desc, workspace tensor or None)."""
    d = _lib.AcmixDesc()
    t = qkv[0]
    B, H, W, _ = t.shape
    d.B, d.H, d.W, d.C = B, H, W, c
    if len(qkv) == 4:
        d.q, d.k, d.v = _slice(t, qkv[1]), _slice(t, qkv[2]), _slice(t, qkv[3])
    ws = None
    if workspace:
        ws = _scratch(d, _lib.lib().somi_acmix_workspace_floats(B, H, W, c), t.device)
    return d, ws


def _acmix_qkv(qkv, c):
    """A (B,H,W,.) tensor holding q, k, v side by side from channel `coff` -> (tensor, q_coff, k_coff, v_coff); or the 4-tuple itself."""
    if isinstance(qkv, torch.Tensor):
        return qkv, 0, c, 2 * c
    if len(qkv) == 2:
        return qkv[0], qkv[1], qkv[1] + c, qkv[1] + 2 * c
    return tuple(qkv)


def _acmix_small(t, n, what):
    if t.numel() != n:
        raise RuntimeError(f'{what} holds {t.numel()} values, {n} are expected')
    return _ptr(_f32c(t))


def acmix_fold_weff(fc_w, dep_w, c):
    """fc.weight (9, 12[, 1, 1]) and dep_conv.weight (c, 9, 3, 3) -> weff (12, 9, c / 4, 4): dep_conv(fc(.)) as one grouped 3x3 conv."""
    weff = torch.empty(12, 9, c // 4, 4, device=fc_w.device, dtype=torch.float32)
    _check_impl(_lib.lib().somi_acmix_fold_weff_f32(_acmix_small(fc_w, 108, 'fc.weight'), _acmix_small(dep_w, c * 81, 'dep_conv.weight'), _ptr(weff),
                                                   int(c), _stream()), 'acmix_fold_weff')
    return weff


def acmix_split_dweff(dweff, fc_w, dep_w, c):
    """The gradient of weff -> (dfc (9, 12), ddep (c, 9, 3, 3))."""
    dfc = torch.empty(9, 12, device=dweff.device, dtype=torch.float32)
    ddep = torch.empty(c, 9, 3, 3, device=dweff.device, dtype=torch.float32)
    _check_impl(_lib.lib().somi_acmix_split_dweff_f32(_acmix_small(dweff, 108 * c, 'dweff'), _acmix_small(fc_w, 108, 'fc.weight'),
                                                     _acmix_small(dep_w, c * 81, 'dep_conv.weight'), _ptr(dfc), _ptr(ddep), int(c), _stream()),
               'acmix_split_dweff')
    return dfc, ddep


def acmix_conv(qkv, c, weff, bias, *, out=None, o_coff=0):
    """The conv half: mix[., 4 d + o] = bias + the grouped 3x3 conv of the 12 sources (q, k, v heads) of dim d with weff (acmix_fold_weff)."""
    qkv = _acmix_qkv(qkv, c)
    B, H, W, _ = qkv[0].shape
    if out is None:
        out = torch.empty(B, H, W, c, device=qkv[0].device, dtype=torch.float32)
    d, _ = _acmix_desc(qkv, c, 'acmix_conv')
    d.mix = _slice(_map(out, qkv[0], 'acmix_conv: a map'), o_coff)
    d.weff, d.bias = _acmix_small(weff, 108 * c, 'weff'), _acmix_small(bias, c, 'bias')
    _check_impl(_lib.lib().somi_acmix_conv_nhwc_f32(C.byref(d), _stream()), 'acmix_conv')
    return out


def acmix_attn(qkv, c, wp, rate1, rate2, *, mix=None, mix_coff=0, out=None, o_coff=0, lse=None, lse_coff=0, want_lse=False):
    """out = rate1 * the 7x7 reflected-window attention of q, k, v (4 heads, position term from wp (c / 4, 2)) [+ rate2 * mix].
    -> (out, lse): lse (B, H, W, 4), the per (pixel, head) log-sum-exp, with want_lse or a given lse."""
    qkv = _acmix_qkv(qkv, c)
    x = qkv[0]
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    if lse is None and want_lse:
        lse = torch.empty(B, H, W, 4, device=x.device, dtype=torch.float32)
    d, _ = _acmix_desc(qkv, c, 'acmix_attn')
    d.out = _slice(_map(out, x, 'acmix_attn: a map'), o_coff)
    if mix is not None:
        d.mix = _slice(_map(mix, x, 'acmix_attn: a map'), mix_coff)
    if lse is not None:
        d.lse = _slice(_map(lse, x, 'acmix_attn: a map'), lse_coff)
    d.wp, d.rate1, d.rate2 = _acmix_small(wp, c // 2, 'wp'), _acmix_small(rate1, 1, 'rate1'), _acmix_small(rate2, 1, 'rate2')
    _check_impl(_lib.lib().somi_acmix_attn_nhwc_f32(C.byref(d), _stream()), 'acmix_attn')
    return out, lse


def acmix_attn_backward_q(dout, qkv, c, wp, rate1, rate2, lse, *, do_coff=0, lse_coff=0, mix=None, mix_coff=0, dq=None, dq_coff=0,
                          accumulate=False, aux=None, aux_coff=0):
    """The query-centred backward.  -> (dq, aux, dwp (c / 4, 2), drates (2,): sum dout . att, sum dout . mix); dq added to with `accumulate`."""
    qkv = _acmix_qkv(qkv, c)
    x = qkv[0]
    B, H, W, _ = x.shape
    if dq is None:
        if accumulate:
            raise RuntimeError('acmix_attn_backward_q: accumulate needs the tensor to add to')
        dq = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    if aux is None:
        aux = torch.empty(B, H, W, ACMIX_AUX, device=x.device, dtype=torch.float32)
    dwp = torch.empty(c // 4, 2, device=x.device, dtype=torch.float32)
    drates = torch.empty(2, device=x.device, dtype=torch.float32)
    d, ws = _acmix_desc(qkv, c, 'acmix_attn_backward_q', workspace=True)     # noqa: F841  (ws alive until the launch is enqueued)
    d.out, d.lse = _slice(_map(dout, x, 'acmix_attn_backward_q: a map'), do_coff), _slice(_map(lse, x, 'acmix_attn_backward_q: a map'), lse_coff)
    d.aux, d.dq = _slice(_map(aux, x, 'acmix_attn_backward_q: a map'), aux_coff), _slice(_map(dq, x, 'acmix_attn_backward_q: a map'), dq_coff)
    if mix is not None:
        d.mix = _slice(_map(mix, x, 'acmix_attn_backward_q: a map'), mix_coff)
    d.wp, d.rate1, d.rate2 = _acmix_small(wp, c // 2, 'wp'), _acmix_small(rate1, 1, 'rate1'), _acmix_small(rate2, 1, 'rate2')
    d.dwp, d.drates, d.accumulate = _ptr(dwp), _ptr(drates), int(accumulate)
    _check_impl(_lib.lib().somi_acmix_attn_bwd_q_nhwc_f32(C.byref(d), _stream()), 'acmix_attn_backward_q')
    return dq, aux, dwp, drates


def acmix_attn_backward_kv(dout, qkv, c, wp, rate1, rate2, lse, aux, *, do_coff=0, lse_coff=0, aux_coff=0, dk=None, dk_coff=0, dv=None,
                           dv_coff=0, accumulate=False):
    """The key-centred backward (after acmix_attn_backward_q, whose aux it reads).  -> (dk, dv), added to with `accumulate`."""
    qkv = _acmix_qkv(qkv, c)
    x = qkv[0]
    B, H, W, _ = x.shape
    if (dk is None or dv is None) and accumulate:
        raise RuntimeError('acmix_attn_backward_kv: accumulate needs the tensors to add to')
    dk = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32) if dk is None else dk
    dv = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32) if dv is None else dv
    d, _ = _acmix_desc(qkv, c, 'acmix_attn_backward_kv')
    d.out, d.lse = _slice(_map(dout, x, 'acmix_attn_backward_kv: a map'), do_coff), _slice(_map(lse, x, 'acmix_attn_backward_kv: a map'), lse_coff)
    d.aux = _slice(_map(aux, x, 'acmix_attn_backward_kv: a map'), aux_coff)
    d.dk, d.dv = _slice(_map(dk, x, 'acmix_attn_backward_kv: a map'), dk_coff), _slice(_map(dv, x, 'acmix_attn_backward_kv: a map'), dv_coff)
    d.wp, d.rate1, d.rate2 = _acmix_small(wp, c // 2, 'wp'), _acmix_small(rate1, 1, 'rate1'), _acmix_small(rate2, 1, 'rate2')
    d.accumulate = int(accumulate)
    _check_impl(_lib.lib().somi_acmix_attn_bwd_kv_nhwc_f32(C.byref(d), _stream()), 'acmix_attn_backward_kv')
    return dk, dv


def acmix_conv_backward_data(dout, c, weff, rate2, dqkv, *, do_coff=0, accumulate=False):
    """dq, dk, dv = rate2 * the transposed grouped conv of dout, into dqkv = (tensor, q_coff, k_coff, v_coff) (or a tensor holding them side by
    side), added to with `accumulate`."""
    dqkv = _acmix_qkv(dqkv, c)
    d, _ = _acmix_desc((dqkv[0],), c, 'acmix_conv_backward_data')
    d.out = _slice(_map(dout, dqkv[0], 'acmix_conv_backward_data: a map'), do_coff)
    d.dq, d.dk, d.dv = _slice(dqkv[0], dqkv[1]), _slice(dqkv[0], dqkv[2]), _slice(dqkv[0], dqkv[3])
    d.weff, d.rate2, d.accumulate = _acmix_small(weff, 108 * c, 'weff'), _acmix_small(rate2, 1, 'rate2'), int(accumulate)
    _check_impl(_lib.lib().somi_acmix_conv_bwd_data_nhwc_f32(C.byref(d), _stream()), 'acmix_conv_backward_data')
    return dqkv[0]


def acmix_conv_backward_weight(dout, qkv, c, rate2, *, do_coff=0):
    """-> (dweff (12, 9, c / 4, 4), dbias (c,)): rate2 * the sums over the map, partials folded in a fixed order."""
    qkv = _acmix_qkv(qkv, c)
    x = qkv[0]
    dweff = torch.empty(12, 9, c // 4, 4, device=x.device, dtype=torch.float32)
    dbias = torch.empty(c, device=x.device, dtype=torch.float32)
    d, ws = _acmix_desc(qkv, c, 'acmix_conv_backward_weight', workspace=True)     # noqa: F841
    d.out = _slice(_map(dout, x, 'acmix_conv_backward_weight: a map'), do_coff)
    d.rate2, d.dweff, d.dbias = _acmix_small(rate2, 1, 'rate2'), _ptr(dweff), _ptr(dbias)
    _check_impl(_lib.lib().somi_acmix_conv_bwd_weight_nhwc_f32(C.byref(d), _stream()), 'acmix_conv_backward_weight')
    return dweff, dbias


# ---------------------------------------------------------------------------------------------- SimAM (simam.hip)
SIMAM_MAX_COVER = 4     # regions over one pixel along an axis (SA_COVER of simam.hip)


def simam_grid(mode, H, W, e_lambda=1e-4, target_size=None, stride=None):
    """The region grid of a SimAM module on an H x W map -> (ny, nx, step_y, step_x, len_y, len_x, stretch_last, n, lambda), what the four
    simam_* calls take as `grid`.  mode 'map': one region, n = H W - 1 (SimAM); 'quadrants': rows split at H // 2 and columns at W // 2, the
    second region the larger one on odd sizes, n = (H // 2)(W // 2) - 1 for all four (SimAMWithSlicing); 'windows': target_size x target_size
    windows at `stride`, starting at range(0, H - t + 1, stride) x range(0, W - t + 1, stride), n = t t - 1 (SimAMWithFlexibleSlicing).
    The limits are raised here, by name, before anything is launched."""
    if mode == 'map':
        if H * W < 2:
            raise RuntimeError(f'SimAM on a {H}x{W} map: one pixel has no variance (the reference divides 0 by 0)')
        return (1, 1, H, W, H, W, 0, float(H * W - 1), float(e_lambda))
    if mode == 'quadrants':
        bh, bw = H // 2, W // 2
        if H < 2 or W < 2 or bh * bw < 2:
            raise RuntimeError(f'SimAMWithSlicing on a {H}x{W} map: a quadrant of {bh}x{bw} pixels has no variance (the reference divides 0 by 0)')
        return (2, 2, bh, bw, bh, bw, 1, float(bh * bw - 1), float(e_lambda))
    if mode != 'windows':
        raise ValueError(f"simam_grid: mode {mode!r} (one of 'map', 'quadrants', 'windows')")
    t, st = target_size, stride
    if H < t or W < t:
        raise RuntimeError(f'SimAMWithFlexibleSlicing: a {H}x{W} map is smaller than target_size {t}: no window fits (the reference returns zeros)')
    return ((H - t) // st + 1, (W - t) // st + 1, st, st, t, t, 0, float(t * t - 1), float(e_lambda))


def _simam_desc(x, c, grid, x_coff, stats, what):
    B, H, W, _ = x.shape
    d = _lib.SimamDesc()
    d.B, d.H, d.W, d.C = B, H, W, c
    d.ny, d.nx, d.step_y, d.step_x, d.len_y, d.len_x, d.stretch_last, d.n, d.lam = grid
    d.x = _slice(x, x_coff)
    if stats is not None:
        if tuple(stats.shape) != (B, d.ny * d.nx, 2, c) or not stats.is_contiguous() or stats.dtype != torch.float32:
            raise RuntimeError(f'{what}: a contiguous fp32 ({B}, {d.ny * d.nx}, 2, {c}) tensor is expected, got {tuple(stats.shape)}')
        d.stats = _ptr(stats)
    return d


def simam_stats(x, c, grid, x_coff=0):
    """Per (image, region, channel) of slice [x_coff, x_coff + c) of x (B,H,W,cs): the mean over the region and the sum of squared deviations
    about it -> stats (B, ny * nx, 2, c).  grid: simam_grid(...)."""
    B = x.shape[0]
    stats = torch.empty(B, grid[0] * grid[1], 2, c, device=x.device, dtype=torch.float32)
    d = _simam_desc(x, c, grid, x_coff, stats, 'simam_stats')
    ws = _scratch(d, _lib.lib().somi_simam_workspace_floats(C.byref(d)), x.device)    # noqa: F841  (alive until the launch is enqueued)
    check(_lib.lib().somi_simam_stats_nhwc_f32(C.byref(d), _stream()), 'simam_stats')
    return stats


def simam_apply(x, stats, c, grid, x_coff=0, *, out=None, o_coff=0, add_input=False):
    """out = [x +] sum over the regions covering a pixel of w * x * sigmoid(d^2 / D + 0.5); a pixel no region covers gets 0 [+ x]."""
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    _map(out, (B, H, W), 'simam_apply: output')
    d = _simam_desc(x, c, grid, x_coff, stats, 'simam_apply: stats')
    d.y, d.add_input = _slice(out, o_coff), int(add_input)
    check(_lib.lib().somi_simam_apply_nhwc_f32(C.byref(d), _stream()), 'simam_apply')
    return out


def simam_backward_sums(dout, x, stats, c, grid, do_coff=0, x_coff=0):
    """The two per (image, region, channel) sums of the backward, A = sum T d and B = sum T d^2 with T = w g x s (1 - s) -> sums (B, ny * nx, 2, c)."""
    B, H, W, _ = x.shape
    _map(dout, (B, H, W), 'simam_backward_sums: dout')
    sums = torch.empty_like(stats)
    d = _simam_desc(x, c, grid, x_coff, stats, 'simam_backward_sums: stats')
    d.y, d.sums = _slice(dout, do_coff), _ptr(sums)
    ws = _scratch(d, _lib.lib().somi_simam_workspace_floats(C.byref(d)), x.device)    # noqa: F841
    check(_lib.lib().somi_simam_bwd_sums_nhwc_f32(C.byref(d), _stream()), 'simam_backward_sums')
    return sums


def simam_backward_input(dout, x, stats, sums, c, grid, do_coff=0, x_coff=0, *, out=None, dx_coff=0, accumulate=False, add_input=False):
    """dx = [g +] sum over the covering regions of (w g s + 2 T d / D - 2 A / (N D) - (8 / n) d B / D^2), written into out's slice at dx_coff, or
    added to it with `accumulate`; add_input: the gradient of apply's `x +`."""
    B, H, W, _ = x.shape
    if out is None:
        if accumulate:
            raise RuntimeError('simam_backward_input: accumulate needs the tensor to add to')
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    _map(dout, (B, H, W), 'simam_backward_input: dout')
    _map(out, (B, H, W), 'simam_backward_input: dx')
    d = _simam_desc(x, c, grid, x_coff, stats, 'simam_backward_input: stats')
    if tuple(sums.shape) != tuple(stats.shape) or not sums.is_contiguous() or sums.dtype != torch.float32:
        raise RuntimeError(f'simam_backward_input: sums must be like stats, got {tuple(sums.shape)}')
    d.y, d.dx, d.sums = _slice(dout, do_coff), _slice(out, dx_coff), _ptr(sums)
    d.accumulate, d.add_input = int(accumulate), int(add_input)
    check(_lib.lib().somi_simam_bwd_input_nhwc_f32(C.byref(d), _stream()), 'simam_backward_input')
    return out


# ---------------------------------------------------------------------------------------------- ASF-YOLO neck (asf.hip)
def zoomcat_small_size(size):
    """The size of Zoom_cat's small map along an axis of the middle map's `size`: read at (h >> 1, w >> 1)."""
    return (size + 1) // 2


def zoomcat(l, m, s, cl, cm, cs, l_coff=0, m_coff=0, s_coff=0, *, out=None, o_coff=0, codes=False):
    """Zoom_cat in one launch: out[..., 0:cl] = max2x2(l) + mean2x2(l), [cl:cl+cm] = m, [cl+cm:] = s at (h >> 1, w >> 1), from out's channel
    o_coff.  l (B,2H,2W,.), m (B,H,W,.), s (B,(H+1)//2,(W+1)//2,.).  m=None: the producer has written m's slice of `out` already; `out` must
    then be given.  codes=True (training): -> (out, codes), one byte per (pixel, quad of l's part) for zoomcat_backward."""
    B, H2, W2, _ = l.shape
    H, W = H2 // 2, W2 // 2
    if H2 != 2 * H or W2 != 2 * W:
        raise RuntimeError(f'zoomcat: l must have even sizes, got {tuple(l.shape)}')
    if m is None and out is None:
        raise RuntimeError('zoomcat: m in place needs the output tensor that holds it')
    if m is not None:
        _map(m, (B, H, W), 'zoomcat: m')
    _map(s, (B, zoomcat_small_size(H), zoomcat_small_size(W)), 'zoomcat: s')
    if out is None:
        out = torch.empty(B, H, W, cl + cm + cs, device=l.device, dtype=torch.float32)
    _map(out, (B, H, W), 'zoomcat: out')
    d = _lib.ZoomcatDesc()
    d.B, d.H, d.W, d.Cl, d.Cm, d.Cs = B, H, W, cl, cm, cs
    d.l, d.s, d.out = _slice(l, l_coff), _slice(s, s_coff), _slice(out, o_coff)
    if m is not None:
        d.m = _slice(m, m_coff)
    arg = torch.empty(B, H, W, max(cl // 4, 1), device=l.device, dtype=torch.uint8) if codes else None
    d.codes = _ptr(arg)
    check(_lib.lib().somi_zoomcat_nhwc_f32(C.byref(d), _stream()), 'zoomcat')
    return (out, arg) if codes else out


def zoomcat_backward(dout, codes, cl, cm, cs, do_coff=0, *, dl=True, dm=None, ds=True, accumulate=(False, False, False)):
    """One owner-computes launch: dl[2h+i, 2w+j] = dout_l[h, w] (1/4 + [code == 2i + j]), dm = dout_m, ds = the sum of dout_s over the pixels a
    small-map pixel fed.  Each of dl / dm / ds: None skips it, True makes a tensor, (tensor, channel offset) is written - or added to where
    accumulate[k].  -> (dl, dm, ds) tensors (None where skipped)."""
    B, H, W, _ = dout.shape
    shapes = ((B, 2 * H, 2 * W, cl), (B, H, W, cm), (B, zoomcat_small_size(H), zoomcat_small_size(W), cs))
    d = _lib.ZoomcatDesc()
    d.B, d.H, d.W, d.Cl, d.Cm, d.Cs = B, H, W, cl, cm, cs
    d.out, d.codes = _slice(dout, do_coff), _ptr(codes)
    outs = []
    for k, (name, tgt) in enumerate((('l', dl), ('m', dm), ('s', ds))):
        if tgt is None:
            outs.append(None)
            continue
        if tgt is True:
            if accumulate[k]:
                raise RuntimeError('zoomcat_backward: accumulate needs the tensor to add to')
            tgt = (torch.empty(*shapes[k], device=dout.device, dtype=torch.float32), 0)
        _map(tgt[0], shapes[k][:3], f'zoomcat_backward: d{name}')
        setattr(d, name, _slice(*tgt))
        d.accumulate[k] = int(accumulate[k])
        outs.append(tgt[0])
    if outs[0] is not None and (codes is None or codes.dtype != torch.uint8 or codes.numel() != B * H * W * (cl // 4)):
        raise RuntimeError(f'zoomcat_backward: codes must hold {B * H * W * (cl // 4)} bytes')
    check(_lib.lib().somi_zoomcat_bwd_nhwc_f32(C.byref(d), _stream()), 'zoomcat_backward')
    return tuple(outs)


def _scalseq_desc(us, c, coffs, what):
    u3, u4, u5 = us
    B, H, W, _ = u3.shape
    if H % 4 or W % 4:
        raise RuntimeError(f'{what}: the P3 map must have sizes that are multiples of 4, got {H}x{W}')
    _map(u4, (B, H // 2, W // 2), f'{what}: u4')
    _map(u5, (B, H // 4, W // 4), f'{what}: u5')
    d = _lib.ScalseqDesc()
    d.B, d.H, d.W, d.C = B, H, W, c
    d.u3, d.u4, d.u5 = _slice(u3, coffs[0]), _slice(u4, coffs[1]), _slice(u5, coffs[2])
    return d


def _scalseq_stats_args(d, st):
    d.mean, d.rstd, d.scale, d.shift = (_ptr(_f32c(v)) for v in st)


def scalseq_stats(us, c, gamma, beta, eps, momentum, running_mean=None, running_var=None, coffs=(0, 0, 0)):
    """BatchNorm3d's batch statistics over ScalSeq's virtual (B,C,3,H,W) stack from the three maps us = (u3, u4, u5) at their own resolutions
    (weights 1, 4, 16; N = 3 B H W) -> (mean, rstd, scale, shift); the running statistics move as nn.BatchNorm3d moves them (pivot of the
    partial sums: running_mean)."""
    if SYNC_BN is not None:
        raise NotImplementedError("ScalSeq's BatchNorm3d has no sync-BN form (--sync-bn): its statistics are taken on one rank")
    d = _scalseq_desc(us, c, coffs, 'scalseq_stats')
    dev = us[0].device
    st = tuple(torch.empty(c, device=dev, dtype=torch.float32) for _ in range(4))
    _scalseq_stats_args(d, st)
    d.gamma, d.beta, d.eps, d.momentum = _ptr(_f32c(gamma)), _ptr(_f32c(beta)), float(eps), float(momentum)
    d.running_mean, d.running_var = _ptr(running_mean), _ptr(running_var)
    ws = _scratch(d, _lib.lib().somi_scalseq_workspace_floats(d.B, d.H, d.W, d.C), dev)    # noqa: F841  (alive until the launch is enqueued)
    check(_lib.lib().somi_scalseq_stats_f32(C.byref(d), _stream()), 'scalseq_stats')
    return st


def scalseq_fuse(us, c, scale=None, shift=None, coffs=(0, 0, 0), *, out=None, o_coff=0, codes=False):
    """out = max_i leaky0.1(scale u_i + shift) per P3 pixel, u4 read at (h / 2, w / 2), u5 at (h / 4, w / 4), ties to the first i; scale / shift
    None: 1 and 0.  codes=True: -> (out, codes), one byte per (pixel, quad) for scalseq_route_backward."""
    d = _scalseq_desc(us, c, coffs, 'scalseq_fuse')
    B, H, W, _ = us[0].shape
    if out is None:
        out = torch.empty(B, H, W, c, device=us[0].device, dtype=torch.float32)
    _map(out, (B, H, W), 'scalseq_fuse: out')
    d.out = _slice(out, o_coff)
    if scale is not None:
        d.scale, d.shift = _ptr(_f32c(scale)), _ptr(_f32c(shift))
    arg = torch.empty(B, H, W, c // 4, device=us[0].device, dtype=torch.uint8) if codes else None
    d.codes = _ptr(arg)
    check(_lib.lib().somi_scalseq_fuse_nhwc_f32(C.byref(d), _stream()), 'scalseq_fuse')
    return (out, arg) if codes else out


def scalseq_route_backward(dout, codes, us, c, st, coffs=(0, 0, 0), *, do_coff=0, dgamma=None, dbeta=None):
    """Pass 1 of ScalSeq's backward: dout and the codes read once per 4x4 tile of P3 -> g3, g4, g5 (the routed gradient times the LeakyReLU
    slope, children summed, at the maps' own resolutions) and sums (2, c) = (sum g, sum g xhat); dgamma / dbeta, when given, are ADDED to."""
    d = _scalseq_desc(us, c, coffs, 'scalseq_route_backward')
    B, H, W, _ = us[0].shape
    _map(dout, (B, H, W), 'scalseq_route_backward: dout')
    if codes.dtype != torch.uint8 or codes.numel() != B * H * W * (c // 4):
        raise RuntimeError(f'scalseq_route_backward: codes must hold {B * H * W * (c // 4)} bytes')
    dev = dout.device
    gs = tuple(torch.empty(*u.shape[:3], c, device=dev, dtype=torch.float32) for u in us)
    sums = torch.empty(2, c, device=dev, dtype=torch.float32)
    d.out, d.codes, d.sums = _slice(dout, do_coff), _ptr(codes), _ptr(sums)
    d.g3, d.g4, d.g5 = (_slice(g, 0) for g in gs)
    _scalseq_stats_args(d, st)
    d.dgamma, d.dbeta = _ptr(dgamma), _ptr(dbeta)
    ws = _scratch(d, _lib.lib().somi_scalseq_workspace_floats(d.B, d.H, d.W, d.C), dev)    # noqa: F841
    check(_lib.lib().somi_scalseq_route_bwd_nhwc_f32(C.byref(d), _stream()), 'scalseq_route_backward')
    return gs, sums


def scalseq_apply_backward(gs, us, c, st, sums, coffs=(0, 0, 0), g_coffs=(0, 0, 0)):
    """Pass 2, in place on gs: du_i = scale (g_i - w_i (m1 + xhat_i m2)), w = 1, 4, 16, m1 = sum g / N, m2 = sum g xhat / N.  -> gs."""
    d = _scalseq_desc(us, c, coffs, 'scalseq_apply_backward')
    for g, u in zip(gs, us):
        _map(g, u.shape[:3], 'scalseq_apply_backward: a gradient map')
    d.g3, d.g4, d.g5 = (_slice(g, o) for g, o in zip(gs, g_coffs))
    _scalseq_stats_args(d, st)
    d.sums = _ptr(_f32c(sums))
    check(_lib.lib().somi_scalseq_apply_bwd_f32(C.byref(d), _stream()), 'scalseq_apply_backward')
    return gs


ECA_KMAX = 9            # ECA_KMAX of asf.hip


def eca_kernel_size(channel, b=1, gamma=2):
    """channel_att's kernel size (models/common.py:4361-4362): 3 for 8 to 64 channels, 5 for 128 to 1024."""
    k = int(abs((math.log(channel, 2) + b) / gamma))
    return k if k % 2 else k + 1


def eca_gate(avg, w):
    """gate[b,c] = sigmoid(sum_j w[j] avg[b, c + j - k // 2]), zero-padded: nn.Conv1d(1, 1, k, padding=k // 2, bias=False) along the channels."""
    B, c = avg.shape
    gate = torch.empty_like(avg)
    check(_lib.lib().somi_eca_gate_f32(_ptr(_f32c(avg)), _ptr(_f32c(w)), w.numel(), _ptr(gate), B, c, _stream()), 'eca_gate')
    return gate


def eca_gate_backward(avg, w, gate, dgate):
    """-> (davg (B, c), dw (k)) of eca_gate, both written."""
    B, c = avg.shape
    davg, dw = torch.empty_like(avg), torch.empty(w.numel(), device=avg.device, dtype=torch.float32)
    check(_lib.lib().somi_eca_gate_bwd_f32(_ptr(_f32c(avg)), _ptr(_f32c(w)), w.numel(), _ptr(_f32c(gate)), _ptr(_f32c(dgate)), _ptr(davg), _ptr(dw),
                                           B, c, _stream()), 'eca_gate_backward')
    return davg, dw


def _asfatt_desc(B, H, W, c, workspace_on=None):
    d = _lib.AsfAttDesc()
    d.B, d.H, d.W, d.C = B, H, W, c
    ws = None
    if workspace_on is not None:
        ws = _scratch(d, _lib.lib().somi_asfatt_workspace_floats(B, H, W, c), workspace_on)
    return d, ws


def _gate_check(g, B, c, what):
    if tuple(g.shape) != (B, c):
        raise RuntimeError(f'{what} must be ({B}, {c}), got {tuple(g.shape)}')
    return _ptr(_f32c(g))


def asf_mix_means(x1, x2, gate, c, x1_coff=0, x2_coff=0, *, t=None, t_coff=0, pool=None, p_coff=0):
    """t = x1 * gate[b,c] + x2 written, and pool (B, H + W, 1, .) = the row means and column means of t from the same pass.  -> (t, pool)."""
    B, H, W, _ = x1.shape
    _map(x2, (B, H, W), 'asf_mix_means: x2')
    if t is None:
        t = torch.empty(B, H, W, c, device=x1.device, dtype=torch.float32)
    if pool is None:
        pool = torch.empty(B, H + W, 1, c, device=x1.device, dtype=torch.float32)
    _map(t, (B, H, W), 'asf_mix_means: t')
    _map(pool, (B, H + W, 1), 'asf_mix_means: pool')
    d, ws = _asfatt_desc(B, H, W, c, x1.device)                   # noqa: F841  (alive until the launch is enqueued)
    d.x1, d.x2, d.t, d.pool, d.gate = _slice(x1, x1_coff), _slice(x2, x2_coff), _slice(t, t_coff), _slice(pool, p_coff), _gate_check(gate, B, c, 'gate')
    check(_lib.lib().somi_asf_mix_means_nhwc_f32(C.byref(d), _stream()), 'asf_mix_means')
    return t, pool


def asf_mix_backward_sums(dt, x1, c, dt_coff=0, x1_coff=0):
    """ds[b,c] = sum over the pixels of dt * x1: the gradient of the gate."""
    B, H, W, _ = x1.shape
    _map(dt, (B, H, W), 'asf_mix_backward_sums: dt')
    ds = torch.empty(B, c, device=x1.device, dtype=torch.float32)
    d, ws = _asfatt_desc(B, H, W, c, x1.device)                   # noqa: F841
    d.x1, d.t, d.ds = _slice(x1, x1_coff), _slice(dt, dt_coff), _ptr(ds)
    check(_lib.lib().somi_asf_mix_bwd_sums_nhwc_f32(C.byref(d), _stream()), 'asf_mix_backward_sums')
    return ds


def asf_mix_backward_input(dt, gate, davg, c, dt_coff=0, *, out=None, dx_coff=0, accumulate=False):
    """dx1 = dt * gate + davg / (H W), written into out's slice at dx_coff, or added to it with `accumulate`."""
    B, H, W, _ = dt.shape
    if out is None:
        if accumulate:
            raise RuntimeError('asf_mix_backward_input: accumulate needs the tensor to add to')
        out = torch.empty(B, H, W, c, device=dt.device, dtype=torch.float32)
    _map(out, (B, H, W), 'asf_mix_backward_input: dx1')
    d, _ = _asfatt_desc(B, H, W, c)
    d.t, d.dx1, d.accumulate = _slice(dt, dt_coff), _slice(out, dx_coff), int(accumulate)
    d.gate, d.davg = _gate_check(gate, B, c, 'gate'), _gate_check(davg, B, c, 'davg')
    check(_lib.lib().somi_asf_mix_bwd_input_nhwc_f32(C.byref(d), _stream()), 'asf_mix_backward_input')
    return out


# ---------------------------------------------------------------------------------------------- CPCA strips (cpca.hip)
CPCA_TAPS = (7, 11, 21)


def _cpca_slice(spec):
    """tensor, or (tensor, channel offset) -> Slice."""
    t, coff = spec if isinstance(spec, (tuple, list)) else (spec, 0)
    return _slice(t, coff)


def _cpca_vec(t, n, what):
    """A parameter-shaped device tensor of n floats (any view of contiguous memory: (C,1,1,k), (C,1,k,1), (C,k), (C,))."""
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise RuntimeError(f'{what}: {n} contiguous fp32 values are expected, got {tuple(t.shape)} {t.dtype}')
    return _ptr(t)


def _cpca_strip_desc(shape, c, ws, biases, axis, flip, taps, what):
    B, H, W, _ = shape
    taps = tuple(int(k) for k in taps)
    d = _lib.CpcaStripDesc()
    d.B, d.H, d.W, d.C, d.axis, d.flip = B, H, W, c, {'w': 0, 'h': 1}[axis], int(bool(flip))
    biases = (None, None, None) if biases is None else biases
    for k in range(3):
        d.taps[k] = taps[k]
        d.w[k] = _cpca_vec(ws[k], c * taps[k], f'{what}: taps {k}')
        d.bias[k] = _cpca_vec(biases[k], c, f'{what}: bias {k}')
    return d


def cpca_fanout(x, ws, biases, c, x_coff=0, *, axis, flip=False, outs=None, taps=CPCA_TAPS):
    """The three strip convs of one tensor: outs[k] = S_k(x) [+ biases[k]], S_k the depthwise conv of taps[k] taps along `axis` ('w' or 'h', zero
    padding k // 2) with the (c, k) weights ws[k], walked backwards with `flip`.  x is read once.  outs: three tensors or (tensor, channel
    offset) pairs (new (B,H,W,c) tensors when None).  -> the three tensors."""
    B, H, W, _ = x.shape
    outs = [torch.empty(B, H, W, c, device=x.device, dtype=torch.float32) for _ in range(3)] if outs is None else list(outs)
    d = _cpca_strip_desc(x.shape, c, ws, biases, axis, flip, taps, 'cpca_fanout')
    d.src[0] = _slice(x, x_coff)
    for k in range(3):
        d.dst[k] = _cpca_slice(outs[k])
    check(_lib.lib().somi_cpca_fanout_nhwc_f32(C.byref(d), _stream()), 'cpca_fanout')
    return [o[0] if isinstance(o, (tuple, list)) else o for o in outs]


def cpca_fanin(ts, through, ws, biases, c, *, axis, flip=False, out=None, o_coff=0, accumulate=False, taps=CPCA_TAPS):
    """out = [out +] through + sum_k (S_k(ts[k]) [+ biases[k]]): the three branches closed by their second strip conv and summed with the
    pass-through tensor in one pass.  ts / through: tensors or (tensor, channel offset) pairs."""
    first = ts[0][0] if isinstance(ts[0], (tuple, list)) else ts[0]
    B, H, W, _ = first.shape
    if out is None:
        if accumulate:
            raise RuntimeError('cpca_fanin: accumulate needs the tensor to add to')
        out = torch.empty(B, H, W, c, device=first.device, dtype=torch.float32)
    d = _cpca_strip_desc(first.shape, c, ws, biases, axis, flip, taps, 'cpca_fanin')
    for k in range(3):
        d.src[k] = _cpca_slice(ts[k])
    d.src[3], d.dst[0], d.accumulate = _cpca_slice(through), _slice(out, o_coff), int(accumulate)
    check(_lib.lib().somi_cpca_fanin_nhwc_f32(C.byref(d), _stream()), 'cpca_fanin')
    return out


def cpca_wgrad(u, ts, ds, dts, c, dw_h, dw_v, db_h, db_v, *, accumulate=False, taps=CPCA_TAPS):
    """All strip weight and bias gradients of s = u + sum_k V_k(H_k(u)) in one call: dw_h[k] (c, k) from (dts[k], u), dw_v[k] from (ds, ts[k]),
    db_h[k] = sum dts[k], db_v[k] = sum ds; written into the given contiguous fp32 tensors (any of them None: skipped), added with `accumulate`.
    u, ts[k], ds, dts[k]: tensors or (tensor, channel offset) pairs."""
    first = u[0] if isinstance(u, (tuple, list)) else u
    B, H, W, _ = first.shape
    taps = tuple(int(k) for k in taps)
    d = _lib.CpcaWgradDesc()
    d.B, d.H, d.W, d.C, d.accumulate = B, H, W, c, int(accumulate)
    d.u, d.ds = _cpca_slice(u), _cpca_slice(ds)
    for k in range(3):
        d.taps[k] = taps[k]
        d.t[k], d.dt[k] = _cpca_slice(ts[k]), _cpca_slice(dts[k])
        d.dw_h[k], d.dw_v[k] = _cpca_vec(dw_h[k], c * taps[k], 'cpca_wgrad: dw_h'), _cpca_vec(dw_v[k], c * taps[k], 'cpca_wgrad: dw_v')
        d.db_h[k], d.db_v[k] = _cpca_vec(db_h[k], c, 'cpca_wgrad: db_h'), _cpca_vec(db_v[k], c, 'cpca_wgrad: db_v')
    ws = _scratch(d, _lib.lib().somi_cpca_wgrad_workspace_floats(B, H, W, c), first.device)
    check(_lib.lib().somi_cpca_wgrad_nhwc_f32(C.byref(d), _stream()), 'cpca_wgrad')


def cpca_gate(x, y, c, x_coff=0, y_coff=0, *, out=None, o_coff=0):
    """out = x * y over c channels (CPCA's conv(s) * a)."""
    if out is None:
        out = torch.empty(*x.shape[:3], c, device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_cpca_gate_nhwc_f32(_slice(x, x_coff), _slice(y, y_coff), _slice(out, o_coff), _npix(x), c, _stream()), 'cpca_gate')
    return out


def cpca_gate_backward(dout, x, y, c, do_coff=0, x_coff=0, y_coff=0):
    """-> (dx, dy) = (dout * y, dout * x), new (B,H,W,c) tensors."""
    dx = torch.empty(*x.shape[:3], c, device=x.device, dtype=torch.float32)
    dy = torch.empty_like(dx)
    check(_lib.lib().somi_cpca_gate_bwd_nhwc_f32(_slice(dout, do_coff), _slice(x, x_coff), _slice(y, y_coff), _slice(dx, 0), _slice(dy, 0),
                                                 _npix(x), c, _stream()), 'cpca_gate_backward')
    return dx, dy


def cpca_sigmoid2(z):
    """z (2B, C): the shared MLP's output on the average rows, then on the maximum rows -> g (B, C) = sigmoid(z[:B]) + sigmoid(z[B:])."""
    B, c = z.shape[0] // 2, z.shape[1]
    g = torch.empty(B, c, device=z.device, dtype=torch.float32)
    check(_lib.lib().somi_cpca_sigmoid2_f32(_ptr(_f32c(z)), _ptr(g), B, c, _stream()), 'cpca_sigmoid2')
    return g


def cpca_sigmoid2_backward(z, dg):
    dz = torch.empty_like(z)
    check(_lib.lib().somi_cpca_sigmoid2_bwd_f32(_ptr(_f32c(z)), _ptr(_f32c(dg)), _ptr(dz), dg.shape[0], dg.shape[1], _stream()),
          'cpca_sigmoid2_backward')
    return dz


def argmax_pixel(x, mx, c, x_coff=0):
    """(B, c) int32: the first pixel of every channel's spatial maximum mx (global_pool's) in slice [x_coff, x_coff + c) of x."""
    B, H, W, _ = x.shape
    out = torch.empty(B, c, device=x.device, dtype=torch.int32)
    check(_lib.lib().somi_cpca_argmax_pixel_nhwc_f32(_slice(x, x_coff), _ptr(_f32c(mx)), _ptr(out), B, H * W, c, _stream()), 'argmax_pixel')
    return out


# ---------------------------------------------------------------------------------------------- tail attention of the CBAM C3 family (cbam_c3.hip)
GATE_MODES = {'product': 0, 'sigmoid_sum': 1}     # SOMI_GATE_PRODUCT, SOMI_GATE_SIGMOID_SUM


def _gate_args(t, ca, sa, c, what):
    B, H, W, _ = t.shape
    if tuple(ca.shape) != (B, c) or tuple(sa.shape) != (B, H, W):
        raise RuntimeError(f'{what}: ca must be ({B}, {c}) and sa ({B}, {H}, {W}), got {tuple(ca.shape)} and {tuple(sa.shape)}')
    return B, H * W, _ptr(_f32c(ca)), _ptr(_f32c(sa))


def gate_combine(t, ca, sa, c, mode, t_coff=0, *, residual=None, res_coff=0, out=None, o_coff=0):
    """out = t * ca * sa (mode 'product') or sigmoid(t * (ca + sa)) ('sigmoid_sum'), + residual when given, over the channel slices
    [coff, coff + c) of t / residual / out; ca (B, c), sa (B, H, W).  -> out (a new (B,H,W,c) tensor when None)."""
    B, HW, pca, psa = _gate_args(t, ca, sa, c, 'gate_combine')
    if out is None:
        out = torch.empty(*t.shape[:3], c, device=t.device, dtype=torch.float32)
    res = _NO_SLICE if residual is None else _slice(_map(residual, t, 'gate_combine: residual'), res_coff)
    check(_lib.lib().somi_gate_combine_nhwc_f32(_slice(t, t_coff), pca, psa, res, _slice(_map(out, t, 'gate_combine: out'), o_coff), B, HW, c,
                                                GATE_MODES[mode], _stream()), 'gate_combine')
    return out


def gate_combine_backward_pixel(dout, t, ca, sa, c, mode, do_coff=0, t_coff=0, *, t_max=None, logit=False):
    """The per-pixel half of gate_combine's backward -> (dsa (B,H,W): the gradient of sa, times sa * (1 - sa) with `logit`; amaxc (B,H,W)
    int32: the first channel of every pixel's maximum of t * ca; amaxp (B, c) int32: the first pixel of every (image, channel) maximum of t,
    found from t_max (B, c), the maxima global_pool took - None without t_max)."""
    B, HW, pca, psa = _gate_args(t, ca, sa, c, 'gate_combine_backward_pixel')
    dsa = torch.empty(*t.shape[:3], device=t.device, dtype=torch.float32)
    amaxc = torch.empty(*t.shape[:3], device=t.device, dtype=torch.int32)
    amaxp = None if t_max is None else torch.empty(B, c, device=t.device, dtype=torch.int32)
    check(_lib.lib().somi_gate_combine_bwd_pixel_f32(_slice(_map(dout, t, 'gate_combine_backward_pixel: dout'), do_coff), _slice(t, t_coff), pca, psa,
                                                     None if t_max is None else _ptr(_f32c(t_max)), _ptr(dsa), _ptr(amaxc), _ptr(amaxp), B, HW, c,
                                                     GATE_MODES[mode], int(logit), _stream()), 'gate_combine_backward_pixel')
    return dsa, amaxc, amaxp


def gate_combine_backward_chan(dout, t, ca, sa, dstats, amaxc, c, mode, do_coff=0, t_coff=0, *, dt=None, dt_coff=0, accumulate=False):
    """The per-element half: dstats (B,H,W,2) = the gradient of [mean_c, max_c] of t * ca from the spatial gate's backward.  -> (dt, dca): dt the
    gradient of t through both gates and the statistics, written into slice dt_coff of `dt` (a new (B,H,W,c) tensor when None; added to it
    with `accumulate`), dca (B, c) the gradient of the channel gate."""
    B, HW, pca, psa = _gate_args(t, ca, sa, c, 'gate_combine_backward_chan')
    if dt is None:
        if accumulate:
            raise RuntimeError('gate_combine_backward_chan: accumulate needs the tensor to add to')
        dt = torch.empty(*t.shape[:3], c, device=t.device, dtype=torch.float32)
    dca = torch.empty(B, c, device=t.device, dtype=torch.float32)
    L = _lib.lib()
    ws = torch.empty(max(L.somi_gate_combine_bwd_workspace_floats(B, HW, c), 4), device=t.device, dtype=torch.float32)
    check(L.somi_gate_combine_bwd_chan_f32(_slice(_map(dout, t, 'gate_combine_backward_chan: dout'), do_coff), _slice(t, t_coff), pca, psa,
                                           _ptr(_f32c(dstats)), _ptr(amaxc), _slice(_map(dt, t, 'gate_combine_backward_chan: dt'), dt_coff), _ptr(dca),
                                           _ptr(ws), ws.numel(), B, HW, c, GATE_MODES[mode], int(accumulate), _stream()), 'gate_combine_backward_chan')
    return dt, dca


def spatial_attn_backward(dlogit, stats, w, k, dw, db, dw_chw=True):
    """Step B of train_blocks.hip on its own: dlogit (B,H,W) = the gradient of the k x k gate conv's output, stats (B,H,W,2) its input, w the
    [k][k][2] packed weight.  -> dstats (B,H,W,2); dw ((1,2,k,k) with dw_chw, else [k][k][2]) and db are accumulated."""
    B, H, W, _ = stats.shape
    dstats = torch.empty_like(stats)
    ws = torch.empty(((B * H * W + 511) // 512) * (2 * k * k + 1), device=stats.device, dtype=torch.float32)
    check(_lib.lib().somi_spatial_attn_bwd_f32(_ptr(_f32c(dlogit)), _ptr(_f32c(stats)), _ptr(w), _ptr(dstats), _ptr(dw), _ptr(db), _ptr(ws), B, H, W, k,
                                               int(dw_chw), _stream()), 'spatial_attn_bwd')
    return dstats


def _dwc_ws(B, H, W, k, dev):
    return torch.empty(max(_lib.lib().somi_dwc_gate_workspace_floats(B, H, W, k), 4), device=dev, dtype=torch.float32)


def dwc_gate_eval(stats, params, run, k, eps):
    """The depthwise-separable spatial gate with running statistics: stats (B,H,W,2) -> sa (B,H,W), one launch.  params: 2 k k + 11 floats,
    run: 6 (somi_dwc_gate_eval_f32)."""
    B, H, W, _ = stats.shape
    sa = torch.empty(B, H, W, device=stats.device, dtype=torch.float32)
    check(_lib.lib().somi_dwc_gate_eval_f32(_ptr(_f32c(stats)), _ptr(_f32c(params)), _ptr(_f32c(run)), _ptr(sa), B, H, W, k, float(eps), _stream()),
          'dwc_gate_eval')
    return sa


def dwc_gate_train(stats, params, run, k, eps, momentum):
    """The gate with batch statistics -> (sa, u (B,H,W,2), p (B,H,W), st (8)): what backward needs; `run` (6 floats, or None) is moved in place."""
    B, H, W, _ = stats.shape
    if B * H * W == 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {(B, 2, H, W)}')
    dev = stats.device
    sa, u = torch.empty(B, H, W, device=dev, dtype=torch.float32), torch.empty(B, H, W, 2, device=dev, dtype=torch.float32)
    p, st = torch.empty(B, H, W, device=dev, dtype=torch.float32), torch.zeros(8, device=dev, dtype=torch.float32)
    ws = _dwc_ws(B, H, W, k, dev)
    check(_lib.lib().somi_dwc_gate_train_f32(_ptr(_f32c(stats)), _ptr(_f32c(params)), _ptr(u), _ptr(p), _ptr(st), _ptr(run), float(momentum),
                                             float(eps), _ptr(sa), _ptr(ws), ws.numel(), B, H, W, k, _stream()), 'dwc_gate_train')
    return sa, u, p, st


def dwc_gate_backward(dsa, stats, u, p, st, params, k, dparams):
    """dsa: the RAW gradient of sa (B,H,W) -> dstats (B,H,W,2); the parameter gradients are added to dparams (the layout of params)."""
    B, H, W, _ = stats.shape
    dstats = torch.empty_like(stats)
    ws = _dwc_ws(B, H, W, k, stats.device)
    check(_lib.lib().somi_dwc_gate_bwd_f32(_ptr(_f32c(dsa)), _ptr(_f32c(stats)), _ptr(_f32c(u)), _ptr(_f32c(p)), _ptr(st), _ptr(_f32c(params)),
                                           _ptr(dstats), _ptr(_f32c(dparams)), _ptr(ws), ws.numel(), B, H, W, k, _stream()), 'dwc_gate_backward')
    return dstats


def _spp_k(k):
    k = [int(v) for v in k]
    return [len(k)] + (k + [0, 0, 0])[:3]


def spp_pool_(buf, c, k, x_coff=0, codes=False):
    """The parallel stride-1 max-pools of slice [x_coff, x_coff + c), one per window size in `k` (ascending odd sizes 3..13, at most 3), into the next
    len(k) slices of `buf`, in one pass.  codes=True (training): -> (buf, codes) with the first row-major maximum of every full window, for
    spp_pool_backward_."""
    B, H, W, cs = buf.shape
    arg = torch.empty(len(k) * B * H * W * c, device=buf.device, dtype=torch.uint8) if codes else None
    check(_lib.lib().somi_spp_pool_nhwc_f32(_ptr(_f32c(buf)), _ptr(arg), B, H, W, c, cs, x_coff, *_spp_k(k), _stream()), 'spp_pool')
    return (buf, arg) if codes else buf


def spp_pool_backward_(dbuf, codes, c, k, x_coff=0):
    """Slice [x_coff, x_coff + c) of dbuf += the gradients of the len(k) pooled slices behind it, routed by spp_pool_'s codes."""
    B, H, W, cs = dbuf.shape
    if codes.dtype != torch.uint8 or codes.numel() != len(k) * B * H * W * c:
        raise RuntimeError(f'spp_pool_backward_: codes must be the {len(k) * B * H * W * c} bytes spp_pool_(codes=True) returned')
    check(_lib.lib().somi_spp_pool_bwd_nhwc_f32(_ptr(codes), _ptr(_f32c(dbuf)), B, H, W, c, cs, x_coff, *_spp_k(k), _stream()), 'spp_pool_backward')
    return dbuf


def _up_out(x, c, out, what):
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, 2 * H, 2 * W, c, device=x.device, dtype=torch.float32)
    _map(out, (B, 2 * H, 2 * W), f'{what}: output')
    return out


def carafe(x, logits, c, k_up, x_coff=0, l_coff=0, *, out=None, y_coff=0, weights=False):
    """CARAFE's reassembly (models/common.py:4482-4489) of slice [x_coff, x_coff + c) of x (B,H,W,cs) by the 4 * k_up^2 encoder logits in slice
    [l_coff, ...) of `logits` (B,H,W,*) -> out (B,2H,2W,*) slice at y_coff.  weights=True (training): -> (out, weights), the softmax weights
    (B,2H,2W,k_up^2) carafe_backward needs - nothing else is kept."""
    B, H, W, _ = x.shape
    _map(logits, (B, H, W), 'carafe: logits')
    out = _up_out(x, c, out, 'carafe')
    wts = torch.empty(B, 2 * H, 2 * W, k_up * k_up, device=x.device, dtype=torch.float32) if weights else None
    check(_lib.lib().somi_carafe_nhwc_f32(_ptr(_f32c(x)), _ptr(_f32c(logits)), _ptr(_f32c(out)), _ptr(wts), B, H, W, c, int(k_up), x.shape[3], x_coff,
                                          logits.shape[3], l_coff, out.shape[3], y_coff, _stream()), 'carafe')
    return (out, wts) if weights else out


def carafe_backward(dy, x, weights, c, k_up, dy_coff=0, x_coff=0, *, out=None, dx_coff=0, dlogits=None, dl_coff=0):
    """-> (dx, dlogits): dx (B,H,W,*) slice at dx_coff, written (not added), and the gradient of the encoder logits (B,H,W,*) slice at dl_coff in the
    logits' own channel layout, from dy (B,2H,2W,*), x and carafe's softmax weights.  Owner-computes, fixed order, no float atomics."""
    B, H, W, _ = x.shape
    kk = int(k_up) * int(k_up)
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    if dlogits is None:
        dlogits = torch.empty(B, H, W, 4 * kk, device=x.device, dtype=torch.float32)
    if (tuple(dy.shape[:3]) != (B, 2 * H, 2 * W) or tuple(out.shape[:3]) != (B, H, W) or tuple(dlogits.shape[:3]) != (B, H, W) or
            tuple(weights.shape) != (B, 2 * H, 2 * W, kk)):
        raise RuntimeError(f'carafe_backward: dy must be ({B}, {2 * H}, {2 * W}, .), dx and dlogits ({B}, {H}, {W}, .), weights ({B}, {2 * H}, {2 * W}, {kk})')
    check(_lib.lib().somi_carafe_bwd_nhwc_f32(_ptr(_f32c(dy)), _ptr(_f32c(x)), _ptr(_f32c(weights)), _ptr(_f32c(out)), _ptr(_f32c(dlogits)), B, H, W, c,
                                              int(k_up), dy.shape[3], dy_coff, x.shape[3], x_coff, out.shape[3], dx_coff, dlogits.shape[3], dl_coff,
                                              _stream()), 'carafe_backward')
    return out, dlogits


_DYS_LAST = None         # the far-tap word of the last dysample_backward (device int32)
_DYS_FAR = {}            # device -> int64 device counter: far taps of every dysample_backward since the last reset


def dysample_far_taps(total=False):
    """FAR bilinear corners of DySample's backward - those added to dx as fp32 atomics because they landed more than 2 pixels from their source pixel
    (0 <=> bit-reproducible), the policy of dcn_overflow_taps.  Default: the last call only (None before any).  total=True: summed over every call on
    every device since reset_dysample_far_taps().  Host sync; diagnostics / tests."""
    if total:
        return int(sum(int(t.item()) for t in _DYS_FAR.values()))
    return None if _DYS_LAST is None else int(_DYS_LAST.item())


def reset_dysample_far_taps():
    for t in _DYS_FAR.values():
        t.zero_()


def _dysample_args(x, offset, init_pos, c, groups, what):
    B, H, W, _ = x.shape
    _map(offset, (B, H, W), f'{what}: offset')
    if init_pos.numel() != 8 * groups or init_pos.dtype != torch.float32 or not init_pos.is_contiguous():
        raise RuntimeError(f'{what}: init_pos must hold {8 * groups} contiguous float32 values')
    if c % groups or (c // groups) % 4:
        raise RuntimeError(f'{what}: needs c % groups == 0 and (c / groups) % 4 == 0, got c={c}, groups={groups}')
    return B, H, W


def dysample(x, offset, init_pos, c, groups, x_coff=0, f_coff=0, *, out=None, y_coff=0):
    """DySample's 'lp' sampling (models/common.py:4277-4296) of slice [x_coff, x_coff + c) of x (B,H,W,cs) at the positions the RAW offset-conv output in
    slice [f_coff, f_coff + 8 * groups) of `offset` gives (the 0.25, init_pos, the border clamp and the pixel shuffle happen in the kernel)
    -> out (B,2H,2W,*) slice at y_coff."""
    B, H, W = _dysample_args(x, offset, init_pos, c, groups, 'dysample')
    out = _up_out(x, c, out, 'dysample')
    check(_lib.lib().somi_dysample_nhwc_f32(_ptr(_f32c(x)), _ptr(_f32c(offset)), _ptr(init_pos), _ptr(_f32c(out)), B, H, W, c, int(groups), x.shape[3],
                                            x_coff, offset.shape[3], f_coff, out.shape[3], y_coff, _stream()), 'dysample')
    return out


def dysample_backward(dy, x, offset, init_pos, c, groups, dy_coff=0, x_coff=0, f_coff=0, *, out=None, dx_coff=0, doffset=None, df_coff=0):
    """-> (dx, doffset): dx (B,H,W,*) slice at dx_coff, written (not added), and the gradient of the raw offset-conv output (B,H,W,*) slice at df_coff in
    its own layout (0.25 included, 0 where the coordinate was clamped).  dx is owner-computes up to 2 pixels of reach; corners beyond go through fp32
    atomics and are counted (dysample_far_taps)."""
    global _DYS_LAST
    B, H, W = _dysample_args(x, offset, init_pos, c, groups, 'dysample_backward')
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    if doffset is None:
        doffset = torch.empty(B, H, W, 8 * groups, device=x.device, dtype=torch.float32)
    if tuple(dy.shape[:3]) != (B, 2 * H, 2 * W) or tuple(out.shape[:3]) != (B, H, W) or tuple(doffset.shape[:3]) != (B, H, W):
        raise RuntimeError(f'dysample_backward: dy must be ({B}, {2 * H}, {2 * W}, .), dx and doffset ({B}, {H}, {W}, .)')
    far = torch.zeros(1, device=x.device, dtype=torch.int32)
    check(_lib.lib().somi_dysample_bwd_nhwc_f32(_ptr(_f32c(dy)), _ptr(_f32c(x)), _ptr(_f32c(offset)), _ptr(init_pos), _ptr(_f32c(out)),
                                                _ptr(_f32c(doffset)), _ptr(far), B, H, W, c, int(groups), dy.shape[3], dy_coff, x.shape[3], x_coff,
                                                offset.shape[3], f_coff, out.shape[3], dx_coff, doffset.shape[3], df_coff, _stream()),
          'dysample_backward')
    _DYS_LAST = far
    tot = _DYS_FAR.get(x.device)
    if tot is None:
        tot = _DYS_FAR[x.device] = torch.zeros(1, dtype=torch.int64, device=x.device)
    tot.add_(far)
    return out, doffset


def bifpn(srcs, ups, w_dev, eps=1e-4, out=None):
    """y = sum_i w_i / (sum_j swish(w_j) + eps) * src_i; `w_dev` is the raw fusion parameter on the device."""
    n = len(srcs)
    B, H, W, Cc = srcs[0].shape
    H, W = H << ups[0], W << ups[0]
    out = torch.empty(B, H, W, Cc, device=srcs[0].device, dtype=torch.float32) if out is None else out
    ptrs = (C.c_void_p * n)(*[_ptr(_f32c(s)) for s in srcs])
    check(_lib.lib().somi_bifpn_nhwc_f32(ptrs, (C.c_int * n)(*ups), _ptr(_f32c(w_dev)), float(eps), n, _ptr(out),
                                         B, H, W, Cc, _stream()), 'bifpn')
    return out


def global_pool(x, c=None, x_coff=0, want_max=True, out=None):
    """out: a contiguous (2B, c) tensor whose halves receive the averages and the maxima (CPCA's shared MLP reads both as one batch)."""
    B, H, W, cs = x.shape
    c = cs - x_coff if c is None else c
    nchunk = _lib.lib().somi_pool_nchunk(H * W)
    ws = torch.empty(2 * B * nchunk * c, device=x.device, dtype=torch.float32)
    if out is not None:
        if tuple(out.shape) != (2 * B, c) or out.dtype != torch.float32 or not out.is_contiguous() or not want_max:
            raise RuntimeError(f'global_pool: out must be a contiguous fp32 ({2 * B}, {c}) tensor and takes both pools, got {tuple(out.shape)} '
                               f'{out.dtype}, want_max={want_max}')
        avg, mx = out[:B], out[B:]
    else:
        avg = torch.empty(B, c, device=x.device, dtype=torch.float32)
        mx = torch.empty(B, c, device=x.device, dtype=torch.float32) if want_max else None
    check(_lib.lib().somi_global_pool_nhwc_f32(_ptr(_f32c(x)), cs, x_coff, B, H * W, c, _ptr(avg), _ptr(mx), _ptr(ws),
                                               _stream()), 'global_pool')
    return avg, mx


def global_pool_act(x, act, post_scale=None, post_shift=None, c=None, x_coff=0):
    """(B, c): post_scale * mean over pixels of act(x) + post_shift - the global average of an activation + per-channel affine map of x without
    writing that tensor (somi_global_pool_act_nhwc_f32)."""
    B, H, W, cs = x.shape
    c = cs - x_coff if c is None else c
    L = _lib.lib()
    ws = torch.empty(2 * B * L.somi_pool_nchunk(H * W) * c, device=x.device, dtype=torch.float32)
    avg = torch.empty(B, c, device=x.device, dtype=torch.float32)
    check(L.somi_global_pool_act_nhwc_f32(_ptr(_f32c(x)), cs, x_coff, B, H * W, c, ACT[act], _ptr(post_scale), _ptr(post_shift), _ptr(avg), _ptr(ws),
                                          _stream()), 'global_pool_act')
    return avg


def affine_silu_pool(x, c, x_coff, scale, shift, out, out_coff=0):
    """out = silu(x * scale + shift) and the global average / max pools of it per (image, channel) in one pass; -> (avg, max) (B, c), or None when
    the kernel does not cover the width (c / 4 must divide 256 or be a multiple of it) - the caller then runs the two separate passes."""
    B, H, W, _ = x.shape
    L = _lib.lib()
    rows = L.somi_affine_silu_pool_rows(B, H * W, c)
    if rows <= 0:
        return None
    ws = torch.empty(2 * B * rows * c, device=x.device, dtype=torch.float32)
    avg = torch.empty(B, c, device=x.device, dtype=torch.float32)
    mx = torch.empty(B, c, device=x.device, dtype=torch.float32)
    check(L.somi_affine_silu_pool_nhwc_f32(_ptr(_f32c(x)), x.shape[3], x_coff, _ptr(scale), _ptr(shift), _ptr(_f32c(out)), out.shape[3], out_coff, B, H * W, c,
                                           _ptr(avg), _ptr(mx), _ptr(ws), _stream()), 'affine_silu_pool')
    return avg, mx


def attn_mlp(mode, avg, mx, W1, b1, W2, b2):
    B, Cc = avg.shape
    out = torch.empty_like(avg)
    check(_lib.lib().somi_attn_mlp_f32(mode, _ptr(avg), _ptr(mx), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(out), B, Cc,
                                       W1.shape[0], _stream()), 'attn_mlp')
    return out


def chan_stats(x, ca, c=None, x_coff=0):
    B, H, W, cs = x.shape
    c = cs - x_coff if c is None else c
    stats = torch.empty(B, H, W, 2, device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_chan_stats_nhwc_f32(_ptr(_f32c(x)), cs, x_coff, _ptr(ca), _ptr(stats), B, H * W, c, _stream()),
          'chan_stats')
    return stats


def spatial_attn(stats, w, bias, k):
    B, H, W, _ = stats.shape
    sa = torch.empty(B, H, W, device=stats.device, dtype=torch.float32)
    check(_lib.lib().somi_spatial_attn_f32(_ptr(stats), _ptr(w), _ptr(_f32c(bias)), _ptr(sa), B, H, W, k, _stream()), 'spatial_attn')
    return sa


def cbam_apply_(x, ca, stats, w, bias, k, c=None, x_coff=0):
    """In place: x[..., slice] *= ca[b,c] * sigmoid(conv_kxk(stats)+bias)  (CBAM, models/common.py:686-688)."""
    B, H, W, cs = x.shape
    c = cs - x_coff if c is None else c
    check(_lib.lib().somi_cbam_apply_nhwc_f32(_ptr(_f32c(x)), cs, x_coff, _ptr(ca), _ptr(stats), _ptr(w), _ptr(_f32c(bias)), _ptr(x), cs,
                                              x_coff, B, H, W, c, k, _stream()), 'cbam_apply')
    return x


def scale_channels(x, s=None, pix=None, out=None):
    B, H, W, Cc = x.shape
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().somi_scale_channels_nhwc_f32(_ptr(_f32c(x)), _ptr(s), _ptr(pix), _ptr(out), B, H * W, Cc, _stream()),
          'scale_channels')
    return out


def detect_decode(box, cls, anchors_px, stride, na, nc, raw=None, z=None, total=0, row_off=0):
    B, ny, nx, box_cs = box.shape
    a = (C.c_float * (na * 2))(*[float(v) for v in anchors_px])
    check(_lib.lib().somi_detect_decode_f32(_ptr(_f32c(box)), box_cs, _ptr(_f32c(cls)), cls.shape[3], a, float(stride),
                                            _ptr(raw), _ptr(z), B, ny, nx, na, nc, total, row_off, _stream()), 'detect_decode')


def detect_plain_decode(t, anchors_px, stride, na, nc, raw=None, z=None, total=0, row_off=0):
    """Plain `Detect` (models/yolo.py:66-98): t (B,ny,nx,>=na*no) -> raw (B,na,ny,nx,no) and rows of z."""
    B, ny, nx, t_cs = t.shape
    a = (C.c_float * (na * 2))(*[float(v) for v in anchors_px])
    check(_lib.lib().somi_detect_plain_decode_f32(_ptr(_f32c(t)), t_cs, a, float(stride), _ptr(raw), _ptr(z), B, ny, nx, na, nc, total,
                                                  row_off, _stream()), 'detect_plain_decode')


def detect_plain_raw_backward(draw, t_cs, na, nc):
    B, _, ny, nx, _ = draw.shape
    dt = torch.empty(B, ny, nx, t_cs, device=draw.device, dtype=torch.float32)
    check(_lib.lib().somi_detect_plain_raw_bwd_f32(_ptr(_f32c(draw)), _ptr(dt), t_cs, B, ny, nx, na, nc, _stream()), 'detect_plain_raw_bwd')
    return dt


def resample_slice(src, src_coff, dst, dst_coff, c, up=0, reduce=False, accumulate=False):
    """reduce=False: dst[b,h,w,dst_coff+c] = src[b,h>>up,w>>up,src_coff+c] (Concat copy with nn.Upsample folded in);
    reduce=True: the adjoint, dst (low resolution) (+)= block sums of src."""
    lo = dst if reduce else src
    B, Hs, Ws, _ = lo.shape
    hi = src if reduce else dst
    if hi.shape[1] != Hs << up or hi.shape[2] != Ws << up or hi.shape[0] != B:
        raise RuntimeError(f'resample_slice: shapes {tuple(src.shape)} / {tuple(dst.shape)} do not differ by 2^{up}')
    check(_lib.lib().somi_resample_slice_nhwc_f32(_ptr(_f32c(src)), src.shape[3], src_coff, _ptr(_f32c(dst)), dst.shape[3], dst_coff, B, Hs, Ws,
                                                  c, up, int(reduce), int(accumulate), _stream()), 'resample_slice')
    return dst


def space_to_depth(x, x_coff, c, out=None, inverse=False, y_coff=0):
    """Focus (models/common.py:1996): (B,2Ho,2Wo,.) slice of c channels -> (B,Ho,Wo,4c); inverse=True maps a gradient in the deep
    layout back to the image layout (allocated with pad4(c) channels unless `out` is given).  A given `out` is written at channels
    [y_coff, y_coff + 4c) (inverse: + c) and nowhere else; an allocated one has its padding channels zeroed."""
    if not inverse:
        B, H, W, _ = x.shape
        if out is None:
            out = torch.empty(B, H // 2, W // 2, (4 * c + 3) // 4 * 4, device=x.device, dtype=torch.float32)
            if 4 * c < out.shape[3]:
                out[..., 4 * c:].zero_()
        check(_lib.lib().somi_space_to_depth_nhwc_f32(_ptr(_f32c(x)), x.shape[3], x_coff, _ptr(_f32c(out)), out.shape[3], y_coff, B, H // 2, W // 2,
                                                      c, 0, _stream()), 'space_to_depth')
        return out
    B, Ho, Wo, _ = x.shape
    out = torch.zeros(B, 2 * Ho, 2 * Wo, (c + 3) // 4 * 4, device=x.device, dtype=torch.float32) if out is None else out
    check(_lib.lib().somi_space_to_depth_nhwc_f32(_ptr(_f32c(x)), x.shape[3], x_coff, _ptr(_f32c(out)), out.shape[3], y_coff, B, Ho, Wo, c, 1,
                                                  _stream()), 'space_to_depth (inverse)')
    return out


def tta_resample(x4, ratio, gs, flip_lr, channels=3, pad=0.447):
    """scale_img(x.flip(3) if flip_lr else x, ratio, gs=gs) (utils/torch_utils.py:270-282) on an ingested (B,H,W,4) image."""
    import math
    B, H, W, _ = x4.shape
    Hs, Ws = (H, W) if ratio == 1.0 else (int(H * ratio), int(W * ratio))
    Hp, Wp = (H, W) if ratio == 1.0 else (math.ceil(H * ratio / gs) * gs, math.ceil(W * ratio / gs) * gs)
    y = torch.empty(B, Hp, Wp, 4, device=x4.device, dtype=torch.float32)
    check(_lib.lib().somi_tta_resample_nhwc4_f32(_ptr(_f32c(x4)), _ptr(y), B, H, W, Hs, Ws, Hp, Wp, int(bool(flip_lr)), float(pad), channels,
                                                 _stream()), 'tta_resample')
    return y


def resize_bilinear_nhwc4(x4, Hn, Wn, channels=3):
    """F.interpolate(x, size=(Hn, Wn), mode='bilinear', align_corners=False) on an ingested (B,H,W,4) image (`--multi-scale`, train.py:257-262)."""
    B, H, W, _ = x4.shape
    y = torch.empty(B, Hn, Wn, 4, device=x4.device, dtype=torch.float32)
    check(_lib.lib().somi_tta_resample_nhwc4_f32(_ptr(_f32c(x4)), _ptr(y), B, H, W, Hn, Wn, Hn, Wn, 0, 0.0, channels, _stream()), 'resize_bilinear')
    return y


def tta_descale_(z, scale, flip_lr, img_w):
    """_descale_pred (models/yolo.py:1292-1308) in place on z (B, n, no)."""
    check(_lib.lib().somi_tta_descale_f32(_ptr(_f32c(z)), z.shape[0] * z.shape[1], z.shape[2], float(scale), int(bool(flip_lr)), float(img_w),
                                          _stream()), 'tta_descale')
    return z


def odconv_weights(gap, fc_w, fc_b, pk, wout, bout, cin, cin_pad, cout, kk, K):
    """Attention heads + per-sample weight synthesis of ODConv (models/common.py:4557-4590), outer BN folded in."""
    B = gap.shape[0]
    hid = fc_w.shape[0]
    ws = torch.empty(B * (cout + kk + cin + K), device=gap.device, dtype=torch.float32)
    check(_lib.lib().somi_odconv_weights_f32(_ptr(gap), _ptr(fc_w), _ptr(fc_b), _ptr(pk['Wf']), _ptr(pk['bf']), _ptr(pk['Ws']),
                                             _ptr(pk['bs']), _ptr(pk['Wc']), _ptr(pk['bc']), _ptr(pk['Ww']), _ptr(pk['bw']),
                                             _ptr(pk['Wk']), _ptr(pk['biask']), _ptr(pk['bn_s']), _ptr(pk['bn_t']),
                                             _ptr(wout), _ptr(bout), _ptr(ws), B, cin, cin_pad, cout, kk, K, hid, _stream()),
          'odconv_weights')
    return wout, bout


def layernorm_act(x, gamma, beta, eps, act='none'):
    """LayerNorm over the last dim of contiguous NHWC + activation (DCNv3 module, modules/dcnv3.py:283-291)."""
    out = torch.empty_like(x)
    C_ = x.shape[-1]
    check(_lib.lib().somi_layernorm_act_nhwc_f32(_ptr(_f32c(x)), _ptr(gamma), _ptr(beta), float(eps), ACT[act], _ptr(out),
                                                 x.numel() // C_, C_, _stream()), 'layernorm_act')
    return out


def group_softmax(x, K):
    """softmax over trailing groups of K (mask logits (N,H,W,G*K) -> softmax per (pixel, group), modules/dcnv3.py:334)."""
    out = torch.empty_like(x)
    check(_lib.lib().somi_group_softmax_f32(_ptr(_f32c(x)), _ptr(out), x.numel() // K, K, _stream()), 'group_softmax')
    return out


def layernorm_gelu_backward(u, gamma, beta, eps, dz, dgamma, dbeta):
    """z = gelu(LayerNorm(u)) -> du; dgamma / dbeta are accumulated."""
    C_ = u.shape[-1]
    n = u.numel() // C_
    du = torch.empty_like(u)
    L = _lib.lib()
    ws = torch.empty(L.somi_layernorm_act_bwd_workspace_floats(n, C_), device=u.device, dtype=torch.float32)
    check(L.somi_layernorm_gelu_bwd_nhwc_f32(_ptr(_f32c(u)), _ptr(gamma), _ptr(beta), float(eps), _ptr(_f32c(dz)), _ptr(du), _ptr(dgamma),
                                             _ptr(dbeta), _ptr(ws), n, C_, _stream()), 'layernorm_gelu_bwd')
    return du


def group_softmax_backward(y, dy, K):
    dx = torch.empty_like(y)
    check(_lib.lib().somi_group_softmax_bwd_f32(_ptr(_f32c(y)), _ptr(_f32c(dy)), _ptr(dx), y.numel() // K, K, _stream()), 'group_softmax_bwd')
    return dx


def cfs_blend_backward(x, xproj, logit, dout, G, Gc):
    """-> (dx, dxproj, dlogit) of out = x*(1-s) + xproj*s, s = sigmoid(logit) broadcast over a group's channels."""
    dx, dxp = torch.empty_like(x), torch.empty_like(x)
    dlogit = torch.zeros_like(logit)                              # pad columns (if any) stay zero
    check(_lib.lib().somi_dcnv3_cfs_blend_bwd_f32(_ptr(_f32c(x)), _ptr(_f32c(xproj)), _ptr(_f32c(logit)), logit.shape[-1], _ptr(_f32c(dout)),
                                                  _ptr(dx), _ptr(dxp), _ptr(dlogit), dlogit.shape[-1], x.numel() // (G * Gc), G, Gc,
                                                  _stream()), 'cfs_blend_bwd')
    return dx, dxp, dlogit


def cfs_blend(x, xproj, logit, G, Gc):
    out = torch.empty_like(x)
    check(_lib.lib().somi_dcnv3_cfs_blend_f32(_ptr(_f32c(x)), _ptr(_f32c(xproj)), _ptr(_f32c(logit)), logit.shape[-1], _ptr(out),
                                              x.numel() // (G * Gc), G, Gc, _stream()), 'cfs_blend')
    return out


def conv2d_dgrad_nhwc(dy, w_dgrad, *, B, H, W, cin, kh, kw, stride=1, pad=0, dil=1, cout=None, dy_coff=0, out=None, dx_coff=0,
                      accumulate=None, acc_coff=0, per_sample_w=False, accumulate2=None, acc2_coff=0):
    """dx of the conv x (B,H,W,cin) -> y (B,Ho,Wo,cout); dy is (B,Ho,Wo,dy_cs); w_dgrad packed [cin][kh*kw*cout].
    dil > 1 runs at stride 1 only (the library refuses the combination)."""
    _, Ho, Wo, dy_cs = dy.shape
    cout = dy_cs - dy_coff if cout is None else cout
    if out is None:
        out = torch.empty(B, H, W, cin, device=dy.device, dtype=torch.float32)
    d = ConvDesc()
    d.prec = CONV_PREC
    d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = B, H, W, cin, Ho, Wo, cout
    d.kh, d.kw, d.stride, d.pad, d.dil, d.per_sample_w = kh, kw, stride, pad, dil, int(per_sample_w)
    _conv_workspace(d, dy.device)
    if accumulate2 is not None:                                   # second added tensor (e.g. the shortcut branch's gradient)
        d.residual2, d.res2_cs, d.res2_coff = _ptr(_f32c(accumulate2)), accumulate2.shape[3], acc2_coff
    if w_dgrad.numel() != (B if per_sample_w else 1) * cin * kh * kw * cout:
        raise RuntimeError('dgrad weight has the wrong number of elements')
    def info():
        g = ConvDesc()                                           # the geometry the kernel runs in: rows = forward-input pixels
        g.B, g.H, g.W, g.Cin, g.Ho, g.Wo, g.Cout = B, Ho, Wo, cout, H, W, cin
        g.kh, g.kw, g.stride, g.dil, g.per_sample_w = kh, kw, stride, dil, int(per_sample_w)
        if stride == 1:
            g.workspace, g.workspace_bytes = d.workspace, d.workspace_bytes
        return _lib.lib().somi_conv2d_kernel_name(C.byref(g)).decode(), 2.0 * B * Ho * Wo * cout * cin * kh * kw, (B, H, W, cin, cout, kh, stride, 2)
    with _timed(info):
        check(_lib.lib().somi_conv2d_dgrad_nhwc_f32(C.byref(d), _ptr(_f32c(dy)), dy_cs, dy_coff, _ptr(_f32c(w_dgrad)), _ptr(_f32c(out)),
                                                    out.shape[3], dx_coff, _ptr(accumulate),
                                                    accumulate.shape[3] if accumulate is not None else 0, acc_coff, _stream()),
              'conv2d_dgrad_nhwc')
    return out


def conv2d_wgrad_nhwc(x, dy, *, kh, kw, stride=1, pad=0, dil=1, cin=None, x_coff=0, cout=None, dy_coff=0, out=None, accumulate=None,
                      per_sample_w=False):
    """dW [Cout][kh*kw*Cin] (forward packing) of the conv x (B,H,W,cin) -> y (B,Ho,Wo,cout) from x and dy."""
    B, H, W, x_cs = x.shape
    _, Ho, Wo, dy_cs = dy.shape
    cin = x_cs - x_coff if cin is None else cin
    cout = dy_cs - dy_coff if cout is None else cout
    d = ConvDesc()
    d.prec = CONV_PREC
    d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = B, H, W, cin, Ho, Wo, cout
    d.kh, d.kw, d.stride, d.pad, d.dil, d.per_sample_w = kh, kw, stride, pad, dil, int(per_sample_w)
    shape = ((B,) if per_sample_w else ()) + (cout, kh * kw * cin)
    if out is None:
        out = torch.empty(*shape, device=x.device, dtype=torch.float32)
    L = _lib.lib()
    nbytes = L.somi_conv2d_wgrad_workspace_bytes(C.byref(d))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device)
    with _timed(lambda: (L.somi_conv2d_wgrad_kernel_name(C.byref(d)).decode(), 2.0 * B * Ho * Wo * cout * cin * kh * kw,
                         (B, H, W, cin, cout, kh, stride, 3))):
        check(L.somi_conv2d_wgrad_nhwc_f32(C.byref(d), _ptr(_f32c(x)), x_cs, x_coff, _ptr(_f32c(dy)), dy_cs, dy_coff, _ptr(_f32c(out)),
                                           _ptr(accumulate), _ptr(ws), nbytes, _stream()), 'conv2d_wgrad_nhwc')
    return out


# ---------------------------------------------------------------------------------------------- grouped / depthwise convolution
# fp32 always: CONV_PREC (--amp bf16 / bf16x3) applies to the dense implicit GEMM only.
def gconv2d_nhwc(x, w, bias=None, *, c1, c2, groups, k, stride=1, x_coff=0, out=None, y_coff=0, cw=None, act='none', residual=None, res_coff=0,
                 bn_stats=None):
    """Grouped conv of x's channel slice [x_coff, x_coff + c1) -> out's slice [y_coff, y_coff + cw); w packed [k*k][c1/groups][w_cs]
    (pack.pack_gconv_weight), pad k // 2.  bn_stats: dict filled in place with the partial channel sums ('part' (2, rows, cw), 'rows')
    around bn_stats['pivot'] - the dense conv2d_nhwc(bn_stats=...) format, for bn_stats_from_partials."""
    B, H, W, x_cs = x.shape
    Ho, Wo = conv_out_size(H, k, stride, k // 2), conv_out_size(W, k, stride, k // 2)
    cw = (c2 + 3) // 4 * 4 if cw is None else cw
    if out is None:
        out = torch.empty(B, Ho, Wo, cw, device=x.device, dtype=torch.float32)
    if tuple(out.shape[:3]) != (B, Ho, Wo) or (residual is not None and tuple(residual.shape[:3]) != (B, Ho, Wo)):
        raise RuntimeError(f'grouped conv: output / residual must be ({B}, {Ho}, {Wo}, .), got {tuple(out.shape)}')
    L = _lib.lib()
    ss = sq = piv = None
    if bn_stats is not None:
        rows = L.somi_gconv2d_stat_rows(B, Ho, Wo, cw)
        part = torch.empty(2, rows, cw, device=x.device, dtype=torch.float32)
        ss, sq, piv = part[0].data_ptr(), part[1].data_ptr(), _ptr(bn_stats.get('pivot'))
        bn_stats['part'], bn_stats['rows'] = part, rows
    check(L.somi_gconv2d_nhwc_f32(_ptr(_f32c(x, 'input')), x_cs, x_coff, B, H, W, c1, _ptr(_f32c(w, 'weight')), w.shape[-1], _ptr(bias), groups, k,
                                  stride, _ptr(_f32c(out, 'output')), out.shape[3], y_coff, c2, cw, ACT[act],
                                  _ptr(None if residual is None else _f32c(residual, 'residual')), 0 if residual is None else residual.shape[3],
                                  res_coff, ss, sq, piv, _stream()), 'gconv2d_nhwc')
    return out


def gconv2d_dgrad_nhwc(dy, w, *, H, W, c1, c2, groups, k, stride=1, dy_coff=0, out=None, dx_coff=0, cx=None, accumulate=None, acc_coff=0,
                       accumulate2=None, acc2_coff=0):
    """Data gradient of gconv2d_nhwc into out's slice [dx_coff, dx_coff + cx) (+ accumulate's and accumulate2's slices; accumulate may be out)."""
    B, Ho, Wo, dy_cs = dy.shape
    cx = (c1 + 3) // 4 * 4 if cx is None else cx
    if out is None:
        out = torch.empty(B, H, W, cx, device=dy.device, dtype=torch.float32)
    a1, a2 = accumulate, accumulate2
    if any(t is not None and tuple(t.shape[:3]) != (B, H, W) for t in (out, a1, a2)):
        raise RuntimeError(f'grouped conv dgrad: output / accumulated tensors must be ({B}, {H}, {W}, .)')
    check(_lib.lib().somi_gconv2d_dgrad_nhwc_f32(_ptr(_f32c(dy, 'gradient')), dy_cs, dy_coff, B, Ho, Wo, c2, _ptr(_f32c(w, 'weight')), w.shape[-1],
                                                 groups, k, stride, _ptr(_f32c(out, 'output')), out.shape[3], dx_coff, H, W, c1, cx,
                                                 _ptr(None if a1 is None else _f32c(a1)), 0 if a1 is None else a1.shape[3], acc_coff,
                                                 _ptr(None if a2 is None else _f32c(a2)), 0 if a2 is None else a2.shape[3], acc2_coff, _stream()),
          'gconv2d_dgrad_nhwc')
    return out


def gconv2d_wgrad_nhwc(x, dy, *, c1, c2, groups, k, stride=1, x_coff=0, dy_coff=0, out=None, accumulate=False):
    """Weight gradient (c2, c1/groups, k, k) of gconv2d_nhwc, written into `out` (or added to it when accumulate)."""
    B, H, W, x_cs = x.shape
    _, Ho, Wo, dy_cs = dy.shape
    L = _lib.lib()
    if out is None:
        out = torch.empty(c2, c1 // groups, k, k, device=x.device, dtype=torch.float32)
    if out.numel() != c2 * (c1 // groups) * k * k or dy.shape[0] != B:
        raise RuntimeError('grouped conv wgrad: weight gradient or batch size does not match')
    n = L.somi_gconv2d_wgrad_workspace_floats(B, Ho, Wo, c2, c1 // groups, k)
    ws = torch.empty(max(n, 4), device=x.device, dtype=torch.float32)
    check(L.somi_gconv2d_wgrad_nhwc_f32(_ptr(_f32c(x, 'input')), x_cs, x_coff, B, H, W, c1, _ptr(_f32c(dy, 'gradient')), dy_cs, dy_coff, Ho, Wo, c2,
                                        groups, k, stride, _ptr(_f32c(out, 'weight gradient')), int(accumulate), _ptr(ws), ws.numel(), _stream()),
          'gconv2d_wgrad_nhwc')
    return out


# ---------------------------------------------------------------------------------------------- large-kernel depthwise conv (dwlk.hip)
# k = 7 or 9, stride 1, pad k // 2, c % 4 == 0; w packed [k*k][1][w_cs] (pack.pack_gconv_weight).  fp32 always.
def dwlk_strip_length():
    """Adjacent outputs of one image row a lane of the dwlk kernels owns."""
    return _lib.lib().somi_dwlk_strip_length()


def dwlk_strips_per_workgroup(B, H, W, c, wgrad=False):
    """Rows of strips a workgroup of dwlk / dwlk_dgrad (wgrad: of dwlk_wgrad) walks at this size (host arithmetic; 0 for a size they refuse)."""
    return _lib.lib().somi_dwlk_strips_per_workgroup(int(B), int(H), int(W), int(c), int(bool(wgrad)))


def _dwlk_maps(B, H, W, what, *tensors):
    for t in tensors:
        if t is not None and (t.dim() != 4 or tuple(t.shape[:3]) != (B, H, W)):
            raise RuntimeError(f'{what}: every map must be ({B}, {H}, {W}, .), got {tuple(t.shape)}')


def _dwlk_work(name, B, H, W, c, k, passes):
    """-> _timed's info: (kernel name, algorithmic FLOPs, shape key)."""
    return lambda: (f'{name}_k{k}', 2.0 * B * H * W * c * k * k, (B, H, W, c, c, k, 1, passes))


def dwlk(x, w, bias=None, *, c, k, x_coff=0, act='none', post_scale=None, post_shift=None, out=None, o_coff=0, residual=None, res_coff=0,
         bn_stats=None):
    """out's slice [o_coff, o_coff + c) = post_scale * act(dwconv_k(x's slice) + bias) + post_shift (+ residual's slice); act 'none' or
    'gelu'.  bn_stats: dict filled in place with the partial channel sums of act(conv + bias) around bn_stats['pivot'] ('part' (2, rows, c),
    'rows'), for bn_stats_from_partials; the tensor written is then the PRE-activation conv + bias, and post_scale / post_shift / residual
    must be None."""
    B, H, W, _ = x.shape
    if out is None:
        out = torch.empty(B, H, W, c, device=x.device, dtype=torch.float32)
    _dwlk_maps(B, H, W, 'dwlk', out, residual)
    if w.numel() != k * k * w.shape[-1]:
        raise RuntimeError(f'dwlk: the weight must be a [{k * k}][1][w_cs] pack, got {tuple(w.shape)}')
    for v, what in ((bias, 'bias'), (post_scale, 'post_scale'), (post_shift, 'post_shift')):
        if v is not None and (v.numel() < c or v.dtype != torch.float32 or not v.is_contiguous()):
            raise RuntimeError(f'dwlk: {what} must be at least {c} contiguous floats')
    L = _lib.lib()
    ss = sq = piv = None
    if bn_stats is not None:
        rows = L.somi_dwlk_stat_rows(B, H, W, c)
        part = torch.empty(2, max(rows, 1), c, device=x.device, dtype=torch.float32)
        ss, sq, piv = part[0].data_ptr(), part[1].data_ptr(), _ptr(bn_stats.get('pivot'))
        bn_stats['part'], bn_stats['rows'] = part, rows
    with _timed(_dwlk_work('dwlk_fwd', B, H, W, c, k, 1)):
        check(L.somi_dwlk_nhwc_f32(_slice(x, x_coff), _ptr(_f32c(w, 'weight')), w.shape[-1], _ptr(bias), k, ACT[act], _ptr(post_scale), _ptr(post_shift),
                                   _slice(out, o_coff), _NO_SLICE if residual is None else _slice(residual, res_coff), B, H, W, c, ss, sq, piv,
                                   _stream()), 'dwlk')
    return out


def dwlk_dgrad(dy, w, *, c, k, dy_coff=0, out=None, dx_coff=0, accumulate=None, acc_coff=0, accumulate2=None, acc2_coff=0):
    """Data gradient of dwlk into out's slice [dx_coff, dx_coff + c) (+ accumulate's and accumulate2's slices; accumulate may be out)."""
    B, H, W, _ = dy.shape
    if out is None:
        out = torch.empty(B, H, W, c, device=dy.device, dtype=torch.float32)
    a1, a2 = accumulate, accumulate2
    _dwlk_maps(B, H, W, 'dwlk_dgrad', out, a1, a2)
    with _timed(_dwlk_work('dwlk_dgrad', B, H, W, c, k, 2)):
        check(_lib.lib().somi_dwlk_dgrad_nhwc_f32(_slice(dy, dy_coff), _ptr(_f32c(w, 'weight')), w.shape[-1], k, _slice(out, dx_coff),
                                                  _NO_SLICE if a1 is None else _slice(a1, acc_coff), _NO_SLICE if a2 is None else _slice(a2, acc2_coff),
                                                  B, H, W, c, _stream()), 'dwlk_dgrad')
    return out


def dwlk_wgrad(x, dy, *, c, k, x_coff=0, dy_coff=0, dw=None, db=None, accumulate=False, bias=True):
    """-> (dw (c, 1, k, k), db (c)): weight and bias gradients of dwlk from one pass, written into dw / db (or added to them when accumulate).
    bias=False and db None: no bias gradient (db comes back None)."""
    B, H, W, _ = x.shape
    _dwlk_maps(B, H, W, 'dwlk_wgrad', dy)
    if dw is None:
        dw = (torch.zeros if accumulate else torch.empty)(c, 1, k, k, device=x.device, dtype=torch.float32)
    if db is None and bias:
        db = (torch.zeros if accumulate else torch.empty)(c, device=x.device, dtype=torch.float32)
    if dw.numel() != c * k * k or (db is not None and db.numel() != c):
        raise RuntimeError(f'dwlk_wgrad: dw must hold {c * k * k} floats and db {c}')
    L = _lib.lib()
    n = L.somi_dwlk_wgrad_workspace_floats(B, H, W, c, k)
    ws = torch.empty(max(n, 4), device=x.device, dtype=torch.float32)
    with _timed(_dwlk_work('dwlk_wgrad', B, H, W, c, k, 3)):
        check(L.somi_dwlk_wgrad_nhwc_f32(_slice(x, x_coff), _slice(dy, dy_coff), B, H, W, c, k, _ptr(_f32c(dw, 'weight gradient')),
                                         _ptr(None if db is None else _f32c(db, 'bias gradient')), int(accumulate), _ptr(ws), ws.numel(), _stream()),
              'dwlk_wgrad')
    return dw, db


# ---------------------------------------------------------------------------------------------- slim-neck GSConv (gsconv.hip)
# ch is the half width c2 // 2 of a GSConv: x1 / x_2 / d1 / d2 are slices of ch channels, the shuffled output and its gradient of 2 * ch.
def gs_tiles_per_workgroup(npix, ch):
    """Pixel tiles a workgroup of gs_shuffle_affine_act / gs_unshuffle walks at this size (host arithmetic; 0 for a size they refuse)."""
    return _lib.lib().somi_gs_tiles_per_workgroup(int(npix), int(ch))


def _gs_map(t, shape, what):
    if t.dim() != 4 or tuple(t.shape[:3]) != tuple(shape):
        raise RuntimeError(f'{what} must be ({shape[0]}, {shape[1]}, {shape[2]}, .), got {tuple(t.shape)}')


def gs_tail(x1, w1, b1, w2, b2, ch, act='silu', x_coff=0, *, out=None, o_coff=0, residual=None, res_coff=0):
    """Inference tail of a GSConv behind its first conv: x_2 = act(dw2(act(dw1(x1) + b1)) + b2) with the intermediate zero outside the image,
    and out's slice [o_coff, o_coff + 2 ch) = shuffle(x1, x_2) (+ residual's slice).  w1 / w2: pack_gconv_weight's [9][1][w_cs] with the
    BatchNorm folded, b1 / b2 the folded biases (at least ch floats).  out must not be x1."""
    B, H, W, _ = x1.shape
    if out is None:
        out = torch.empty(B, H, W, 2 * ch, device=x1.device, dtype=torch.float32)
    _gs_map(out, (B, H, W), 'gs_tail: output')
    if residual is not None:
        _gs_map(residual, (B, H, W), 'gs_tail: residual')
    if w1.shape != w2.shape or w1.numel() != 9 * w1.shape[-1] or min(b1.numel(), b2.numel()) < ch:
        raise RuntimeError(f'gs_tail: weights must be two [9][1][w_cs] packs and the biases {ch} floats')
    check(_lib.lib().somi_gs_tail_nhwc_f32(_slice(x1, x_coff), _ptr(_f32c(w1)), _ptr(_f32c(b1)), _ptr(_f32c(w2)), _ptr(_f32c(b2)), w1.shape[-1],
                                           ACT[act], _slice(out, o_coff), _NO_SLICE if residual is None else _slice(residual, res_coff),
                                           B, H, W, ch, _stream()), 'gs_tail')
    return out


def gs_shuffle_affine_act(z1, y2, ch, scale=None, shift=None, act='none', z_coff=0, y_coff=0, *, out=None, o_coff=0, residual=None, res_coff=0):
    """Training forward: out's slice = shuffle(z1, act(y2 * scale + shift)) (+ residual's slice); scale = shift = None is the identity."""
    if out is None:
        out = torch.empty(*z1.shape[:3], 2 * ch, device=z1.device, dtype=torch.float32)
    for t, what in ((y2, 'y2'), (out, 'output')) + (() if residual is None else ((residual, 'residual'),)):
        _gs_map(t, z1.shape[:3], f'gs_shuffle_affine_act: {what}')
    if (scale is None) != (shift is None) or (scale is not None and min(scale.numel(), shift.numel()) < ch):
        raise RuntimeError(f'gs_shuffle_affine_act: scale and shift come together, {ch} floats each')
    check(_lib.lib().somi_gs_shuffle_affine_act_nhwc_f32(_slice(z1, z_coff), _slice(y2, y_coff), _ptr(scale), _ptr(shift), ACT[act],
                                                         _slice(out, o_coff), _NO_SLICE if residual is None else _slice(residual, res_coff),
                                                         _npix(z1), ch, _stream()), 'gs_shuffle_affine_act')
    return out


def gs_unshuffle(dout, ch, do_coff=0, *, d1=None, d2=None, d1_coff=0, d2_coff=0):
    """Training backward: the gradient of the shuffled output's slice [do_coff, do_coff + 2 ch) -> (d1, d2), the gradients of x1 and x_2."""
    d1, d2 = (torch.empty(*dout.shape[:3], ch, device=dout.device, dtype=torch.float32) if d is None else d for d in (d1, d2))
    for t, what in ((d1, 'd1'), (d2, 'd2')):
        _gs_map(t, dout.shape[:3], f'gs_unshuffle: {what}')
    check(_lib.lib().somi_gs_unshuffle_nhwc_f32(_slice(dout, do_coff), _slice(d1, d1_coff), _slice(d2, d2_coff), _npix(dout), ch, _stream()),
          'gs_unshuffle')
    return d1, d2


# ---------------------------------------------------------------------------------------------- PSA attention
# fp32 always, key_dim 32 / head_dim 64 (attention.hip).
def psa_attention(qkv, heads, *, qkv_coff=0, out=None, o_coff=0, lse=False, v_out=False):
    """Multi-head attention of AttentionPSA over the NHWC qkv Conv output's slice [qkv_coff, qkv_coff + 128*heads) (per head q 32 | k 32 |
    v 64) -> out's slice [o_coff, o_coff + 64*heads).  lse: also return the log-sum-exp (B, heads, H*W) the backward needs; v_out: also
    return v as a contiguous (B, H, W, 64*heads) tensor.  -> (out, lse or None, v or None)"""
    B, H, W, cs = qkv.shape
    N = H * W
    if out is None:
        out = torch.empty(B, H, W, 64 * heads, device=qkv.device, dtype=torch.float32)
    _map(out, (B, H, W), 'psa attention: output')
    lt = torch.empty(B, heads, N, device=qkv.device, dtype=torch.float32) if lse else None
    vt = torch.empty(B, H, W, 64 * heads, device=qkv.device, dtype=torch.float32) if v_out else None
    check(_lib.lib().somi_psa_attention_f32(_ptr(_f32c(qkv, 'qkv')), cs, qkv_coff, B, N, heads, _ptr(_f32c(out, 'output')), out.shape[3],
                                            o_coff, _ptr(lt), _ptr(vt), _stream()), 'psa_attention')
    return out, lt, vt


def psa_attention_backward(qkv, o, dout, lse, heads, *, qkv_coff=0, o_coff=0, do_coff=0, out=None, g_coff=0, dv_add=None):
    """Gradient of psa_attention w.r.t. q, k and v, written into out's slice [g_coff, g_coff + 128*heads) in the qkv layout.  dv_add: a
    contiguous (B, H, W, 64*heads) tensor added to dv (the gradient that reached v through pe)."""
    B, H, W, cs = qkv.shape
    N = H * W
    if out is None:
        out = torch.empty(B, H, W, 128 * heads, device=qkv.device, dtype=torch.float32)
    if any(t is not None and tuple(t.shape[:3]) != (B, H, W) for t in (o, dout, out, dv_add)) or tuple(lse.shape) != (B, heads, N):
        raise RuntimeError(f'psa attention backward: tensors must be ({B}, {H}, {W}, .) and lse ({B}, {heads}, {N})')
    if dv_add is not None and (dv_add.shape[3] != 64 * heads or not dv_add.is_contiguous()):
        raise RuntimeError('psa attention backward: dv_add must be a contiguous (B, H, W, 64*heads) tensor')
    ws = torch.empty(B * heads * N, device=qkv.device, dtype=torch.float32)
    check(_lib.lib().somi_psa_attention_backward_f32(_ptr(_f32c(qkv, 'qkv')), cs, qkv_coff, _ptr(_f32c(o, 'output')), o.shape[3], o_coff,
                                                     _ptr(_f32c(dout, 'gradient')), dout.shape[3], do_coff, _ptr(_f32c(lse, 'lse')), B, N,
                                                     heads, _ptr(_f32c(out, 'qkv gradient')), out.shape[3], g_coff,
                                                     _ptr(None if dv_add is None else _f32c(dv_add)), _ptr(ws), _stream()),
          'psa_attention_backward')
    return out


# ---------------------------------------------------------------------------------------------- Swin window attention
# fp32 always, window 8 / head_dim 32 (swin.hip).  Whole contiguous tensors.
def _swin_args(qkv, table, heads, shift, region_ids, what):
    B, H, W, c3 = qkv.shape
    if c3 % 3 or c3 // 3 != 32 * heads:
        raise NotImplementedError(f'{what}: head_dim 32 only, got {c3 // 3} channels for {heads} heads')
    if tuple(table.shape) != (225, heads):
        raise RuntimeError(f'{what}: the bias table must be (225, {heads}), got {tuple(table.shape)}')
    if shift:
        hp, wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
        if region_ids is None or region_ids.dtype != torch.int32 or tuple(region_ids.shape) != (wp, hp) or not region_ids.is_contiguous():
            raise RuntimeError(f'{what}: a shifted layer needs a contiguous int32 region-id map of shape ({wp}, {hp})')
    return B, H, W, c3 // 3


def window_attention(qkv, table, heads, shift=0, region_ids=None, *, lse=False):
    """8x8-window multi-head attention of SwinTransformerLayer over the bias-free qkv Linear's output (B,H,W,3C) (channel = which*C + head*32
    + d), with the relative-position bias `table` (225, heads), the cyclic `shift` (0 or 4), the zero padding up to the window grid and the
    shift mask from `region_ids` (int32 (Wp,Hp), blocks.swin_region_ids) -> (o (B,H,W,C), lse or None): the log-sum-exp the backward needs."""
    B, H, W, C_ = _swin_args(qkv, table, heads, shift, region_ids, 'window attention')
    L = _lib.lib()
    out = torch.empty(B, H, W, C_, device=qkv.device, dtype=torch.float32)
    lt = torch.empty(L.somi_swin_attention_lse_floats(B, H, W, heads), device=qkv.device, dtype=torch.float32) if lse else None
    check(L.somi_swin_attention_f32(_ptr(_f32c(qkv, 'qkv')), _ptr(_f32c(table, 'bias table')), _ptr(region_ids if shift else None), B, H, W, C_,
                                    heads, shift, _ptr(out), _ptr(lt), _stream()), 'window_attention')
    return out, lt


def window_attention_backward(qkv, table, dout, lse, heads, shift=0, region_ids=None, *, dtable):
    """Gradient of window_attention w.r.t. q, k and v -> (B,H,W,3C) in the qkv layout; the bias table's gradient is accumulated into
    `dtable` (225, heads), in a fixed order."""
    B, H, W, C_ = _swin_args(qkv, table, heads, shift, region_ids, 'window attention backward')
    if tuple(dout.shape) != (B, H, W, C_) or tuple(dtable.shape) != (225, heads):
        raise RuntimeError(f'window attention backward: dout must be ({B}, {H}, {W}, {C_}) and dtable (225, {heads})')
    L = _lib.lib()
    out = torch.empty_like(qkv)
    ws = torch.empty(L.somi_swin_attention_bwd_workspace_floats(B, H, W, heads), device=qkv.device, dtype=torch.float32)
    check(L.somi_swin_attention_backward_f32(_ptr(_f32c(qkv, 'qkv')), _ptr(_f32c(table, 'bias table')), _ptr(region_ids if shift else None),
                                             _ptr(_f32c(dout, 'gradient')), _ptr(_f32c(lse, 'lse')), B, H, W, C_, heads, shift, _ptr(out),
                                             _ptr(_f32c(dtable, 'table gradient')), _ptr(ws), _stream()), 'window_attention_backward')
    return out


def layernorm_backward(u, gamma, eps, dy, dgamma, dbeta, add=None):
    """y = LayerNorm(u) over the last dim -> du (+ add, the gradient of a residual branch around the norm); dgamma / dbeta are accumulated."""
    C_ = u.shape[-1]
    n = u.numel() // C_
    du = torch.empty_like(u)
    L = _lib.lib()
    ws = torch.empty(L.somi_layernorm_bwd_workspace_floats(n, C_), device=u.device, dtype=torch.float32)
    check(L.somi_layernorm_bwd_nhwc_f32(_ptr(_f32c(u)), _ptr(gamma), float(eps), _ptr(_f32c(dy)), _ptr(None if add is None else _f32c(add)),
                                        _ptr(du), _ptr(dgamma), _ptr(dbeta), _ptr(ws), n, C_, _stream()), 'layernorm_backward')
    return du


def gelu_backward_(u, dy):
    """dy *= gelu'(u) in place (exact GELU)."""
    check(_lib.lib().somi_gelu_bwd_f32(_ptr(_f32c(u)), _ptr(_f32c(dy)), _ptr(dy), u.numel(), _stream()), 'gelu_backward')
    return dy


# ---------------------------------------------------------------------------------------------- training-mode helpers
def _npix(t):
    return t.shape[0] * t.shape[1] * t.shape[2]


# --sync-bn (reference train.py:165-167, torch.nn.SyncBatchNorm): set to the torch.distributed module (train.TrainStep(sync_bn=True) does
# it around its step) and every BatchNorm statistic below spans the batches of all ranks: one small all-gather per layer and direction.
SYNC_BN = None
SYNC_BN_GROUP = None     # the process group of these all-gathers.  TrainStep gives sync-BN a group of its OWN: on the default group every
#                          blocking all-gather would queue behind the asynchronous gradient buckets (collectives of one RCCL communicator run
#                          in issue order) and stall the backward pass until they finish - the overlap of the exchange would be lost.


def _gather_records(rec):
    """all-gather of one [2C + 1] double record per rank -> (flat [world * (2C + 1)] tensor, world)."""
    world = SYNC_BN.get_world_size(SYNC_BN_GROUP)
    out = torch.empty(world * rec.numel(), dtype=torch.float64, device=rec.device)
    SYNC_BN.all_gather_into_tensor(out, rec, group=SYNC_BN_GROUP)
    return out, world


def _bn_stats_sync(x, x_coff, n, c, part, rows, gamma, beta, eps, momentum, running_mean, running_var):
    L, dev = _lib.lib(), (x if x is not None else part).device
    mean, rstd, scale, shift = (torch.empty(c, device=dev, dtype=torch.float32) for _ in range(4))
    rec = torch.empty(2 * c + 1, device=dev, dtype=torch.float64)
    ws = torch.empty(2 * max(1024, L.somi_red_nchunk(n)) * c, device=dev, dtype=torch.float32)
    if part is not None:
        check(L.somi_bn_local_sums_f64(None, 0, 0, n, c, _ptr(running_mean), part[0].data_ptr(), part[1].data_ptr(), rows, _ptr(rec), _ptr(ws),
                                       _stream()), 'bn_local_sums')
    else:
        check(L.somi_bn_local_sums_f64(_ptr(_f32c(x)), x.shape[3], x_coff, n, c, _ptr(running_mean), None, None, 0, _ptr(rec), _ptr(ws),
                                       _stream()), 'bn_local_sums')
    allrec, world = _gather_records(rec)
    check(L.somi_bn_stats_from_sums_f64(_ptr(allrec), world, c, float(eps), float(momentum), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
                                        _ptr(scale), _ptr(shift), _ptr(running_mean), _ptr(running_var), _stream()), 'bn_stats_from_sums')
    return mean, rstd, scale, shift


def bn_stats(x, c, x_coff, gamma, beta, eps, momentum, running_mean=None, running_var=None, act='none'):
    """Batch statistics of a channel slice - of act(x) when `act` is given, without storing act(x) - -> (mean, rstd, scale, shift);
    optionally updates the running statistics."""
    dev = x.device
    n = _npix(x)
    if SYNC_BN is not None:
        if act != 'none':
            raise RuntimeError('bn_stats(act=...) has no sync-BN form: materialise act(x) first (blocks.SEAM does)')
        return _bn_stats_sync(x, x_coff, n, c, None, 0, gamma, beta, eps, momentum, running_mean, running_var)
    mean, rstd, scale, shift = (torch.empty(c, device=dev, dtype=torch.float32) for _ in range(4))
    ws = torch.empty(2 * _lib.lib().somi_red_nchunk(n) * c, device=dev, dtype=torch.float32)
    check(_lib.lib().somi_bn_stats_act_nhwc_f32(_ptr(_f32c(x)), x.shape[3], x_coff, ACT[act], n, c, float(eps), float(momentum), _ptr(gamma),
                                                _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(scale), _ptr(shift), _ptr(running_mean),
                                                _ptr(running_var), _ptr(ws), _stream()), 'bn_stats')
    return mean, rstd, scale, shift


def bn_stats_from_partials(part, rows, npix, c, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """Batch statistics from the partial sums a convolution's epilogue left (conv2d_nhwc(..., bn_stats={'pivot': running_mean}));
    `running_mean` must be that same pivot.  -> (mean, rstd, scale, shift); updates the running statistics."""
    dev = part.device
    if SYNC_BN is not None:
        return _bn_stats_sync(None, 0, npix, c, part, rows, gamma, beta, eps, momentum, running_mean, running_var)
    mean, rstd, scale, shift = (torch.empty(c, device=dev, dtype=torch.float32) for _ in range(4))
    ws = torch.empty(2 * 1024 * c, device=dev, dtype=torch.float32)
    check(_lib.lib().somi_bn_stats_partials_f32(part[0].data_ptr(), part[1].data_ptr(), rows, npix, c, float(eps), float(momentum), _ptr(gamma),
                                                _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(scale), _ptr(shift), _ptr(running_mean),
                                                _ptr(running_var), _ptr(ws), _stream()), 'bn_stats_partials')
    return mean, rstd, scale, shift


def chan_affine_act(x, c, x_coff, scale, shift, act, order, out, out_coff=0, residual=None, res_coff=0):
    check(_lib.lib().somi_chan_affine_act_nhwc_f32(_ptr(_f32c(x)), x.shape[3], x_coff, _ptr(scale), _ptr(shift), ACT[act], order,
                                                   _ptr(_f32c(out)), out.shape[3], out_coff, _npix(x), c,
                                                   _ptr(residual), residual.shape[3] if residual is not None else 0, res_coff,
                                                   _stream()), 'chan_affine_act')
    return out


def pack_dgrad_weights(w_packed, cout, taps, cin):
    """[cout][taps][cin] (forward packing) -> [cin][taps][cout] (operand of conv2d_dgrad_nhwc)."""
    out = torch.empty(cin, taps * cout, device=w_packed.device, dtype=torch.float32)
    check(_lib.lib().somi_pack_dgrad_weights_f32(_ptr(_f32c(w_packed)), _ptr(out), cout, taps, cin, _stream()), 'pack_dgrad_weights')
    return out


def bn_act_backward(dz, dz_coff, x, x_coff, c, mean, rstd, scale, shift, act, order, batch_stats, dx, dx_coff=0, dgamma=None,
                    dbeta=None, pooled=None):
    """pooled = (davg, dmax, amaxp), each (B, c): the gradient of a channel attention's global average / max pools over this tensor, i.e.
    dz_eff = dz + davg / HW + [pixel == amaxp] * dmax.  The image-aligned kernels take it on the fly (dz is only read); under sync-BN - whose
    reduce / apply entries have no such form - it is added to dz in place by a pass of its own first.  dmax / amaxp may be None (average pool
    only); dz may be None when nothing else reads the tensor (the pooled part is the whole gradient)."""
    n = _npix(x)
    if pooled is not None:
        davg, dmax, amaxp = pooled
        if SYNC_BN is None and batch_stats and davg.shape[1] == c and x.dim() == 4:
            B, HW = x.shape[0], x.shape[1] * x.shape[2]
            L = _lib.lib()
            ws = torch.empty(2 * L.somi_bn_pooled_rows(B, HW) * c + 3 * ((c + 3) // 4 * 4), device=x.device, dtype=torch.float32)
            check(L.somi_bn_act_backward_pooled_nhwc_f32(_ptr(None if dz is None else _f32c(dz)), 0 if dz is None else dz.shape[3], dz_coff,
                                                         _ptr(_f32c(x)), x.shape[3], x_coff, _ptr(mean),
                                                         _ptr(rstd), _ptr(scale), _ptr(shift), ACT[act], order, _ptr(davg), _ptr(dmax),
                                                         _ptr(amaxp), _ptr(_f32c(dx)), dx.shape[3], dx_coff, _ptr(dgamma), _ptr(dbeta), B, HW, c,
                                                         _ptr(ws), _stream()), 'bn_act_backward_pooled')
            return dx
        if dz is None:                                            # dz = None: the pooled part is the whole incoming gradient
            dz, dz_coff = torch.zeros_like(x), x_coff
        pool_backward_add_(dz, dz_coff, davg.shape[1], davg, dmax, amaxp)
    if SYNC_BN is not None and batch_stats:
        L = _lib.lib()
        dzc, xc, dxc = _f32c(dz), _f32c(x), _f32c(dx)
        rec = torch.empty(2 * c + 1, device=x.device, dtype=torch.float64)
        ws = torch.empty(2 * L.somi_red_nchunk(n) * c + 3 * ((c + 3) // 4 * 4), device=x.device, dtype=torch.float32)
        check(L.somi_bn_act_backward_sums_f64(_ptr(dzc), dzc.shape[3], dz_coff, _ptr(xc), xc.shape[3], x_coff, _ptr(mean), _ptr(scale),
                                              _ptr(shift), ACT[act], order, n, c, _ptr(rec), _ptr(ws), _stream()), 'bn_act_backward_sums')
        allrec, world = _gather_records(rec)
        check(L.somi_bn_act_backward_apply_sync_f32(_ptr(dzc), dzc.shape[3], dz_coff, _ptr(xc), xc.shape[3], x_coff, _ptr(mean), _ptr(rstd),
                                                    _ptr(scale), _ptr(shift), ACT[act], order, _ptr(rec), _ptr(allrec), world, _ptr(dxc),
                                                    dxc.shape[3], dx_coff, _ptr(dgamma), _ptr(dbeta), n, c, _ptr(ws), _stream()),
              'bn_act_backward_apply_sync')
        return dx
    ws = torch.empty(2 * _lib.lib().somi_red_nchunk(n) * c + 3 * ((c + 3) // 4 * 4), device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_bn_act_backward_nhwc_f32(_ptr(_f32c(dz)), dz.shape[3], dz_coff, _ptr(_f32c(x)), x.shape[3], x_coff, _ptr(mean),
                                                   _ptr(rstd), _ptr(scale), _ptr(shift), ACT[act], order, int(batch_stats), _ptr(_f32c(dx)),
                                                   dx.shape[3], dx_coff, _ptr(dgamma), _ptr(dbeta), n, c, _ptr(ws), _stream()),
          'bn_act_backward')
    return dx


def chan_sum_(x, c, x_coff, out_accumulate):
    n = _npix(x)
    ws = torch.empty(2 * _lib.lib().somi_red_nchunk(n) * c, device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_chan_sum_nhwc_f32(_ptr(_f32c(x)), x.shape[3], x_coff, n, c, _ptr(out_accumulate), _ptr(ws), _stream()), 'chan_sum')
    return out_accumulate


def add_(a, a_coff, b, b_coff, c, out=None, out_coff=None):
    """out[slice] = a[slice] + b[slice]; defaults to in place on a."""
    out = a if out is None else out
    out_coff = a_coff if out_coff is None else out_coff
    check(_lib.lib().somi_add_nhwc_f32(_ptr(_f32c(a)), a.shape[3], a_coff, _ptr(_f32c(b)), b.shape[3], b_coff, _ptr(_f32c(out)),
                                       out.shape[3], out_coff, _npix(a), c, _stream()), 'add')
    return out


def cbam_backward(dt2, t, t_coff, c, ca, sa, stats, w7, k, dw7, db7, t_max, dw_chw=False, bn=None):
    """Steps A-D of train_blocks.hip: turns d(t*ca*sa) (dt2, whole tensor, modified in place) into the part of dt that flows
    through the two multiplications and the spatial branch; returns dca (B,C) and amaxp (B,C) int32: the first pixel that holds each channel's
    maximum (step D, found by value inside step A's pass from t_max (B,C), the spatial maximum of t the forward pooled).
    dw7 / db7 are accumulated; dw7 is [k][k][2] like w7, or (dw_chw) laid out (2,k,k) like nn.Conv2d's weight.
    bn = (y, scale, shift, mean) of the Conv -> BatchNorm -> SiLU that produced t: step C is NOT run as a pass of its own - dt2 is left
    alone, dca comes from the reduction half of the fused BatchNorm backward, and a third value is returned: the state cbam_bn_backward_apply needs."""
    B, H, W, _ = t.shape
    dev = t.device
    L = _lib.lib()
    dlogit = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    amaxc = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    amaxp = torch.empty(B, c, device=dev, dtype=torch.int32)
    check(L.somi_cbam_bwd_pixel_argmax_f32(_ptr(_f32c(dt2)), dt2.shape[3], 0, _ptr(_f32c(t)), t.shape[3], t_coff, _ptr(ca), _ptr(sa), _ptr(t_max),
                                           _ptr(dlogit), _ptr(amaxc), _ptr(amaxp), B, H * W, c, _stream()), 'cbam_bwd_pixel')
    dstats = torch.empty(B, H, W, 2, device=dev, dtype=torch.float32)
    ws = torch.empty(((B * H * W + 511) // 512) * (2 * k * k + 1), device=dev, dtype=torch.float32)
    check(L.somi_spatial_attn_bwd_f32(_ptr(dlogit), _ptr(stats), _ptr(w7), _ptr(dstats), _ptr(dw7), _ptr(db7), _ptr(ws), B, H, W, k,
                                      int(dw_chw), _stream()), 'spatial_attn_bwd')
    dca = torch.empty(B, c, device=dev, dtype=torch.float32)
    if bn is not None:
        y, scale, shift, mean = bn
        ws3 = torch.empty(L.somi_cbam_bn_bwd_workspace_floats(B, H * W, c), device=dev, dtype=torch.float32)
        head = (_ptr(_f32c(dt2)), dt2.shape[3], 0, _ptr(_f32c(y)), y.shape[3], 0, _ptr(scale), _ptr(shift), _ptr(mean))
        check(L.somi_cbam_bn_bwd_reduce_f32(*head, _ptr(ca), _ptr(sa), _ptr(dstats), _ptr(amaxc), _ptr(amaxp), _ptr(dca), _ptr(ws3), B, H * W, c,
                                            _stream()), 'cbam_bn_bwd_reduce')
        return dca, amaxp, (dt2, y, scale, shift, mean, ca, sa, dstats, amaxc, amaxp, ws3, c)
    ws2 = torch.empty(B * L.somi_img_nchunk(H * W) * c, device=dev, dtype=torch.float32)
    check(L.somi_cbam_bwd_chan_f32(_ptr(dt2), dt2.shape[3], 0, _ptr(t), t.shape[3], t_coff, _ptr(ca), _ptr(sa), _ptr(dstats), _ptr(amaxc),
                                   _ptr(dca), _ptr(ws2), B, H * W, c, _stream()), 'cbam_bwd_chan')
    return dca, amaxp


def cbam_bn_backward_apply(state, rstd, davg, dmax, dx, dgamma, dbeta):
    """Second half of the fused CBAM + BatchNorm backward (somi_cbam_bn_bwd_apply_f32): state from cbam_backward(bn=...), davg / dmax (B,C) from the
    channel attention's MLP backward on the dca it returned; writes the gradient w.r.t. the convolution output into dx, accumulates dgamma / dbeta."""
    d, y, scale, shift, mean, ca, sa, dstats, amaxc, amaxp, ws, c = state
    B, H, W, _ = y.shape
    check(_lib.lib().somi_cbam_bn_bwd_apply_f32(_ptr(d), d.shape[3], 0, _ptr(y), y.shape[3], 0, _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd), _ptr(ca),
                                                _ptr(sa), _ptr(dstats), _ptr(amaxc), _ptr(amaxp), _ptr(davg), _ptr(dmax), _ptr(_f32c(dx)), dx.shape[3], 0,
                                                _ptr(dgamma), _ptr(dbeta), _ptr(ws), B, H * W, c, _stream()), 'cbam_bn_bwd_apply')
    return dx


def attn_mlp_backward(mode, dout, out, avg, mx, W1, b1, W2, dW1, db1, dW2, db2):
    B, Cc = avg.shape
    davg = torch.empty_like(avg)
    dmax = torch.empty_like(avg) if mode == 0 else None
    L = _lib.lib()
    ws = torch.empty(L.somi_attn_mlp_bwd_workspace_floats(B, Cc, W1.shape[0]), device=avg.device, dtype=torch.float32)
    check(L.somi_attn_mlp_bwd_f32(mode, _ptr(dout), _ptr(out), _ptr(avg), _ptr(mx), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(dW1),
                                  _ptr(db1), _ptr(dW2), _ptr(db2), _ptr(davg), _ptr(dmax), _ptr(ws), B, Cc, W1.shape[0], _stream()),
          'attn_mlp_bwd')
    return davg, dmax


def pool_backward_add_(dt, d_coff, c, davg, dmax=None, amaxp=None):
    B, H, W, cs = dt.shape
    check(_lib.lib().somi_pool_bwd_add_nhwc_f32(_ptr(_f32c(dt)), cs, d_coff, _ptr(davg), _ptr(dmax), _ptr(amaxp), B, H * W, c, _stream()),
          'pool_bwd_add')
    return dt


def detect_raw_backward(draw, box_cs, cls_cs, na, nc):
    B, _, ny, nx, _ = draw.shape
    dbox = torch.empty(B, ny, nx, box_cs, device=draw.device, dtype=torch.float32)
    dcls = torch.empty(B, ny, nx, cls_cs, device=draw.device, dtype=torch.float32)
    check(_lib.lib().somi_detect_raw_bwd_f32(_ptr(_f32c(draw)), _ptr(dbox), box_cs, _ptr(dcls), cls_cs, B, ny, nx, na, nc, _stream()),
          'detect_raw_bwd')
    return dbox, dcls


def sppf_pool_backward_(buf, dbuf, c, x_coff=0, codes=None):
    """codes: what sppf_pool_(codes=True) returned (then `buf` is not read); else the windows are searched again."""
    B, H, W, cs = dbuf.shape
    ws = torch.empty(3 * B * H * W * c, device=dbuf.device, dtype=torch.uint8) if codes is None else codes
    check(_lib.lib().somi_sppf_pool_bwd_nhwc_f32(_ptr(_f32c(buf)) if codes is None else None, _ptr(_f32c(dbuf)), _ptr(ws), B, H, W, c, cs, x_coff,
                                                 _stream()), 'sppf_pool_bwd')
    return dbuf


def bifpn_backward(srcs, ups, w_dev, dout, dw, eps=1e-4):
    n = len(srcs)
    B, H, W, Cc = dout.shape
    dsrcs = [torch.empty_like(s) for s in srcs]
    sp = (C.c_void_p * n)(*[_ptr(_f32c(s)) for s in srcs])
    dp = (C.c_void_p * n)(*[_ptr(d) for d in dsrcs])
    ws = torch.empty(3 * 2048, device=dout.device, dtype=torch.float32)
    check(_lib.lib().somi_bifpn_bwd_nhwc_f32(sp, dp, (C.c_int * n)(*ups), _ptr(_f32c(w_dev)), float(eps), n,
                                             _ptr(_f32c(dout)), _ptr(dw), _ptr(ws), B, H, W, Cc, _stream()), 'bifpn_bwd')
    return dsrcs


def dwconv3x3_backward(dy, x, w, dw, dbias, dx_accumulate=None):
    B, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    ws = torch.empty(max(_lib.lib().somi_dwconv3x3_bwd_workspace_floats(B, W, Cc), 1), device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_dwconv3x3_bwd_nhwc_f32(_ptr(_f32c(dy)), _ptr(_f32c(x)), _ptr(w), _ptr(dx), _ptr(dx_accumulate), _ptr(dw), _ptr(dbias),
                                                 _ptr(ws), B, H, W, Cc, _stream()), 'dwconv3x3_bwd')
    return dx


def scale_channels_backward(dout, x, s):
    B, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    ds = torch.empty(B, Cc, device=x.device, dtype=torch.float32)
    ws = torch.empty(B * _lib.lib().somi_img_nchunk(H * W) * Cc, device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_scale_channels_bwd_nhwc_f32(_ptr(_f32c(dout)), _ptr(_f32c(x)), _ptr(s), _ptr(dx), _ptr(ds), _ptr(ws), B, H * W, Cc,
                                                      _stream()), 'scale_channels_bwd')
    return dx, ds


def linear(x, W, bias, act, out=None, out_off=0):
    """Small dense layer on (B, nin) rows (ODConv attention heads): out[:, out_off:out_off+nout] = act(x W^T + bias)."""
    B, nin = x.shape
    nout = W.shape[0]
    out = torch.empty(B, nout, device=x.device, dtype=torch.float32) if out is None else out
    check(_lib.lib().somi_linear_f32(_ptr(_f32c(x)), x.shape[1], _ptr(_f32c(W)), _ptr(bias), ACT[act], _ptr(out), out.shape[1], out_off, B, nin,
                                     nout, _stream()), 'linear')
    return out


def linear_backward(x, W, dy, y, off, act, dW, db, dx=None, accumulate=False):
    B, nin = x.shape
    nout = W.shape[0]
    ws = torch.empty(B * nout, device=x.device, dtype=torch.float32)
    check(_lib.lib().somi_linear_bwd_f32(_ptr(_f32c(x)), nin, _ptr(_f32c(W)), _ptr(dy), _ptr(y), y.shape[1], off, ACT[act], _ptr(dW), _ptr(db),
                                         _ptr(dx), dx.shape[1] if dx is not None else 0, int(accumulate), _ptr(ws), B, nin, nout, _stream()),
          'linear_bwd')
    return dx


def odconv_synth(attn, Wk, biask, cin, cin_pad, cout, kk, K):
    B = attn.shape[0]
    wout = torch.empty(B, cout, kk * cin_pad, device=attn.device, dtype=torch.float32)
    bout = torch.empty(B, cout, device=attn.device, dtype=torch.float32)
    check(_lib.lib().somi_odconv_synth_f32(_ptr(attn), _ptr(Wk), _ptr(biask), _ptr(wout), _ptr(bout), B, cin, cin_pad, cout, kk, K, _stream()),
          'odconv_synth')
    return wout, bout


def odconv_synth_backward(dWb, attn, Wk, biask, dbias_b, dWk, dbiask, cin, cin_pad, cout, kk, K):
    B = attn.shape[0]
    dattn = torch.empty_like(attn)
    L = _lib.lib()
    ws = torch.empty(L.somi_odconv_synth_bwd_workspace_floats(B, cin, cout, kk, K), device=attn.device, dtype=torch.float32)
    check(L.somi_odconv_synth_bwd_f32(_ptr(_f32c(dWb)), _ptr(attn), _ptr(Wk), _ptr(biask), _ptr(dbias_b), _ptr(dWk), _ptr(dbiask),
                                      _ptr(dattn), _ptr(ws), B, cin, cin_pad, cout, kk, K, _stream()), 'odconv_synth_bwd')
    return dattn
