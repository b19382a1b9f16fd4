"""Plain-PyTorch restatement of the reference's ASF-YOLO neck, the CPU oracle of tests/test_asf_host.py and tests/test_asf_gpu.py: Zoom_cat
(models/common.py:4312-4327), ScalSeq (:4330-4355) and attention_model with channel_att and local_att (:4358-4424), written from their
semantics, literally (the stacked (B,C,3,H,W) tensor, the upsampled maps) and in the low-resolution form the kernels compute:

  * Zoom_cat: the 2x2 max plus the 2x2 mean of l, m, and s replicated 2x, concatenated.  A tie in a window goes to its first pixel in
    row-major order (adaptive_max_pool2d);
  * ScalSeq: the Conv3d(1x1x1) acts per pixel and nearest upsampling at exactly 2x and 4x only replicates pixels, so u_i = conv3d(.) can be
    taken at each level's own resolution; the BatchNorm3d batch statistics over the stack are the three maps' sums weighted 1, 4 and 16 with
    N = 3 B H W (running variance times N / (N - 1)); the depth maximum is taken after the affine and the LeakyReLU, a tie going to the first
    depth index (p3, then p4, then p5).  scalseq_lowres(weights=(1, 1, 1)) and scalseq_lowres(count='BHW') are WRONG variants the host tests
    rule out;
  * attention_model: t = x1 * sigmoid(conv1d_k(mean of x1)) + x2, then t * s_h * s_w with the two gates from t's row and column means.

tests/golden/block_asf_*.npz, generated from the reference's own classes, pin the literal forms.  register(monkeypatch) puts the three names
into the oracle's parser for the length of a test."""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


# ---------------------------------------------------------------------------------------------- the literal forms
class Zoom_cat(nn.Module):
    def __init__(self, in_dim):
        super().__init__()

    def forward(self, x):
        l, m, s = x
        size = m.shape[2:]
        pooled = F.adaptive_max_pool2d(l, size) + F.adaptive_avg_pool2d(l, size)
        return torch.cat([pooled, m, F.interpolate(s, size, mode='nearest')], 1)


class ScalSeq(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.conv1 = OB.Conv(512, channel, 1)
        self.conv2 = OB.Conv(1024, channel, 1)
        self.conv3d = nn.Conv3d(channel, channel, kernel_size=(1, 1, 1))
        self.bn = nn.BatchNorm3d(channel)
        self.act = nn.LeakyReLU(0.1)
        self.pool_3d = nn.MaxPool3d(kernel_size=(3, 1, 1))

    def forward(self, x):
        p3, p4, p5 = x
        size = p3.shape[2:]
        levels = [p3, F.interpolate(self.conv1(p4), size, mode='nearest'), F.interpolate(self.conv2(p5), size, mode='nearest')]
        stack = torch.stack(levels, 2)                            # (B, C, 3, H, W)
        return self.pool_3d(self.act(self.bn(self.conv3d(stack)))).squeeze(2)


def eca_kernel_size(channel, b=1, gamma=2):
    k = int(abs((math.log(channel, 2) + b) / gamma))
    return k if k % 2 else k + 1


class channel_att(nn.Module):
    def __init__(self, channel, b=1, gamma=2):
        super().__init__()
        k = eca_kernel_size(channel, b, gamma)
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv = nn.Conv1d(1, 1, kernel_size=k, padding=(k - 1) // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        avg = x.mean((2, 3))                                      # (B, C): the conv runs along the channels
        return x * self.sigmoid(self.conv(avg[:, None, :]))[:, 0, :, None, None]


class local_att(nn.Module):
    def __init__(self, channel, reduction=16):
        super().__init__()
        self.conv_1x1 = nn.Conv2d(channel, channel // reduction, kernel_size=1, stride=1, bias=False)
        self.relu = nn.ReLU()
        self.bn = nn.BatchNorm2d(channel // reduction)
        self.F_h = nn.Conv2d(channel // reduction, channel, kernel_size=1, stride=1, bias=False)
        self.F_w = nn.Conv2d(channel // reduction, channel, kernel_size=1, stride=1, bias=False)
        self.sigmoid_h = nn.Sigmoid()
        self.sigmoid_w = nn.Sigmoid()

    def forward(self, x):
        h, w = x.shape[2:]
        rows = x.mean(3, keepdim=True)                            # (B, C, H, 1)
        cols = x.mean(2, keepdim=True).transpose(2, 3)            # (B, C, W, 1)
        y = self.relu(self.bn(self.conv_1x1(torch.cat([rows, cols], 2))))
        s_h = self.sigmoid_h(self.F_h(y[:, :, :h]))               # (B, C, H, 1)
        s_w = self.sigmoid_w(self.F_w(y[:, :, h:])).transpose(2, 3)
        return x * s_h * s_w


class attention_model(nn.Module):
    def __init__(self, ch=256):
        super().__init__()
        self.channel_att = channel_att(ch)
        self.local_att = local_att(ch)

    def forward(self, x):
        return self.local_att(self.channel_att(x[0]) + x[1])


# ---------------------------------------------------------------------------------------------- the low-resolution form of ScalSeq
def first_max(levels):
    """Maximum over a list of equal-shape tensors, a tie going to the first: -> (values, index of the winner)."""
    best, idx = levels[0], torch.zeros_like(levels[0], dtype=torch.long)
    for i, v in enumerate(levels[1:], 1):
        take = v > best
        best, idx = torch.where(take, v, best), torch.where(take, torch.full_like(idx, i), idx)
    return best, idx


def up(t, n):
    return t.repeat_interleave(n, 2).repeat_interleave(n, 3)


def union_stats(us, weights=(1, 4, 16), count='3BHW'):
    """Per-channel mean and biased variance of the NCHW maps us = (u3, u4, u5) weighted as the stack holds them -> (mean, var, N)."""
    B, _, H, W = us[0].shape
    N = {'3BHW': 3 * B * H * W, 'BHW': B * H * W}[count]
    mean = sum(w * u.sum((0, 2, 3)) for w, u in zip(weights, us)) / N
    var = sum(w * ((u - mean[None, :, None, None]) ** 2).sum((0, 2, 3)) for w, u in zip(weights, us)) / N
    return mean, var, N


def scalseq_lowres(mod, x, weights=(1, 4, 16), count='3BHW'):
    """ScalSeq's forward on the module `mod` (the literal class above) without the stack and without upsampled inputs of the conv: differentiable,
    updates mod.bn's running buffers in training mode as nn.BatchNorm3d does.  weights / count other than the defaults are the WRONG variants."""
    p3, p4, p5 = x
    c = mod.conv3d.out_channels
    w, b = mod.conv3d.weight.view(c, c), mod.conv3d.bias
    us = [torch.einsum('oc,bchw->bohw', w, t) + b[None, :, None, None] for t in (p3, mod.conv1(p4), mod.conv2(p5))]
    bn = mod.bn
    if mod.training:
        mean, var, N = union_stats(us, weights, count)
        with torch.no_grad():
            bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean)
            bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * var * N / (N - 1))
            bn.num_batches_tracked += 1
    else:
        mean, var = bn.running_mean, bn.running_var
    scale = bn.weight / torch.sqrt(var + bn.eps)
    shift = bn.bias - mean * scale
    zs = [F.leaky_relu(u * scale[None, :, None, None] + shift[None, :, None, None], 0.1) for u in us]
    return first_max([zs[0], up(zs[1], 2), up(zs[2], 4)])[0]


# ---------------------------------------------------------------------------------------------- fp64 references of the kernels (NHWC)
def windows2(l):
    """(B,2H,2W,C) -> the four window positions in row-major order, each (B,H,W,C)."""
    return [l[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]


def zoomcat_ref(l, m, s):
    """-> (out (B,H,W,Cl+Cm+Cs), codes (B,H,W,Cl) = the window position 2i + j of the maximum, the first on a tie).  s is read at
    (h >> 1, w >> 1), which is nearest interpolation for a small map of (H + 1) // 2 x (W + 1) // 2."""
    H, W = m.shape[1:3]
    win = windows2(l)
    mx, codes = first_max(win)
    return torch.cat([mx + sum(win) / 4, m, up(s.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)[:, :H, :W]], -1), codes


def zoomcat_bwd_ref(dout, codes, cl, cm):
    """-> (dl, dm, ds) from the definition: dl[2h+i, 2w+j] = dout_l (1/4 + [code == 2i + j]), ds = the sum over the pixels a small-map pixel fed."""
    B, H, W, _ = dout.shape
    dl = dout.new_zeros(B, 2 * H, 2 * W, cl)
    for k, (i, j) in enumerate((i, j) for i in (0, 1) for j in (0, 1)):
        dl[:, i::2, j::2] = dout[..., :cl] * (0.25 + (codes == k).to(dout.dtype))
    d_s = dout[..., cl + cm:]
    d_s = F.pad(d_s, (0, 0, 0, W % 2, 0, H % 2))                  # an odd map: the missing children are zeros
    Hs, Ws = d_s.shape[1] // 2, d_s.shape[2] // 2
    return dl, dout[..., cl:cl + cm], d_s.reshape(B, Hs, 2, Ws, 2, -1).sum((2, 4))


def scalseq_tail_ref(us, gamma, beta, eps, dout=None):
    """The tail behind the NHWC maps us = (u3, u4, u5) in their dtype (fp64 in the tests): statistics, output, codes and - with dout - the
    backward's g_i, sums, du_i (autograd through the batch statistics), dgamma, dbeta."""
    us = [u.detach().clone().requires_grad_(True) for u in us]
    nc = [u.permute(0, 3, 1, 2) for u in us]
    gamma, beta = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    mean, var, N = union_stats(nc)
    rstd = 1 / torch.sqrt(var + eps)
    scale, shift = gamma * rstd, beta - mean * gamma * rstd
    ys = [u * scale + shift for u in us]
    zs = [F.leaky_relu(y, 0.1) for y in ys]
    full = [zs[0], up(zs[1].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1), up(zs[2].permute(0, 3, 1, 2), 4).permute(0, 2, 3, 1)]
    out, codes = first_max(full)
    r = dict(mean=mean.detach(), var=var.detach(), var_unbiased=(var * N / (N - 1)).detach(), rstd=rstd.detach(), scale=scale.detach(),
             shift=shift.detach(), out=out.detach(), codes=codes, candidates=[f.detach() for f in full])
    if dout is None:
        return r
    out.backward(dout)
    B, H, W, C = us[0].shape
    gs = []
    for i, (y, n) in enumerate(zip(ys, (1, 2, 4))):
        routed = (dout * (codes == i)).reshape(B, H // n, n, W // n, n, C).sum((2, 4))
        gs.append(routed * torch.where(y.detach() > 0, torch.ones_like(routed), torch.full_like(routed, 0.1)))
    xh = [((u - mean) * rstd).detach() for u in us]
    r.update(g=gs, sum_g=sum(g.sum((0, 1, 2)) for g in gs), sum_gx=sum((g * x).sum((0, 1, 2)) for g, x in zip(gs, xh)),
             du=[u.grad for u in us], dgamma=gamma.grad, dbeta=beta.grad)
    return r


def eca_ref(avg, w, dgate=None):
    """gate = sigmoid(conv1d(avg)) along the channels, zero-padded; with dgate -> (gate, davg, dw)."""
    avg, w = avg.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    gate = torch.sigmoid(F.conv1d(avg[:, None, :], w.view(1, 1, -1), padding=w.numel() // 2))[:, 0]
    if dgate is None:
        return gate.detach()
    gate.backward(dgate)
    return gate.detach(), avg.grad, w.grad


# ---------------------------------------------------------------------------------------------- one-tensor faces for parity.check_block
class Packed(nn.Module):
    """A several-input block behind parity.check_block's one-tensor procedure: the input is (B, n, 1, 1), every image's n values the inputs'
    (C, H, W) blocks flattened one after the other.  `shapes`: the (C, H, W) of the inputs.  Around the restatement it splits the NCHW tensor
    (autograd sees the split); around a somi_amd block it builds the NHWC Acts and gathers backward's list of gradients back into one Act."""

    def __init__(self, inner, shapes, mine):
        super().__init__()
        self.inner, self.shapes, self.mine = inner, [tuple(s) for s in shapes], mine

    def _split(self, flat):
        parts, o = [], 0
        for c, h, w in self.shapes:
            parts.append(flat[:, o:o + c * h * w].reshape(-1, c, h, w))
            o += c * h * w
        return parts

    def forward(self, x):
        if not self.mine:
            return self.inner(self._split(x[:, :, 0, 0]))
        from somi_amd.blocks import Act
        return self.inner([Act(p.permute(0, 2, 3, 1).contiguous()) for p in self._split(x.t[:, 0, 0, x.coff:x.coff + x.c])])

    def backward(self, dout):
        from somi_amd.blocks import Act
        ds = self.inner.backward(dout)
        flat = torch.cat([d.t[..., d.coff:d.coff + d.c].permute(0, 3, 1, 2).reshape(d.t.shape[0], -1) for d in ds], 1)
        return Act(flat[:, None, None, :].contiguous())


def packed(ns, make, shapes):
    """make(ns) behind Packed; ns is this module (the restatement) or somi_amd.blocks."""
    return Packed(make(ns), shapes, ns.__name__ != __name__)


# tag -> (constructor over a namespace, the inputs' NCHW shapes); the first four are the fixtures' blocks and shapes (tests/golden/block_<tag>.npz)
BLOCKS = {
    'asf_zoom_cat': (lambda ns: ns.Zoom_cat(8), [(2, 4, 4, 8), (2, 8, 2, 4), (2, 12, 1, 2)]),          # unequal widths
    'asf_scalseq': (lambda ns: ns.ScalSeq(8), [(2, 8, 4, 8), (2, 512, 2, 4), (2, 1024, 1, 2)]),
    'asf_attention_64': (lambda ns: ns.attention_model(64), [(2, 64, 5, 7), (2, 64, 5, 7)]),            # k = 3
    'asf_attention_128': (lambda ns: ns.attention_model(128), [(1, 128, 3, 2), (1, 128, 3, 2)]),        # k = 5
    'asf_attention_256': (lambda ns: ns.attention_model(256), [(2, 256, 6, 10), (2, 256, 6, 10)]),
}
FIXTURES = [t for t in BLOCKS if t != 'asf_attention_256']


def packed_case(tag):
    """-> (make over a namespace, the (B, n, 1, 1) shape) for parity.check_block."""
    make, shapes = BLOCKS[tag]
    chw = [s[1:] for s in shapes]
    return (lambda ns: packed(ns, make, chw)), (shapes[0][0], sum(c * h * w for c, h, w in chw), 1, 1)


# ---------------------------------------------------------------------------------------------- the parser table
_ROWS = {'Zoom_cat': Zoom_cat, 'ScalSeq': ScalSeq, 'attention_model': attention_model}


def register(monkeypatch):
    """The three names in the oracle's parse_model (test-time only: nothing under oracle/ changes).  In the oracle's own pass each row stands as
    a Concat of the inputs whose widths add up to the row's c2 - all three for Zoom_cat (c2 = 3 * args[0], checked), the first one for
    ScalSeq and attention_model (c2 = args[0], the first input's width) - then the modules are built with their arguments as written and the
    save list is taken from the rows as written."""
    from oracle.somi_ref import model as OM
    inner = OM.parse_model

    def parse_model(d, ch):
        rows = d['backbone'] + d['head']
        swapped = dict(d, backbone=[], head=[[f if name == 'Zoom_cat' else f[:1], n, 'Concat', [1]] if name in _ROWS else [f, n, name, args]
                                             for f, n, name, args in rows])
        seq, _ = inner(swapped, ch)
        layers = list(seq)
        save = []
        for i, (f, n, name, args) in enumerate(rows):
            save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
            if name in _ROWS:
                m_ = _ROWS[name](*args)
                m_.i, m_.f, m_.type = i, f, name
                m_.np = sum(p.numel() for p in m_.parameters())
                layers[i] = m_
        return nn.Sequential(*layers), sorted(save)
    monkeypatch.setattr(OM, 'parse_model', parse_model)


def oracle_model(cfg):
    """The oracle Model of a yolov5_asf_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


GRAPH_SEED = 0


def graph_case():
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_asf_cfg(depth=0.33, nc=4), batch 2, 128 x 128."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_asf_cfg
    cfg = yolov5_asf_cfg(depth=0.33, nc=4)
    ref = fill_state(oracle_model(cfg), 1)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 128, nc=4, seed=GRAPH_SEED)
    return cfg, ref, imgs, targets

