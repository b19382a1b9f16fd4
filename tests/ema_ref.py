"""Plain-PyTorch restatement of the reference's efficient multi-scale attention, the CPU oracle of tests/test_ema_host.py and
tests/test_ema_gpu.py: EMA (models/common.py:5263-5292), iRMB_EMA (:5409-5451), iRMB_EMABottleneck (:5454-5470) and C2f_iRMB_EMA (:5473-5497),
written from their semantics:

  * the map is seen as `factor` groups of cg = channels / factor channels; every group of every image goes through the same weights;
  * a group is averaged over its width and over its height, the two results laid end to end go through ONE 1x1 conv (with bias), and the H-part
    and the W-part, each through a sigmoid, gate the group's pixels by row and by column; the gated group is normalised per channel over its
    pixels (a GroupNorm with one channel per group, affine, eps 1e-5): x1;
  * the group also goes through a 3x3 conv (with bias): x2;
  * the per-channel means of x1 and of x2, each soft-maxed over the cg channels, weigh the OTHER map; the two weighted sums over the channels, added,
    go through a sigmoid and gate every channel of the group's pixel;
  * iRMB_EMA at its defaults: a BatchNorm, EMA, e + SiLU(BatchNorm(depthwise 3x3 (e))), a 1x1 conv without bias, plus the block's input;
    iRMB_EMABottleneck attends the output of its conv pair and adds the input when shortcut and c1 == c2; C2f_iRMB_EMA is a C2f of such
    bottlenecks (3x3 / 3x3, e = 1.0).  tests/golden/block_ema*.npz, generated from the reference's own classes, pin all of that.

register(monkeypatch) teaches the oracle's parse_model the four names for the length of a test, as rows built from the yaml arguments as written
whose channels pass through (the reference's generic branch, models/yolo.py:1648-1650).  The kernel-level fp64 references of ema.hip are at the
end."""
import copy
import math
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


class EMA(nn.Module):
    def __init__(self, channels, factor=8):
        super().__init__()
        self.groups = factor
        cg = channels // factor
        assert cg > 0
        self.gn = nn.GroupNorm(cg, cg)
        self.conv1x1 = nn.Conv2d(cg, cg, 1)
        self.conv3x3 = nn.Conv2d(cg, cg, 3, padding=1)

    def forward(self, x):
        B, C, H, W = x.shape
        gx = x.reshape(B * self.groups, -1, H, W)
        hw = self.conv1x1(torch.cat([gx.mean(3), gx.mean(2)], 2).unsqueeze(3))             # (B g, cg, H + W, 1)
        a_h, a_w = torch.sigmoid(hw[:, :, :H]), torch.sigmoid(hw[:, :, H:]).transpose(2, 3)
        x1 = self.gn(gx * a_h * a_w)
        x2 = self.conv3x3(gx)
        p1 = F.softmax(x1.mean((2, 3)), 1)[:, :, None, None]
        p2 = F.softmax(x2.mean((2, 3)), 1)[:, :, None, None]
        wgt = (p1 * x2).sum(1, keepdim=True) + (p2 * x1).sum(1, keepdim=True)
        return (gx * torch.sigmoid(wgt)).reshape(B, C, H, W)


class _ConvNorm(nn.Module):
    """conv (no bias) [-> BatchNorm -> SiLU]: the children `conv` and `norm` of the reference's ConvNormAct."""

    def __init__(self, dim, k, groups, norm):
        super().__init__()
        self.conv = nn.Conv2d(dim, dim, k, 1, math.ceil((k - 1) / 2), groups=groups, bias=False)
        self.norm = nn.BatchNorm2d(dim, eps=1e-6) if norm else nn.Identity()
        self.act = nn.SiLU() if norm else nn.Identity()

    def forward(self, x):
        return self.act(self.norm(self.conv(x)))


class iRMB_EMA(nn.Module):
    def __init__(self, dim_in):
        super().__init__()
        self.norm = nn.BatchNorm2d(dim_in, eps=1e-6)
        self.ema = EMA(dim_in)
        self.conv_local = _ConvNorm(dim_in, 3, dim_in, True)
        self.proj = _ConvNorm(dim_in, 1, 1, False)

    def forward(self, x):
        e = self.ema(self.norm(x))
        return x + self.proj(e + self.conv_local(e))


class iRMB_EMABottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, k[0], 1)
        self.cv2 = OB.Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2
        self.iRMB = iRMB_EMA(c2)

    def forward(self, x):
        y = self.iRMB(self.cv2(self.cv1(x)))
        return x + y if self.add else y


class C2f_iRMB_EMA(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = OB.Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = OB.Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(iRMB_EMABottleneck(self.c, self.c, shortcut, g, k=(3, 3), e=1.0) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        for m in self.m:
            y.append(m(y[-1]))
        return self.cv2(torch.cat(y, 1))


_ROWS = {'EMA': EMA, 'iRMB_EMA': iRMB_EMA, 'iRMB_EMABottleneck': iRMB_EMABottleneck, 'C2f_iRMB_EMA': C2f_iRMB_EMA}


def register(monkeypatch):
    """The four names in the oracle's parse_model (test-time only: nothing under oracle/ changes): such a row is built here from its arguments as
    written and stands in the oracle's pass as an nn.Upsample row, which takes the same branch (c2 = ch[f])."""
    from oracle.somi_ref import model as OM
    inner = OM.parse_model

    def parse_model(d, ch):
        rows = d['backbone'] + d['head']
        swapped = dict(d, backbone=[], head=[[f, n, 'nn.Upsample', [None, 1, 'nearest']] if name in _ROWS else [f, n, name, args]
                                             for f, n, name, args in rows])
        seq, save = inner(swapped, ch)
        layers = list(seq)
        for i, (f, n, name, args) in enumerate(rows):
            if name in _ROWS:
                m_ = _ROWS[name](*args)
                m_.i, m_.f, m_.type = i, f, name
                m_.np = sum(p.numel() for p in m_.parameters())
                layers[i] = m_
        return nn.Sequential(*layers), save
    monkeypatch.setattr(OM, 'parse_model', parse_model)


def oracle_model(cfg):
    """The oracle Model of a yolov5_ema_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


# ---------------------------------------------------------------------------------------------- the seeded cases
# EMA has no kink and no arg-max, but conv1x1.bias is badly conditioned: its gradient is a sum over B * g * (H + W) rows of terms of both signs
# (the reference alone, fp32 CPU against fp64, reaches 1.7e-4 of its largest entry on some seeds).  So the seeded cases below are read from
# the reference alone: tools/gen_ema_golden.py --seeds prints, per candidate, the fp32 CPU restatement's worst parameter gradient against its fp64
# twin in units of the bar its test applies.  Blocks, input seeds 0..5: 0.001 .. 0.012 of 1e-3 * scale + 2e-5, outputs <= 9e-7 and dx <= 1.1e-6
# of their largest value - every candidate is far inside, seed 0 is taken.  Graphs, (fill, batch) in (1..3) x (0..2): 'c2f' 0.108 .. 0.243 of
# 2e-3 * scale + 2e-6, 'row' 0.054 .. 0.102; (1, 0) is taken for both (0.137 and 0.089).  tests/test_ema_host.py asserts half the bar there.
BLOCKS = {                         # tag -> (constructor over a namespace, NCHW shape)
    'ema32': (lambda ns: ns.EMA(32), (2, 32, 5, 7)),
    'ema16_f4': (lambda ns: ns.EMA(16, 4), (1, 16, 9, 4)),
    'ema256_f4': (lambda ns: ns.EMA(256, 4), (2, 256, 5, 7)),       # cg = 64: the widest group
    'irmb32': (lambda ns: ns.iRMB_EMA(32), (2, 32, 5, 7)),
    'bottleneck32': (lambda ns: ns.iRMB_EMABottleneck(32, 32, True), (2, 32, 5, 7)),
    'bottleneck32_nosc': (lambda ns: ns.iRMB_EMABottleneck(32, 32, False), (2, 32, 5, 7)),
    'c2f32': (lambda ns: ns.C2f_iRMB_EMA(32, 32, 1), (2, 32, 5, 7)),          # hidden width 16: EMA(16) has cg = 2, refused on the path
    'c2f64_n2': (lambda ns: ns.C2f_iRMB_EMA(64, 64, 2, True), (2, 64, 6, 5)),
}
GPU_BLOCKS = [t for t in BLOCKS if t != 'c2f32']
BLOCK_SEEDS = {'ema32': 0, 'ema16_f4': 0, 'ema256_f4': 0, 'irmb32': 0, 'bottleneck32': 0, 'bottleneck32_nosc': 0, 'c2f32': 0, 'c2f64_n2': 0}
# where -> (fill_state seed, synthetic_batch seed); candidates (1..3) x (0..2)
GRAPH_SEEDS = {'c2f': (1, 0), 'row': (1, 0)}
GRAPH_WIDTH = 0.5                  # 'c2f' at 0.25 would have a hidden width of 16 in its first block: two channels per group


def block_case(tag, seed=None):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    make, shape = BLOCKS[tag]
    ref = make(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*shape, generator=gen), gen


def graph_case(where, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_ema_cfg at width 0.5, nc 10, batch 2, 64x64."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_ema_cfg
    fill, batch = GRAPH_SEEDS[where] if seeds is None else seeds
    cfg = yolov5_ema_cfg(GRAPH_WIDTH, 0.33, nc=10, where=where)
    ref = fill_state(oracle_model(cfg), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=10, seed=batch)
    return cfg, ref, imgs, targets


def worst_grad_ratio(ref, ref64, rel, atol):
    """The fp32 module's worst parameter gradient against its fp64 twin's, in units of rel * scale + atol."""
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    return worst


# ---------------------------------------------------------------------------------------------- kernel-level references (NHWC)
EPS = 1e-5

# (B, H, W, C, factor): C 16 with factor 4, 32 (cg = 4: one quad per group), 64, 256 (cg = 32), 256 with factor 4 (cg = 64: the widest group);
# maps 5x7 (H = 5: two row chunks of 4, so two partials per (b, c); C = 256: two column chunks as well), 1x3 and 1x1; 9x70 at C = 16 (more than
# one workgroup along W); 48 channels with factor 4 (cg = 12: groups of three lanes, 21 columns per workgroup, groups across wave boundaries)
KERNEL_SHAPES = [(2, 5, 7, 32, 8), (1, 5, 7, 16, 4), (2, 5, 7, 64, 8), (1, 5, 7, 256, 8), (1, 5, 7, 256, 4), (2, 1, 3, 32, 8), (2, 1, 1, 32, 8),
                 (1, 1, 1, 256, 8), (1, 9, 70, 16, 4), (1, 5, 23, 48, 4)]
KERNEL_CASES = [(s, kind) for s in KERNEL_SHAPES for kind in ('plain',)] + [((2, 5, 7, 32, 8), 'pooled50'), ((2, 5, 7, 64, 8), 'mean30'),
                                                                            ((1, 5, 7, 256, 8), 'pooled50')]


def kernel_inputs(shape, kind='plain', seed=None):
    """The fp32 inputs of the four kernels.  kind: 'plain'; 'pooled50': x2 with per-(b, c) means of magnitude ~50 (a softmax without the
    maximum subtracted overflows); 'mean30': x with a per-channel mean about 30 times its spread (a naive variance fails)."""
    B, H, W, C, g = shape
    cg = C // g
    gen = torch.Generator().manual_seed(sum(shape) * 7 + len(kind) if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    t = dict(x=r(B, H, W, C), x2=r(B, H, W, C), hw=r(B, H + W, C), dout=r(B, H, W, C), res=r(B, H, W, C), have=r(B, H, W, C),
             gamma=1 + 0.3 * r(cg), beta=0.5 * r(cg))
    if kind == 'pooled50':
        t['x2'] = t['x2'] + 50.0 * r(B, 1, 1, C)
    if kind == 'mean30':
        t['x'] = 30.0 + t['x']
        t['hw'] = 0.1 * t['hw'] + 3.0                             # gates near 1 and nearly flat: t keeps a mean of ~30 spreads
    return t


def kernel_forward(t, g, dtype=torch.float64, literal=True):
    """The forward from the inputs (autograd leaves where they take gradients).  -> dict of results.  literal: x11 = softmax(mean x1), the
    reference's formula; else softmax(beta)."""
    x, x2, hw, gamma, beta = (t[k].to(dtype) for k in ('x', 'x2', 'hw', 'gamma', 'beta'))
    B, H, W, C = x.shape
    cg = C // g
    sg = torch.sigmoid(hw)
    tt = x * sg[:, :H, None] * sg[:, None, H:]
    mean = tt.mean((1, 2))
    m2 = ((tt - mean[:, None, None]) ** 2).sum((1, 2))
    rstd = 1 / torch.sqrt(m2 / (H * W) + EPS)
    th = (tt - mean[:, None, None]) * rstd[:, None, None]
    x1 = gamma.repeat(g) * th + beta.repeat(g)
    mx2 = x2.mean((1, 2))
    x21 = F.softmax(mx2.view(B, g, cg), -1).view(B, C)
    x11 = F.softmax((x1.mean((1, 2)) if literal else beta.repeat(g).expand(B, C)).reshape(B, g, cg), -1).view(B, C)
    wgt = (x11[:, None, None] * x2 + x21[:, None, None] * x1).view(B, H, W, g, cg).sum(-1)
    s = torch.sigmoid(wgt).repeat_interleave(cg, -1)
    return dict(sg=sg, t=tt, mean=mean, m2=m2, rstd=rstd, mx2=mx2, x21=x21, x11=x11, x1=x1, wgt=wgt, s=s, out=x * s)


def kernel_reference(t, g, dtype=torch.float64):
    """fp64 (or fp32, for the host test's half-bar check) results of the four kernels, the backward by autograd of the literal formula:
    stats (B, 3, C), vec (B, 4, C), out, out_res; dx (direct part) and dt with dx + dt * gates = autograd's dx; dx2, dsg (the gradient of hw),
    dgamma, dbeta; dw = dwgt over the group's channels, sums (B, 3, C)."""
    leaves = {k: t[k].to(dtype).clone().requires_grad_(True) for k in ('x', 'x2', 'hw', 'gamma', 'beta')}
    f = kernel_forward(leaves, g, dtype)
    f['wgt'].retain_grad()
    f['t'].retain_grad()
    dout = t['dout'].to(dtype)
    f['out'].backward(dout)
    B, H, W, C = t['x'].shape
    cg = C // g
    with torch.no_grad():
        dw = f['wgt'].grad.repeat_interleave(cg, -1)
        dx = dout * f['s']
        th = (f['t'] - f['mean'][:, None, None]) * f['rstd'][:, None, None]
        sums = torch.stack([(dw * th).sum((1, 2)), dw.sum((1, 2)), (dw * leaves['x2']).sum((1, 2))], 1)
        want = dict(stats=torch.stack([f['mean'], f['m2'], f['mx2']], 1),
                    vec=torch.stack([f['mean'], f['rstd'], f['x21'], f['x11']], 1),
                    out=f['out'], out_res=f['out'] + t['res'].to(dtype), dx=dx, dw=dw, sums=sums, dt=f['t'].grad, dx2=leaves['x2'].grad,
                    dsg=leaves['hw'].grad, dgamma=leaves['gamma'].grad, dbeta=leaves['beta'].grad, dx_total=leaves['x'].grad, sg=f['sg'])
    return {k: v.detach() for k, v in want.items()}
