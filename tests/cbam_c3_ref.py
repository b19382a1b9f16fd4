"""Plain-PyTorch restatement of the reference's CBAM C3 family, the CPU oracle of tests/test_cbam_c3_host.py and tests/test_cbam_c3_gpu.py:
DepthWiseConv and SpatialAttentionModuleDWC (models/common.py:361-389, 425-438), CBAMBottleneckDWC (:953-972), SCBAMBottleneck (:975-995),
C3CBAM (:494-504) and the five C3 variants C3_CBAM, C3_CBAMS, C3_CBAM_DWC, C3_CBAMS_DWC, C3_SCBAM (:1640-1705), written from their semantics
over oracle.somi_ref.blocks (Conv, C3, CBAMBottleneck, ChannelAttentionModule, SpatialAttentionModule):

  * the C3 variants are a C3 with `self.m` replaced; e = 1.0 and k = ((1, 1), (3, 3)) go to the bottleneck BY KEYWORD;
  * C3_CBAM (kernel_size 7) and C3_CBAMS (3) hold CBAMBottleneck: ratio 8, attention between cv1 (1x1) and cv2;
  * CBAMBottleneckDWC(c1, c2, shortcut, g, e, k, ratio=16, kernel_size=7) - e BEFORE k -: x2 = cv2(cv1(x)); t1 = ca(x2) * x2; out = sa(t1) * t1
    (+ x), sa the depthwise-separable gate: stats = [mean_c, max_c]; u = depthwise k x k conv (2 channels, bias); v = relu(BN(u)); p = 1x1
    conv 2 -> 1 (bias); q = relu(BN1(p)); sa = sigmoid(q) - the ReLU comes BEFORE the sigmoid, so sa lies in [0.5, 1); k is 3 or 7;
  * SCBAMBottleneck(c1, c2, shortcut, g, e, ratio=16, kernel_size=7): cv1 1x1, cv2 3x3; yc = ca(x2) * x2; ys = sa(yc) * x2 - the gate is computed
    from yc but multiplies x2 -; out = sigmoid(yc + ys) (+ x);
  * C3CBAM(c1, c2): a bare CBAM on its input, ratio 16, 7x7 gate; c2 is ignored.
tests/golden/block_c3_cbam.npz ... block_scbam_bneck_nosc.npz, generated from the reference's own classes, pin all of that.

register(monkeypatch) puts the six rows into the oracle's parse_model tables for the length of a test (the five C3 variants repeated inside, as
in the reference, models/yolo.py:1473-1477 and 1487-1490); oracle_model builds the oracle Model of a yolov5_cbam_cfg.

THE SEED RULE.  Three discontinuities can make two correct fp32 implementations disagree: the global max-pool's winner per (image, channel),
the channel arg-max per pixel in the spatial gate, and the two ReLUs of the depthwise-separable gate.  For each seeded case the FIRST candidate
is taken at which (1) the fp64 restatement's smallest top-two gap over every pooled maximum is >= MIN_GAP (cpca_ref.MIN_GAP = 4e-4, that
file's derivation), (2) its smallest top-two gap over every per-pixel channel maximum is >= MIN_GAP, (3) its smallest |pre-ReLU| value in any
depthwise-separable gate is >= MIN_GAP and (4) the fp32 restatement's worst gradient against fp64 is below half the bar its test applies.
Block candidates are the input seeds 0..7, graph candidates (fill 1..4) x (batch 0..3) in that order, as in cpca_ref, then further fills in
the same order (graph_candidates); `choose` below is the rule.  `python tools/gen_cbam_c3_golden.py --seeds` prints the tables."""
import copy
import sys

import torch
import torch.nn as nn

from cpca_ref import MIN_GAP, grad_bars
from oracle.somi_ref import blocks as OB

ChannelAttentionModule = OB.ChannelAttentionModule
SpatialAttentionModule = OB.SpatialAttentionModule
CBAMBottleneck = OB.CBAMBottleneck


class DepthWiseConv(nn.Module):
    def __init__(self, in_channel, out_channel, kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.depth_conv = nn.Conv2d(in_channel, in_channel, kernel_size, stride, padding, groups=in_channel)
        self.bn = nn.BatchNorm2d(in_channel)
        self.point_conv = nn.Conv2d(in_channel, out_channel, 1, 1, 0)
        self.relu = nn.ReLU()
        self.bn1 = nn.BatchNorm2d(out_channel)

    def forward(self, x):
        return self.relu(self.bn1(self.point_conv(self.relu(self.bn(self.depth_conv(x))))))


class SpatialAttentionModuleDWC(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        assert kernel_size in (3, 7), 'kernel size must be 3 or 7'
        self.cv1 = DepthWiseConv(2, 1, kernel_size, padding=3 if kernel_size == 7 else 1)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return torch.sigmoid(self.cv1(torch.cat([x.mean(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)], dim=1)))


class CBAMBottleneckDWC(nn.Module):
    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, k=(3, 3), ratio=16, kernel_size=7):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, k[0], 1)
        self.cv2 = OB.Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2
        self.channel_attention = ChannelAttentionModule(c2, ratio)
        self.spatial_attention = SpatialAttentionModuleDWC(kernel_size)

    def forward(self, x):
        x2 = self.cv2(self.cv1(x))
        out = self.channel_attention(x2) * x2
        out = self.spatial_attention(out) * out
        return x + out if self.add else out


class SCBAMBottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, ratio=16, kernel_size=7):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.cv2 = OB.Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2
        self.channel_attention = ChannelAttentionModule(c2, ratio)
        self.spatial_attention = SpatialAttentionModule(kernel_size)
        self.sigmoid = nn.Sigmoid()

    def gated(self, x2, yc):
        return self.spatial_attention(yc) * x2                    # the gate is computed from yc but multiplies x2

    def forward(self, x):
        x2 = self.cv2(self.cv1(x))
        yc = self.channel_attention(x2) * x2
        out = self.sigmoid(yc + self.gated(x2, yc))
        return x + out if self.add else out


class C3CBAM(nn.Module):
    def __init__(self, c1, c2):
        super().__init__()
        self.kernel_size = 7
        self.channel_attention = ChannelAttentionModule(c1)
        self.spatial_attention = SpatialAttentionModule(self.kernel_size)

    def forward(self, x):
        out = self.channel_attention(x) * x
        return self.spatial_attention(out) * out


def _c3(bottleneck, default_kernel=None):
    class _C3(OB.C3):
        def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, **kw):
            super().__init__(c1, c2, n, shortcut, g, e)
            c_ = int(c2 * e)
            if default_kernel is not None:
                kw = dict(kernel_size=kw.pop('kernel_size', default_kernel), k=((1, 1), (3, 3)), **kw)
            self.m = nn.Sequential(*(bottleneck(c_, c_, shortcut, g, e=1.0, **kw) for _ in range(n)))
    return _C3


class C3_CBAM(_c3(CBAMBottleneck, 7)):
    pass


class C3_CBAMS(_c3(CBAMBottleneck, 3)):
    pass


class C3_CBAM_DWC(_c3(CBAMBottleneckDWC, 7)):
    pass


class C3_CBAMS_DWC(_c3(CBAMBottleneckDWC, 3)):
    pass


class C3_SCBAM(_c3(SCBAMBottleneck)):
    pass


# ---------------------------------------------------------------------------------------------- WRONG restatements the host tests rule out
class ProductSCBAMBottleneck(SCBAMBottleneck):
    """(a) SCBAM with ys = sa(yc) * yc: the plain CBAM product inside the sigmoid."""

    def gated(self, x2, yc):
        return self.spatial_attention(yc) * yc


class NoFinalReluDWC(DepthWiseConv):
    """(b) the depthwise-separable gate without its final ReLU (the gate then reaches below 0.5)."""

    def forward(self, x):
        return self.bn1(self.point_conv(self.relu(self.bn(self.depth_conv(x)))))


class ReluBeforeBn1DWC(DepthWiseConv):
    """(b') the gate with BN1 after the ReLU."""

    def forward(self, x):
        return self.bn1(self.relu(self.point_conv(self.relu(self.bn(self.depth_conv(x))))))


def wrong_dwc_bottleneck(gate_cls):
    """CBAMBottleneckDWC(64, 64, False, ...) whose gate is one of the two wrong forms (same parameter names: fill_state gives the same weights)."""
    blk = CBAMBottleneckDWC(64, 64, False, 1, 1.0, ((1, 1), (3, 3)))
    blk.spatial_attention.cv1 = gate_cls(2, 1, 7, padding=3)
    return blk


ROWS = dict(C3_CBAM=C3_CBAM, C3_CBAMS=C3_CBAMS, C3_CBAM_DWC=C3_CBAM_DWC, C3_CBAMS_DWC=C3_CBAMS_DWC, C3_SCBAM=C3_SCBAM, C3CBAM=C3CBAM)
REPEATED_INSIDE = ('C3_CBAM', 'C3_CBAMS', 'C3_CBAM_DWC', 'C3_CBAMS_DWC', 'C3_SCBAM')
VARIANTS = ('cbam', 'cbams', 'cbam_dwc', 'cbams_dwc', 'scbam', 'row')


def register(monkeypatch):
    """The rows in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, **ROWS))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | set(REPEATED_INSIDE))


def oracle_model(cfg):
    """The oracle Model of a yolov5_cbam_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


# ---------------------------------------------------------------------------------------------- the seeds (the rule: this module's docstring)
BLOCK_SHAPE = (2, 64, 5, 7)
BLOCK_SHAPES = {'c3_cbams_dwc_wide': (1, 32, 23, 26)}      # the 3x3 stencil with interior pixels, H != W
BLOCKS = {                                        # tag -> constructor over a namespace; candidates are the input seeds 0..7 of parity.check_block
    'c3_cbam': lambda ns: ns.C3_CBAM(64, 64, 2),
    'c3_cbams': lambda ns: ns.C3_CBAMS(64, 64, 2),
    'c3_scbam': lambda ns: ns.C3_SCBAM(64, 64, 2),
    'c3cbam': lambda ns: ns.C3CBAM(64, 64),
    'scbam_bneck_sc': lambda ns: ns.SCBAMBottleneck(64, 64, True, 1, 1.0),
    'scbam_bneck_nosc': lambda ns: ns.SCBAMBottleneck(64, 64, False, 1, 1.0),
    'c3_cbam_64_32': lambda ns: ns.C3_CBAM(64, 32, 1, False),
    'c3_cbam_dwc': lambda ns: ns.C3_CBAM_DWC(64, 64, 2),
    'c3_cbams_dwc': lambda ns: ns.C3_CBAMS_DWC(64, 64, 2),
    'cbam_dwc_bneck_sc': lambda ns: ns.CBAMBottleneckDWC(64, 64, True, 1, 1.0, ((1, 1), (3, 3))),
    'cbam_dwc_bneck_nosc': lambda ns: ns.CBAMBottleneckDWC(64, 64, False, 1, 1.0, ((1, 1), (3, 3))),
}
# `python tools/gen_cbam_c3_golden.py --seeds`; (pooled gap, channel gap, fp32 against fp64 x the bar) of the rows that decide:
#   c3_cbam 0: 9.5e-04, 1.1e-03, 0.020     c3_cbams 0: 9.5e-04, 2.9e-03, 0.013     c3_cbam_64_32 0: 2.8e-03, 2.6e-02, 0.002
#   c3_scbam 0: 2.0e-04 (misses), 7.3e-04, 0.005;  1: 2.5e-03, 3.1e-03, 0.002
#   c3cbam   0: 9.3e-04, 2.9e-04 (misses), 0.000;  1: 7.8e-03, 5.7e-03, 0.000
#   scbam_bneck_sc / _nosc 0: 1.6e-03, 7.0e-03, 0.001
#   (with the pre-ReLU margin third:)  c3_cbam_dwc 0: 2.7e-03, 1.6e-03, 2.0e-03, 0.179     c3_cbams_dwc 0: 7.2e-03, 2.3e-03, 4.7e-04, 0.298
#   cbam_dwc_bneck_sc / _nosc 0: pre-ReLU 3.2e-04 (misses);  1: 1.9e-03, 4.6e-03, 5.9e-03, 0.477
BLOCK_SEEDS = {'c3_cbam': 0, 'c3_cbams': 0, 'c3_scbam': 1, 'c3cbam': 1, 'scbam_bneck_sc': 0, 'scbam_bneck_nosc': 0, 'c3_cbam_64_32': 0,
               'c3_cbam_dwc': 0, 'c3_cbams_dwc': 0, 'cbam_dwc_bneck_sc': 1, 'cbam_dwc_bneck_nosc': 1}
# a fixture without a seeded GPU case: C3_CBAMS_DWC(32, 32, 2) on (1, 32, 23, 26) - none of its input seeds 0..7 passes the rule
FIXTURE_ONLY = {'c3_cbams_dwc_wide': lambda ns: ns.C3_CBAMS_DWC(32, 32, 2)}
# variant -> (fill_state seed, synthetic_batch seed); candidates (1..4) x (0..3) in that order
#   cbam  (1, 0): 4.8e-04, 7.8e-04, 0.063        cbams (1, 0): 4.8e-04, 7.8e-04, 0.164
#   row   (2, 2): 1.6e-03, 1.4e-02, 0.114; the six before it have pooled gaps of 1.4e-05 .. 2.1e-04 (1024-channel maxima over a 2x2 map)
#   scbam: none of the sixteen passes - seven bottlenecks take a channel maximum at every pixel of maps down to 2x2 and a pooled maximum of
#       every channel, and the smaller of the two gaps is 1.0e-06 .. 3.1e-04 (fp32 against fp64 0.035 .. 0.147 throughout).  The candidate
#       list therefore goes on in the same order, fill 5, 6, ... with batch 0..3 each (GRAPH_FILLS bounds it), and the rule stays what it is:
#       (5, 0): 1.2e-03, 2.4e-04 (misses);  (5, 1): 4.7e-04, 4.0e-04 (4.001e-04), 0.090 - the first of all candidates that passes
GRAPH_FILLS = range(1, 9)
#   cbam_dwc  (4, 2): 5.4e-04, 1.8e-03, pre-ReLU 4.2e-04, 0.278 - the fourteen before it miss a margin (smallest 1.3e-05 .. 3.8e-04), (1, 2) also the bar
#   cbams_dwc (1, 0): channel gap 2.4e-04 (misses);  (1, 1): 1.8e-03, 5.9e-04, 6.8e-04, 0.063
GRAPH_SEEDS = {'cbam': (1, 0), 'cbams': (1, 0), 'cbam_dwc': (4, 2), 'cbams_dwc': (1, 1), 'scbam': (5, 1), 'row': (2, 2)}


def graph_candidates():
    """(fill_state seed, synthetic_batch seed) in the order the rule tries them: cpca_ref's sixteen, then further fills in the same order."""
    return [(fill, batch) for fill in GRAPH_FILLS for batch in range(4)]


def choose(figures):
    """The rule on a list of candidates' figures, in candidate order -> the index of the first that passes."""
    return next(i for i, fig in enumerate(figures) if passes(fig))


def block_shape(tag):
    return BLOCK_SHAPES.get(tag, BLOCK_SHAPE)


class gaps:
    """Context manager over the forwards run inside: .pooled, the smallest gap between the largest and second-largest value of any (image,
    channel) plane a ChannelAttentionModule pools; .channel, the same over the channels of every pixel a spatial gate reads; .relu, the
    smallest |value| entering a ReLU of a depthwise-separable gate (inf where the model has none)."""

    def __init__(self, model):
        self.model, self.hooks = model, []
        self.pooled = self.channel = self.relu = float('inf')

    def _relu(self, mod, inp):
        self.relu = min(self.relu, inp[0].detach().abs().min().item())

    def _pooled(self, mod, inp):
        top = inp[0].detach().flatten(2).topk(2, dim=2)[0]
        self.pooled = min(self.pooled, (top[..., 0] - top[..., 1]).min().item())

    def _channel(self, mod, inp):
        top = inp[0].detach().topk(2, dim=1)[0]
        self.channel = min(self.channel, (top[:, 0] - top[:, 1]).min().item())

    def __enter__(self):
        for m in self.model.modules():
            if isinstance(m, ChannelAttentionModule):
                self.hooks.append(m.register_forward_pre_hook(self._pooled))
            elif isinstance(m, (SpatialAttentionModule, SpatialAttentionModuleDWC)):
                self.hooks.append(m.register_forward_pre_hook(self._channel))
            elif isinstance(m, DepthWiseConv):
                self.hooks.append(m.relu.register_forward_pre_hook(self._relu))
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()
        return False


def passes(figures):
    """The rule on (pooled gap, channel gap, pre-ReLU margin, fp32 against fp64 in units of the bar)."""
    pooled, channel, relu, bars = figures
    return min(pooled, channel, relu) >= MIN_GAP and bars < 0.5


def block_case(tag, seed=None, make=None):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    ref = (make or BLOCKS[tag])(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*block_shape(tag), generator=gen), gen


def block_figures(tag, seed=None):
    """-> (pooled gap, channel gap of the fp64 restatement, fp32 against fp64 in units of parity.check_block's bars: 1e-3 * scale
    + 2e-5 per parameter gradient, 1e-3 * scale for dx)."""
    ref, x, gen = block_case(tag, seed)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    with gaps(ref64) as g:
        y64 = ref64(x64)
    y = ref(x32)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    y64.backward(dy.double())
    return g.pooled, g.channel, g.relu, grad_bars(ref, ref64, 1e-3, 2e-5, [(x32.grad, x64.grad)])


def graph_case(variant, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_cbam_cfg at width 0.25, nc 10, batch 2, 64x64."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_cbam_cfg
    fill, batch = GRAPH_SEEDS[variant] if seeds is None else seeds
    cfg = yolov5_cbam_cfg(0.25, 0.33, nc=10, variant=variant)
    ref = fill_state(oracle_model(cfg), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=10, seed=batch)
    return cfg, ref, imgs, targets


def graph_figures(variant, seeds=None):
    """-> (pooled gap, channel gap of the fp64 oracle model, fp32 against fp64 in units of parity.check_train_step's bar
    2e-3 * scale + 2e-6)."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    _, ref, imgs, targets = graph_case(variant, seeds)
    ref64 = copy.deepcopy(ref).double()
    ref.train(), ref64.train()
    with gaps(ref64) as g:
        out64 = ref64(imgs.double() / 255)
    OLoss(ref64)(out64, targets.double())[0].backward()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    return g.pooled, g.channel, g.relu, grad_bars(ref, ref64, 2e-3, 2e-6)
