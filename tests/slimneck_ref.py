"""Plain-PyTorch restatement of the reference's slim-neck blocks, the CPU oracle of tests/test_slimneck_host.py and tests/test_slimneck_gpu.py:
GSConv, GSBottleneck and VoVGSCSP (models/common.py:9586-9681), GSCBAMBottleneck (:737-757) and VoVGSCSPCBAM (:2697-2711), written from their
semantics:

  * GSConv(c1, c2, k, s, p, g, d, act), c_ = c2 // 2: x1 = cv1(x), a Conv block; x_2 = cv2_2(cv2_1(x1)), TWO stacked depthwise 3x3 Conv
    blocks (each conv -> BatchNorm -> activation), not the paper's one 5x5; the output is the channel DE-interleave of s = cat(x1, x_2): the
    even channels of s, then the odd ones (output o reads s[2 o] for o < c_, s[2 (o - c_) + 1] otherwise) - not channel_shuffle(groups=2),
    which interleaves the two halves.  act=False switches the activation off on all three convs;
  * GSBottleneck: GSConv 1x1 -> GSConv 3x3 without activation, plus a 1x1 Conv without activation of the input, always added;
  * VoVGSCSP: cv3(cat(cv2(x), gsb(cv1(x)))), cv2's branch FIRST; `res`, a 3x3 Conv without activation, is built and never called;
  * GSCBAMBottleneck: GSConv -> x * channel attention -> x * spatial attention -> GSConv 3x3 without activation, + the input when shortcut
    and c1 == c2; VoVGSCSPCBAM is VoVGSCSP with GSCBAMBottleneck(c_, c_, e=1.0) bottlenecks, `res` as unused.
    tests/golden/block_gs*.npz, generated from the reference's own classes, pin all of that.

register(monkeypatch) puts GSConv and VoVGSCSPCBAM (repeated inside, models/yolo.py:1473-1474 and 1489) into the oracle's parse_model tables
for the length of a test."""
import copy
import sys

import torch
import torch.nn as nn

from oracle.somi_ref import blocks as OB


def deinterleave(s):
    """The shuffle that closes every GSConv: even source channels, then odd ones."""
    return torch.cat((s[:, 0::2], s[:, 1::2]), 1)


class GSConv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = OB.Conv(c1, c_, k, s, p, g, d, act)
        self.cv2_1 = OB.Conv(c_, c_, 3, 1, p, c_, d, act)
        self.cv2_2 = OB.Conv(c_, c_, 3, 1, p, c_, d, act)

    def shuffle(self, s):
        return deinterleave(s)

    def forward(self, x):
        x1 = self.cv1(x)
        return self.shuffle(torch.cat((x1, self.cv2_2(self.cv2_1(x1))), 1))


class GSBottleneck(nn.Module):
    def __init__(self, c1, c2, k=3, s=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.conv_lighting = nn.Sequential(GSConv(c1, c_, 1, 1), GSConv(c_, c2, 3, 1, act=False))
        self.shortcut = OB.Conv(c1, c2, 1, 1, act=False)

    def forward(self, x):
        return self.conv_lighting(x) + self.shortcut(x)


class VoVGSCSP(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.cv2 = OB.Conv(c1, c_, 1, 1)
        self.gsb = nn.Sequential(*(self.bottleneck(c_) for _ in range(n)))
        self.res = OB.Conv(c_, c_, 3, 1, act=False)
        self.cv3 = OB.Conv(2 * c_, c2, 1)

    def bottleneck(self, c_):
        return GSBottleneck(c_, c_, e=1.0)

    def forward(self, x):
        return self.cv3(torch.cat((self.cv2(x), self.gsb(self.cv1(x))), 1))


class GSCBAMBottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, k=(1, 3), ratio=8, kernel_size=3):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = GSConv(c1, c_, k[0], 1)
        self.cv2 = GSConv(c_, c2, k[1], 1, act=False)
        self.add = shortcut and c1 == c2
        self.channel_attention = OB.ChannelAttentionModule(c_, ratio)
        self.spatial_attention = OB.SpatialAttentionModule(kernel_size)

    def forward(self, x):
        t = self.cv1(x)
        t = self.channel_attention(t) * t
        t = self.spatial_attention(t) * t
        t = self.cv2(t)
        return x + t if self.add else t


class VoVGSCSPCBAM(VoVGSCSP):
    def bottleneck(self, c_):
        return GSCBAMBottleneck(c_, c_, e=1.0)


# ---------------------------------------------------------------------------------------------- WRONG restatements the host tests rule out
class InterleavingGSConv(GSConv):
    """GSConv closed by channel_shuffle(groups=2): x1[0], x_2[0], x1[1], x_2[1], ..."""

    def shuffle(self, s):
        b, n, h, w = s.shape
        return s.view(b, 2, n // 2, h, w).transpose(1, 2).reshape(b, n, h, w)


class OneFiveGSConv(GSConv):
    """The paper's form: ONE depthwise 5x5 Conv behind cv1."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__(c1, c2, k, s, p, g, d, act)
        del self.cv2_1
        self.cv2_2 = OB.Conv(c2 // 2, c2 // 2, 5, 1, None, c2 // 2, d, act)

    def forward(self, x):
        x1 = self.cv1(x)
        return self.shuffle(torch.cat((x1, self.cv2_2(x1)), 1))


class SwappedVoVGSCSP(VoVGSCSP):
    """C3's order: the bottleneck branch first in the concatenation."""

    def forward(self, x):
        return self.cv3(torch.cat((self.gsb(self.cv1(x)), self.cv2(x)), 1))


class ResVoVGSCSP(VoVGSCSP):
    """A VoVGSCSP that sends the bottleneck branch through `res`."""

    def forward(self, x):
        return self.cv3(torch.cat((self.cv2(x), self.res(self.gsb(self.cv1(x)))), 1))


def register(monkeypatch):
    """GSConv and VoVGSCSPCBAM in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, GSConv=GSConv, VoVGSCSPCBAM=VoVGSCSPCBAM))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'VoVGSCSPCBAM'})


# ---------------------------------------------------------------------------------------------- the cases and their seeds
# The channel attention's global maximum sends its gradient to ONE pixel per (image, channel) and the spatial attention's channel maximum to ONE
# channel per pixel; where the largest and the second-largest value are closer than the distance between two correct fp32 forwards, the two
# sides may pick differently - a discontinuity, not an error.  So every seeded case is chosen from the restatement alone, by the rule
# tests/cpca_ref.py uses: the FIRST candidate whose fp32 restatement stays below half the test's bar against its own fp64 copy and whose
# smallest gap (max_gap, over every maximum either attention of the fp64 restatement takes) is at least MIN_GAP = 4e-4, twice the 2e-4 that
# the training outputs of such graphs were measured apart (cpca_ref.py).  Blocks without attention have no maximum: their gap is infinite.
# `python tools/gen_slimneck_golden.py --seeds` prints the table.
MIN_GAP = 4e-4
BLOCK_SHAPE = (2, 32, 5, 7)
BLOCK_SHAPES = {'gsconv_s2': (2, 32, 9, 6), 'gsconv_noact': (2, 16, 5, 7)}       # stride 2 over an odd and an even size; c_ = 12
BLOCKS = {                                        # tag -> constructor over a namespace; candidates are the input seeds 0..7 of parity.check_block
    'gsconv': lambda ns: ns.GSConv(32, 32, 1, 1),
    'gsconv_s2': lambda ns: ns.GSConv(32, 48, 3, 2),
    'gsconv_noact': lambda ns: ns.GSConv(16, 24, 3, 1, act=False),
    'gsbottleneck': lambda ns: ns.GSBottleneck(32, 32),
    'vovgscsp': lambda ns: ns.VoVGSCSP(32, 32, 1),
    'gscbam': lambda ns: ns.GSCBAMBottleneck(32, 32, e=1.0),
    'vovgscspcbam': lambda ns: ns.VoVGSCSPCBAM(32, 64, 2, False),
}
NO_GRAD = ('res.conv.weight', 'res.bn.weight', 'res.bn.bias')     # of the blocks that have `res`
# every candidate of every block is at 0.001 .. 0.19 x the bar; seed 0 has the gaps   gscbam 4.591e-03   vovgscspcbam 4.456e-03
BLOCK_SEEDS = {'gsconv': 0, 'gsconv_s2': 0, 'gsconv_noact': 0, 'gsbottleneck': 0, 'vovgscsp': 0, 'gscbam': 0, 'vovgscspcbam': 0}
# (fill_state seed, synthetic_batch seed); candidates (1..4) x (0..3) in that order
#   (1, 0): max gap 4.656e-04, fp32 against fp64 0.511 x the bar;  (1, 1): 4.546e-04, 0.223   (eight attentions on maps down to 2x2; of the
#   sixteen candidates nine have a gap below MIN_GAP and three are beyond the bar themselves: 1.176, 2.149, 3.209)
GRAPH_SEEDS = {'slimneck': (1, 1)}


def block_shape(tag):
    return BLOCK_SHAPES.get(tag, BLOCK_SHAPE)


class max_gap:
    """Context manager: the smallest gap between the largest and the second-largest value any attention of `model` takes a maximum over, in the
    forwards run inside (.value): per (image, channel) over the pixels for a channel attention, per pixel over the channels for a spatial one."""

    def __init__(self, model):
        self.model, self.value, self.hooks = model, float('inf'), []

    def _see(self, mod, inp):
        x = inp[0].detach()
        if isinstance(mod, OB.ChannelAttentionModule):
            top = x.flatten(2).topk(2, dim=2)[0] if x.shape[2] * x.shape[3] > 1 else None
        else:
            top = x.topk(2, dim=1)[0].movedim(1, -1)
        if top is not None:
            self.value = min(self.value, (top[..., 0] - top[..., 1]).min().item())

    def __enter__(self):
        kinds = (OB.ChannelAttentionModule, OB.SpatialAttentionModule)
        self.hooks = [m.register_forward_pre_hook(self._see) for m in self.model.modules() if isinstance(m, kinds)]
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()
        return False


def grad_bars(ref, ref64, rel, atol, extra=()):
    """The fp32 restatement's worst gradient error against its fp64 copy in units of rel * scale + atol, over the parameters that have a
    gradient; extra: (fp32, fp64) tensor pairs judged at rel * scale (the input gradient)."""
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        if q.grad is None:
            continue
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    for a, b in extra:
        worst = max(worst, (a.double() - b).abs().max().item() / (rel * (b.abs().max().item() + 1e-12)))
    return worst


def block_case(tag, seed=None, make=None):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    ref = (make or BLOCKS[tag])(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*block_shape(tag), generator=gen), gen


def block_figures(tag, seed=None):
    """-> (max gap of the fp64 restatement, fp32 against fp64 in units of parity.check_block's bars: 1e-3 * scale + 2e-5 per parameter gradient,
    1e-3 * scale for dx)."""
    ref, x, gen = block_case(tag, seed)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    with max_gap(ref64) as mg:
        y64 = ref64(x64)
    y = ref(x32)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    y64.backward(dy.double())
    return mg.value, grad_bars(ref, ref64, 1e-3, 2e-5, [(x32.grad, x64.grad)])


def graph_case(tag='slimneck', seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_slimneck_cfg at width 0.25, nc 4, batch 2, 64x64; the caller
    has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_slimneck_cfg
    fill, batch = GRAPH_SEEDS[tag] if seeds is None else seeds
    cfg = yolov5_slimneck_cfg(0.25, 0.33, nc=4)
    ref = fill_state(OModel(copy.deepcopy(cfg)), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=4, seed=batch)
    return cfg, ref, imgs, targets


def graph_figures(tag='slimneck', seeds=None):
    """-> (max gap of the fp64 oracle model, fp32 against fp64 in units of parity.check_train_step's bar 2e-3 * scale + 2e-6)."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    _, ref, imgs, targets = graph_case(tag, seeds)
    ref64 = copy.deepcopy(ref).double()
    ref.train(), ref64.train()
    with max_gap(ref64) as mg:
        out64 = ref64(imgs.double() / 255)
    OLoss(ref64)(out64, targets.double())[0].backward()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    return mg.value, grad_bars(ref, ref64, 2e-3, 2e-6)
