"""Plain-PyTorch restatement of the reference's large-kernel depthwise blocks, the CPU oracle of tests/test_convnext_host.py and
tests/test_convnext_gpu.py: LayerNorm_s, ConvNextBlock and CNeB (models/common.py:6728-6791), ConvMix and CSPCM (:7149-7180), written from
their semantics:

  * LayerNorm_s(c, eps=1e-6): layer norm over the channels of a channels-last map, with weight and bias;
  * ConvNextBlock(dim): depthwise 7x7 conv with bias (pad 3) -> LayerNorm over C (eps 1e-6) -> Linear(dim, 4 dim) -> exact GELU ->
    Linear(4 dim, dim) -> times the per-channel parameter gamma (1e-6 at construction; None when layer_scale_init_value <= 0) -> plus the
    block's input.  gamma scales the BRANCH, not the sum.  Parameter order: gamma first (a parameter of the block itself), then the children;
  * CNeB(c1, c2, n): cv3(cat(m(cv1(x)), cv2(x))), the block branch FIRST, m = n ConvNextBlocks of width c_ = int(c2 * e);
  * ConvMix(dim, dim1, k=9): x = x + BN(GELU(dwconv_k(x) + bias)), then BN(GELU(conv1x1(x) + bias)) - each BatchNorm BEHIND its activation;
    dim1 is ignored;
  * CSPCM(c1, c2, n): cv3(cat(m(cv1(x)), cv2(x))), m = n ConvMix(c_, c_), the block branch first as well.
    tests/golden/block_cnx*.npz, generated from the reference's own classes, pin all of that.

register(monkeypatch) puts CNeB (repeated inside, models/yolo.py:1523-1530), ConvMix and CSPCM (not repeated inside, :1531-1535) into the
oracle's parse_model tables for the length of a test.  The fp64 references of the three dwlk kernels live here too."""
import copy
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB

LN_EPS = 1e-6


class LayerNorm_s(nn.Module):
    eps_default = LN_EPS

    def __init__(self, normalized_shape, eps=None, data_format='channels_last'):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = self.eps_default if eps is None else eps
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):                                         # (B, H, W, C)
        return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)


class ConvNextBlock(nn.Module):
    norm_cls = LayerNorm_s

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = self.norm_cls(dim)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim)) if layer_scale_init_value > 0 else None
        self.drop_path = nn.Identity()

    def branch(self, x):
        t = self.dwconv(x).permute(0, 2, 3, 1)
        return self.pwconv2(self.act(self.pwconv1(self.norm(t))))  # channels last

    def forward(self, x):
        t = self.branch(x)
        if self.gamma is not None:
            t = self.gamma * t
        return x + t.permute(0, 3, 1, 2)


class CNeB(nn.Module):
    block = ConvNextBlock

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.cv2 = OB.Conv(c1, c_, 1, 1)
        self.cv3 = OB.Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(self.block(c_) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class ConvMix(nn.Module):
    def __init__(self, dim, dim1, kernel_size=9):
        super().__init__()
        self.Resnet = nn.Sequential(nn.Conv2d(dim, dim, kernel_size, groups=dim, padding=kernel_size // 2), nn.GELU(), nn.BatchNorm2d(dim))
        self.Conv_1x1 = nn.Sequential(nn.Conv2d(dim, dim, 1), nn.GELU(), nn.BatchNorm2d(dim))

    def forward(self, x):
        return self.Conv_1x1(x + self.Resnet(x))


class CSPCM(nn.Module):
    block = ConvMix

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.cv2 = OB.Conv(c1, c_, 1, 1)
        self.cv3 = OB.Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(self.block(c_, c_) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


# ---------------------------------------------------------------------------------------------- WRONG restatements the host tests rule out
class NormThenActConvMix(ConvMix):
    """The usual order: BatchNorm in front of the GELU (same parameters, same state dict)."""

    def forward(self, x):
        r, c = self.Resnet, self.Conv_1x1
        x = x + r[1](r[2](r[0](x)))
        return c[1](c[2](c[0](x)))


class Dim1ConvMix(ConvMix):
    """A ConvMix that honours dim1: the 1x1 conv maps dim -> dim1."""

    def __init__(self, dim, dim1, kernel_size=9):
        super().__init__(dim, dim1, kernel_size)
        self.Conv_1x1 = nn.Sequential(nn.Conv2d(dim, dim1, 1), nn.GELU(), nn.BatchNorm2d(dim1))


class SwappedCNeB(CNeB):
    """cv2's branch first in the concatenation."""

    def forward(self, x):
        return self.cv3(torch.cat((self.cv2(x), self.m(self.cv1(x))), 1))


class SwappedCSPCM(CSPCM):
    """cv2's branch first in the concatenation."""

    def forward(self, x):
        return self.cv3(torch.cat((self.cv2(x), self.m(self.cv1(x))), 1))


class GammaOnSumBlock(ConvNextBlock):
    """gamma applied to input + branch instead of the branch."""

    def forward(self, x):
        return (self.gamma * (x.permute(0, 2, 3, 1) + self.branch(x))).permute(0, 3, 1, 2)


class TorchEpsLayerNorm(LayerNorm_s):
    """nn.LayerNorm's default eps."""
    eps_default = 1e-5


class TorchEpsBlock(ConvNextBlock):
    norm_cls = TorchEpsLayerNorm


def register(monkeypatch):
    """CNeB, ConvMix and CSPCM in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, CNeB=CNeB, ConvMix=ConvMix, CSPCM=CSPCM))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'CNeB'})


# ---------------------------------------------------------------------------------------------- the cases and their seeds
# No block here takes a maximum, so there is no gap rule: a seeded case is the FIRST candidate at which the fp32 restatement's gradients stay
# below half the test's bar against its own fp64 copy.  `python tools/gen_convnext_golden.py --seeds` prints the table.
BLOCK_SHAPE = (2, 32, 5, 7)
BLOCK_SHAPES = {'cnxblock': (2, 16, 5, 7), 'cneb_16_48': (2, 16, 5, 7), 'convmix': (2, 16, 5, 7), 'convmix_k7': (2, 12, 5, 7)}
BLOCKS = {                                        # tag -> constructor over a namespace; candidates are the input seeds 0..7 of parity.check_block
    'cnxblock': lambda ns: ns.ConvNextBlock(16),                  # on 5 x 7, a map smaller than the kernel
    'cneb': lambda ns: ns.CNeB(32, 32, 2),
    'cneb_16_48': lambda ns: ns.CNeB(16, 48, 1),
    'convmix': lambda ns: ns.ConvMix(16, 16),
    'convmix_k7': lambda ns: ns.ConvMix(12, 12, 7),
    'cspcm': lambda ns: ns.CSPCM(32, 32, 1),
}
FIXTURES = {'block_cnxblock': 'cnxblock', 'block_cnxcneb': 'cneb', 'block_cnxcneb_16_48': 'cneb_16_48', 'block_cnxconvmix': 'convmix',
            'block_cnxconvmix_k7': 'convmix_k7', 'block_cnxcspcm': 'cspcm'}
# every candidate of every block is at 0.000 .. 0.167 x the bar (the worst: cspcm, 0.072 .. 0.167)
FLAT_FIXTURE = 'block_cnxblock_flat'              # ConvNextBlock(16), eval, on a zero input: the LayerNorm sees the conv's bias alone
BLOCK_SEEDS = {'cnxblock': 0, 'cneb': 0, 'cneb_16_48': 0, 'convmix': 0, 'convmix_k7': 0, 'cspcm': 0}
# (fill_state seed, synthetic_batch seed); candidates (1..4) x (0..3) in that order
#   cneb  (1, 0): 0.067 x the bar (all sixteen 0.020 .. 0.067);  cspcm (1, 0): 0.460 (all sixteen 0.171 .. 0.460: eight ConvMix blocks whose
#   two BatchNorms sit behind a GELU, on maps down to 2x2 at batch 2)
GRAPH_SEEDS = {'cneb': (1, 0), 'cspcm': (1, 0)}


def block_shape(tag):
    return BLOCK_SHAPES.get(tag, BLOCK_SHAPE)


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
    """-> fp32 against fp64 in units of parity.check_block's bars: 1e-3 * scale + 2e-5 per parameter gradient, 1e-3 * scale for dx."""
    ref, x, gen = block_case(tag, seed)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    y64, y = ref64(x64), ref(x32)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    y64.backward(dy.double())
    return grad_bars(ref, ref64, 1e-3, 2e-5, [(x32.grad, x64.grad)])


def graph_case(where, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_convnext_cfg at width 0.25, nc 4, batch 2, 64x64; the
    caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_convnext_cfg
    fill, batch = GRAPH_SEEDS[where] if seeds is None else seeds
    cfg = yolov5_convnext_cfg(0.25, 0.33, nc=4, where=where)
    ref = fill_state(OModel(copy.deepcopy(cfg)), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=4, seed=batch)
    return cfg, ref, imgs, targets


def graph_figures(where, seeds=None):
    """-> fp32 against fp64 in units of parity.check_train_step's bar 2e-3 * scale + 2e-6."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    _, ref, imgs, targets = graph_case(where, seeds)
    ref64 = copy.deepcopy(ref).double()
    ref.train(), ref64.train()
    OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    return grad_bars(ref, ref64, 2e-3, 2e-6)


# ---------------------------------------------------------------------------------------------- the dwlk kernels (dwlk.hip), NHWC references
KS = (7, 9)
# one quad; three quads in four lanes (no power of two); five in eight; 17 in 32 - more than 64 lanes a pixel row would be 65 quads, the second
# channel chunk: 260 channels
WIDTHS = (4, 12, 20, 68, 260)
STRIP = 8                                                         # ops.dwlk_strip_length(), asserted by the host test
# three images on a map smaller than the kernel; one pixel; ragged; one row of strip + 1 and one of 2 * strip - 1 pixels
SHAPES = [(3, 5, 7), (1, 1, 1), (2, 33, 3), (1, 1, STRIP + 1), (1, 1, 2 * STRIP - 1)]
# per width the smallest number of strips at which a workgroup of the forward / data gradient walks twice (about 2 x 2048 workgroups' worth of
# strips: 256 / nq strips a workgroup row, nq the power of two that covers the quads, 64 at most, two chunks at 260 channels), as (B, H, W)
# with one or two strips a row; and the same for the weight gradient's plan (2 x 512 workgroups' worth).  The last workgroup's second row
# lies past the end.  Narrow widths need many strips, so their rows are short.
WALK_FWD = {4: (1, 1048321, 1), 12: (1, 262081, 3), 20: (1, 131041, 3), 68: (1, 16381, 9), 260: (1, 4095, 9)}
WALK_WGRAD = {4: (1, 130945, 9), 12: (1, 32737, 9), 20: (1, 16369, 9), 68: (1, 4093, 9), 260: (1, 1023, 9)}


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))


def _taps(x, k):
    """(r, q, the slices of the output and of the input that tap (r, q) of a k x k stencil with pad k // 2 joins) for the taps that reach the map."""
    H, W = x.shape[1:3]
    p = k // 2
    for r in range(k):
        for q in range(k):
            dh, dw = r - p, q - p
            if abs(dh) >= H or abs(dw) >= W:
                continue                                          # the tap reads padding only
            oh, ow = slice(max(0, -dh), min(H, H - dh)), slice(max(0, -dw), min(W, W - dw))
            ih, iw = slice(max(0, dh), min(H, H + dh)), slice(max(0, dw), min(W, W + dw))
            yield r, q, (slice(None), oh, ow), (slice(None), ih, iw)


def dwlk_fwd_ref(x, w, bias=None, act='none'):
    """x (B,H,W,C), w (C,1,k,k) -> act(conv + bias), NHWC, in x's dtype: y[h, w] = sum_rq w[r, q] x[h + r - p, w + q - p], zero outside the map,
    as k * k shifted multiply-adds (no im2col: the walking shapes have a million rows)."""
    k = w.shape[-1]
    y = torch.zeros_like(x)
    for r, q, o, i in _taps(x, k):
        y[o] += x[i] * w[:, 0, r, q]
    if bias is not None:
        y += bias
    return gelu64(y) if act == 'gelu' else y


def dwlk_grads_ref(x, w, dy):
    """-> (dx, dw, db) of y = conv(x, w) + b under the output gradient dy, NHWC / (C,1,k,k) / (C), in the inputs' dtype."""
    k = w.shape[-1]
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for r, q, o, i in _taps(x, k):
        dx[i] += dy[o] * w[:, 0, r, q]
        dw[:, 0, r, q] = (dy[o] * x[i]).sum((0, 1, 2))
    return dx, dw, dy.sum((0, 1, 2))


def kernel_case(c, k, shape, seed=0):
    """-> dict of the dense fp32 tensors of one kernel case: x, dy, res, acc (B,H,W,c), w (c,1,k,k), bias, ps, pt, pivot (c)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * c + 10 * k + seed + B * H * W)
    r = lambda *s: torch.randn(*s, generator=g)                   # noqa: E731
    return dict(x=r(B, H, W, c), dy=r(B, H, W, c), res=r(B, H, W, c), acc=r(B, H, W, c), w=r(c, 1, k, k) / k, bias=r(c) * 0.5,
                ps=torch.rand(c, generator=g) + 0.5, pt=r(c) * 0.5, pivot=r(c) * 0.1)
