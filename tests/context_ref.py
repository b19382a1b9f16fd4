"""Plain-PyTorch restatement of the reference's dilated-convolution context blocks, the CPU oracle of tests/test_dilated_conv_host.py and
tests/test_context_gpu.py: ASPP (models/common.py:1829-1843) and DWR, DWRSeg_Conv, Bottleneck_DWRSeg, C2f_DWR (:7431-7511), written from
their semantics on oracle.somi_ref.blocks.Conv (conv -> BatchNorm -> SiLU, which takes the dilation d and pads d * (k - 1) / 2 for it):

  * ASPP halves the channels with a 1x1 Conv; the result t, its 3x3 stride-1 max-pool and one bare 3x3 convolution of t per entry of k
    (no bias, no norm, no activation; dilation = padding = (k_i - 1) // 2, i.e. 2, 4, 6 for the default (5, 9, 13)) are concatenated in that
    order and go through a 1x1 Conv;
  * DWR takes t = Conv3x3(x) to dim / 2 channels, runs three 3x3 Convs over t - dilation 1 to dim channels, dilations 3 and 5 to dim / 2
    each -, concatenates them in that order, and adds x to a 1x1 Conv of the 2 * dim channels;
  * DWRSeg_Conv is a 1x1 Conv, a DWR (kept under the reference's attribute name `dcnv3`), a BatchNorm and then a GELU;
  * Bottleneck_DWRSeg is a k[0] Conv and a DWRSeg_Conv, plus x when shortcut and c1 == c2;
  * C2f_DWR is C2f with Bottleneck_DWRSeg(c, c, shortcut, g, ((3, 3), (3, 3)), 1.0) blocks: the two halves of cv1's output and every
    block's output, each block reading the piece before it, concatenated into cv2.

tests/golden/block_aspp.npz, block_aspp_k37.npz, block_dwr.npz, block_dwrseg.npz and block_c2f_dwr.npz, generated from the reference's own
classes by tools/gen_context_golden.py, pin all of that.  register(monkeypatch) puts ASPP and C2f_DWR into the oracle's parser tables for
the length of a test, C2f_DWR among the modules repeated inside, as in the reference (models/yolo.py:1487-1490)."""
import copy
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


class ASPP(nn.Module):
    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.m = nn.ModuleList([nn.Conv2d(c_, c_, 3, 1, (v - 1) // 2, (v - 1) // 2, bias=False) for v in k])
        self.cv2 = OB.Conv(c_ * (len(k) + 2), c2, 1, 1)

    def forward(self, x):
        t = self.cv1(x)
        return self.cv2(torch.cat([t, F.max_pool2d(t, 3, 1, 1)] + [m(t) for m in self.m], 1))


class DWR(nn.Module):
    def __init__(self, dim):
        super().__init__()
        h = dim // 2
        self.conv_3x3 = OB.Conv(dim, h, 3)
        self.conv_3x3_d1 = OB.Conv(h, dim, 3, d=1)
        self.conv_3x3_d3 = OB.Conv(h, h, 3, d=3)
        self.conv_3x3_d5 = OB.Conv(h, h, 3, d=5)
        self.conv_1x1 = OB.Conv(2 * dim, dim, 1)

    def forward(self, x):
        t = self.conv_3x3(x)
        return x + self.conv_1x1(torch.cat([self.conv_3x3_d1(t), self.conv_3x3_d3(t), self.conv_3x3_d5(t)], 1))


class DWRSeg_Conv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, groups=1, dilation=1):
        super().__init__()
        self.conv = OB.Conv(in_channels, out_channels, 1)
        self.dcnv3 = DWR(out_channels)
        self.bn = nn.BatchNorm2d(out_channels)
        self.gelu = nn.GELU()

    def forward(self, x):
        return self.gelu(self.bn(self.dcnv3(self.conv(x))))


class Bottleneck_DWRSeg(nn.Module):
    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, k[0], 1)
        self.cv2 = DWRSeg_Conv(c_, c2, k[1], 1, groups=g)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        y = self.cv2(self.cv1(x))
        return x + y if self.add else y


class C2f_DWR(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = OB.Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = OB.Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck_DWRSeg(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    def forward(self, x):
        t = self.cv1(x)
        pieces = [t[:, :self.c], t[:, self.c:]]
        for m in self.m:
            pieces.append(m(pieces[-1]))
        return self.cv2(torch.cat(pieces, 1))


def register(monkeypatch):
    """ASPP and C2f_DWR in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, ASPP=ASPP, C2f_DWR=C2f_DWR))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'C2f_DWR'})


BLOCK_SHAPE = (2, 64, 7, 9)       # the fixtures' shape
BLOCKS = {                         # tag -> constructor over a namespace (this module, or somi_amd.blocks); the fixture is tests/golden/block_<tag>.npz
    'aspp': lambda ns: ns.ASPP(64, 64),
    'aspp_k37': lambda ns: ns.ASPP(64, 32, (3, 7)),
    'dwr': lambda ns: ns.DWR(64),
    'dwrseg': lambda ns: ns.Bottleneck_DWRSeg(64, 64, True, 1, ((3, 3), (3, 3)), 1.0),
    'c2f_dwr': lambda ns: ns.C2f_DWR(64, 128, 2, True),
}
# Nothing in these blocks has a kink but the 3x3 max-pool's choice among near-equal values, which a random input does not produce; the seeds
# are parity.check_block's defaults unless tools/gen_context_golden.py --seeds (the fp32 CPU oracle against its fp64 copy, in units of the
# bars the tests apply) shows a candidate where the ORACLE itself is ill-conditioned.  Its table for the seeds below is in that tool's output.
BLOCK_SEEDS = {tag: len(tag) for tag in BLOCKS}
GRAPH_SEEDS = {'aspp': (1, 0), 'dwr': (1, 0), 'both': (1, 0)}     # where -> (fill_state seed, synthetic_batch seed)


def block_case(tag, seed=None):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    ref = BLOCKS[tag](sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*BLOCK_SHAPE, generator=gen), gen


def oracle_model(cfg):
    """The oracle Model of a yolov5_context_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


def graph_case(where, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_context_cfg at width 0.25, nc 10, batch 2, 64x64."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_context_cfg
    fill, batch = GRAPH_SEEDS[where] if seeds is None else seeds
    cfg = yolov5_context_cfg(0.25, 0.33, nc=10, where=where)
    ref = fill_state(oracle_model(cfg), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=10, seed=batch)
    return cfg, ref, imgs, targets
