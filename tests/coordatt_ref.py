"""Plain-PyTorch restatement of the reference's coordinate attention, the CPU oracle of tests/test_coordatt_host.py and
tests/test_coordatt_gpu.py: CoorAttention (models/common.py:1399-1450), CABottleneck (:4884-4922) and C3_CA (:4925-4931), written from their
semantics:

  * the attended map is averaged over its width and over its height; the two (B, C, H) and (B, C, W) results are laid end to end along one axis
    and go through ONE 1x1 conv (with bias) to mip = max(8, c1 // 32) channels, a BatchNorm and h-swish (u * relu6(u + 3) / 6);
  * the H-part and the W-part each get their own 1x1 conv (with bias) back to C channels and a sigmoid;
  * every pixel is multiplied by the gate of its column and by the gate of its row;
  * CABottleneck attends the output of its 1x1 -> 3x3 conv pair and adds the input when shortcut and c1 == c2; C3_CA is a C3 with such
    bottlenecks (e = 1.0).  tests/golden/block_coordatt.npz, block_cabottleneck_*.npz and block_c3_ca.npz, generated from the reference's
    own classes, pin all of that.

register(monkeypatch) puts C3_CA and CoorAttention into the oracle's parser tables for the length of a test - C3_CA NOT among the modules
repeated inside, as in the reference (models/yolo.py:1487-1490)."""
import copy
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


class _Gated(nn.Module):
    def _make_gates(self, c1, c2, mip):
        self.conv1 = nn.Conv2d(c1, mip, 1)
        self.bn1 = nn.BatchNorm2d(mip)
        self.conv_h = nn.Conv2d(mip, c2, 1)
        self.conv_w = nn.Conv2d(mip, c2, 1)

    def attend(self, t):
        H = t.shape[2]
        u = self.bn1(self.conv1(torch.cat([t.mean(3), t.mean(2)], 2).unsqueeze(3)))       # (B, mip, H + W, 1)
        u = u * F.relu6(u + 3) / 6
        a_h = torch.sigmoid(self.conv_h(u[:, :, :H]))                                      # (B, C, H, 1)
        a_w = torch.sigmoid(self.conv_w(u[:, :, H:])).transpose(2, 3)                      # (B, C, 1, W)
        return t * a_w * a_h


class CoorAttention(_Gated):
    def __init__(self, inp, oup, reduction=32):
        super().__init__()
        self._make_gates(inp, oup, max(8, inp // reduction))

    def forward(self, x):
        return self.attend(x)


class CABottleneck(_Gated):
    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, ratio=32):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.cv2 = OB.Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2
        self._make_gates(c1, c2, max(8, c1 // ratio))

    def forward(self, x):
        y = self.attend(self.cv2(self.cv1(x)))
        return x + y if self.add else y


class C3_CA(OB.C3):
    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(CABottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))


def repeat_c3_ca(ns, c, n):
    """What the parsers make of a [-1, n, 'C3_CA', [c]] row: n whole blocks (nn.Sequential in the reference and the oracle, Repeat on the path)."""
    blocks = [ns.C3_CA(c, c) for _ in range(n)]
    return ns.Repeat(*blocks) if hasattr(ns, 'Repeat') else nn.Sequential(*blocks)


def register(monkeypatch):
    """C3_CA and CoorAttention in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, C3_CA=C3_CA, CoorAttention=CoorAttention))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) - {'C3_CA', 'CoorAttention'})


# ---------------------------------------------------------------------------------------------- the kink and the seeds
# h-swish has kinks at u = -3 and u = +3 (relu6(u + 3) switches on and saturates there).  An input of it - an output of bn1 - that lies closer
# to a kink than the distance between two correct fp32 forwards (1e-4 .. 2e-4 behind batch-statistics BatchNorms) can fall on either side, and one
# flipped element moves its layer's gradients by far more than any bar.  So every seeded case below is chosen from the reference alone: among the
# candidates, the one whose fp64 oracle keeps every bn1 output farthest from +-3 (kink_margin), and tests/test_coordatt_host.py asserts that the
# fp32 CPU oracle meets the gradient bar against fp64 there.  tools/gen_coordatt_golden.py --seeds prints the table these were read from.
BLOCK_SHAPE = (2, 64, 5, 7)       # the fixtures' shape
BLOCKS = {                         # tag -> (constructor over a namespace, candidates are the input seeds 0..7 of parity.check_block)
    'coordatt': lambda ns: ns.CoorAttention(64, 64),
    'cabottleneck_sc': lambda ns: ns.CABottleneck(64, 64, True, 1, 1.0),
    'cabottleneck_nosc': lambda ns: ns.CABottleneck(64, 64, False, 1, 1.0),
    'c3_ca': lambda ns: ns.C3_CA(64, 64, 1),
    'c3_ca_x2': lambda ns: repeat_c3_ca(ns, 64, 2),
}
# kink margins of the candidates (fp64 oracle): coordatt 4.4e-3 .. 2.5e-1 (seed 2); cabottleneck, both forms, 6.0e-3 .. 1.9e-1 (seed 2);
# c3_ca 7.0e-3 .. 1.5e-1 (seed 3); two C3_CA in a row 3.5e-3 .. 1.0e-1 (seed 2)
BLOCK_SEEDS = {'coordatt': 2, 'cabottleneck_sc': 2, 'cabottleneck_nosc': 2, 'c3_ca': 3, 'c3_ca_x2': 2}
# where -> (fill_state seed, synthetic_batch seed); candidates (1..4) x (0..3).  'c3' (eight bn1 layers on 16x16 .. 2x2 maps): 3.1e-4 at (3, 0)
# .. 3.8e-2 at (4, 1); 'row' (one bn1 on the 2x2 map): 3.1e-1 .. 1.13 at (3, 3)
GRAPH_SEEDS = {'c3': (4, 1), 'row': (3, 3)}


class kink_margin:
    """Context manager: the smallest distance of any bn1 output of `model` from the kinks at +-3 over the forwards run inside (.value)."""

    def __init__(self, model):
        self.model, self.value, self.hooks = model, float('inf'), []

    def _see(self, mod, inp, out):
        self.value = min(self.value, ((out.detach().abs() - 3).abs().min().item()))

    def __enter__(self):
        self.hooks = [m.register_forward_hook(self._see) for n, m in self.model.named_modules() if n.split('.')[-1] == 'bn1']
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()
        return False


def block_case(tag, seed=None, make=None):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    ref = (make or BLOCKS[tag])(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*BLOCK_SHAPE, generator=gen), gen


def oracle_model(cfg):
    """The oracle Model of a yolov5_ca_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


def graph_case(where, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_ca_cfg at width 0.25, nc 10, batch 2, 64x64."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_ca_cfg
    fill, batch = GRAPH_SEEDS[where] if seeds is None else seeds
    cfg = yolov5_ca_cfg(0.25, 0.33, nc=10, where=where)
    ref = fill_state(oracle_model(cfg), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=10, seed=batch)
    return cfg, ref, imgs, targets
