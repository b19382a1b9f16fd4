"""Plain-PyTorch restatement of the reference's MultiSEAM (models/common.py:8508-8555), the CPU oracle of tests/test_seam_host.py and
tests/test_seam_gpu.py, written from its semantics:

  * three branches, one per patch size p (3 / 5 / 7 by default): a patch-embedding conv (kernel p, stride p, no padding, with bias: the rows and
    columns beyond the last whole patch are not read), SiLU, BatchNorm, then `depth` stages of {z + BatchNorm(SiLU(depthwise 3x3 of z)), 1x1 conv
    with bias, SiLU, BatchNorm} - the activation stands IN FRONT of every BatchNorm;
  * each branch output and x itself are averaged over their pixels, and the four (B, C) vectors are averaged;
  * that vector goes through Linear(C, C / r) -> ReLU -> Linear(C / r, C) -> Sigmoid (no biases), then exp, and scales x per (image, channel);
  * torch's default initialisation (SEAM's xavier initialiser is not called).

SEAM with n stages is the oracle's own class (oracle.somi_ref.blocks.SEAM takes any n).  tests/golden/block_multiseam.npz, block_multiseam_d2.npz
and block_seam_n2.npz, generated from the reference's own classes (tools/gen_seam_golden.py), pin both.

register(monkeypatch) puts MultiSEAM into the oracle's parser tables for the length of a test - NOT among the modules repeated inside, as in the
reference (models/yolo.py:1475, 1487-1490)."""
import copy
import sys

import torch
import torch.nn as nn

from oracle.somi_ref import blocks as OB

SEAM = OB.SEAM
Residual = OB.Residual


def _branch(c, depth, p):
    layers = [nn.Conv2d(c, c, p, p), nn.SiLU(), nn.BatchNorm2d(c)]
    for _ in range(depth):
        layers.append(nn.Sequential(Residual(nn.Sequential(nn.Conv2d(c, c, 3, 1, 1, groups=c), nn.SiLU(), nn.BatchNorm2d(c))),
                                    nn.Conv2d(c, c, 1), nn.SiLU(), nn.BatchNorm2d(c)))
    return nn.Sequential(*layers)


class MultiSEAM(nn.Module):
    def __init__(self, c1, c2, depth, kernel_size=3, patch_size=(3, 5, 7), reduction=16):
        super().__init__()
        assert kernel_size == 3 and len(patch_size) == 3
        c = c1                                                     # c2 follows c1 whatever was asked for
        self.DCovN0, self.DCovN1, self.DCovN2 = (_branch(c, depth, p) for p in patch_size)
        self.fc = nn.Sequential(nn.Linear(c, c // reduction, bias=False), nn.ReLU(inplace=True), nn.Linear(c // reduction, c, bias=False), nn.Sigmoid())

    def forward(self, x):
        pooled = [b(x).mean(dim=(2, 3)) for b in (self.DCovN0, self.DCovN1, self.DCovN2)]
        y = (pooled[0] + pooled[1] + pooled[2] + x.mean(dim=(2, 3))) / 4
        return x * torch.exp(self.fc(y))[:, :, None, None]


def register(monkeypatch):
    """MultiSEAM in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, MultiSEAM=MultiSEAM))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) - {'MultiSEAM'})


# ---------------------------------------------------------------------------------------------- the cases and their seeds
# Every BatchNorm here normalises over few values (the p = 7 branch sees a 2 x 2 map at 15 x 17 and ONE pixel at 7 x 9: two values per channel),
# where 1 / sqrt(var + eps) amplifies the distance between two correct fp32 forwards.  So every seeded case is judged by the reference alone:
# tests/test_seam_host.py asserts that the fp32 CPU oracle meets the test's own gradient bar against its fp64 copy at the seed used, and
# tools/gen_seam_golden.py --seeds prints the table the seeds were read from.
BLOCK_SHAPE = (2, 64, 15, 17)     # the fixtures' shape: the branches see 5x5, 3x3 and 2x2 maps and every patch size leaves a remainder
SMALL_SHAPE = (2, 64, 7, 9)       # one 7x7 patch: Ho = Wo = 1 in the last branch
BLOCKS = {                         # tag -> (constructor over a namespace, shape)
    'multiseam': (lambda ns: ns.MultiSEAM(64, 64, 1), BLOCK_SHAPE),
    'multiseam_d2': (lambda ns: ns.MultiSEAM(64, 64, 2), BLOCK_SHAPE),
    'seam_n2': (lambda ns: ns.SEAM(64, 64, 2), BLOCK_SHAPE),
    'multiseam_small': (lambda ns: ns.MultiSEAM(64, 64, 1), SMALL_SHAPE),
    'seam_n1': (lambda ns: ns.SEAM(64, 64, 1), BLOCK_SHAPE),      # the control: what the path ran before
}
FIXTURES = ('multiseam', 'multiseam_d2', 'seam_n2')
# fp32 CPU oracle against fp64 in units of the block bar (1e-3 * scale + 2e-5), input seeds 0..3 (tools/gen_seam_golden.py --seeds)
# multiseam 0.002 (seed 0) .. 0.004; multiseam_d2 0.005 (0) .. 0.010; seam_n2 0.007 (0) .. 0.011; multiseam_small 0.043 (1) .. 0.215;
# seam_n1 0.005 (1) .. 0.020
BLOCK_SEEDS = {'multiseam': 0, 'multiseam_d2': 0, 'seam_n2': 0, 'multiseam_small': 1, 'seam_n1': 1}
# how -> (fill_state seed, synthetic_batch seed); candidates (1..2) x (0..1), in units of the graph bar (2e-3 * scale + 2e-6):
# 'multi' 0.053 at (1, 0) .. 8.47 at (2, 0); 'seam2' 0.060 at (1, 0) .. 7.13 at (2, 0)
GRAPH_SEEDS = {'multi': (1, 0), 'seam2': (1, 0)}
GRAPH_IMG = 256                    # the smallest size at which the P4 site (16 x 16) still gives the p = 7 branch a 2 x 2 map


def block_case(tag, seed=None):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    make, shape = BLOCKS[tag]
    ref = make(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*shape, generator=gen), gen


def graph_cfg(how):
    from somi_amd.configs import somi_cfg
    return somi_cfg(0.25, 0.33, nc=10, seam='multi') if how == 'multi' else somi_cfg(0.25, 0.33, nc=10, seam='seam', seam_depth=2)


def oracle_model(cfg):
    """The oracle Model of a somi_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


def graph_case(how, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: somi_cfg at width 0.25, nc 10, batch 2, 256 x 256."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    fill, batch = GRAPH_SEEDS[how] if seeds is None else seeds
    cfg = graph_cfg(how)
    ref = fill_state(oracle_model(cfg), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, GRAPH_IMG, nc=10, seed=batch)
    return cfg, ref, imgs, targets
