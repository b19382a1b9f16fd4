#!/usr/bin/env python3
"""Writes tests/golden/block_c3_cbam.npz, block_c3_cbams.npz, block_c3_cbam_dwc.npz, block_c3_cbams_dwc.npz, block_c3_scbam.npz,
block_c3cbam.npz, block_cbam_dwc_bneck_nosc.npz, block_scbam_bneck_nosc.npz and block_c3_cbams_dwc_wide.npz: the reference's own C3_CBAM,
C3_CBAMS, C3_CBAM_DWC, C3_CBAMS_DWC and C3_SCBAM (64, 64, n = 2; models/common.py:1640-1705), C3CBAM(64, 64) (:494-504),
CBAMBottleneckDWC(64, 64, False, 1, 1.0, ((1, 1), (3, 3))) (:953-972) and SCBAMBottleneck(64, 64, False, 1, 1.0) (:975-995) in eval and train
mode on one input - batch 2, 64 channels, 5x7 on a grid of 1/2 -, and C3_CBAMS_DWC(32, 32, 2) on (1, 32, 23, 26), where the 3x3 stencil has
interior pixels and H != W.  Importing oracle.gen_golden installs the stub harness that makes the reference importable.  The fixtures hold data
only: the input and the two outputs (weights are regenerated from parameter names by fill_state).  tests/test_cbam_c3_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_cbam_c3_golden.py

With --seeds it writes nothing and prints the tables tests/cbam_c3_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the three
margins of the seed rule (pooled-maximum gap, per-pixel channel-maximum gap, smallest |pre-ReLU| of a depthwise-separable gate; fp64
restatement) and the fp32 restatement's worst gradient against fp64 in units of the bar its test applies, up to the first candidate that
passes (--all: every candidate).  That mode needs the oracle and the test restatement only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(141)
    x = (torch.randn(2, 64, 5, 7, generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses to a fraction of its size
    xw = (torch.randn(1, 32, 23, 26, generator=g) * 2).round() / 2
    k = ((1, 1), (3, 3))
    cases = {'block_c3_cbam': (lambda: RC.C3_CBAM(64, 64, 2), x),
             'block_c3_cbams': (lambda: RC.C3_CBAMS(64, 64, 2), x),
             'block_c3_cbam_dwc': (lambda: RC.C3_CBAM_DWC(64, 64, 2), x),
             'block_c3_cbams_dwc': (lambda: RC.C3_CBAMS_DWC(64, 64, 2), x),
             'block_c3_scbam': (lambda: RC.C3_SCBAM(64, 64, 2), x),
             'block_c3cbam': (lambda: RC.C3CBAM(64, 64), x),
             'block_cbam_dwc_bneck_nosc': (lambda: RC.CBAMBottleneckDWC(64, 64, False, 1, 1.0, k), x),
             'block_scbam_bneck_nosc': (lambda: RC.SCBAMBottleneck(64, 64, False, 1, 1.0), x),
             'block_c3_cbams_dwc_wide': (lambda: RC.C3_CBAMS_DWC(32, 32, 2), xw)}
    for name, (make, inp) in cases.items():
        mod = G.fill_state(make(), 0)
        RY.initialize_weights(mod)
        rec = dict(x=inp)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(inp.clone())
        G.save(name, **rec)


class _Patch:
    """The one-call subset of pytest's monkeypatch cbam_c3_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def seed_tables():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import cbam_c3_ref as R
    R.register(_Patch())
    fmt = 'pooled gap {:.3e}, channel gap {:.3e}, pre-ReLU {:.3e}, fp32 against fp64 {:.3f} x the bar'
    for tag in R.BLOCKS:
        for seed in range(8):
            fig = R.block_figures(tag, seed)
            print(f'block {tag:18s} seed {seed}: ' + fmt.format(*fig) + ('   <- passes' if R.passes(fig) else ''), flush=True)
            if R.passes(fig) and '--all' not in sys.argv:
                break
    for variant in R.VARIANTS:
        for fill, batch in R.graph_candidates():
            fig = R.graph_figures(variant, (fill, batch))
            print(f'graph {variant:9s} seeds ({fill}, {batch}): ' + fmt.format(*fig) + ('   <- passes' if R.passes(fig) else ''), flush=True)
            if R.passes(fig) and '--all' not in sys.argv:
                break


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
