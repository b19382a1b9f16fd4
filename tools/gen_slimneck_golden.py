#!/usr/bin/env python3
"""Writes tests/golden/block_gsconv.npz, block_gsconv_s2.npz, block_gsconv_noact.npz, block_gsbottleneck.npz, block_gsvovgscsp.npz,
block_gscbam.npz and block_gsvovgscspcbam.npz: the reference's own GSConv(32, 32, 1, 1), GSConv(32, 48, 3, 2), GSConv(16, 24, 3, 1, act=False),
GSBottleneck(32, 32), VoVGSCSP(32, 32, 1) (models/common.py:9586-9681), GSCBAMBottleneck(32, 32, e=1.0) (:737-757) and
VoVGSCSPCBAM(32, 64, 2, False) (:2697-2711) in eval and train mode on one input each - batch 2, 5x7, except the stride-2 GSConv at 9x6, where
the stride meets an odd and an even size.  Importing oracle.gen_golden installs the stub harness that makes the reference importable.  The
fixtures hold data only: the input and the two outputs (weights are regenerated from parameter names by fill_state).
tests/test_slimneck_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_slimneck_golden.py

With --seeds it writes nothing and prints the tables tests/slimneck_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the
smallest gap between the largest and second-largest value of any maximum an attention of the fp64 restatement takes, and the fp32
restatement's worst gradient against fp64 in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5 per parameter and 1e-3 * scale
for dx, parity.check_block; the graph: 2e-3 * scale + 2e-6, parity.check_train_step).  That mode needs the oracle and the test restatement
only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURES = {'block_gsconv': 'gsconv', 'block_gsconv_s2': 'gsconv_s2', 'block_gsconv_noact': 'gsconv_noact', 'block_gsbottleneck': 'gsbottleneck',
            'block_gsvovgscsp': 'vovgscsp', 'block_gscbam': 'gscbam', 'block_gsvovgscspcbam': 'vovgscspcbam'}


def write_fixtures():
    from oracle import gen_golden as G
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import slimneck_ref as R
    g = torch.Generator().manual_seed(151)
    for name, tag in FIXTURES.items():
        inp = (torch.randn(*R.block_shape(tag), generator=g) * 2).round() / 2      # a grid of 1/2: the file compresses to a fraction of its size
        mod = G.fill_state(R.BLOCKS[tag](G.RC), 0)                # the constructor over the reference's own namespace
        G.RY.initialize_weights(mod)
        rec = dict(x=inp)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(inp.clone())
        G.save(name, **rec)


class _Patch:
    """The one-call subset of pytest's monkeypatch slimneck_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def seed_tables():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import slimneck_ref as R
    R.register(_Patch())
    for tag in R.BLOCKS:
        for seed in range(8):
            gap, bars = R.block_figures(tag, seed)
            print(f'block {tag:14s} seed {seed}: max gap {gap:.3e}, fp32 against fp64 {bars:.3f} x the bar', flush=True)
    for tag in R.GRAPH_SEEDS:
        for fill in range(1, 5):
            for batch in range(4):
                gap, bars = R.graph_figures(tag, (fill, batch))
                print(f'graph {tag} seeds ({fill}, {batch}): max gap {gap:.3e}, fp32 against fp64 {bars:.3f} x the bar', flush=True)


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
