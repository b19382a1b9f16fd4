#!/usr/bin/env python3
"""Writes tests/golden/block_cnxblock.npz, block_cnxcneb.npz, block_cnxcneb_16_48.npz, block_cnxconvmix.npz, block_cnxconvmix_k7.npz and
block_cnxcspcm.npz: the reference's own ConvNextBlock(16), CNeB(32, 32, 2), CNeB(16, 48, 1) (models/common.py:6751-6791), ConvMix(16, 16),
ConvMix(12, 12, 7) and CSPCM(32, 32, 1) (:7149-7180) in eval and train mode on one input each - batch 2, 5x7, a map smaller than either
kernel; and block_cnxblock_flat.npz, ConvNextBlock(16) in eval mode on a zero input, the case that tells LayerNorm's eps 1e-6 from 1e-5.
Importing oracle.gen_golden installs the stub harness that makes the reference importable.  The fixtures hold data only: the input and the
outputs (weights are regenerated from parameter names by fill_state).  tests/test_convnext_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_convnext_golden.py

With --seeds it writes nothing and prints the tables tests/convnext_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the
fp32 restatement's worst gradient against fp64 in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5 per parameter and
1e-3 * scale for dx, parity.check_block; the graphs: 2e-3 * scale + 2e-6, parity.check_train_step).  That mode needs the oracle and the test
restatement only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import convnext_ref as R
    g = torch.Generator().manual_seed(163)
    for name, tag in R.FIXTURES.items():
        inp = (torch.randn(*R.block_shape(tag), generator=g) * 2).round() / 2      # a grid of 1/2: the file compresses to a fraction of its size
        mod = G.fill_state(R.BLOCKS[tag](G.RC), 0)                # the constructor over the reference's own namespace
        G.RY.initialize_weights(mod)
        rec = dict(x=inp)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(inp.clone())
        G.save(name, **rec)
    # the one case where LayerNorm's eps shows: on a zero input the 7x7 conv returns its bias at every pixel, whose variance over the channels
    # is of order 1e-2, and the block's output is the branch alone
    mod = G.fill_state(G.RC.ConvNextBlock(16), 0).eval()
    inp = torch.zeros(*R.block_shape('cnxblock'))
    with torch.no_grad():
        G.save(R.FLAT_FIXTURE, x=inp, out_eval=mod(inp.clone()))


class _Patch:
    """The one-call subset of pytest's monkeypatch convnext_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def seed_tables():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import convnext_ref as R
    R.register(_Patch())
    for tag in R.BLOCKS:
        for seed in range(8):
            print(f'block {tag:12s} seed {seed}: fp32 against fp64 {R.block_figures(tag, seed):.3f} x the bar', flush=True)
    for where in R.GRAPH_SEEDS:
        for fill in range(1, 5):
            for batch in range(4):
                print(f'graph {where} seeds ({fill}, {batch}): fp32 against fp64 {R.graph_figures(where, (fill, batch)):.3f} x the bar', flush=True)


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
