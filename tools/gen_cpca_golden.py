#!/usr/bin/env python3
"""Writes tests/golden/block_cpca.npz, block_cpca_wide.npz, block_cpcabottleneck_sc.npz, block_cpcabottleneck_nosc.npz and block_c3cpca.npz:
the reference's own CPCA(64) and CPCA(16) (models/common.py:5782-5815), CPCABottleneck(64, 64, shortcut, 1, ((1, 1), (3, 3)), 1.0) with and
without the shortcut (:5818-5859) and C3CPCA(64, 64, 2) (:1684-1689) in eval and train mode on one input each - batch 2, 64 channels, 5x7,
except the `wide` one: batch 1, 16 channels, 23x26, where the 21-tap strips have interior pixels and a swapped axis shows.  Importing
oracle.gen_golden installs the stub harness that makes the reference importable.  The fixtures hold data only: the input and the two outputs
(weights are regenerated from parameter names by fill_state).  tests/test_cpca_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_cpca_golden.py

With --seeds it writes nothing and prints the tables tests/cpca_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the smallest
gap between the largest and second-largest value of any channel maximum the fp64 restatement pools, and the fp32 restatement's worst gradient
against fp64 in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5 per parameter and 1e-3 * scale for dx, parity.check_block;
graphs: 2e-3 * scale + 2e-6, parity.check_train_step).  That mode needs the oracle and the test restatement only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(137)
    x = (torch.randn(2, 64, 5, 7, generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses to a fraction of its size
    xw = (torch.randn(1, 16, 23, 26, generator=g) * 2).round() / 2
    cases = {'block_cpca': (lambda: RC.CPCA(64), x),
             'block_cpca_wide': (lambda: RC.CPCA(16), xw),
             'block_cpcabottleneck_sc': (lambda: RC.CPCABottleneck(64, 64, True, 1, ((1, 1), (3, 3)), 1.0), x),
             'block_cpcabottleneck_nosc': (lambda: RC.CPCABottleneck(64, 64, False, 1, ((1, 1), (3, 3)), 1.0), x),
             'block_c3cpca': (lambda: RC.C3CPCA(64, 64, 2), x)}
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
    """The one-call subset of pytest's monkeypatch cpca_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def seed_tables():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import cpca_ref as R
    R.register(_Patch())
    for tag in R.BLOCKS:
        for seed in range(8):
            gap, bars = R.block_figures(tag, seed)
            print(f'block {tag:20s} seed {seed}: max gap {gap:.3e}, fp32 against fp64 {bars:.3f} x the bar', flush=True)
    for where in ('c3', 'row'):
        for fill in range(1, 5):
            for batch in range(4):
                gap, bars = R.graph_figures(where, (fill, batch))
                print(f'graph {where:3s} seeds ({fill}, {batch}): max gap {gap:.3e}, fp32 against fp64 {bars:.3f} x the bar', flush=True)


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
