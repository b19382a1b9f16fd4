#!/usr/bin/env python3
"""Writes tests/golden/block_coordatt.npz, block_cabottleneck_sc.npz, block_cabottleneck_nosc.npz and block_c3_ca.npz: the reference's own
CoorAttention(64, 64) (models/common.py:1399-1450), CABottleneck(64, 64, shortcut, 1, 1.0) with and without the shortcut (:4884-4922) and
C3_CA(64, 64, 1) (:4925-4931) in eval and train mode on one input (batch 2, 64 channels, 5x7) - importing oracle.gen_golden installs the stub
harness that makes the reference importable.  The fixtures hold data only: the input and the two outputs (weights are regenerated from parameter
names by fill_state).  tests/test_coordatt_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_coordatt_golden.py

With --seeds it writes nothing and prints the tables tests/coordatt_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the
smallest distance of any bn1 output of the fp64 oracle from h-swish's kinks at +-3, and the fp32 oracle's worst parameter gradient against
fp64 in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5, parity.grads_close; graphs: 2e-3 * scale + 2e-6,
parity.check_train_step).  That mode needs the oracle and the test restatement only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(131)
    x = (torch.randn(2, 64, 5, 7, generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses to a fraction of its size
    cases = {'block_coordatt': lambda: RC.CoorAttention(64, 64),
             'block_cabottleneck_sc': lambda: RC.CABottleneck(64, 64, True, 1, 1.0),
             'block_cabottleneck_nosc': lambda: RC.CABottleneck(64, 64, False, 1, 1.0),
             'block_c3_ca': lambda: RC.C3_CA(64, 64, 1)}
    for name, make in cases.items():
        mod = G.fill_state(make(), 0)
        RY.initialize_weights(mod)
        rec = dict(x=x)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(x.clone())
        G.save(name, **rec)


class _Patch:
    """The two-call subset of pytest's monkeypatch coordatt_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def _bars(ref, ref64, rel, atol):
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    return worst


def seed_tables():
    import copy
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import coordatt_ref as R
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(_Patch())
    for tag in R.BLOCKS:
        for seed in range(8):
            ref, x, gen = R.block_case(tag, seed)
            ref64 = copy.deepcopy(ref).double().train()
            ref.train()
            with R.kink_margin(ref64) as km:
                y64 = ref64(x.double())
            y = ref(x)
            dy = torch.randn(y.shape, generator=gen)
            y.backward(dy)
            y64.backward(dy.double())
            print(f'block {tag:18s} seed {seed}: kink margin {km.value:.3e}, fp32 against fp64 {_bars(ref, ref64, 1e-3, 2e-5):.3f} x the bar')
    for where in ('c3', 'row'):
        for fill in range(1, 5):
            for batch in range(4):
                _, ref, imgs, targets = R.graph_case(where, (fill, batch))
                ref64 = copy.deepcopy(ref).double().train()
                ref.train()
                with R.kink_margin(ref64) as km:
                    out64 = ref64(imgs.double() / 255)
                OLoss(ref64)(out64, targets.double())[0].backward()
                OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
                print(f'graph {where:3s} seeds ({fill}, {batch}): kink margin {km.value:.3e}, fp32 against fp64 {_bars(ref, ref64, 2e-3, 2e-6):.3f} x the bar')


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
