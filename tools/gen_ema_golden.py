#!/usr/bin/env python3
"""Writes tests/golden/block_ema32.npz, block_ema16_f4.npz, block_ema_irmb32.npz, block_ema_bottleneck32.npz, block_ema_c2f32.npz and
block_ema_c2f64_n2.npz: the reference's own EMA(32) (models/common.py:5263-5292) at 2x32x5x7, EMA(16, 4) at 1x16x9x4, iRMB_EMA(32) (:5409-5451),
iRMB_EMABottleneck(32, 32, True) (:5454-5470) and C2f_iRMB_EMA(32, 32, 1) (:5473-5497) at 2x32x5x7 and C2f_iRMB_EMA(64, 64, 2, True) at
2x64x6x5, in eval and train mode on one input - importing oracle.gen_golden installs the stub harness that makes the reference importable
(timm is a stub there; the default paths of iRMB_EMA never call it).  The fixtures hold data only: the input and the two outputs (weights are
regenerated from parameter names by fill_state).  tests/test_ema_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_ema_golden.py

With --seeds it writes nothing and prints the tables tests/ema_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the fp32
restatement's worst parameter gradient against its fp64 twin in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5,
parity.grads_close; graphs: 2e-3 * scale + 2e-6, parity.check_train_step), and its output and input-gradient errors.  That mode needs the
oracle and the test restatement only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURES = {'block_ema32': ('ema32', lambda M: M.EMA(32)), 'block_ema16_f4': ('ema16_f4', lambda M: M.EMA(16, 4)),
            'block_ema_irmb32': ('irmb32', lambda M: M.iRMB_EMA(32)),
            'block_ema_bottleneck32': ('bottleneck32', lambda M: M.iRMB_EMABottleneck(32, 32, True)),
            'block_ema_c2f32': ('c2f32', lambda M: M.C2f_iRMB_EMA(32, 32, 1)),
            'block_ema_c2f64_n2': ('c2f64_n2', lambda M: M.C2f_iRMB_EMA(64, 64, 2, True))}
SHAPES = {'ema16_f4': (1, 16, 9, 4), 'c2f64_n2': (2, 64, 6, 5)}


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    for name, (tag, make) in FIXTURES.items():
        g = torch.Generator().manual_seed(151)
        x = (torch.randn(*SHAPES.get(tag, (2, 32, 5, 7)), generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses well
        mod = G.fill_state(make(RC), 0)
        RY.initialize_weights(mod)
        rec = dict(x=x)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(x.clone())
        G.save(name, **rec)


class _Patch:
    """The one-call subset of pytest's monkeypatch ema_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def seed_tables():
    import copy
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import ema_ref as R
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(_Patch())
    for tag in R.BLOCKS:
        for seed in range(6):
            ref, x, gen = R.block_case(tag, seed)
            ref64 = copy.deepcopy(ref).double().train()
            ref.train()
            x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
            y, y64 = ref(x32), ref64(x64)
            dy = torch.randn(y.shape, generator=gen)
            y.backward(dy)
            y64.backward(dy.double())
            eo = (y.double() - y64).abs().max().item() / y64.abs().max().item()
            ex = (x32.grad.double() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
            print(f'block {tag:18s} seed {seed}: out {eo:.1e}, dx {ex:.1e} of max, parameter gradients '
                  f'{R.worst_grad_ratio(ref, ref64, 1e-3, 2e-5):.3f} x the bar')
    for where in ('c2f', 'row'):
        for fill in range(1, 4):
            for batch in range(3):
                _, ref, imgs, targets = R.graph_case(where, (fill, batch))
                ref64 = copy.deepcopy(ref).double().train()
                ref.train()
                OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
                OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
                print(f'graph {where:3s} seeds ({fill}, {batch}): fp32 against fp64 {R.worst_grad_ratio(ref, ref64, 2e-3, 2e-6):.3f} x the bar')


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
