#!/usr/bin/env python3
"""Writes tests/golden/block_acmix32.npz, block_acmix16to32.npz and block_acmix64_min.npz: the reference's own ACmix (models/common.py:7281-7365)
as ACmix(32, 32) at 2x32x5x7, ACmix(16, 32) at 1x16x9x4 and ACmix(64, 64) at 2x64x4x4 (the smallest map its ReflectionPad2d(3) takes) on one input
- importing oracle.gen_golden installs the stub harness that makes the reference importable.  The fixtures hold data only: the input (a grid of
1/2), the output under fill_state(., 0) and the output with both rates put back to 0.5 (fill_state draws rates of a few hundredths, which nearly
hide the conv half).  Weights are regenerated from parameter names by fill_state.  tests/test_acmix_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_acmix_golden.py

With --seeds it writes nothing and prints the tables tests/acmix_ref.py's BLOCK_SEEDS and GRAPH_SEEDS were read from: per candidate the fp32
restatement's worst parameter gradient against its fp64 twin in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5,
parity.grads_close; graphs: 2e-3 * scale + 2e-6, parity.check_train_step), and its output and input-gradient errors.  That mode needs the
oracle and the test restatement only, not the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURES = {'block_acmix32': ((32, 32), (2, 32, 5, 7)), 'block_acmix16to32': ((16, 32), (1, 16, 9, 4)),
            'block_acmix64_min': ((64, 64), (2, 64, 4, 4))}


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    for name, (args, shape) in FIXTURES.items():
        g = torch.Generator().manual_seed(167)
        x = (torch.randn(*shape, generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses well
        mod = G.fill_state(RC.ACmix(*args), 0)
        RY.initialize_weights(mod)
        mod.eval()
        rec = dict(x=x)
        with torch.no_grad():
            rec['out'] = mod(x.clone())
            mod.rate1.fill_(0.5)
            mod.rate2.fill_(0.5)
            rec['out_half'] = mod(x.clone())
        G.save(name, **rec)


class _Patch:
    """The one-call subset of pytest's monkeypatch acmix_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def seed_tables():
    import copy
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import acmix_ref as R
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(_Patch())
    for tag in R.BLOCKS:
        for rates in R.RATES:
            for seed in range(3):
                ref, x, gen = R.block_case(tag, rates, seed)
                ref64 = copy.deepcopy(ref).double().train()
                ref.train()
                x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
                y, y64 = ref(x32), ref64(x64)
                dy = torch.randn(y.shape, generator=gen)
                y.backward(dy)
                y64.backward(dy.double())
                eo = (y.double() - y64).abs().max().item() / y64.abs().max().item()
                ex = (x32.grad.double() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
                print(f'block {tag:12s} {rates:6s} seed {seed}: out {eo:.1e}, dx {ex:.1e} of max, parameter gradients '
                      f'{R.worst_grad_ratio(ref, ref64, 1e-3, 2e-5):.3f} x the bar')
    for where in ('row', 'p3'):
        for fill in range(1, 4):
            for batch in range(2):
                _, ref, imgs, targets = R.graph_case(where, (fill, batch))
                ref64 = copy.deepcopy(ref).double().train()
                ref.train()
                OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
                OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
                print(f'graph {where:3s} seeds ({fill}, {batch}): fp32 against fp64 {R.worst_grad_ratio(ref, ref64, 2e-3, 2e-6):.3f} x the bar')


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
