#!/usr/bin/env python3
"""Writes tests/golden/block_multiseam.npz, block_multiseam_d2.npz and block_seam_n2.npz: the reference's own MultiSEAM(64, 64, 1) and
MultiSEAM(64, 64, 2) (models/common.py:8508-8555) and SEAM(64, 64, 2) (:8448-8505) in eval and train mode on one input (batch 2, 64 channels,
15x17: the three branches see 5x5, 3x3 and 2x2 maps and every patch size leaves a remainder on at least one axis) - importing oracle.gen_golden
installs the stub harness that makes the reference importable.  The fixtures hold data only: the input and the two outputs (weights are
regenerated from parameter names by fill_state).  tests/test_seam_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_seam_golden.py

With --seeds it writes nothing and prints what tests/seam_ref.py's BLOCK_SEEDS and GRAPH_SEEDS are judged by: per candidate the fp32 CPU
oracle's worst parameter gradient against its fp64 copy in units of the bar its test applies (blocks: 1e-3 * scale + 2e-5,
parity.grads_close; graphs: 2e-3 * scale + 2e-6, parity.check_train_step).  That mode needs the oracle and the test restatement only, not the
reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(151)
    x = (torch.randn(2, 64, 15, 17, generator=g) * 2).round() / 2   # a grid of 1/2: the file compresses to a fraction of its size
    cases = {'block_multiseam': lambda: RC.MultiSEAM(64, 64, 1),
             'block_multiseam_d2': lambda: RC.MultiSEAM(64, 64, 2),
             'block_seam_n2': lambda: RC.SEAM(64, 64, 2)}
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
    """The one-call subset of pytest's monkeypatch seam_ref.register needs."""

    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def _bars(ref, ref64, rel, atol):
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        if q.grad is None:                                        # ODConv_3rd's conv.reduction: unused in the reference's forward
            assert p.grad is None
            continue
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    return worst


def seed_tables():
    import copy
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    import seam_ref as R
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(_Patch())
    for tag in R.BLOCKS:
        for seed in sorted({R.BLOCK_SEEDS[tag], 0, 1, 2, 3}):
            ref, x, gen = R.block_case(tag, seed)
            ref64 = copy.deepcopy(ref).double().train()
            ref.train()
            y64, y = ref64(x.double()), ref(x)
            dy = torch.randn(y.shape, generator=gen)
            y.backward(dy)
            y64.backward(dy.double())
            mark = ' <- BLOCK_SEEDS' if seed == R.BLOCK_SEEDS[tag] else ''
            print(f'block {tag:15s} seed {seed}: fp32 against fp64 {_bars(ref, ref64, 1e-3, 2e-5):.3f} x the bar{mark}')
    for how in R.GRAPH_SEEDS:
        for fill in range(1, 3):
            for batch in range(2):
                _, ref, imgs, targets = R.graph_case(how, (fill, batch))
                ref64 = copy.deepcopy(ref).double().train()
                ref.train()
                OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
                OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
                mark = ' <- GRAPH_SEEDS' if (fill, batch) == R.GRAPH_SEEDS[how] else ''
                print(f'graph {how:5s} seeds ({fill}, {batch}): fp32 against fp64 {_bars(ref, ref64, 2e-3, 2e-6):.3f} x the bar{mark}')


if __name__ == '__main__':
    seed_tables() if '--seeds' in sys.argv[1:] else write_fixtures()
