#!/usr/bin/env python3
"""Measurement of the fused loss (loss.hip) under every box-regression rule on the MI355X at the SOMI head's shape: batch 32, grids
160 / 80 / 40 / 20, 4 anchors, 10 classes, the targets of `synthetic_batch`.

Prints ONE JSON line.  Per rule setting of somi_amd.loss.RULE_SETTINGS, and for the default `ComputeLoss(model)` first: one ComputeLoss call with value
and gradient (the call as the training step makes it: descriptor, workspace and gradient tensors included) in microseconds - device events
around `--reps` calls after `--warmup` calls - and its ratio to the default rule measured in the same process.  No threshold is attached.

    python tools/loss_bench.py [--batch 32] [--warmup 10] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd')]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loss_bench needs the MI355X')
    from somi_amd.configs import HYP_VISDRONE, SOMI_ANCHORS, synthetic_batch
    from somi_amd.loss import RULE_SETTINGS, ComputeLoss
    nc, na, strides = 10, 4, (4, 8, 16, 32)
    anchors = torch.tensor(SOMI_ANCHORS, dtype=torch.float32).view(4, na, 2) / torch.tensor(strides).view(4, 1, 1)
    g = torch.Generator().manual_seed(0)
    p = [torch.randn(a.batch, na, 640 // s, 640 // s, nc + 5, generator=g).cuda().requires_grad_(True) for s in strides]
    _, targets = synthetic_batch(a.batch, 64, nc=nc, seed=0)
    targets = targets.cuda()
    from types import SimpleNamespace
    model = SimpleNamespace(hyp=dict(HYP_VISDRONE), model=[SimpleNamespace(anchors=anchors, nl=4, na=na, nc=nc)])   # what ComputeLoss reads of a model

    def timed(kw):
        crit = ComputeLoss(model, **kw)

        def call():
            loss, _ = crit(p, targets)
            loss.backward()
            for t in p:
                t.grad = None
        for _ in range(a.warmup):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps
    base = timed({})
    rows = {}
    for tag, kw in RULE_SETTINGS.items():
        t = timed(kw)
        rows[tag] = dict(us=round(t, 1), vs_default=round(t / base, 3))
    print(json.dumps(dict(batch=a.batch, grids=[640 // s for s in strides], na=na, nc=nc, targets=int(targets.shape[0]), warmup=a.warmup,
                          reps=a.reps, device=torch.cuda.get_device_name(0), default_us=round(base, 1), rules=rows)))


if __name__ == '__main__':
    main()
