#!/usr/bin/env python3
"""Measurement of dilated convolution and the context blocks built on it (blocks.ASPP, blocks.C2f_DWR) on the MI355X.

Prints ONE JSON line, batch `--batch` (32):
  kernels   forward, data gradient and weight gradient of a 3x3 256 -> 256 conv at 40x40 (stride 1, pad = d) for d = 1, 3, 5: *_us with
            (min, max), *_tflops (2 * B * H * W * Cout * Cin * 9 flop each) and, for d > 1, *_ratio = time / time of the d = 1 twin - the same
            shape and the same FLOPs, so the ratio is what the dilated tap walk costs.
  blocks    aspp = ASPP(512, 512) at 20x20, c2f_dwr = C2f_DWR(256, 256, 1, True) at 40x40: training forward and backward (bwd_us as
            (forward + backward) - forward) and the eval forward, each against the tests' restatement (tests/context_ref.py) run eagerly on the
            same GPU in the same process (eager_*); ratio = eager (forward + backward) / ours, eval_ratio likewise.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.
Fails without a GPU: nothing here falls back to another path.

    python tools/context_bench.py [--batch 32] [--reps 10] [--rounds 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

DILATIONS = (1, 3, 5)
KERNEL_SHAPE = dict(H=40, W=40, Cin=256, Cout=256, k=3)


def _events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _alternate(fns, reps, rounds):
    """(median, min, max) microseconds of each function over `rounds` rounds, the functions taking turns inside every round."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(_events_us(fn, reps))
    return [(statistics.median(g), min(g), max(g)) for g in got]


def _r1(v):
    return round(v, 1)


def bench_kernels(B, reps, rounds):
    from somi_amd import ops
    H, W, Cin, Cout, k = (KERNEL_SHAPE[n] for n in ('H', 'W', 'Cin', 'Cout', 'k'))
    gen = torch.Generator().manual_seed(7)
    x, dy = torch.randn(B, H, W, Cin, generator=gen).cuda(), torch.randn(B, H, W, Cout, generator=gen).cuda()
    w = (torch.randn(Cout, k * k * Cin, generator=gen) / math.sqrt(k * k * Cin)).cuda()
    wt = (torch.randn(Cin, k * k * Cout, generator=gen) / math.sqrt(k * k * Cout)).cuda()
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
    fns = []
    for d in DILATIONS:
        geo = dict(kh=k, kw=k, stride=1, pad=d, dil=d)
        fns += [lambda geo=geo: ops.conv2d_nhwc(x, w, None, act='none', out=y, **geo),
                lambda geo=geo: ops.conv2d_dgrad_nhwc(dy, wt, B=B, H=H, W=W, cin=Cin, out=dx, **geo),
                lambda geo=geo: ops.conv2d_wgrad_nhwc(x, dy, out=dw, **geo)]
    us = _alternate(fns, reps, rounds)
    flop = 2.0 * B * H * W * Cout * Cin * k * k
    rec = dict(B=B, **KERNEL_SHAPE)
    for i, d in enumerate(DILATIONS):
        r = {}
        for j, what in enumerate(('fwd', 'dgrad', 'wgrad')):
            med, lo, hi = us[3 * i + j]
            r[f'{what}_us'], r[f'{what}_us_spread'], r[f'{what}_tflops'] = _r1(med), [_r1(lo), _r1(hi)], round(flop / med * 1e-6, 1)
            if d > 1:
                r[f'{what}_ratio'] = round(med / us[j][0], 3)
        rec[f'd{d}'] = r
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import context_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(c + S)
    x, dy = torch.randn(B, S, S, c, generator=gen).cuda(), torch.randn(B, S, S, c, generator=gen).cuda()
    mine, eager = make(MB).cuda().train(), make(R).cuda().train()
    mine_e, eager_e = make(MB).cuda().eval(), make(R).cuda().eval()
    xe, dye = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True), dy.permute(0, 3, 1, 2).contiguous()
    xn = xe.detach()

    def fwd():
        mine(Act(x))

    def both():
        mine(Act(x))
        mine.backward(Act(dy))

    def efwd():
        eager(xe)

    def eboth():
        xe.grad = None
        eager(xe).backward(dye)

    def ev():
        mine_e(Act(x))

    def eev():
        with torch.no_grad():
            eager_e(xn)
    us = _alternate([fwd, both, efwd, eboth, ev, eev], reps, rounds)
    med = [u[0] for u in us]
    return dict(C=c, H=S, W=S, B=B, fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                ratio=round(med[3] / med[1], 2), fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])],
                eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])], eval_us=_r1(med[4]), eager_eval_us=_r1(med[5]),
                eval_ratio=round(med[5] / med[4], 2), eval_us_spread=[_r1(us[4][1]), _r1(us[4][2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('context_bench needs the MI355X')
    rec = dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds,
               kernels=bench_kernels(a.batch, a.reps, a.rounds),
               aspp=bench_block(lambda M: M.ASPP(512, 512), 512, 20, a.batch, a.reps, a.rounds),
               c2f_dwr=bench_block(lambda M: M.C2f_DWR(256, 256, 1, True), 256, 40, a.batch, a.reps, a.rounds))
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
