#!/usr/bin/env python3
"""Measurement of coordinate attention (coordatt.hip, blocks.CoorAttention / CABottleneck / C3_CA) on the MI355X.

Prints ONE JSON line.  Cases, batch `--batch` (32), training mode: the maps the C3_CA rows of yolov5s see at 640 x 640, i.e. the hidden width
C = 32 at 160x160, 64 at 80x80, 128 at 40x40, 256 at 20x20.  Per case:
  kernels   means / apply (with the shortcut) / bwd_gates / bwd_input: *_us, and *_gbs = algorithmic bytes per second, where the algorithmic
            bytes are what the pass must move: means reads x and writes the (B, H + W, C) means; apply reads x, the shortcut and the gates and
            writes out; bwd_gates reads dout, x and the gates and writes the two gate gradients; bwd_input reads dout, the gates and the two
            mean gradients and writes dx.  Partial sums in the workspace are not counted (they are overhead, not algorithm).
            eager_means_us / eager_apply_us / eager_bwd_us: the same stages in eager PyTorch on NCHW tensors (the backward by autograd of the
            product, forward + backward - forward: it stands against bwd_gates + bwd_input together).
  blocks    coordatt = CoorAttention(C, C), cabottleneck = CABottleneck(C, C, True, 1, 1.0), c3_ca = C3_CA(2C, 2C, 1): fwd_us, bwd_us as
            (forward + backward) - forward, the tests' restatement (tests/coordatt_ref.py) run eagerly on the same GPU in the same process
            (eager_*), ratio = eager (forward + backward) / ours.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/coordatt_bench.py [--batch 32] [--reps 10] [--rounds 7]
    python tools/coordatt_bench.py --trace 256,20        # the four kernels of one case alone, 50 calls each, nothing timed: the run for
                                                         # `rocprofv3 --kernel-trace --stats`, whose per-kernel durations exclude the launches
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

CASES = ((32, 160), (64, 80), (128, 40), (256, 20))


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


def bench_kernels(C, S, B, reps, rounds):
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    x, res, dout = r(B, S, S, C), r(B, S, S, C), r(B, S, S, C)
    gates, grads = torch.sigmoid(r(B, 2 * S, 1, 2 * C)), r(B, 2 * S, 1, C)
    a_h, a_w = (gates, 0, 0), (gates, C, S)
    out, dx, dg = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(gates)
    pool = torch.empty(B, 2 * S, 1, C, device='cuda')
    xe, rese, doute = (t.permute(0, 3, 1, 2).contiguous() for t in (x, res, dout))
    xe.requires_grad_(True)
    ahe = gates[:, :S, 0, :C].permute(0, 2, 1).contiguous().unsqueeze(3).requires_grad_(True)       # (B, C, S, 1)
    awe = gates[:, S:, 0, C:].permute(0, 2, 1).contiguous().unsqueeze(2).requires_grad_(True)       # (B, C, 1, S)

    def e_apply():
        return rese + xe * awe * ahe

    def e_both():
        xe.grad = ahe.grad = awe.grad = None
        e_apply().backward(doute)
    fns = [lambda: ops.coordatt_means(x, C, out=pool),
           lambda: ops.coordatt_apply(x, a_h, a_w, C, res=res, out=out),
           lambda: ops.coordatt_backward_gates(dout, x, a_h, a_w, C, da_h=(dg, 0, 0), da_w=(dg, C, S)),
           lambda: ops.coordatt_backward_input(dout, a_h, a_w, (grads, 0, 0), (grads, 0, S), C, out=dx),
           lambda: torch.cat([xe.mean(3), xe.mean(2)], 2), e_apply, e_both]
    us = _alternate(fns, reps, rounds)
    med = [u[0] for u in us]
    n, rows = 4.0 * B * S * S * C, 4.0 * B * 2 * S * C            # bytes of one map, of one (B, H + W, C) row tensor
    nbytes = dict(means=n + rows, apply=3 * n + rows, bwd_gates=2 * n + 2 * rows, bwd_input=2 * n + 2 * rows)
    rec = {}
    for i, k in enumerate(nbytes):
        rec[f'{k}_us'], rec[f'{k}_us_spread'], rec[f'{k}_gbs'] = _r1(med[i]), [_r1(us[i][1]), _r1(us[i][2])], _r1(nbytes[k] / med[i] * 1e-3)
    rec.update(eager_means_us=_r1(med[4]), eager_apply_us=_r1(med[5]), eager_bwd_us=_r1(med[6] - med[5]),
               means_ratio=round(med[4] / med[0], 2), apply_ratio=round(med[5] / med[1], 2),
               bwd_ratio=round((med[6] - med[5]) / (med[2] + med[3]), 2))
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import coordatt_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(c + S)
    x, dy = torch.randn(B, S, S, c, generator=gen).cuda(), torch.randn(B, S, S, c, generator=gen).cuda()
    mine, eager = make(MB).cuda().train(), make(R).cuda().train()
    xe, dye = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True), dy.permute(0, 3, 1, 2).contiguous()

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
    us = _alternate([fwd, both, efwd, eboth], reps, rounds)
    med = [u[0] for u in us]
    return dict(fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                ratio=round(med[3] / med[1], 2), fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])],
                eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--trace', metavar='C,S', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('coordatt_bench needs the MI355X')
    if a.trace:
        C, S = (int(v) for v in a.trace.split(','))
        bench_kernels(C, S, a.batch, 50, 1)
        print(json.dumps(dict(traced=dict(C=C, H=S, W=S, B=a.batch, calls_per_kernel=53))))
        return
    cases = []
    for C, S in CASES:
        rec = dict(C=C, H=S, W=S, B=a.batch, kernels=bench_kernels(C, S, a.batch, a.reps, a.rounds))
        rec['coordatt'] = bench_block(lambda M: M.CoorAttention(C, C), C, S, a.batch, a.reps, a.rounds)
        rec['cabottleneck'] = bench_block(lambda M: M.CABottleneck(C, C, True, 1, 1.0), C, S, a.batch, a.reps, a.rounds)
        rec['c3_ca'] = bench_block(lambda M: M.C3_CA(2 * C, 2 * C, 1), 2 * C, S, a.batch, a.reps, a.rounds)
        cases.append(rec)
    print(json.dumps(dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
