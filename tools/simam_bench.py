#!/usr/bin/env python3
"""Measurement of the SimAM attention family (simam.hip, blocks.SimAM / SimAMWithSlicing / SimAMWithFlexibleSlicing / Conv_SWS / PSSimAM) on
the MI355X.

Prints ONE JSON line.  Cases, batch `--batch` (32), training mode, (C, map) = (32, 160), (64, 80), (128, 40), (256, 20), (512, 20); each
case in four region grids: `map` (SimAM), `quadrants` (SimAMWithSlicing), `win8` and `win8_r0.5` (SimAMWithFlexibleSlicing at target 8,
overlap 0 and 0.5: 20 x 20 and 39 x 39 windows on the 160 x 160 map).  Per case and grid:
  kernels   stats / apply / bwd_sums / bwd_input: *_us, and *_gbs = algorithmic bytes per second, where the algorithmic bytes are what the pass
            must move: stats reads x; apply reads x and writes out; bwd_sums reads dout and x; bwd_input reads dout and x and writes dx.  The
            (B, regions, 2, C) statistics and the per-chunk partials are not counted (they are overhead, not algorithm).
  block     the gate module: fwd_us, bwd_us as (forward + backward) - forward, the tests' restatement (tests/simam_ref.py) run eagerly on the
            same GPU in the same process (eager_*), ratio = eager (forward + backward) / ours.  The restatement's window form is the vectorised
            closed form, not the reference's Python double loop over windows.
Per case also conv_sws = Conv_SWS(C, 2C, 8, 0.5, 1e-4, 3, 2) and pssimam = PSSimAM(C, C) against their restatements.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/simam_bench.py [--batch 32] [--reps 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

CASES = ((32, 160), (64, 80), (128, 40), (256, 20), (512, 20))
GRIDS = {'map': ('map', None, None, lambda M, C: M.SimAM(C)),
         'quadrants': ('quadrants', None, None, lambda M, C: M.SimAMWithSlicing(C)),
         'win8': ('windows', 8, 8, lambda M, C: M.SimAMWithFlexibleSlicing(C, 8, 0.0)),
         'win8_r0.5': ('windows', 8, 4, lambda M, C: M.SimAMWithFlexibleSlicing(C, 8, 0.5))}


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


def bench_kernels(mode, t, st, C, S, B, reps, rounds):
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C)
    x, dout = (torch.randn(B, S, S, C, generator=gen).cuda() for _ in range(2))
    grid = ops.simam_grid(mode, S, S, 1e-4, t, st)
    stats = ops.simam_stats(x, C, grid)
    sums = ops.simam_backward_sums(dout, x, stats, C, grid)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    fns = [lambda: ops.simam_stats(x, C, grid),
           lambda: ops.simam_apply(x, stats, C, grid, out=out),
           lambda: ops.simam_backward_sums(dout, x, stats, C, grid),
           lambda: ops.simam_backward_input(dout, x, stats, sums, C, grid, out=dx)]
    us = _alternate(fns, reps, rounds)
    n = 4.0 * B * S * S * C                                       # bytes of one map
    rec = dict(regions=grid[0] * grid[1])
    for (k, nbytes), u in zip((('stats', n), ('apply', 2 * n), ('bwd_sums', 2 * n), ('bwd_input', 3 * n)), us):
        rec[f'{k}_us'], rec[f'{k}_us_spread'], rec[f'{k}_gbs'] = _r1(u[0]), [_r1(u[1]), _r1(u[2])], _r1(nbytes / u[0] * 1e-3)
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import simam_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(c + S)
    x = torch.randn(B, S, S, c, generator=gen).cuda()
    mine, eager = make(MB).cuda().train(), make(R).cuda().train()
    xe = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = mine(Act(x))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    mine.backward(Act(dy))
    dye = dy[..., :y.c].permute(0, 3, 1, 2).contiguous()

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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('simam_bench needs the MI355X')
    cases = []
    for C, S in CASES:
        rec = dict(C=C, H=S, W=S, B=a.batch)
        for name, (mode, t, st, make) in GRIDS.items():
            rec[name] = dict(kernels=bench_kernels(mode, t, st, C, S, a.batch, a.reps, a.rounds),
                             block=bench_block(lambda M: make(M, C), C, S, a.batch, a.reps, a.rounds))
        rec['conv_sws'] = bench_block(lambda M: M.Conv_SWS(C, 2 * C, 8, 0.5, 1e-4, 3, 2), C, S, a.batch, a.reps, a.rounds)
        rec['pssimam'] = bench_block(lambda M: M.PSSimAM(C, C), C, S, a.batch, a.reps, a.rounds)
        cases.append(rec)
        print(f'case C={C} {S}x{S} done', file=sys.stderr, flush=True)
    print(json.dumps(dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
