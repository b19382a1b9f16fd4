#!/usr/bin/env python3
"""Measurement of efficient multi-scale attention (ema.hip, blocks.EMA / iRMB_EMA / iRMB_EMABottleneck / C2f_iRMB_EMA) on the MI355X.

Prints ONE JSON line.  Cases, batch `--batch` (32): the hidden maps of the C2f_iRMB_EMA rows of configs.yolov5_ema_cfg(where='c2f') at 640 x 640,
i.e. C = 32 at 160x160, 64 at 80x80, 128 at 40x40, 256 at 20x20 (factor 8: 4, 8, 16 and 32 channels per group).  Per case:
  kernels   stats / gate / bwd_gate / bwd_norm: *_us, and *_gbs = algorithmic bytes per second, where the algorithmic bytes are what the pass
            must move: stats reads x and x2; gate reads x and x2 and writes out; bwd_gate reads dout, x and x2 and writes dx and dwgt; bwd_norm
            reads x and dwgt and writes dt and dx2; each also the (B, H + W, C) gates (bwd_norm writes their gradient as well).  Partial sums in
            the workspace and the per-(b, c) vectors are not counted (overhead, not algorithm).
  blocks    ema = EMA(C), irmb = iRMB_EMA(C), bottleneck = iRMB_EMABottleneck(C, C, True, e = 1.0), c2f = C2f_iRMB_EMA(2C, 2C, 1, True):
            training fwd_us and bwd_us as (forward + backward) - forward, infer_us the eval forward, against the tests' restatement
            (tests/ema_ref.py) run eagerly on the same GPU in the same process (eager_*); ratio = eager (forward + backward) / ours,
            infer_ratio = eager / ours.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/ema_bench.py [--batch 32] [--reps 10] [--rounds 7]
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
FACTOR = 8


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
    g, cg = FACTOR, C // FACTOR
    gen = torch.Generator().manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    x, x2, dout = r(B, S, S, C), r(B, S, S, C), r(B, S, S, C)
    sg, gamma, beta = torch.sigmoid(r(B, 2 * S, C)), 1 + 0.3 * r(cg), 0.5 * r(cg)
    out, dx, dw, dt = (torch.empty_like(x) for _ in range(4))
    dsg = torch.empty_like(sg)
    dg, db = torch.zeros(cg, device='cuda'), torch.zeros(cg, device='cuda')
    _, vec = ops.ema_stats(x, sg, C, g, gamma, beta, 1e-5, x2=x2)
    _, _, _, bvec = ops.ema_backward_gate(dout, x, x2, sg, vec, C, g, gamma, beta, dg, db, dx=dx, dw=dw)
    keep = dw.clone()

    def norm():
        ops.ema_backward_norm(x, sg, dw, vec, bvec, C, g, gamma, beta, dt=dt, dsg=dsg)       # dw is rewritten in place: the values drift, the traffic does not
    fns = [lambda: ops.ema_stats(x, sg, C, g, gamma, beta, 1e-5, x2=x2),
           lambda: ops.ema_gate(x, x2, sg, vec, C, g, gamma, beta, out=out),
           lambda: ops.ema_backward_gate(dout, x, x2, sg, vec, C, g, gamma, beta, dg, db, dx=dx, dw=keep),
           norm]
    us = _alternate(fns, reps, rounds)
    n, rows = 4.0 * B * S * S * C, 4.0 * B * 2 * S * C            # bytes of one map, of one (B, H + W, C) row tensor
    nbytes = dict(stats=2 * n + rows, gate=3 * n + rows, bwd_gate=5 * n + rows, bwd_norm=4 * n + 2 * rows)
    rec = dict(partials=ops.ema_partials(B, S, S, C))
    for i, k in enumerate(nbytes):
        rec[f'{k}_us'], rec[f'{k}_us_spread'], rec[f'{k}_gbs'] = _r1(us[i][0]), [_r1(us[i][1]), _r1(us[i][2])], _r1(nbytes[k] / us[i][0] * 1e-3)
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import ema_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(c + S)
    x, dy = torch.randn(B, S, S, c, generator=gen).cuda(), torch.randn(B, S, S, c, generator=gen).cuda()
    mine, eager = make(MB).cuda().train(), make(R).cuda().train()
    mine_e, eager_e = make(MB).cuda().eval(), make(R).cuda().eval()
    xe, dye = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True), dy.permute(0, 3, 1, 2).contiguous()
    xi = xe.detach()

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

    def infer():
        with torch.no_grad():
            mine_e(Act(x))

    def einfer():
        with torch.no_grad():
            eager_e(xi)
    us = _alternate([fwd, both, efwd, eboth, infer, einfer], reps, rounds)
    med = [u[0] for u in us]
    return dict(fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                ratio=round(med[3] / med[1], 2), fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])],
                eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])], infer_us=_r1(med[4]), eager_infer_us=_r1(med[5]),
                infer_ratio=round(med[5] / med[4], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ema_bench needs the MI355X')
    cases = []
    for C, S in CASES:
        rec = dict(C=C, H=S, W=S, B=a.batch, kernels=bench_kernels(C, S, a.batch, a.reps, a.rounds))
        rec['ema'] = bench_block(lambda M: M.EMA(C), C, S, a.batch, a.reps, a.rounds)
        rec['irmb'] = bench_block(lambda M: M.iRMB_EMA(C), C, S, a.batch, a.reps, a.rounds)
        rec['bottleneck'] = bench_block(lambda M: M.iRMB_EMABottleneck(C, C, True, e=1.0), C, S, a.batch, a.reps, a.rounds)
        rec['c2f'] = bench_block(lambda M: M.C2f_iRMB_EMA(2 * C, 2 * C, 1, True), 2 * C, S, a.batch, a.reps, a.rounds)
        cases.append(rec)
    print(json.dumps(dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, map_passes=dict(
        forward='means, stats, gate (+ conv3x3)', backward='bwd_gate, bwd_norm, means broadcast (+ conv3x3 wgrad and dgrad)'), cases=cases)))


if __name__ == '__main__':
    main()
