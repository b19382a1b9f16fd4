#!/usr/bin/env python3
"""Measurement of the CBAM C3 family (cbam_c3.hip, blocks.C3_CBAM / C3_SCBAM / C3CBAM) on the MI355X.

Prints ONE JSON line.  Batch `--batch` (32), training mode.
  combine   the gate-combine passes alone at C = 128 on 40x40 (the hidden width of C3_SCBAM(256, 256)) and C = 32 on 160x160 (the first
            backbone row), in both modes: forward (with the shortcut), the per-pixel backward pass, the per-element backward pass; *_us and
            *_gbs = algorithmic bytes per second - 3 tensor passes for the forward (t and the shortcut read, out written), 2 for the per-pixel
            pass (dout and t read), 3 for the per-element pass (dout and t read, dt written); the gates, the arg-max maps and the partial rows
            are not counted.
  dwc_gate  the depthwise-separable spatial gate (k = 7) alone on the statistics maps of the same two cases: training forward, backward,
            inference, *_us and algorithmic GB/s.
  blocks    c3_cbam = C3_CBAM(256, 256, 1) and c3_cbam_dwc = C3_CBAM_DWC(256, 256, 1) at 40x40, c3_scbam = C3_SCBAM(128, 128, 1) at 80x80, c3cbam = C3CBAM(256, 256) at 20x20: fwd_us,
            bwd_us as (forward + backward) - forward, the tests' restatement (tests/cbam_c3_ref.py) run eagerly on the same GPU in the same
            process (eager_*), ratio = eager (forward + backward) / ours.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/cbam_c3_bench.py [--batch 32] [--reps 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

COMBINE_CASES = ((128, 40), (32, 160))


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


def bench_combine(C, S, B, reps, rounds):
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    t, res, dout, out, dt = r(B, S, S, C), r(B, S, S, C), r(B, S, S, C), torch.empty(B, S, S, C, device='cuda'), torch.empty(B, S, S, C, device='cuda')
    ca, sa, dstats = torch.sigmoid(r(B, C)), torch.sigmoid(r(B, S, S)), r(B, S, S, 2)
    t_max = t.reshape(B, -1, C).max(1)[0].contiguous()
    n = 4.0 * B * S * S * C
    rec = {}
    for mode in ('product', 'sigmoid_sum'):
        _, amaxc, _ = ops.gate_combine_backward_pixel(dout, t, ca, sa, C, mode, t_max=t_max)
        fns = [lambda: ops.gate_combine(t, ca, sa, C, mode, residual=res, out=out),
               lambda: ops.gate_combine_backward_pixel(dout, t, ca, sa, C, mode, t_max=t_max, logit=True),
               lambda: ops.gate_combine_backward_chan(dout, t, ca, sa, dstats, amaxc, C, mode, dt=dt)]
        us = _alternate(fns, reps, rounds)
        for (k, passes), u in zip((('fwd', 3), ('bwd_pixel', 2), ('bwd_chan', 3)), us):
            rec[f'{mode}_{k}_us'], rec[f'{mode}_{k}_us_spread'] = _r1(u[0]), [_r1(u[1]), _r1(u[2])]
            rec[f'{mode}_{k}_gbs'] = _r1(passes * n / u[0] * 1e-3)
    return rec


def bench_dwc_gate(C, S, B, reps, rounds, k=7):
    """The depthwise-separable gate alone on the (B, S, S, 2) statistics map behind a C-channel tensor: training forward (3 launches), backward
    (6), inference (1); bytes: stats read + sa written (+ u, p written in training; backward reads dsa, stats, u, p and writes dstats)."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(S)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    stats, dsa, params = r(B, S, S, 2), r(B, S, S), r(2 * k * k + 11) * 0.3
    params[2 * k * k + 2:2 * k * k + 4], params[2 * k * k + 9] = 1.0, 1.0
    run = torch.tensor([0., 0., 1., 1., 0., 1.]).cuda()
    sa, u, p, st = ops.dwc_gate_train(stats, params, run, k, 1e-3, 0.03)
    dparams = torch.zeros_like(params)
    us = _alternate([lambda: ops.dwc_gate_train(stats, params, run, k, 1e-3, 0.03), lambda: ops.dwc_gate_backward(dsa, stats, u, p, st, params, k, dparams),
                     lambda: ops.dwc_gate_eval(stats, params, run, k, 1e-3)], reps, rounds)
    n = 4.0 * B * S * S
    rec = dict(C=C, H=S, W=S, k=k)
    for (name, floats), t in zip((('train_fwd', 6), ('bwd', 8), ('eval', 3)), us):
        rec[f'{name}_us'], rec[f'{name}_us_spread'], rec[f'{name}_gbs'] = _r1(t[0]), [_r1(t[1]), _r1(t[2])], _r1(floats * n / t[0] * 1e-3)
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import cbam_c3_ref as R
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
    return dict(C=c, H=S, W=S, fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                fwd_ratio=round(med[2] / med[0], 2), ratio=round(med[3] / med[1], 2), fwd_us_spread=[_r1(us[0][1]), _r1(us[0][2])],
                fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])], eager_fwd_us_spread=[_r1(us[2][1]), _r1(us[2][2])],
                eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cbam_c3_bench needs the MI355X')
    combine = [dict(C=C, H=S, W=S, **bench_combine(C, S, a.batch, a.reps, a.rounds)) for C, S in COMBINE_CASES]
    blocks = dict(c3_cbam=bench_block(lambda M: M.C3_CBAM(256, 256, 1), 256, 40, a.batch, a.reps, a.rounds),
                  c3_cbam_dwc=bench_block(lambda M: M.C3_CBAM_DWC(256, 256, 1), 256, 40, a.batch, a.reps, a.rounds),
                  c3_scbam=bench_block(lambda M: M.C3_SCBAM(128, 128, 1), 128, 80, a.batch, a.reps, a.rounds),
                  c3cbam=bench_block(lambda M: M.C3CBAM(256, 256), 256, 20, a.batch, a.reps, a.rounds))
    dwc = [bench_dwc_gate(C, S, a.batch, a.reps, a.rounds) for C, S in COMBINE_CASES]
    print(json.dumps(dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, combine=combine, dwc_gate=dwc,
                          blocks=blocks)))


if __name__ == '__main__':
    main()
