#!/usr/bin/env python3
"""Measurement of channel prior convolutional attention (cpca.hip, blocks.CPCA / CPCABottleneck / C3CPCA) on the MI355X.

Prints ONE JSON line.  Batch `--batch` (32), training mode.
  strips    the strip kernels alone at the maps they see: C = 512 at 20x20 (CPCA behind SPPF of yolov5s at 640^2), C = 128 at 40x40 (the hidden
            width of C3CPCA(256, 256)), and C = 32 at 160x160 (the first C3CPCA row), where the tensors leave the caches.  fanout_w / fanin_h
            (the forward), fanout_h_flip / fanin_w_flip (the data gradient), wgrad: *_us, and *_gbs = algorithmic bytes per second - 4 tensor
            passes for a fan-out (one read, three written), 5 for a fan-in (four read, one written), 8 reads for wgrad; taps, biases and the
            partial rows of wgrad are not counted.  eager_fwd_us / eager_bwd_us: the six depthwise convs and three adds in eager PyTorch on
            NCHW tensors, forward and (forward + backward) - forward (it stands against the two backward strips and wgrad together).
  blocks    cpca = CPCA(512) at 20x20, c3cpca = C3CPCA(256, 256, 1) at 40x40: fwd_us, bwd_us as (forward + backward) - forward, the tests'
            restatement (tests/cpca_ref.py) run eagerly on the same GPU in the same process (eager_*), ratio = eager (forward + backward) / ours.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/cpca_bench.py [--batch 32] [--reps 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

STRIP_CASES = ((512, 20), (128, 40), (32, 160))
TAPS = (7, 11, 21)


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


def bench_strips(C, S, B, reps, rounds):
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    u, ds = r(B, S, S, C), r(B, S, S, C)
    wh, wv = [r(C, 1, 1, k) / k ** 0.5 for k in TAPS], [r(C, 1, k, 1) / k ** 0.5 for k in TAPS]
    bh, bv = [r(C) for _ in TAPS], [r(C) for _ in TAPS]
    ts, dts = [torch.empty_like(u) for _ in TAPS], [torch.empty_like(u) for _ in TAPS]
    s, du = torch.empty_like(u), torch.empty_like(u)
    grads = [[torch.zeros_like(w) for w in wh], [torch.zeros_like(w) for w in wv], [torch.zeros(C, device='cuda') for _ in TAPS],
             [torch.zeros(C, device='cuda') for _ in TAPS]]
    ue, dse = u.permute(0, 3, 1, 2).contiguous().requires_grad_(True), ds.permute(0, 3, 1, 2).contiguous()
    params = [p.clone().requires_grad_(True) for p in (*wh, *wv, *bh, *bv)]

    def e_fwd():
        out = ue
        for i, k in enumerate(TAPS):
            t = F.conv2d(ue, params[i], params[6 + i], padding=(0, k // 2), groups=C)
            out = out + F.conv2d(t, params[3 + i], params[9 + i], padding=(k // 2, 0), groups=C)
        return out

    def e_both():
        ue.grad = None
        for p in params:
            p.grad = None
        e_fwd().backward(dse)
    fns = [lambda: ops.cpca_fanout(u, wh, bh, C, axis='w', outs=ts),
           lambda: ops.cpca_fanin(ts, u, wv, bv, C, axis='h', out=s),
           lambda: ops.cpca_fanout(ds, wv, None, C, axis='h', flip=True, outs=dts),
           lambda: ops.cpca_fanin(dts, ds, wh, None, C, axis='w', flip=True, out=du),
           lambda: ops.cpca_wgrad(u, ts, ds, dts, C, *grads),
           e_fwd, e_both]
    us = _alternate(fns, reps, rounds)
    med = [v[0] for v in us]
    n = 4.0 * B * S * S * C
    nbytes = dict(fanout_w=4 * n, fanin_h=5 * n, fanout_h_flip=4 * n, fanin_w_flip=5 * n, wgrad=8 * n)
    rec = {}
    for i, k in enumerate(nbytes):
        rec[f'{k}_us'], rec[f'{k}_us_spread'], rec[f'{k}_gbs'] = _r1(med[i]), [_r1(us[i][1]), _r1(us[i][2])], _r1(nbytes[k] / med[i] * 1e-3)
    rec.update(eager_fwd_us=_r1(med[5]), eager_bwd_us=_r1(med[6] - med[5]), fwd_ratio=round(med[5] / (med[0] + med[1]), 2),
               bwd_ratio=round((med[6] - med[5]) / (med[2] + med[3] + med[4]), 2))
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import cpca_ref as R
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
        raise SystemExit('cpca_bench needs the MI355X')
    strips = [dict(C=C, H=S, W=S, **bench_strips(C, S, a.batch, a.reps, a.rounds)) for C, S in STRIP_CASES]
    blocks = dict(cpca=bench_block(lambda M: M.CPCA(512), 512, 20, a.batch, a.reps, a.rounds),
                  c3cpca=bench_block(lambda M: M.C3CPCA(256, 256, 1), 256, 40, a.batch, a.reps, a.rounds))
    print(json.dumps(dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, strips=strips, blocks=blocks)))


if __name__ == '__main__':
    main()
