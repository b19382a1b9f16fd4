#!/usr/bin/env python3
"""Measurement of the large-kernel depthwise kernels (dwlk.hip) and the blocks on them (blocks.CNeB / ConvMix / CSPCM) on the MI355X.

Prints ONE JSON line.
  kernels   forward (bias + GELU + post-affine + residual, the ConvMix inference launch; and with statistics, its training launch), data
            gradient (+ acc1) and weight + bias gradient at k = 7 and 9, at the hidden widths and maps configs.yolov5_convnext_cfg takes at 640^2
            (c_ = 32 on 160x160 ... 256 on 20x20), batch --batch.  *_us; *_tfma = algorithmic multiply-adds (k * k per output element) per
            second / 1e12; *_gbs = algorithmic bytes per second: x read + y written (+ the residual / acc1 read) for the two stencils, x + dy
            read for the weight gradient.  gconv5_us: the parent's 5x5 depthwise forward (somi_gconv2d_nhwc_f32, k = 5, bias, no activation)
            at the same shape in the same process, the arms taking turns; plain_us: the new forward in the same form (bias only); vs5 =
            plain_us / gconv5_us against the tap ratio k * k / 25 that extending the direct stencil would have cost.
  blocks    CNeB(2 c, 2 c, 1), ConvMix(c, c) and CSPCM(2 c, 2 c, 1) at (c, map) = (64, 80) and (128, 40): train (batch --batch) fwd_us, bwd_us as
            (forward + backward) - forward, ratio = eager (forward + backward) / ours; eval fwd_us and ratio.  Eager is the tests'
            restatement (tests/convnext_ref.py) on the same GPU in the same process.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/convnext_bench.py [--batch 32] [--reps 5] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

SHAPES = ((32, 160), (64, 80), (128, 40), (256, 20))             # (c_, map) of the four swapped backbone rows at width 0.50, 640^2
BLOCK_SHAPES = ((64, 80), (128, 40))
BLOCKS = {'cneb': lambda c: (lambda M: M.CNeB(2 * c, 2 * c, 1), 2 * c), 'convmix': lambda c: (lambda M: M.ConvMix(c, c), c),
          'cspcm': lambda c: (lambda M: M.CSPCM(2 * c, 2 * c, 1), 2 * c)}


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


def _filled(make, ns, seed=3):
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    ref = fill_state(make(ns), seed)
    OB.initialize_weights(ref)
    return ref


def bench_kernels(c, S, B, reps, rounds):
    from somi_amd import ops
    from somi_amd.pack import pack_gconv_weight
    gen = torch.Generator().manual_seed(c + S)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    x, dy, res, y = r(B, S, S, c), r(B, S, S, c), r(B, S, S, c), torch.empty(B, S, S, c, device='cuda')
    bias, ps, pt, piv = r(c), r(c), r(c), r(c)
    w5 = pack_gconv_weight(r(c, 1, 5, 5) / 5)
    n = 4.0 * B * S * S * c                                       # bytes of one tensor pass
    rec = dict(C=c, H=S, W=S)
    for k in (7, 9):
        w = pack_gconv_weight(r(c, 1, k, k) / k)
        dw, db = torch.empty(c, 1, k, k, device='cuda'), torch.empty(c, device='cuda')
        fns = [lambda: ops.gconv2d_nhwc(x, w5, bias, c1=c, c2=c, groups=c, k=5, out=y),
               lambda: ops.dwlk(x, w, bias, c=c, k=k, out=y),
               lambda: ops.dwlk(x, w, bias, c=c, k=k, act='gelu', post_scale=ps, post_shift=pt, out=y, residual=res),
               lambda: ops.dwlk(x, w, bias, c=c, k=k, act='gelu', out=y, bn_stats={'pivot': piv}),
               lambda: ops.dwlk_dgrad(dy, w, c=c, k=k, out=y, accumulate=res),
               lambda: ops.dwlk_wgrad(x, dy, c=c, k=k, dw=dw, db=db)]
        us = _alternate(fns, reps, rounds)
        fma = 1.0 * B * S * S * c * k * k
        out = dict(gconv5_us=_r1(us[0][0]), gconv5_us_spread=[_r1(us[0][1]), _r1(us[0][2])], plain_us=_r1(us[1][0]),
                   plain_us_spread=[_r1(us[1][1]), _r1(us[1][2])], vs5=round(us[1][0] / us[0][0], 2), taps_vs5=round(k * k / 25, 2),
                   strips_per_workgroup=[ops.dwlk_strips_per_workgroup(B, S, S, c), ops.dwlk_strips_per_workgroup(B, S, S, c, True)])
        for key, u, passes in (('fwd', us[2], 3), ('fwd_stats', us[3], 2), ('dgrad', us[4], 3), ('wgrad', us[5], 2)):
            out[key] = dict(us=_r1(u[0]), us_spread=[_r1(u[1]), _r1(u[2])], tfma=round(fma / u[0] * 1e-6, 2), gbs=_r1(passes * n / u[0] * 1e-3))
        rec[f'k{k}'] = out
    return rec


def bench_block(make, c, S, B, reps, rounds):
    import convnext_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    eager = _filled(make, R).cuda()
    mine = make(MB)
    mine.load_state_dict(eager.state_dict())
    for m in mine.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.03
    mine = mine.cuda()
    gen = torch.Generator().manual_seed(c + S)
    rec = dict(C=c, H=S, W=S)
    mine.train(), eager.train()
    x = torch.randn(B, S, S, c, generator=gen).cuda()
    y = mine(Act(x))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    mine.backward(Act(dy.clone()))
    xe, dye = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True), dy[..., y.coff:y.coff + y.c].permute(0, 3, 1, 2).contiguous()

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
    rec['train'] = dict(fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                        fwd_ratio=round(med[2] / med[0], 2), ratio=round(med[3] / med[1], 2),
                        fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])], eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])])
    mine.eval(), eager.eval()
    xn = xe.detach()

    def ev():
        with torch.no_grad():
            mine(Act(x))

    def eev():
        with torch.no_grad():
            eager(xn)
    us = _alternate([ev, eev], reps, rounds)
    rec['eval'] = dict(fwd_us=_r1(us[0][0]), eager_fwd_us=_r1(us[1][0]), ratio=round(us[1][0] / us[0][0], 2),
                       fwd_us_spread=[_r1(us[0][1]), _r1(us[0][2])], eager_fwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('convnext_bench needs the MI355X')
    kernels = [bench_kernels(c, S, a.batch, a.reps, a.rounds) for c, S in SHAPES]
    blocks = {}
    for name, mk in BLOCKS.items():
        blocks[name] = []
        for c, S in BLOCK_SHAPES:
            make, width = mk(c)
            blocks[name].append(bench_block(make, width, S, a.batch, a.reps, a.rounds))
    print(json.dumps(dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, kernels=kernels, blocks=blocks)))


if __name__ == '__main__':
    main()
