#!/usr/bin/env python3
"""Measurement of the patch-embedding convolutions (kernel = stride = p, no padding) and of the blocks built on them (blocks.MultiSEAM) and of
blocks.SEAM with two stages, on the MI355X.

Prints ONE JSON line (and keeps a copy in profiles/seam_bench_line.json unless --no-save), batch `--batch` (32):
  kernels   (a) forward, data gradient and weight gradient of the p x p / stride p 256 -> 256 conv for p = 3, 5, 7 on 160x160 and 80x80 maps, each
            beside its FLOP-equal twin: the 1x1 256 -> 256 conv over a (Ho * p) x (Wo * p) map (the part of the map the patches cover, as a
            tensor of its own) - 2 * B * Ho * Wo * p^2 * 256^2 flop both.  *_us with (min, max), *_tflops, twin_*_us and *_ratio = time / twin's
            time (reported, not judged).
  parent    with --parent-lib PATH (a libsomi_hip.so built from the parent commit): the p = 7 launches again in fresh child processes, this
            build and the parent's alternating (`--ab` runs each), medians per launch and ratio = this / parent.  The parent runs p = 7 on
            the generic path, so it is the yardstick for the PATCH instantiation.
  blocks    (b) MultiSEAM(256, 256, 1) and SEAM(256, 256, 2) at 160x160 and 80x80: training forward and backward (bwd_us as (forward +
            backward) - forward) and the eval forward, each against the tests' restatement (tests/seam_ref.py) run eagerly on channels_last
            tensors of the same shapes on the same GPU in the same process (eager_*); ratio = eager (forward + backward) / ours, eval_ratio likewise.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.
Fails without a GPU: nothing here falls back to another path.

    python tools/seam_bench.py [--batch 32] [--reps 10] [--rounds 7] [--parent-lib PATH] [--only kernels|p7|blocks]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

PATCHES = (3, 5, 7)
SIZES = (160, 80)
C = 256
OUT = os.path.join(ROOT, 'profiles', 'seam_bench_line.json')


def _events_us(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _alternate(fns, reps, rounds):
    """(median, min, max) microseconds of each function over `rounds` rounds, the functions taking turns inside every round."""
    import torch
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


def _conv_fns(B, S, p, gen, twin):
    """The three launches of the p x p / stride p conv on an S x S map, or (twin) of the 1x1 conv over the (Ho * p) x (Wo * p) map."""
    import torch
    from somi_amd import ops
    Ho = S // p
    H, k = (Ho * p, 1) if twin else (S, p)
    Hy = H if twin else Ho
    x, dy = torch.randn(B, H, H, C, generator=gen).cuda(), torch.randn(B, Hy, Hy, C, generator=gen).cuda()
    w = (torch.randn(C, k * k * C, generator=gen) / math.sqrt(k * k * C)).cuda()
    wt = (torch.randn(C, k * k * C, generator=gen) / math.sqrt(k * k * C)).cuda()
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
    geo = dict(kh=k, kw=k, stride=k, pad=0)
    return [lambda: ops.conv2d_nhwc(x, w, None, act='none', out=y, **geo),
            lambda: ops.conv2d_dgrad_nhwc(dy, wt, B=B, H=H, W=H, cin=C, out=dx, **geo),
            lambda: ops.conv2d_wgrad_nhwc(x, dy, out=dw, **geo)]


def bench_kernels(B, reps, rounds, patches=PATCHES, twins=True):
    import torch
    gen = torch.Generator().manual_seed(7)
    rec = dict(B=B, C=C)
    for S in SIZES:
        fns = []
        for p in patches:
            fns += _conv_fns(B, S, p, gen, False)
            if twins:
                fns += _conv_fns(B, S, p, gen, True)
        us = _alternate(fns, reps, rounds)
        per = 6 if twins else 3
        for i, p in enumerate(patches):
            flop = 2.0 * B * (S // p) ** 2 * p * p * C * C
            r = dict(Ho=S // p, gflop=round(flop * 1e-9, 1))
            for j, what in enumerate(('fwd', 'dgrad', 'wgrad')):
                med, lo, hi = us[per * i + j]
                r[f'{what}_us'], r[f'{what}_us_spread'], r[f'{what}_tflops'] = _r1(med), [_r1(lo), _r1(hi)], round(flop / med * 1e-6, 1)
                if twins:
                    tm = us[per * i + 3 + j][0]
                    r[f'twin_{what}_us'], r[f'twin_{what}_tflops'], r[f'{what}_ratio'] = _r1(tm), round(flop / tm * 1e-6, 1), round(med / tm, 3)
            rec[f's{S}_p{p}'] = r
        del fns
        torch.cuda.empty_cache()
    return rec


def bench_parent(a):
    """The p = 7 launches in fresh child processes, this build and the parent's taking turns.  -> per launch: medians of both and their ratio."""
    runs = {'this': [], 'parent': []}
    for _ in range(a.ab):
        for side in ('parent', 'this'):
            env = dict(os.environ)
            env.pop('SOMI_HIP_LIB', None)
            if side == 'parent':
                env['SOMI_HIP_LIB'] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--only', 'p7', '--no-save', '--batch', str(a.batch), '--reps', str(a.reps),
                                '--rounds', str(a.rounds)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
            if r.returncode != 0:
                return dict(error=f'{side} build: exit {r.returncode}: {r.stderr[-400:]}')
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1])['kernels'])
    rec = dict(runs_each=a.ab)
    for S in SIZES:
        key = f's{S}_p7'
        for what in ('fwd', 'dgrad', 'wgrad'):
            t = [r[key][f'{what}_us'] for r in runs['this']]
            q = [r[key][f'{what}_us'] for r in runs['parent']]
            rec[f'{key}_{what}'] = dict(this_us=t, parent_us=q, ratio=round(statistics.median(t) / statistics.median(q), 3))
    return rec


def bench_block(make, S, B, reps, rounds):
    import torch
    import seam_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(C + S)
    x, dy = torch.randn(B, S, S, C, generator=gen).cuda(), torch.randn(B, S, S, C, generator=gen).cuda()
    mine, eager = make(MB).cuda().train(), make(R).cuda().to(memory_format=torch.channels_last).train()
    mine_e, eager_e = make(MB).cuda().eval(), make(R).cuda().to(memory_format=torch.channels_last).eval()
    xe, dye = x.permute(0, 3, 1, 2).requires_grad_(True), dy.permute(0, 3, 1, 2)      # channels_last views of the same NHWC storage
    assert xe.is_contiguous(memory_format=torch.channels_last)
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
    return dict(C=C, H=S, W=S, B=B, fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                ratio=round(med[3] / med[1], 2), fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])],
                eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])], eval_us=_r1(med[4]), eager_eval_us=_r1(med[5]),
                eval_ratio=round(med[5] / med[4], 2), eval_us_spread=[_r1(us[4][1]), _r1(us[4][2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--ab', type=int, default=3, help='child runs per build of the comparison with --parent-lib')
    ap.add_argument('--parent-lib', default=None, help='a libsomi_hip.so of the parent commit: p = 7 launches on both builds, in child processes')
    ap.add_argument('--only', choices=('kernels', 'p7', 'blocks'), default=None)
    ap.add_argument('--no-save', action='store_true')
    a = ap.parse_args()
    rec = dict(batch=a.batch, reps=a.reps, rounds=a.rounds)
    if a.parent_lib and a.only in (None, 'kernels'):               # before this process opens the device: one child at a time
        rec['parent'] = bench_parent(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('seam_bench needs the MI355X')
    rec['device'] = torch.cuda.get_device_name(0)
    if a.only == 'p7':
        rec['kernels'] = bench_kernels(a.batch, a.reps, a.rounds, patches=(7,), twins=False)
    elif a.only in (None, 'kernels'):
        rec['kernels'] = bench_kernels(a.batch, a.reps, a.rounds)
    if a.only in (None, 'blocks'):
        for S in SIZES:
            rec[f'multiseam_{S}'] = bench_block(lambda M: M.MultiSEAM(C, C, 1), S, a.batch, a.reps, a.rounds)
            torch.cuda.empty_cache()
            rec[f'seam_n2_{S}'] = bench_block(lambda M: M.SEAM(C, C, 2), S, a.batch, a.reps, a.rounds)
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if not a.no_save:
        with open(OUT, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
