#!/usr/bin/env python3
"""Measurement of the slim-neck blocks (gsconv.hip, blocks.GSConv / GSCBAMBottleneck / VoVGSCSPCBAM) on the MI355X.

Prints ONE JSON line.
  kernels   the three kernels alone at half width c_ = 64 (a GSConv(128, 128)) on 80x80 and 40x40 maps: tail at batch 32 and 128 (inference),
            shuffle and unshuffle at batch 32 (training).  *_us, and *_gbs = algorithmic bytes per second: c_ read + 2 c_ written per pixel for
            the tail (weights and the halo's second read not counted), 2 c_ + 2 c_ for the two streaming kernels.  tail_eager_us: what stands
            behind cv1 in the restatement (two depthwise Conv blocks in eval mode, two torch.cat and the reshape / permute) in eager PyTorch.
  blocks    GSConv(128, 128, 1, 1), GSConv(128, 128, 3, 1, act=False) and VoVGSCSPCBAM(256, 256, 1, False) at 80x80 and 40x40.  train
            (batch 32): fwd_us, bwd_us as (forward + backward) - forward, ratio = eager (forward + backward) / ours; eval (batch 32 and 128):
            fwd_us and ratio.  Eager is the tests' restatement (tests/slimneck_ref.py) on the same GPU in the same process.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/slimneck_bench.py [--batch 32] [--eval-batches 32 128] [--reps 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

MAPS = (80, 40)
HALF = 64
BLOCKS = {'gsconv_1x1': (lambda M: M.GSConv(128, 128, 1, 1), 128), 'gsconv_3x3_noact': (lambda M: M.GSConv(128, 128, 3, 1, act=False), 128),
          'vovgscspcbam': (lambda M: M.VoVGSCSPCBAM(256, 256, 1, False), 256)}


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


def bench_kernels(S, B, eval_batches, reps, rounds):
    import slimneck_ref as R
    from somi_amd import ops
    from somi_amd.pack import pack_gconv_weight
    c = HALF
    gen = torch.Generator().manual_seed(S)
    r = lambda *s: torch.randn(*s, generator=gen).cuda()          # noqa: E731
    w1, w2, b1, b2 = pack_gconv_weight(r(c, 1, 3, 3) / 3), pack_gconv_weight(r(c, 1, 3, 3) / 3), r(c), r(c)
    eager = _filled(lambda ns: ns.GSConv(2 * c, 2 * c, 1, 1), R).cuda().eval()
    rec = {}
    for b in eval_batches:
        x1, out = r(b, S, S, c), torch.empty(b, S, S, 2 * c, device='cuda')
        xe = x1.permute(0, 3, 1, 2).contiguous()

        def e_tail(xe=xe):
            with torch.no_grad():
                return eager.shuffle(torch.cat((xe, eager.cv2_2(eager.cv2_1(xe))), 1))
        us = _alternate([lambda x1=x1, out=out: ops.gs_tail(x1, w1, b1, w2, b2, c, 'silu', out=out), e_tail], reps, rounds)
        n = 4.0 * b * S * S * c
        rec[f'tail_b{b}'] = dict(us=_r1(us[0][0]), us_spread=[_r1(us[0][1]), _r1(us[0][2])], gbs=_r1(3 * n / us[0][0] * 1e-3),
                                 eager_us=_r1(us[1][0]), ratio=round(us[1][0] / us[0][0], 2))
    z1, y2, out, res = r(B, S, S, c), r(B, S, S, c), torch.empty(B, S, S, 2 * c, device='cuda'), r(B, S, S, 2 * c)
    d1, d2, scale, shift = torch.empty_like(z1), torch.empty_like(z1), r(c), r(c)
    us = _alternate([lambda: ops.gs_shuffle_affine_act(z1, y2, c, scale, shift, 'silu', out=out),
                     lambda: ops.gs_shuffle_affine_act(z1, y2, c, scale, shift, 'none', out=out, residual=res),
                     lambda: ops.gs_unshuffle(res, c, d1=d1, d2=d2)], reps, rounds)
    n = 4.0 * B * S * S * c
    for key, u, passes in (('shuffle', us[0], 4), ('shuffle_residual', us[1], 6), ('unshuffle', us[2], 4)):
        rec[f'{key}_b{B}'] = dict(us=_r1(u[0]), us_spread=[_r1(u[1]), _r1(u[2])], gbs=_r1(passes * n / u[0] * 1e-3),
                                  tiles_per_workgroup=ops.gs_tiles_per_workgroup(B * S * S, c))
    return rec


def bench_block(make, c, S, B, eval_batches, reps, rounds):
    import slimneck_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    eager = _filled(make, R).cuda()
    mine = make(MB)
    mine.load_state_dict(eager.state_dict())
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
        mine.backward(Act(dy))          # the attention's backward works in dy in place: its values change, the work does not

    def efwd():
        eager(xe)

    def eboth():
        xe.grad = None
        eager(xe).backward(dye)
    us = _alternate([fwd, both, efwd, eboth], reps, rounds)
    med = [u[0] for u in us]
    rec[f'train_b{B}'] = dict(fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                              fwd_ratio=round(med[2] / med[0], 2), ratio=round(med[3] / med[1], 2),
                              fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])], eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])])
    del xe, dye, dy, y
    mine.eval(), eager.eval()
    for b in eval_batches:
        x = torch.randn(b, S, S, c, generator=gen).cuda()
        xe = x.permute(0, 3, 1, 2).contiguous()

        def ev(x=x):
            with torch.no_grad():
                mine(Act(x))

        def eev(xe=xe):
            with torch.no_grad():
                eager(xe)
        us = _alternate([ev, eev], reps, rounds)
        rec[f'eval_b{b}'] = dict(fwd_us=_r1(us[0][0]), eager_fwd_us=_r1(us[1][0]), ratio=round(us[1][0] / us[0][0], 2),
                                 fwd_us_spread=[_r1(us[0][1]), _r1(us[0][2])], eager_fwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])])
        del x, xe
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--eval-batches', type=int, nargs='+', default=[32, 128])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('slimneck_bench needs the MI355X')
    kernels = [dict(half=HALF, H=S, W=S, **bench_kernels(S, a.batch, a.eval_batches, a.reps, a.rounds)) for S in MAPS]
    blocks = {name: [bench_block(make, c, S, a.batch, a.eval_batches, a.reps, a.rounds) for S in MAPS] for name, (make, c) in BLOCKS.items()}
    print(json.dumps(dict(batch=a.batch, eval_batches=a.eval_batches, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds,
                          kernels=kernels, blocks=blocks)))


if __name__ == '__main__':
    main()
