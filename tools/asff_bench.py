#!/usr/bin/env python3
"""Measurement of the ASFF head's blocks (asff.hip, blocks.ASFF) on the MI355X.

Prints ONE JSON line.  Cases, batch `--batch` (32), training mode, the level shapes of a 640 x 640 image: ASFF(0) at 20x20, ASFF(1) at 40x40,
ASFF(2) at 80x80, each on the pyramid P5 (512, 20x20), P4 (256, 40x40), P3 (128, 80x80).  Per case:
  fwd_us / bwd_us               the whole block: forward, and backward as (forward + backward) - forward
  eager_fwd_us / eager_bwd_us   the tests' restatement of the reference (tests/asff_ref.py) run eagerly on the same GPU in the same process,
                                autograd for the backward
  ratio                         eager (forward + backward) / ours (forward + backward)
  fuse_fwd_us / fuse_bwd_us     the fusion kernels alone on the block's resized maps and weight maps (training forward: p is written), with
                                fuse_fwd_gbs / fuse_bwd_gbs = their algorithmic traffic per second: forward reads every r_i and v_i once at its own
                                resolution and writes fused and p; backward reads dfused, r_i, v_i and p and writes every dr_i and dv_i at its own
                                resolution
  eager_fuse_fwd_us / eager_fuse_bwd_us   the stage the kernels replace, eagerly: nearest upsampling of the low-resolution maps, the 48-channel concat,
                                the 1x1 conv, the softmax, three products and two sums (backward by autograd: forward + backward - forward)
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/asff_bench.py [--batch 32] [--reps 10] [--rounds 7]
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


def bench(level, B, reps, rounds):
    import asff_ref as R
    from somi_amd import blocks as MB
    from somi_amd import ops
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(level)
    dims, sides = (512, 256, 128), (20, 40, 80)
    xs = [torch.randn(B, s, s, c, generator=gen).cuda() for c, s in zip(dims, sides)]
    C, side = dims[level], sides[level]
    dy = torch.randn(B, side, side, C, generator=gen).cuda()
    mine, eager = MB.ASFF(level).cuda().train(), R.ASFF(level).cuda().train()
    xe = [x.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for x in xs]
    dye = dy.permute(0, 3, 1, 2).contiguous()

    def fwd():
        mine(*(Act(x) for x in xs))

    def both():
        mine(*(Act(x) for x in xs))
        mine.backward(Act(dy))

    def efwd():
        eager(*xe)

    def eboth():
        for x in xe:
            x.grad = None
        eager(*xe).backward(dye)
    # the fusion stage alone, at the block's own resolutions
    ups = [u for _, u in mine._resizers()]
    rs = [torch.randn(B, side >> u, side >> u, C, generator=gen).cuda() for u in ups]
    vs = [torch.randn(B, side >> u, side >> u, 16, generator=gen).cuda() for u in ups]
    w, b = (torch.randn(3, 48, generator=gen) * 0.3).cuda(), torch.randn(3, generator=gen).cuda()
    rd, vd = [(t, 0) for t in rs], [(t, 0) for t in vs]
    _, p = ops.asff_fuse(rd, vd, ups, ups, w, b, C, weights=True)
    dw, db = torch.zeros(3, 48, device='cuda'), torch.zeros(3, device='cuda')
    re_ = [t.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in rs]
    ve = [t.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in vs]
    conv = torch.nn.Conv2d(48, 3, 1).cuda()

    def kf():
        ops.asff_fuse(rd, vd, ups, ups, w, b, C, weights=True)

    def kb():
        ops.asff_fuse_backward(dy, rd, vd, ups, ups, w, b, p, C, dw, db)

    def _efuse():
        up = lambda t, u: F.interpolate(t, scale_factor=1 << u, mode='nearest') if u else t       # noqa: E731
        r = [up(t, u) for t, u in zip(re_, ups)]
        pe = F.softmax(conv(torch.cat([up(t, u) for t, u in zip(ve, ups)], 1)), dim=1)
        return r[0] * pe[:, 0:1] + r[1] * pe[:, 1:2] + r[2] * pe[:, 2:]

    def ef():
        _efuse()

    def eb():
        for t in re_ + ve:
            t.grad = None
        conv.zero_grad(set_to_none=True)
        _efuse().backward(dye)
    us = _alternate([fwd, both, efwd, eboth, kf, kb, ef, eb], reps, rounds)
    med = [u[0] for u in us]
    npix = B * side * side
    low = sum((C + 16) * (npix >> (2 * u)) for u in ups)          # every r_i and v_i once, at its own resolution
    fwd_bytes = 4.0 * (low + (C + 3) * npix)
    bwd_bytes = 4.0 * ((C + 3) * npix + 2 * low)
    r1 = lambda v: round(v, 1)                                    # noqa: E731
    return dict(case=f'asff{level}', B=B, C=C, H=side, W=side, ups=ups, fwd_us=r1(med[0]), bwd_us=r1(med[1] - med[0]),
                eager_fwd_us=r1(med[2]), eager_bwd_us=r1(med[3] - med[2]), ratio=round(med[3] / med[1], 2),
                fwd_bwd_us_spread=[r1(us[1][1]), r1(us[1][2])], eager_fwd_bwd_us_spread=[r1(us[3][1]), r1(us[3][2])],
                fuse_fwd_us=r1(med[4]), fuse_bwd_us=r1(med[5]), fuse_fwd_us_spread=[r1(us[4][1]), r1(us[4][2])],
                fuse_bwd_us_spread=[r1(us[5][1]), r1(us[5][2])], fuse_fwd_gbs=r1(fwd_bytes / med[4] * 1e-3), fuse_bwd_gbs=r1(bwd_bytes / med[5] * 1e-3),
                eager_fuse_fwd_us=r1(med[6]), eager_fuse_bwd_us=r1(med[7] - med[6]), fuse_fwd_ratio=round(med[6] / med[4], 2),
                fuse_bwd_ratio=round((med[7] - med[6]) / med[5], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('asff_bench needs the MI355X')
    res = dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds,
               cases=[bench(level, a.batch, a.reps, a.rounds) for level in range(3)])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
