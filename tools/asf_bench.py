#!/usr/bin/env python3
"""Measurement of the ASF-YOLO neck (asf.hip, blocks.Zoom_cat / ScalSeq / attention_model) on the MI355X.

Prints ONE JSON line.  Shapes are those of configs.yolov5_asf_cfg at 640 x 640, batch `--batch` (32), training mode:
  zoom_cat_row12   l 80 x 80, m 40 x 40, s 20 x 20, 512 channels each        zoom_cat_row16   l 160 x 160, m 80 x 80, s 40 x 40, 256 channels each
  scalseq_row24    p3 80 x 80 x 256, p4 40 x 40 x 512, p5 20 x 20 x 1024     attention_row25  two 80 x 80 x 256 maps
Per case:
  kernels   *_us and *_gbs = algorithmic bytes per second, the algorithmic bytes being the tensors a pass must move (code bytes, per-channel
            vectors and partials are not counted): zoomcat reads l, m, s and writes out; zoomcat_bwd reads dout's l and s parts and writes dl
            and ds (dm is a slice of dout, as the block hands it out); scalseq stats reads u3, u4, u5 (21/16 of a P3 map); fuse reads them and
            writes out; route reads dout and the three maps and writes g3, g4, g5; apply reads g and u and writes g; mix_means reads x1, x2 and
            writes t; mix_bwd_sums reads dt and x1; mix_bwd_input reads dt and writes dx1; the ECA gate works on (B, C) vectors (time only).
  block     fwd_us, bwd_us as (forward + backward) - forward, and the tests' literal restatement (tests/asf_ref.py) run eagerly on the same GPU
            in the same process (eager_*); ratio_fwd = eager forward / ours, ratio = eager (forward + backward) / ours.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/asf_bench.py [--batch 32] [--reps 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402


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


def _kernel_record(names_bytes, us):
    rec = {}
    for (k, nbytes), u in zip(names_bytes, us):
        rec[f'{k}_us'], rec[f'{k}_us_spread'] = _r1(u[0]), [_r1(u[1]), _r1(u[2])]
        if nbytes:
            rec[f'{k}_gbs'] = _r1(nbytes / u[0] * 1e-3)
    return rec


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen).cuda()


def bench_zoomcat_kernels(B, H, C, reps, rounds):
    """m is H x H; l, m, s all C wide."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C + H)
    l, m, s = _rand(gen, B, 2 * H, 2 * H, C), _rand(gen, B, H, H, C), _rand(gen, B, H // 2, H // 2, C)
    dout = _rand(gen, B, H, H, 3 * C)
    out = torch.empty(B, H, H, 3 * C, device='cuda')
    _, codes = ops.zoomcat(l, m, s, C, C, C, out=out, codes=True)
    dl, ds = torch.empty_like(l), torch.empty_like(s)
    us = _alternate([lambda: ops.zoomcat(l, m, s, C, C, C, out=out, codes=True),
                     lambda: ops.zoomcat_backward(dout, codes, C, C, C, dl=(dl, 0), ds=(ds, 0))], reps, rounds)
    nm = 4.0 * B * H * H * C
    return _kernel_record((('zoomcat', nm * (4 + 1 + 0.25 + 3)), ('zoomcat_bwd', nm * (1 + 1 + 4 + 0.25))), us)


def bench_scalseq_kernels(B, H, C, reps, rounds):
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C + H)
    us_ = tuple(_rand(gen, B, H // n, H // n, C) for n in (1, 2, 4))
    dout = _rand(gen, B, H, H, C)
    gamma, beta = torch.rand(C, generator=gen).cuda() + 0.5, _rand(gen, C)
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    st = ops.scalseq_stats(us_, C, gamma, beta, 1e-5, 0.1, rm, rv)
    out = torch.empty(B, H, H, C, device='cuda')
    _, codes = ops.scalseq_fuse(us_, C, st[2], st[3], out=out, codes=True)
    gs, sums = ops.scalseq_route_backward(dout, codes, us_, C, st)
    us = _alternate([lambda: ops.scalseq_stats(us_, C, gamma, beta, 1e-5, 0.1, rm, rv),
                     lambda: ops.scalseq_fuse(us_, C, st[2], st[3], out=out, codes=True),
                     lambda: ops.scalseq_route_backward(dout, codes, us_, C, st),
                     lambda: ops.scalseq_apply_backward(gs, us_, C, st, sums)], reps, rounds)
    n3 = 4.0 * B * H * H * C
    lo = 21.0 / 16.0
    return _kernel_record((('scalseq_stats', n3 * lo), ('scalseq_fuse', n3 * (lo + 1)), ('scalseq_route', n3 * (1 + 2 * lo)),
                           ('scalseq_apply', n3 * 3 * lo)), us)


def bench_attention_kernels(B, H, C, reps, rounds):
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C + H)
    x1, x2, dt = (_rand(gen, B, H, H, C) for _ in range(3))
    avg, dgate, davg = (_rand(gen, B, C) for _ in range(3))
    w = _rand(gen, ops.eca_kernel_size(C))
    gate = ops.eca_gate(avg, w)
    t, pool, dx1 = torch.empty_like(x1), torch.empty(B, 2 * H, 1, C, device='cuda'), torch.empty_like(x1)
    us = _alternate([lambda: ops.eca_gate(avg, w), lambda: ops.eca_gate_backward(avg, w, gate, dgate),
                     lambda: ops.asf_mix_means(x1, x2, gate, C, t=t, pool=pool),
                     lambda: ops.asf_mix_backward_sums(dt, x1, C),
                     lambda: ops.asf_mix_backward_input(dt, gate, davg, C, out=dx1)], reps, rounds)
    n = 4.0 * B * H * H * C
    return _kernel_record((('eca_gate', 0), ('eca_gate_bwd', 0), ('mix_means', 3 * n), ('mix_bwd_sums', 2 * n), ('mix_bwd_input', 2 * n)), us)


def bench_block(make, shapes, reps, rounds, seed):
    """shapes: the inputs' (B, C, H, W)."""
    import asf_ref as R
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(seed)
    xs = [_rand(gen, b, h, w, c) for b, c, h, w in shapes]
    mine, eager = make(MB).cuda().train(), make(R).cuda().train()
    xe = [x.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for x in xs]
    y = mine([Act(x) for x in xs])
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    mine.backward(Act(dy))
    dye = dy[..., :y.c].permute(0, 3, 1, 2).contiguous()

    def fwd():
        mine([Act(x) for x in xs])

    def both():
        mine([Act(x) for x in xs])
        mine.backward(Act(dy))

    def efwd():
        eager(xe)

    def eboth():
        for x in xe:
            x.grad = None
        eager(xe).backward(dye)
    us = _alternate([fwd, both, efwd, eboth], reps, rounds)
    med = [u[0] for u in us]
    return dict(fwd_us=_r1(med[0]), bwd_us=_r1(med[1] - med[0]), eager_fwd_us=_r1(med[2]), eager_bwd_us=_r1(med[3] - med[2]),
                ratio_fwd=round(med[2] / med[0], 2), ratio=round(med[3] / med[1], 2), fwd_bwd_us_spread=[_r1(us[1][1]), _r1(us[1][2])],
                eager_fwd_bwd_us_spread=[_r1(us[3][1]), _r1(us[3][2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('asf_bench needs the MI355X')
    B, k = a.batch, (a.reps, a.rounds)
    cases = {}
    for name, H, C in (('zoom_cat_row12', 40, 512), ('zoom_cat_row16', 80, 256)):
        cases[name] = dict(m=[H, H, C], kernels=bench_zoomcat_kernels(B, H, C, *k),
                           block=bench_block(lambda M: M.Zoom_cat(C), [(B, C, 2 * H, 2 * H), (B, C, H, H), (B, C, H // 2, H // 2)], *k, seed=H))
        print(f'{name} done', file=sys.stderr, flush=True)
    cases['scalseq_row24'] = dict(p3=[80, 80, 256], kernels=bench_scalseq_kernels(B, 80, 256, *k),
                                  block=bench_block(lambda M: M.ScalSeq(256), [(B, 256, 80, 80), (B, 512, 40, 40), (B, 1024, 20, 20)], *k, seed=24))
    print('scalseq_row24 done', file=sys.stderr, flush=True)
    cases['attention_row25'] = dict(x=[80, 80, 256], kernels=bench_attention_kernels(B, 80, 256, *k),
                                    block=bench_block(lambda M: M.attention_model(256), [(B, 256, 80, 80), (B, 256, 80, 80)], *k, seed=25))
    print(json.dumps(dict(batch=B, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
