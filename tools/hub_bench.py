#!/usr/bin/env python3
"""Measurement of the max-pool kernels (pool.hip) and the stock hub graphs they open, on the MI355X.

Prints ONE JSON line:
  pool2: every pooling shape of yolov3-tiny at `--batch` x `--size`^2 (the five nn.MaxPool2d(2, 2, 0) maps from size^2 x 16 down, and the zero-padded
         nn.MaxPool2d(2, 1, 0) at (size / 32)^2 x 512): training forward (values + codes) and backward in microseconds (device events around `--reps`
         launches after a warm-up, median of `--rounds` rounds), the algorithmic bytes (one read of x, one write of y, the codes; backward likewise)
         over that time as GB/s and as a share of the 8 TB/s HBM peak, and beside it eager PyTorch's max_pool2d (+ F.pad) forward + backward on
         channels_last tensors of the same shape, measured in the same rounds, the two alternating; `ratio` = eager / (forward + backward).
  spp:   the same for the parallel windows of SPP in yolov3-spp ((5, 9, 13) at 512 channels, stride 32), yolov5-p6 ((3, 5, 7), 512 channels, stride 64)
         and yolov5-p7 ((3, 5), 640 channels, stride 128); for (5, 9, 13) also the chained 5x5 kernels the SPP block itself keeps using for that set.
  train / infer: images/s of TrainStep.step and of the eval forward for yolov3, yolov3-tiny (their own multiples), yolov5-panet (width 0.5, depth 0.33)
         and yolov5s, synthetic batch, weights from configs.fill_state.

    python tools/hub_bench.py [--batch 32] [--size 640] [--steps 3] [--warmup 2] [--reps 20] [--rounds 5]
    python tools/hub_bench.py --only train-tiny --steps 3 --warmup 1          # a few yolov3-tiny training steps (under rocprofv3)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd')]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8.0e12


def _events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _alternate(fns, reps, rounds):
    """Median microseconds of each function over `rounds` rounds, the functions taking turns inside every round."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(_events_us(fn, reps))
    return [statistics.median(g) for g in got]


def _row(us_f, us_b, us_e, bytes_f, bytes_b):
    return dict(fwd_us=round(us_f, 1), bwd_us=round(us_b, 1), fwd_gbs=round(bytes_f / us_f / 1e3, 1), bwd_gbs=round(bytes_b / us_b / 1e3, 1),
                fwd_peak_share=round(bytes_f / (us_f * 1e-6) / HBM_PEAK, 3), bwd_peak_share=round(bytes_b / (us_b * 1e-6) / HBM_PEAK, 3),
                eager_fwd_bwd_us=round(us_e, 1), ratio=round(us_e / (us_f + us_b), 2))


def bench_pool2(B, side, C, stride, pad, reps, rounds):
    from somi_amd import ops
    x = torch.randn(B, side, side, C, device='cuda')
    y, codes = ops.maxpool2(x, C, stride=stride, pad=pad, codes=True)
    dy = torch.randn_like(y)
    dx = torch.empty_like(x)
    xe = x.permute(0, 3, 1, 2).detach().requires_grad_(True)     # NCHW view of the NHWC storage = channels_last
    dye = dy.permute(0, 3, 1, 2)
    assert xe.is_contiguous(memory_format=torch.channels_last)

    def fwd():
        ops.maxpool2(x, C, stride=stride, pad=pad, out=y, codes=True)

    def bwd():
        ops.maxpool2_backward(dy, codes, C, side, side, stride=stride, pad=pad, out=dx)

    def eager():
        xe.grad = None
        F.max_pool2d(F.pad(xe, pad) if any(pad) else xe, 2, stride, 0).backward(dye)
    us_f, us_b, us_e = _alternate([fwd, bwd, eager], reps, rounds)
    n_in, n_out = x.numel(), y.numel()
    return dict(B=B, H=side, W=side, C=C, stride=stride, pad=list(pad), **_row(us_f, us_b, us_e, 4 * n_in + 5 * n_out, 5 * n_out + 4 * n_in))


def bench_spp(B, side, C, k, reps, rounds):
    from somi_amd import ops
    nk = len(k)
    buf = torch.randn(B, side, side, (nk + 1) * C, device='cuda')
    dbuf = torch.randn_like(buf)
    _, codes = ops.spp_pool_(buf, C, k, 0, codes=True)
    xe = buf[..., :C].contiguous().permute(0, 3, 1, 2).detach().requires_grad_(True)
    dys = [torch.randn(B, side, side, C, device='cuda').permute(0, 3, 1, 2) for _ in k]

    def fwd():
        ops.spp_pool_(buf, C, k, 0, codes=True)

    def bwd():
        ops.spp_pool_backward_(dbuf, codes, C, k, 0)

    def eager():
        xe.grad = None
        torch.autograd.backward([F.max_pool2d(xe, kk, 1, kk // 2) for kk in k], dys)
    fns = [fwd, bwd, eager]
    if tuple(k) == (5, 9, 13):
        c5 = ops.sppf_pool_(buf, C, 0, codes=True)[1]
        fns += [lambda: ops.sppf_pool_(buf, C, 0, codes=True), lambda: ops.sppf_pool_backward_(buf, dbuf, C, 0, codes=c5)]
    us = _alternate(fns, reps, rounds)
    n = B * side * side * C
    row = dict(B=B, H=side, W=side, C=C, k=list(k), **_row(us[0], us[1], us[2], n * (4 + 5 * nk), n * (5 * nk + 8)))
    if len(us) > 3:
        row.update(chained5_fwd_us=round(us[3], 1), chained5_bwd_us=round(us[4], 1))
    return row


def _cfg(name):
    from somi_amd import configs
    return {'yolov3': lambda: configs.yolov3_cfg(''), 'yolov3-tiny': lambda: configs.yolov3_cfg('tiny'),
            'yolov5-panet': lambda: configs.yolov5_hub_cfg('panet', 0.5, 0.33), 'yolov5s': lambda: configs.yolov5_cfg()}[name]()


def bench_graph(name, batch, size, steps, warmup, train):
    from somi_amd.configs import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    model = fill_state(Model(_cfg(name)), 1).cuda()
    imgs, targets = synthetic_batch(batch, size, nc=80, seed=0)
    imgs, targets = imgs.cuda(), targets.cuda()
    if train:
        tr = TrainStep(model, dict(HYP_VISDRONE), batch)
        run = lambda: tr.step(imgs, targets)                                                     # noqa: E731
    else:
        model.eval()

        def run():
            with torch.no_grad():
                model(imgs)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dict(ms_per_step=round(dt * 1e3, 2), images_per_s=round(batch / dt, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', choices=['all', 'pool', 'train-tiny'], default='all')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hub_bench needs the MI355X')
    res = dict(batch=a.batch, size=a.size, device=torch.cuda.get_device_name(0))
    if a.only in ('all', 'pool'):
        s = a.size
        res['pool2'] = [bench_pool2(a.batch, s >> i, 16 << i, 2, (0, 0, 0, 0), a.reps, a.rounds) for i in range(5)]
        res['pool2'].append(bench_pool2(a.batch, s >> 5, 512, 1, (0, 1, 0, 1), a.reps, a.rounds))
        res['spp'] = [bench_spp(a.batch, s >> 5, 512, (5, 9, 13), a.reps, a.rounds), bench_spp(a.batch, s >> 6, 512, (3, 5, 7), a.reps, a.rounds),
                      bench_spp(a.batch, s >> 7, 640, (3, 5), a.reps, a.rounds)]
    if a.only == 'train-tiny':
        res['train'] = {'yolov3-tiny': bench_graph('yolov3-tiny', a.batch, a.size, a.steps, a.warmup, True)}
    elif a.only == 'all':
        names = ('yolov3', 'yolov3-tiny', 'yolov5-panet', 'yolov5s')
        res['train'] = {n: bench_graph(n, a.batch, a.size, a.steps, a.warmup, True) for n in names}
        res['infer'] = {n: bench_graph(n, a.batch, a.size, a.steps, a.warmup, False) for n in names}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
