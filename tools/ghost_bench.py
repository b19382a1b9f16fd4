#!/usr/bin/env python3
"""Measurement of the grouped / depthwise convolution and the yolov5s-ghost graph (models/hub/yolov5s-ghost.yaml) on the MI355X.

Prints ONE JSON line:
  dw_layers: every distinct grouped-conv shape of the yolov5s-ghost graph at the given batch / size (width 0.5): forward (eval form: folded
             BatchNorm + act), data- and weight-gradient times in microseconds (device events around `--reps` launches after a warm-up),
             and algorithmic GB/s = the bytes the layer must move (input + output activations, logical channels, fp32) over that time, with
             the share of the 8 TB/s HBM peak;
  train / infer: images/s of TrainStep.step and of the eval forward for yolov5s-ghost and stock yolov5s (same batch and size, synthetic
             batch, weights from configs.fill_state), and their ratio.

    python tools/ghost_bench.py [--batch 32] [--size 640] [--steps 10] [--warmup 3] [--reps 50]
    python tools/ghost_bench.py --only train-ghost --steps 3 --warmup 1        # the ghost training step alone (under rocprofv3)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd')]

import torch  # noqa: E402

HBM_PEAK = 8.0e12


def _events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def ghost_layer_shapes(batch, size):
    """(B, H, W, c1, c2, groups, k, stride) of every grouped conv one eval forward of yolov5s-ghost launches."""
    from somi_amd import ops
    from somi_amd.configs import fill_state, yolov5_ghost_cfg
    from somi_amd.model import Model
    seen, real = [], ops.gconv2d_nhwc

    def spy(x, w, bias=None, **kw):
        key = (x.shape[0], x.shape[1], x.shape[2], kw['c1'], kw['c2'], kw['groups'], kw['k'], kw.get('stride', 1))
        if key not in seen:
            seen.append(key)
        return real(x, w, bias, **kw)
    model = fill_state(Model(yolov5_ghost_cfg()), 1).cuda().eval()
    ops.gconv2d_nhwc = spy
    try:
        with torch.no_grad():
            model(torch.zeros(batch, 3, size, size, dtype=torch.uint8, device='cuda'))
    finally:
        ops.gconv2d_nhwc = real
    torch.cuda.synchronize()
    return seen


def bench_layers(batch, size, reps):
    from somi_amd import ops
    from somi_amd.pack import pack_gconv_weight, pad4
    out = []
    for B, H, W, c1, c2, g, k, s in ghost_layer_shapes(batch, size):
        Ho, Wo = ops.conv_out_size(H, k, s, k // 2), ops.conv_out_size(W, k, s, k // 2)
        x = torch.randn(B, H, W, pad4(c1), device='cuda')
        dy = torch.randn(B, Ho, Wo, pad4(c2), device='cuda')
        wp = pack_gconv_weight(torch.randn(c2, c1 // g, k, k), pad4(c2)).cuda()
        bias = torch.zeros(pad4(c2), device='cuda')
        y = torch.empty(B, Ho, Wo, pad4(c2), device='cuda')
        dx = torch.empty(B, H, W, pad4(c1), device='cuda')
        dw = torch.zeros(c2, c1 // g, k, k, device='cuda')
        geo = dict(c1=c1, c2=c2, groups=g, k=k, stride=s)
        fwd = lambda: ops.gconv2d_nhwc(x, wp, bias, out=y, act='silu', **geo)                     # noqa: E731
        dgr = lambda: ops.gconv2d_dgrad_nhwc(dy, wp, H=H, W=W, out=dx, **geo)                     # noqa: E731
        wgr = lambda: ops.gconv2d_wgrad_nhwc(x, dy, out=dw, accumulate=True, **geo)              # noqa: E731
        row = dict(B=B, H=H, W=W, c1=c1, c2=c2, groups=g, k=k, stride=s)
        bx, by = 4.0 * B * H * W * c1, 4.0 * B * Ho * Wo * c2
        for name, fn, nbytes in (('fwd', fwd, bx + by), ('dgrad', dgr, by + bx), ('wgrad', wgr, bx + by)):
            for _ in range(3):
                fn()
            us = _events_us(fn, reps)
            row[f'{name}_us'] = round(us, 2)
            row[f'{name}_GBps'] = round(nbytes / (us * 1e-6) / 1e9, 1)
            row[f'{name}_hbm_pct'] = round(100.0 * nbytes / (us * 1e-6) / HBM_PEAK, 1)
        out.append(row)
    return out


def bench_graph(cfg_name, batch, size, steps, warmup, train):
    from somi_amd.configs import HYP_VISDRONE, fill_state, synthetic_batch, yolov5_cfg, yolov5_ghost_cfg
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    cfg = yolov5_ghost_cfg() if cfg_name == 'ghost' else yolov5_cfg()
    model = fill_state(Model(cfg), 1).cuda()
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
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--only', choices=['all', 'layers', 'train-ghost'], default='all')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ghost_bench needs the MI355X')
    res = dict(batch=a.batch, size=a.size, device=torch.cuda.get_device_name(0))
    if a.only in ('all', 'layers'):
        res['dw_layers'] = bench_layers(a.batch, a.size, a.reps)
    if a.only == 'train-ghost':
        res['train'] = {'yolov5s-ghost': bench_graph('ghost', a.batch, a.size, a.steps, a.warmup, True)}
    elif a.only == 'all':
        res['train'] = {n: bench_graph(g, a.batch, a.size, a.steps, a.warmup, True) for n, g in (('yolov5s-ghost', 'ghost'), ('yolov5s', 's'))}
        res['infer'] = {n: bench_graph(g, a.batch, a.size, a.steps, a.warmup, False) for n, g in (('yolov5s-ghost', 'ghost'), ('yolov5s', 's'))}
        for k in ('train', 'infer'):
            res[k]['ghost_over_yolov5s_time'] = round(res[k]['yolov5s-ghost']['ms_per_step'] / res[k]['yolov5s']['ms_per_step'], 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
