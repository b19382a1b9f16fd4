#!/usr/bin/env python3
"""Measurement of the PSA attention kernels and the yolov10 graph (models/hub/yolov10.yaml) on the MI355X.

Prints ONE JSON line:
  attention: PSA at width 1.0 (8 heads, 512 channels per branch) at batch 32, N = 400 (640x640) and batch 8, N = 1600 (1280x1280):
             forward (with the log-sum-exp and the v copy, as training runs it) and backward in microseconds (device events around
             `--reps` launches after a warm-up) and TFLOP/s, with the forward counted as 2*B*heads*N^2*96 and the backward as 2.5x that;
             beside it the same math in eager PyTorch (matmul + softmax, N x N materialised, autograd backward) on the same GPU, and the
             peak memory each allocates above its inputs;
  train / infer: images/s of TrainStep.step and of the eval forward for yolov10 at widths 1.0 and 0.25 (depth 1.0 / 0.33), synthetic batch,
             weights from configs.fill_state.

    python tools/yolov10_bench.py [--batch 32] [--size 640] [--steps 5] [--warmup 2] [--reps 20]
    python tools/yolov10_bench.py --only train-w1 --steps 1 --warmup 1        # one width-1.0 training step (under rocprofv3)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd')]

import torch  # noqa: E402


def _events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench_attention(B, side, heads, reps):
    from somi_amd import ops
    N = side * side
    qkv = torch.randn(B, side, side, 128 * heads, device='cuda')
    dout = torch.randn(B, side, side, 64 * heads, device='cuda')
    o, lse, _ = ops.psa_attention(qkv, heads, lse=True, v_out=True)
    g = torch.empty_like(qkv)
    fwd = lambda: ops.psa_attention(qkv, heads, out=o, lse=True, v_out=True)                        # noqa: E731
    bwd = lambda: ops.psa_attention_backward(qkv, o, dout, lse, heads, out=g)                      # noqa: E731

    def both():
        fwd()
        bwd()

    def eager():
        t = qkv.detach().view(B, N, heads, 128).permute(0, 2, 1, 3).requires_grad_(True)
        q, k, v = t[..., :32], t[..., 32:64], t[..., 64:]
        p = (q @ k.transpose(-2, -1) * 32 ** -0.5).softmax(-1)
        y = (p @ v).permute(0, 2, 1, 3).reshape(B, side, side, 64 * heads)
        y.backward(dout)
        return t.grad

    def eager_fwd():
        with torch.no_grad():
            t = qkv.view(B, N, heads, 128).permute(0, 2, 1, 3)
            p = (t[..., :32] @ t[..., 32:64].transpose(-2, -1) * 32 ** -0.5).softmax(-1)
            return (p @ t[..., 64:]).permute(0, 2, 1, 3).reshape(B, side, side, 64 * heads)
    for fn in (fwd, bwd, eager, eager_fwd):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    flop = 2.0 * B * heads * N * N * 96
    us_f, us_b, us_e, us_ef = _events_us(fwd, reps), _events_us(bwd, reps), _events_us(eager, reps), _events_us(eager_fwd, reps)
    row = dict(B=B, N=N, heads=heads, fwd_us=round(us_f, 1), bwd_us=round(us_b, 1), fwd_tflops=round(flop / us_f / 1e6, 2),
               bwd_tflops=round(2.5 * flop / us_b / 1e6, 2), fwd_bwd_us=round(us_f + us_b, 1), eager_fwd_us=round(us_ef, 1),
               eager_fwd_bwd_us=round(us_e, 1), speedup_fwd=round(us_ef / us_f, 2), speedup_fwd_bwd=round(us_e / (us_f + us_b), 2),
               peak_mib=_peak_mib(both), eager_peak_mib=_peak_mib(eager))
    return row


def bench_graph(width, depth, batch, size, steps, warmup, train):
    from somi_amd.configs import HYP_VISDRONE, fill_state, synthetic_batch, yolov10_cfg
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    model = fill_state(Model(yolov10_cfg(width, depth)), 1).cuda()
    imgs, targets = synthetic_batch(batch, size, nc=10, seed=0)
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
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', choices=['all', 'attention', 'train-w1'], default='all')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('yolov10_bench needs the MI355X')
    res = dict(batch=a.batch, size=a.size, device=torch.cuda.get_device_name(0))
    if a.only in ('all', 'attention'):
        res['attention'] = [bench_attention(32, 20, 8, a.reps), bench_attention(8, 40, 8, a.reps)]
    graphs = (('w1.0', 1.0, 1.0), ('w0.25', 0.25, 0.33))
    if a.only == 'train-w1':
        res['train'] = {'w1.0': bench_graph(1.0, 1.0, a.batch, a.size, a.steps, a.warmup, True)}
    elif a.only == 'all':
        res['train'] = {n: bench_graph(w, d, a.batch, a.size, a.steps, a.warmup, True) for n, w, d in graphs}
        res['infer'] = {n: bench_graph(w, d, a.batch, a.size, a.steps, a.warmup, False) for n, w, d in graphs}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
