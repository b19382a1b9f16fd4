#!/usr/bin/env python3
"""Measurement of the two learned 2x upsamplers (upsample.hip, blocks.CARAFE / blocks.DySample) on the MI355X.

Prints ONE JSON line.  For each block at the SOMI neck's three upsampling sites - `--channels` (256) channels, source maps of 20^2 / 40^2 / 80^2
(a 640 px image), batch `--batch` (32) - in training mode:
  fwd_us / bwd_us             the whole block (its convs and BatchNorms included): forward, and backward as (forward + backward) - forward
  kernel_fwd_us / _bwd_us     the upsampling kernels alone (ops.carafe + ops.carafe_backward, ops.dysample + ops.dysample_backward)
  eager_fwd_us / _bwd_us      eager PyTorch of the reference's formulation on the same GPU in the same process: CARAFE = nearest upsample -> nn.Unfold
                              (dilation 2) -> einsum with the pixel-shuffled softmax; DySample = pixel_shuffle of the coordinates -> grid_sample
  ratio                       eager (forward + backward) / ours (forward + backward)
  peak_mb / eager_peak_mb     peak allocated memory of one forward + backward above what was allocated before it
Device events around `reps` calls after a warm-up, the median of `--rounds` rounds; the two sides take turns inside every round.

    python tools/upsample_bench.py [--batch 32] [--channels 256] [--sizes 20 40 80] [--reps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd')]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402


class _ConvBnAct(nn.Module):
    def __init__(self, c1, c2, k=1, act=True):
        super().__init__()
        self.conv, self.bn, self.act = nn.Conv2d(c1, c2, k, 1, k // 2, bias=False), nn.BatchNorm2d(c2, 1e-3, 0.03), nn.SiLU() if act else nn.Identity()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class EagerCARAFE(nn.Module):
    """The formulation with the unfolded tensor (B, C, k_up^2, 2H, 2W)."""

    def __init__(self, c, k_enc=3, k_up=5, c_mid=64):
        super().__init__()
        self.comp, self.enc = _ConvBnAct(c, c_mid), _ConvBnAct(c_mid, (2 * k_up) ** 2, k_enc, act=False)
        self.unfold = nn.Unfold(k_up, dilation=2, padding=k_up // 2 * 2)

    def forward(self, x):
        b, c, h, w = x.shape
        wts = torch.softmax(F.pixel_shuffle(self.enc(self.comp(x)), 2), 1)
        cols = self.unfold(F.interpolate(x, scale_factor=2, mode='nearest')).view(b, c, -1, 2 * h, 2 * w)
        return torch.einsum('bkhw,bckhw->bchw', wts, cols)


class EagerDySample(nn.Module):
    """The formulation through pixel_shuffle, permute and grid_sample (style 'lp')."""

    def __init__(self, c, groups=4):
        super().__init__()
        self.groups = groups
        self.offset = nn.Conv2d(c, 8 * groups, 1)
        nn.init.normal_(self.offset.weight, 0, 0.001)
        nn.init.zeros_(self.offset.bias)
        h = torch.tensor([-0.25, 0.25])
        self.register_buffer('init_pos', torch.stack([h.view(1, 1, 2).expand(groups, 2, 2), h.view(1, 2, 1).expand(groups, 2, 2)]).reshape(1, -1, 1, 1))

    def forward(self, x):
        B, C, H, W = x.shape
        off = (self.offset(x) * 0.25 + self.init_pos).reshape(B, 2, -1, H, W)
        base = torch.stack(torch.meshgrid(torch.arange(W, device=x.device) + 0.5, torch.arange(H, device=x.device) + 0.5, indexing='xy')).view(1, 2, 1, H, W)
        norm = torch.tensor([W, H], device=x.device, dtype=x.dtype).view(1, 2, 1, 1, 1)
        coords = 2 * (base + off) / norm - 1
        coords = F.pixel_shuffle(coords.reshape(B, -1, H, W), 2).reshape(B, 2, -1, 2 * H, 2 * W).permute(0, 2, 3, 4, 1).contiguous().flatten(0, 1)
        return F.grid_sample(x.reshape(B * self.groups, -1, H, W), coords, mode='bilinear', align_corners=False,
                             padding_mode='border').reshape(B, -1, 2 * H, 2 * W)


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
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(_events_us(fn, reps))
    return [statistics.median(g) for g in got]


def _peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench(kind, B, C, side, reps, rounds):
    from somi_amd import blocks as MB
    from somi_amd import ops
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(side)
    x = torch.randn(B, side, side, C, generator=gen).cuda()
    dy = torch.randn(B, 2 * side, 2 * side, C, generator=gen).cuda()
    mine = (MB.CARAFE(C, 3, 5) if kind == 'carafe' else MB.DySample(C)).cuda().train()
    eager = (EagerCARAFE(C) if kind == 'carafe' else EagerDySample(C)).cuda().train()
    xe = x.permute(0, 3, 1, 2).detach().requires_grad_(True)     # NCHW view of the NHWC storage = channels_last
    dye = dy.permute(0, 3, 1, 2)

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
    if kind == 'carafe':
        logits = torch.randn(B, side, side, 100, generator=gen).cuda()
        out, wts = ops.carafe(x, logits, C, 5, weights=True)
        dxk, dlk = ops.carafe_backward(dy, x, wts, C, 5)
        kf = lambda: ops.carafe(x, logits, C, 5, out=out, weights=True)                            # noqa: E731
        kb = lambda: ops.carafe_backward(dy, x, wts, C, 5, out=dxk, dlogits=dlk)                   # noqa: E731
    else:
        off = (torch.randn(B, side, side, 32, generator=gen) * 0.25).cuda()
        ip = mine.init_pos.reshape(-1)
        out = ops.dysample(x, off, ip, C, 4)
        dxk, dok = ops.dysample_backward(dy, x, off, ip, C, 4)
        kf = lambda: ops.dysample(x, off, ip, C, 4, out=out)                                        # noqa: E731
        kb = lambda: ops.dysample_backward(dy, x, off, ip, C, 4, out=dxk, doffset=dok)             # noqa: E731
    both(), eboth()                                                                                 # gradients allocated before peaks are read
    peak, epeak = _peak_mb(both), _peak_mb(eboth)
    us = _alternate([fwd, both, efwd, eboth, kf, kb], reps, rounds)
    return dict(B=B, C=C, H=side, W=side, fwd_us=round(us[0], 1), bwd_us=round(us[1] - us[0], 1), kernel_fwd_us=round(us[4], 1),
                kernel_bwd_us=round(us[5], 1), eager_fwd_us=round(us[2], 1), eager_bwd_us=round(us[3] - us[2], 1), ratio=round(us[3] / us[1], 2),
                peak_mb=peak, eager_peak_mb=epeak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--sizes', type=int, nargs='+', default=[20, 40, 80])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('upsample_bench needs the MI355X')
    res = dict(batch=a.batch, channels=a.channels, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds)
    for kind in ('carafe', 'dysample'):
        res[kind] = [bench(kind, a.batch, a.channels, s, a.reps, a.rounds) for s in a.sizes]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
