#!/usr/bin/env python3
"""Measurement of the Swin blocks (swin.hip, blocks.SwinTransformerBlock / blocks.C3STR) on the MI355X.

Prints ONE JSON line.  Cases, batch `--batch` (32), training mode: SwinTransformerBlock(256, 256, 8, 2) at 20x20 (padded to 24x24) and at
40x40, C3STR(512, 512, 2) at 20x20.  Per case:
  fwd_us / bwd_us               the whole block: forward, and backward as (forward + backward) - forward
  eager_fwd_us / eager_bwd_us   the tests' restatement of the reference (tests/swin_ref.py: roll, pad, window partition, bias gather, mask add,
                                softmax, two matmuls) run eagerly on the same GPU in the same process, autograd for the backward
  ratio                         eager (forward + backward) / ours (forward + backward)
  attn_fwd_us / attn_bwd_us     the attention kernels alone on the block's qkv tensor (layer 1: shifted), with attn_fwd_gbs / attn_bwd_gbs = their
                                algorithmic traffic per second: forward 4C floats per real token (3C read, C written), backward 3C + C read and 3C
                                written per token plus the log-sum-exp
  qkv_attn_us / eager_qkv_attn_us   the part the kernel replaces, qkv Linear included on both sides: ours = 1x1 conv on the map + the kernel; eager =
                                pad, roll, partition, Linear, scores + bias + mask, softmax, P v, window reverse, roll back, crop (forward only)
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds; the sides take turns inside every round.

    python tools/swin_bench.py [--batch 32] [--reps 10] [--rounds 7]
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


def _eager_qkv_attn(layer, n):
    """swin_ref.SwinTransformerLayer.forward between norm1 and the residual add, without proj: n is the normalised map in the layer's frame."""
    import swin_ref as R
    ws, sh = layer.window_size, layer.shift_size
    B, A1, A2, C = n.shape
    P1, P2 = -(-A1 // ws) * ws, -(-A2 // ws) * ws
    n = F.pad(n, (0, 0, 0, P2 - A2, 0, P1 - A1))
    mask = None
    if sh > 0:
        n = torch.roll(n, (-sh, -sh), (1, 2))
        mask = R.shift_mask(P1, P2, ws, sh).to(n.device)
    w = R.to_windows(n, ws)
    at = layer.attn
    n_, N, h = w.shape[0], w.shape[1], at.num_heads
    q, k, v = at.qkv(w).view(n_, N, 3, h, C // h).permute(2, 0, 3, 1, 4)
    s = (q * at.scale) @ k.transpose(-2, -1)
    s = s + at.relative_position_bias_table[at.relative_position_index.view(-1)].view(N, N, h).permute(2, 0, 1)
    if mask is not None:
        s = (s.view(-1, mask.shape[0], h, N, N) + mask[None, :, None]).view(-1, h, N, N)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(n_, N, C)
    o = R.from_windows(o, B, P1, P2, ws)
    if sh > 0:
        o = torch.roll(o, (sh, sh), (1, 2))
    return o[:, :A1, :A2].contiguous()


def bench(name, make, B, C, side, reps, rounds):
    import swin_ref as R
    from somi_amd import blocks as MB
    from somi_amd import ops
    from somi_amd.blocks import Act
    gen = torch.Generator().manual_seed(side + C)
    x = torch.randn(B, side, side, C, generator=gen).cuda()
    dy = torch.randn(B, side, side, C, generator=gen).cuda()
    mine, eager = make(MB).cuda().train(), make(R).cuda().train()
    xe = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    dye = dy.permute(0, 3, 1, 2).contiguous()

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
    # the attention alone, on the shifted layer's shapes
    lay = (mine.m if hasattr(mine, 'm') else mine).tr[1]
    elay = (eager.m if hasattr(eager, 'm') else eager).tr[1]
    c, heads = lay.attn.dim, lay.attn.num_heads
    n1 = torch.randn(B, side, side, c, generator=gen).cuda()
    pk = lay.attn._packed(n1.device)
    ids = lay._region_ids(side, side, n1.device)
    qkv = ops.conv2d_nhwc(n1, pk['wqkv'], None, kh=1, kw=1)
    do = torch.randn(B, side, side, c, generator=gen).cuda()
    _, lse = ops.window_attention(qkv, pk['table'], heads, 4, ids, lse=True)
    gt = torch.zeros(225, heads, device='cuda')
    ne = n1.permute(0, 2, 1, 3).contiguous()

    def kf():
        ops.window_attention(qkv, pk['table'], heads, 4, ids, lse=True)

    def kb():
        ops.window_attention_backward(qkv, pk['table'], do, lse, heads, 4, ids, dtable=gt)

    def qa():
        ops.window_attention(ops.conv2d_nhwc(n1, pk['wqkv'], None, kh=1, kw=1), pk['table'], heads, 4, ids)

    def eqa():
        with torch.no_grad():
            _eager_qkv_attn(elay, ne)
    us = _alternate([fwd, both, efwd, eboth, kf, kb, qa, eqa], reps, rounds)
    med = [u[0] for u in us]
    tokens = B * side * side
    nwin = B * (-(-side // 8)) ** 2
    fwd_bytes = 4.0 * tokens * 4 * c
    bwd_bytes = 4.0 * tokens * 7 * c + 4.0 * nwin * heads * 64
    r1 = lambda v: round(v, 1)                                   # noqa: E731
    return dict(case=name, B=B, C=C, H=side, W=side, attn_C=c, heads=heads, fwd_us=r1(med[0]), bwd_us=r1(med[1] - med[0]),
                eager_fwd_us=r1(med[2]), eager_bwd_us=r1(med[3] - med[2]), ratio=round(med[3] / med[1], 2),
                fwd_bwd_us_spread=[r1(us[1][1]), r1(us[1][2])], eager_fwd_bwd_us_spread=[r1(us[3][1]), r1(us[3][2])],
                attn_fwd_us=r1(med[4]), attn_bwd_us=r1(med[5]), attn_fwd_us_spread=[r1(us[4][1]), r1(us[4][2])],
                attn_bwd_us_spread=[r1(us[5][1]), r1(us[5][2])], attn_fwd_gbs=r1(fwd_bytes / med[4] * 1e-3), attn_bwd_gbs=r1(bwd_bytes / med[5] * 1e-3),
                qkv_attn_us=r1(med[6]), eager_qkv_attn_us=r1(med[7]), qkv_attn_ratio=round(med[7] / med[6], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('swin_bench needs the MI355X')
    cases = [('swinblock_256_20', lambda M: M.SwinTransformerBlock(256, 256, 8, 2), 256, 20),
             ('swinblock_256_40', lambda M: M.SwinTransformerBlock(256, 256, 8, 2), 256, 40),
             ('c3str_512_20', lambda M: M.C3STR(512, 512, 2), 512, 20)]
    res = dict(batch=a.batch, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds,
               cases=[bench(n, mk, a.batch, c, s, a.reps, a.rounds) for n, mk, c, s in cases])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
