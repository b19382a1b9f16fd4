#!/usr/bin/env python3
"""Measurement of ACmix (acmix.hip, blocks.ACmix) on the MI355X.

Prints ONE JSON line.  Cases, batch `--batch` (32): the two rows of configs.yolov5_acmix_cfg at 640 x 640 and width 0.5, i.e. ACmix(512, 512) on
the 20x20 map ('row') and ACmix(128, 128) on the 80x80 map ('p3').  Per case:
  kernels   attn / bwd_q (with its three small reduction launches) / bwd_kv / conv / conv_bwd_data / conv_bwd_weight (with its fold) / proj (the
            stacked 1x1 conv c1 -> 3 c2): *_us; for the three attention kernels *_gflops from 196 C flop per pixel forward (two products per tap,
            head dim and multiply-add), 392 C for bwd_q (three window products and the score recompute) and 392 C for bwd_kv.
  block     training fwd_us and bwd_us as (forward + backward) - forward, infer_us the eval forward, against the tests' restatement
            (tests/acmix_ref.py: the literal formula with unfold) run eagerly on the same GPU in the same process (eager_*), the two sides taking
            turns inside every round; ratio = eager (forward + backward) / ours, infer_ratio = eager / ours; *_peak_mib =
            torch.cuda.max_memory_allocated over a training forward + backward of that side, above what was allocated before it.
Device events around `reps` calls after a warm-up, median and (min, max) of `--rounds` rounds.  If eager runs out of memory at the batch, the
batch is halved for BOTH sides and the line says so (batch_used).

    python tools/acmix_bench.py [--batch 32] [--reps 3] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

CASES = (('row', 512, 20), ('p3', 128, 80))


def _events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _alternate(fns, reps, rounds, warm=2):
    """(median, min, max) microseconds of each function over `rounds` rounds, the functions taking turns inside every round."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(_events_us(fn, reps))
    return [(statistics.median(g), min(g), max(g)) for g in got]


def _r1(v):
    return round(v, 1)


def bench_kernels(C, S, B, reps, rounds):
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight
    g = torch.Generator(device='cuda').manual_seed(1)
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)    # noqa: E731
    x, qkv, dout, dqkv = r(B, S, S, C), r(B, S, S, 3 * C), r(B, S, S, C), torch.empty(B, S, S, 3 * C, device='cuda')
    wp, fc, dep, bias = 0.5 * r(C // 4, 2), r(9, 12) / 3.5, r(C, 9, 3, 3) / 3, 0.1 * r(C)
    r1, r2 = torch.full((1,), 0.5, device='cuda'), torch.full((1,), 0.5, device='cuda')
    w, b = pack_conv_weight(r(3 * C, C, 1, 1) / C ** 0.5), 0.1 * r(3 * C)
    weff = ops.acmix_fold_weff(fc, dep, C)
    mix = ops.acmix_conv(qkv, C, weff, bias)
    out, lse = ops.acmix_attn(qkv, C, wp, r1, r2, mix=mix, want_lse=True)
    _, aux, _, _ = ops.acmix_attn_backward_q(dout, qkv, C, wp, r1, r2, lse, mix=mix, dq=dqkv)
    fns = dict(attn=lambda: ops.acmix_attn(qkv, C, wp, r1, r2, mix=mix, out=out, lse=lse),
               bwd_q=lambda: ops.acmix_attn_backward_q(dout, qkv, C, wp, r1, r2, lse, mix=mix, dq=dqkv, aux=aux),
               bwd_kv=lambda: ops.acmix_attn_backward_kv(dout, qkv, C, wp, r1, r2, lse, aux, dk=dqkv, dk_coff=C, dv=dqkv, dv_coff=2 * C),
               conv=lambda: ops.acmix_conv(qkv, C, weff, bias, out=mix),
               conv_bwd_data=lambda: ops.acmix_conv_backward_data(dout, C, weff, r2, dqkv),
               conv_bwd_weight=lambda: ops.acmix_split_dweff(ops.acmix_conv_backward_weight(dout, qkv, C, r2)[0], fc, dep, C),
               proj=lambda: ops.conv2d_nhwc(x, w, b, kh=1, kw=1, cin=C, cout=3 * C, out=qkv))
    res = {}
    flop = dict(attn=196, bwd_q=392, bwd_kv=392)
    for (name, _), (med, lo, hi) in zip(fns.items(), _alternate(list(fns.values()), reps, rounds)):
        res[name + '_us'] = [_r1(med), _r1(lo), _r1(hi)]
        if name in flop:
            res[name + '_gflops'] = round(flop[name] * C * B * S * S / med / 1e3)
    return res


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20)


def bench_block(C, S, B, reps, rounds):
    import acmix_ref as R
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref = fill_state(R.ACmix(C, C), 5)
    with torch.no_grad():
        ref.rate1.fill_(0.5)
        ref.rate2.fill_(0.5)
    mine = MB.ACmix(C, C)
    mine.load_state_dict(ref.state_dict())
    ref, mine = ref.cuda(), mine.cuda()
    g = torch.Generator(device='cuda').manual_seed(2)
    x, dy = torch.randn(B, S, S, C, device='cuda', generator=g), torch.randn(B, S, S, C, device='cuda', generator=g)
    xe, dye = x.permute(0, 3, 1, 2).contiguous(), dy.permute(0, 3, 1, 2).contiguous()

    def ours_fb():
        mine(Act(x))
        mine.backward(Act(dy))

    def eager_fb():
        xg = xe.detach().requires_grad_(True)
        ref(xg).backward(dye)
        for p in ref.parameters():
            p.grad = None

    def ours_inf():
        with torch.no_grad():
            mine(Act(x))

    def eager_inf():
        with torch.no_grad():
            ref(xe)

    res = {}
    mine.train(), ref.train()
    res['peak_mib'], res['eager_peak_mib'] = _peak_mib(ours_fb), _peak_mib(eager_fb)
    (fb, e_fb, f, e_f) = _alternate([ours_fb, eager_fb, lambda: mine(Act(x)), lambda: ref(xe)], reps, rounds, warm=1)
    mine.eval(), ref.eval()
    (inf, e_inf) = _alternate([ours_inf, eager_inf], reps, rounds, warm=1)
    res.update(fwd_us=_r1(f[0]), bwd_us=_r1(fb[0] - f[0]), fwd_bwd_us=[_r1(v) for v in fb], eager_fwd_us=_r1(e_f[0]), eager_bwd_us=_r1(e_fb[0] - e_f[0]),
               eager_fwd_bwd_us=[_r1(v) for v in e_fb], ratio=round(e_fb[0] / fb[0], 2), infer_us=[_r1(v) for v in inf],
               eager_infer_us=[_r1(v) for v in e_inf], infer_ratio=round(e_inf[0] / inf[0], 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    out = dict(tool='acmix_bench', device=torch.cuda.get_device_name(0), batch=a.batch, reps=a.reps, rounds=a.rounds, cases={})
    for where, C, S in CASES:
        B = a.batch
        while True:
            try:
                rec = dict(C=C, S=S, batch_used=B, kernels=bench_kernels(C, S, B, a.reps, a.rounds), block=bench_block(C, S, B, a.reps, a.rounds))
                break
            except torch.OutOfMemoryError:
                if B == 1:
                    raise
                B //= 2                                           # for BOTH sides
                torch.cuda.empty_cache()
        out['cases'][where] = rec
    print(json.dumps(out))


if __name__ == '__main__':
    main()
