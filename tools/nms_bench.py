#!/usr/bin/env python3
"""Measurement of the NMS selection rules (nms.hip) on the MI355X at the SOMI head's shape: batch 32, 136000 predictions, 10 classes.

Prints ONE JSON line.  Per setting (`val`: conf 0.001 / iou 0.6 / multi_label, the val.sh thresholds; `default`: conf 0.25 / iou 0.45) and per
`window`: the default thresholds on the same predictions with objectness zeroed behind the first rows, so that every image has about 2500
candidates and merge-NMS, which only runs for 1 < candidates < 3000, does run) and per
mode ('iou', the five penalised rules, 'soft', and merge on 'iou' and 'CIoU'): the whole non_max_suppression_raw call in microseconds (device
events around `--reps` launches after a warm-up, median of `--rounds` rounds, the modes taking turns inside every round), and its ratio to
'iou' measured in the same process.  For 'soft' and the merge rows also the selection step alone in eager PyTorch on the same GPU (the
restatement of tests/nms_variants_ref.py, given the candidates already sorted) on `--eager-images` images, scaled to the batch, and
`vs_eager` = that over the product's whole call.  `forward_ms` is the eval forward of the flagship graph at the same batch, for scale.

Predictions are synthetic: clustered boxes (about `--per` near-duplicates per object) with objectness**2-distributed scores, so that the
`val` setting reaches the 30000-candidate cap on every image and the `default` setting keeps a few thousand.

    python tools/nms_bench.py [--batch 32] [--n 136000] [--nc 10] [--reps 20] [--rounds 5] [--no-forward]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'yolo-somi_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

SETTINGS = dict(val=dict(conf_thres=0.001, iou_thres=0.6, multi_label=True), default=dict(conf_thres=0.25, iou_thres=0.45))
ROWS = [('iou', False), ('GIoU', False), ('DIoU', False), ('CIoU', False), ('EIoU', False), ('SIoU', False), ('soft', False),
        ('iou', True), ('CIoU', True)]


def synthetic_pred(B, n, nc, per, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device='cuda')                                    # noqa: E731
    k = max(1, n // per)
    which = torch.randint(0, k, (B, n), generator=g, device='cuda')
    centre, size = r(B, k, 2) * 640, r(B, k, 2) * 60 + 6
    pred = torch.empty(B, n, 5 + nc, device='cuda')
    pred[..., 0:2] = torch.gather(centre, 1, which[..., None].expand(-1, -1, 2)) + (r(B, n, 2) - 0.5) * 8
    pred[..., 2:4] = torch.gather(size, 1, which[..., None].expand(-1, -1, 2)) * (0.7 + 0.6 * r(B, n, 2))
    pred[..., 4] = r(B, n) ** 2
    pred[..., 5:] = r(B, n, nc) ** 2
    return pred


def _events_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _alternate(fns, reps, rounds):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(_events_us(fn, reps))
    return [statistics.median(g) for g in got]


def eager_selection_us(pred, kw, mode, merge, images):
    """The selection step of the restatement in eager PyTorch on the GPU (candidates and their order given), microseconds per image."""
    import nms_variants_ref as R
    iou_thres = kw['iou_thres']
    total = 0.0                                                   # the candidates are rebuilt with torch ops outside the timed region
    for b in range(images):
        x = pred[b]
        x = x[x[:, 4] > kw['conf_thres']]
        conf = x[:, 5:] * x[:, 4:5]
        box = torch.cat((x[:, :2] - x[:, 2:4] / 2, x[:, :2] + x[:, 2:4] / 2), 1)
        if kw.get('multi_label'):
            i, j = (conf > kw['conf_thres']).nonzero(as_tuple=False).T
            x = torch.cat((box[i], conf[i, j, None], j[:, None].float()), 1)
        else:
            c, j = conf.max(1, keepdim=True)
            x = torch.cat((box, c, j.float()), 1)[c.view(-1) > kw['conf_thres']]
        x = x[torch.argsort(x[:, 4], descending=True, stable=True)[:30000]]
        boxes, scores = x[:, :4] + x[:, 5:6] * 4096, x[:, 4].clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == 'soft':
            R.soft_nms(boxes, scores, iou_thres, 0.5, 0.25, max_det=300)
        else:
            keep = R.penalised_nms(boxes, scores, iou_thres, mode, max_det=300) if mode != 'iou' else _eager_greedy(boxes, iou_thres)
            if merge and 1 < x.shape[0] < 3000:
                R.merge_nms(x, boxes, scores, keep.to(x.device), iou_thres)
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total / images * 1e6


def _eager_greedy(boxes, iou_thres):
    """Plain greedy NMS as the loop the reference's NMS() runs, with box_iou as the overlap (sorted input)."""
    import nms_variants_ref as R
    order = torch.arange(boxes.shape[0], device=boxes.device)
    keep = []
    while order.numel() > 0 and len(keep) < 300:
        keep.append(int(order[0]))
        if order.numel() == 1:
            break
        iou = R.box_iou(boxes[order[:1]], boxes[order[1:]])[0]
        order = order[1:][~(iou > iou_thres)]
    return torch.tensor(keep, dtype=torch.long)


def forward_ms(batch, steps=3, warmup=2):
    from somi_amd.configs import fill_state, somi_cfg, synthetic_batch, SOMI_ANCHORS
    from somi_amd.model import Model
    model = fill_state(Model(somi_cfg(1.0, 1.0, anchors=SOMI_ANCHORS, dcn=True)), 1).cuda().eval()
    imgs, _ = synthetic_batch(batch, 640, seed=0)
    imgs = imgs.cuda()
    with torch.no_grad():
        for _ in range(warmup):
            model(imgs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model(imgs)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--n', type=int, default=136000)
    ap.add_argument('--nc', type=int, default=10)
    ap.add_argument('--per', type=int, default=40, help='predictions per synthetic object')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--eager-images', type=int, default=2)
    ap.add_argument('--no-forward', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nms_bench needs the MI355X')
    from somi_amd.nms import non_max_suppression_raw
    pred = synthetic_pred(a.batch, a.n, a.nc, a.per)
    res = dict(batch=a.batch, n=a.n, nc=a.nc, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0))
    best = (pred[..., 5:] * pred[..., 4:5]).amax(2)
    share = (best > SETTINGS['default']['conf_thres']).float().mean().item()
    windowed = pred.clone()
    windowed[:, int(2500 / max(share, 1e-6)):, 4] = 0               # about 2500 candidates per image: inside the merge size window
    for name, kw in list(SETTINGS.items()) + [('window', SETTINGS['default'])]:
        if name == 'window':
            pred = windowed
        cand = (pred[..., 5:] * pred[..., 4:5] > kw['conf_thres']).sum((1, 2)) if kw.get('multi_label') else \
            ((pred[..., 5:] * pred[..., 4:5]).amax(2) > kw['conf_thres']).sum(1)
        fns = [lambda m=m, mg=mg: non_max_suppression_raw(pred, nms=m, merge=mg, **kw) for m, mg in ROWS]
        us = _alternate(fns, a.reps, a.rounds)
        _, count = non_max_suppression_raw(pred, **kw)
        rows = {}
        for (m, mg), t in zip(ROWS, us):
            row = dict(us=round(t, 1), vs_iou=round(t / us[0], 3))
            if m == 'soft' or mg:
                e = eager_selection_us(pred, kw, m, mg, a.eager_images) * a.batch
                row.update(eager_selection_us=round(e, 1), vs_eager=round(e / t, 2))
            rows[m + ('+merge' if mg else '')] = row
        res[name] = dict(candidates_mean=round(cand.float().mean().item(), 1), candidates_max=int(cand.max()), kept_mean=round(count.float().mean().item(), 1), modes=rows)
    if not a.no_forward:
        res['forward_ms'] = round(forward_ms(a.batch), 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
