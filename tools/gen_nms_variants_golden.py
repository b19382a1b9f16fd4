#!/usr/bin/env python3
"""Writes tests/golden/nms_variants.npz: the reference's own `NMS`, `soft_nms` and merge-NMS (utils/general.py:925-951, :834-862, :698-704)
on fixed clustered boxes, run through oracle.gen_golden's stub harness (importing it makes the reference importable and installs the
restated greedy core as torchvision.ops.nms).  The `merge = True` form of non_max_suppression is obtained by substituting that one
assignment (:643) in the function's source at generation time and exec-ing it in the reference module's namespace; nothing of that
source is written anywhere.  The fixture holds data only: inputs, kept indices, output rows, decayed scores and, per case, the smallest
distance of any decision the reference takes from flipping, in fp32 spacings of the compared quantity (tests/nms_variants_ref.py
records them while it retraces the reference's run; the generator first checks that it does retrace it, index for index and score for
score).  Seeds are searched until every distance is at least MIN_MARGIN spacings, and inputs hold no exact score ties (the reference's
argsort is not stable).  tests/test_nms_variants_host.py and tests/test_nms_variants_gpu.py read the file.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_nms_variants_golden.py
"""
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402
import nms_variants_ref as R  # noqa: E402

RG = G.RG


def clustered_boxes(n, seed, extent=640.0, per=6):
    """n xyxy boxes in clusters of about `per` near-duplicates, and n distinct scores."""
    g = torch.Generator().manual_seed(seed)
    k = max(1, n // per)
    centre = torch.rand(k, 2, generator=g) * extent
    size = torch.rand(k, 2, generator=g) * 60 + 8
    which = torch.randint(0, k, (n,), generator=g)
    c = centre[which] + torch.randn(n, 2, generator=g) * 4
    wh = size[which] * (1 + 0.25 * torch.randn(n, 2, generator=g)).clamp(0.3, 2.0)
    boxes = torch.cat((c - wh / 2, c + wh / 2), 1)
    scores = torch.rand(n, generator=g) * 0.98 + 0.01
    assert scores.unique().numel() == n
    return boxes, scores


def clustered_pred(B, n, nc, seed, live_rows):
    """(B, n, 5+nc) decoded predictions over clustered boxes; image b has objectness > 0 on its first live_rows[b] rows only."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.zeros(B, n, 5 + nc)
    for b in range(B):
        boxes, _ = clustered_boxes(n, seed * 7 + b, per=4)
        pred[b, :, 0:2] = (boxes[:, :2] + boxes[:, 2:]) / 2
        pred[b, :, 2:4] = boxes[:, 2:] - boxes[:, :2]
        pred[b, :live_rows[b], 4] = torch.rand(live_rows[b], generator=g) * 0.9 + 0.1
        pred[b, :, 5:] = torch.rand(n, nc, generator=g)
    return pred


def reference_merge_nms():
    """The reference's non_max_suppression with its `merge = False` assignment (:643) turned on."""
    src = inspect.getsource(RG.non_max_suppression)
    assert src.count('merge = False') == 1
    ns = {}
    exec(compile(src.replace('merge = False', 'merge = True'), '<reference non_max_suppression, merge on>', 'exec'), vars(RG), ns)
    return ns['non_max_suppression']


def search(make, what):
    for seed in range(1000, 1200):
        rec, margins = make(seed)
        if rec is not None and min(margins.values()) >= R.MIN_MARGIN:
            print(f'{what}: seed {seed}, margins ' + ', '.join(f'{k} {v:.0f}' for k, v in margins.items()))
            return rec, seed
    raise SystemExit(f'{what}: no seed met the margin condition')


def main():
    rec = {}
    thr = 0.45

    def nms_case(seed):
        boxes, scores = clustered_boxes(600, seed)
        out, margins = dict(nms_boxes=boxes, nms_scores=scores, nms_thr=thr), {}
        for mode in R.PENALISED:
            keep = RG.NMS(boxes, scores, thr, class_nms=mode)
            m = {}
            assert torch.equal(R.penalised_nms(boxes, scores, thr, mode, margins=m), keep), mode
            out[f'nms_keep_{mode}'] = keep
            out[f'nms_margin_{mode}'] = m['thr']
            margins[mode] = m['thr']
        return out, margins
    r, _ = search(nms_case, 'NMS')
    rec.update(r)

    for tag, n, kw in (('soft_a', 300, dict(iou_thresh=0.3, sigma=0.5, score_threshold=0.25)),
                       ('soft_b', 200, dict(iou_thresh=0.45, sigma=0.3, score_threshold=0.1))):
        def soft_case(seed, n=n, kw=kw):
            boxes, scores = clustered_boxes(n, seed)
            order = torch.argsort(scores, descending=True)
            boxes, scores = boxes[order].contiguous(), scores[order].contiguous()
            s_ref, s_mine, m = scores.clone(), scores.clone(), {}
            keep = RG.soft_nms(boxes, s_ref, **kw)
            mine = R.soft_nms(boxes, s_mine, kw['iou_thresh'], kw['sigma'], kw['score_threshold'], drop_last=True, margins=m)
            assert torch.equal(mine, keep) and torch.equal(s_mine, s_ref), 'the restatement does not retrace the reference'
            if set(m) != {'thr', 'score', 'gap'}:
                return None, None
            out = {f'{tag}_boxes': boxes, f'{tag}_scores': scores, f'{tag}_keep': keep, f'{tag}_decayed': s_ref,
                   f'{tag}_params': torch.tensor([kw['iou_thresh'], kw['sigma'], kw['score_threshold']], dtype=torch.float64),
                   f'{tag}_margins': torch.tensor([m['thr'], m['score'], m['gap']], dtype=torch.float64)}
            return out, m
        r, _ = search(soft_case, tag)
        rec.update(r)

    merge_nms = reference_merge_nms()
    mkw = dict(conf_thres=0.02, iou_thres=0.5, multi_label=True)

    def merge_case(seed):
        pred = clustered_pred(2, 1200, 3, seed, live_rows=(420, 1200))
        out = merge_nms(pred.clone(), **mkw)
        info = []
        mine = R.non_max_suppression(pred.clone(), merge=True, info=info, **mkw)
        if not (1 < info[0]['n'] < 3000 <= info[1]['n']):
            return None, None
        for a, b in zip(mine, out):
            assert a.shape == b.shape and torch.equal(a[:, 4:], b[:, 4:]) and torch.allclose(a, b, rtol=1e-5, atol=1e-3)
        m = {}
        R.non_max_suppression(pred.clone(), merge=True, margins=m, **mkw)      # the merge decisions: plain IoU against the threshold
        rec_ = dict(merge_pred=pred, merge_out0=out[0], merge_out1=out[1], merge_margin=m['merge'],
                    merge_n=torch.tensor([info[0]['n'], info[1]['n']]))
        return rec_, m
    r, _ = search(merge_case, 'merge')
    rec.update(r)
    G.save('nms_variants', **rec)


def pipeline_seeds():
    """Searches, per case of nms_variants_ref.PIPELINE_CASES, the first seed whose clustered_pred meets the margin condition under every
    mode the case runs (fp32 restatement on the CPU), and prints the table to paste there."""
    only = [a for a in sys.argv[1:] if not a.startswith('--')]
    for tag, (kw, modes, merge, _) in R.PIPELINE_CASES.items():
        if only and tag not in only:
            continue
        for seed in range(1, 400):
            worst = float('inf')
            for mode in modes:
                m = {}
                R.run_case(tag, mode, seed=seed, margins=m)
                worst = min([worst] + list(m.values()))
                if worst < R.MIN_MARGIN:
                    break
            if worst >= R.MIN_MARGIN:
                print(f'{tag!r}: seed {seed} (smallest margin {worst:.0f} spacings)')
                break
        else:
            raise SystemExit(f'{tag}: no seed met the margin condition')


if __name__ == '__main__':
    pipeline_seeds() if '--pipeline-seeds' in sys.argv[1:] else main()
