"""Plain-torch restatements of the reference's other NMS rules (test infrastructure, CPU): the penalised greedy `NMS`
(utils/general.py:925-951 over utils/metrics.bbox_iou :490-579), `soft_nms` (:834-862 over box_iou_for_nms :868-892) and merge-NMS
(:698-704), in the reference's operation order and in whatever dtype the tensors have - fp32 for the bit / index comparisons, fp64 for
the anchored value bounds.  tests/golden/nms_variants.npz pins them to the reference's own functions (tests/test_nms_variants_host.py).

Every decision a rule takes can be recorded: pass `margins=dict()` and it receives, per kind of decision, the smallest distance from
flipping in units of the fp32 spacing of the compared quantity ('thr': metric against iou_thres, 'score': score against
score_threshold, 'gap': best against second-best live score at a Soft-NMS pick, 'merge': plain IoU of a kept box and a candidate
against iou_thres in merge-NMS).
"""
import math

import numpy as np
import torch

from oracle.somi_ref.nms import box_iou, greedy_nms, xywh2xyxy

PENALISED = ('GIoU', 'DIoU', 'CIoU', 'EIoU', 'SIoU')
MODES = ('iou',) + PENALISED + ('soft',)
MIN_MARGIN = 64.0                     # fp32 spacings every recorded decision must keep from flipping


def _spacings(a, b):
    """|a - b| in units of the fp32 spacing of the larger magnitude (elementwise, float64 numpy)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ref = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(np.float32).tiny).astype(np.float32)
    return np.abs(a - b) / np.spacing(ref).astype(np.float64)


def _note(margins, kind, a, b):
    if margins is None:
        return
    a = a.detach().double().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().double().numpy() if isinstance(b, torch.Tensor) else b
    s = _spacings(a, b)
    if s.size:
        margins[kind] = min(margins.get(kind, float('inf')), float(s.min()))


def _corners(box):
    return box[..., 0], box[..., 1], box[..., 2], box[..., 3]


def _overlap(p, q):
    """Intersection area and the enclosing box's width and height of p (4,) against q (n,4)."""
    px1, py1, px2, py2 = _corners(p)
    qx1, qy1, qx2, qy2 = _corners(q)
    inter = (torch.minimum(px2, qx2) - torch.maximum(px1, qx1)).clamp(0) * (torch.minimum(py2, qy2) - torch.maximum(py1, qy1)).clamp(0)
    return inter, torch.maximum(px2, qx2) - torch.minimum(px1, qx1), torch.maximum(py2, qy2) - torch.minimum(py1, qy1)


def _centre_offsets(p, q):
    """Twice the centre distance along x and y, in the reference's order of additions."""
    px1, py1, px2, py2 = _corners(p)
    qx1, qy1, qx2, qy2 = _corners(q)
    return qx1 + qx2 - px1 - px2, qy1 + qy2 - py1 - py2


def _aspect_term(wp, hp, wq, hq):
    return (4 / math.pi ** 2) * (torch.atan(wq / hq) - torch.atan(wp / hp)).pow(2)


def bbox_iou(box1, box2, mode, eps=1e-7):
    """utils/metrics.py bbox_iou(box1 (4,), box2 (n,4), x1y1x2y2=True, <mode>=True) at alpha = 1 -> (n,): `h + eps`, `union + eps`, then
    `inter / (union + eps)`; the pow(., alpha) steps are exact at alpha = 1 and are left out."""
    px1, py1, px2, py2 = _corners(box1)
    qx1, qy1, qx2, qy2 = _corners(box2)
    inter, cw, ch = _overlap(box1, box2)
    wp, hp = px2 - px1, py2 - py1 + eps
    wq, hq = qx2 - qx1, qy2 - qy1 + eps
    union = wp * hp + wq * hq - inter + eps
    iou = inter / (union + eps)
    if mode == 'GIoU':
        hull = cw * ch + eps
        return iou - ((hull - union) / hull + eps)
    diag2 = (cw ** 2 + ch ** 2) + eps
    ox, oy = _centre_offsets(box1, box2)
    dist2 = (ox ** 2 + oy ** 2) / 4
    if mode == 'DIoU':
        return iou - dist2 / diag2
    if mode == 'CIoU':
        v = _aspect_term(wp, hp, wq, hq)
        a = v / (v - iou + (1 + eps))
        return iou - (dist2 / diag2 + (v * a + eps))
    if mode == 'EIoU':
        dw2 = ((qx2 - qx1) - (px2 - px1)) ** 2
        dh2 = ((qy2 - qy1) - (py2 - py1)) ** 2
        return iou - (dist2 / diag2 + dw2 / (cw ** 2 + eps) + dh2 / (ch ** 2 + eps))
    assert mode == 'SIoU', mode
    sx, sy = ox * 0.5 + eps, oy * 0.5 + eps                        # centre offsets
    hyp = torch.pow(sx ** 2 + sy ** 2, 0.5)
    sin_x, sin_y = torch.abs(sx) / hyp, torch.abs(sy) / hyp
    sin_a = torch.where(sin_x > pow(2, 0.5) / 2, sin_y, sin_x)
    angle = torch.cos(torch.arcsin(sin_a) * 2 - math.pi / 2)
    g = angle - 2
    distance = 2 - torch.exp(g * (sx / cw) ** 2) - torch.exp(g * (sy / ch) ** 2)
    rel_w = torch.abs(wp - wq) / torch.max(wp, wq)
    rel_h = torch.abs(hp - hq) / torch.max(hp, hq)
    shape = torch.pow(1 - torch.exp(-1 * rel_w), 4) + torch.pow(1 - torch.exp(-1 * rel_h), 4)
    return iou - (0.5 * (distance + shape) + eps)


def box_iou_for_nms(box1, box2, eps=1e-7):
    """utils/general.py box_iou_for_nms(box1 (4,), box2 (n,4), CIoU=True) -> (n,): h clamped at eps, one `+ eps` on the union."""
    px1, py1, px2, py2 = _corners(box1)
    qx1, qy1, qx2, qy2 = _corners(box2)
    wp, hp = px2 - px1, (py2 - py1).clamp(eps)
    wq, hq = qx2 - qx1, (qy2 - qy1).clamp(eps)
    inter, cw, ch = _overlap(box1, box2)
    iou = inter / (wp * hp + wq * hq - inter + eps)
    diag2 = cw ** 2 + ch ** 2 + eps
    ox, oy = _centre_offsets(box1, box2)
    dist2 = (ox ** 2 + oy ** 2) / 4
    v = _aspect_term(wp, hp, wq, hq)
    a = v / (v - iou + (1 + eps))
    return iou - (dist2 / diag2 + v * a)


def penalised_nms(boxes, scores, iou_thres, mode, margins=None, max_det=None):
    """The reference's NMS(): indices kept, in stable descending-score order; candidate j goes iff !(metric(kept, j) <= iou_thres).
    max_det stops after that many picks (the first max_det picks do not depend on what follows them)."""
    order = torch.argsort(scores, descending=True, stable=True)
    keep = []
    while order.numel() > 0:
        i = order[0]
        keep.append(int(i))
        if order.numel() == 1 or (max_det is not None and len(keep) >= max_det):
            break
        m = bbox_iou(boxes[i], boxes[order[1:]], mode)
        _note(margins, 'thr', m[~torch.isnan(m)], float(np.float32(iou_thres)))
        order = order[1:][m <= iou_thres]
    return torch.tensor(keep, dtype=torch.long)


def soft_nms(boxes, scores, iou_thres=0.3, sigma=0.5, score_threshold=0.25, max_det=None, drop_last=False, margins=None):
    """Soft-NMS on candidates in the given order; `scores` is decayed in place; returns the picks in pick order.
    drop_last=True reproduces the reference's soft_nms exactly: its `while order.numel() > 1` loop leaves with one candidate in hand
    and drops it, and when exactly one other candidate is left its `(iou > thresh).nonzero()` runs on a 0-dim tensor, comes back empty
    and that candidate is not decayed.  The kept form (the product's) decays it like any other and keeps the last candidate."""
    n = scores.shape[0]
    live = torch.ones(n, dtype=torch.bool, device=scores.device)
    keep = []
    cur = 0
    while n:
        if drop_last and int(live.sum()) == 1:
            break
        keep.append(cur)
        live[cur] = False
        if (max_det is not None and len(keep) >= max_det) or not live.any():
            break
        idx = live.nonzero().view(-1)
        if not (drop_last and idx.numel() == 1):
            m = box_iou_for_nms(boxes[cur], boxes[idx])
            _note(margins, 'thr', m, float(np.float32(iou_thres)))
            hit = m > iou_thres
            scores[idx[hit]] *= torch.exp(-torch.pow(m[hit], 2) / sigma)
        s = scores[idx]
        _note(margins, 'score', s, float(np.float32(score_threshold)))
        ok = s > score_threshold
        live[idx[~ok]] = False
        idx, s = idx[ok], s[ok]
        if not idx.numel():
            break
        k = int(torch.argmax(s))                                   # first maximum: the lowest index on an exact tie
        if idx.numel() > 1:
            top = torch.topk(s, 2).values
            _note(margins, 'gap', top[0:1], top[1:2])
        cur = int(idx[k])
    return torch.tensor(keep, dtype=torch.long)


def merge_nms(x, boxes, scores, keep, iou_thres, redundant=True, margins=None):
    """general.py:698-704 on one image: x (n,6) rows, boxes the class-offset boxes, keep the indices already cut to max_det.
    Returns (rows of the kept boxes with merged coordinates, the per-row cluster sizes), both after the `redundant` filter."""
    iou = box_iou(boxes[keep], boxes)
    _note(margins, 'merge', iou[~torch.isnan(iou)], float(np.float32(iou_thres)))
    iou = iou > iou_thres
    weights = iou * scores[None]
    rows = x[keep].clone()
    rows[:, :4] = torch.mm(weights, x[:, :4]) / weights.sum(1, keepdim=True)
    size = iou.sum(1)
    if redundant:
        rows, size = rows[size > 1], size[size > 1]
    return rows, size


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, labels=(),
                        max_det=300, nms='iou', merge=False, sigma=0.5, score_threshold=0.25, dtype=None, margins=None, info=None):
    """utils/general.py:629-711 with the selection rule chosen by `nms` / `merge`.  Candidates are built in fp32 exactly as the oracle's
    non_max_suppression builds them and put in stable descending-score order (what torchvision.ops.nms and NMS() do inside, and what the
    product hands every rule); `dtype` (torch.float64) then switches the selection arithmetic.  info, if a list, receives per image a
    dict(n=candidates, xmax=max |coordinate| of the candidates' boxes, size=cluster sizes of the merged rows or None)."""
    assert nms in MODES and not (merge and nms == 'soft')
    nc = prediction.shape[2] - 5
    cand = prediction[..., 4] > conf_thres
    max_wh, max_nms = 4096, 30000
    multi_label &= nc > 1
    out = [torch.zeros((0, 6), dtype=dtype or torch.float32)] * prediction.shape[0]
    for xi, x in enumerate(prediction):
        x = x[cand[xi]]
        if labels and len(labels[xi]):
            l = labels[xi]
            v = torch.zeros((len(l), nc + 5))
            v[:, :4] = l[:, 1:5]
            v[:, 4] = 1.0
            v[range(len(l)), l[:, 0].long() + 5] = 1.0
            x = torch.cat((x, v), 0)
        rec = dict(n=0, size=None)
        if info is not None:
            info.append(rec)
        if not x.shape[0]:
            continue
        x[:, 5:] *= x[:, 4:5]
        box = xywh2xyxy(x[:, :4])
        if multi_label:
            i, j = (x[:, 5:] > conf_thres).nonzero(as_tuple=False).T
            x = torch.cat((box[i], x[i, j + 5, None], j[:, None].float()), 1)
        else:
            conf, j = x[:, 5:].max(1, keepdim=True)
            x = torch.cat((box, conf, j.float()), 1)[conf.view(-1) > conf_thres]
        if classes is not None:
            x = x[(x[:, 5:6] == torch.tensor(classes)).any(1)]
        n = rec['n'] = x.shape[0]
        if not n:
            continue
        rec['xmax'] = float(x[:, :4].abs().max())
        x = x[torch.argsort(x[:, 4], descending=True, stable=True)[:max_nms]]
        c = x[:, 5:6] * (0 if agnostic else max_wh)
        boxes = x[:, :4] + c                                       # fp32, like the product; exact in fp64 too
        if dtype is not None:
            x, boxes = x.to(dtype), boxes.to(dtype)
        scores = x[:, 4]                                           # a view: Soft-NMS decays the rows' scores
        if nms == 'iou':
            keep = greedy_nms(boxes, scores, iou_thres)
        elif nms == 'soft':
            keep = soft_nms(boxes, scores, iou_thres, sigma, score_threshold, max_det=max_det, margins=margins)
        else:
            keep = penalised_nms(boxes, scores, iou_thres, nms, margins=margins)
        keep = keep[:max_det]
        if merge and 1 < n < 3000:
            out[xi], rec['size'] = merge_nms(x, boxes, scores, keep, iou_thres, margins=margins)
        else:
            out[xi] = x[keep]
    return out


# ------------------------------------------------------------------------------------------------ differential inputs
def clustered_pred(seed, n=800, nc=4, live=(260, 800, 0, 1)):
    """(len(live), n, 5+nc) decoded predictions over clusters of near-duplicate boxes; image b has objectness > 0 on its first live[b] rows
    only (0: an image with no candidates, 1: a single candidate)."""
    g = torch.Generator().manual_seed(seed)
    B = len(live)
    pred = torch.zeros(B, n, 5 + nc)
    k = n // 4
    for b in range(B):
        centre = torch.rand(k, 2, generator=g) * 640
        size = torch.rand(k, 2, generator=g) * 60 + 8
        which = torch.randint(0, k, (n,), generator=g)
        pred[b, :, 0:2] = centre[which] + torch.randn(n, 2, generator=g) * 4
        pred[b, :, 2:4] = size[which] * (1 + 0.25 * torch.randn(n, 2, generator=g)).clamp(0.3, 2.0)
        pred[b, :live[b], 4] = torch.rand(live[b], generator=g) * 0.9 + 0.1
        pred[b, :, 5:] = torch.rand(n, nc, generator=g) * 0.95 + 0.05
    return pred


def case_labels(pred):
    """A-priori label rows [cls, x, y, w, h] (general.py:651-658) for image 0, none for the others."""
    lb = torch.tensor([[1., 300., 300., 40., 50.], [3., 100., 420., 24., 18.], [0., *pred[0, 5, :4].tolist()]])
    return [lb] + [torch.zeros(0, 5)] * (pred.shape[0] - 1)


# tag: (keywords, modes, merge, seed).  The seeds were searched on the CPU (tools/gen_nms_variants_golden.py --pipeline-seeds) so that
# every decision the fp32 restatement takes on clustered_pred(seed) keeps MIN_MARGIN fp32 spacings from flipping; the tests re-assert it.
# With conf_thres = 0.001 and multi_label image 1 has 3200 candidates (outside the merge window), image 0 has 1040 (inside).
PIPELINE_CASES = {
    'default': (dict(conf_thres=0.25, iou_thres=0.45), PENALISED + ('soft',), False, 1),
    'multi': (dict(conf_thres=0.3, iou_thres=0.6, multi_label=True), PENALISED + ('soft',), False, 3),
    'agnostic': (dict(conf_thres=0.3, iou_thres=0.5, agnostic=True), ('DIoU', 'CIoU', 'soft'), False, 1),
    'classes': (dict(conf_thres=0.2, iou_thres=0.45, classes=[0, 2], multi_label=True), ('GIoU', 'SIoU', 'soft'), False, 3),
    # the label rows all score exactly 1.0: an exact tie, which Soft-NMS's margin condition excludes, so the greedy rules only
    'labels': (dict(conf_thres=0.3, iou_thres=0.5, labels=True, multi_label=True), ('EIoU', 'CIoU'), False, 1),
    'maxdet': (dict(conf_thres=0.05, iou_thres=0.9, multi_label=True, max_det=15), ('DIoU', 'SIoU', 'soft'), False, 1),
    'soft_params': (dict(conf_thres=0.2, iou_thres=0.3, sigma=0.3, score_threshold=0.4), ('soft',), False, 1),
    'merge': (dict(conf_thres=0.001, iou_thres=0.6, multi_label=True), ('iou', 'DIoU', 'CIoU'), True, 2),
    'merge_default': (dict(conf_thres=0.25, iou_thres=0.45), ('iou', 'GIoU', 'SIoU'), True, 1),
}


def run_case(tag, mode, seed=None, dtype=None, margins=None, info=None):
    """The restatement on one (case, mode); -> (prediction tensor, keywords for the product's call, list of output rows)."""
    kw, _, merge, s = PIPELINE_CASES[tag]
    pred = clustered_pred(s if seed is None else seed)
    kw = dict(kw)
    if kw.get('labels'):
        kw['labels'] = case_labels(pred)
    out = non_max_suppression(pred.clone(), nms=mode, merge=merge, dtype=dtype, margins=margins, info=info, **kw)
    return pred, dict(kw, nms=mode, merge=merge), out
