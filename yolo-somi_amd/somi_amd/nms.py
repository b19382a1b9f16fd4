"""`non_max_suppression` with the reference's signature (utils/general.py:629-630), executed by somi_nms_f32.

Returns a list of (n_i, 6) [x1, y1, x2, y2, conf, cls] tensors on the prediction's device.  One device->host copy of
the per-image counts happens at the end (the reference syncs per image inside its Python loop, and val.py:189 copies
results to the CPU anyway).  `labels` (a-priori boxes for autolabelling, :651-658) are appended as rows of the prediction tensor.

The reference's other selection rules are keyword-only arguments behind `max_det` (somi_nms_ex_f32):
  nms='iou'                  the default, torchvision.ops.nms (:694): the call above, unchanged.
  nms='GIoU'|'DIoU'|'CIoU'|'EIoU'|'SIoU'   the reference's `NMS(boxes, scores, iou_thres, class_nms)` (:925-951) in place of :694.
  nms='soft'                 `soft_nms(boxes, scores, iou_thres, sigma, score_threshold)` (:834-862, the commented line :695) on the
                             score-sorted candidates; output rows carry the decayed scores.
  merge=True                 merge-NMS (:643, :698-704) with `redundant`; not with nms='soft'.
Two deliberate deviations: an unknown `nms` name raises ValueError (the reference's NMS() silently runs SIoU), and Soft-NMS keeps the
last remaining candidate (the reference's `while order.numel() > 1` loop leaves with it in hand and drops it, so an image with a single
detection comes back empty there).  An exact score tie between live Soft-NMS candidates goes to the lowest index.
`NMS` and `soft_nms` are the standalone functions on boxes and scores (somi_nms_boxes_f32).
"""
import torch

from . import _lib
from ._lib import check
from .ops import _ptr, _stream


MODES = {'iou': 0, 'GIoU': 1, 'DIoU': 2, 'CIoU': 3, 'EIoU': 4, 'SIoU': 5, 'soft': 6}          # SOMI_NMS_* of include/somi_hip.h
MAX_BOXES = 30000                                                                            # standalone forms: the pipeline's max_nms


def _mode(nms, merge=False):
    if nms not in MODES:
        raise ValueError(f'unknown NMS mode {nms!r}: expected one of {", ".join(MODES)}')
    if merge and nms == 'soft':
        raise NotImplementedError("merge=True is not available with nms='soft': merge-NMS averages the candidates a greedy rule "
                                  'suppresses, and Soft-NMS suppresses none')
    return MODES[nms]


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                        labels=(), max_det=300, *, nms='iou', merge=False, sigma=0.5, score_threshold=0.25):
    det, count = non_max_suppression_raw(prediction, conf_thres, iou_thres, classes, agnostic, multi_label, labels, max_det,
                                         nms=nms, merge=merge, sigma=sigma, score_threshold=score_threshold)
    counts = count.cpu().tolist()
    return [det[b, :counts[b]] for b in range(det.shape[0])]


def non_max_suppression_raw(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                            labels=(), max_det=300, *, nms='iou', merge=False, sigma=0.5, score_threshold=0.25):
    """Same selection, left on the device: det (B, max_det, 6) and count (B) int32 - no host synchronisation, so a following device
    step (wbf.weighted_boxes_fusion_batch) can consume them stream-ordered."""
    assert 0 <= conf_thres <= 1, f'Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0'
    assert 0 <= iou_thres <= 1, f'Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0'
    mode = _mode(nms, merge)
    if not prediction.is_cuda:
        raise RuntimeError('somi_amd NMS runs on the MI355X only (no CPU fallback)')
    if prediction.dtype != torch.float32 or not prediction.is_contiguous():
        raise RuntimeError('prediction tensor has to be contiguous float32')
    B, n, no = prediction.shape
    nc = no - 5
    if labels and any(len(l) for l in labels):
        # a-priori labels (utils/general.py:651-658): each image's label rows [cls, x, y, w, h] become predictions with objectness 1 and a
        # one-hot class, appended BEHIND the image's own rows (the candidate order the reference builds); padding rows have
        # objectness 0 and drop out at the first threshold
        kmax = max(len(l) for l in labels)
        aug = torch.zeros(B, n + kmax, no, dtype=torch.float32, device=prediction.device)
        aug[:, :n] = prediction
        for xi, l in enumerate(labels):
            if len(l):
                l = torch.as_tensor(l, dtype=torch.float32, device=prediction.device)
                aug[xi, n:n + len(l), :4] = l[:, 1:5]
                aug[xi, n:n + len(l), 4] = 1.0
                aug[xi, torch.arange(n, n + len(l), device=prediction.device), l[:, 0].long() + 5] = 1.0
        prediction, n = aug, n + kmax
    ml = bool(multi_label) and nc > 1
    mask = None                                                  # NULL: keep every class
    if classes is not None:
        import ctypes
        words = [0] * ((nc + 63) // 64)
        for c in classes:
            if 0 <= int(c) < nc:
                words[int(c) >> 6] |= 1 << (int(c) & 63)
        mask = (ctypes.c_uint64 * len(words))(*words)
    L = _lib.lib()
    det = torch.empty(B, max_det, 6, dtype=torch.float32, device=prediction.device)
    count = torch.empty(B, dtype=torch.int32, device=prediction.device)
    if mode or merge:
        nbytes = L.somi_nms_ex_workspace_bytes(B, n, nc, int(ml), mode, int(bool(merge)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=prediction.device)
        check(L.somi_nms_ex_f32(_ptr(prediction), B, n, nc, float(conf_thres), float(iou_thres), int(ml), int(bool(agnostic)), mask,
                                int(max_det), mode, int(bool(merge)), float(sigma), float(score_threshold), _ptr(det), _ptr(count),
                                _ptr(ws), nbytes, _stream()), 'non_max_suppression')
        return det, count
    nbytes = L.somi_nms_workspace_bytes(B, n, nc, int(ml))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=prediction.device)
    check(L.somi_nms_f32(_ptr(prediction), B, n, nc, float(conf_thres), float(iou_thres), int(ml), int(bool(agnostic)), mask,
                         int(max_det), _ptr(det), _ptr(count), _ptr(ws), nbytes, _stream()), 'non_max_suppression')
    return det, count


def _boxes_nms(boxes, scores, mode, iou_thres, sigma, score_threshold, who):
    if not (boxes.is_cuda and scores.is_cuda):
        raise RuntimeError('somi_amd NMS runs on the MI355X only (no CPU fallback)')
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or not boxes.is_contiguous() or not scores.is_contiguous():
        raise RuntimeError('boxes and scores have to be contiguous float32')
    if boxes.dim() != 2 or boxes.shape[1] != 4 or scores.shape != boxes.shape[:1]:
        raise ValueError(f'boxes (n, 4) and scores (n) expected, got {tuple(boxes.shape)} and {tuple(scores.shape)}')
    n = boxes.shape[0]
    if n > MAX_BOXES:
        raise ValueError(f'{who} takes at most {MAX_BOXES} boxes (the max_nms of non_max_suppression), got {n}')
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    L = _lib.lib()
    nbytes = L.somi_nms_boxes_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=boxes.device)
    keep = torch.empty(n, dtype=torch.int64, device=boxes.device)
    count = torch.empty(1, dtype=torch.int32, device=boxes.device)
    check(L.somi_nms_boxes_f32(_ptr(boxes), _ptr(scores), n, mode, float(iou_thres), float(sigma), float(score_threshold), _ptr(keep),
                               _ptr(count), _ptr(ws), nbytes, _stream()), who)
    return keep[:int(count.item())]


def NMS(boxes, scores, iou_thres, class_nms='CIoU'):
    """utils/general.py:925-951: indices (int64, on the device) kept by greedy NMS under the GIoU / DIoU / CIoU / EIoU / SIoU overlap of
    utils/metrics.bbox_iou, in descending score order (equal scores in index order).  Any other `class_nms` raises ValueError - the
    reference runs SIoU for every name it does not know.  At most 30000 boxes."""
    if class_nms == 'soft':
        raise ValueError("NMS() is the greedy rule; Soft-NMS is soft_nms()")
    return _boxes_nms(boxes, scores, _mode(class_nms), iou_thres, 0.5, 0.25, 'NMS')


def soft_nms(bboxes, scores, iou_thresh=0.3, sigma=0.5, score_threshold=0.25):
    """utils/general.py:834-862: indices (int64, on the device) in pick order; `scores` is decayed in place.  Like the reference it takes
    the candidates in the given order and picks index 0 first, so callers pass score-sorted input.  The last remaining candidate is kept
    (the reference drops it).  At most 30000 boxes."""
    return _boxes_nms(bboxes, scores, MODES['soft'], iou_thresh, sigma, score_threshold, 'soft_nms')
