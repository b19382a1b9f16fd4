"""Case builders for the tests of what follows NMS in the validation path (test infrastructure, numpy / torch on the CPU only): weighted
boxes fusion (csrc/wbf.hip) and the validation metrics (csrc/valmetrics.hip) at exact ties, exactly on their thresholds, past one trip
of their strided loops and over the whole label range.  tests/test_postnms_edges_host.py proves on the CPU that each case sits on the
edge it names; tests/test_postnms_edges_gpu.py runs them on the device against the oracles (oracle/somi_ref/wbf.py, metrics.py), whose
tie rules (`_desc`, `np.argmax`, lowest index) are the specification.

All coordinates are dyadic rationals - multiples of 1/128 in [0, 1] for WBF, multiples of 16 px for the metrics - and the scores that
have to tie are dyadic too, so products, sums and IoUs are exact in fp32 and fp64 and a tie is a tie in bits.

A WBF case is (boxes_list, scores_list, labels_list, kwargs): float32 boxes and scores, int64 labels, kwargs for both the oracle and
`somi_amd.wbf.weighted_boxes_fusion`.  `oracle_wbf` calls the oracle under the float32 contract of the C ABI: weights, iou_thr and
skip_box_thr rounded to float32 first.
"""
import functools

import numpy as np
import torch

from oracle.somi_ref import metrics as OM
from oracle.somi_ref import wbf as OW

F = np.float32
U = 1.0 / 128


def _case(models, **kw):
    """models: per model a list of (box, score, label) -> the four-tuple of a case"""
    bl = [np.array([m[0] for m in rows], dtype=F).reshape(-1, 4) for rows in models]
    sl = [np.array([m[1] for m in rows], dtype=F).reshape(-1) for rows in models]
    ll = [np.array([m[2] for m in rows], dtype=np.int64).reshape(-1) for rows in models]
    kwargs = dict(weights=None, iou_thr=0.625, skip_box_thr=0.0)
    kwargs.update(kw)
    return bl, sl, ll, kwargs


def f32(v):
    return float(np.float32(v))


def contract_kwargs(kw):
    """The kwargs as the C ABI sees them: float32 values (held in Python floats)."""
    w = kw.get('weights')
    return dict(weights=None if w is None else [f32(v) for v in w], iou_thr=f32(kw['iou_thr']), skip_box_thr=f32(kw['skip_box_thr']))


def oracle_wbf(case, float32_contract=True):
    """-> (boxes (n, 4) float32, scores (n) float32, labels (n) int64) of the oracle, stored as the device stores them."""
    bl, sl, ll, kw = case
    kw = contract_kwargs(kw) if float32_contract else dict(kw)
    b, s, l = OW.weighted_boxes_fusion([x.tolist() for x in bl], [x.tolist() for x in sl], [x.tolist() for x in ll], **kw)
    return (np.asarray(b, dtype=np.float64).reshape(-1, 4).astype(F), np.asarray(s, dtype=np.float64).astype(F),
            np.asarray(l, dtype=np.float64).astype(np.int64))


def iou64(a, b):
    """IoU of two xyxy boxes in float64, in the order of operations of the oracle's `_best_match`."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    inter = np.maximum(np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]), 0) * np.maximum(np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]), 0)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def best_match_last(fused, new_box, thr):
    """`oracle.somi_ref.wbf._best_match` with the wrong tie rule: the LAST cluster of highest IoU.  Only the host test uses it, to show that
    a case's expected output depends on the rule."""
    if fused.shape[0] == 0:
        return -1
    iou = np.array([iou64(f[4:], new_box[4:]) if f[0] == new_box[0] else -1.0 for f in fused])
    k = len(iou) - 1 - int(np.argmax(iou[::-1]))
    return k if iou[k] > thr else -1


# ------------------------------------------------------------------------------------------------ WBF: the cluster scan's tie rule
TIE_PAIRS = ((3, 66), (66, 3), (5, 69), (70, 130))      # winner on a higher lane; the later founder wins; one lane; both past trip one
TIE_FOUNDERS = 140
TIE_A = (0.0, 0.0, 8 * U, 8 * U)                        # side 1/16
TIE_B = (2 * U, 0.0, 10 * U, 8 * U)                     # A + 1/64 in x: IoU(A, B) = 0.6, they stay apart at 0.625
TIE_C = (1 * U, 0.0, 9 * U, 8 * U)                      # A + 1/128 in x: IoU 7/9 with both


def tie(rA, rB):
    """One label, 140 cluster founders from model 0 with scores 0.99 - 0.005 k (visited in that order, so founder k is cluster k): rank rA
    is A, rank rB is B, the others are boxes of side 1/32 in distinct cells of a 16 x 16 grid (cell (0, 0), where A, B and C live, and its
    neighbour (1, 0), which B reaches into, left out).  Model 1's single box C, score 0.2, comes last and has the same IoU with A and B:
    it has to join the one of lower cluster index."""
    cells = [(i, j) for j in range(16) for i in range(16) if (i, j) not in ((0, 0), (1, 0))]
    rows = []
    for k in range(TIE_FOUNDERS):
        if k == rA:
            box = TIE_A
        elif k == rB:
            box = TIE_B
        else:
            i, j = cells[(k * 7) % len(cells)]
            box = (i * 8 * U, j * 8 * U, i * 8 * U + 4 * U, j * 8 * U + 4 * U)
        rows.append((box, 0.99 - 0.005 * k, 11))
    return _case([rows, [(TIE_C, 0.2, 11)]], iou_thr=0.625, skip_box_thr=0.0)


# ------------------------------------------------------------------------------------------------ WBF: on the thresholds
IOU_PAIR = ((0.0, 0.0, 0.5, 0.5), (0.0, 0.0, 0.5, 0.25))    # IoU 0.5 exactly


def at_iou_threshold(iou_thr):
    """Two boxes of IoU 0.5 under one label: two clusters at iou_thr = 0.5 (the rule is a strict >), one at 0.25."""
    return _case([[(IOU_PAIR[0], 0.75, 3)], [(IOU_PAIR[1], 0.5, 3)]], iou_thr=iou_thr)


SKIP_THR = 0.25


def at_skip_threshold():
    """Scores exactly on skip_box_thr, one float32 below and one above: `score < thr` drops the middle one only."""
    below, above = np.nextafter(F(SKIP_THR), F(0)), np.nextafter(F(SKIP_THR), F(1))
    rows = [((0.0, 0.0, 0.25, 0.25), SKIP_THR, 1), ((0.5, 0.0, 0.75, 0.25), below, 1), ((0.0, 0.5, 0.25, 0.75), above, 1)]
    return _case([rows, []], skip_box_thr=SKIP_THR)


# ------------------------------------------------------------------------------------------------ WBF: label order, ties in both sorts
LABEL_ORDER = (7, 2, 70, 63, 64, 0)


def label_order_and_score_ties(three_only=False):
    """Labels first appear (among the boxes that pass the filters) in the order 7, 2, 70, 63, 64, 0; label 0's very first row lies below
    skip_box_thr, so its first appearance is its later row.  Lone boxes of score 0.5 in several labels, a lone box of score 1.0 and
    two-member clusters whose mean is 0.5 all tie in the final sort (0.25 and 0.5 after the rescale by min(count, 2) / 2): the later flat
    index goes first, and the flat order is the labels' first-appearance order.  Label 2 also holds X, Y, Z of equal score where Y matches
    both X and Z: visited later-first (Z, Y, X) the clusters are {Z, Y}, {X}; any other order of the tie gives other boxes.
    three_only: just the lone boxes of labels 7, 2, 70."""
    def cell(i, j, w=16, h=16):
        return (i * 20 * U, j * 20 * U, (i * 20 + w) * U, (j * 20 + h) * U)
    if three_only:
        return _case([[(cell(0, 0), 0.5, 7), (cell(1, 0), 0.5, 2), (cell(2, 0), 0.5, 70)]], iou_thr=0.55, skip_box_thr=0.125)
    m0 = [(cell(5, 0), 0.0625, 0),                           # dropped: label 0 does not appear here
          (cell(0, 0), 0.5, 7), (cell(1, 0), 0.5, 2), (cell(2, 0), 0.5, 70),
          (cell(3, 0), 0.75, 63), (cell(4, 0), 0.5, 64), (cell(5, 1), 1.0, 0),
          (cell(0, 1), 0.625, 7), (cell(1, 1), 1.0, 2), (cell(2, 1), 0.5, 70), (cell(3, 1), 0.5, 63),
          ((0.0, 0.75, 0.5, 1.0), 0.375, 2)]                 # X
    m1 = [(cell(3, 0), 0.25, 63), (cell(4, 0), 0.5, 64), (cell(0, 1), 0.375, 7),
          ((0.125, 0.75, 0.625, 1.0), 0.375, 2),             # Y
          ((0.25, 0.75, 0.75, 1.0), 0.375, 2),               # Z
          (cell(5, 2), 0.5, 0), (cell(4, 2), 0.5, 64)]
    return _case([m0, m1], iou_thr=0.55, skip_box_thr=0.125)


# ------------------------------------------------------------------------------------------------ WBF: the whole label range
WIDE_PER_MODEL = 140
WIDE_ONLY_MODEL1 = 77


def wide_labels():
    """Two models, 140 boxes each, 22 labels out of range(80) with 64..79 among them (what a model with nc = 80 produces), one label that
    only model 1 reports: more labels than the four waves, so every wave takes several.  Both models see the same 60 objects, shifted by
    a few 1/128."""
    rng = np.random.RandomState(2024)
    labels = np.array([0, 1, 7, 15, 31, 32, 33, 47, 62, 63, 64, 65, 66, 69, 70, 72, 75, 76, 78, 79, 40])
    centre = rng.randint(16, 100, (60, 2))
    size = rng.randint(6, 24, (60, 2))
    obj_label = labels[rng.randint(0, len(labels), 60)]
    obj_label[:len(labels)] = labels                         # every label occurs
    models = []
    for t in range(2):
        pick = rng.randint(0, 60, WIDE_PER_MODEL)
        pick[:60] = rng.permutation(60)
        xy = centre[pick] + rng.randint(-2, 3, (WIDE_PER_MODEL, 2))
        wh = size[pick] + rng.randint(-1, 2, (WIDE_PER_MODEL, 2))
        box = np.concatenate([xy - wh // 2, xy - wh // 2 + wh], 1) * U
        score = rng.randint(4, 128, WIDE_PER_MODEL) / 128.0
        lab = obj_label[pick].copy()
        if t == 1:
            lab[5::17] = WIDE_ONLY_MODEL1
        models.append([(tuple(b), s, l) for b, s, l in zip(box, score, lab)])
    return _case(models, iou_thr=0.625, skip_box_thr=0.0)


# ------------------------------------------------------------------------------------------------ WBF: float32 weights
FRACTIONAL_WEIGHTS = (0.7, 0.3, 1.5)


def fractional_weights():
    """Three models with weights 0.7, 0.3, 1.5 - the first two are no float32 values - over 12 objects that every model reports once or
    twice, so clusters hold 3 to 6 members, more than sum(weights) = 2.5 (the min(count, sum) branch), and three lone boxes."""
    rng = np.random.RandomState(7)
    centre = np.stack([np.arange(12) % 4 * 30 + 16, np.arange(12) // 4 * 40 + 20], 1)
    models = []
    for t in range(3):
        pick = np.concatenate([np.arange(12), rng.randint(0, 12, 6)])
        xy = centre[pick] + rng.randint(-1, 2, (18, 2))
        wh = np.array([24, 32]) + rng.randint(-1, 2, (18, 2))
        box = np.concatenate([xy - wh // 2, xy - wh // 2 + wh], 1) * U
        score = rng.randint(20, 127, 18) / 128.0 + rng.randint(0, 2, 18) * 2.0 ** -12
        rows = [(tuple(b), s, p % 3) for b, s, p in zip(box, score, pick)]
        rows.append(((t * 10 * U, 120 * U, (t * 10 + 8) * U, 128 * U), 0.5, 1))
        models.append(rows)
    return _case(models, weights=list(FRACTIONAL_WEIGHTS), iou_thr=0.625, skip_box_thr=0.0)


# ------------------------------------------------------------------------------------------------ WBF: degenerate inputs
DEGENERATE = ('nothing_survives', 'one_model_empty', 'all_identical', 'reversed', 'outside')


def degenerate(kind):
    if kind == 'nothing_survives':                           # zero area, below the threshold, clipped to zero area: count 0
        m0 = [((0.25, 0.25, 0.25, 0.5), 0.9, 1), ((0.5, 0.5, 0.75, 0.5), 0.9, 2), ((0.0, 0.0, 0.25, 0.25), 0.125, 1)]
        m1 = [((0.5, 0.5, 0.75, 0.75), np.nextafter(F(SKIP_THR), F(0)), 1), ((1.0, 0.25, 1.5, 0.5), 0.9, 3)]
        return _case([m0, m1], skip_box_thr=SKIP_THR)
    if kind == 'one_model_empty':
        m1 = [((0.0, 0.0, 0.25, 0.25), 0.75, 4), ((0.0, 0.0, 0.25, 0.25), 0.5, 4), ((0.5, 0.5, 0.75, 0.75), 0.5, 66)]
        return _case([[], m1])
    if kind == 'all_identical':                              # one cluster of 70 members, scores with ties
        box = (0.25, 0.125, 0.5, 0.625)
        return _case([[(box, (40 + k % 9) / 64.0, 9) for k in range(40)], [(box, (40 + k % 7) / 64.0, 9) for k in range(30)]])
    if kind == 'reversed':                                   # corners reversed on x, on y, on both; they meet their ordered twins
        m0 = [((0.5, 0.25, 0.25, 0.5), 0.75, 1), ((0.5, 0.75, 0.75, 0.5), 0.625, 1), ((0.25, 1.0, 0.0, 0.75), 0.5, 65)]
        m1 = [((0.25, 0.25, 0.5, 0.5), 0.5, 1), ((0.5, 0.5, 0.75, 0.75), 0.5, 1), ((0.0, 0.75, 0.25, 1.0), 0.25, 65)]
        return _case([m0, m1])
    if kind == 'outside':                                    # entirely outside [0, 1]: clipped to zero area and dropped; one straddles
        m0 = [((-0.5, -0.5, -0.25, -0.25), 0.9, 1), ((1.25, 0.25, 1.5, 0.5), 0.9, 1), ((0.25, 1.0, 0.5, 1.5), 0.9, 1),
              ((-0.25, 0.5, 0.25, 0.75), 0.75, 1)]
        m1 = [((0.0, 0.5, 0.25, 0.75), 0.5, 1), ((0.25, -1.0, 0.5, -0.5), 0.5, 2)]
        return _case([m0, m1])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def wbf_cases():
    """name -> case, in a fixed order"""
    cases = {f'tie_{a}_{b}': tie(a, b) for a, b in TIE_PAIRS}
    cases['at_iou_threshold_0.5'] = at_iou_threshold(0.5)
    cases['at_iou_threshold_0.25'] = at_iou_threshold(0.25)
    cases['at_skip_threshold'] = at_skip_threshold()
    cases['label_order_and_score_ties'] = label_order_and_score_ties()
    cases['wide_labels'] = wide_labels()
    cases['fractional_weights'] = fractional_weights()
    for kind in DEGENERATE:
        cases['degenerate_' + kind] = degenerate(kind)
    return cases


WBF_CASE_NAMES = tuple(f'tie_{a}_{b}' for a, b in TIE_PAIRS) + ('at_iou_threshold_0.5', 'at_iou_threshold_0.25', 'at_skip_threshold',
                                                               'label_order_and_score_ties', 'wide_labels', 'fractional_weights') + \
    tuple('degenerate_' + k for k in DEGENERATE)


@functools.lru_cache(maxsize=None)
def wbf_expected(name):
    return oracle_wbf(wbf_cases()[name])


# ------------------------------------------------------------------------------------------------ WBF: the cases as images of a batch
BATCH_SIZE = 1024.0                                          # a power of two: box * size and the kernel's division by it are exact


def _group_key(kw):
    w = kw['weights']
    return (None if w is None else tuple(w), kw['iou_thr'], kw['skip_box_thr'])


@functools.lru_cache(maxsize=None)
def wbf_batches():
    """The cases grouped by their kwargs (one `weighted_boxes_fusion_batch` call has one set): -> list of dicts with names, dets (per model
    (B, max_det, 6) float32 in pixels, rows sorted by confidence as NMS leaves them), counts (per model (B) int32), n_models, max_det,
    kwargs.  A case with fewer models than its group gets empty ones (count 0).  max_det is the group's largest count, so in the first
    group `wide_labels` fills every model to max_det."""
    groups = {}
    for name in WBF_CASE_NAMES:
        groups.setdefault(_group_key(wbf_cases()[name][3]), []).append(name)
    out = []
    for names in groups.values():
        cases = [wbf_cases()[n] for n in names]
        nm = max(len(c[0]) for c in cases)
        max_det = max(1, max(len(s) for c in cases for s in c[1]))
        dets = [np.zeros((len(cases), max_det, 6), F) for _ in range(nm)]
        counts = [np.zeros(len(cases), np.int32) for _ in range(nm)]
        for b, (bl, sl, ll, _) in enumerate(cases):
            for t in range(len(bl)):
                order = np.argsort(-sl[t], kind='stable')
                k = len(order)
                dets[t][b, :k, :4] = bl[t][order] * F(BATCH_SIZE)
                dets[t][b, :k, 4] = sl[t][order]
                dets[t][b, :k, 5] = ll[t][order]
                counts[t][b] = k
        out.append(dict(names=names, dets=dets, counts=counts, n_models=nm, max_det=max_det, kwargs=cases[0][3]))
    return out


def batch_image_case(group, b, counts=None):
    """Image b of a batch group as a WBF case on the normalised, clipped boxes (what the kernel gathers)."""
    counts = group['counts'] if counts is None else counts
    bl, sl, ll = [], [], []
    for d, c in zip(group['dets'], counts):
        k = int(c[b])
        bl.append(np.clip(d[b, :k, :4] / F(BATCH_SIZE), 0, 1).astype(F))
        sl.append(d[b, :k, 4].copy())
        ll.append(d[b, :k, 5].astype(np.int64))
    return bl, sl, ll, group['kwargs']


# ------------------------------------------------------------------------------------------------ metrics: process_batch
IOUV = torch.linspace(0.5, 0.95, 10)

MATCH_LAB = [[1, 0, 0, 64, 64], [1, 0, 0, 64, 64], [1, 100, 100, 164, 164]]
MATCH_DET = [[0, 0, 64, 32, .9, 1], [0, 0, 64, 48, .8, 1], [0, 0, 64, 64, .7, 1], [100, 100, 164, 164, .6, 1], [100, 100, 164, 164, .6, 1]]
MATCH_CORRECT = [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                 [0, 1, 1, 1, 1, 1, 0, 0, 0, 0],
                 [0, 0, 0, 0, 0, 0, 1, 1, 1, 1],
                 [1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
                 [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]


def match_levels_and_duplicates():
    """IoU 0.5 and 0.75 exactly on a level (the float32 linspace holds both exactly), duplicate labels (the lowest label takes every tie)
    and duplicate detections (the lowest detection keeps the label) -> (det, lab, iouv, the expected matrix as a literal)."""
    return torch.tensor(MATCH_DET), torch.tensor(MATCH_LAB, dtype=torch.float32), IOUV, torch.tensor(MATCH_CORRECT, dtype=torch.bool)


STRIDE_N = 301


def match_stride(T):
    """301 detections, more than the 256 threads that stride over them.  0..299 are one box: 0..255 of class 1 on label 0 (detection 0
    keeps it), 256..299 of class 2 on label 1, the same box in class 2, which only they match (256, the lowest, keeps it).  Detection
    300 (class 4) has IoU 0.75 with label 3 of its class and IoU 1 with label 2 of class 3, listed first: that one has to be ignored.
    -> (det, lab, iouv of T levels)."""
    box = [64., 64., 128., 128.]
    lab = torch.tensor([[1.] + box, [2.] + box, [3., 192., 64., 256., 112.], [4., 192., 64., 256., 128.]])
    det = torch.zeros(STRIDE_N, 6)
    det[:300, :4] = torch.tensor(box)
    det[:256, 5], det[256:300, 5] = 1, 2
    det[300] = torch.tensor([192., 64., 256., 112., 0.5, 4.])
    det[:, 4] = 1.0 - torch.arange(STRIDE_N) / 512
    iouv = torch.tensor([0.5]) if T == 1 else torch.linspace(0.5, 0.95, T)
    return det, lab, iouv


# ------------------------------------------------------------------------------------------------ metrics: confusion matrix
CONFUSION_NC, CONFUSION_CONF, CONFUSION_IOU = 5, 0.25, 0.5


def confusion_ties():
    """-> (dets, labs): eight images, one edge each.  Boxes are 64 px squares on a 128 px lattice unless stated."""
    def sq(i, j=0):
        return [i * 128., j * 128., i * 128. + 64, j * 128. + 64]
    above = float(np.nextafter(F(CONFUSION_CONF), F(1)))
    dets, labs = [], []
    # 0: two identical detections on one label: the lower keeps it, the other is (class, background)
    labs.append([[1.] + sq(0)])
    dets.append([sq(0) + [.9, 1.], sq(0) + [.9, 2.]])
    # 1: one detection on two duplicate labels: it takes the lower, the other label is (background, class)
    labs.append([[2.] + sq(1), [3.] + sq(1)])
    dets.append([sq(1) + [.9, 4.]])
    # 2: IoU exactly 0.5 = iou_thres: no match (strict >); a matched pair beside it, so the detection counts as a false positive
    labs.append([[3.] + sq(0), [4.] + sq(2)])
    dets.append([[0., 0., 64., 32., .9, 3.], sq(2) + [.8, 4.]])
    # 3: confidence exactly 0.25 = conf: dropped (strict >); one float32 above it: kept
    labs.append([[1.] + sq(0), [2.] + sq(1)])
    dets.append([sq(0) + [CONFUSION_CONF, 1.], sq(1) + [above, 2.]])
    # 4: labels and detections, no match: the labels are missed, no false positive is counted (`if n:`)
    labs.append([[0.] + sq(0), [1.] + sq(1)])
    dets.append([sq(2) + [.9, 0.], sq(3) + [.9, 1.], [0., 0., 64., 32., .9, 0.]])
    # 5: no labels: nothing is counted
    labs.append([])
    dets.append([sq(0) + [.9, 1.], sq(1) + [.9, 2.]])
    # 6: 300 detections.  Label 0: all but four have IoU 0.75 with it, 270 and 290 are the label's box (270, the lower, keeps it, class 2).
    #    Label 1: detections 5 and 260 are its box (5 keeps it, class 1).  Everything else is a false positive of class 0.
    labs.append([[0.] + sq(0), [3.] + sq(2)])
    d = [[0., 0., 64., 48., .9, 0.] for _ in range(300)]
    d[270], d[290] = sq(0) + [.5, 2.], sq(0) + [.9, 3.]
    d[5], d[260] = sq(2) + [.6, 1.], sq(2) + [.7, 4.]
    d[100][4] = CONFUSION_CONF                                # dropped: the indices the oracle sees shift, the order does not
    dets.append(d)
    # 7: no detections: every label is missed
    labs.append([[4.] + sq(0), [4.] + sq(0)])
    dets.append([])
    return ([torch.tensor(d, dtype=torch.float32).reshape(-1, 6) for d in dets],
            [torch.tensor(l, dtype=torch.float32).reshape(-1, 5) for l in labs])


def confusion_expected(dets, labs):
    cm = OM.ConfusionMatrix(CONFUSION_NC, CONFUSION_CONF, CONFUSION_IOU)
    for d, l in zip(dets, labs):
        cm.process_batch(d, l)
    return cm.matrix


# ------------------------------------------------------------------------------------------------ metrics: ap_per_class
AP_CLASSES = dict(big=0, mid=2, single=5, target_only=7, pred_only=9)


@functools.lru_cache(maxsize=None)
def ap_ties(all_false=False):
    """-> (tp (N, 10) bool, conf (N), pred_cls (N), target_cls (M)) as numpy arrays.  Confidences are k/16 with many at exactly 1.0 and
    0.0; inside every tie group true and false positives alternate irregularly, so the order of the tie decides the curve.  Class 0 has
    650 detections (several 256-chunks of the gather, several blocks of the rank), class 2 has 90, class 5 a single one, class 7 occurs
    among the targets only and class 9 among the predictions only.  all_false: the same with an all-false tp (a flat mean F1)."""
    rng = np.random.RandomState(5)
    n = dict(big=650, mid=90, single=1, pred_only=12)
    cls = np.concatenate([np.full(k, AP_CLASSES[name], np.float32) for name, k in n.items()])
    N = cls.size
    perm = rng.permutation(N)
    cls = cls[perm]
    conf = (rng.randint(0, 17, N) / 16.0).astype(np.float32)
    conf[rng.permutation(N)[:40]] = 1.0
    conf[rng.permutation(N)[:40]] = 0.0
    levels = np.where(rng.rand(N) < 0.55, rng.randint(1, 11, N), 0)          # correct at the first `levels` IoU levels
    tp = np.arange(10)[None, :] < levels[:, None]
    if all_false:
        tp = np.zeros_like(tp)
    target = np.concatenate([np.full(400, 0.), np.full(70, 2.), np.full(3, 5.), np.full(6, 7.)]).astype(np.float32)
    return tp, conf, cls, target[rng.permutation(target.size)]


def ap_per_class_tie_reversed(tp, conf, pred_cls, target_cls):
    """The oracle's ap_per_class under the wrong tie rule (equal confidences in descending index order)."""
    order = np.lexsort((-np.arange(conf.size), -conf))
    return OM.ap_per_class(tp[order], conf[order], pred_cls[order], target_cls)
