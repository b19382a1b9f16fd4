"""CPU-side conditions of the post-NMS edge cases (tests/postnms_edges_ref.py): a case that does not sit on the edge it names proves
nothing on the device, so every precondition is asserted here with the oracles' own formulas - ties are ties in bits, thresholds are
hit exactly, the wrong tie rule changes the expected output, and the float32 contract of the WBF arguments is visible in the result."""
import numpy as np
import pytest
import torch

import postnms_edges_ref as E
from oracle.somi_ref import metrics as OM
from oracle.somi_ref import wbf as OW
from oracle.somi_ref.nms import box_iou


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ WBF
def test_coordinates_are_dyadic():
    for name, (bl, sl, ll, kw) in E.wbf_cases().items():
        for b in bl:
            assert np.array_equal(b * 128, np.round(b * 128)), name
        assert len(bl) == len(sl) == len(ll) and all(len(b) == len(s) == len(l) for b, s, l in zip(bl, sl, ll)), name
        assert max((len(s) for s in sl), default=0) <= 700, name
    assert tuple(E.wbf_cases()) == E.WBF_CASE_NAMES


@pytest.mark.parametrize('rA,rB', E.TIE_PAIRS)
def test_tie_is_a_tie_and_the_rule_decides(rA, rB, monkeypatch):
    bl, sl, ll, kw = case = E.tie(rA, rB)
    thr = kw['iou_thr']
    a, b, c = E.iou64(E.TIE_C, E.TIE_A), E.iou64(E.TIE_C, E.TIE_B), E.iou64(E.TIE_A, E.TIE_B)
    assert a.tobytes() == b.tobytes() and a > thr and a == 7 / 9          # equal in bits, above the threshold
    assert c == 0.6 and c < thr                                           # A and B stay apart
    assert np.array_equal(bl[0][rA], np.array(E.TIE_A, np.float32)) and np.array_equal(bl[0][rB], np.array(E.TIE_B, np.float32))
    assert (np.diff(sl[0]) < 0).all() and sl[1][0] < sl[0].min()          # founders are visited in list order, C last
    wb, ws, wl = want = E.oracle_wbf(case)
    assert len(ws) == E.TIE_FOUNDERS >= 130 and (wl == 11).all()          # 140 clusters under one label: three trips of the lane scan
    x1 = sorted(wb[(wb[:, 1] == 0) & (wb[:, 3] == 8 * E.U), 0].tolist())  # the two clusters of side 1/16: the loser as it was, the winner moved
    assert len(x1) == 2
    if rA < rB:
        assert 0 < x1[0] < E.U and x1[1] == 2 * E.U                       # A took C
    else:
        assert x1[0] == 0 and E.U < x1[1] < 2 * E.U                       # B took C
    monkeypatch.setattr(OW, '_best_match', E.best_match_last)
    assert not same(E.oracle_wbf(case), want)                             # the other winner changes the output
    monkeypatch.undo()
    assert same(E.oracle_wbf(case), want)


def test_tie_lanes():
    lanes = [((a & 63), (b & 63), a // 64, b // 64) for a, b in E.TIE_PAIRS]
    (a0, b0, _, _), (a1, b1, _, _), (a2, b2, _, _), (_, _, ta, tb) = lanes
    assert a0 > b0 and E.TIE_PAIRS[0][0] < E.TIE_PAIRS[0][1]              # the winner sits on a higher lane than the loser
    assert E.TIE_PAIRS[1][0] > E.TIE_PAIRS[1][1]                          # the later founder (B's rank is lower) wins
    assert a2 == b2                                                       # one lane
    assert ta >= 1 and tb >= 1                                            # both beyond the first trip


def test_iou_threshold_cases_sit_on_the_threshold():
    iou = E.iou64(*E.IOU_PAIR)
    assert iou == 0.5 == E.f32(0.5)
    two, one = E.wbf_expected('at_iou_threshold_0.5'), E.wbf_expected('at_iou_threshold_0.25')
    assert len(two[1]) == 2 and len(one[1]) == 1
    assert np.array_equal(two[0], np.array(E.IOU_PAIR, np.float32))       # apart: both boxes as they came


def test_skip_threshold_case_sits_on_the_threshold():
    bl, sl, ll, kw = E.at_skip_threshold()
    thr = np.float32(kw['skip_box_thr'])
    s = sl[0]
    assert s[0] == thr and s[1] < thr < s[2]
    assert np.nextafter(s[1], np.float32(1)) == thr == np.nextafter(s[2], np.float32(0))
    wb, ws, wl = E.wbf_expected('at_skip_threshold')
    assert len(ws) == 2 and sorted(wb[:, 0].tolist()) == [0.0, 0.0] and sorted(wb[:, 1].tolist()) == [0.0, 0.5]


def test_label_order_and_score_ties():
    wb, ws, wl = E.oracle_wbf(E.label_order_and_score_ties(three_only=True))
    assert wl.tolist() == [70, 2, 7] and ws.tolist() == [.5, .5, .5]
    bl, sl, ll, kw = case = E.label_order_and_score_ties()
    flat_s, flat_l = np.concatenate(sl), np.concatenate(ll)
    seen = list(dict.fromkeys(flat_l[flat_s >= np.float32(kw['skip_box_thr'])].tolist()))
    assert tuple(seen) == E.LABEL_ORDER and flat_l[0] == 0 and flat_s[0] < kw['skip_box_thr']
    wb, ws, wl = E.wbf_expected('label_order_and_score_ties')
    groups = {float(v): wl[ws == v].tolist() for v in np.unique(ws)}
    assert len(groups[0.5]) == 5 and len(groups[0.25]) >= 6               # lone boxes, clusters and the 1.0 box tie in the final sort
    rank = {l: i for i, l in enumerate(E.LABEL_ORDER)}
    for v, labels in groups.items():                                      # inside a tie: the later label of the flat order first
        assert [rank[l] for l in labels] == sorted((rank[l] for l in labels), reverse=True), (v, labels)
    assert len(set(groups[0.5])) >= 4
    # X, Y, Z of label 2: {Z, Y} and {X}
    xs = wb[(wl == 2) & (wb[:, 1] == 0.75)]
    assert sorted(map(tuple, xs[:, [0, 2]].tolist())) == [(0.0, 0.5), (0.1875, 0.6875)]


def test_wide_labels_reach_past_64():
    bl, sl, ll, kw = E.wide_labels()
    assert all(len(s) == E.WIDE_PER_MODEL for s in sl)
    assert E.WIDE_ONLY_MODEL1 in ll[1] and E.WIDE_ONLY_MODEL1 not in ll[0]
    wb, ws, wl = E.wbf_expected('wide_labels')
    out = set(wl.tolist())
    assert len(out) > 4 * 4 and E.WIDE_ONLY_MODEL1 in out and max(out) == 79 and min(out) == 0
    assert {63, 64} <= out and sum(l >= 64 for l in out) >= 8
    assert int((wl >= 64).sum()) >= 20                                    # what the 64-label kernel lost


def test_label_capacity_is_named_in_the_header_and_covers_the_configs():
    import os
    import re
    from somi_amd import wbf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'somi_hip.h')).read()
    cap = int(re.search(r'#define\s+SOMI_WBF_MAX_LABELS\s+(\d+)', header).group(1))
    bad = int(re.search(r'#define\s+SOMI_WBF_BAD_LABEL\s+\((-?\d+)\)', header).group(1))
    assert cap == wbf.MAX_LABELS >= 80 and bad == wbf.BAD_LABEL < 0        # 80: the largest nc the repository's configs build
    assert max(max(l.max(initial=0) for l in c[2]) for c in E.wbf_cases().values()) == 79


def test_fractional_weights_show_the_float32_contract():
    case = E.fractional_weights()
    w = case[3]['weights']
    assert [E.f32(v) != v for v in w] == [True, True, False]
    b32, s32, l32 = E.oracle_wbf(case)
    b64, s64, l64 = E.oracle_wbf(case, float32_contract=False)
    assert len(s32) == len(s64) and np.array_equal(l32, l64)
    assert int((s32 != s64).sum()) >= 1 or int((b32 != b64).sum()) >= 1   # the double weights give other float32 results
    print('fused scores that differ:', int((s32 != s64).sum()), 'coordinates that differ:', int((b32 != b64).sum()))
    # clusters larger than sum(weights)
    wsum = float(np.sum([E.f32(v) for v in w]))
    assert wsum == 2.5
    n_in = sum(len(s) for s in case[1])
    assert n_in - len(s32) >= 30 and len(s32) <= 3 + 12 + 6                # 57 boxes in at most 21 clusters: most hold 3 or more


@pytest.mark.parametrize('kind', E.DEGENERATE)
def test_degenerate_cases(kind):
    bl, sl, ll, kw = E.degenerate(kind)
    wb, ws, wl = E.wbf_expected('degenerate_' + kind)
    if kind == 'nothing_survives':
        assert len(ws) == 0 and sum(len(s) for s in sl) == 5
    elif kind == 'one_model_empty':
        assert len(sl[0]) == 0 and wl.tolist() == [4, 66] and ws.tolist() == [0.625, 0.25]
    elif kind == 'all_identical':
        assert len(ws) == 1 and sum(len(s) for s in sl) == 70 and np.array_equal(wb[0], bl[0][0])
    elif kind == 'reversed':
        assert any((b[:, 2] < b[:, 0]).any() for b in bl) and any((b[:, 3] < b[:, 1]).any() for b in bl)
        assert any(((b[:, 2] < b[:, 0]) & (b[:, 3] < b[:, 1])).any() for b in bl)
        assert len(ws) == 3 and (wb[:, 2] > wb[:, 0]).all() and (wb[:, 3] > wb[:, 1]).all()
    else:
        assert len(ws) == 1 and np.array_equal(wb[0], np.array([0, 0.5, 0.25, 0.75], np.float32))


def test_batches_cover_the_cases():
    groups = E.wbf_batches()
    assert sorted(n for g in groups for n in g['names']) == sorted(E.WBF_CASE_NAMES) and len(groups) <= 8
    first = groups[0]
    b = first['names'].index('wide_labels')
    assert all(int(c[b]) == first['max_det'] for c in first['counts'])     # count == max_det for every model
    for g in groups:
        for d in g['dets']:
            assert np.array_equal(d[..., :4], np.round(d[..., :4])) and d.shape[1:] == (g['max_det'], 6)
        for b, name in enumerate(g['names']):
            case = E.batch_image_case(g, b)
            for t, s in enumerate(case[1]):
                assert (np.diff(s) <= 0).all(), (name, t)                 # sorted by confidence, as NMS leaves the rows
            if len(E.wbf_cases()[name][0]) == g['n_models'] and g['kwargs']['weights'] is None:
                got, want = E.oracle_wbf(case), E.wbf_expected(name)
                assert len(got[1]) == len(want[1]) and sorted(got[1].tolist()) == sorted(want[1].tolist()), name


# ------------------------------------------------------------------------------------------------ metrics
def test_match_literal_equals_the_oracle():
    det, lab, iouv, literal = E.match_levels_and_duplicates()
    assert torch.equal(OM.process_batch(det, lab, iouv), literal)
    iou = box_iou(lab[:, 1:], det[:, :4])
    assert iou[0, 0] == iouv[0] == 0.5 and iou[0, 1] == iouv[5] == 0.75    # exactly on a level, in float32
    assert torch.equal(iou[0], iou[1]) and torch.equal(det[3], det[4])     # duplicate labels, duplicate detections


@pytest.mark.parametrize('T', [1, 16])
def test_match_stride(T):
    det, lab, iouv = E.match_stride(T)
    assert det.shape[0] == E.STRIDE_N > 256 and iouv.numel() == T
    want = OM.process_batch(det, lab, iouv)
    rows = want.any(1).nonzero().view(-1).tolist()
    assert rows == [0, 256, 300]
    assert want[0].all() and want[256].all()
    iou = box_iou(lab[:, 1:], det[300:, :4])[:, 0]
    assert iou[2] == 1.0 and iou[3] == 0.75 and lab[2, 0] != det[300, 5] == lab[3, 0]
    assert torch.equal(want[300], iouv <= 0.75) and (T == 1 or not want[300].all())   # label 2 (another class) was ignored


def test_confusion_ties():
    dets, labs = E.confusion_ties()
    nc = E.CONFUSION_NC
    each = []
    for d, l in zip(dets, labs):
        cm = OM.ConfusionMatrix(nc, E.CONFUSION_CONF, E.CONFUSION_IOU)
        cm.process_batch(d, l)
        each.append(cm.matrix)
    def cells(m):
        return {(int(i), int(j)): int(m[i, j]) for i, j in zip(*np.nonzero(m))}
    assert cells(each[0]) == {(1, 1): 1, (2, nc): 1}
    assert cells(each[1]) == {(4, 2): 1, (nc, 3): 1}
    assert cells(each[2]) == {(4, 4): 1, (nc, 3): 1, (3, nc): 1}
    assert float(box_iou(labs[2][:1, 1:], dets[2][:1, :4])) == E.CONFUSION_IOU
    assert cells(each[3]) == {(nc, 1): 1, (2, 2): 1} and float(dets[3][0, 4]) == E.CONFUSION_CONF
    assert cells(each[4]) == {(nc, 0): 1, (nc, 1): 1}
    assert cells(each[5]) == {}
    assert cells(each[6]) == {(2, 0): 1, (1, 3): 1, (0, nc): 295, (3, nc): 1, (4, nc): 1} and dets[6].shape[0] == 300
    assert cells(each[7]) == {(nc, 4): 2}
    assert np.array_equal(E.confusion_expected(dets, labs), sum(each))


def test_ap_ties():
    tp, conf, cls, target = E.ap_ties()
    assert np.array_equal(conf * 16, np.round(conf * 16)) and (conf == 1).sum() >= 20 and (conf == 0).sum() >= 20
    c = E.AP_CLASSES
    assert (cls == c['big']).sum() > 600 and (cls == c['single']).sum() == 1
    assert (cls == c['target_only']).sum() == 0 and (target == c['target_only']).sum() > 0
    assert (cls == c['pred_only']).sum() > 0 and (target == c['pred_only']).sum() == 0
    for k in (c['big'], c['mid']):                                        # a confidence tie with differing tp, in every class that can have one
        sel = cls == k
        assert any(len(set(tp[sel & (conf == v), 0].tolist())) == 2 for v in np.unique(conf[sel])), k
    p, r, ap, f1, classes = OM.ap_per_class(tp, conf, cls, target)
    assert classes.tolist() == [0, 2, 5, 7] and (ap[3] == 0).all() and (ap[:2] > 0).all()
    p2, r2, ap2, f12, _ = E.ap_per_class_tie_reversed(tp, conf, cls, target)
    assert not np.array_equal(ap, ap2)                                    # the order inside the ties decides the curve
    assert np.abs(ap[:2] - ap2[:2]).max() > 1e-6                          # far above the comparison's bar


def test_ap_all_false():
    tp, conf, cls, target = E.ap_ties(all_false=True)
    assert not tp.any()
    p, r, ap, f1, classes = OM.ap_per_class(tp, conf, cls, target)
    assert (f1 == 0).all() and (ap == 0).all() and classes.tolist() == [0, 2, 5, 7]
