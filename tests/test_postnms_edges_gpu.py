"""What follows NMS in the validation path, on the MI355X, at the places where it decides by comparison: weighted boxes fusion
(somi_wbf_f32, somi_wbf_batch_f32) and the validation metrics (somi_val_match_f32, somi_confusion_matrix_f32, somi_ap_per_class_f64) at
exact ties, exactly on their thresholds, past one trip of their strided loops, over the label range of an 80-class model and under
fractional weights.

The cases are built by tests/postnms_edges_ref.py from dyadic coordinates, so a tie is a tie in bits; tests/test_postnms_edges_host.py
shows on the CPU that each case sits on its edge and that the wrong tie rule changes the expected output.  Bars: every WBF comparison is
the one of test_wbf_matches_oracle (equal count, equal labels, boxes and scores array_equal after the oracle's result is stored as
float32), every match / confusion comparison is exact, AP / P / R / F1 use the bar of tests/test_metrics_gpu.py (rtol 1e-9, atol 1e-12).
The oracle is called under the float32 contract of the C ABI (weights and thresholds rounded to float32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import postnms_edges_ref as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7


def assert_wbf(got, want, what):
    gb, gs, gl = got
    wb, ws, wl = want
    assert len(gs) == len(ws) and gb.shape == wb.shape, (what, len(gs), len(ws))
    assert np.array_equal(gl, wl), what                                   # same clusters, same order
    assert np.array_equal(gb, wb), what                                   # bit-exact after the float32 store
    assert np.array_equal(gs, ws), what


# ------------------------------------------------------------------------------------------------ WBF, one image per launch
@pytest.mark.parametrize('name', E.WBF_CASE_NAMES)
def test_wbf_case_matches_oracle(name):
    from somi_amd.wbf import weighted_boxes_fusion
    bl, sl, ll, kw = E.wbf_cases()[name]
    gb, gs, gl = weighted_boxes_fusion(bl, sl, ll, **kw)
    assert_wbf((np.asarray(gb, np.float32).reshape(-1, 4), np.asarray(gs, np.float32), np.asarray(gl).astype(np.int64)),
               E.wbf_expected(name), name)


def test_wbf_label_capacity():
    """Labels up to SOMI_WBF_MAX_LABELS - 1 fuse like the oracle; one outside raises before the launch (no box vanishes silently)."""
    from somi_amd import wbf
    assert wbf.MAX_LABELS >= 80 and wbf.BAD_LABEL == -1
    box = (0.25, 0.25, 0.5, 0.5)
    case = E._case([[(box, 0.75, wbf.MAX_LABELS - 1), ((0.5, 0.5, 0.75, 0.75), 0.5, 0)], [(box, 0.5, wbf.MAX_LABELS - 1)]])
    gb, gs, gl = wbf.weighted_boxes_fusion(*case[:3], **case[3])
    assert_wbf((gb, gs, gl.astype(np.int64)), E.oracle_wbf(case), 'label 127')
    assert sorted(gl.tolist()) == [0, wbf.MAX_LABELS - 1]
    for bad in (wbf.MAX_LABELS, -1, 1000):
        case = E._case([[(box, 0.75, 3)], [(box, 0.5, bad)]])
        with pytest.raises(ValueError, match='labels'):
            wbf.weighted_boxes_fusion(*case[:3], **case[3])


# ------------------------------------------------------------------------------------------------ WBF, the cases as images of a batch
def run_batch(group, counts=None):
    from somi_amd.wbf import weighted_boxes_fusion_batch
    counts = group['counts'] if counts is None else counts
    out = weighted_boxes_fusion_batch([torch.from_numpy(d).to(DEV) for d in group['dets']], [torch.from_numpy(c).to(DEV) for c in counts],
                                      (E.BATCH_SIZE, E.BATCH_SIZE), **group['kwargs'])
    return [o.cpu().numpy() for o in out]


def assert_batch(got, group, counts=None):
    gb, gs, gl, gc = got
    for b, name in enumerate(group['names']):
        want = E.oracle_wbf(E.batch_image_case(group, b, counts))
        k = int(gc[b])
        assert k == len(want[1]), f'{name}: {k} fused boxes, oracle {len(want[1])}'
        assert_wbf((gb[b, :k], gs[b, :k], gl[b, :k].astype(np.int64)), want, name)


@pytest.mark.parametrize('g', range(len(E.wbf_batches())), ids=lambda g: '+'.join(E.wbf_batches()[g]['names'])[:60])
def test_wbf_batch_matches_oracle_image_by_image(g):
    group = E.wbf_batches()[g]
    assert_batch(run_batch(group), group)


def test_wbf_batch_clamps_counts():
    """Counts above max_det and below 0 are clamped: the result equals the call with max_det and 0."""
    group = E.wbf_batches()[0]
    full, empty = group['names'].index('wide_labels'), group['names'].index('degenerate_one_model_empty')
    assert all(int(c[full]) == group['max_det'] for c in group['counts']) and int(group['counts'][0][empty]) == 0
    odd = [c.copy() for c in group['counts']]
    odd[0][full] = group['max_det'] + 5
    odd[0][empty] = -3
    got, ref = run_batch(group, odd), run_batch(group)
    assert_batch(got, group)                                              # against the oracle on the clamped counts
    assert np.array_equal(got[3], ref[3])
    for b in range(len(group['names'])):
        k = int(ref[3][b])
        assert all(np.array_equal(x[b, :k], y[b, :k]) for x, y in zip(got[:3], ref[:3])), group['names'][b]


def test_wbf_batch_marks_images_with_a_label_out_of_range():
    """The batch form has its labels on the device and adds no host synchronisation: an image with a class outside
    [0, SOMI_WBF_MAX_LABELS) gets count SOMI_WBF_BAD_LABEL, the other images are fused as usual."""
    from somi_amd import wbf
    box = (0.25, 0.25, 0.5, 0.5)
    def image(label):
        return E._case([[(box, 0.75, 3), ((0.5, 0.5, 0.75, 0.75), 0.5, label)], [(box, 0.5, 3)]])
    labels = [wbf.MAX_LABELS - 1, wbf.MAX_LABELS, 5, -1, 64]
    cases = [image(l) for l in labels]
    dets = [np.zeros((len(cases), 2, 6), np.float32) for _ in range(2)]
    counts = [np.zeros(len(cases), np.int32) for _ in range(2)]
    for b, (bl, sl, ll, _) in enumerate(cases):
        for t in range(2):
            k = len(sl[t])
            dets[t][b, :k, :4], dets[t][b, :k, 4], dets[t][b, :k, 5], counts[t][b] = bl[t] * np.float32(E.BATCH_SIZE), sl[t], ll[t], k
    group = dict(names=[f'label {l}' for l in labels], dets=dets, counts=counts, kwargs=cases[0][3])
    gb, gs, gl, gc = run_batch(group)
    assert gc.tolist() == [2, wbf.BAD_LABEL, 2, wbf.BAD_LABEL, 2]
    for b in (0, 2, 4):
        assert_wbf((gb[b, :2], gs[b, :2], gl[b, :2].astype(np.int64)), E.oracle_wbf(cases[b]), group['names'][b])


# ------------------------------------------------------------------------------------------------ WBF through the C ABI: scratch, outputs, refusals
def _flat(case):
    bl, sl, ll, kw = case
    boxes = torch.from_numpy(np.concatenate(bl)).to(DEV).contiguous()
    scores = torch.from_numpy(np.concatenate(sl)).to(DEV).contiguous()
    labels = torch.from_numpy(np.concatenate(ll).astype(np.int32)).to(DEV).contiguous()
    model = torch.from_numpy(np.concatenate([np.full(len(s), t, np.int32) for t, s in enumerate(sl)])).to(DEV).contiguous()
    return boxes, scores, labels, model


def _weights(kw, nm):
    w = kw['weights'] if kw['weights'] is not None else [1.0] * nm
    return (C.c_float * nm)(*[float(v) for v in w])


def _outputs(*shape):
    return (torch.full(shape + (4,), float(SENTINEL), device=DEV), torch.full(shape, float(SENTINEL), device=DEV),
            torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV))


def test_wbf_with_dirty_workspace_and_guarded_outputs():
    """somi_wbf_f32 on a workspace of 0xFF bytes and sentinel-filled outputs: the wrapper's result, and no row at or beyond count written."""
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream
    from somi_amd.wbf import weighted_boxes_fusion
    name = 'label_order_and_score_ties'
    case = E.wbf_cases()[name]
    kw = case[3]
    boxes, scores, labels, model = _flat(case)
    n, nm = boxes.shape[0], len(case[0])
    L = _lib.lib()
    nbytes = L.somi_wbf_workspace_bytes(n)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ob, osc, ol = _outputs(n)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = L.somi_wbf_f32(_ptr(boxes), _ptr(scores), _ptr(labels), _ptr(model), n, nm, _weights(kw, nm), kw['iou_thr'], kw['skip_box_thr'],
                        _ptr(ob), _ptr(osc), _ptr(ol), _ptr(cnt), _ptr(ws), nbytes, _stream())
    assert rc == 0
    k = int(cnt.item())
    wb, wsc, wl = weighted_boxes_fusion(*case[:3], **kw)
    assert 0 < k == len(wsc) < n
    assert np.array_equal(ob[:k].cpu().numpy(), wb) and np.array_equal(osc[:k].cpu().numpy(), wsc) and np.array_equal(ol[:k].cpu().numpy(), wl)
    assert (ob[k:] == SENTINEL).all() and (osc[k:] == SENTINEL).all() and (ol[k:] == SENTINEL).all()
    assert_wbf((wb, wsc, wl.astype(np.int64)), E.wbf_expected(name), name)


def _batch_args(group):
    from somi_amd.ops import _ptr
    dets = [torch.from_numpy(d).to(DEV) for d in group['dets']]
    counts = [torch.from_numpy(c).to(DEV) for c in group['counts']]
    nm = len(dets)
    dp = (C.c_void_p * nm)(*[_ptr(d) for d in dets])
    cp = (C.c_void_p * nm)(*[_ptr(c) for c in counts])
    return dets, counts, dp, cp


def test_wbf_batch_with_dirty_workspace_and_guarded_outputs():
    """somi_wbf_batch_f32 likewise: every image's rows at and beyond its count - where a write meant for another image's slice would
    land - still hold the sentinel."""
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream
    group = E.wbf_batches()[0]
    kw = group['kwargs']
    dets, counts, dp, cp = _batch_args(group)
    B, max_det, nm = len(group['names']), group['max_det'], group['n_models']
    N = nm * max_det
    L = _lib.lib()
    nbytes = L.somi_wbf_batch_workspace_bytes(B, max_det, nm)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ob, osc, ol = _outputs(B, N)
    cnt = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = L.somi_wbf_batch_f32(dp, cp, B, max_det, nm, _weights(kw, nm), E.BATCH_SIZE, E.BATCH_SIZE, kw['iou_thr'], kw['skip_box_thr'],
                              _ptr(ob), _ptr(osc), _ptr(ol), _ptr(cnt), _ptr(ws), nbytes, _stream())
    assert rc == 0
    got = [t.cpu().numpy() for t in (ob, osc, ol, cnt)]
    ref = run_batch(group)
    assert np.array_equal(got[3], ref[3]) and (got[3] >= 0).all() and (got[3] < N).any()
    for b, name in enumerate(group['names']):
        k = int(got[3][b])
        assert all(np.array_equal(x[b, :k], y[b, :k]) for x, y in zip(got[:3], ref[:3])), name
        assert all((x[b, k:] == SENTINEL).all() for x in got[:3]), name
    assert_batch(ref, group)


def test_wbf_refuses_bad_arguments_before_any_launch():
    """A workspace one byte short: SOMI_EWORKSPACE; 17 models, an empty batch: SOMI_EINVAL.  Nothing is launched: the outputs keep
    their sentinel."""
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream
    EINVAL, EWORKSPACE = -1, -3
    L = _lib.lib()
    case = E.wbf_cases()['at_iou_threshold_0.5']
    kw = case[3]
    boxes, scores, labels, model = _flat(case)
    n = boxes.shape[0]
    nbytes = L.somi_wbf_workspace_bytes(n)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    ob, osc, ol = _outputs(n)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)

    def single(nm, wbytes):
        return L.somi_wbf_f32(_ptr(boxes), _ptr(scores), _ptr(labels), _ptr(model), n, nm, (C.c_float * 17)(*[1.0] * 17), kw['iou_thr'],
                              kw['skip_box_thr'], _ptr(ob), _ptr(osc), _ptr(ol), _ptr(cnt), _ptr(ws), wbytes, _stream())
    assert single(2, nbytes - 1) == EWORKSPACE
    assert single(17, nbytes) == EINVAL
    group = E.wbf_batches()[1]
    dets, counts, _, _ = _batch_args(group)
    B, max_det, nm = len(group['names']), group['max_det'], group['n_models']
    dp = (C.c_void_p * 17)(*[_ptr(dets[t % nm]) for t in range(17)])
    cp = (C.c_void_p * 17)(*[_ptr(counts[t % nm]) for t in range(17)])
    bbytes = L.somi_wbf_batch_workspace_bytes(B, max_det, 17)
    assert bbytes >= L.somi_wbf_batch_workspace_bytes(B, max_det, nm)
    bws = torch.zeros(bbytes, dtype=torch.uint8, device=DEV)
    bb, bsc, bl = _outputs(B, 17 * max_det)
    bcnt = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)

    def batch(B_, nm_, wbytes):
        return L.somi_wbf_batch_f32(dp, cp, B_, max_det, nm_, (C.c_float * 17)(*[1.0] * 17), E.BATCH_SIZE, E.BATCH_SIZE, kw['iou_thr'],
                                    kw['skip_box_thr'], _ptr(bb), _ptr(bsc), _ptr(bl), _ptr(bcnt), _ptr(bws), wbytes, _stream())
    assert batch(B, nm, L.somi_wbf_batch_workspace_bytes(B, max_det, nm) - 1) == EWORKSPACE
    assert batch(B, 17, bbytes) == EINVAL
    assert batch(0, nm, bbytes) == EINVAL
    torch.cuda.synchronize()
    assert int(cnt.item()) == SENTINEL and (bcnt == SENTINEL).all() and (osc == SENTINEL).all() and (bsc == SENTINEL).all()
    assert batch(B, nm, bbytes) == 0                                      # the same buffers, valid arguments: accepted
    torch.cuda.synchronize()
    assert (bcnt >= 0).all()


# ------------------------------------------------------------------------------------------------ metrics
def test_match_levels_and_duplicates():
    from oracle.somi_ref.metrics import process_batch as oracle
    from somi_amd.metrics import process_batches
    det, lab, iouv, literal = E.match_levels_and_duplicates()
    got = process_batches([det.to(DEV)], [lab.to(DEV)], iouv.to(DEV))[0].cpu()
    assert torch.equal(got, oracle(det, lab, iouv))
    assert torch.equal(got, literal)


@pytest.mark.parametrize('T', [1, 16])
def test_match_stride(T):
    from oracle.somi_ref.metrics import process_batch as oracle
    from somi_amd.metrics import process_batches
    det, lab, iouv = E.match_stride(T)
    want = oracle(det, lab, iouv)
    got = process_batches([det.to(DEV), det[:3].to(DEV)], [lab.to(DEV), lab.to(DEV)], iouv.to(DEV))
    assert torch.equal(got[0].cpu(), want)
    assert torch.equal(got[1].cpu(), want[:3])


def test_match_refuses_seventeen_levels():
    from somi_amd.metrics import process_batches
    det, lab, _ = E.match_stride(1)
    with pytest.raises(RuntimeError, match=r'code -1'):                    # SOMI_EINVAL from the argument check, nothing launched
        process_batches([det.to(DEV)], [lab.to(DEV)], torch.linspace(0.5, 0.95, 17, device=DEV))


def test_confusion_ties():
    from somi_amd.metrics import ConfusionMatrix
    dets, labs = E.confusion_ties()
    want = E.confusion_expected(dets, labs)
    one = ConfusionMatrix(E.CONFUSION_NC, E.CONFUSION_CONF, E.CONFUSION_IOU)
    for b, (d, l) in enumerate(zip(dets, labs)):
        before = one.matrix
        one.process_batch(d.to(DEV), l.to(DEV))
        assert np.array_equal(one.matrix - before, E.confusion_expected([d], [l])), f'image {b}'
    assert np.array_equal(one.matrix, want)
    batch = ConfusionMatrix(E.CONFUSION_NC, E.CONFUSION_CONF, E.CONFUSION_IOU)
    batch.process_batches([d.to(DEV) for d in dets], [l.to(DEV) for l in labs])
    assert np.array_equal(batch.matrix, want)


@pytest.mark.parametrize('all_false', [False, True])
def test_ap_ties(all_false):
    from oracle.somi_ref.metrics import ap_per_class as oracle
    from somi_amd.metrics import ap_per_class
    tp, conf, cls, target = E.ap_ties(all_false)
    wp, wr, wap, wf1, wcls = oracle(tp, conf, cls, target)
    T = torch.from_numpy
    p, r, ap, f1, cls_ = ap_per_class(T(tp).to(DEV), T(conf).to(DEV), T(cls).to(DEV), T(target).to(DEV))
    assert np.array_equal(cls_.cpu().numpy(), wcls)
    for a, b, what in ((p, wp, 'p'), (r, wr, 'r'), (ap, wap, 'ap'), (f1, wf1, 'f1')):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-9, atol=1e-12, err_msg=what)
