"""The NMS kernels at the boundaries of their middle stages, on the MI355X: the tie rule of the top-30000 select across 4096-candidate
chunks, its level-2 / level-3 histograms, exactly 30000 and 30001 candidates, the emit's direct-store path, the carry of the count scan
(more than 256 count chunks) and of the select scan (more than 256 select chunks), the rank sort past its first 2048-key tile with
negative scores and both zeros, and the greedy rounds with the kept list, the max_det stop inside a round and max_det up to 1024.

The scenes are built by tests/nms_edges_ref.py (lattice sites and witnesses); tests/test_nms_edges_host.py shows on the CPU that each
scene's expected output changes under the wrong selection it targets.  Every comparison is shapes and torch.equal against the oracle
(oracle/somi_ref/nms.py) or the restatements (tests/nms_variants_ref.py): lattice boxes are identical or disjoint, so no rule's decision is
near its threshold and kept rows are copies of candidates.  Merged coordinates alone carry a bound, the one of
test_pipeline_matches_the_restatement: (cluster size + 8) * 2^-24 * max|x| against the fp64 restatement.  Scene 2 keeps max_det = 300:
its 20 sites x 10 classes and the witnesses stay below it."""
import pytest
import torch

import nms_edges_ref as E

pytestmark = pytest.mark.gpu


def product(pred, **kw):
    from somi_amd.nms import non_max_suppression
    return [o.cpu() for o in non_max_suppression(pred.cuda(), **kw)]


def assert_rows(got, want, what):
    assert len(got) == len(want), what
    for b, (o, w) in enumerate(zip(got, want)):
        assert o.shape == w.shape, (what, b, tuple(o.shape), tuple(w.shape))
        assert torch.equal(o, w), (what, b)


CUT_CASES = [(kind, 'iou') for kind in E.CUT_KINDS] + [('ties', 'DIoU'), ('ties', 'soft')]


@pytest.mark.parametrize('kind,mode', CUT_CASES)
def test_the_cut_at_30000(kind, mode):
    pred, _ = E.cut_scene(kind)
    want, margins = E.cut_expected(kind, mode)
    assert E.margins_hold(margins), margins
    if mode == 'iou':
        from oracle.somi_ref.nms import non_max_suppression as oracle
        assert_rows(oracle(pred.clone(), **E.CUT_KW), want, 'the restatement against the oracle')
    assert_rows(product(pred, nms=mode, **E.CUT_KW), want, (kind, mode))


def test_the_cut_under_multi_label_with_direct_stores():
    assert_rows(product(E.multi_cut_scene()[0], **E.MULTI_KW), E.multi_cut_expected(), 'multi-label cut')


@pytest.mark.parametrize('n,mode', [(n, 'iou') for n in E.ORDER_SIZES] + [(4097, 'GIoU')])
def test_the_whole_order(n, mode):
    from somi_amd.nms import NMS
    from oracle.somi_ref.nms import greedy_nms
    import nms_variants_ref as R
    boxes, scores = E.order_scene(n)
    want = E.order_expected(n)
    if mode == 'GIoU':
        assert torch.equal(R.penalised_nms(boxes, scores, 0.45, mode), want)
    elif n <= 4097:
        assert torch.equal(greedy_nms(boxes, scores, 0.45), want)
    keep = NMS(boxes.cuda(), scores.cuda(), 0.45, class_nms=mode).cpu()
    assert keep.shape == want.shape, (n, mode, tuple(keep.shape))
    if not torch.equal(keep, want):
        bad = (keep != want).nonzero().view(-1)
        p = int(bad[0])
        raise AssertionError(f'n = {n}, {mode}: {bad.numel()} of {n} positions differ, the first at {p}: got index {int(keep[p])} '
                             f'(score {float(scores[keep[p]])!r}), want {int(want[p])} (score {float(scores[want[p]])!r})')


@pytest.mark.parametrize('leaders,max_det', [(1100, m) for m in E.ROUNDS_MAX_DET] + [(700, 1024)])
def test_rounds_kept_list_and_max_det(leaders, max_det):
    want, _, _ = E.rounds_expected(leaders, max_det)
    assert want[0].shape[0] == min(leaders, max_det)
    assert_rows(product(E.rounds_scene(leaders)[0], max_det=max_det, **E.ROUNDS_KW), want, (leaders, max_det))


def test_merge_over_1024_kept():
    pred, _ = E.rounds_scene(1100)
    want, margins, info = E.rounds_expected(1100, 1024, True)
    want64, _, _ = E.rounds_expected(1100, 1024, True, torch.float64)
    assert E.margins_hold(margins), margins
    got = product(pred, max_det=1024, merge=True, **E.ROUNDS_KW)
    for b, (o, w, w64) in enumerate(zip(got, want, want64)):
        assert o.shape == w.shape == w64.shape, (b, tuple(o.shape), tuple(w.shape))
        assert torch.equal(o[:, 4:], w[:, 4:]), b                            # membership, the `redundant` filter, conf and class
        bound = (info[b]['size'].double() + 8)[:, None] * 2.0 ** -24 * info[b]['xmax']
        err = (o[:, :4].double() - w64[:, :4]).abs()
        print(f'image {b}: {o.shape[0]} merged rows, worst coordinate error at {(err / bound).max().item():.2f} of the bound')
        assert (err <= bound).all(), b


@pytest.mark.parametrize('nc', E.CARRY_NC)
def test_count_scan_carry(nc):
    assert_rows(product(E.carry_scene(nc)[0], **E.CARRY_KW), E.carry_expected(nc), f'nc = {nc}')


def test_select_scan_carry():
    assert_rows(product(E.select_carry_scene()[0], **E.MULTI_KW), E.select_carry_expected(), 'select carry')
