"""CPU-side conditions of the NMS stage-boundary scenes (tests/nms_edges_ref.py): a scene that does not show the decision it targets proves
nothing, so every condition is asserted here on the references' outputs alone.  The witness just inside the cut is in the expected output
and the one just outside is not; the cap max_det did not hide the tail; and three wrong selections, applied on the CPU to the scene's own
candidate list, each change the expected output of the scene that targets them: one tie too many or too few, ties taken in descending
index order, and a prefix scan that drops its carry after 256 chunks."""
import pytest
import torch

import nms_edges_ref as E
import nms_variants_ref as R
from oracle.somi_ref import nms as O


def same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


def tie_witnesses(meta, out):
    """[(tie rank, candidate index, present)] of a tie scene's witnesses"""
    return [(k, int(meta['tie_index'][k]), E.has_site(out, s)) for k, s in zip(meta['witness_ranks'], meta['witness_sites'])]


def check_tie_scene(meta, out, max_det=300):
    r = meta['r']
    wit = tie_witnesses(meta, out)
    assert {r - 1, r} <= set(meta['witness_ranks'])
    for k, _, present in wit:
        assert present == (k < r), (k, r)
    inside = {i // E.SEL_CHUNK for _, i, p in wit if p}
    outside = {i // E.SEL_CHUNK for _, i, p in wit if not p}
    assert inside and outside and (len(inside | outside) > 1)
    assert out.shape[0] < max_det
    return wit


def perturbed(x, kw, **how):
    return E.finish(x, E.select(x[:, 4], **how), kw['iou_thres'])


# ------------------------------------------------------------------------------------------------ scene 1
@pytest.mark.parametrize('kind', E.CUT_KINDS)
def test_cut_scene_shows_the_cut(kind):
    pred, meta = E.cut_scene(kind)
    want, margins = E.cut_expected(kind)
    oracle = O.non_max_suppression(pred.clone(), **E.CUT_KW)
    assert all(same(a, b) for a, b in zip(want, oracle))
    assert E.margins_hold(margins), margins
    x, rows = E.candidates(pred[0], E.CUT_KW['conf_thres'])
    assert same(perturbed(x, E.CUT_KW), want[0])                           # the staged restatement is the reference
    assert E.candidates(pred[1], 0.25)[0].shape[0] <= E.MAX_NMS and want[1].shape[0] > 0 and want[2].shape[0] == 0
    assert all(w.shape[0] < 300 for w in want)
    if kind == 'ties':
        assert x.shape[0] == E.CUT_N and torch.equal(rows, torch.arange(E.CUT_N))      # candidate index = row index
        wit = check_tie_scene(meta, want[0])
        assert int((x[:, 4] == 0.5).sum()) == 3000 and int((x[:, 4] > 0.5).sum()) == 28500 and meta['r'] == 1500
        assert torch.equal(meta['tie_index'], meta['tie_rows'])
        ties = meta['tie_rows']
        for m in range(E.SEL_CHUNK, E.CUT_N, E.SEL_CHUNK):                  # the tied rows on each side of every chunk border
            k = int((ties < m).sum())
            assert {k - 1, k} <= set(meta['witness_ranks'])
        assert len(wit) >= 7 + 2 * 8 - 4
        assert len(meta['low_sites']) == 5 and not any(E.has_site(want[0], s) for s in meta['low_sites'])
        assert int(ties.min()) < E.SEL_CHUNK and int(ties.max()) >= E.CUT_N - E.SEL_CHUNK   # scattered over the whole image
        return
    present = [E.has_site(want[0], s) for s in meta['witness_sites']]
    if kind == 'exact':
        assert x.shape[0] == E.MAX_NMS and all(present)
        return
    assert x.shape[0] == (E.MAX_NMS + 1 if kind == 'plus1' else E.CUT_N)
    assert present == [k < E.MAX_NMS for k in meta['witness_ranks']] and E.MAX_NMS - 1 in meta['witness_ranks']
    chunk = [i // E.SEL_CHUNK for i in meta['witness_index']]
    assert len({c for c, p in zip(chunk, present) if p} | {c for c, p in zip(chunk, present) if not p}) > 1
    s = x[:, 4].sort(descending=True).values
    if kind == 'plus1':
        assert s[-4] == s[-1] and s[-5] > s[-4]
        assert meta['witness_index'] == sorted(meta['witness_index'])      # the one left out is the last of the tie in index order
    else:
        assert s.unique().numel() == s.numel()
        bits = s[E.MAX_NMS - 9:E.MAX_NMS + 9].view(torch.int32)
        assert (bits[:-1] - bits[1:] == (1 if kind == 'ulp' else 256)).all()
        if kind == 'ulp':
            assert (bits >> 8).unique().numel() == 1                        # one level-2 bin: the level-3 histogram alone decides


@pytest.mark.parametrize('mode', ['DIoU', 'soft'])
def test_cut_scene_under_the_other_rules(mode):
    pred, meta = E.cut_scene('ties')
    want, margins = E.cut_expected('ties', mode)
    assert E.margins_hold(margins) and 'thr' in margins, margins
    check_tie_scene(meta, want[0])
    base = E.cut_expected('ties')[0]
    assert all(same(a, b) for a, b in zip(want, base))                      # lattice boxes: every rule keeps the same rows, undecayed


@pytest.mark.parametrize('kind', ['ties', 'ulp', 'mid', 'plus1'])
def test_cut_scene_notices_a_wrong_selection(kind):
    pred, _ = E.cut_scene(kind)
    want = E.cut_expected(kind)[0][0]
    x, _ = E.candidates(pred[0], 0.25)
    assert not same(perturbed(x, E.CUT_KW, take=E.MAX_NMS + 1), want)       # (a) one too many
    assert not same(perturbed(x, E.CUT_KW, take=E.MAX_NMS - 1), want)       #     one too few
    if kind in ('ties', 'plus1'):
        assert not same(perturbed(x, E.CUT_KW, ties_descending=True), want)    # (b)


# ------------------------------------------------------------------------------------------------ scene 2
def test_multi_label_cut_scene():
    pred, meta = E.multi_cut_scene()
    want = E.multi_cut_expected()[0]
    x, rows = E.candidates(pred[0], 0.25, True)
    assert same(perturbed(x, E.MULTI_KW), want)
    check_tie_scene(meta, want)                                             # also: fewer than max_det = 300 rows
    assert int((x[:, 4] == 0.5).sum()) == 3000 and int((x[:, 4] > 0.5).sum()) == 28500
    tied = (x[:, 4] == 0.5).nonzero().view(-1)
    assert torch.equal(tied, meta['tie_index'])                             # candidate indices of the finished scene
    per_chunk = torch.bincount(torch.div(rows, 512, rounding_mode='floor'), minlength=8)
    print('entries per 512-row chunk:', per_chunk.tolist())
    assert per_chunk.numel() == 8 and int(per_chunk.min()) > 4096           # the emit's direct-store path, every chunk
    for m in range(E.SEL_CHUNK, x.shape[0], E.SEL_CHUNK):
        k = int((tied < m).sum())
        assert {k - 1, k} <= set(meta['witness_ranks'])
    for k, s in zip(meta['witness_ranks'], meta['witness_sites']):          # a witness row keeps its tied class alone
        row = pred[0, meta['tie_rows'][k], 5:]
        assert int((row > 0).sum()) == 1 and row[meta['tie_cls'][k]] == 0.5
    assert not same(perturbed(x, E.MULTI_KW, take=E.MAX_NMS + 1), want)
    assert not same(perturbed(x, E.MULTI_KW, take=E.MAX_NMS - 1), want)
    assert not same(perturbed(x, E.MULTI_KW, ties_descending=True), want)


# ------------------------------------------------------------------------------------------------ scene 3
@pytest.mark.parametrize('n', [n for n in E.ORDER_SIZES if n <= 4097])
def test_order_scene(n):
    boxes, scores = E.order_scene(n)
    want = E.order_expected(n)
    assert torch.equal(O.greedy_nms(boxes, scores, 0.45), want)             # disjoint: everything is kept, in rank order
    if n == 4097:
        m = {}
        assert torch.equal(R.penalised_nms(boxes, scores, 0.45, 'GIoU', margins=m), want) and E.margins_hold(m)
    if n >= 14:
        assert scores.min() < 0 < scores.max() and (scores * 64).frac().abs().max() == 0 and 32 < scores.unique().numel() <= 64
        zero = (scores == 0).nonzero().view(-1)
        pos = {int(i): p for p, i in enumerate(want.tolist())}
        assert [pos[int(i)] for i in zero] == list(range(pos[int(zero[0])], pos[int(zero[0])] + zero.numel()))   # +-0.0: one tie, in index order
        assert torch.signbit(scores[10:14]).tolist() == [False, True, True, False]


def test_order_scene_is_disjoint_at_30000():
    boxes, scores = E.order_scene(30000)
    cell = (boxes[:, 0] // 20).long() * 1000 + (boxes[:, 1] // 20).long()
    assert cell.unique().numel() == 30000 and ((boxes[:, 2:] - boxes[:, :2]) == 12).all() and (boxes[:, :2] % 20 == 4).all()
    assert E.order_expected(30000).numel() == 30000


# ------------------------------------------------------------------------------------------------ scene 4
@pytest.mark.parametrize('leaders,max_det', [(1100, m) for m in E.ROUNDS_MAX_DET] + [(700, 1024)])
def test_rounds_scene(leaders, max_det):
    pred, meta = E.rounds_scene(leaders)
    want, _, _ = E.rounds_expected(leaders, max_det)
    assert pred.shape[1] == leaders + 1500 < 3000
    assert want[0].shape[0] == min(leaders, max_det) and same(want[0], want[1])
    x, _ = E.candidates(pred[0], 0.25)
    assert x.shape[0] == leaders + 1500 and x[:, 4].unique().numel() == x.shape[0]
    drop = meta['follower_drop']
    assert int((drop > 1024).sum()) >= 100 and int((drop == 1).sum()) >= 250 and (drop > 0).all()
    # every output row is a leader, in score order: no follower got through
    lead_score = (0.95 - 4 * 2.0 ** -14 * torch.arange(leaders, dtype=torch.float64)).float()
    assert torch.equal(want[0][:, 4], lead_score[:want[0].shape[0]])
    assert len({tuple(b) for b in want[0][:, [0, 1, 5]].tolist()}) == want[0].shape[0]


def test_rounds_scene_merge():
    pred, _ = E.rounds_scene(1100)
    want, margins, info = E.rounds_expected(1100, 1024, True)
    assert E.margins_hold(margins) and 'merge' in margins
    assert all(r['n'] == 2600 and r['size'] is not None for r in info)
    assert 300 < want[0].shape[0] <= 400 and same(want[0][:, 4:], want[1][:, 4:])   # `redundant`: only leaders with followers stay


# ------------------------------------------------------------------------------------------------ scene 5
@pytest.mark.parametrize('nc', E.CARRY_NC)
def test_count_carry_scene(nc):
    pred, meta = E.carry_scene(nc)
    want = E.carry_expected(nc)[0]
    ch = meta['chunk_rows']
    n = pred.shape[1]
    assert (n + ch - 1) // ch == 258 > E.SCAN_WIDTH and n % ch
    x, rows = E.candidates(pred[0], 0.25)
    assert x.shape[0] == meta['n_cand'] and 550 <= x.shape[0] <= 650
    chunks = set(torch.div(rows, ch, rounding_mode='floor').tolist())
    assert {0, 255, 256, 257} <= chunks and len(chunks) > 100
    assert same(perturbed(x, E.CARRY_KW), want) and want.shape[0] < 300
    late = pred[0, meta['late'], 4]
    assert (meta['late'] >= 256 * ch).all() and all(bool((want[:, 4] == s).any()) for s in late)     # rows from chunks >= 256
    a, b = meta['pair'].tolist()
    assert a // ch == 255 and b // ch == 256 and pred[0, a, 4] == pred[0, b, 4]
    pa, pb = O.xywh2xyxy(pred[0, [a, b], :4])
    assert float(O.box_iou(pa[None], pb[None])) > 0.8 and not torch.equal(pa, pb)
    on_site = want[want[:, 4] == pred[0, a, 4]]
    assert on_site.shape[0] == 1 and torch.equal(on_site[0, :4], pa)        # the earlier one wins
    # (c) a scan without its carry
    lost = E.emit_without_carry(x, rows, ch)
    assert not same(perturbed(lost, E.CARRY_KW), want)
    # (b) the pair in the other order
    assert not same(perturbed(x, E.CARRY_KW, ties_descending=True), want)


# ------------------------------------------------------------------------------------------------ scene 6
def test_select_carry_scene():
    pred, meta = E.select_carry_scene()
    want = E.select_carry_expected()[0]
    x, _ = E.candidates(pred[0], 0.25, True)
    assert x.shape[0] > E.SELECT_CARRY_BORDER and (x.shape[0] + E.SEL_CHUNK - 1) // E.SEL_CHUNK > E.SCAN_WIDTH
    assert same(perturbed(x, E.MULTI_KW), want)
    check_tie_scene(meta, want)
    tied = (x[:, 4] == 0.5).nonzero().view(-1)
    assert torch.equal(tied, meta['tie_index']) and int((x[:, 4] > 0.5).sum()) == 28500
    r = meta['r']
    late = int((tied[:r] >= E.SELECT_CARRY_BORDER).sum())
    assert 0.4 * r <= late <= 0.6 * r, late
    k = int((tied < E.SELECT_CARRY_BORDER).sum())
    assert {k - 1, k} <= set(meta['witness_ranks']) and k - 1 < r           # witnesses on both sides of candidate 1,048,576
    assert not same(perturbed(x, E.MULTI_KW, take=E.MAX_NMS + 1), want)
    assert not same(perturbed(x, E.MULTI_KW, take=E.MAX_NMS - 1), want)
    assert not same(perturbed(x, E.MULTI_KW, ties_descending=True), want)
    lost = E.select_without_carry(x[:, 4])
    assert not same(E.finish(x, lost, 0.45), want)                          # (c)
