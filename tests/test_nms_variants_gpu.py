"""The NMS variants on the MI355X: penalised greedy NMS (GIoU / DIoU / CIoU / EIoU / SIoU), Soft-NMS and merge-NMS against the reference's
own outputs (tests/golden/nms_variants.npz) and against the plain-torch restatements (tests/nms_variants_ref.py) on fixed-seed clustered
inputs, through non_max_suppression, NMS and soft_nms.

Bars.  GIoU / DIoU / EIoU: torch.equal on indices and rows everywhere, exact duplicates, score ties and zero-size boxes included (their
arithmetic is + - * / min max).  CIoU / SIoU / Soft-NMS go through atan / asin / cos / exp, so the bar is index-exact on inputs whose every
decision keeps MIN_MARGIN fp32 spacings from flipping (a condition on the inputs, chosen on the CPU beforehand and re-asserted here);
decayed scores against the restatement in fp64 on the same fp32 inputs: |got - want64| <= max(2 x the fp32 restatement's own error,
16 fp32 roundings of the value).  Merge: membership, the `redundant` filter, conf and class exact; each merged coordinate within
(k + 8) * 2^-24 * max|x| of the fp64 restatement (k the row's cluster size, max|x| over the candidates' coordinates): the worst case of
a k-term non-negative weighted mean in fp32 in any summation order.
Every test here uses a keyword or a function the feature adds."""
import pytest
import torch

import nms_variants_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
EXACT = ('GIoU', 'DIoU', 'EIoU')


def assert_values(got, want64, ref32, what):
    """|got - want64| <= max(2 x max |ref32 - want64|, 16 * 2^-24 * |want64|), elementwise."""
    got, want64, ref32 = got.detach().cpu().double(), want64.double(), ref32.double()
    e_ref = (ref32 - want64).abs().max().item() if want64.numel() else 0.0
    allow = torch.maximum(torch.full_like(want64, 2 * e_ref), 16 * 2.0 ** -24 * want64.abs())
    err = (got - want64).abs()
    print(f'{what}: max error {err.max().item() if err.numel() else 0.0:.3e}, the fp32 restatement\'s own {e_ref:.3e}, '
          f'worst ratio to the bar {(err / allow.clamp_min(1e-300)).max().item() if err.numel() else 0.0:.2f}')
    assert (err <= allow).all(), what


def product(pred, kw):
    from somi_amd.nms import non_max_suppression
    kw = dict(kw)
    if kw.get('labels'):
        kw['labels'] = [l.cuda() for l in kw['labels']]
    return non_max_suppression(pred.cuda(), **kw)


# ------------------------------------------------------------------------------------------------ the reference's own outputs
@pytest.mark.parametrize('mode', R.PENALISED)
def test_NMS_matches_the_reference(golden, mode):
    from somi_amd.nms import NMS
    g = golden('nms_variants')
    keep = NMS(T(g['nms_boxes']).cuda(), T(g['nms_scores']).cuda(), float(g['nms_thr']), class_nms=mode)
    assert keep.dtype == torch.int64 and keep.is_cuda
    assert torch.equal(keep.cpu(), T(g[f'nms_keep_{mode}']))


@pytest.mark.parametrize('tag', ['soft_a', 'soft_b'])
def test_soft_nms_matches_the_reference(golden, tag):
    from somi_amd.nms import soft_nms
    g = golden('nms_variants')
    boxes, scores = T(g[f'{tag}_boxes']), T(g[f'{tag}_scores'])
    thr, sigma, sthr = (float(v) for v in g[f'{tag}_params'])
    ref_keep, ref_scores = T(g[f'{tag}_keep']), T(g[f'{tag}_decayed'])
    s = scores.cuda()
    keep = soft_nms(boxes.cuda(), s, thr, sigma, sthr)
    assert keep.dtype == torch.int64 and keep.is_cuda
    s32, s64 = scores.clone(), scores.double()
    want = R.soft_nms(boxes, s32, thr, sigma, sthr)
    want64 = R.soft_nms(boxes.double(), s64, thr, sigma, sthr)
    assert torch.equal(want, want64)
    assert torch.equal(keep.cpu(), want)                                   # the reference's picks plus at most its last candidate
    assert torch.equal(keep.cpu()[:ref_keep.numel()], ref_keep) and keep.numel() - ref_keep.numel() in (0, 1)
    assert_values(s, s64, s32, f'{tag} decayed scores')                    # in place, every candidate
    assert_values(s[ref_keep.cuda()], s64[ref_keep], ref_scores[ref_keep], f'{tag} kept scores against the reference')


def test_merge_matches_the_reference(golden):
    g = golden('nms_variants')
    pred = T(g['merge_pred'])
    kw = dict(conf_thres=0.02, iou_thres=0.5, multi_label=True, merge=True)
    got = product(pred, kw)
    info = []
    want64 = R.non_max_suppression(pred.clone(), dtype=torch.float64, info=info, **kw)
    for b in range(2):
        ref = T(g[f'merge_out{b}'])
        assert got[b].shape == ref.shape and torch.equal(got[b][:, 4:].cpu(), ref[:, 4:]), f'image {b}: membership / conf / class'
    assert torch.equal(got[1].cpu(), T(g['merge_out1']))                   # >= 3000 candidates: unmerged, bit for bit
    bound = (info[0]['size'].double() + 8)[:, None] * 2.0 ** -24 * info[0]['xmax']
    err = (got[0][:, :4].cpu().double() - want64[0][:, :4]).abs()
    print(f'merge: worst coordinate error at {(err / bound).max().item():.2f} of the bound')
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ differential, whole pipeline
PIPELINE = [(tag, mode) for tag, (_, modes, _, _) in R.PIPELINE_CASES.items() for mode in modes]


@pytest.mark.parametrize('tag,mode', PIPELINE)
def test_pipeline_matches_the_restatement(tag, mode):
    margins, info = {}, []
    pred, kw, want = R.run_case(tag, mode, margins=margins, info=info)
    assert all(v >= R.MIN_MARGIN for v in margins.values()), margins      # the condition on the inputs
    merge = kw['merge']
    got = product(pred, kw)
    assert len(got) == len(want)
    assert sum(int(w.shape[0]) for w in want) > 0 and want[2].shape[0] == 0     # image 2 has no candidates
    for b, (o, w) in enumerate(zip(got, want)):
        assert o.shape == w.shape, (tag, mode, b, o.shape, w.shape)
    if mode != 'soft' and not merge:
        for b, (o, w) in enumerate(zip(got, want)):                        # rows are copies of candidates: exact in every greedy mode
            assert torch.equal(o.cpu(), w), (tag, mode, b)
        return
    info64 = []
    _, _, want64 = R.run_case(tag, mode, dtype=torch.float64, info=info64)
    for b, (o, w, w64) in enumerate(zip(got, want, want64)):
        assert w64.shape == w.shape
        o = o.cpu()
        assert torch.equal(o[:, 5], w[:, 5]), (tag, mode, b)
        if mode == 'soft':
            assert torch.equal(o[:, :4], w[:, :4]), (tag, mode, b)
            assert_values(o[:, 4], w64[:, 4], w[:, 4], f'{tag} image {b} decayed scores')
        else:
            assert torch.equal(o[:, 4], w[:, 4]), (tag, mode, b)
            if info[b]['size'] is None:                                    # outside the size window: unmerged
                assert torch.equal(o, w), (tag, mode, b)
                continue
            bound = (info[b]['size'].double() + 8)[:, None] * 2.0 ** -24 * info[b]['xmax']
            assert ((o[:, :4].double() - w64[:, :4]).abs() <= bound).all(), (tag, mode, b)
    if merge:
        n = [r['n'] for r in info]
        assert any(1 < v < 3000 for v in n) and any(v >= 3000 or v <= 1 for v in n)


def tie_boxes(n, seed):
    """Clustered boxes with exact duplicate rows, exact score ties and zero-size boxes."""
    g = torch.Generator().manual_seed(seed)
    k = n // 5
    centre, size = torch.rand(k, 2, generator=g) * 320, torch.rand(k, 2, generator=g) * 50 + 6
    which = torch.randint(0, k, (n,), generator=g)
    c = centre[which] + torch.randn(n, 2, generator=g) * 3
    wh = size[which] * (1 + 0.2 * torch.randn(n, 2, generator=g)).clamp(0.4, 1.8)
    boxes = torch.cat((c - wh / 2, c + wh / 2), 1)
    scores = (torch.rand(n, generator=g) * 64).floor() / 64 + 1 / 128      # 64 distinct values: ties everywhere
    boxes[20:30] = boxes[20]                                               # duplicates with different scores
    boxes[40:50] = boxes[40]
    scores[40:50] = scores[40]                                             # ... and with the same score
    boxes[60:64, 2:] = boxes[60:64, :2]                                    # zero-size
    boxes[64:68, 2] = boxes[64:68, 0]                                      # zero width
    boxes[68:72] = boxes[68]
    boxes[68:72, 3] = boxes[68, 1]                                         # zero height, duplicated
    return boxes, scores


@pytest.mark.parametrize('mode', EXACT)
def test_exact_modes_on_ties_duplicates_and_zero_size_boxes(mode):
    from somi_amd.nms import NMS
    for n, thr, seed in ((700, 0.45, 5), (1500, 0.2, 6)):
        boxes, scores = tie_boxes(n, seed)
        want = R.penalised_nms(boxes, scores, thr, mode)
        keep = NMS(boxes.cuda(), scores.cuda(), thr, class_nms=mode)
        assert torch.equal(keep.cpu(), want), (mode, n)
        assert 0 < want.numel() < n
    # the same through the pipeline: duplicate rows, tied confidences, zero-size boxes, a near-duplicate cluster
    pred = R.clustered_pred(11, n=600, nc=3, live=(600, 300, 0))
    pred[0, 100:110] = pred[0, 100]
    pred[0, 120:130, 4:] = pred[0, 120, 4:]
    pred[0, 140:150, 2:4] = 0
    pred[1, 10:20, 2] = 0
    pred[..., 4] = (pred[..., 4] * 32).floor() / 32
    pred[..., 5:] = (pred[..., 5:] * 16).ceil() / 16
    for kw in (dict(conf_thres=0.1, iou_thres=0.45, multi_label=True), dict(conf_thres=0.25, iou_thres=0.3, agnostic=True)):
        want = R.non_max_suppression(pred.clone(), nms=mode, **kw)
        got = product(pred, dict(kw, nms=mode))
        for b, (o, w) in enumerate(zip(got, want)):
            assert o.shape == w.shape and torch.equal(o.cpu(), w), (mode, kw, b)


def test_two_launches_are_bit_identical():
    from somi_amd.nms import NMS, soft_nms
    pred, kw, _ = R.run_case('merge', 'iou')
    p = pred.cuda()
    for mode in R.MODES:
        for merge in (False, True):
            if merge and mode == 'soft':
                continue
            k = dict(kw, nms=mode, merge=merge)
            a, b = product(p, k), product(p, k)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (mode, merge)
    boxes, scores = tie_boxes(900, 9)
    for mode in R.PENALISED:
        assert torch.equal(NMS(boxes.cuda(), scores.cuda(), 0.4, mode), NMS(boxes.cuda(), scores.cuda(), 0.4, mode))
    order = torch.argsort(scores, descending=True, stable=True)
    s1, s2 = scores[order].cuda(), scores[order].cuda()
    assert torch.equal(soft_nms(boxes[order].cuda(), s1), soft_nms(boxes[order].cuda(), s2)) and torch.equal(s1, s2)


def test_soft_nms_edge_cases():
    """One box is kept (the reference returns nothing); no boxes give no indices; an exact tie goes to the lowest index."""
    from somi_amd.nms import NMS, soft_nms
    b = torch.tensor([[10., 10., 50., 60.], [200., 200., 240., 260.], [400., 10., 450., 60.]]).cuda()
    assert soft_nms(b[:1].contiguous(), torch.tensor([0.9]).cuda()).tolist() == [0]
    assert soft_nms(b, torch.tensor([0.9, 0.5, 0.5]).cuda()).tolist() == [0, 1, 2]
    assert soft_nms(b, torch.tensor([0.9, 0.2, 0.5]).cuda()).tolist() == [0, 2]
    assert soft_nms(b[:0], torch.zeros(0).cuda()).numel() == 0 and NMS(b[:0], torch.zeros(0).cuda(), 0.5).numel() == 0
    assert NMS(b, torch.tensor([0.1, 0.9, 0.5]).cuda(), 0.5, 'DIoU').tolist() == [1, 2, 0]
    out = product(torch.tensor([[[30., 35., 40., 50., 0.9, 0.8, 0.1]]]), dict(nms='soft'))
    assert out[0].shape == (1, 6)                                          # an image with a single detection keeps it


# the cases of tests/test_nms_gpu.py
DEFAULT_CASES = dict(default=dict(conf_thres=0.25, iou_thres=0.45),
                     val=dict(conf_thres=0.4, iou_thres=0.2, multi_label=True),
                     bench=dict(conf_thres=0.001, iou_thres=0.6, multi_label=True),
                     agnostic=dict(conf_thres=0.3, iou_thres=0.5, agnostic=True),
                     classes=dict(conf_thres=0.2, iou_thres=0.45, classes=[1, 3, 7]),
                     maxdet=dict(conf_thres=0.05, iou_thres=0.9, multi_label=True, max_det=20),
                     none=dict(conf_thres=0.9999, iou_thres=0.45))


@pytest.mark.parametrize('tag', list(DEFAULT_CASES))
def test_default_mode_is_todays_call(golden, tag):
    from somi_amd.nms import non_max_suppression
    g = golden('nms')
    pred = T(g['pred']).cuda()
    today = non_max_suppression(pred, **DEFAULT_CASES[tag])
    out = non_max_suppression(pred, nms='iou', merge=False, **DEFAULT_CASES[tag])
    for b, (o, t) in enumerate(zip(out, today)):
        assert torch.equal(o, t) and torch.equal(o.cpu(), T(g[f'{tag}_{b}'])), (tag, b)
