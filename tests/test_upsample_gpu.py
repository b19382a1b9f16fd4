"""The two learned 2x upsamplers of the neck on the MI355X (upsample.hip): the four kernels against the fp64 CPU restatement
(tests/upsample_ref.py) under torch autograd - channel slices of wider tensors, maps smaller than the halo, odd sizes, channel counts that fill
neither a wave nor one 64-channel chunk and more than one chunk - the blocks against torch autograd on the restatement, and whole graphs (BiFPN and
Concat consumers) against the oracle Model.  Bar: 1e-3 relative (BASELINE) through parity.rel_close, atol 1e-5 where the expected tensor is
analytically zero; untouched channels and repeated launches bit for bit."""
import copy

import pytest
import torch

import upsample_ref as R
from parity import check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nchw, nhwc, rel_close

pytestmark = pytest.mark.gpu

CASES = [(1, 4, 1, 1), (1, 4, 2, 3), (2, 12, 5, 7), (3, 36, 9, 11), (1, 132, 13, 6)]
_ids = lambda c: 'x'.join(map(str, c))                            # noqa: E731


def _zero_atol(want):
    return 1e-5 if not want.any() else 0.0


def _close(got, want, what):
    rel_close(got, want, what=what, atol=_zero_atol(want))


def _carafe_case(case, k, scale, seed):
    """-> the wide host tensors and the fp64 results: out, dx, dlogits, softmax weights per output pixel."""
    B, C, H, W = case
    kk = k * k
    gen = torch.Generator().manual_seed(seed)
    xb = torch.randn(B, H, W, C + 12, generator=gen)
    lb = torch.randn(B, H, W, 4 * kk + 8, generator=gen) * scale
    dyb = torch.randn(B, 2 * H, 2 * W, C + 8, generator=gen)
    x64 = nchw(xb[..., 4:4 + C]).double().contiguous().requires_grad_(True)
    l64 = nchw(lb[..., 4:4 + 4 * kk]).double().contiguous().requires_grad_(True)
    out64 = R.carafe_reassemble(x64, l64, k)
    out64.backward(nchw(dyb[..., 4:4 + C]).double())
    p64 = torch.softmax(l64.detach().view(B, kk, 4, H, W), 1)     # [b, tap, dy*2+dx, h, w] -> (B, 2H, 2W, kk)
    p64 = p64.view(B, kk, 2, 2, H, W).permute(0, 4, 2, 5, 3, 1).reshape(B, 2 * H, 2 * W, kk)
    return xb, lb, dyb, nhwc(out64.detach()), nhwc(x64.grad), nhwc(l64.grad), p64


@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_carafe_kernels(case, k):
    """somi_carafe_nhwc_f32 / somi_carafe_bwd_nhwc_f32 against fp64: output, saved softmax weights, dx and dlogits, every tensor a slice of a wider
    one at a non-zero offset; channels outside the written slices stay bit-identical; the eval form (no weights) writes the same output; two
    launches are bit-identical."""
    from somi_amd import ops
    B, C, H, W = case
    kk = k * k
    xb, lb, dyb, out64, dx64, dl64, p64 = _carafe_case(case, k, 1.0, sum(case) + k)
    xg, lg, dyg = xb.cuda(), lb.cuda(), dyb.cuda()
    og = torch.full((B, 2 * H, 2 * W, C + 16), 7.0).cuda()
    _, wts = ops.carafe(xg, lg, C, k, 4, 4, out=og, y_coff=8, weights=True)
    _close(og[..., 8:8 + C], out64, f'carafe k{k} out')
    assert (og[..., :8] == 7).all() and (og[..., 8 + C:] == 7).all(), 'channels outside the output slice were written'
    assert tuple(wts.shape) == (B, 2 * H, 2 * W, kk)
    _close(wts, p64, f'carafe k{k} softmax weights')
    og2 = torch.full((B, 2 * H, 2 * W, C + 16), 7.0).cuda()
    ops.carafe(xg, lg, C, k, 4, 4, out=og2, y_coff=8)             # eval form
    assert torch.equal(og, og2), 'the eval form differs from the training form'
    runs = []
    for _ in range(2):
        dxg = torch.full((B, H, W, C + 8), 3.0).cuda()
        dlg = torch.full((B, H, W, 4 * kk + 8), 5.0).cuda()
        ops.carafe_backward(dyg, xg, wts, C, k, 4, 4, out=dxg, dx_coff=4, dlogits=dlg, dl_coff=4)
        runs.append((dxg, dlg))
    dxg, dlg = runs[0]
    _close(dxg[..., 4:4 + C], dx64, f'carafe k{k} dx')
    _close(dlg[..., 4:4 + 4 * kk], dl64, f'carafe k{k} dlogits')
    assert (dxg[..., :4] == 3).all() and (dxg[..., 4 + C:] == 3).all(), 'channels outside the dx slice were written'
    assert (dlg[..., :4] == 5).all() and (dlg[..., 4 + 4 * kk:] == 5).all(), 'channels outside the dlogits slice were written'
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), 'two launches differ'
    og3 = torch.full((B, 2 * H, 2 * W, C + 16), 7.0).cuda()
    ops.carafe(xg, lg, C, k, 4, 4, out=og3, y_coff=8)
    assert torch.equal(og, og3), 'two forward launches differ'
    assert torch.equal(xg.cpu(), xb) and torch.equal(lg.cpu(), lb) and torch.equal(dyg.cpu(), dyb), 'an input was written'


@pytest.mark.parametrize('k', [3, 5])
def test_carafe_softmax_subtracts_the_maximum(k):
    """Logits scaled by 200 (exp would overflow fp32 without the subtraction): finite and at the bar, forward and backward."""
    from somi_amd import ops
    case = (2, 12, 5, 7)
    B, C, H, W = case
    kk = k * k
    xb, lb, dyb, out64, dx64, dl64, p64 = _carafe_case(case, k, 200.0, 77 + k)
    assert lb.abs().max() > 400
    og = torch.full((B, 2 * H, 2 * W, C + 16), 7.0).cuda()
    _, wts = ops.carafe(xb.cuda(), lb.cuda(), C, k, 4, 4, out=og, y_coff=8, weights=True)
    _close(og[..., 8:8 + C], out64, f'carafe k{k} x200 out')
    _close(wts, p64, f'carafe k{k} x200 softmax weights')
    dxg, dlg = ops.carafe_backward(dyb.cuda(), xb.cuda(), wts, C, k, 4, 4)
    _close(dxg, dx64, f'carafe k{k} x200 dx')
    _close(dlg, dl64, f'carafe k{k} x200 dlogits')


def _groups_for(C):
    """groups 1 and the largest of {2, 4} that keeps (C / groups) % 4 == 0."""
    return [1] + [g for g in (4, 2) if C % g == 0 and (C // g) % 4 == 0][:1]


# the issue's five shapes (every one admits groups = 1 only) and three more that admit 2 and 4 groups, so that the group indexing runs at kernel level
DYS_CASES = [(c, g) for c in CASES + [(2, 16, 5, 7), (3, 40, 9, 11), (1, 136, 4, 6)] for g in _groups_for(c[1])]


def _init_pos(G):
    return torch.tensor([-0.25, 0.25, -0.25, 0.25] * G + [-0.25, -0.25, 0.25, 0.25] * G)


def _dysample_case(case, G, reach, seed0):
    """Offsets from a seeded generator, scaled so that |0.25 * o + init_pos| reaches `reach` pixels.  The seed is the first from seed0 on for which
    no unclamped sampling coordinate lies within 1e-4 pixel of an integer (a hundred times fp32's error on a coordinate of order 1: there the
    fp32 kernel and the fp64 reference take the same bilinear cell); nothing is excluded, and the condition is asserted."""
    B, C, H, W = case
    ip = _init_pos(G)
    for seed in range(seed0, seed0 + 200):
        gen = torch.Generator().manual_seed(seed)
        ob = torch.randn(B, H, W, 8 * G + 8, generator=gen)
        ob = ob / ob.abs().max() * (reach - 0.25) * 4 * 0.991    # not the round figure: the largest offset must not land on a pixel centre
        sx, sy = R.dysample_coords(nchw(ob[..., 4:4 + 8 * G]).double(), ip.double().view(1, -1, 1, 1), G)
        ux, uy = (sx >= 0) & (sx <= W - 1), (sy >= 0) & (sy <= H - 1)     # the border itself counts as unclamped here: it is an integer
        dist = torch.cat([(sx - sx.round()).abs()[ux], (sy - sy.round()).abs()[uy]])
        if dist.numel() == 0 or dist.min() > 1e-4:
            break
    assert dist.numel() == 0 or dist.min() > 1e-4, 'no seed keeps the unclamped coordinates away from the integers'
    clamped = 1 - (ux.float().mean().item() + uy.float().mean().item()) / 2
    xb = torch.randn(B, H, W, C + 12, generator=gen)
    dyb = torch.randn(B, 2 * H, 2 * W, C + 8, generator=gen)
    x64 = nchw(xb[..., 4:4 + C]).double().contiguous().requires_grad_(True)
    o64 = nchw(ob[..., 4:4 + 8 * G]).double().contiguous().requires_grad_(True)
    out64 = R.dysample_sample(x64, o64, ip.double().view(1, -1, 1, 1), G)
    out64.backward(nchw(dyb[..., 4:4 + C]).double())
    print(f'dysample {case} G{G}: seed {seed}, {100 * clamped:.1f} % of coordinates clamped, nearest integer at {dist.min().item() if dist.numel() else float("nan"):.2e}')
    return xb, ob, dyb, ip, nhwc(out64.detach()), nhwc(x64.grad), nhwc(o64.grad)


@pytest.mark.parametrize('case,G', DYS_CASES, ids=[_ids(c) + f'g{g}' for c, g in DYS_CASES])
def test_dysample_kernels(case, G):
    """somi_dysample_nhwc_f32 / somi_dysample_bwd_nhwc_f32 against fp64 with offsets that reach about 1.5 pixels (the border clamp is exercised):
    output, dx and doffset (0 where the coordinate was clamped), every tensor a slice of a wider one at a non-zero offset; channels outside the
    written slices stay bit-identical; no far tap; two launches are bit-identical."""
    from somi_amd import ops
    B, C, H, W = case
    xb, ob, dyb, ip, out64, dx64, do64 = _dysample_case(case, G, 1.5, 1000 + sum(case) + G)
    xg, og_, dyg, ipg = xb.cuda(), ob.cuda(), dyb.cuda(), ip.cuda()
    outs = []
    for _ in range(2):
        yg = torch.full((B, 2 * H, 2 * W, C + 16), 7.0).cuda()
        ops.dysample(xg, og_, ipg, C, G, 4, 4, out=yg, y_coff=8)
        outs.append(yg)
    yg = outs[0]
    _close(yg[..., 8:8 + C], out64, f'dysample G{G} out')
    assert (yg[..., :8] == 7).all() and (yg[..., 8 + C:] == 7).all(), 'channels outside the output slice were written'
    assert torch.equal(outs[0], outs[1]), 'two forward launches differ'
    runs = []
    for _ in range(2):
        dxg = torch.full((B, H, W, C + 8), 3.0).cuda()
        dog = torch.full((B, H, W, 8 * G + 8), 5.0).cuda()
        ops.dysample_backward(dyg, xg, og_, ipg, C, G, 4, 4, 4, out=dxg, dx_coff=4, doffset=dog, df_coff=4)
        assert ops.dysample_far_taps() == 0, 'a tap within 2 pixels of its source pixel went through an atomic'
        runs.append((dxg, dog))
    dxg, dog = runs[0]
    _close(dxg[..., 4:4 + C], dx64, f'dysample G{G} dx')
    _close(dog[..., 4:4 + 8 * G], do64, f'dysample G{G} doffset')
    assert (dxg[..., :4] == 3).all() and (dxg[..., 4 + C:] == 3).all(), 'channels outside the dx slice were written'
    assert (dog[..., :4] == 5).all() and (dog[..., 4 + 8 * G:] == 5).all(), 'channels outside the doffset slice were written'
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), 'two launches differ'
    assert torch.equal(xg.cpu(), xb) and torch.equal(og_.cpu(), ob) and torch.equal(dyg.cpu(), dyb), 'an input was written'


def test_dysample_far_taps_are_counted_and_still_correct():
    """Offsets scaled to 4 pixels on (2, 12, 9, 11): some corners land more than 2 pixels from their source pixel, go to dx as fp32 atomics and
    are counted; dx and doffset still meet the bar (bit-identity is not claimed there)."""
    from somi_amd import ops
    case, G = (2, 12, 9, 11), 1
    B, C, H, W = case
    xb, ob, dyb, ip, out64, dx64, do64 = _dysample_case(case, G, 4.0, 2000)
    ops.reset_dysample_far_taps()
    _close(ops.dysample(xb.cuda(), ob.cuda(), ip.cuda(), C, G, 4, 4), out64, 'dysample 4 px out')
    dxg, dog = ops.dysample_backward(dyb.cuda(), xb.cuda(), ob.cuda(), ip.cuda(), C, G, 4, 4, 4)
    far = ops.dysample_far_taps()
    print(f'far taps: {far}')
    assert far > 0 and ops.dysample_far_taps(total=True) == far
    _close(dxg, dx64, 'dysample 4 px dx')
    _close(dog[..., :8 * G], do64, 'dysample 4 px doffset')


BLOCKS = {'carafe': (lambda M: M.CARAFE(32, 3, 5), (2, 32, 7, 9)), 'carafe_k3': (lambda M: M.CARAFE(16, 1, 3, 16), (2, 16, 6, 5)),
          'dysample': (lambda M: M.DySample(32), (2, 32, 7, 9)), 'dysample_g2': (lambda M: M.DySample(24, 2, 'lp', 2), (2, 24, 6, 5))}


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_upsample_blocks_eval_train_backward(tag):
    """The four fixture configurations: eval forward (BatchNorm folded), training forward, hand-written backward against torch autograd on the CPU
    restatement - output, dx, every parameter gradient and the updated running statistics."""
    from somi_amd import ops
    mk, shape = BLOCKS[tag]
    check_block(mk, R, shape, tag)
    if tag.startswith('dysample'):
        assert ops.dysample_far_taps() == 0


def _graph_cfg(graph, up):
    from somi_amd.configs import UPSAMPLE_ROWS, tiny_somi_cfg, yolov5_cfg
    if graph == 'yolov5':
        return yolov5_cfg(0.25, 0.33, nc=10, upsample=up)
    cfg = tiny_somi_cfg()
    rows = [i for i, r in enumerate(cfg['head']) if r[2] == 'nn.Upsample']
    assert len(rows) == 1
    cfg['head'][rows[0]] = [-1, 1, *copy.deepcopy(UPSAMPLE_ROWS[up])]
    return cfg


@pytest.mark.parametrize('up', ['carafe', 'dysample'])
@pytest.mark.parametrize('graph', ['tiny_somi', 'yolov5'])
def test_upsample_graph_training_step_eval_and_checkpoint(graph, up, monkeypatch):
    """tiny_somi_cfg (the upsampler feeds a BiFPN) and yolov5 at width 0.25 / depth 0.33 (both feed a Concat), batch 2, 64x64, against the oracle
    Model built through the upsample_ref registration: one training forward, ComputeLoss and backward (outputs, loss, every parameter gradient,
    BatchNorm statistics), the eval forward, two fresh TrainStep.step runs bit-identical, attempt_load of a pickled oracle model."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd import blocks as MB
    from somi_amd import ops
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = _graph_cfg(graph, up)
    ref = fill_state(OModel(cfg), 3)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    n_up = sum(isinstance(m, MB.CARAFE if up == 'carafe' else MB.DySample) for m in mine.model)
    assert n_up == (1 if graph == 'tiny_somi' else 2) and not any(isinstance(m, MB.Upsample) for m in mine.model)
    ref.hyp = mine.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 64, nc=10, seed=2)
    what = f'{graph}+{up}'
    # ODConv_3rd's conv.reduction is unused in the reference's forward (and here), so autograd leaves it without a gradient on both sides, which
    # check_train_step does not allow for: it starts from an explicit zero gradient on both sides, and must still hold exactly zero afterwards
    unused = [n for n, _ in ref.named_parameters() if '.conv.reduction.' in n]
    assert bool(unused) == (graph == 'tiny_somi')
    for mod in (ref, mine):
        for n, p in mod.named_parameters():
            if n in unused:
                p.grad = torch.zeros_like(p)
    ops.reset_dysample_far_taps()
    check_train_step(ref, mine, imgs, targets, what)
    for mod in (ref, mine):
        assert not any(p.grad.any() for n, p in mod.named_parameters() if n in unused), 'an unused parameter received a gradient'
    check_eval(ref, mine, imgs, what)
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    assert ops.dysample_far_taps(total=True) == 0
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'upsample_ref'), what)
