"""The remaining stock hub graphs on the MI355X (models/hub/yolov3*.yaml, yolov5-fpn / -panet / -p6 / -p7.yaml): the max-pool kernels of pool.hip
against torch's max_pool2d and its autograd on the CPU in fp64, the new blocks against torch autograd on the CPU restatement
(tests/hub_ref.py), the five-level loss against the oracle loss, whole graphs against the oracle Model.  Bars: selection (values, arg-max
codes) exact; pool gradients n roundings of the sum of their terms' magnitudes, n the number of terms; blocks and graphs 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import hub_ref as R
from parity import (check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nchw, nhwc,
                    rel_close)

pytestmark = pytest.mark.gpu


def _tie_map(B, H, W, C, gen, kind):
    """Inputs with exact ties: 'const' a constant map, 'quant' a map quantised to a few values with a constant patch, 'neg' negative
    everywhere (a zero border wins over it) with ties, 'rand' plain noise."""
    x = torch.randn(B, H, W, C, generator=gen)
    if kind == 'const':
        x = torch.full_like(x, -0.2)
    elif kind == 'quant':
        x = (x * 1.5).round() / 2
        x[:, : max(H // 2, 1), : max(W // 2, 1)] = 0.5
    elif kind == 'neg':
        x = -((x * 2).round().abs() / 4) - 0.25
    return x


POOL2 = [(2, 8, 8, 8, 2, (0, 0, 0, 0)), (2, 7, 9, 16, 2, (0, 0, 0, 0)), (1, 5, 5, 8, 1, (0, 1, 0, 1)), (2, 3, 3, 4, 1, (0, 1, 0, 1)),
         (2, 6, 5, 72, 1, (0, 1, 0, 1)), (1, 9, 4, 12, 2, (0, 1, 0, 1)), (3, 2, 2, 4, 2, (0, 0, 0, 0)), (1, 1, 1, 8, 1, (0, 1, 0, 1)),
         (2, 4, 6, 8, 1, (0, 0, 0, 0)), (1, 6, 6, 8, 1, (1, 1, 1, 1)), (1, 13, 11, 20, 2, (1, 0, 1, 0))]


@pytest.mark.parametrize('kind', ['rand', 'const', 'quant', 'neg'])
@pytest.mark.parametrize('case', POOL2, ids=lambda c: 'x'.join(map(str, c[:5])) + 'p' + ''.join(map(str, c[5])))
def test_maxpool2_kernels(case, kind):
    """nn.MaxPool2d(2, s, 0) over a zero pad folded into the read, slices of wider tensors: values and arg-max codes equal torch's (CPU, fp64)
    exactly; the gradient equals autograd's bit for bit at stride 2 (windows do not overlap: no sums) and within 4 roundings of the terms'
    magnitudes at stride 1; untouched channels stay; two launches are bit-identical."""
    from somi_amd import ops
    B, H, W, C, s, pad = case
    gen = torch.Generator().manual_seed(sum(case[:5]) + len(kind))
    xoff, yoff = 4, 8
    xb = torch.randn(B, H, W, C + 12, generator=gen)
    xb[..., xoff:xoff + C] = _tie_map(B, H, W, C, gen, kind)
    x64 = nchw(xb[..., xoff:xoff + C]).double().contiguous().requires_grad_(True)
    xp = F.pad(x64, pad)
    y64, idx = F.max_pool2d(xp, 2, s, 0, return_indices=True)
    Ho, Wo, Wp = y64.shape[2], y64.shape[3], xp.shape[3]
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    codes64 = ((idx // Wp - ho * s) * 2 + (idx % Wp - wo * s)).to(torch.uint8)
    out = torch.full((B, Ho, Wo, C + 16), 7.0)
    og = out.cuda()
    _, codes = ops.maxpool2(xb.cuda(), C, xoff, stride=s, pad=pad, out=og, y_coff=yoff, codes=True)
    assert torch.equal(og[..., yoff:yoff + C].cpu().double(), nhwc(y64.detach())), 'values'
    assert torch.equal(codes.view(B, Ho, Wo, C).cpu(), nhwc(codes64)), 'arg-max codes'
    assert (og[..., :yoff] == 7).all() and (og[..., yoff + C:] == 7).all(), 'channels outside the slice were written'
    og2 = torch.full((B, Ho, Wo, C + 16), 7.0).cuda()
    ops.maxpool2(xb.cuda(), C, xoff, stride=s, pad=pad, out=og2, y_coff=yoff)          # eval form: no codes
    assert torch.equal(og, og2)
    dyb = torch.randn(B, Ho, Wo, C + 8, generator=gen)
    dy = nchw(dyb[..., 4:4 + C]).double()
    y64.backward(dy)
    dx64 = x64.grad.clone()
    x64.grad = None
    F.max_pool2d(F.pad(x64, pad), 2, s, 0).backward(dy.abs())
    mag = x64.grad
    dxb = torch.full((B, H, W, C + 8), 3.0).cuda()
    ops.maxpool2_backward(dyb.cuda(), codes, C, H, W, 4, stride=s, pad=pad, out=dxb, dx_coff=4)
    got = nchw(dxb[..., 4:4 + C]).cpu().double()
    if s == 2:
        assert torch.equal(got, dx64), 'stride-2 gradient is a pure scatter: bit for bit'
    else:
        bar = 4 * 2.0 ** -24 * mag
        worst = ((got - dx64).abs() - bar).max().item()
        print(f'k2/s1 dx: worst excess over the bar {worst:.3e}')
        assert ((got - dx64).abs() <= bar).all(), f'dx beyond 4 roundings of its terms by {worst:.3e}'
    assert (dxb[..., :4] == 3).all() and (dxb[..., 4 + C:] == 3).all()
    dxb2 = torch.full((B, H, W, C + 8), 3.0).cuda()
    ops.maxpool2_backward(dyb.cuda(), codes, C, H, W, 4, stride=s, pad=pad, out=dxb2, dx_coff=4)
    assert torch.equal(dxb, dxb2)


def test_zero_pad_wins_over_negative_activations_and_drops_their_gradient():
    """A 3x3 map of -0.2 through ZeroPad2d([0, 1, 0, 1]) + MaxPool2d(2, 1, 0): 0 in the last row and column, no gradient for them."""
    from somi_amd import ops
    x = torch.full((1, 3, 3, 4), -0.2).cuda()
    y, codes = ops.maxpool2(x, 4, stride=1, pad=(0, 1, 0, 1), codes=True)
    want = torch.full((3, 3), -0.2)
    want[2, :] = 0
    want[:, 2] = 0
    assert torch.equal(y[0, :, :, 0].cpu(), want)
    dx = ops.maxpool2_backward(torch.ones_like(y), codes, 4, 3, 3, stride=1, pad=(0, 1, 0, 1))
    wantd = torch.zeros(3, 3)
    wantd[0, 0] = wantd[0, 1] = wantd[1, 0] = wantd[1, 1] = 1
    assert torch.equal(dx[0, :, :, 1].cpu(), wantd)


SPPK = [(3, 5, 7), (3, 5), (5, 9, 13), (7,), (13,)]
SPPMAP = [(2, 9, 6, 8), (1, 2, 3, 12), (2, 5, 5, 72), (1, 13, 17, 4), (1, 1, 1, 4)]


@pytest.mark.parametrize('kind', ['rand', 'const', 'quant'])
@pytest.mark.parametrize('shape', SPPMAP, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('k', SPPK, ids=lambda k: 'k' + '_'.join(map(str, k)))
def test_spp_parallel_window_kernels(k, shape, kind):
    """The parallel stride-1 windows written in place into the concat slices: values and full-window arg-max codes equal torch's max_pool2d
    (CPU, fp64) exactly - maps smaller than the window, odd sizes, C not a multiple of 64, a non-zero channel offset, exact ties; the gradient
    within sum(k^2) roundings of the sum of its terms' magnitudes (from the fp64 run on |dout|); two launches bit-identical."""
    from somi_amd import ops
    B, H, W, C = shape
    nk, coff = len(k), 8
    cs = coff + (nk + 1) * C + 4
    gen = torch.Generator().manual_seed(sum(shape) + sum(k) + len(kind))
    buf = torch.full((B, H, W, cs), 9.0)
    buf[..., coff:coff + C] = _tie_map(B, H, W, C, gen, kind)
    x64 = nchw(buf[..., coff:coff + C]).double().contiguous().requires_grad_(True)
    bg = buf.cuda()
    _, codes = ops.spp_pool_(bg, C, k, coff, codes=True)
    codes = codes.view(nk, B, H, W, C).cpu()
    hh = torch.arange(H).view(1, 1, H, 1)
    ww = torch.arange(W).view(1, 1, 1, W)
    ys = []
    for i, kk in enumerate(k):
        y64, idx = F.max_pool2d(x64, kk, 1, kk // 2, return_indices=True)
        ys.append(y64)
        c64 = ((idx // W - hh + kk // 2) * kk + (idx % W - ww + kk // 2)).to(torch.uint8)
        assert torch.equal(bg[..., coff + (i + 1) * C:coff + (i + 2) * C].cpu().double(), nhwc(y64.detach())), f'values of window {kk}'
        assert torch.equal(codes[i], nhwc(c64)), f'arg-max codes of window {kk}'
    assert torch.equal(bg[..., :coff + C].cpu(), buf[..., :coff + C]) and (bg[..., coff + (nk + 1) * C:] == 9).all()
    bg2 = buf.cuda()
    ops.spp_pool_(bg2, C, k, coff)                                # eval form: no codes
    assert torch.equal(bg, bg2)
    db = torch.randn(B, H, W, cs, generator=gen)
    douts = [nchw(db[..., coff + (i + 1) * C:coff + (i + 2) * C]).double() for i in range(nk)]
    own = nchw(db[..., coff:coff + C]).double()
    torch.autograd.backward(ys, douts, retain_graph=True)
    dx64 = x64.grad + own
    x64.grad = None
    torch.autograd.backward(ys, [d.abs() for d in douts])
    mag = x64.grad + own.abs()
    dg = db.cuda()
    ops.spp_pool_backward_(dg, codes.cuda().view(-1), C, k, coff)
    got = nchw(dg[..., coff:coff + C]).cpu().double()
    bar = sum(v * v for v in k) * 2.0 ** -24 * mag
    worst = ((got - dx64).abs() - bar).max().item()
    print(f'spp {k} dx: worst excess over the bar {worst:.3e}')
    assert ((got - dx64).abs() <= bar).all(), f'dx beyond sum(k^2) roundings of its terms by {worst:.3e}'
    assert torch.equal(dg[..., :coff].cpu(), db[..., :coff]) and torch.equal(dg[..., coff + C:].cpu(), db[..., coff + C:])
    dg2 = db.cuda()
    ops.spp_pool_backward_(dg2, codes.cuda().view(-1), C, k, coff)
    assert torch.equal(dg, dg2)


def test_constant_map_routes_to_the_first_row_major_maximum():
    """A constant 5x5 map through MaxPool2d(3, 1, 1): gradient 4 on pixel (0, 0), as torch's CPU autograd gives."""
    from somi_amd import ops
    buf = torch.zeros(1, 5, 5, 8)
    buf[..., :4] = 1.0
    x = buf[..., :4].permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(x, 3, 1, 1).sum().backward()
    assert x.grad[0, 0, 0, 0] == 4
    _, codes = ops.spp_pool_(buf.cuda(), 4, (3,), 0, codes=True)
    d = torch.zeros(1, 5, 5, 8)
    d[..., 4:] = 1.0
    dg = d.cuda()
    ops.spp_pool_backward_(dg, codes, 4, (3,), 0)
    assert torch.equal(dg[0, :, :, 0].cpu(), x.grad[0, 0])


def _mk_padpool(M):
    if M is R:
        return R.PadPool((0, 1, 0, 1), 2, 1)
    m = M.MaxPool2d(2, 1, 0)
    m.pad = (0, 1, 0, 1)
    return m


def _OB():
    from oracle.somi_ref import blocks as OB
    return OB


BLOCKS = {'csp_sc': (lambda M: M.BottleneckCSP(32, 32, 1, True), (2, 32, 9, 11), 0.0),
          'csp_nosc': (lambda M: M.BottleneckCSP(24, 32, 1, False), (2, 24, 7, 9), 0.0),
          'csp_n2': (lambda M: M.BottleneckCSP(32, 64, 2, True), (2, 32, 8, 6), 0.0),
          'csp_n3_wide': (lambda M: M.BottleneckCSP(64, 128, 3, False), (3, 64, 5, 7), 0.0),
          'spp357': (lambda M: (_OB() if M is R else M).SPP(32, 32, (3, 5, 7)), (2, 32, 9, 6), 0.0),
          'spp35_2x3': (lambda M: (_OB() if M is R else M).SPP(32, 24, (3, 5)), (2, 32, 2, 3), 0.0),
          'spp7': (lambda M: (_OB() if M is R else M).SPP(16, 32, (7,)), (2, 16, 8, 8), 0.0),
          'seq2': (lambda M: nn.Sequential(_OB().Bottleneck(32, 32), _OB().Bottleneck(32, 32)) if M is R else
                   M.Repeat(M.Bottleneck(32, 32), M.Bottleneck(32, 32)), (2, 32, 7, 9), 0.0),
          'seq3_nosc': (lambda M: nn.Sequential(*(_OB().Bottleneck(16, 16, False) for _ in range(3))) if M is R else
                        M.Repeat(*(M.Bottleneck(16, 16, False) for _ in range(3))), (2, 16, 6, 6), 0.0),
          'padpool': (_mk_padpool, (2, 8, 5, 7), -0.5),
          'pool_s2_odd': (lambda M: nn.MaxPool2d(2, 2, 0) if M is R else M.MaxPool2d(2, 2, 0), (2, 16, 7, 9), 0.0)}


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_hub_blocks_eval_train_backward(tag):
    """Eval forward (BatchNorm folded), training forward, hand-written backward against torch autograd on the CPU restatement: output,
    dx, every parameter gradient (BatchNorm's included) and the updated running statistics."""
    mk, shape, shift = BLOCKS[tag]
    check_block(mk, R, shape, tag, shift=shift)


def hub_batch(batch, size, nc, seed):
    """uint8 images and targets whose boxes span 3 % to 90 % of the image log-uniformly, so that anchors of every level from P3 to P7 find matches
    (oracle.somi_ref.testing.synthetic_batch draws VisDrone-sized boxes, which never reach the coarse levels)."""
    gen = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (batch, 3, size, size), generator=gen, dtype=torch.uint8)
    rows = []
    for b in range(batch):
        n = 40
        cls = torch.randint(0, nc, (n, 1), generator=gen).float()
        wh = torch.exp(torch.rand(n, 2, generator=gen) * (torch.tensor(0.9).log() - torch.tensor(0.03).log()) + torch.tensor(0.03).log())
        xy = torch.rand(n, 2, generator=gen) * 0.9 + 0.05
        rows.append(torch.cat([torch.full((n, 1), float(b)), cls, xy, wh], 1))
    return imgs, torch.cat(rows, 0)


def entries_per_level(ref, preds, targets):
    """How many (anchor, target, offset) entries the oracle's build_targets matches at each level."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    return [int(ix[0].numel()) for ix in OLoss(ref).build_targets(preds, targets)[2]]


#        name            cfg keywords                                                     batch size seed  full
GRAPHS = [('yolov3-tiny', dict(width=0.25, depth=1.0, nc=10), 2, 160, 1, True),
          ('yolov3-spp', dict(width=0.25, depth=0.33, nc=10), 2, 96, 1, True),
          ('yolov5-panet', dict(width=0.25, depth=0.33, nc=10), 2, 128, 1, True),
          ('yolov5-p7', dict(width=0.25, depth=0.33, nc=10, anchors=R.P7_ANCHORS_256), 8, 256, 1, True),
          ('yolov5-fpn', dict(width=0.25, depth=0.33, nc=10), 2, 128, 1, False),
          ('yolov5-p6', dict(width=0.25, depth=0.33, nc=10, anchors=R.P6_ANCHORS), 2, 128, 1, False),
          ('yolov3', dict(width=0.25, depth=0.33, nc=10), 2, 64, 1, False)]


@pytest.mark.parametrize('name,kw,batch,size,seed,full', GRAPHS, ids=[g[0] for g in GRAPHS])
def test_hub_graph_training_step_eval_and_checkpoint(name, kw, batch, size, seed, full, monkeypatch):
    """A hub graph at width 0.25 against the oracle Model: the eval forward; for the `full` ones also one training forward,
    ComputeLoss and backward (outputs, loss, every parameter gradient, BatchNorm statistics) on a batch whose targets reach EVERY detection
    level (asserted), two fresh TrainStep.step runs bit-identical, and attempt_load of a pickled oracle model.

    Batch 2, except yolov5-p7 at 256 px: its P7 map is 2x2, so at batch 2 the BatchNorms there normalise over 8 samples and the fp32 CPU oracle
    is itself no witness at the bar - against its own fp64 copy it is off by 1.26 x the bar (model.2.cv2.bn.bias; measured on the CPU, as was the
    GPU path's 1.35 x on the same parameter).  At batch 8 (32 samples, what the other graphs' coarsest maps see) the oracle is within 0.21 x
    the bar of fp64; the test asserts that it is within half the bar, so the reference cannot fail the check on its own."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state
    from somi_amd import blocks as MB
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = R.hub_cfg(name, **kw)
    ref = fill_state(OModel(cfg), 3)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    ref.hyp = mine.hyp = dict(HYP_VISDRONE)
    imgs, targets = hub_batch(batch, size, 10, seed)
    if name == 'yolov3-spp':
        assert [len(m) for m in mine.model if isinstance(m, MB.Repeat)] == [3, 3]       # the 3-long Sequentials are in the graph under test
    if full:
        pr = check_train_step(ref, mine, imgs, targets, name)
        hit = entries_per_level(ref, pr, targets)
        print(f'{name}: entries per level {hit}, maps {[tuple(p.shape[2:4]) for p in pr]}')
        assert len(hit) == len(cfg['head'][-1][0]) and all(h > 0 for h in hit), f'a detection level has no target: {hit}'
        if name == 'yolov5-p7':                                   # the fp32 oracle has to be a witness at this bar (see the docstring)
            ref64 = copy.deepcopy(ref).double()
            ref64.zero_grad()
            OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
            own = max((p.grad.double() - q.grad).abs().max().item() / (2e-3 * (q.grad.abs().max().item() + 1e-9) + 2e-6)
                      for p, q in zip(ref.parameters(), ref64.parameters()))
            print(f'{name}: the fp32 oracle is {own:.3f} x the bar from its fp64 copy')
            assert own <= 0.5, f'the fp32 oracle is {own:.2f} x the bar from fp64: no witness at this batch'
    check_eval(ref, mine, imgs, name)
    if not full:
        return
    check_two_steps_bit_identical(cfg, state, imgs, targets, batch)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'hub_ref'), name)


@pytest.mark.parametrize('nl', [5, 2])
def test_five_and_two_level_loss_against_the_oracle(nl, monkeypatch):
    """ComputeLoss in isolation on random predictions: five levels (yolov5-p7: the fifth travels beside the four-level descriptor) and two
    (yolov3-tiny, on the five-entry balance table): value, items and the gradient of every level against the oracle loss; every level has targets."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.loss import ComputeLoss
    from somi_amd.model import Model
    R.register(monkeypatch)
    name, kw, size = ('yolov5-p7', dict(anchors=R.P7_ANCHORS_256), 256) if nl == 5 else ('yolov3-tiny', {}, 160)
    cfg = R.hub_cfg(name, width=0.25, depth=0.33, nc=10, **kw)
    ref, mine = OModel(cfg), Model(cfg)
    ref.hyp = mine.hyp = dict(HYP_VISDRONE)
    det = ref.model[-1]
    assert det.nl == nl
    gen = torch.Generator().manual_seed(11 + nl)
    _, targets = hub_batch(3, size, 10, 5)
    pr = [torch.randn(3, det.na, int(size / s), int(size / s), det.no, generator=gen).requires_grad_(True) for s in ref.stride.tolist()]
    hit = entries_per_level(ref, pr, targets)
    assert len(hit) == nl and all(h > 0 for h in hit), hit
    lr, ir = OLoss(ref)(pr, targets)
    lr.backward()
    pm = [p.detach().cuda().requires_grad_(True) for p in pr]
    mine.model[-1].anchors = mine.model[-1].anchors.cuda()
    lm, im = ComputeLoss(mine)(pm, targets.cuda())
    lm.backward()
    rel_close(lm, lr, rel=1e-4, what=f'{nl}-level loss')
    rel_close(im, ir, rel=1e-4, what=f'{nl}-level loss items')
    for l, (a, b) in enumerate(zip(pm, pr)):
        assert b.grad.abs().max() > 0
        rel_close(a.grad, b.grad, what=f'{nl}-level loss: gradient of level {l}', atol=1e-9)
    lm2, _ = ComputeLoss(mine)([p.detach().requires_grad_(True) for p in pm], targets.cuda())
    assert torch.equal(lm2.detach(), lm.detach())
