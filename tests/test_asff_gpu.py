"""The ASFF head on the MI355X (ASFF_Detect, ASFF, add_conv; asff.hip, pool.hip): the fusion kernels against fp64 autograd on the CPU,
max_pool2d(3, 2, 1) against torch's CPU kernel and autograd, Conv-BN-LeakyReLU, the three ASFF blocks and the head against torch autograd on
the CPU restatement (tests/asff_ref.py), the whole yolov5s graph with the head against the oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import asff_ref as R
from parity import (bn_hyper, buffers_close, check_block, check_checkpoint_roundtrip, check_eval, check_train_step,
                    check_two_steps_bit_identical, nhwc, rel_close)

pytestmark = pytest.mark.gpu

SHIFTS = [(2, 1, 0), (1, 0, 0), (0, 0, 0)]


def _up64(t, up):
    return t.repeat_interleave(1 << up, 1).repeat_interleave(1 << up, 2)


def _fuse64(rs, vs, r_ups, v_ups, w, b, dout):
    """fp64 autograd restatement on NHWC tensors -> fused, p, the largest logit, [dr_i], [dv_i], dW, db."""
    rs = [t.double().requires_grad_(True) for t in rs]
    vs = [t.double().requires_grad_(True) for t in vs]
    w, b = w.double().requires_grad_(True), b.double().requires_grad_(True)
    cat = torch.cat([_up64(v, u) for v, u in zip(vs, v_ups)], -1)
    logits = cat @ w.t() + b
    p = logits.softmax(-1)
    fused = sum(_up64(r, u) * p[..., i:i + 1] for i, (r, u) in enumerate(zip(rs, r_ups)))
    fused.backward(dout.double())
    return fused.detach(), p.detach(), logits.detach().max().item(), [t.grad for t in rs], [t.grad for t in vs], w.grad, b.grad


def _wide(t, dev='cuda'):
    """t as channels [4, 4 + c) of a tensor 8 channels wider, the rest 7.0 (a sentinel the kernels must leave)."""
    out = torch.full((*t.shape[:3], t.shape[3] + 8), 7.0)
    out[..., 4:4 + t.shape[3]] = t
    return out.to(dev)


def _fuse_case(C, base, B, r_ups, v_ups, gen, vscale=1.0):
    from somi_amd import ops
    U = max(r_ups + v_ups)
    H, W = base[0] << U, base[1] << U
    rs = [torch.randn(B, H >> u, W >> u, C, generator=gen) for u in r_ups]
    vs = [torch.randn(B, H >> u, W >> u, 16, generator=gen) * vscale for u in v_ups]
    w, b = torch.randn(3, 48, generator=gen) * 0.3, torch.randn(3, generator=gen)
    dout = torch.randn(B, H, W, C, generator=gen)
    want = _fuse64(rs, vs, r_ups, v_ups, w, b, dout)
    rd, vd = [(_wide(t), 4) for t in rs], [(_wide(t), 4) for t in vs]
    wd, bd, dd = w.cuda(), b.cuda(), _wide(dout)
    tag = f'C{C} {base} B{B} r{r_ups} v{v_ups}'

    def run():
        out = torch.full((B, H, W, C + 8), 7.0, device='cuda')
        _, p = ops.asff_fuse(rd, vd, r_ups, v_ups, wd, bd, C, out=out, o_coff=4, weights=True)
        dw, db = torch.ones(3, 48, device='cuda'), torch.ones(3, device='cuda')
        drs = [(torch.full_like(t, 7.0), 4) for t, _ in rd]
        dvs = [(torch.full_like(t, 7.0), 4) for t, _ in vd]
        ops.asff_fuse_backward(dd, rd, vd, r_ups, v_ups, wd, bd, p, C, dw, db, do_coff=4, drs=drs, dvs=dvs)
        return [out, p, dw, db] + [t for t, _ in drs] + [t for t, _ in dvs]

    first, second = run(), run()
    torch.cuda.synchronize()
    for i, (a_, b_) in enumerate(zip(first, second)):
        assert torch.equal(a_, b_), f'{tag}: two launches differ in result {i}'
    out, p, dw, db = first[:4]
    rel_close(out[..., 4:4 + C], want[0], what=f'{tag} fused')
    rel_close(p, want[1], what=f'{tag} p')
    for i in range(3):
        rel_close(first[4 + i][..., 4:4 + C], want[3][i], what=f'{tag} dr{i}')
        rel_close(first[7 + i][..., 4:20], want[4][i], what=f'{tag} dv{i}')
    rel_close(dw, want[5] + 1, what=f'{tag} dW accumulated onto ones')
    rel_close(db, want[6] + 1, what=f'{tag} db accumulated onto ones')
    for t, c in [(out, C)] + [(t, C) for t in first[4:7]] + [(t, 16) for t in first[7:10]]:
        assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + c:] == 7.0).all()), f'{tag}: a kernel wrote outside its slice'
    eval_out = ops.asff_fuse(rd, vd, r_ups, v_ups, wd, bd, C, out=torch.full_like(out, 7.0), o_coff=4)
    assert torch.equal(eval_out, out), f'{tag}: the forward without p differs'
    return want, (rd, vd, wd, bd, dd, p)


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('base', [(1, 1), (3, 5)], ids=['1x1', '3x5'])
@pytest.mark.parametrize('C', [4, 20, 128])
def test_fusion_kernels_against_fp64(C, base, B):
    """fused, p, every dr_i, every dv_i, dW and db (accumulated onto ones) at 1e-3 of each quantity's largest value, for the three shift sets of
    the sources times the three of the weight maps; every tensor a slice of a wider one; two launches bit-identical."""
    gen = torch.Generator().manual_seed(C + 7 * base[1] + B)
    for r_ups in SHIFTS:
        for v_ups in SHIFTS:
            _fuse_case(C, base, B, r_ups, v_ups, gen)


def test_fusion_softmax_subtracts_the_maximum_and_dr_accumulates():
    """Weight maps scaled until the largest logit is beyond 88.73, where a naive exp(logit) is inf in fp32; and dr_accumulate adds to what dr holds."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(11)
    want, (rd, vd, wd, bd, dd, p) = _fuse_case(20, (3, 5), 2, (2, 1, 0), (1, 0, 0), gen, vscale=40.0)
    assert want[2] > 88.73, f'largest logit {want[2]:.1f}: a naive exp would not overflow'
    dw, db = torch.zeros(3, 48, device='cuda'), torch.zeros(3, device='cuda')
    drs = [(torch.ones_like(t), 4) for t, _ in rd]
    ops.asff_fuse_backward(dd, rd, vd, (2, 1, 0), (1, 0, 0), wd, bd, p, 20, dw, db, do_coff=4, drs=drs, accumulate=(True, False, True))
    for i, acc in enumerate((1, 0, 1)):
        rel_close(drs[i][0][..., 4:24], want[3][i] + acc, what=f'dr{i} accumulate={bool(acc)}')


def _pool_inputs(kind, shape, gen):
    if kind == 'negative':
        return -torch.rand(*shape, generator=gen) - 0.5           # a zero pad would win every border window
    if kind == 'ties':
        return torch.randint(-2, 3, shape, generator=gen).float()
    return torch.randn(*shape, generator=gen)


@pytest.mark.parametrize('kind', ['random', 'negative', 'ties'])
@pytest.mark.parametrize('C', [4, 128])
@pytest.mark.parametrize('hw', [(4, 4), (5, 7), (8, 12)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_maxpool3s2_against_torch_cpu(hw, C, kind):
    """F.max_pool2d(x, 3, stride=2, padding=1): the pooled values and the gradient routing equal torch's CPU kernel and autograd exactly (first
    maximum in row-major order, windows added in row-major order), out of and into channel slices; two launches bit-identical."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(hw[0] * hw[1] + C)
    B, (H, W) = 2, hw
    x = _pool_inputs(kind, (B, C, H, W), gen).requires_grad_(True)
    y = F.max_pool2d(x, 3, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    assert tuple(y.shape[2:]) == (ops.maxpool3s2_out_size(H), ops.maxpool3s2_out_size(W))
    xd, dyd = _wide(nhwc(x.detach())), _wide(nhwc(dy))

    def run():
        out = torch.full((B, y.shape[2], y.shape[3], C + 8), 7.0, device='cuda')
        _, codes = ops.maxpool3s2(xd, C, 4, out=out, y_coff=4, codes=True)
        dx = torch.full((B, H, W, C + 8), 7.0, device='cuda')
        ops.maxpool3s2_backward(dyd, codes, C, H, W, 4, out=dx, dx_coff=4)
        return out, codes, dx

    (out, codes, dx), second = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_) for a_, b_ in zip((out, codes, dx), second)), 'two launches differ'
    assert torch.equal(out[..., 4:4 + C].cpu(), nhwc(y.detach())), 'pooled values differ from torch'
    assert torch.equal(dx[..., 4:4 + C].cpu(), nhwc(x.grad)), 'the gradient is routed differently from torch CPU autograd'
    for t in (out, dx):
        assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + C:] == 7.0).all()), 'a kernel wrote outside its slice'
    assert int(codes.max()) <= 8
    assert torch.equal(ops.maxpool3s2(xd, C, 4), out[..., 4:4 + C]), 'the forward without codes differs'


@pytest.mark.parametrize('k,s', [(1, 1), (3, 1), (3, 2)])
def test_conv_bn_leaky(k, s):
    """add_conv 16 -> 24 on 12x10, batch 2: eval, training forward, dx, the parameter gradients and the running statistics."""
    check_block(lambda M: M.add_conv(16, 24, k, s), R, (2, 16, 12, 10), f'add_conv k{k} s{s}', shift=0.2)


@pytest.mark.parametrize('level', [0, 1, 2])
def test_asff_block(level):
    """ASFF(level) on a P5 2x3 / P4 4x6 / P3 8x12 pyramid, batch 2: eval and training forward, the three input gradients, every parameter gradient
    (weight_levels included) and every running statistic - the variance of a weight map computed at low resolution included."""
    check_block(lambda M: R.Packed3(M, lambda ns: ns.ASFF(level)), R, (2, R.PACKED, 2, 3), f'asff{level}')


def _head(ns):
    return ns.ASFF_Detect(3, R.ANCHORS, (128, 256, 512))


def test_asff_detect_head_training():
    """The head, nc 3, batch 2: training raws, the three input gradients through the reversed chain, every parameter gradient, every running
    statistic.  A chain built from the original maps fails here."""
    check_block(lambda M: R.PackedHead(M, _head), R, (2, R.PACKED, 2, 3), 'asff_detect', eval_too=False)


def test_asff_detect_head_eval():
    """z and each raw against the restatement, each at its own scale."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    ref, mine = _head(R), _head(MB)
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    mine.load_state_dict(ref.state_dict())
    ref.stride = mine.stride = torch.tensor(R.STRIDES)
    mine = bn_hyper(mine).cuda().eval()
    ref.eval()
    gen = torch.Generator().manual_seed(4)
    p3, p4, p5 = (torch.randn(2, c, 2 * f, 3 * f, generator=gen) for c, f in ((128, 4), (256, 2), (512, 1)))
    with torch.no_grad():
        z_ref, raws_ref = ref([p3, p4, p5])
        z, raws = mine([MB.Act(nhwc(t).cuda()) for t in (p3, p4, p5)])
    rel_close(z, z_ref, what='head eval z')
    for i, (a_, b_) in enumerate(zip(raws, raws_ref)):
        rel_close(a_, b_, what=f'head eval raw{i}')
    buffers_close(mine, ref, 'head eval')


def test_asff_graph_training_step_eval_and_checkpoint():
    """yolov5s (width 0.5, depth 0.33) with the ASFF head, nc 10, batch 2, 96x64 against the oracle Model: one training forward, ComputeLoss and
    backward, the eval forward; two fresh TrainStep.step runs bit-identical; a pickled oracle model loads; two steps leave a finite loss and move
    the weight_levels conv of the last ASFF.  The weights' and the batch's seeds are asff_ref.GRAPH_SEEDS, chosen from the reference alone: the pair that keeps
    every LeakyReLU input of the head farthest from the kink (the figures are there).  With the Swin graph test's pair (3, 2) the fp32 oracle itself
    is 11.5 x the gradient bar away from fp64 and this path 4.7 x away from the oracle (34 parameters beyond the bar); with (5, 7) one flipped element
    of asffs.0.stride_level_1 put that layer's BatchNorm bias 31 x off while every other head parameter stayed below 0.1 x."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    cfg, ref, imgs, targets = R.graph_case()
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, 'yolov5s-asff')
    check_eval(ref, mine, imgs, 'yolov5s-asff')
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'asff_ref'), 'yolov5s-asff')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    for _ in range(2):
        loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss after two steps is not finite: {loss.tolist()}'
    k = 'model.24.asffs.2.weight_levels.weight'
    assert not torch.equal(m.state_dict()[k].cpu(), state[k]), 'two steps left the weight_levels conv of the last ASFF where it was'
