"""Coordinate attention on the MI355X (CoorAttention, CABottleneck, C3_CA; coordatt.hip): the four kernels against an fp64 restatement, the blocks
against torch autograd on the CPU restatement (tests/coordatt_ref.py), the yolov5s graphs of configs.yolov5_ca_cfg against the oracle Model.
Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch

import coordatt_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step,
                    check_two_steps_bit_identical, nhwc, rel_close)

pytestmark = pytest.mark.gpu


def _case(shape, seed):
    """Inputs of the four kernels (NHWC, fp32, CPU) and their fp64 results."""
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    t = dict(x=r(B, H, W, C), res=r(B, H, W, C), dout=r(B, H, W, C), a_h=torch.sigmoid(r(B, H, C)), a_w=torch.sigmoid(r(B, W, C)),
             gh=r(B, H, C), gw=r(B, W, C), have=r(B, H, W, C))
    d = {k: v.double() for k, v in t.items()}
    gate = d['a_h'][:, :, None] * d['a_w'][:, None]
    want = dict(pool=torch.cat([d['x'].mean(2), d['x'].mean(1)], 1), out=d['x'] * gate, out_res=d['res'] + d['x'] * gate,
                da_h=(d['dout'] * d['x'] * d['a_w'][:, None]).sum(2), da_w=(d['dout'] * d['x'] * d['a_h'][:, :, None]).sum(1),
                dx=d['dout'] * gate + d['gh'][:, :, None] / W + d['gw'][:, None] / H)
    return t, want


# H != W (a transposed gate shows); degenerate axes; more than one workgroup along W (130 columns of 8 channels: 128 per workgroup), along H
# (rows go in chunks of at most 32, of 4 on maps this small), along both with a ragged last chunk
SHAPES = [(2, 5, 7, 32), (1, 1, 9, 8), (2, 9, 1, 8), (1, 67, 35, 16), (1, 3, 130, 8), (1, 130, 3, 8)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernels_against_fp64(shape):
    """means, apply (with and without the shortcut), backward gates and backward input on whole tensors, the gates as plain (B,H,C) / (B,W,C)
    tensors, at 1e-3 of each result's largest value; every kernel run twice, bit-identical."""
    from somi_amd import ops
    B, H, W, C = shape
    t, want = _case(shape, 3 + sum(shape))
    g = {k: v.cuda() for k, v in t.items()}
    assert ops._lib.lib().somi_coordatt_workspace_floats(B, H, W, C) > 0

    def run():
        pool = ops.coordatt_means(g['x'], C)
        out = ops.coordatt_apply(g['x'], g['a_h'], g['a_w'], C)
        out_res = ops.coordatt_apply(g['x'], g['a_h'], g['a_w'], C, res=g['res'])
        da_h, da_w = ops.coordatt_backward_gates(g['dout'], g['x'], g['a_h'], g['a_w'], C)
        dx = ops.coordatt_backward_input(g['dout'], g['a_h'], g['a_w'], g['gh'], g['gw'], C)
        return dict(pool=pool.view(B, H + W, C), out=out, out_res=out_res, da_h=da_h, da_w=da_w, dx=dx)

    first, second = run(), run()
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(first[k], second[k]), f'{shape}: two launches differ in {k}'
        rel_close(first[k], want[k], what=f'{shape} {k}')


def _wide(t, dev='cuda'):
    """t as channels [4, 4 + c) of a tensor 8 channels wider, the rest 7.0 (a sentinel the kernels must leave)."""
    out = torch.full((*t.shape[:-1], t.shape[-1] + 8), 7.0)
    out[..., 4:4 + t.shape[-1]] = t
    return out.to(dev)


def _untouched(t, c, what):
    assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + c:] == 7.0).all()), f'{what}: a kernel wrote outside its slice'


def test_kernels_on_slices_of_wider_tensors():
    """Input, output and shortcut as channel slices at a non-zero offset of wider tensors, and the gates the way the blocks hold them: the two
    halves - rows [0, H) and [H, H + W) - of one (B, H + W, .) tensor, at two channel offsets; pool, da_h / da_w and gh / gw likewise.  Nothing
    outside a slice, and no row of a gate gradient outside its half, is written."""
    from somi_amd import ops
    shape = B, H, W, C = (2, 6, 5, 12)
    t, want = _case(shape, 77)
    x, res, dout = _wide(t['x']), _wide(t['res']), _wide(t['dout'])
    gates = torch.full((B, H + W, 2 * C + 8), 7.0)
    gates[:, :H, 4:4 + C], gates[:, H:, 4 + C:4 + 2 * C] = t['a_h'], t['a_w']
    grads = torch.full((B, H + W, C + 8), 7.0)
    grads[:, :H, 4:4 + C], grads[:, H:, 4:4 + C] = t['gh'], t['gw']
    gates, grads = gates.cuda(), grads.cuda()
    a_h, a_w = (gates, 4, 0), (gates, 4 + C, H)
    pool = ops.coordatt_means(x, C, 4, out=torch.full((B, H + W, 1, C + 8), 7.0, device='cuda'), o_coff=4)
    out = ops.coordatt_apply(x, a_h, a_w, C, 4, res=res, res_coff=4, out=torch.full_like(x, 7.0), o_coff=4)
    dg = torch.full_like(gates, 7.0)
    ops.coordatt_backward_gates(dout, x, a_h, a_w, C, 4, 4, da_h=(dg, 4, 0), da_w=(dg, 4 + C, H))
    dx = ops.coordatt_backward_input(dout, a_h, a_w, (grads, 4, 0), (grads, 4, H), C, 4, out=torch.full_like(x, 7.0), dx_coff=4)
    torch.cuda.synchronize()
    rel_close(pool[:, :, 0, 4:4 + C], want['pool'], what='sliced pool')
    rel_close(out[..., 4:4 + C], want['out_res'], what='sliced out')
    rel_close(dg[:, :H, 4:4 + C], want['da_h'], what='sliced da_h')
    rel_close(dg[:, H:, 4 + C:4 + 2 * C], want['da_w'], what='sliced da_w')
    rel_close(dx[..., 4:4 + C], want['dx'], what='sliced dx')
    for name, ten in (('pool', pool), ('out', out), ('dx', dx)):
        _untouched(ten, C, name)
    _untouched(dg, 2 * C, 'gate gradients')
    assert bool((dg[:, H:, 4:4 + C] == 7.0).all()) and bool((dg[:, :H, 4 + C:4 + 2 * C] == 7.0).all()), 'a gate gradient left its half'


@pytest.mark.parametrize('shape', [(2, 5, 7, 32), (1, 67, 35, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_backward_input_accumulates(shape):
    """accumulate=True adds the input gradient to what dx holds; two launches from the same start are bit-identical."""
    from somi_amd import ops
    B, H, W, C = shape
    t, want = _case(shape, 5)
    g = {k: v.cuda() for k, v in t.items()}
    runs = []
    for _ in range(2):
        dx = g['have'].clone()
        ops.coordatt_backward_input(g['dout'], g['a_h'], g['a_w'], g['gh'], g['gw'], C, out=dx, accumulate=True)
        runs.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(*runs), 'two accumulating launches differ'
    rel_close(runs[0], want['dx'] + t['have'].double(), what=f'{shape} dx accumulated')


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """CoorAttention, CABottleneck with and without the shortcut, C3_CA with one bottleneck and two C3_CA in a row (what the parser makes of n = 2)
    at the fixtures' shape (batch 2, 64 channels, 5x7): eval forward, training forward, dx, every parameter gradient and bn1's running statistics
    (parity.buffers_close).  The input seeds are coordatt_ref.BLOCK_SEEDS, chosen from the reference alone by h-swish's kink margin."""
    check_block(R.BLOCKS[tag], R, R.BLOCK_SHAPE, tag, seed=R.BLOCK_SEEDS[tag])


@pytest.mark.parametrize('tag', ['coordatt', 'cabottleneck_sc', 'c3_ca'])
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) - which the three blocks take although the graph walk does not use it on them - leaves
    R + dx in `have`, R what it held and dx what a plain backward of the same forward returns."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case(tag)
    mine = R.BLOCKS[tag](MB)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda().train()
    xd = nhwc(x).cuda()
    y = mine(Act(xd.clone()))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    dx = mine.backward(Act(dy.clone()))
    dx = dx.t[..., dx.coff:dx.coff + 64].clone()
    mine(Act(xd.clone()))
    have = torch.randn(xd.shape, generator=gen).cuda()
    before = have.clone()
    got = mine.backward(Act(dy.clone()), dx_out=Act(have), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have, before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')


@pytest.mark.parametrize('where', ['c3', 'row'])
def test_ca_graph_training_step_eval_and_checkpoint(where, monkeypatch):
    """yolov5s 6.0 at width 0.25 with C3_CA in the backbone ('c3': rows of 1, 2, 3 and 1 blocks) or a CoorAttention row behind SPPF ('row'), nc 10,
    batch 2, 64x64, against the oracle Model: one training forward, ComputeLoss and backward, the eval forward; two fresh TrainStep.step runs
    bit-identical; a pickled oracle model loads; a step moves the gate convs.  Seeds: coordatt_ref.GRAPH_SEEDS (the kink margins are there)."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-ca-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-ca-{where}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'coordatt_ref'), f'yolov5s-ca-{where}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    moved = [k for k in state if k.endswith(('conv_h.weight', 'conv_w.bias', 'conv1.weight', 'bn1.weight', 'bn1.running_mean'))]
    assert len(moved) == (5 * 7 if where == 'c3' else 5)
    for k in moved:
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
