"""Channel prior convolutional attention on the MI355X (CPCA, CPCABottleneck, C3CPCA; cpca.hip): the strip kernels and their weight gradients
against an fp64 restatement, the blocks against torch autograd on the CPU restatement (tests/cpca_ref.py), the yolov5s graphs of
configs.yolov5_cpca_cfg against the oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import cpca_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step,
                    check_two_steps_bit_identical, nhwc, rel_close)

pytestmark = pytest.mark.gpu

TAPS = (7, 11, 21)
# the map smaller than every strip; degenerate axes; ragged tiles on both axes (67 = 64 + 3 positions, 35 lines); more than one workgroup along
# the strip (130 = 64 + 64 + 2) on either axis; a quad count that is no power of two (3 quads: 85 lanes per quad, one lane idle)
SHAPES = [(2, 5, 7, 32), (1, 1, 23, 8), (1, 23, 1, 8), (1, 67, 35, 16), (1, 3, 130, 8), (1, 130, 3, 8), (2, 24, 22, 12)]
# Shapes at which a workgroup WALKS several tiles (somi_cpca_tiles_per_workgroup > 1), as every batch-32 launch of training does: the plan walks
# only once 1024 (strips) or 512 (weight gradient) workgroups exist, so the strip axis is 4 long (a tile of 4 positions x 3 lines, 2 for the
# weight gradient) and the other axis 1555 - 1.6 M floats.  128 channels: 16 quads a workgroup, two quad chunks over blockIdx.z.  1555 lines in
# groups of 3 x 2: the last workgroup's second tile lies outside the map (the loop's early exit), the one before is ragged.
WALK_SHAPES = [(2, 4, 1555, 128), (2, 1555, 4, 128)]
TRAINING_COMBOS = [('w', False, True), ('h', False, True), ('h', True, False), ('w', True, False)]      # forward pair, data-gradient pair
IDS = lambda s: 'x'.join(map(str, s))     # noqa: E731


def test_walk_shapes_walk():
    """The two WALK_SHAPES make the strip kernels walk 2 tiles and the weight gradient's first stage 4, each along the short axis; every shape
    of SHAPES stays at one tile - so both forms of the loop are under test."""
    from somi_amd import _lib
    tiles = _lib.lib().somi_cpca_tiles_per_workgroup
    for shape, axis in zip(WALK_SHAPES, (1, 0)):
        assert (tiles(*shape, axis, 0), tiles(*shape, axis, 1)) == (2, 4), shape
    assert all(tiles(*s, ax, wg) == 1 for s in SHAPES for ax in (0, 1) for wg in (0, 1))


def _strip64(x, w, bias, axis, flip):
    """S_k of the NHWC fp64 tensor x: the depthwise conv with the (C, k) taps w along `axis`, zero padding k // 2, taps backwards with flip."""
    C, k = w.shape
    w = w.flip(1) if flip else w
    x = x.permute(0, 3, 1, 2)
    if axis == 'w':
        y = F.conv2d(x, w.view(C, 1, 1, k), bias, padding=(0, k // 2), groups=C)
    else:
        y = F.conv2d(x, w.view(C, 1, k, 1), bias, padding=(k // 2, 0), groups=C)
    return y.permute(0, 2, 3, 1)


def _case(shape, seed):
    """Inputs of the strip kernels (NHWC fp32, CPU): a tensor, three branch tensors, a pass-through, a start value, taps and biases."""
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    return dict(x=r(B, H, W, C), ts=[r(B, H, W, C) for _ in TAPS], through=r(B, H, W, C), have=r(B, H, W, C),
                ws=[r(C, k) / k ** 0.5 for k in TAPS], bs=[r(C) for _ in TAPS])


def _want_fanout(t, axis, flip, bias):
    return [_strip64(t['x'].double(), w.double(), b.double() if bias else None, axis, flip) for w, b in zip(t['ws'], t['bs'])]


def _want_fanin(t, axis, flip, bias):
    out = t['through'].double()
    for x, w, b in zip(t['ts'], t['ws'], t['bs']):
        out = out + _strip64(x.double(), w.double(), b.double() if bias else None, axis, flip)
    return out


@pytest.mark.parametrize('shape', SHAPES + WALK_SHAPES, ids=IDS)
def test_strip_kernels_against_fp64(shape):
    """Fan-out and fan-in on whole tensors, along W and along H, taps as stored and flipped, with and without bias, at 1e-3 of each result's
    largest value; every kernel run twice, bit-identical.  The WALK_SHAPES run the four combinations training uses."""
    from somi_amd import ops
    B, H, W, C = shape
    t = _case(shape, 3 + sum(shape))
    g = {k: [v.cuda() for v in val] if isinstance(val, list) else val.cuda() for k, val in t.items()}
    for axis, flip, bias in TRAINING_COMBOS if shape in WALK_SHAPES else itertools.product('wh', (False, True), (True, False)):
        what = f'{shape} axis {axis} flip {flip} bias {bias}'
        bs = g['bs'] if bias else None
        runs = []
        for _ in range(2):
            outs = ops.cpca_fanout(g['x'], g['ws'], bs, C, axis=axis, flip=flip)
            s = ops.cpca_fanin(g['ts'], g['through'], g['ws'], bs, C, axis=axis, flip=flip)
            runs.append(outs + [s])
        torch.cuda.synchronize()
        for a, b in zip(*runs):
            assert torch.equal(a, b), f'{what}: two launches differ'
        for k, (got, want) in enumerate(zip(runs[0][:3], _want_fanout(t, axis, flip, bias))):
            rel_close(got, want, what=f'{what} fan-out {TAPS[k]}')
        rel_close(runs[0][3], _want_fanin(t, axis, flip, bias), what=f'{what} fan-in')


def _wgrad_case(shape, seed):
    """u, the taps and biases of the six strip convs, ds -> the kernel's inputs (u, t_k, ds, dt_k; fp32) and the fp64 gradients of
    s = u + sum_k V_k(H_k(u)) for the output gradient ds."""
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    u, ds = r(B, H, W, C), r(B, H, W, C)
    wh, wv = [r(C, k) / k ** 0.5 for k in TAPS], [r(C, k) / k ** 0.5 for k in TAPS]
    bh, bv = [r(C) for _ in TAPS], [r(C) for _ in TAPS]
    p64 = [[v.double().requires_grad_(True) for v in grp] for grp in (wh, wv, bh, bv)]
    ts = [_strip64(u.double(), w, b, 'w', False) for w, b in zip(p64[0], p64[2])]
    s = u.double() + sum(_strip64(tk, w, b, 'h', False) for tk, w, b in zip(ts, p64[1], p64[3]))
    grads = torch.autograd.grad(s, [*ts, *itertools.chain(*p64)], ds.double())
    dts, want = grads[:3], [list(grads[3 + 3 * i:6 + 3 * i]) for i in range(4)]
    inputs = dict(u=u, ts=[v.detach().float() for v in ts], ds=ds, dts=[v.float() for v in dts])
    return inputs, want, r


def _run_wgrad(ops, g, C, targets, accumulate):
    ops.cpca_wgrad(g['u'], g['ts'], g['ds'], g['dts'], C, *targets, accumulate=accumulate)


@pytest.mark.parametrize('shape', SHAPES + WALK_SHAPES, ids=IDS)
def test_weight_and_bias_gradients_against_fp64(shape):
    """All 78 tap gradients and the six bias gradients of one call, written in nn.Conv2d's layouts ((C,1,1,k) and (C,1,k,1)) and accumulated
    onto a given start; two launches bit-identical."""
    from somi_amd import ops
    B, H, W, C = shape
    inputs, want, r = _wgrad_case(shape, 11 + sum(shape))
    g = {k: [v.cuda() for v in val] if isinstance(val, list) else val.cuda() for k, val in inputs.items()}
    assert ops._lib.lib().somi_cpca_wgrad_workspace_floats(B, H, W, C) > 0
    shapes = [[(C, 1, 1, k) for k in TAPS], [(C, 1, k, 1) for k in TAPS], [(C,)] * 3, [(C,)] * 3]
    runs = []
    for _ in range(2):
        targets = [[torch.full(s, 7.0, device='cuda') for s in grp] for grp in shapes]
        _run_wgrad(ops, g, C, targets, False)
        runs.append(targets)
    start = [[r(*s) for s in grp] for grp in shapes]
    acc = []
    for _ in range(2):
        targets = [[v.cuda() for v in grp] for grp in start]
        _run_wgrad(ops, g, C, targets, True)
        acc.append(targets)
    torch.cuda.synchronize()
    names = ('dw_h', 'dw_v', 'db_h', 'db_v')
    for gi, k in itertools.product(range(4), range(3)):
        what = f'{shape} {names[gi]}[{TAPS[k]}]'
        assert torch.equal(runs[0][gi][k], runs[1][gi][k]) and torch.equal(acc[0][gi][k], acc[1][gi][k]), f'{what}: two launches differ'
        rel_close(runs[0][gi][k].flatten(), want[gi][k].flatten(), what=what)
        rel_close(acc[0][gi][k].flatten(), want[gi][k].flatten() + start[gi][k].double().flatten(), what=what + ' accumulated')
    for k in range(1, 3):                                         # the three vertical bias gradients are the same column sum of ds
        assert torch.equal(runs[0][3][0], runs[0][3][k])


def _wide(t, dev='cuda'):
    """t as channels [4, 4 + c) of a tensor 8 channels wider, the rest 7.0 (a sentinel the kernels must leave)."""
    out = torch.full((*t.shape[:-1], t.shape[-1] + 8), 7.0)
    out[..., 4:4 + t.shape[-1]] = t
    return out.to(dev)


def _untouched(t, c, what):
    assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + c:] == 7.0).all()), f'{what}: a kernel wrote outside its slice'


@pytest.mark.parametrize('axis', ['w', 'h'])
def test_kernels_on_slices_of_wider_tensors(axis):
    """Inputs and outputs as channel slices at offset 4 of tensors 8 channels wider, filled with a sentinel: the results are the whole-tensor
    ones and nothing outside a slice is written.  The gate product and its backward likewise."""
    from somi_amd import ops
    shape = B, H, W, C = (2, 9, 11, 12)
    t = _case(shape, 77)
    ws, bs = [w.cuda() for w in t['ws']], [b.cuda() for b in t['bs']]
    outs = [torch.full((B, H, W, C + 8), 7.0, device='cuda') for _ in TAPS]
    ops.cpca_fanout(_wide(t['x']), ws, bs, C, 4, axis=axis, outs=[(o, 4) for o in outs])
    s = torch.full((B, H, W, C + 8), 7.0, device='cuda')
    ops.cpca_fanin([(_wide(v), 4) for v in t['ts']], (_wide(t['through']), 4), ws, bs, C, axis=axis, out=s, o_coff=4)
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(zip(outs, _want_fanout(t, axis, False, True))):
        rel_close(got[..., 4:4 + C], want, what=f'sliced fan-out {TAPS[k]} along {axis}')
        _untouched(got, C, f'fan-out {TAPS[k]}')
    rel_close(s[..., 4:4 + C], _want_fanin(t, axis, False, True), what=f'sliced fan-in along {axis}')
    _untouched(s, C, 'fan-in')
    if axis == 'h':
        return
    inputs, want, _ = _wgrad_case(shape, 78)
    sl = lambda v: (_wide(v), 4)                                  # noqa: E731
    targets = [[torch.zeros(C, k, device='cuda') for k in TAPS], [torch.zeros(C, k, device='cuda') for k in TAPS],
               [torch.zeros(C, device='cuda') for _ in TAPS], [torch.zeros(C, device='cuda') for _ in TAPS]]
    ops.cpca_wgrad(sl(inputs['u']), [sl(v) for v in inputs['ts']], sl(inputs['ds']), [sl(v) for v in inputs['dts']], C, *targets)
    for gi, k in itertools.product(range(4), range(3)):
        rel_close(targets[gi][k].flatten(), want[gi][k].flatten(), what=f'sliced wgrad group {gi} taps {TAPS[k]}')
    x, y, d = t['x'], t['through'], t['have']
    out = ops.cpca_gate(_wide(x), _wide(y), C, 4, 4, out=torch.full((B, H, W, C + 8), 7.0, device='cuda'), o_coff=4)
    dx, dy = ops.cpca_gate_backward(_wide(d), _wide(x), _wide(y), C, 4, 4, 4)
    rel_close(out[..., 4:4 + C], x.double() * y.double(), what='sliced gate product')
    _untouched(out, C, 'gate product')
    rel_close(dx, d.double() * y.double(), what='gate backward dx')
    rel_close(dy, d.double() * x.double(), what='gate backward dy')


@pytest.mark.parametrize('shape', [(2, 5, 7, 32), (1, 67, 35, 16)], ids=IDS)
def test_fanin_accumulates(shape):
    """accumulate=True adds the fan-in to what the output holds; two launches from the same start are bit-identical."""
    from somi_amd import ops
    B, H, W, C = shape
    t = _case(shape, 5)
    g = {k: [v.cuda() for v in val] if isinstance(val, list) else val.cuda() for k, val in t.items()}
    for axis in 'wh':
        runs = []
        for _ in range(2):
            out = g['have'].clone()
            ops.cpca_fanin(g['ts'], g['through'], g['ws'], g['bs'], C, axis=axis, flip=True, out=out, accumulate=True)
            runs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(*runs), 'two accumulating launches differ'
        rel_close(runs[0], _want_fanin(t, axis, True, True) + t['have'].double(), what=f'{shape} fan-in along {axis} accumulated')


def test_small_passes_against_fp64():
    """The sum of two sigmoids and its backward; the first pixel of every channel maximum, ties included."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(9)
    z, dg = torch.randn(6, 40, generator=gen) * 3, torch.randn(3, 40, generator=gen)
    z64 = z.double().requires_grad_(True)
    g64 = torch.sigmoid(z64[:3]) + torch.sigmoid(z64[3:])
    g64.backward(dg.double())
    rel_close(ops.cpca_sigmoid2(z.cuda()), g64, what='sigmoid2')
    rel_close(ops.cpca_sigmoid2_backward(z.cuda(), dg.cuda()), z64.grad, what='sigmoid2 backward')
    x = (torch.randn(2, 9, 31, 12, generator=gen) * 2).round() / 2          # a grid of 1/2: ties
    xw = _wide(x)
    flat = x.reshape(2, -1, 12)
    mx = flat.max(1)[0]
    first = (flat == mx[:, None]).int().argmax(1)
    assert bool(((flat == mx[:, None]).sum(1) > 1).any()), 'the case has no tie'
    got = ops.argmax_pixel(xw, mx.cuda(), 12, 4)
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), first), 'not the first pixel of the maximum'


def test_channel_attention_backward_into_a_given_tensor():
    """CPCA_ChannelAttention alone: forward and dx against autograd on the restatement; backward(dx_out=) writes a channel slice of a wider
    tensor, adds to it with accumulate=True, and need_dx=False returns None with the MLP's gradients taken."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    from oracle.somi_ref.testing import fill_state
    gen = torch.Generator().manual_seed(4)
    ref = fill_state(R.CPCA_ChannelAttention(32, 8), 5)
    mine = MB.CPCA_ChannelAttention(32, 8)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda().train()
    x = torch.randn(2, 32, 6, 9, generator=gen).requires_grad_(True)
    y = ref(x)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    xd, dyd = nhwc(x.detach()).cuda(), nhwc(dy).cuda()
    rel_close(mine(Act(xd)).t, nhwc(y), what='channel attention forward')
    rel_close(mine.backward(Act(dyd)).t, nhwc(x.grad), what='channel attention dx')
    for (n, p), (_, q) in zip(mine.named_parameters(), ref.named_parameters()):
        rel_close(p.grad, q.grad, what=f'channel attention d{n}', atol=2e-5)
    have = torch.randn(2, 6, 9, 40, generator=gen)
    for accumulate in (False, True):
        mine(Act(xd))
        out = have.clone().cuda()
        got = mine.backward(Act(dyd), dx_out=Act(out, 4, 32), accumulate=accumulate)
        assert got.t.data_ptr() == out.data_ptr() and got.coff == 4
        want = have.double()
        want[..., 4:36] = nhwc(x.grad).double() + (want[..., 4:36] if accumulate else 0)
        rel_close(out, want, what=f'channel attention dx_out, accumulate={accumulate}')
    mine(Act(xd))
    before = mine.fc1.weight.grad.clone()
    assert mine.backward(Act(dyd), need_dx=False) is None and not torch.equal(mine.fc1.weight.grad, before)


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """CPCA at the fixtures' two shapes, CPCABottleneck with and without the shortcut, C3CPCA with two bottlenecks: eval forward, training
    forward, dx and every parameter gradient - the summed gradient of the shared `conv` under its one name (parity.grads_close compares by
    name).  The input seeds are cpca_ref.BLOCK_SEEDS, chosen from the restatement alone."""
    check_block(R.BLOCKS[tag], R, R.block_shape(tag), tag, seed=R.BLOCK_SEEDS[tag])


@pytest.mark.parametrize('tag', ['cpca', 'cpcabottleneck_sc', 'c3cpca'])
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`, R what it held and dx what a plain backward of the same forward
    returns."""
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
def test_cpca_graph_training_step_eval_and_checkpoint(where, monkeypatch):
    """yolov5s 6.0 at width 0.25 with C3CPCA in the backbone ('c3': 1, 2, 3 and 1 bottlenecks) or a CPCA row behind SPPF ('row'), nc 10,
    batch 2, 64x64, against the oracle Model: one training forward, ComputeLoss and backward, the eval forward; two fresh TrainStep.step runs
    bit-identical; a pickled oracle model loads; a step moves the strip convs.  Seeds: cpca_ref.GRAPH_SEEDS."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-cpca-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-cpca-{where}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'cpca_ref'), f'yolov5s-cpca-{where}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    moved = [k for k in state if k.endswith(('dconv1_7.weight', 'dconv21_1.bias', 'dconv5_5.weight', 'ca.fc1.weight', 'ca.fc2.bias'))
             or (k.endswith(('.conv.weight', '.conv.bias')) and k.rsplit('.', 2)[0] + '.dconv5_5.weight' in state)]
    assert len(moved) == (7 * 7 if where == 'c3' else 7)
    for k in moved:
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
