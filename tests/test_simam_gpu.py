"""The SimAM attention family on the MI355X (SimAM, SimAMWithSlicing, SimAMWithFlexibleSlicing, Conv_SWS, PSSimAM; simam.hip): the four kernels
against an fp64 restatement, the blocks against torch autograd on the CPU restatement (tests/simam_ref.py), the yolov5s graphs of
configs.yolov5_simam_cfg against the oracle Model.  Bar 1e-3 relative (BASELINE); the fp32 CPU restatement itself sits at 1.2e-5 or better on
outputs and 5e-6 or better on gradients against fp64."""
import copy

import pytest
import torch

import simam_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step,
                    check_two_steps_bit_identical, nchw, nhwc, rel_close)

pytestmark = pytest.mark.gpu


def _case(mode, shape, t=None, st=None, seed=0, x=None):
    """Inputs of the four kernels (NHWC, fp32, CPU) and their fp64 results: stats and sums as (B, regions, C), out and dx with and without the
    added input.  The gradient is autograd's of the restatement; the per-region sums follow their definition."""
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(seed)
    t32 = dict(x=torch.randn(B, H, W, C, generator=gen) if x is None else x, dout=torch.randn(B, H, W, C, generator=gen),
               have=torch.randn(B, H, W, C, generator=gen))
    x64 = nchw(t32['x']).double().contiguous().requires_grad_(True)
    g64 = nchw(t32['dout']).double()
    lam = 1e-4
    out = {'map': lambda: R.gate(x64, H * W - 1, lam), 'quadrants': lambda: R.quadrants(x64, lam), 'windows': lambda: R.windows(x64, t, st, lam)}[mode]()
    out.backward(g64)
    regions, n = R.region_list(mode, H, W, t, st)
    mean, S, A, Bs = [], [], [], []
    xd = x64.detach()
    for ys, xs, w in regions:
        xr = xd[..., ys, xs]
        d = xr - xr.mean((2, 3), keepdim=True)
        D = 4 * ((d * d).sum((2, 3), keepdim=True) / n + lam)
        s = torch.sigmoid(d * d / D + 0.5)
        T = w * g64[..., ys, xs] * xr * s * (1 - s)
        mean.append(xr.mean((2, 3))), S.append((d * d).sum((2, 3))), A.append((T * d).sum((2, 3))), Bs.append((T * d * d).sum((2, 3)))
    want = dict(mean=torch.stack(mean, 1), S=torch.stack(S, 1), A=torch.stack(A, 1), B=torch.stack(Bs, 1), out=nhwc(out.detach()),
                out_add=nhwc(out.detach() + xd), dx=nhwc(x64.grad), dx_add=nhwc(x64.grad + g64))
    return t32, want


def _run(ops, g, C, grid):
    stats = ops.simam_stats(g['x'], C, grid)
    sums = ops.simam_backward_sums(g['dout'], g['x'], stats, C, grid)
    return dict(mean=stats[:, :, 0], S=stats[:, :, 1], A=sums[:, :, 0], B=sums[:, :, 1],
                out=ops.simam_apply(g['x'], stats, C, grid), out_add=ops.simam_apply(g['x'], stats, C, grid, add_input=True),
                dx=ops.simam_backward_input(g['dout'], g['x'], stats, sums, C, grid),
                dx_add=ops.simam_backward_input(g['dout'], g['x'], stats, sums, C, grid, add_input=True))


def _check(mode, shape, t=None, st=None, x=None):
    from somi_amd import ops
    B, H, W, C = shape
    t32, want = _case(mode, shape, t, st, 3 + sum(shape), x)
    g = {k: v.cuda() for k, v in t32.items()}
    grid = ops.simam_grid(mode, H, W, 1e-4, t, st)
    first, second = _run(ops, g, C, grid), _run(ops, g, C, grid)
    torch.cuda.synchronize()
    what = f'{mode} {shape}' + (f' t={t} st={st}' if t else '')
    for k in first:
        assert torch.equal(first[k], second[k]), f'{what}: two launches differ in {k}'
        rel_close(first[k], want[k], what=f'{what} {k}')
    return first, want


# a chunk is 8 * NL pixels of one region, NL = 256 / min(C / 4, 256) pixel lanes
MAP_SHAPES = [(2, 5, 7, 32), (1, 2, 1, 8),       # H != W; two pixels, n = 1
              (1, 67, 35, 16),                   # the pixel split: 2345 pixels in five chunks of 512, the last one ragged (297)
              (1, 3, 2, 1032)]                   # the channel-quad split: 258 quads in chunks of 256, the last one of 2
QUADRANT_SHAPES = [(1, 7, 5, 8), (1, 2, 4, 8),   # unequal regions sharing one n; the smallest allowed
                   (2, 33, 18, 16),
                   (1, 13, 11, 256)]             # the pixel split over unequal regions: chunks of 32, regions of 30, 36, 35 and 42 pixels - one
#                                                  chunk for the first, two (the second ragged) for the others
WINDOW_CASES = [((1, 11, 13, 8), 4, 4), ((1, 11, 13, 8), 4, 2), ((1, 11, 13, 8), 5, 3),    # r = 0, 0.5 and (t = 5) 0.3: uncovered pixels, 1 / k
                ((1, 8, 8, 8), 8, 4),            # one window is the whole map
                ((2, 40, 40, 32), 8, 4),
                ((1, 96, 96, 8), 4, 2)]          # the region split: 47 x 47 = 2209 windows in bands of two, the last band ragged (one window)


@pytest.mark.parametrize('shape', MAP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_whole_map_kernels_against_fp64(shape):
    """stats, apply, backward sums and backward input (the last two with and without the added input) at 1e-3 of each result's largest
    value; every kernel run twice, bit-identical."""
    _check('map', shape)


@pytest.mark.parametrize('shape', QUADRANT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_quadrant_kernels_against_fp64(shape):
    _check('quadrants', shape)


@pytest.mark.parametrize('shape,t,st', WINDOW_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_window_kernels_against_fp64(shape, t, st):
    """Also: the output is exactly 0 on pixels no window covers, exactly x with the added input, and their gradient 0 or g."""
    got, _ = _check('windows', shape, t, st)
    bare = R.coverage(shape[1], shape[2], t, st) == 0
    if bare.any():
        assert bool((got['out'].cpu()[:, bare] == 0).all()) and bool((got['dx'].cpu()[:, bare] == 0).all())


def test_statistics_about_the_mean_on_a_map_with_an_offset():
    """1000 + randn: sum x^2 - N mu^2 in fp32 is off by 2.3e-2 .. 3.4e-2 of the largest value here and fails the bar; statistics about the mean
    pass it (S itself is judged at the bar, next to the mean 1000 times its size)."""
    shape = (1, 9, 11, 8)
    x = 1000 + torch.randn(*shape, generator=torch.Generator().manual_seed(11))
    _check('map', shape, x=x)
    _check('windows', shape, 4, 2, x=x)


def test_a_constant_channel_gets_sigmoid_of_one_half():
    """One channel constant over the map: S = 0, the output is finite and x * sigmoid(0.5), the gradient finite (g * sigmoid(0.5))."""
    shape = (2, 5, 7, 8)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(5))
    x[..., 3] = 1.75
    got, want = _check('map', shape, x=x)
    assert bool((got['S'][..., 3] == 0).all())
    half = torch.sigmoid(torch.tensor(0.5, dtype=torch.float64))
    rel_close(got['out'][..., 3], torch.full(shape[:3], 1.75, dtype=torch.float64) * half, what='constant channel out')
    rel_close(got['dx'][..., 3], want['dx'][..., 3], what='constant channel dx')
    _check('quadrants', shape, x=x)


def _wide(t, dev='cuda'):
    """t as channels [4, 4 + c) of a tensor 8 channels wider, the rest 7.0 (a sentinel the kernels must leave)."""
    out = torch.full((*t.shape[:-1], t.shape[-1] + 8), 7.0)
    out[..., 4:4 + t.shape[-1]] = t
    return out.to(dev)


def _untouched(t, c, what):
    assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + c:] == 7.0).all()), f'{what}: a kernel wrote outside its slice'


@pytest.mark.parametrize('mode,shape,t,st', [('map', (2, 6, 5, 12), None, None), ('quadrants', (2, 7, 5, 12), None, None),
                                             ('windows', (2, 11, 13, 12), 4, 2)], ids=lambda v: str(v))
def test_kernels_on_slices_of_wider_tensors(mode, shape, t, st):
    """Input, output, dout and dx as channel slices at offset 4 of tensors 8 channels wider (PSSimAM's b is such a slice of cv1's output):
    nothing outside a slice is written; accumulate=True leaves R + dx, bit-identical over two runs."""
    from somi_amd import ops
    B, H, W, C = shape
    t32, want = _case(mode, shape, t, st, 77)
    grid = ops.simam_grid(mode, H, W, 1e-4, t, st)
    x, dout = _wide(t32['x']), _wide(t32['dout'])
    stats = ops.simam_stats(x, C, grid, 4)
    out = ops.simam_apply(x, stats, C, grid, 4, out=torch.full_like(x, 7.0), o_coff=4, add_input=True)
    sums = ops.simam_backward_sums(dout, x, stats, C, grid, 4, 4)
    dx = ops.simam_backward_input(dout, x, stats, sums, C, grid, 4, 4, out=torch.full_like(x, 7.0), dx_coff=4)
    runs = []
    for _ in range(2):
        acc = _wide(t32['have'])
        ops.simam_backward_input(dout, x, stats, sums, C, grid, 4, 4, out=acc, dx_coff=4, accumulate=True, add_input=True)
        runs.append(acc)
    torch.cuda.synchronize()
    rel_close(stats[:, :, 0], want['mean'], what=f'{mode} sliced mean')
    rel_close(stats[:, :, 1], want['S'], what=f'{mode} sliced S')
    rel_close(out[..., 4:4 + C], want['out_add'], what=f'{mode} sliced out')
    rel_close(sums[:, :, 0], want['A'], what=f'{mode} sliced A')
    rel_close(sums[:, :, 1], want['B'], what=f'{mode} sliced B')
    rel_close(dx[..., 4:4 + C], want['dx'], what=f'{mode} sliced dx')
    assert torch.equal(*runs), 'two accumulating launches differ'
    rel_close(runs[0][..., 4:4 + C], want['dx_add'] + t32['have'].double(), what=f'{mode} sliced dx accumulated')
    for name, ten in (('x', x), ('dout', dout), ('out', out), ('dx', dx), ('accumulated dx', runs[0])):
        _untouched(ten, C, name)


@pytest.mark.parametrize('tag', list(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """The six fixture blocks at the fixtures' shapes and Conv_SWS without overlap: eval forward, training forward, dx, every parameter gradient
    and the running statistics (parity.check_block).  The 16-channel gates run on whole tensors; PSSimAM's gate reads a slice at offset 16."""
    make, shape = R.BLOCKS[tag]
    check_block(make, R, shape, tag)


@pytest.mark.parametrize('tag', ['simam', 'simam_conv_sws', 'simam_pssimam'])
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`, R what it held and dx what a plain backward of the same forward
    returns."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case(tag)
    cin = x.shape[1]
    mine = R.BLOCKS[tag][0](MB)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda().train()
    xd = nhwc(x).cuda()
    y = mine(Act(xd.clone()))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    dx = mine.backward(Act(dy.clone()))
    dx = dx.t[..., dx.coff:dx.coff + cin].clone()
    mine(Act(xd.clone()))
    have = torch.randn(xd.shape, generator=gen).cuda()
    before = have.clone()
    got = mine.backward(Act(dy.clone()), dx_out=Act(have), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have, before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')


@pytest.mark.parametrize('where', R.WHERE)
def test_simam_graph_training_step_eval_and_checkpoint(where, monkeypatch):
    """yolov5s 6.0 at width 0.25 with a SimAM, SimAMWithSlicing or PSSimAM row behind SPPF, or Conv_SWS as the P3 and P4 stride-2 convs, nc 10,
    batch 2, against the oracle Model: one training forward, ComputeLoss and backward, the eval forward; two fresh TrainStep.step runs
    bit-identical; a pickled oracle model loads; a step moves the Conv_SWS and PSSimAM weights.  64 x 64 images - the two Conv_SWS rows see 16 x 16
    (3 x 3 windows at stride 4) and 8 x 8 (one window) - except 'slicing' at 128 x 128: at 64 x 64 its row would sit on a 2 x 2 map, quadrants of
    one pixel, which the reference turns into 0 / 0 and the block refuses by name (simam_ref.GRAPH_SIZE)."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-simam-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-simam-{where}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'simam_ref'), f'yolov5s-simam-{where}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    prefixes = {'sws': ('model.3.', 'model.5.'), 'ps': ('model.10.',)}.get(where, ())
    moved = [k for k in state if k.startswith(prefixes) and k.endswith(('conv.weight', 'bn.weight', 'bn.running_mean'))] if prefixes else []
    assert len(moved) == {'sws': 6, 'ps': 12}.get(where, 0)
    for k in moved:
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
