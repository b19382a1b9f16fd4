"""The slim-neck blocks on the MI355X (GSConv, GSBottleneck, VoVGSCSP, GSCBAMBottleneck, VoVGSCSPCBAM; gsconv.hip): the shuffle and its
inverse bit for bit against the reference's reshape / permute expression, the fused inference tail against an fp64 restatement of its two
depthwise convs, the blocks against torch autograd on the CPU restatement (tests/slimneck_ref.py), the graph of
configs.yolov5_slimneck_cfg against the oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import slimneck_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step,
                    check_two_steps_bit_identical, nhwc, rel_close)

pytestmark = pytest.mark.gpu

# half widths: one quad; two; three - the group of eight source channels that straddles x1 | x_2, and no power of two; five - the same, ten
# source quads in sixteen lanes; 17 quads a half, 34 source quads: more than 32 lanes wide, no power of two
WIDTHS = (4, 8, 12, 20, 68)
# three images (nothing crosses images); one pixel; ragged
SHAPES = [(3, 5, 7), (1, 1, 1), (2, 33, 3)]
# per half width a shape at which a workgroup WALKS two tiles (ops.gs_tiles_per_workgroup > 1), as every batch-32 launch of training does:
# the plan walks once 2 x 2048 workgroups' worth of tiles exist, and a tile is 256 / nq pixels, so the narrow widths need many pixels.
# The sizes are no multiple of a tile: the last workgroup's second tile lies past the end (the loop's early exit), the one before is ragged.
WALK_SHAPES = {4: (1, 1024, 515), 8: (1, 512, 515), 12: (1, 256, 515), 20: (1, 128, 515), 68: (1, 129, 131)}
IDS = lambda s: 'x'.join(map(str, s))     # noqa: E731
SENTINEL = -77.0


def test_walk_shapes_walk():
    """Every WALK_SHAPES entry makes the two streaming kernels walk two tiles per workgroup; every shape of SHAPES stays at one - so both forms
    of the loop are under test."""
    from somi_amd import ops
    for ch, (b, h, w) in WALK_SHAPES.items():
        assert ops.gs_tiles_per_workgroup(b * h * w, ch) == 2, (ch, b, h, w)
    assert all(ops.gs_tiles_per_workgroup(b * h * w, ch) == 1 for ch in WIDTHS for b, h, w in SHAPES)


def _reference_shuffle(x1, x_2):
    """models/common.py:9602-9610 on NHWC halves -> NHWC."""
    x2 = torch.cat((x1, x_2), 3).permute(0, 3, 1, 2).contiguous()
    b, n, h, w = x2.size()
    y = x2.reshape(b * n // 2, 2, h * w).permute(1, 0, 2).reshape(2, -1, n // 2, h, w)
    return torch.cat((y[0], y[1]), 1).permute(0, 2, 3, 1).contiguous()


def _in_slice(t, coff, total):
    """t (B,H,W,c) as the slice [coff, coff + c) of a `total`-channel tensor filled with SENTINEL, on the GPU."""
    wide = torch.full((*t.shape[:3], total), SENTINEL)
    wide[..., coff:coff + t.shape[3]] = t
    return wide.cuda()


def _untouched(wide, coff, c, what):
    assert bool((wide[..., :coff] == SENTINEL).all()) and bool((wide[..., coff + c:] == SENTINEL).all()), f'{what}: channels around the slice were written'


@pytest.mark.parametrize('ch', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES + ['walk'], ids=lambda s: s if isinstance(s, str) else IDS(s))
def test_shuffle_and_unshuffle(shape, ch):
    """shuffle(z1, y2) with no affine map (and with scale 1, shift 0) and no activation equals the reference's expression bit for bit, on whole
    tensors and on slices of wider tensors at non-zero offsets whose other channels stay untouched; unshuffle inverts it bit for bit; with a real
    scale / shift, SiLU and a residual it is within 1e-3 of fp64; two launches are bit-identical."""
    from somi_amd import ops
    B, H, W = WALK_SHAPES[ch] if shape == 'walk' else shape
    gen = torch.Generator().manual_seed(ch + B * H * W)
    z1, y2, res = torch.randn(B, H, W, ch, generator=gen), torch.randn(B, H, W, ch, generator=gen), torch.randn(B, H, W, 2 * ch, generator=gen)
    scale, shift = torch.randn(ch, generator=gen), torch.randn(ch, generator=gen)
    want = _reference_shuffle(z1, y2)
    what = f'c_ {ch} at {(B, H, W)}'
    # whole tensors
    got = ops.gs_shuffle_affine_act(z1.cuda(), y2.cuda(), ch)
    assert torch.equal(got.cpu(), want), f'{what}: the shuffle is not the reference expression'
    one = ops.gs_shuffle_affine_act(z1.cuda(), y2.cuda(), ch, torch.ones(ch).cuda(), torch.zeros(ch).cuda())
    assert torch.equal(one.cpu(), want), f'{what}: scale 1, shift 0 changes bits'
    d1, d2 = ops.gs_unshuffle(got, ch)
    assert torch.equal(d1.cpu(), z1) and torch.equal(d2.cpu(), y2), f'{what}: unshuffle does not invert shuffle'
    # slices of wider tensors: z1 at 4 of ch + 8, y2 at 8 of ch + 12, out at 4 of 2 ch + 12, residual at 8 of 2 ch + 8
    zw, yw, rw = _in_slice(z1, 4, ch + 8), _in_slice(y2, 8, ch + 12), _in_slice(res, 8, 2 * ch + 8)
    want64 = _reference_shuffle(z1.double(), F.silu(y2.double() * scale.double() + shift.double())) + res.double()
    runs = []
    for _ in range(2):
        ow = torch.full((B, H, W, 2 * ch + 12), SENTINEL).cuda()
        ops.gs_shuffle_affine_act(zw, yw, ch, scale.cuda(), shift.cuda(), 'silu', 4, 8, out=ow, o_coff=4, residual=rw, res_coff=8)
        runs.append(ow.cpu())
    assert torch.equal(*runs), f'{what}: two launches differ'
    _untouched(runs[0], 4, 2 * ch, f'{what} shuffle')
    rel_close(runs[0][..., 4:4 + 2 * ch], want64, what=f'{what} shuffle with affine, SiLU and residual')
    ow = torch.full((B, H, W, 2 * ch + 12), SENTINEL).cuda()
    ops.gs_shuffle_affine_act(zw, yw, ch, None, None, 'none', 4, 8, out=ow, o_coff=4)
    assert torch.equal(ow.cpu()[..., 4:4 + 2 * ch], want), f'{what}: the shuffle between slices is not the reference expression'
    d1w, d2w = torch.full((B, H, W, ch + 4), SENTINEL).cuda(), torch.full((B, H, W, ch + 8), SENTINEL).cuda()
    for _ in range(2):
        ops.gs_unshuffle(ow, ch, 4, d1=d1w, d2=d2w, d1_coff=4, d2_coff=0)
    assert torch.equal(d1w.cpu()[..., 4:], z1) and torch.equal(d2w.cpu()[..., :ch], y2), f'{what}: unshuffle between slices'
    _untouched(d1w.cpu(), 4, ch, f'{what} d1')
    _untouched(d2w.cpu(), 0, ch, f'{what} d2')


def _tail64(x1, w1, b1, w2, b2, act, padded_first_stage=False):
    """x_2 of a GSConv behind x1 (NHWC fp64) with BatchNorm folded: act(dw2(t) + b2), t = act(dw1(x1) + b1) inside the image and zero outside.
    padded_first_stage: the WRONG form a fused kernel computes when it evaluates the first stage on the halo too - the ring around the image
    then holds act(b1 + the taps that reach the image) where the second conv must read zeros."""
    C = x1.shape[3]
    a = F.silu if act == 'silu' else (lambda v: v)
    x = x1.permute(0, 3, 1, 2)
    if padded_first_stage:
        t = a(F.conv2d(x, w1.view(C, 1, 3, 3), b1, padding=2, groups=C))
        y = a(F.conv2d(t, w2.view(C, 1, 3, 3), b2, padding=0, groups=C))
    else:
        t = a(F.conv2d(x, w1.view(C, 1, 3, 3), b1, padding=1, groups=C))
        y = a(F.conv2d(t, w2.view(C, 1, 3, 3), b2, padding=1, groups=C))
    return y.permute(0, 2, 3, 1)


# one pixel; one row; one column; smaller than the stencil's reach; exactly a tile of either form (16 x 16, and 8 x 16 from 8 quads up); a tile
# plus 3 on both axes; two tiles plus 1 (the seams)
MAPS = [(1, 1), (1, 9), (9, 1), (2, 3), (16, 16), (8, 16), (19, 19), (33, 33)]
# half widths of the tail: 1, 2 and 3 quads (the three narrow forms, the last with an idle lane in four); 5 quads (two chunks of 4, the second
# with one); 18 quads (the wide form: three chunks of 8, the last with two)
TAIL_WIDTHS = (4, 8, 12, 20, 72)


@pytest.mark.parametrize('ch', TAIL_WIDTHS)
@pytest.mark.parametrize('hw', MAPS, ids=IDS)
def test_eval_tail_against_fp64(hw, ch):
    """ops.gs_tail on two images, with SiLU and without activation, with and without a residual, from a slice into a slice of wider tensors
    (the weights' row stride wider than the layer): 1e-3 of fp64, other channels untouched, two launches bit-identical.  The biases are of
    order 1, so the intermediate's zero outside the image shows: the border pixels of the expected result differ from the form that pads the
    second conv with act(b1 + ...) by more than the bar, and the kernel has to be on the right side of that."""
    from somi_amd import ops
    from somi_amd.pack import pack_gconv_weight
    H, W = hw
    B = 2
    gen = torch.Generator().manual_seed(ch + 100 * H + W)
    x1, res = torch.randn(B, H, W, ch, generator=gen), torch.randn(B, H, W, 2 * ch, generator=gen)
    w1, w2 = torch.randn(ch, 3, 3, generator=gen) / 3, torch.randn(ch, 3, 3, generator=gen) / 3
    b1, b2 = 1 + torch.rand(ch, generator=gen), -1 - torch.rand(ch, generator=gen)
    p1, p2 = (pack_gconv_weight(w.view(ch, 1, 3, 3), ch + 4).cuda() for w in (w1, w2))
    xw, rw = _in_slice(x1, 4, ch + 8), _in_slice(res, 8, 2 * ch + 12)
    for act in ('silu', 'none'):
        x2 = _tail64(x1.double(), w1.double(), b1.double(), w2.double(), b2.double(), act)
        wrong = _tail64(x1.double(), w1.double(), b1.double(), w2.double(), b2.double(), act, padded_first_stage=True)
        border = torch.ones(H, W, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        scale = x2.abs().max().item()
        apart = (x2 - wrong)[:, border].abs().amax(-1).min().item()     # at every border pixel, in its most affected channel
        print(f'c_ {ch} at {H}x{W}, {act}: the two paddings are at least {apart:.3e} apart on the border, scale {scale:.3e}')
        assert apart > 1e-3 * scale, 'the case does not tell the two paddings apart'
        assert not (~border).any() or (x2 - wrong)[:, ~border].abs().max().item() < 1e-12, 'the two paddings differ inside the map'
        for with_res in (False, True):
            what = f'tail c_ {ch} at {B}x{H}x{W}, {act}, residual {with_res}'
            want = _reference_shuffle(x1.double(), x2) + (res.double() if with_res else 0)
            runs = []
            for _ in range(2):
                ow = torch.full((B, H, W, 2 * ch + 8), SENTINEL).cuda()
                ops.gs_tail(xw, p1, b1.cuda(), p2, b2.cuda(), ch, act, 4, out=ow, o_coff=4, residual=rw if with_res else None, res_coff=8)
                runs.append(ow.cpu())
            assert torch.equal(*runs), f'{what}: two launches differ'
            _untouched(runs[0], 4, 2 * ch, what)
            rel_close(runs[0][..., 4:4 + 2 * ch], want, what=what)
            if not with_res:
                # the x1 half is a copy, and the x_2 half alone holds the bar of ITS scale (with SiLU behind a negative bias x_2 is much smaller than x1)
                assert torch.equal(runs[0][..., 4:4 + ch // 2], x1[..., 0::2]), f'{what}: x1\'s even channels are not copied'
                got2 = torch.cat((runs[0][..., 4 + ch // 2:4 + ch], runs[0][..., 4 + ch + ch // 2:4 + 2 * ch]), 3)
                rel_close(got2, torch.cat((want[..., ch // 2:ch], want[..., ch + ch // 2:]), 3), what=f'{what}, the x_2 half')
    whole = ops.gs_tail(x1.cuda(), p1, b1.cuda(), p2, b2.cuda(), ch, 'none')        # whole tensors, an output of its own
    rel_close(whole, _reference_shuffle(x1.double(), x2), what=f'tail c_ {ch} at {B}x{H}x{W} on whole tensors')


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """Every fixture case: eval forward (the fused tail), training forward, dx, every parameter gradient, every running statistic.  `res` has
    no gradient on either side and keeps its statistics.  The input seeds are slimneck_ref.BLOCK_SEEDS, chosen from the restatement alone."""
    has_res = tag in ('vovgscsp', 'vovgscspcbam')
    check_block(R.BLOCKS[tag], R, R.block_shape(tag), tag, seed=R.BLOCK_SEEDS[tag], no_grad=R.NO_GRAD if has_res else ())


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`, R what it held and dx what a plain backward of the same forward
    returns; need_dx=False returns None and still takes the parameter gradients."""
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
    dx = dx.t[..., dx.coff:dx.coff + x.shape[1]].clone()
    mine(Act(xd.clone()))
    have = torch.randn(xd.shape, generator=gen).cuda()
    before = have.clone()
    got = mine.backward(Act(dy.clone()), dx_out=Act(have), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have, before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')
    mine(Act(xd.clone()))
    first = next(p for n, p in mine.named_parameters() if n.endswith('cv2_1.conv.weight'))
    g = first.grad.clone()
    assert mine.backward(Act(dy.clone()), need_dx=False) is None and not torch.equal(first.grad, g), f'{tag}: need_dx=False'


def test_gsconv_writes_a_given_slice_with_a_residual():
    """GSConv.forward(x, out=<slice>, residual=<slice>) in eval and training mode: the slice holds the restatement's output plus the residual,
    the channels around it stay as they were."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case('gsconv_s2')
    mine = R.BLOCKS['gsconv_s2'](MB)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda()
    res = torch.randn(2, 5, 3, 48 + 8, generator=gen)
    for mode in ('eval', 'train'):
        ref.train(mode == 'train'), mine.train(mode == 'train')
        with torch.no_grad():
            want = nhwc(ref(x)).double() + res[..., 8:].double()
        out = torch.full((2, 5, 3, 48 + 12), SENTINEL).cuda()
        got = mine(Act(nhwc(x).cuda()), out=Act(out, 4, 48), residual=Act(res.cuda(), 8, 48))
        assert got.t.data_ptr() == out.data_ptr() and (got.coff, got.c) == (4, 48)
        _untouched(out.cpu(), 4, 48, f'GSConv {mode}')
        rel_close(out[..., 4:52], want, what=f'GSConv {mode} into a slice with a residual')


def test_slimneck_graph_training_step_eval_and_checkpoint(monkeypatch):
    """configs.yolov5_slimneck_cfg at width 0.25 / depth 0.33, nc 4, batch 2, 64x64 (the P5 rows run on 2x2 maps) against the oracle Model: one
    training forward, ComputeLoss and backward, the eval forward; two fresh TrainStep.step runs bit-identical; a pickled oracle model loads;
    a step moves the depthwise convs and the attention of a neck row and leaves `res` exactly where it was.  Seeds: slimneck_ref.GRAPH_SEEDS."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd import blocks as MB
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case()
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    assert [type(mine.model[i]) for i in (10, 13, 14, 17, 18, 20, 21, 23)] == [MB.GSConv, MB.VoVGSCSPCBAM] * 4
    # `res` never runs in the reference's forward (and here), so autograd leaves it without a gradient on both sides, which check_train_step
    # does not allow for: it starts from an explicit zero gradient on both sides, and must still hold exactly zero afterwards
    unused = [n for n, _ in ref.named_parameters() if '.res.' in n]
    assert len(unused) == 4 * 3
    for mod in (ref, mine):
        for n, p in mod.named_parameters():
            if n in unused:
                p.grad = torch.zeros_like(p)
    check_train_step(ref, mine, imgs, targets, 'yolov5s-slimneck')
    for mod in (ref, mine):
        assert not any(p.grad.any() for n, p in mod.named_parameters() if n in unused), 'an unused parameter received a gradient'
    check_eval(ref, mine, imgs, 'yolov5s-slimneck')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'slimneck_ref'), 'yolov5s-slimneck')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    after = m.state_dict()
    moved = [k for k in state if k.endswith(('cv2_1.conv.weight', 'cv2_2.bn.running_mean', 'channel_attention.shared_MLP.0.weight'))]
    assert len(moved) == 4 * (1 + 2) * 2 + 4 * 1, len(moved)       # per GSConv two; a row and its bottleneck's two GSConvs; one attention a bottleneck
    for k in moved:
        assert not torch.equal(after[k].cpu(), state[k]), f'a step left {k} where it was'
    still = [k for k in state if '.res.' in k]
    assert len(still) == 4 * 6
    for k in still:
        assert torch.equal(after[k].cpu(), state[k]), f'a step moved {k}, which never runs'
