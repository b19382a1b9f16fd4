"""Grouped / depthwise convolution and the Ghost module set on the MI355X (DWConv, GhostConv, GhostBottleneck, C3Ghost,
models/hub/yolov5s-ghost.yaml): the kernels against fp64 F.conv2d(groups=...) on the CPU, the blocks against torch autograd on the CPU
reference classes (tests/ghost_ref.py), the whole graph against the oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import ghost_ref as R
from parity import (check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nchw, nhwc,
                    rel_close)

pytestmark = pytest.mark.gpu


def _p4(c):
    return (c + 3) // 4 * 4


# (B, H, W, c1, c2, k, stride): depthwise 4 / 12 / 64 / 256 / 80 (stored at 96: pad channels), multiplier 8 -> 16, gcd grouping 12 -> 8
KCASES = [(1, 13, 17, 4, 4, 3, 1), (3, 13, 17, 12, 12, 5, 2), (1, 16, 15, 64, 64, 3, 2), (1, 9, 7, 256, 256, 5, 1), (3, 11, 10, 80, 80, 3, 1),
          (3, 13, 17, 8, 16, 3, 1), (1, 13, 17, 12, 8, 5, 2), (1, 6, 5, 8, 8, 1, 2)]


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v), 'two launches differ'
    return a


@pytest.mark.parametrize('case', KCASES, ids=lambda c: 'x'.join(map(str, c)))
def test_grouped_conv_kernels(case):
    """Forward (raw + BatchNorm partial sums; folded + act into a channel slice with a residual slice), data gradient (accumulating, and
    with a second added slice) and weight gradient (accumulating) against fp64 on the CPU; every launch twice, bit-identical."""
    from somi_amd import ops
    from somi_amd.pack import pack_gconv_weight, pad4
    B, H, W, c1, c2, k, s = case
    g = __import__('math').gcd(c1, c2)
    gen = torch.Generator().manual_seed(sum(case))
    xcs = _p4(c1) + 8
    xall = torch.randn(B, H, W, xcs, generator=gen)
    x64 = nchw(xall[..., 4:4 + c1]).double().requires_grad_(True)
    w = torch.randn(c2, c1 // g, k, k, generator=gen) / k
    y64 = F.conv2d(x64, w.double(), None, s, k // 2, 1, g)
    Ho, Wo = y64.shape[2:]
    cp = pad4(c2)
    wp = pack_gconv_weight(w, cp).cuda()
    xd = xall.cuda()
    piv = torch.zeros(cp)
    piv[:c2] = torch.randn(c2, generator=gen) * 0.1
    pivd = piv.cuda()

    def fwd():
        st = {'pivot': pivd}
        y = ops.gconv2d_nhwc(xd, wp, c1=c1, c2=c2, groups=g, k=k, stride=s, x_coff=4, cw=cp, bn_stats=st)
        return y, st['part']
    y, part = _twice(fwd)
    yw = nhwc(y64.detach())
    rel_close(y[..., :c2], yw, what='forward')
    assert not y[..., c2:].any(), 'pad channels are not zero'
    t = yw - piv[:c2].double()
    rel_close(part[0].sum(0)[:c2], t.sum((0, 1, 2)), what='partial sums', atol=1e-4 * t.abs().sum().item() / c2)
    rel_close(part[1].sum(0)[:c2], (t * t).sum((0, 1, 2)), what='partial sums of squares')

    # folded: bias + SiLU + residual into slices
    bias = torch.zeros(cp)
    bias[:c2] = torch.randn(c2, generator=gen)
    res = torch.randn(B, Ho, Wo, c2 + 8, generator=gen)
    out0 = torch.full((B, Ho, Wo, c2 + 12), 7.0).cuda()

    def fold():
        o = out0.clone()
        ops.gconv2d_nhwc(xd, wp, bias.cuda(), c1=c1, c2=c2, groups=g, k=k, stride=s, x_coff=4, out=o, y_coff=8, cw=c2, act='silu',
                         residual=res.cuda(), res_coff=4)
        return (o,)
    o, = _twice(fold)
    want = F.silu(y64.detach() + bias[:c2].double().view(1, -1, 1, 1))
    rel_close(o[..., 8:8 + c2], nhwc(want) + res[..., 4:4 + c2].double(), what='folded forward')
    assert (o[..., :8] == 7).all() and (o[..., 8 + c2:] == 7).all(), 'channels outside the slice were written'

    # data gradient: dy a channel slice, written into a slice, + an accumulated slice + a second added slice
    dyall = torch.randn(B, Ho, Wo, cp + 4, generator=gen)
    dy = dyall[..., 4:4 + c2]
    (dx64,) = torch.autograd.grad(y64, x64, nchw(dy).double().contiguous())
    acc = torch.randn(B, H, W, xcs, generator=gen)
    add2 = torch.randn(B, H, W, _p4(c1), generator=gen)
    cx = c1 if c1 % 4 == 0 else _p4(c1)

    def dgrad():
        o = acc.clone().cuda()
        ops.gconv2d_dgrad_nhwc(dyall.cuda(), wp, H=H, W=W, c1=c1, c2=c2, groups=g, k=k, stride=s, dy_coff=4, out=o, dx_coff=4, cx=cx, accumulate=o,
                               acc_coff=4, accumulate2=add2.cuda())
        return (o,)
    o, = _twice(dgrad)
    rel_close(o[..., 4:4 + c1], acc[..., 4:4 + c1].double() + add2[..., :c1].double() + nhwc(dx64), what='dgrad')
    assert torch.equal(o[..., :4].cpu(), acc[..., :4])

    # weight gradient, accumulated into an existing gradient
    wv = w.double().requires_grad_(True)
    (dw64,) = torch.autograd.grad(F.conv2d(x64.detach(), wv, None, s, k // 2, 1, g), wv, nchw(dy).double().contiguous())
    g0 = torch.randn(w.shape, generator=gen)

    def wgrad():
        o = g0.clone().cuda()
        ops.gconv2d_wgrad_nhwc(xd, dyall.cuda(), c1=c1, c2=c2, groups=g, k=k, stride=s, x_coff=4, dy_coff=4, out=o, accumulate=True)
        return (o,)
    o, = _twice(wgrad)
    rel_close(o, g0.double() + dw64, what='wgrad')


BLOCKS = {'dwconv_k5s2': (lambda M: M.DWConv(16, 16, 5, 2), (2, 16, 13, 17)),
          'dwconv_mult': (lambda M: M.DWConv(8, 16, 3, 1), (3, 8, 9, 11)),
          'dwconv_gcd': (lambda M: M.DWConv(12, 8, 5, 2, act=False), (1, 12, 13, 17)),
          'ghost_k1s1': (lambda M: M.GhostConv(16, 32, 1, 1), (2, 16, 12, 10)),
          'ghost_k3s2_noact': (lambda M: M.GhostConv(16, 16, 3, 2, act=False), (2, 16, 13, 17)),
          'ghost_k1s2_noact': (lambda M: M.GhostConv(12, 16, 1, 2, act=False), (1, 12, 9, 9)),
          'ghostbottleneck_s1': (lambda M: M.GhostBottleneck(16, 16), (2, 16, 11, 13)),
          'ghostbottleneck_s2': (lambda M: M.GhostBottleneck(16, 32, 3, 2), (3, 16, 13, 17)),
          'c3ghost_n1': (lambda M: M.C3Ghost(32, 32, 1), (2, 32, 10, 10)),
          'c3ghost_n2': (lambda M: M.C3Ghost(24, 32, 2, False), (2, 24, 9, 11))}


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_ghost_blocks_eval_train_backward(tag):
    """Eval forward (BatchNorm folded), training forward, hand-written backward against torch autograd on the CPU classes: output, dx,
    every parameter gradient (BatchNorm's included) and the updated running statistics."""
    mk, shape = BLOCKS[tag]
    check_block(mk, R, shape, tag)


def test_yolov5s_ghost_graph_training_step_eval_and_checkpoint(monkeypatch):
    """yolov5s-ghost at width 0.25, batch 2, 160x160 against the oracle Model: one training forward, ComputeLoss and backward (outputs, loss,
    every parameter gradient, BatchNorm statistics), the eval forward; two fresh TrainStep.step runs bit-identical; attempt_load of a
    pickled ghost model reproduces the eval forward."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_ghost_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov5_ghost_cfg(0.25)
    ref = fill_state(OModel(cfg), 3)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    ref.hyp = mine.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 160, nc=80, seed=2)
    check_train_step(ref, mine, imgs, targets, 'yolov5s-ghost')
    check_eval(ref, mine, imgs, 'yolov5s-ghost')
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle',), 'yolov5s-ghost')
