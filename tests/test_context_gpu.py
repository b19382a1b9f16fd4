"""The dilated-convolution context blocks on the MI355X (ASPP; DWR, Bottleneck_DWRSeg / DWRSeg_Conv, C2f_DWR): the blocks against the test
restatement (tests/context_ref.py, pinned to the reference by tests/golden/block_*.npz) on the CPU - eval forward, training forward, input
gradient, every parameter gradient, running statistics - and the three yolov5_context_cfg graphs against the oracle Model."""
import copy

import pytest
import torch

import context_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nhwc,
                    rel_close)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """ASPP with the default rates (2, 4, 6) and with (1, 3) to another width, DWR, Bottleneck_DWRSeg with the shortcut and C2f_DWR with two
    blocks, at the fixtures' shape (batch 2, 64 channels, 7x9 - rates 4, 5 and 6 reach beyond the map from most pixels)."""
    check_block(R.BLOCKS[tag], R, R.BLOCK_SHAPE, tag, seed=R.BLOCK_SEEDS[tag])


@pytest.mark.parametrize('tag', ['aspp', 'dwr', 'dwrseg'])
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) - the signature every new block takes - leaves R + dx in `have`, R what it held and dx what a
    plain backward of the same forward returns."""
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


@pytest.mark.parametrize('where', ['aspp', 'dwr', 'both'])
def test_context_graph_training_step_and_eval(where, monkeypatch):
    """yolov5s 6.0 at width 0.25 with ASPP in SPPF's row ('aspp'), C2f_DWR in the P4 / P5 backbone rows ('dwr': 3 and 1 blocks) or both, nc 10,
    batch 2, 64x64, against the oracle Model: one training forward, ComputeLoss and backward, then the eval forward.  On 'both' also: two fresh
    TrainStep.step runs are bit-identical, and a pickled oracle model loads through checkpoint.attempt_load."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-context-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-context-{where}')
    assert mine.fuse() is mine
    if where == 'both':
        check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
        check_checkpoint_roundtrip(ref, imgs, ('oracle', 'context_ref'), 'yolov5s-context-both')
