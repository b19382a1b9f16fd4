"""MultiSEAM (models/common.py:8508-8555) and SEAM with n > 1 stages (:8448-8505) on the MI355X against the CPU restatement (tests/seam_ref.py,
pinned to the reference's own classes by tests/golden/block_multiseam*.npz and block_seam_n2.npz): the block procedure of parity.check_block -
eval forward, training forward, dx, every parameter gradient, the running statistics of every BatchNorm - and the graph procedure on somi_cfg
with the three SEAM rows swapped.  Seeds: seam_ref.BLOCK_SEEDS / GRAPH_SEEDS, judged by the reference alone (tests/test_seam_host.py).
Single GPU only: the ops.SYNC_BN branches of the blocks are not run here."""
import copy

import pytest
import torch

import seam_ref as R
from parity import check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_seam_blocks_against_the_restatement(tag):
    """(2, 64, 15, 17): the branches see 5x5, 3x3 and 2x2 maps and every patch conv leaves rows and columns of dx no tap reaches; (2, 64, 7, 9): the
    p = 7 branch sees one pixel.  seam_n1 is the control: the form the path ran before."""
    make, shape = R.BLOCKS[tag]
    check_block(make, R, shape, tag, seed=R.BLOCK_SEEDS[tag])


@pytest.mark.parametrize('how', sorted(R.GRAPH_SEEDS))
def test_seam_graph_training_step_eval_and_checkpoint(how, monkeypatch):
    """somi_cfg at width 0.25 / depth 0.33, nc 10, with MultiSEAM rows ('multi') or SEAM rows of two stages ('seam2'), batch 2, 256x256 (the P4
    site is 16x16: a 2x2 map in the p = 7 branch), against the oracle Model: one training forward, ComputeLoss and backward, the eval forward; two
    fresh TrainStep.step runs bit-identical; a pickled oracle model loads; a step moves the new parameters and statistics."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd import blocks as MB
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(how)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    rows = [m for m in mine.model if isinstance(m, MB.MultiSEAM if how == 'multi' else MB.SEAM)]
    assert len(rows) == 3 and not any(type(m) is (MB.SEAM if how == 'multi' else MB.MultiSEAM) for m in mine.model)
    # ODConv_3rd's conv.reduction is unused in the reference's forward (and here), so autograd leaves it without a gradient on both sides, which
    # check_train_step does not allow for: it starts from an explicit zero gradient on both sides, and must still hold exactly zero afterwards
    unused = [n for n, _ in ref.named_parameters() if '.conv.reduction.' in n]
    assert unused
    for mod in (ref, mine):
        for n, p in mod.named_parameters():
            if n in unused:
                p.grad = torch.zeros_like(p)
    what = f'somi-{how}'
    check_train_step(ref, mine, imgs, targets, what)
    for mod in (ref, mine):
        assert not any(p.grad.any() for n, p in mod.named_parameters() if n in unused), 'an unused parameter received a gradient'
    check_eval(ref, mine, imgs, what)
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'seam_ref'), what)
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    leaves = ('DCovN2.0.weight', 'DCovN0.2.running_mean', 'fc.2.weight') if how == 'multi' else ('DCovN.4.0.fn.0.weight', 'DCovN.4.3.running_mean', 'fc.2.weight')
    moved = [k for k in state if k.endswith(leaves)]
    assert len(moved) == 3 * 3
    for k in moved:
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
