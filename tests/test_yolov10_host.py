"""CPU checks of the YOLOv10 module set (models/hub/yolov10.yaml): the test restatement (tests/yolov10_ref.py) reproduces the reference's
own classes through the tests/golden/block_*.npz fixtures, the product graph is built like the reference's - parameter names and shapes,
strides, save list, anchors, parameter counts - and the limits of the MI355X path are explicit."""
import os

import numpy as np
import pytest
import torch

import yolov10_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

FIXTURES = {'c2f_sc': lambda: R.C2f(32, 32, 2, True), 'c2f_nosc': lambda: R.C2f(24, 32, 1, False), 'scdown': lambda: R.SCDown(16, 32, 3, 2),
            'cib': lambda: R.CIB(32, 32, True, e=1.0), 'c2fcib': lambda: R.C2fCIB(32, 32, 1, True), 'attnpsa': lambda: R.AttentionPSA(128, 2),
            'psa': lambda: R.PSA(256, 256)}


@pytest.mark.parametrize('tag', list(FIXTURES))
def test_restatement_reproduces_the_reference_blocks(tag):
    """Eval and train outputs of the reference's classes under fill_state weights (oracle.gen_golden.run_block), fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    mod = fill_state(FIXTURES[tag](), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['in0'])
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        err = (y - want).abs().max().item()
        assert err <= 1e-5 * want.abs().max().item(), f'{tag} {mode}: {err:.3e}'


@pytest.mark.parametrize('width,depth,anchors,params', [(0.25, 0.33, None, 1520663), (1.0, 1.0, 3, 39046343)])
def test_yolov10_graph_matches_the_reference(width, depth, anchors, params, monkeypatch):
    from oracle.somi_ref import Model as OModel
    from somi_amd.configs import yolov10_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov10_cfg(width, depth, anchors=anchors)
    ref, mine = OModel(cfg), Model(cfg)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters()) == params
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save
    assert torch.equal(mine.model[-1].anchors, ref.model[-1].anchors)
    if anchors == 3:                                              # the yaml's placeholders, list(range(6)) per level, over the strides
        assert mine.model[-1].anchors[0].flatten().tolist() == [0, 0.125, 0.25, 0.375, 0.5, 0.625]
    assert [m.type for m in mine.model] == [m.type for m in ref.model]
    mine.load_state_dict(ref.state_dict())                       # reference-format state_dicts load


def test_yolov10_cfg_is_the_hub_yaml():
    from somi_amd.configs import COCO_ANCHORS, yolov10_cfg
    cfg = yolov10_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (10, 1.0, 1.0, COCO_ANCHORS)
    assert yolov10_cfg(anchors=3)['anchors'] == 3
    assert [row[2] for row in cfg['backbone']] == ['Conv', 'Conv', 'C2f', 'Conv', 'C2f', 'SCDown', 'C2f', 'SCDown', 'C2fCIB', 'SPPF', 'PSA']
    assert cfg['head'][-1] == [[16, 19, 22], 1, 'Detect', ['nc', 'anchors']]


def test_yolov10_blocks_keep_reference_parameter_layout():
    from somi_amd import blocks as MB
    for mk in (lambda M: M.C2f(24, 32, 2, True), lambda M: M.SCDown(16, 32, 3, 2), lambda M: M.CIB(32, 32, True, e=1.0),
               lambda M: M.C2fCIB(32, 64, 2, True), lambda M: M.AttentionPSA(128, 2), lambda M: M.PSA(256, 256)):
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    assert MB.PSA(512, 512).attn.num_heads == 4


def test_yolov10_limits_are_explicit():
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov10_cfg
    from somi_amd.model import Model
    with pytest.raises(NotImplementedError, match='RepVGGDW'):
        MB.C2fCIB(64, 64, 1, True, lk=True)
    with pytest.raises(NotImplementedError, match='multiple of 64'):
        MB.PSA(320, 320)                                          # 160 channels per branch
    with pytest.raises(NotImplementedError, match='head_dim 64'):
        MB.AttentionPSA(128, 4)
    with pytest.raises(ValueError, match='c1 == c2'):
        MB.PSA(256, 512)
    with pytest.raises(NotImplementedError, match='multiple of 64'):
        Model(yolov10_cfg(0.33, 0.33))                            # PSA at 344 channels: 172 per branch, head_dim 86


def test_c3tr_is_still_rejected_next_to_the_yolov10_set():
    from somi_amd.configs import yolov10_cfg
    from somi_amd.model import Model
    cfg = yolov10_cfg(0.25, 0.33)
    cfg['backbone'][8][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)
