"""CPU checks of the Ghost module set (models/hub/yolov5s-ghost.yaml): the product graph is built like the reference's - parameter names and
shapes, strides, save list, anchors - and the grouped Conv's limits are explicit."""
import pytest
import torch

from ghost_ref import register


@pytest.mark.parametrize('width', [0.5, 0.25])
def test_yolov5s_ghost_graph_matches_the_reference(width, monkeypatch):
    from oracle.somi_ref import Model as OModel
    from somi_amd.configs import yolov5_ghost_cfg
    from somi_amd.model import Model
    register(monkeypatch)
    cfg = yolov5_ghost_cfg(width)
    ref, mine = OModel(cfg), Model(cfg)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save
    assert torch.equal(mine.model[-1].anchors, ref.model[-1].anchors)
    assert [m.type for m in mine.model] == [m.type for m in ref.model]
    mine.load_state_dict(ref.state_dict())                       # reference-format state_dicts load


def test_ghost_blocks_keep_reference_parameter_layout():
    import ghost_ref as R
    from somi_amd import blocks as MB
    for mk in (lambda M: M.DWConv(12, 8, 5, 2), lambda M: M.DWConv(8, 16, 3), lambda M: M.GhostConv(16, 32, 3, 2, act=False),
               lambda M: M.GhostBottleneck(16, 32, 3, 2), lambda M: M.C3Ghost(32, 32, 2)):
        a, b = mk(R), mk(MB)
        assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    assert MB.DWConv(12, 8).conv.groups == 4
    assert isinstance(MB.GhostConv(8, 16, act=False).cv2.act, torch.nn.Identity)


def test_grouped_conv_limits_are_explicit():
    from somi_amd import blocks as MB
    with pytest.raises(NotImplementedError, match='dilated'):
        MB.Conv(8, 8, 3, 1, None, 8, d=2)
    with pytest.raises(NotImplementedError, match='input channels per group'):
        MB.Conv(64, 64, 3, 1, None, 2)
    with pytest.raises(NotImplementedError, match='grouped Conv'):
        MB.Conv(8, 8, 7, 1, None, 8)
    assert MB.Conv(64, 64, 3, 1, None, 4).conv.groups == 4       # 16 per group is the widest on the path


def test_c3tr_is_still_rejected():
    from somi_amd.configs import yolov5_ghost_cfg
    from somi_amd.model import Model
    cfg = yolov5_ghost_cfg(0.25)
    cfg['backbone'][9][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)
