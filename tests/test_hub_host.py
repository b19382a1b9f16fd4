"""CPU checks of the remaining stock hub graphs (models/hub/yolov3.yaml, yolov3-spp.yaml, yolov3-tiny.yaml, yolov5-fpn.yaml, yolov5-panet.yaml,
yolov5-p6.yaml, yolov5-p7.yaml): the test restatement (tests/hub_ref.py) reproduces the reference's own classes through the
tests/golden/block_hub_*.npz fixtures, the product graphs are built like the reference's - parameter names, order and shapes, strides, save list,
anchors, parameter counts (also against tests/golden/hub_graphs.json, recorded from the reference's own Model) - the config helpers hold the yamls'
tables, and the limits of the MI355X path are explicit."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import hub_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _fixtures():
    from oracle.somi_ref import blocks as OB
    return {'hub_csp_sc': lambda: R.BottleneckCSP(32, 32, 1, True), 'hub_csp_nosc': lambda: R.BottleneckCSP(24, 32, 1, False),
            'hub_csp_n2': lambda: R.BottleneckCSP(32, 64, 2, True), 'hub_spp357': lambda: OB.SPP(32, 32, (3, 5, 7)),
            'hub_spp35': lambda: OB.SPP(32, 24, (3, 5)), 'hub_seq2': lambda: nn.Sequential(OB.Bottleneck(32, 32), OB.Bottleneck(32, 32)),
            'hub_padpool': lambda: nn.Sequential(nn.ZeroPad2d([0, 1, 0, 1]), nn.MaxPool2d(2, 1, 0))}


@pytest.mark.parametrize('tag', ['hub_csp_sc', 'hub_csp_nosc', 'hub_csp_n2', 'hub_spp357', 'hub_spp35', 'hub_seq2', 'hub_padpool'])
def test_restatement_reproduces_the_reference_blocks(tag):
    """Eval and train outputs of the reference's classes under fill_state weights (oracle.gen_golden.run_block), fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    mod = fill_state(_fixtures()[tag](), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['in0'])
    for mode in ('eval', 'train'):
        if f'out_{mode}' not in d:
            assert tag == 'hub_padpool' and mode == 'train'       # parameter-free: one output
            continue
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        assert y.shape == want.shape
        err = (y - want).abs().max().item()
        assert err <= 1e-5 * want.abs().max().item(), f'{tag} {mode}: {err:.3e}'
    if tag == 'hub_padpool':                                      # the fixture is there for the zero border: it must win somewhere
        assert (x < 0).any() and (torch.from_numpy(d['out_eval'])[:, :, -1, :] == 0).any()


@pytest.mark.parametrize('width,depth', [(1.0, 1.0), (0.25, 0.33)])
@pytest.mark.parametrize('name', list(R.HUB))
def test_hub_graph_matches_the_reference(name, width, depth, monkeypatch):
    from oracle.somi_ref import Model as OModel
    from somi_amd import blocks as MB
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = R.hub_cfg(name, width=width, depth=depth)
    ref, mine = OModel(cfg), Model(cfg)
    want = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    got = [(k, tuple(v.shape)) for k, v in mine.state_dict().items()]
    assert got == want                                            # names, order and shapes
    params = sum(p.numel() for p in mine.parameters())
    assert params == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist()
    assert mine.save == ref.save
    assert torch.equal(mine.model[-1].anchors, ref.model[-1].anchors)
    assert [m.type for m in mine.model] == [m.type for m in ref.model]
    assert [m.np for m in mine.model] == [m.np for m in ref.model]
    mine.load_state_dict(ref.state_dict())                       # reference-format state_dicts load
    rec = json.load(open(os.path.join(GOLDEN, 'hub_graphs.json')))[name]   # the reference's own Model on the yaml: the second witness
    assert mine.stride.tolist() == rec['strides'] and len(mine.model) == rec['layers']
    if (width, depth) == (1.0, 1.0):
        assert params == rec['params'] and len(got) == rec['entries']
    else:                                                         # the reduced graphs keep a repeat above 1 where the yaml has one
        reps = [len(m) for m in mine.model if isinstance(m, MB.Repeat)] + [len(m.m) for m in mine.model if isinstance(m, (MB.BottleneckCSP, MB.C3))]
        assert name == 'yolov3-tiny' or max(reps) >= 3, reps
    if name.startswith('yolov3') and name != 'yolov3-tiny' and depth == 0.33:
        assert [len(m) for m in mine.model if isinstance(m, MB.Repeat)] == [3, 3]      # the 8-repeat stages: model.6.0 .. model.6.2
        assert 'model.6.2.cv2.bn.running_var' in dict(got)


def test_hub_cfgs_are_the_hub_yamls():
    from somi_amd.configs import COCO_ANCHORS, YOLOV3_TINY_ANCHORS, yolov3_cfg, yolov5_hub_cfg
    mods = lambda rows: [row[2] for row in rows]                  # noqa: E731
    dark = ['Conv', 'Conv', 'Bottleneck', 'Conv', 'Bottleneck', 'Conv', 'Bottleneck', 'Conv', 'Bottleneck', 'Conv', 'Bottleneck']
    for variant, second in (('', ['Conv', [512, [1, 1]]]), ('spp', ['SPP', [512, [5, 9, 13]]])):
        cfg = yolov3_cfg(variant)
        assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 1.0, 1.0, COCO_ANCHORS)
        assert mods(cfg['backbone']) == dark and [row[1] for row in cfg['backbone']] == [1, 1, 1, 1, 2, 1, 8, 1, 8, 1, 4]
        assert cfg['head'][1][2:] == second and cfg['head'][5][0] == -2 and cfg['head'][-2] == [-1, 2, 'Bottleneck', [256, False]]
        assert cfg['head'][-1] == [[27, 22, 15], 1, 'Detect', ['nc', 'anchors']]
    cfg = yolov3_cfg('tiny')
    assert cfg['anchors'] == YOLOV3_TINY_ANCHORS == [[10, 14, 23, 27, 37, 58], [81, 82, 135, 169, 344, 319]]
    assert mods(cfg['backbone']) == ['Conv', 'nn.MaxPool2d'] * 5 + ['Conv', 'nn.ZeroPad2d', 'nn.MaxPool2d']
    assert cfg['backbone'][11][3] == [[0, 1, 0, 1]] and cfg['backbone'][12][3] == [2, 1, 0] and cfg['backbone'][1][3] == [2, 2, 0]
    assert cfg['head'][-1] == [[19, 15], 1, 'Detect', ['nc', 'anchors']]
    cfg = yolov5_hub_cfg('fpn')
    assert mods(cfg['backbone']) == ['Focus', 'Conv', 'Bottleneck', 'Conv', 'BottleneckCSP', 'Conv', 'BottleneckCSP', 'Conv', 'SPP', 'BottleneckCSP']
    assert cfg['backbone'][2][1] == 3 and cfg['backbone'][9] == [-1, 6, 'BottleneckCSP', [1024]] and cfg['anchors'] == COCO_ANCHORS
    assert cfg['head'][-1] == [[18, 14, 10], 1, 'Detect', ['nc', 'anchors']]
    cfg = yolov5_hub_cfg('panet')
    assert mods(cfg['backbone']) == ['Focus', 'Conv', 'BottleneckCSP', 'Conv', 'BottleneckCSP', 'Conv', 'BottleneckCSP', 'Conv', 'SPP', 'BottleneckCSP']
    assert mods(cfg['head']).count('BottleneckCSP') == 4 and cfg['head'][-1] == [[17, 20, 23], 1, 'Detect', ['nc', 'anchors']]
    cfg = yolov5_hub_cfg('p6')
    assert mods(cfg['backbone']) == ['Focus'] + ['Conv', 'C3'] * 4 + ['Conv', 'SPP', 'C3'] and cfg['backbone'][10][3] == [1024, [3, 5, 7]]
    assert cfg['anchors'] == 3 and cfg['head'][-1] == [[23, 26, 29, 32], 1, 'Detect', ['nc', 'anchors']]
    assert [row[0] for row in cfg['head'] if row[2] == 'Concat'] == [[-1, 8], [-1, 6], [-1, 4], [-1, 20], [-1, 16], [-1, 12]]
    cfg = yolov5_hub_cfg('p7')
    assert mods(cfg['backbone']) == ['Focus'] + ['Conv', 'C3'] * 5 + ['Conv', 'SPP', 'C3'] and cfg['backbone'][12][3] == [1280, [3, 5]]
    assert cfg['anchors'] == 3 and cfg['head'][-1] == [[29, 32, 35, 38, 41], 1, 'Detect', ['nc', 'anchors']]
    assert [row[0] for row in cfg['head'] if row[2] == 'Concat'] == [[-1, 10], [-1, 8], [-1, 6], [-1, 4], [-1, 26], [-1, 22], [-1, 18], [-1, 14]]
    assert [row[3][0] for row in cfg['head'] if row[2] == 'C3'] == [1024, 768, 512, 256, 512, 768, 1024, 1280]


def test_hub_blocks_keep_reference_parameter_layout():
    from oracle.somi_ref import blocks as OB
    from somi_amd import blocks as MB
    pairs = [(R.BottleneckCSP(24, 32, 2, True), MB.BottleneckCSP(24, 32, 2, True)), (OB.SPP(32, 32, (3, 5, 7)), MB.SPP(32, 32, (3, 5, 7))),
             (OB.SPP(32, 24, [3, 5]), MB.SPP(32, 24, [3, 5])),
             (nn.Sequential(OB.Bottleneck(16, 16), OB.Bottleneck(16, 16)), MB.Repeat(MB.Bottleneck(16, 16), MB.Bottleneck(16, 16)))]
    for a, b in pairs:
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    names = list(MB.BottleneckCSP(24, 32, 2, True).state_dict())
    assert names[names.index('cv2.weight'):names.index('cv2.weight') + 2] == ['cv2.weight', 'cv3.weight'] and 'bn.running_mean' in names
    assert 'm.1.cv2.conv.weight' in names and isinstance(MB.Repeat(MB.Bottleneck(8, 8)), nn.Sequential)
    assert not list(MB.MaxPool2d(2, 2, 0).state_dict()) and not list(MB.ZeroPad2d([0, 1, 0, 1]).state_dict())


def test_optimizer_groups_take_the_plain_convs_and_the_shared_batchnorm():
    """train.py:125-133 on a BottleneckCSP: `bn` is an nn.BatchNorm2d (group 0), cv2 / cv3 weights are 'every other .weight' (group 1), no biases."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    blk = MB.BottleneckCSP(16, 16, 1)
    g0, g1, g2 = reference_param_groups(blk)
    ids = lambda ps: {id(p) for p in ps}                          # noqa: E731
    assert id(blk.bn.weight) in ids(g0) and {id(blk.cv2.weight), id(blk.cv3.weight)} <= ids(g1) and id(blk.bn.bias) in ids(g2)
    assert len(g0) + len(g1) + len(g2) == len(list(blk.parameters()))


def test_hub_limits_are_explicit():
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov3_cfg, yolov5_hub_cfg
    from somi_amd.model import Model
    for k in ((4, 6), (3, 15), (3, 5, 7, 9), (5, 3), ()):          # even, beyond 13, four windows, descending, none
        with pytest.raises(NotImplementedError, match='1 to 3 ascending odd window sizes, each 3 <= k <= 13'):
            MB.SPP(32, 32, k)
    MB.SPP(32, 32, (7,)), MB.SPP(32, 32, (13,)), MB.SPP(32, 32)
    with pytest.raises(NotImplementedError, match='kernel 2, stride 1 or 2, padding 0'):
        MB.MaxPool2d(3, 2, 1)
    with pytest.raises(NotImplementedError, match='four pads of 0 or 1'):
        MB.ZeroPad2d([0, 2, 0, 2])
    cfg = yolov3_cfg('tiny', 0.25)                                # a ZeroPad2d that no MaxPool2d follows
    cfg['backbone'][12] = [-1, 1, 'Conv', [512, 3, 1]]
    with pytest.raises(NotImplementedError, match='runs only directly in front of an nn.MaxPool2d'):
        Model(cfg)
    cfg = yolov3_cfg('tiny', 0.25)                                # ... or whose output something else reads as well
    cfg['head'][5][0] = [-1, 11]
    with pytest.raises(NotImplementedError, match='its only reader'):
        Model(cfg)
    cfg = yolov5_hub_cfg('p7', 0.25, 0.33)                        # a sixth level
    cfg['head'][-1][0] = [29, 32, 35, 38, 41, 41]
    with pytest.raises(NotImplementedError, match='at most 5 detection levels'):
        Model(cfg)
    m = Model(yolov5_hub_cfg('p7', 0.25, 0.33))
    m.hyp = {}
    m.model[-1].nl = 6
    from somi_amd.loss import ComputeLoss
    with pytest.raises(NotImplementedError, match='at most 5 detection levels'):
        ComputeLoss(m)
    cfg = yolov5_hub_cfg('p6', 0.25, 0.33)
    cfg['head'][2] = [[-1, 8], 6, 'Concat', [1]]
    with pytest.raises(NotImplementedError, match='repeats of'):
        Model(cfg)


def test_five_level_loss_uses_the_five_entry_balance_and_two_levels_too():
    from somi_amd.loss import ComputeLoss
    from somi_amd.model import Model
    for name, want in (('yolov5-p7', 5), ('yolov3-tiny', 2), ('yolov5-panet', 3)):
        m = Model(R.hub_cfg(name, width=0.25, depth=0.33))
        m.hyp = {}
        cl = ComputeLoss(m)
        assert cl.nl == want and cl.balance == ([4.0, 1.0, 0.4] if want == 3 else [4.0, 1.0, 0.25, 0.06, 0.02])
