"""CPU checks of the CBAM C3 family (C3_CBAM, C3_CBAMS, C3_SCBAM: models/common.py:1640-1705; SCBAMBottleneck, :975-995; C3CBAM, :494-504): the
test restatement (tests/cbam_c3_ref.py) reproduces the reference's own classes through the tests/golden/block_c3_cbam*.npz, block_c3_scbam.npz,
block_c3cbam.npz and block_scbam_bneck_nosc.npz fixtures, and a plausible wrong restatement does not; parameter counts, state-dict keys and
shapes are the reference's; the parser gives the oracle Model's layer table for every variant of configs.yolov5_cbam_cfg; the seeded cases of
the GPU tests are the ones the seed rule gives; limits raise by name before any launch; the new entry points are declared, bound, exported and
refuse bad arguments without a launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cbam_c3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_gate_combine_nhwc_f32', 'somi_gate_combine_bwd_pixel_f32', 'somi_gate_combine_bwd_workspace_floats',
               'somi_gate_combine_bwd_chan_f32', 'somi_gate_combine_pixel_trips')
FIXTURES = {'block_c3_cbam': 'c3_cbam', 'block_c3_cbams': 'c3_cbams', 'block_c3_scbam': 'c3_scbam', 'block_c3cbam': 'c3cbam',
            'block_scbam_bneck_nosc': 'scbam_bneck_nosc', 'block_c3_cbam_dwc': 'c3_cbam_dwc', 'block_c3_cbams_dwc': 'c3_cbams_dwc',
            'block_cbam_dwc_bneck_nosc': 'cbam_dwc_bneck_nosc', 'block_c3_cbams_dwc_wide': 'c3_cbams_dwc_wide'}
ROW_OF = {'cbam': 'C3_CBAM', 'cbams': 'C3_CBAMS', 'cbam_dwc': 'C3_CBAM_DWC', 'cbams_dwc': 'C3_CBAMS_DWC', 'scbam': 'C3_SCBAM', 'row': 'C3CBAM'}
NEW_DWC_SYMBOLS = ('somi_dwc_gate_workspace_floats', 'somi_dwc_gate_trips', 'somi_dwc_gate_eval_f32', 'somi_dwc_gate_train_f32',
                   'somi_dwc_gate_bwd_f32')


def _make(tag):
    return R.BLOCKS.get(tag) or R.FIXTURE_ONLY[tag]


def _fixture_errors(name, make):
    """-> {mode: max error / max value} of make(R) under fill_state weights against the fixture."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == R.block_shape(FIXTURES[name])
    assert bool((x * 2 == (x * 2).round()).all()), 'the fixture input lies on a grid of 1/2'
    out = {}
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        assert y.shape == want.shape
        out[mode] = (y - want).abs().max().item() / want.abs().max().item()
    return out


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_restatement_reproduces_the_reference(name):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    for mode, err in _fixture_errors(name, _make(FIXTURES[name])).items():
        assert err <= 1e-5, f'{name} {mode}: {err:.3e}'


def test_wrong_restatement_is_ruled_out():
    """SCBAM with ys = sa(yc) * yc instead of sa(yc) * x2 misses both SCBAM fixtures by more than 1e-3 in both modes."""
    errs = _fixture_errors('block_scbam_bneck_nosc', lambda ns: ns.ProductSCBAMBottleneck(64, 64, False, 1, 1.0))
    assert min(errs.values()) > 1e-3, f'the product restatement fits the bottleneck fixture: {errs}'

    class WrongC3(R.C3_SCBAM):
        def __init__(self, *a):
            super().__init__(*a)
            self.m = torch.nn.Sequential(*(R.ProductSCBAMBottleneck(32, 32, True, 1, e=1.0) for _ in self.m))
    errs = _fixture_errors('block_c3_scbam', lambda ns: WrongC3(64, 64, 2))
    assert min(errs.values()) > 1e-3, f'the product restatement fits the C3 fixture: {errs}'


def test_wrong_dwc_gates_are_ruled_out_and_the_signature_order_holds():
    """(b) The depthwise-separable gate without its final ReLU, or with BN1 after the ReLU, misses the bottleneck fixture by more than 1e-3 in
    both modes.  CBAMBottleneckDWC takes e BEFORE k: built positionally as if k came first it fails to construct, as the reference's does."""
    from somi_amd import blocks as MB
    for gate in (R.NoFinalReluDWC, R.ReluBeforeBn1DWC):
        errs = _fixture_errors('block_cbam_dwc_bneck_nosc', lambda ns, gate=gate: ns.wrong_dwc_bottleneck(gate))
        assert min(errs.values()) > 1e-3, f'{gate.__name__} fits the fixture: {errs}'
    for ns in (R, MB):
        with pytest.raises(TypeError):
            ns.CBAMBottleneckDWC(64, 64, True, 1, ((1, 1), (3, 3)), 1.0)
    d = np.load(os.path.join(GOLDEN, 'block_c3_cbams_dwc_wide.npz'))
    assert d['x'].shape[2] != d['x'].shape[3] and min(d['x'].shape[2:]) > 7


def test_parameter_counts_and_layout_are_the_reference_s():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    count = lambda m: sum(p.numel() for p in m.parameters())      # noqa: E731
    want = {'c3_cbam': 29966, 'c3_cbams': 29806, 'c3_cbam_dwc': 29726, 'c3_cbams_dwc': 29566, 'c3_scbam': 29706, 'c3cbam': 679}
    for tag, n in want.items():
        assert count(R.BLOCKS[tag](R)) == count(R.BLOCKS[tag](MB)) == n, tag
    makes = list(R.BLOCKS.values()) + [lambda M: M.C3_CBAM(32, 64, 3, False), lambda M: M.C3_CBAMS(128, 128, 1), lambda M: M.C3CBAM(512, 512),
                                       lambda M: M.SCBAMBottleneck(32, 32, True, 1, 0.5), lambda M: M.C3_SCBAM(64, 128, 2, True, 1, 0.25)]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # a checkpoint of the restatement loads ...
        a.load_state_dict(b.state_dict())                         # ... and ours loads there
    sd = MB.C3_SCBAM(64, 64, 2).state_dict()
    assert tuple(sd['m.0.spatial_attention.cv1.weight'].shape) == (1, 2, 7, 7) and tuple(sd['m.1.channel_attention.shared_MLP.2.bias'].shape) == (32,)
    assert tuple(sd['m.0.channel_attention.shared_MLP.0.weight'].shape) == (2, 32)            # ratio 16
    assert tuple(MB.C3_CBAM(64, 64).state_dict()['m.0.channel_attention.shared_MLP.0.weight'].shape) == (4, 32)     # ratio 8
    assert tuple(MB.C3_CBAMS(64, 64).state_dict()['m.0.spatial_attention.cv1.weight'].shape) == (1, 2, 3, 3)
    assert list(MB.C3CBAM(64, 128).state_dict()) == ['channel_attention.shared_MLP.0.weight', 'channel_attention.shared_MLP.0.bias',
                                                     'channel_attention.shared_MLP.2.weight', 'channel_attention.shared_MLP.2.bias',
                                                     'spatial_attention.cv1.weight', 'spatial_attention.cv1.bias']
    sd = MB.C3_CBAM_DWC(64, 64, 2).state_dict()
    assert tuple(sd['m.0.spatial_attention.cv1.depth_conv.weight'].shape) == (2, 1, 7, 7) and tuple(sd['m.1.spatial_attention.cv1.bn1.running_var'].shape) == (1,)
    assert tuple(sd['m.0.spatial_attention.cv1.point_conv.weight'].shape) == (1, 2, 1, 1) and 'm.0.spatial_attention.cv1.bn.num_batches_tracked' in sd
    assert tuple(MB.C3_CBAMS_DWC(64, 64).state_dict()['m.0.spatial_attention.cv1.depth_conv.weight'].shape) == (2, 1, 3, 3)
    blk = MB.C3_SCBAM(128, 128, 2)
    assert len(blk.m) == 2 and all(type(m) is MB.SCBAMBottleneck and m.add and m.cv2.conv.kernel_size == (3, 3) for m in blk.m)
    assert blk.m[0].cv1.conv.out_channels == 64 and blk.m[0].cv1.conv.kernel_size == (1, 1)       # e = 1.0 inside
    blk = MB.C3_CBAM(128, 128, 2)
    assert all(type(m) is MB.CBAMBottleneck and m.cv1.conv.kernel_size == (1, 1) and m.cv2.conv.kernel_size == (3, 3) for m in blk.m)
    assert blk.m[0].spatial_attention.cv1.kernel_size == (7, 7) and MB.C3_CBAMS(64, 64).m[0].spatial_attention.cv1.kernel_size == (3, 3)
    assert MB.C3_CBAM(64, 64, 1, True, 1, 0.5, 5).m[0].spatial_attention.cv1.kernel_size == (5, 5)


def test_contract_and_limits_are_explicit():
    from somi_amd import blocks as MB
    new = (MB.SCBAMBottleneck, MB.C3_CBAM, MB.C3_CBAMS, MB.C3_SCBAM, MB.C3CBAM, MB.CBAMBottleneckDWC, MB.C3_CBAM_DWC, MB.C3_CBAMS_DWC)
    for cls in (MB.DepthWiseConv, MB.SpatialAttentionModuleDWC):
        assert (cls.__dict__['accumulates'], cls.__dict__['folds_pooled'], cls.__dict__['reduction']) == (False, False, 1), cls.__name__
    for cls in new:                                               # declared on the class itself, not inherited
        assert (cls.__dict__['accumulates'], cls.__dict__['folds_pooled'], cls.__dict__['reduction']) == (False, False, 1), cls.__name__
        assert list(inspect.signature(cls.backward).parameters)[:5] == ['self', 'dout', 'dx_out', 'accumulate', 'need_dx'], cls.__name__
    assert issubclass(MB.C3_SCBAM, MB.C3) and MB.C3.accumulates is True
    assert list(inspect.signature(MB.CBAMBottleneck.backward).parameters)[:5] == ['self', 'dout', 'dx_out', 'accumulate', 'need_dx']
    act = lambda c, cs=None: MB.Act(torch.zeros(1, 4, 4, cs or c), 0, c)     # noqa: E731   (a CPU tensor: nothing can launch)
    # hidden width not a multiple of 4
    with pytest.raises(NotImplementedError, match=r'C3_CBAM\(20, 20\): hidden width 10 is not a multiple of 4'):
        MB.C3_CBAM(20, 20).eval()(act(20))
    with pytest.raises(NotImplementedError, match=r'C3_SCBAM\(36, 36\): hidden width 18 is not a multiple of 4'):
        MB.C3_SCBAM(36, 36).eval()(act(36))
    # no hidden neuron: C3_CBAM* below 8 hidden channels, the ratio-16 blocks below 16
    with pytest.raises(NotImplementedError, match=r'C3_CBAMS\(8, 8\): 4 channels at ratio 8 leave'):
        MB.C3_CBAMS(8, 8).eval()(act(8))
    with pytest.raises(NotImplementedError, match=r'C3_SCBAM\(16, 16\): 8 channels at ratio 16 leave'):
        MB.C3_SCBAM(16, 16).eval()(act(16))
    with pytest.raises(NotImplementedError, match=r'SCBAMBottleneck\(12, 12\): 12 channels at ratio 16 leave'):
        MB.SCBAMBottleneck(12, 12).eval()(act(12))
    with pytest.raises(NotImplementedError, match=r'C3CBAM\(8\): 8 channels at ratio 16 leave'):
        MB.C3CBAM(8, 8).eval()(act(8))
    with pytest.raises(NotImplementedError, match=r'C3CBAM\(2048\): the channel attention\'s MLP runs on at most 1024 channels'):
        MB.C3CBAM(2048, 2048).eval()(MB.Act(torch.zeros(1, 1, 1, 2048)))
    # the spatial gate's kernel
    with pytest.raises(NotImplementedError, match=r'C3_CBAM\(64, 64\): kernel_size 9 of the spatial gate is not built, only 3, 5 and 7'):
        MB.C3_CBAM(64, 64, 1, True, 1, 0.5, 9)
    with pytest.raises(NotImplementedError, match=r'SCBAMBottleneck\(64, 64\): kernel_size 4'):
        MB.SCBAMBottleneck(64, 64, kernel_size=4)
    # C3_CBAM's bottleneck scales a whole tensor in training: 80 hidden channels are stored as a slice of 96
    with pytest.raises(NotImplementedError, match=r'C3_CBAM\(160, 160\): the CBAM training path works on whole tensors, and 80 channels'):
        MB.C3_CBAM(160, 160).train()(act(160))
    # the tail-attention blocks hand exact-width tensors on: a width stored padded is refused by name too, in both modes
    with pytest.raises(NotImplementedError, match=r'C3_SCBAM\(160, 160\): the gated tensors are exactly 80 channels wide'):
        MB.C3_SCBAM(160, 160).eval()(act(160))
    with pytest.raises(NotImplementedError, match=r'SCBAMBottleneck\(80, 80\): the gated tensors are exactly 80 channels wide'):
        MB.SCBAMBottleneck(80, 80).train()(act(80, 96))
    with pytest.raises(NotImplementedError, match=r'C3CBAM\(80\): the gated tensors are exactly 80 channels wide'):
        MB.C3CBAM(80, 80).eval()(act(80, 96))
    # the depthwise-separable blocks: ratio 16, k in {3, 7}, not under sync-BN, and a training forward of the gate needs B H W > 1
    with pytest.raises(NotImplementedError, match=r'C3_CBAM_DWC\(16, 16\): 8 channels at ratio 16 leave'):
        MB.C3_CBAM_DWC(16, 16).eval()(act(16))
    with pytest.raises(NotImplementedError, match=r'CBAMBottleneckDWC\(20, 20\): hidden width 20|CBAMBottleneckDWC\(18, 18\): hidden width 18 is not a multiple of 4'):
        MB.CBAMBottleneckDWC(18, 18).eval()(act(18, 20))
    with pytest.raises(NotImplementedError, match=r'C3_CBAMS_DWC\(64, 64\): kernel_size 5 of the depthwise-separable gate is not built, only 3 and 7'):
        MB.C3_CBAMS_DWC(64, 64, 1, True, 1, 0.5, 5)
    with pytest.raises(NotImplementedError, match='SpatialAttentionModuleDWC: kernel_size 5 is not built'):
        MB.SpatialAttentionModuleDWC(5)
    from somi_amd import ops
    ops.SYNC_BN = 'all-gather'
    try:
        with pytest.raises(NotImplementedError, match=r'C3_CBAM_DWC\(64, 64\): the gate\'s two BatchNorms take local batch statistics; not under ops.SYNC_BN'):
            MB.C3_CBAM_DWC(64, 64).train()(act(64))
        with pytest.raises(NotImplementedError, match=r'CBAMBottleneckDWC\(64, 64\): the gate'):
            MB.CBAMBottleneckDWC(64, 64).train()(act(64))
    finally:
        ops.SYNC_BN = None
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        ops.dwc_gate_train(torch.zeros(1, 1, 1, 2), torch.zeros(29), torch.zeros(6), 3, 1e-3, 0.03)
    with pytest.raises(RuntimeError, match='got a map of 8'):
        MB.C3CBAM(16, 16).eval()(act(8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.C3CBAM(16, 16).eval()(act(16))
    with pytest.raises(NotImplementedError, match='adds its input gradient into dx_out, or returns it'):
        MB.CBAMBottleneck(8, 8).backward(None, dx_out=None, accumulate=True)
    with pytest.raises(NotImplementedError, match='adds its input gradient into dx_out, or returns it'):
        MB.CBAMBottleneck(8, 8).backward(None, need_dx=False)


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_cbam_graph_matches_the_oracle(variant, monkeypatch):
    """The same layer table (types, from, parameter counts, n inside), state dict and strides as the oracle Model."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cbam_cfg, yolov5_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov5_cbam_cfg(0.25, 0.33, nc=10, variant=variant)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert [m.np for m in mine.model] == [m.np for m in ref.model]
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [(m.i, m.f, m.type) for m in mine.model] == [(m.i, m.f, m.type) for m in ref.model]
    mine.load_state_dict(ref.state_dict())
    assert mine.fuse() is mine
    base = yolov5_cfg(0.25, 0.33, nc=10)
    name = ROW_OF[variant]
    if variant == 'row':
        assert cfg['backbone'][:10] == base['backbone'] and cfg['backbone'][10] == [-1, 1, 'C3CBAM', [1024]]
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 15], [-1, 11], [18, 21, 24]]
        assert type(mine.model[10]) is MB.C3CBAM and mine.model[10].channel_attention.shared_MLP[0].in_features == 256
    else:
        assert cfg['head'] == base['head'] and [r[2] for r in cfg['backbone']].count(name) == 4
        assert [r[:2] + r[3:] for r in cfg['backbone']] == [r[:2] + r[3:] for r in base['backbone']]
        assert [type(mine.model[i]) for i in (2, 4, 6, 8)] == [getattr(MB, name)] * 4 and [len(mine.model[i].m) for i in (2, 4, 6, 8)] == [1, 2, 3, 1]
        assert [len(ref.model[i].m) for i in (2, 4, 6, 8)] == [1, 2, 3, 1]
        gate = 'cv1.bn1.running_var' if variant.endswith('dwc') else 'cv1.bias'
        assert f'model.6.m.2.spatial_attention.{gate}' in got and 'model.4.m.1.channel_attention.shared_MLP.2.bias' in got


def test_parser_tables_and_refusals():
    from somi_amd import configs as C
    from somi_amd.model import Model, _CH, _REPEAT_INSIDE
    for name in ('C3_CBAM', 'C3_CBAMS', 'C3_CBAM_DWC', 'C3_CBAMS_DWC', 'C3_SCBAM'):
        assert name in _CH and name in _REPEAT_INSIDE
    assert 'C3CBAM' in _CH and 'C3CBAM' not in _REPEAT_INSIDE
    cfg = C.yolov5_cbam_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, C.COCO_ANCHORS)
    assert [r[2] for r in cfg['backbone']] == ['Conv', 'Conv', 'C3_CBAM', 'Conv', 'C3_CBAM', 'Conv', 'C3_CBAM', 'Conv', 'C3_CBAM', 'SPPF']
    with pytest.raises(ValueError, match="variant must be one of"):
        C.yolov5_cbam_cfg(variant='neck')
    cfg = C.yolov5_cbam_cfg(0.25, 0.33, nc=10, variant='row')
    cfg['backbone'][10][3] = [512]                                # names another width than its input's 256
    with pytest.raises(ValueError, match=r"a 'C3CBAM' row that names 128 channels \(scaled\) behind 256"):
        Model(cfg)
    cfg = C.yolov5_cbam_cfg(0.25, 0.33, nc=10, variant='row')
    cfg['backbone'][10][1] = 6                                    # 6 x depth 0.33 = 2 repeats: the reference's nn.Sequential of whole modules
    with pytest.raises(NotImplementedError, match="2 repeats of 'C3CBAM' as an nn.Sequential are not on the path"):
        Model(cfg)
    for outside in ('C3TR', 'BAM'):
        cfg = C.yolov5_cbam_cfg(0.25, 0.33, nc=10)
        cfg['backbone'][8][2] = outside
        with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
            Model(cfg)
    names = set(ROW_OF.values())
    others = [C.yolov5_cfg(), C.yolov5_cfg(version='5.0'), C.yolov5_cpca_cfg(), C.yolov5_cpca_cfg(where='row'), C.yolov5_ghost_cfg(),
              C.yolov10_cfg(0.25, 0.33), C.somi_cfg(0.25, 0.33), C.yolov3_cfg('', 0.25, 0.33), C.yolov5_hub_cfg('p6', 0.25, 0.33)]
    for cfg in others:
        assert not names & {r[2] for r in cfg['backbone'] + cfg['head']}


def test_optimizer_groups_follow_the_reference():
    """train.py:125-133: every .bias in the bias group, BatchNorm weights without decay, every other .weight (conv, Linear) decayed."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    for mk in R.BLOCKS.values():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert sorted(g0 + g1 + g2) == sorted(names.values()), 'a parameter is in no group'
        assert all(n.endswith('.bias') for n in g2) and not any(n.endswith('.bias') for n in g0 + g1)
        dwc = any('depth_conv' in n for n in names.values())
        for leaf in ('shared_MLP.0.weight', 'shared_MLP.2.weight') + (('depth_conv.weight', 'point_conv.weight') if dwc else ('spatial_attention.cv1.weight',)):
            assert any(n.endswith(leaf) for n in g1) and not any(n.endswith(leaf) for n in g0 + g2)
        assert all(n.endswith(('bn.weight', 'bn1.weight')) for n in g0)
        if dwc:                                                   # the gate's two BatchNorm weights are not decayed
            assert any(n.endswith('cv1.bn.weight') for n in g0) and any(n.endswith('cv1.bn1.weight') for n in g0)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]


def test_block_seeds_are_the_ones_the_rule_gives():
    """cbam_c3_ref.BLOCK_SEEDS: per block the first of the seeds 0..7 that passes the seed rule - computed from the restatement alone."""
    for tag in R.BLOCKS:
        figs = []
        for seed in range(8):
            figs.append(R.block_figures(tag, seed))
            print(f'{tag} seed {seed}: pooled gap {figs[-1][0]:.3e}, channel gap {figs[-1][1]:.3e}, pre-ReLU {figs[-1][2]:.3e}, fp32 against fp64 {figs[-1][3]:.3f} x the bar')
            if R.passes(figs[-1]):
                break
        assert R.BLOCK_SEEDS[tag] == R.choose(figs), f'{tag}: the rule gives seed {R.choose(figs)}'


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_graph_seeds_are_the_ones_the_rule_gives(variant, monkeypatch):
    """cbam_c3_ref.GRAPH_SEEDS: the first candidate of cbam_c3_ref.graph_candidates() - (fill 1..4) x (batch 0..3), then further fills in the
    same order - that passes the rule; every candidate before it misses a margin."""
    R.register(monkeypatch)
    cands = R.graph_candidates()
    assert cands[:16] == [(fill, batch) for fill in range(1, 5) for batch in range(4)]
    figs = []
    for cand in cands:
        figs.append(R.graph_figures(variant, cand))
        print(f'{variant} {cand}: pooled gap {figs[-1][0]:.3e}, channel gap {figs[-1][1]:.3e}, pre-ReLU {figs[-1][2]:.3e}, fp32 oracle against fp64 at {figs[-1][3]:.3f} x the bar')
        if R.passes(figs[-1]):
            break
    assert R.passes(figs[-1]), f'{variant}: no candidate passes'
    assert R.GRAPH_SEEDS[variant] == cands[R.choose(figs)], f'{variant}: the rule gives {cands[R.choose(figs)]}'
    assert min(figs[-1][:3]) >= R.MIN_GAP and figs[-1][3] < 0.5


def test_walk_shape_makes_the_per_pixel_pass_walk():
    """somi_gate_combine_pixel_trips is the per-pixel pass's plan as host arithmetic (grid cap, waves, lanes per pixel): the GPU tests' WALK_SHAPE
    makes the busiest wave take a second trip of its grid-stride loop, every other shape one; sizes the pass refuses give 0."""
    from somi_amd import _lib
    from test_cbam_c3_gpu import SHAPES, WALK_SHAPE
    trips = _lib.lib().somi_gate_combine_pixel_trips
    B, H, W, C = WALK_SHAPE
    assert trips(B, H * W, C) == 2
    assert all(trips(b, h * w, c) == 1 for b, h, w, c in SHAPES)
    assert trips(32, 160 * 160, 32) == 13 and trips(32, 40 * 40, 128) == 4     # the shapes training runs at: 8 and 2 pixels a wave and trip
    assert trips(1, 4, 6) == 0 and trips(0, 4, 8) == 0 and trips(70000, 4, 8) == 0


def test_new_symbols_are_declared_bound_and_exported():
    from somi_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS + NEW_DWC_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/somi_hip.h'
        assert name in _lib.SIGNATURES, f'{name} is not bound in _lib.SIGNATURES'
        assert hasattr(L, name), f'{name} is not exported'
        proto = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert not re.search(r'_coff\b', proto), f'{name} takes a slice as loose *_coff parameters'
    assert '#define SOMI_ABI_VERSION 15' in hdr and _lib.lib().somi_abi_version() == _lib.ABI_VERSION == 15      # new symbols only
    for fn in ('gate_combine', 'gate_combine_backward_pixel', 'gate_combine_backward_chan', 'spatial_attn_backward'):
        assert callable(getattr(ops, fn))
    assert ops.GATE_MODES == {'product': 0, 'sigmoid_sum': 1} and '#define SOMI_GATE_SIGMOID_SUM 1' in hdr
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'cbam_c3.hip' in mk
    src = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'cbam_c3.hip')).read()
    assert 'SOMI_REQUIRE_SLICES' in src and not re.search(r'\batomicAdd\b', src)


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    """Every slice an entry point reads or writes, broken in six ways, is SOMI_EINVAL with a message that names it; C not a multiple of 4, an
    unknown mode, a missing gate, an arg-max half given alone and bad sizes are refused; a short workspace is SOMI_EWORKSPACE.  A rejected call
    launches nothing, so the made-up addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    S = lambda i: _lib.Slice(0x10000 * (i + 1), 16, 4)            # noqa: E731
    none = _lib.Slice(None, 0, 0)
    CA, SA, P1, P2, P3, WS = 0x900000, 0x910000, 0x920000, 0x930000, 0x940000, 0x950000
    err = lambda: L.somi_last_error()                             # noqa: E731

    def fwd(t=None, res=None, out=None, ca=CA, sa=SA, B=1, HW=24, C=8, mode=0):
        return L.somi_gate_combine_nhwc_f32(t or S(0), ca, sa, res or S(1), out or S(2), B, HW, C, mode, None)

    def pix(dout=None, t=None, ca=CA, sa=SA, t_max=P1, dsa=P2, amaxc=P3, amaxp=WS, B=1, HW=24, C=8, mode=1, logit=0):
        return L.somi_gate_combine_bwd_pixel_f32(dout or S(0), t or S(1), ca, sa, t_max, dsa, amaxc, amaxp, B, HW, C, mode, logit, None)

    def chan(dout=None, t=None, dt=None, ca=CA, sa=SA, dstats=P1, amaxc=P2, dca=P3, ws=WS, floats=1 << 20, B=1, HW=24, C=8, mode=0, acc=0):
        return L.somi_gate_combine_bwd_chan_f32(dout or S(0), t or S(1), ca, sa, dstats, amaxc, dt or S(2), dca, ws, floats, B, HW, C, mode, acc, None)

    for fn, fields in ((fwd, ('t', 'out', 'res')), (pix, ('dout', 't')), (chan, ('dout', 't', 'dt'))):
        for field in fields:
            for what, brk in BREAKS:
                if field == 'res' and what == 'pointer NULL':
                    continue                                      # an absent shortcut is legal
                s = S(3)
                brk(s)
                shown = 'residual' if field == 'res' else field
                assert fn(**{field: s}) == -1, f'{fn.__name__}: {field}: {what} is let through'
                assert f'{shown} = ['.encode() in err(), f'{fn.__name__}: {field}: {what}: {err()}'
        assert fn(C=6) == -1 and b'not a multiple of 4' in err()
        assert fn(C=0) == -1 and b'not a multiple of 4' in err()
        assert fn(mode=2) == -1 and b'neither product (0) nor sigmoid-sum (1)' in err()
        assert fn(B=0) == -1 and b'bad sizes' in err() and fn(HW=-1) == -1 and fn(B=70000) == -1
        assert fn(B=4096, HW=1 << 20) == -1 and b'bad sizes' in err()
        assert fn(B=65535, HW=4, C=1 << 16) == -1 and b'B * C' in err()
        assert fn(ca=None) == -1 and fn(sa=None) == -1 and fn(ca=CA + 4) == -1
    assert fwd(res=none, t=_lib.Slice(0x10000, 16, 6)) == -1 and b't = [' in err()
    assert pix(t_max=None) == -1 and b'come together' in err() and pix(amaxp=None) == -1 and pix(t_max=P1 + 4) == -1
    assert pix(dsa=None) == -1 and pix(amaxc=None) == -1
    assert chan(dstats=None) == -1 and chan(amaxc=None) == -1 and chan(dca=None) == -1 and chan(dstats=P1 + 4) == -1
    assert chan(ws=None) == -1 and chan(ws=WS + 4) == -1 and b'workspace' in err()
    need = L.somi_gate_combine_bwd_workspace_floats(2, 300, 8)
    assert need == 2 * 2 * 8                                      # one row of C partial sums per (image, 256-pixel chunk)
    assert chan(B=2, HW=300, floats=need - 1) == -3, 'a short workspace is let through'
    assert L.somi_gate_combine_bwd_workspace_floats(1, 256, 32) == 32 and L.somi_gate_combine_bwd_workspace_floats(1, 257, 32) == 64
    assert L.somi_gate_combine_bwd_workspace_floats(1, 4, 6) == 0 and L.somi_gate_combine_bwd_workspace_floats(0, 4, 8) == 0


def test_dwc_gate_entry_points_refuse_bad_arguments_without_a_launch():
    """Null pointers, a misaligned map, k = 5, one value per channel in training and a short workspace are refused before any launch; the
    workspace size and the trip count are host arithmetic."""
    from somi_amd import _lib
    L = _lib.lib()
    A = [0x10000 * (i + 1) for i in range(10)]
    need = L.somi_dwc_gate_workspace_floats(2, 5, 7, 7)
    assert need == 2 * (128 * 13 + 1 * 100) + 4 * 70 + 4 and L.somi_dwc_gate_workspace_floats(2, 5, 7, 5) == 0
    assert L.somi_dwc_gate_workspace_floats(2, 130, 67, 3) == 2 * (128 * 13 + 5 * 20) + 4 * 17420 + 4
    assert [L.somi_dwc_gate_trips(*s) for s in ((2, 5, 7), (2, 130, 67), (1, 128, 256), (2, 130, 130), (0, 1, 1))] == [1, 1, 1, 2, 0]

    def ev(stats=A[0], params=A[1], run=A[2], sa=A[3], k=7, B=2):
        return L.somi_dwc_gate_eval_f32(stats, params, run, sa, B, 5, 7, k, 1e-3, None)

    def tr(stats=A[0], params=A[1], u=A[2], p=A[3], st=A[4], sa=A[5], ws=A[6], floats=1 << 20, k=7, B=2, H=5):
        return L.somi_dwc_gate_train_f32(stats, params, u, p, st, None, 0.03, 1e-3, sa, ws, floats, B, H, 7, k, None)

    def bw(dsa=A[0], stats=A[1], u=A[2], p=A[3], st=A[4], params=A[5], dstats=A[6], dparams=A[7], ws=A[8], floats=1 << 20, k=7, B=2):
        return L.somi_dwc_gate_bwd_f32(dsa, stats, u, p, st, params, dstats, dparams, ws, floats, B, 5, 7, k, None)

    for fn, ptrs in ((ev, ('stats', 'params', 'run', 'sa')), (tr, ('stats', 'params', 'u', 'p', 'st', 'sa', 'ws')),
                     (bw, ('dsa', 'stats', 'u', 'p', 'st', 'params', 'dstats', 'dparams', 'ws'))):
        for name in ptrs:
            assert fn(**{name: None}) == -1, f'{fn.__name__}: {name} NULL is let through'
        assert fn(stats=A[0] + 4) == -1 and fn(B=0) == -1
        assert fn(k=5) == -1 and b'kernel_size 5 is not built, only 3 and 7' in L.somi_last_error()
    assert tr(ws=A[6] + 4) == -1 and tr(floats=need - 1) == -3 and bw(floats=need - 1) == -3
    assert L.somi_dwc_gate_train_f32(A[0], A[1], A[2], A[3], A[4], None, 0.03, 1e-3, A[5], A[6], 1 << 20, 1, 1, 1, 7, None) == -1
    assert b'more than one value per channel' in L.somi_last_error()
