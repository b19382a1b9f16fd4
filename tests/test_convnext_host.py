"""CPU checks of the large-kernel depthwise blocks (LayerNorm_s, ConvNextBlock, CNeB: models/common.py:6728-6791; ConvMix, CSPCM: :7149-7180):
the test restatement (tests/convnext_ref.py) reproduces the reference's own classes through the tests/golden/block_cnx*.npz fixtures, and
five plausible wrong restatements do not; state-dict keys, shapes and the parameter order are the restatement's; the parser gives the oracle
Model's layer table for both forms of configs.yolov5_convnext_cfg; every parameter but the gammas is in exactly one optimizer group; the
seeded cases of the GPU tests are the ones the selection rule gives; limits raise by name; the new entry points are declared, bound, exported
and refuse bad arguments without a launch; the launch plan is host arithmetic; and the fp32 CPU reference of the three kernels holds half of
each bar of tests/test_convnext_gpu.py at every case it uses."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnext_ref as R
from support_kernels_ref import POINT, REDUCED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_dwlk_nhwc_f32', 'somi_dwlk_dgrad_nhwc_f32', 'somi_dwlk_wgrad_nhwc_f32', 'somi_dwlk_wgrad_workspace_floats',
               'somi_dwlk_stat_rows', 'somi_dwlk_strips_per_workgroup', 'somi_dwlk_strip_length')


def _fixture_errors(name, make):
    """-> {mode: max error / max value} of make(R) under fill_state weights against the fixture."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == R.block_shape(R.FIXTURES[name])
    assert bool((x * 2 == (x * 2).round()).all()), 'the fixture input lies on a grid of 1/2'
    out = {}
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        assert y.shape == want.shape, f'{name} {mode}: {tuple(y.shape)} vs {tuple(want.shape)}'
        out[mode] = (y - want).abs().max().item() / want.abs().max().item()
    return out


@pytest.mark.parametrize('name', sorted(R.FIXTURES))
def test_restatement_reproduces_the_reference(name):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    for mode, err in _fixture_errors(name, R.BLOCKS[R.FIXTURES[name]]).items():
        assert err <= 1e-5, f'{name} {mode}: {err:.3e}'
    d = np.load(os.path.join(GOLDEN, 'block_cnxcneb_16_48.npz'))
    assert d['x'].shape == (2, 16, 5, 7) and d['out_eval'].shape == (2, 48, 5, 7)     # a map smaller than either kernel


def test_wrong_restatements_are_ruled_out():
    """BatchNorm in front of the GELU in ConvMix, the cv2 branch first in CNeB and in CSPCM, gamma applied to the sum and a LayerNorm with
    eps 1e-5 each miss a fixture by more than 1e-4 (fill_state's gamma is of order 0.1, so the layer scale shows); a ConvMix that honours
    dim1 has another state dict and returns dim1 channels."""
    errs = _fixture_errors('block_cnxconvmix', lambda ns: ns.NormThenActConvMix(16, 16))
    assert min(errs.values()) > 1e-3, f'BatchNorm before GELU fits the fixture: {errs}'
    errs = _fixture_errors('block_cnxconvmix_k7', lambda ns: ns.NormThenActConvMix(12, 12, 7))
    assert min(errs.values()) > 1e-3, f'BatchNorm before GELU fits the k = 7 fixture: {errs}'
    errs = _fixture_errors('block_cnxcneb', lambda ns: ns.SwappedCNeB(32, 32, 2))
    assert min(errs.values()) > 1e-3, f'the swapped concatenation fits the CNeB fixture: {errs}'
    errs = _fixture_errors('block_cnxcspcm', lambda ns: ns.SwappedCSPCM(32, 32, 1))
    assert min(errs.values()) > 1e-3, f'the swapped concatenation fits the CSPCM fixture: {errs}'
    errs = _fixture_errors('block_cnxblock', lambda ns: ns.GammaOnSumBlock(16))
    assert min(errs.values()) > 1e-3, f'gamma on the sum fits the fixture: {errs}'
    # eps: on the random fixture the conv's output varies by order 1 over the channels and 1e-5 against 1e-6 moves the output by 2e-6 of its
    # scale; on the zero input the LayerNorm sees the conv's bias alone (variance of order 1e-2) and the output is the branch alone
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, R.FLAT_FIXTURE + '.npz'))
    x, want = torch.from_numpy(d['x']), torch.from_numpy(d['out_eval'])
    assert not x.any() and tuple(x.shape) == R.block_shape('cnxblock')
    errs = {}
    for cls in (R.ConvNextBlock, R.TorchEpsBlock):
        with torch.no_grad():
            errs[cls.__name__] = ((fill_state(cls(16), 0).eval()(x) - want).abs().max() / want.abs().max()).item()
    assert errs['ConvNextBlock'] <= 1e-5 and errs['TorchEpsBlock'] > 1e-4, f'LayerNorm with eps 1e-5 fits the zero-input fixture: {errs}'
    a, b = R.ConvMix(16, 24), R.Dim1ConvMix(16, 24)
    assert tuple(a.state_dict()['Conv_1x1.0.weight'].shape) == (16, 16, 1, 1) and tuple(b.state_dict()['Conv_1x1.0.weight'].shape) == (24, 16, 1, 1)
    assert a(torch.zeros(1, 16, 3, 3)).shape[1] == 16 and b(torch.zeros(1, 16, 3, 3)).shape[1] == 24
    with pytest.raises(RuntimeError):
        b.load_state_dict(a.state_dict())


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    makes = list(R.BLOCKS.values()) + [lambda M: M.CNeB(64, 128, 3), lambda M: M.CSPCM(64, 32, 2), lambda M: M.ConvMix(32, 64, 7),
                                       lambda M: M.ConvNextBlock(24, 0., 0.), lambda M: M.ConvNextBlock(8, 0., 0.5), lambda M: M.LayerNorm_s(12)]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # a checkpoint of the restatement loads ...
        a.load_state_dict(b.state_dict())                         # ... and ours loads there
    blk = MB.ConvNextBlock(16)
    assert [n for n, _ in blk.named_parameters()] == ['gamma', 'dwconv.weight', 'dwconv.bias', 'norm.weight', 'norm.bias', 'pwconv1.weight',
                                                     'pwconv1.bias', 'pwconv2.weight', 'pwconv2.bias']
    assert [n for n, _ in blk.named_children()] == ['dwconv', 'norm', 'pwconv1', 'act', 'pwconv2', 'drop_path']
    assert tuple(blk.dwconv.weight.shape) == (16, 1, 7, 7) and blk.dwconv.padding == (3, 3) and blk.dwconv.groups == 16
    assert tuple(blk.pwconv1.weight.shape) == (64, 16) and tuple(blk.pwconv2.weight.shape) == (16, 64)
    assert blk.norm.eps == 1e-6 and blk.norm.normalized_shape == (16,) and blk.norm.data_format == 'channels_last'
    assert torch.equal(blk.gamma.detach(), torch.full((16,), 1e-6)) and isinstance(blk.drop_path, torch.nn.Identity)
    assert MB.ConvNextBlock(16, 0., 0.).gamma is None and MB.ConvNextBlock(16, layer_scale_init_value=-1.).gamma is None
    assert list(inspect.signature(MB.ConvNextBlock.__init__).parameters) == ['self', 'dim', 'drop_path', 'layer_scale_init_value']
    assert list(inspect.signature(MB.LayerNorm_s.__init__).parameters) == ['self', 'normalized_shape', 'eps', 'data_format']
    assert list(inspect.signature(MB.CNeB.__init__).parameters) == ['self', 'c1', 'c2', 'n', 'shortcut', 'g', 'e']
    assert list(inspect.signature(MB.ConvMix.__init__).parameters) == ['self', 'dim', 'dim1', 'kernel_size']
    assert list(inspect.signature(MB.CSPCM.__init__).parameters) == ['self', 'c1', 'c2', 'n', 'e']
    cneb = MB.CNeB(32, 64, 3)
    assert [n for n, _ in cneb.named_children()] == ['cv1', 'cv2', 'cv3', 'm'] and len(cneb.m) == 3 and all(type(b) is MB.ConvNextBlock for b in cneb.m)
    assert cneb.m[0].dwconv.in_channels == 32 and cneb.cv3.conv.in_channels == 64
    mix = MB.ConvMix(16, 40)
    assert [n for n, _ in mix.named_parameters()] == ['Resnet.0.weight', 'Resnet.0.bias', 'Resnet.2.weight', 'Resnet.2.bias', 'Conv_1x1.0.weight',
                                                     'Conv_1x1.0.bias', 'Conv_1x1.2.weight', 'Conv_1x1.2.bias']
    assert tuple(mix.Resnet[0].weight.shape) == (16, 1, 9, 9) and tuple(mix.Conv_1x1[0].weight.shape) == (16, 16, 1, 1)      # dim1 is ignored
    assert isinstance(mix.Resnet[1], torch.nn.GELU) and isinstance(mix.Resnet[2], torch.nn.BatchNorm2d)
    csp = MB.CSPCM(32, 32, 2)
    assert [n for n, _ in csp.named_children()] == ['cv1', 'cv2', 'cv3', 'm'] and [type(b) for b in csp.m] == [MB.ConvMix] * 2
    assert csp.m[0].Resnet[0].kernel_size == (9, 9)


def test_contract_and_limits_are_explicit():
    from somi_amd import blocks as MB
    for cls in (MB.LayerNorm_s, MB.ConvNextBlock, MB.CNeB, MB.ConvMix, MB.CSPCM):
        assert (cls.accumulates, cls.folds_pooled, cls.reduction) == (False, False, 1), cls.__name__
        assert list(inspect.signature(cls.backward).parameters)[1:5] == ['dout', 'dx_out', 'accumulate', 'need_dx'], cls.__name__
    assert not issubclass(MB.CNeB, MB.C3) and MB.C3.accumulates is True
    with pytest.raises(NotImplementedError, match='channels_first'):
        MB.LayerNorm_s(8, data_format='channels_first')
    with pytest.raises(NotImplementedError):
        MB.LayerNorm_s(8, data_format='nchw')
    with pytest.raises(NotImplementedError, match=r'ConvNextBlock\(drop_path=0.1\): stochastic depth is not on the path'):
        MB.ConvNextBlock(8, 0.1)
    for k in (3, 5, 11):
        with pytest.raises(NotImplementedError, match=rf'ConvMix\(kernel_size={k}\): the large-kernel depthwise kernels have k = 7 and k = 9 only'):
            MB.ConvMix(8, 8, k)
    A = MB.Act
    for mode in (True, False):
        for blk, c in ((MB.ConvNextBlock(6), 6), (MB.ConvMix(6, 6), 6)):      # c % 4
            with pytest.raises(NotImplementedError, match=r'takes a whole \(B,H,W,6\) tensor with c % 4 == 0'):
                blk.train(mode)(A(torch.zeros(1, 4, 4, 6)))
        for blk in (MB.ConvNextBlock(8), MB.ConvMix(8, 8, 7)):               # a slice of a wider tensor
            with pytest.raises(NotImplementedError, match=r'takes a whole \(B,H,W,8\) tensor with c % 4 == 0, got channels \[4, 12\) of 16'):
                blk.train(mode)(A(torch.zeros(1, 4, 4, 16), 4, 8))
    with pytest.raises(NotImplementedError, match='CNeB hidden width 6 must be a multiple of 4'):
        MB.CNeB(8, 12, 1).eval()(A(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(NotImplementedError, match='CSPCM hidden width 10 must be a multiple of 4'):
        MB.CSPCM(16, 20, 1).eval()(A(torch.zeros(1, 4, 4, 16)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.ConvMix(8, 8).eval()(A(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.ConvNextBlock(8).eval()(A(torch.zeros(1, 4, 4, 8)))
    # what stays as it was: the large-kernel CIB, a grouped Conv with k = 7
    with pytest.raises(NotImplementedError):
        MB.CIB(16, 16, lk=True)
    with pytest.raises(NotImplementedError):
        MB.Conv(16, 16, 7, 1, None, 16)


def test_parser_placement_and_optimizer_groups():
    """CNeB in the (c1, c2, ...) branch and repeated inside (models/yolo.py:1523-1530); ConvMix and CSPCM there and NOT repeated inside
    (:1531-1535): n > 1 is a Repeat.  A ConvMix row must name the channels behind it.  train.py:125-133 groups every parameter that is a
    `.weight` or a `.bias`; gamma is neither, so it is in no group - on the restatement as here."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_convnext_cfg
    from somi_amd.model import Model, _CH, _REPEAT_INSIDE
    from somi_amd.optim import reference_param_groups
    assert _CH['CNeB'] is MB.CNeB and _CH['ConvMix'] is MB.ConvMix and _CH['CSPCM'] is MB.CSPCM
    assert 'CNeB' in _REPEAT_INSIDE and 'ConvMix' not in _REPEAT_INSIDE and 'CSPCM' not in _REPEAT_INSIDE
    for name in ('ConvNextBlock', 'LayerNorm_s'):
        assert name not in _CH
        cfg = yolov5_convnext_cfg(0.25, 0.33, nc=4)
        cfg['backbone'][2][2] = name
        with pytest.raises(NotImplementedError, match=f"module '{name}' is outside the SOMI hot path"):
            Model(cfg)
    cfg = yolov5_convnext_cfg(0.25, 0.67, nc=4)
    cfg['backbone'][4] = [-1, 6, 'ConvMix', [256, 7]]             # 64 channels at width 0.25, behind a Conv of 64: legal, four in a row
    m = Model(cfg)
    assert type(m.model[4]) is MB.Repeat and [type(b) for b in m.model[4]] == [MB.ConvMix] * 4 and m.model[4][0].Resnet[0].kernel_size == (7, 7)
    cfg['backbone'][4] = [-1, 1, 'ConvMix', [512]]
    with pytest.raises(ValueError, match=r"a 'ConvMix' row that names 128 channels \(scaled\) behind 64"):
        Model(cfg)
    cfg['backbone'][4] = [-1, 6, 'CSPCM', [512]]
    with pytest.raises(NotImplementedError, match='4 repeats of CSPCM from 64 to 128 channels'):
        Model(cfg)
    for tag, mk in R.BLOCKS.items():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        gammas = sorted(n for n in names.values() if n == 'gamma' or n.endswith('.gamma'))
        assert sorted(g0 + g1 + g2 + gammas) == sorted(names.values()) and not set(gammas) & set(g0 + g1 + g2), 'only the gammas are in no group'
        assert len(set(g0 + g1 + g2)) == len(g0 + g1 + g2), 'a parameter is in two groups'
        assert len(gammas) == {'cnxblock': 1, 'cneb': 2, 'cneb_16_48': 1}.get(tag, 0)
        assert all(n.endswith('.bias') for n in g2) and all(n.endswith(('bn.weight', 'Resnet.2.weight', 'Conv_1x1.2.weight')) for n in g0)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]
        if gammas:
            assert any(n.endswith('norm.weight') for n in g1) and any(n.endswith('dwconv.weight') for n in g1)      # LayerNorm's scale decays


def test_convnext_graphs_match_the_oracle(monkeypatch):
    """The same layer table, state dict and parameter count as the oracle Model for both forms, at depth 0.33 and 0.67 (n > 1 inside CNeB, and
    CSPCM rows that are Repeats of whole modules)."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cfg, yolov5_convnext_cfg
    from somi_amd.model import Model
    from oracle.somi_ref import Model as OModel
    R.register(monkeypatch)
    for where, cls in (('cneb', MB.CNeB), ('cspcm', MB.CSPCM)):
        for width, depth in ((0.25, 0.33), (0.25, 0.67)):
            cfg = yolov5_convnext_cfg(width, depth, nc=4, where=where)
            ref, mine = OModel(cfg), Model(cfg)
            want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
            got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
            assert list(got) == list(want)
            assert got == want
            assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
            assert [m.np for m in mine.model] == [m.np for m in ref.model]
            assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
            assert mine.save == ref.save and [(m.i, m.f, m.type) for m in mine.model] == [(m.i, m.f, m.type) for m in ref.model]
            mine.load_state_dict(ref.state_dict())
            ref.load_state_dict(mine.state_dict())
            assert mine.fuse() is mine
            ns = [1, 2, 3, 1] if depth == 0.33 else [2, 4, 6, 2]
            rows = [mine.model[i] for i in (2, 4, 6, 8)]
            if where == 'cneb':
                assert [type(r) for r in rows] == [cls] * 4 and [len(r.m) for r in rows] == ns
                assert f'model.6.m.{ns[2] - 1}.gamma' in got and 'model.2.m.0.norm.weight' in got
            else:
                assert [type(r) for r in rows] == [cls if n == 1 else MB.Repeat for n in ns]
                assert [len(r) if isinstance(r, MB.Repeat) else 1 for r in rows] == ns
                assert all(type(b) is cls and len(b.m) == 1 for r in rows if isinstance(r, MB.Repeat) for b in r)
                assert (f'model.6.{ns[2] - 1}.m.0.Resnet.2.running_var' in got) and ('model.8.m.0.Conv_1x1.0.bias' in got) == (ns[3] == 1)
            base = yolov5_cfg(width, depth, nc=4)
            assert cfg['head'] == base['head'] and [r[:2] + r[3:] for r in cfg['backbone']] == [r[:2] + r[3:] for r in base['backbone']]
            swapped = [(a[2], b[2]) for a, b in zip(base['backbone'], cfg['backbone']) if a[2] != b[2]]
            assert swapped == [('C3', cls.__name__)] * 4


def test_cfg_defaults_and_the_other_cfgs_are_unchanged():
    from somi_amd import configs
    from somi_amd.model import Model
    cfg = configs.yolov5_convnext_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, configs.COCO_ANCHORS)
    assert list(inspect.signature(configs.yolov5_convnext_cfg).parameters) == ['width', 'depth', 'nc', 'anchors', 'where']
    assert inspect.signature(configs.yolov5_convnext_cfg).parameters['where'].default == 'cneb'
    assert [r[2] for r in cfg['backbone']] == ['Conv', 'Conv', 'CNeB', 'Conv', 'CNeB', 'Conv', 'CNeB', 'Conv', 'CNeB', 'SPPF']
    assert [r[2] for r in configs.yolov5_convnext_cfg(where='cspcm')['backbone']][2::2] == ['CSPCM'] * 4
    with pytest.raises(ValueError, match=r"where must be one of \('cneb', 'cspcm'\), got 'convmix'"):
        configs.yolov5_convnext_cfg(where='convmix')
    others = [configs.yolov5_cfg(), configs.yolov5_cfg(version='5.0'), configs.yolov5_ghost_cfg(), configs.yolov5_cpca_cfg(), configs.yolov5_asf_cfg(),
              configs.yolov5_swin_cfg(), configs.yolov5_slimneck_cfg(), configs.yolov10_cfg(), configs.somi_cfg()]
    assert all(r[2] not in ('CNeB', 'ConvMix', 'CSPCM') for c in others for r in c['backbone'] + c['head'])
    cfg = configs.yolov5_convnext_cfg(0.25, 0.33, nc=4)
    cfg['backbone'][8][2] = 'C3TR'                                # stays outside
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


def test_block_seeds_are_the_ones_the_rule_gives():
    """convnext_ref.BLOCK_SEEDS: per block the first of the seeds 0..7 whose fp32-against-fp64 figure is below half the bar - computed from the
    restatement alone."""
    for tag in R.BLOCKS:
        for seed in range(8):
            bars = R.block_figures(tag, seed)
            print(f'{tag} seed {seed}: fp32 against fp64 {bars:.3f} x the bar')
            if bars < 0.5:
                break
        assert R.BLOCK_SEEDS[tag] == seed, f'{tag}: the rule gives seed {seed}'


@pytest.mark.parametrize('where', sorted(R.GRAPH_SEEDS))
def test_the_graph_case_is_one_the_fp32_oracle_can_be_judged_on(where, monkeypatch):
    """convnext_ref.GRAPH_SEEDS is the FIRST of the candidates (fill 1..4) x (batch 0..3) at which the fp32 CPU oracle's parameter gradients are
    below half check_train_step's bar (2e-3 * scale + 2e-6) against its own fp64 twin's."""
    R.register(monkeypatch)
    for cand in ((fill, batch) for fill in range(1, 5) for batch in range(4)):
        bars = R.graph_figures(where, cand)
        print(f'{where} {cand}: fp32 oracle against fp64 at {bars:.3f} x the bar')
        if bars < 0.5:
            break
    assert R.GRAPH_SEEDS[where] == cand, f'the rule gives {cand}'


def test_new_symbols_are_declared_bound_and_exported():
    from somi_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/somi_hip.h'
        assert name in _lib.SIGNATURES, f'{name} is not bound in _lib.SIGNATURES'
        assert hasattr(L, name), f'{name} is not exported'
    for fn in ('dwlk', 'dwlk_dgrad', 'dwlk_wgrad', 'dwlk_strips_per_workgroup', 'dwlk_strip_length'):
        assert callable(getattr(ops, fn))
    assert 'the tensor WRITTEN is the pre-activation' in hdr and 'act(conv + bias) - stat_pivot' in hdr
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'dwlk.hip' in mk and 'dwlk' not in mk.split('ATOMIC_SRCS :=')[1].splitlines()[0]       # no -munsafe-fp-atomics
    src = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'dwlk.hip')).read()
    assert 'SOMI_REQUIRE_SLICES' in src and not re.search(r'\batomic[A-Z]\w*\b', src) and 'asm' not in src


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def _calls(_lib, L):
    """name -> (call(slices, **scalars), the slices in argument order, which of them are optional): made-up addresses, C = 8."""
    S = _lib.Slice
    w = dict(w=0xA0000, w_cs=8, bias=0xB0000, k=9, act=2, ps=0xC0000, pt=0xD0000, B=1, H=4, W=6, C=8, ssum=None, ssq=None, piv=None,
             dw=0xE0000, db=0xF0000, acc=0, ws=0x100000, ws_floats=1 << 40)

    def fwd(s, **kw):
        a = dict(w, **kw)
        return L.somi_dwlk_nhwc_f32(s['x'], a['w'], a['w_cs'], a['bias'], a['k'], a['act'], a['ps'], a['pt'], s['y'], s['residual'], a['B'], a['H'],
                                    a['W'], a['C'], a['ssum'], a['ssq'], a['piv'], None)

    def dgrad(s, **kw):
        a = dict(w, **kw)
        return L.somi_dwlk_dgrad_nhwc_f32(s['dy'], a['w'], a['w_cs'], a['k'], s['dx'], s['acc1'], s['acc2'], a['B'], a['H'], a['W'], a['C'], None)

    def wgrad(s, **kw):
        a = dict(w, **kw)
        return L.somi_dwlk_wgrad_nhwc_f32(s['x'], s['dy'], a['B'], a['H'], a['W'], a['C'], a['k'], a['dw'], a['db'], a['acc'], a['ws'], a['ws_floats'],
                                          None)
    make = lambda names: {n: S(0x10000 * (i + 1), 16, 4) for i, n in enumerate(names)}     # noqa: E731  width 8 from offset 4 of 16
    return {'dwlk': (fwd, lambda: make(('x', 'y', 'residual')), ('residual',)),
            'dwlk dgrad': (dgrad, lambda: make(('dy', 'dx', 'acc1', 'acc2')), ('acc1', 'acc2')),
            'dwlk wgrad': (wgrad, lambda: make(('x', 'dy')), ())}


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    """Every slice an entry point reads or writes, broken in six ways, is SOMI_EINVAL with a message that names it (an optional slice without a
    pointer is no slice); k = 5 and 11, channels that are no multiple of 4, another activation and a tensor beyond 2^30 floats are
    SOMI_ENOTIMPL; empty sizes, missing or misaligned weights and vectors, a narrow weight stride, one statistics buffer without the other and
    statistics together with a post-affine or a residual are SOMI_EINVAL; a short workspace is SOMI_EWORKSPACE.  A rejected call launches
    nothing, so the made-up addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    calls = _calls(_lib, L)
    for who, (call, slices, optional) in calls.items():
        for field in slices():
            for what, brk in BREAKS:
                s = slices()
                brk(s[field])
                if field in optional and what == 'pointer NULL':
                    continue
                assert call(s) == -1, f'{who}: {field}: {what} is let through'
                assert f'{who}: {field} = ['.encode() in L.somi_last_error(), f'{who}: {field}: {what}: {L.somi_last_error()}'
        for k in (5, 11, 3, 0):
            assert call(slices(), k=k) == -2 and f'kernel size {k} (7 or 9 only'.encode() in L.somi_last_error(), f'{who}: k = {k}: {L.somi_last_error()}'
        for c in (6, 2):
            assert call(slices(), C=c) == -2 and f'{c} channels (a multiple of 4 only)'.encode() in L.somi_last_error(), f'{who}: C = {c}'
        for kw in (dict(H=0), dict(B=-1), dict(W=0), dict(C=0)):
            assert call(slices(), **kw) == -1 and b'bad sizes' in L.somi_last_error(), f'{who} {kw}: {L.somi_last_error()}'
        assert call(slices(), B=1 << 14, H=1 << 7, W=1 << 7) == -2 and b'more than 2^30 floats' in L.somi_last_error(), who
    fwd, slices, _ = calls['dwlk']
    for kw, rc, word in ((dict(act=1), -2, b'activation 1 (none or gelu only)'), (dict(act=3), -2, b'activation 3'), (dict(w=None), -1, b'w must be 16 B aligned'),
                         (dict(w=0xA0004), -1, b'w must be 16 B aligned'), (dict(w_cs=4), -1, b'row stride w_cs (4)'), (dict(w_cs=10), -1, b'row stride w_cs (10)'),
                         (dict(bias=0xB0008), -1, b'bias, post_scale and post_shift'), (dict(pt=0xD0004), -1, b'bias, post_scale and post_shift'),
                         (dict(ssum=0x200000), -1, b'bad statistics buffers'), (dict(ssum=0x200000, ssq=0x300004), -1, b'bad statistics buffers'),
                         (dict(ssum=0x200000, ssq=0x300000, ps=None, pt=None), -1, b'with statistics the pre-activation is written'),
                         (dict(ssum=0x200000, ssq=0x300000), -1, b'with statistics the pre-activation is written')):
        assert fwd(slices(), **kw) == rc and word in L.somi_last_error(), f'dwlk {kw}: {L.somi_last_error()}'
    dgrad, slices, _ = calls['dwlk dgrad']
    assert dgrad(slices(), w=None) == -1 and dgrad(slices(), w_cs=6) == -1 and b'row stride w_cs (6)' in L.somi_last_error()
    wgrad, slices, _ = calls['dwlk wgrad']
    assert wgrad(slices(), dw=None) == -1 and b'dw and a 16-byte aligned workspace' in L.somi_last_error()
    assert wgrad(slices(), ws=0x100008) == -1 and wgrad(slices(), ws=None) == -1
    need = L.somi_dwlk_wgrad_workspace_floats(1, 4, 6, 8, 9)
    assert need == 82 * 8 and wgrad(slices(), ws_floats=need - 1) == -3 and b'workspace too small' in L.somi_last_error()


def test_the_plan_export_is_host_arithmetic():
    """A workgroup is nq quads wide (the power of two that covers C / 4, 64 at most, further quads in a second grid dimension) and 256 / nq
    strips of 8 outputs tall; it walks as many such rows of strips as leave about 2048 workgroups (512 for the weight gradient), 64 at most.
    The shapes of tests/test_convnext_gpu.py: the plain ones walk once under both plans, the walking ones are the smallest that walk twice."""
    from somi_amd import _lib, ops
    walks = ops.dwlk_strips_per_workgroup
    assert ops.dwlk_strip_length() == R.STRIP == 8
    assert all(walks(*s, c) == 1 and walks(*s, c, True) == 1 for c in R.WIDTHS for s in R.SHAPES)
    for c, (b, h, w) in R.WALK_FWD.items():
        assert walks(b, h, w, c) == 2 and walks(b, h - 1, w, c) == 1, (c, b, h, w)
    for c, (b, h, w) in R.WALK_WGRAD.items():
        assert walks(b, h, w, c, True) == 2 and walks(b, h - 1, w, c, True) == 1 and walks(b, h, w, c) == 1, (c, b, h, w)
    assert walks(32, 160, 160, 32) == 1 and walks(32, 160, 160, 32, True) == 6      # 102400 strips, 32 a workgroup row: 3200 rows
    assert walks(32, 20, 20, 256) == 1 and walks(128, 160, 160, 64) == 12 and walks(128, 160, 160, 64, True) == 50
    assert walks(1 << 12, 1 << 10, 1 << 7, 4) == 64               # 2^26 strips, 256 a workgroup row: 128 rows a workgroup, capped
    assert walks(0, 4, 4, 8) == 0 and walks(1, 4, 4, 6) == 0 and walks(1, 4, 4, 0) == 0 and walks(1, -1, 4, 8) == 0
    L = _lib.lib()
    assert L.somi_dwlk_stat_rows(3, 5, 7, 12) == 1 and L.somi_dwlk_stat_rows(1, 4, 4, 6) == 0
    assert L.somi_dwlk_stat_rows(32, 160, 160, 32) == 3200 and L.somi_dwlk_wgrad_workspace_floats(32, 160, 160, 32, 7) == 534 * 50 * 32


CASES = [(k, c, s) for k in R.KS for c in R.WIDTHS for s in R.SHAPES + ['walk', 'walk_wgrad']]


@pytest.mark.parametrize('k,c,shape', CASES, ids=lambda v: v if isinstance(v, str) else ('x'.join(map(str, v)) if isinstance(v, tuple) else str(v)))
def test_fp32_cpu_reference_holds_half_of_each_kernel_bar(k, c, shape):
    """The bars of the kernel tests are the project's POINT (pointwise results) and REDUCED (sums over pixels), of max |want|: an fp32
    computation of each quantity on the CPU stays below HALF of its bar against fp64 at every case the GPU tests use, the walking shapes
    included - so the bars can be held in fp32 and a miss on the GPU is the kernel's."""
    shape = {'walk': R.WALK_FWD[c], 'walk_wgrad': R.WALK_WGRAD[c]}.get(shape, shape)
    t = R.kernel_case(c, k, shape)
    d = {n: v.double() for n, v in t.items()}

    def ratio(got, want, bar):
        return ((got.double() - want).abs().max() / (bar * (want.abs().max() + 1e-12))).item()
    pre32, pre = R.dwlk_fwd_ref(t['x'], t['w'], t['bias']), R.dwlk_fwd_ref(d['x'], d['w'], d['bias'])
    full32 = F.gelu(pre32) * t['ps'] + t['pt'] + t['res']
    full = R.gelu64(pre) * d['ps'] + d['pt'] + d['res']
    g32, g = F.gelu(pre32) - t['pivot'], R.gelu64(pre) - d['pivot']
    (dx32, dw32, db32), (dx, dw, db) = R.dwlk_grads_ref(t['x'], t['w'], t['dy']), R.dwlk_grads_ref(d['x'], d['w'], d['dy'])
    figures = dict(pre=ratio(pre32, pre, POINT), full=ratio(full32, full, POINT), dx=ratio(dx32 + t['acc'], dx + d['acc'], POINT),
                   sum=ratio(g32.sum((0, 1, 2)), g.sum((0, 1, 2)), REDUCED), sumsq=ratio((g32 * g32).sum((0, 1, 2)), (g * g).sum((0, 1, 2)), REDUCED),
                   dw=ratio(dw32, dw, REDUCED), db=ratio(db32, db, REDUCED))
    print(f'k {k} c {c} {shape}: ' + ', '.join(f'{n} {v:.3f}' for n, v in figures.items()))
    assert max(figures.values()) <= 0.5, figures


def test_kernel_references_are_the_convolution():
    """The shifted-sum references of convnext_ref (written so that a million-row map needs no im2col) equal torch's conv2d and its autograd in
    fp64, on a map smaller than the kernel, a ragged one and a single pixel."""
    for k in R.KS:
        for shape in R.SHAPES:
            d = {n: v.double() for n, v in R.kernel_case(12, k, shape).items()}
            x, w, b = d['x'].clone().requires_grad_(True), d['w'].clone().requires_grad_(True), d['bias'].clone().requires_grad_(True)
            y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=k // 2, groups=12).permute(0, 2, 3, 1)
            y.backward(d['dy'])
            assert (R.dwlk_fwd_ref(d['x'], d['w'], d['bias']) - y).abs().max() < 1e-12
            assert (R.dwlk_fwd_ref(d['x'], d['w'], d['bias'], 'gelu') - F.gelu(y)).abs().max() < 1e-12
            for got, want in zip(R.dwlk_grads_ref(d['x'], d['w'], d['dy']), (x.grad, w.grad, b.grad)):
                assert (got - want).abs().max() < 1e-12 * max(1.0, want.abs().max().item())
