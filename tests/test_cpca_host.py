"""CPU checks of channel prior convolutional attention (CPCA_ChannelAttention, CPCA, CPCABottleneck: models/common.py:5753-5859; C3CPCA,
:1684-1689): the test restatement (tests/cpca_ref.py) reproduces the reference's own classes through the tests/golden/block_cpca*.npz and
block_c3cpca.npz fixtures, and two plausible wrong restatements do not; state-dict keys and shapes are the restatement's; the parser gives the
oracle Model's layer table for both forms of configs.yolov5_cpca_cfg; the seeded cases of the GPU tests are the ones the selection rule gives;
limits raise by name; the new entry points are declared, bound, exported and refuse bad arguments without a launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cpca_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_cpca_fanout_nhwc_f32', 'somi_cpca_fanin_nhwc_f32', 'somi_cpca_wgrad_nhwc_f32', 'somi_cpca_wgrad_workspace_floats',
               'somi_cpca_tiles_per_workgroup', 'somi_cpca_strip_desc_bytes', 'somi_cpca_wgrad_desc_bytes', 'somi_cpca_gate_nhwc_f32', 'somi_cpca_gate_bwd_nhwc_f32',
               'somi_cpca_sigmoid2_f32', 'somi_cpca_sigmoid2_bwd_f32', 'somi_cpca_argmax_pixel_nhwc_f32')

FIXTURES = {'block_cpca': 'cpca', 'block_cpca_wide': 'cpca_wide', 'block_cpcabottleneck_sc': 'cpcabottleneck_sc',
            'block_cpcabottleneck_nosc': 'cpcabottleneck_nosc', 'block_c3cpca': 'c3cpca'}


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
    for mode, err in _fixture_errors(name, R.BLOCKS[FIXTURES[name]]).items():
        assert err <= 1e-5, f'{name} {mode}: {err:.3e}'


def test_wrong_restatements_are_ruled_out():
    """Padding V_k with H_k's bias instead of zeros misses the wide fixture (23 rows: every output row of the 21-tap branch reads rows outside
    the map); three separate 1x1 convs have another parameter count and another state dict."""
    errs = _fixture_errors('block_cpca_wide', lambda ns: ns.BiasPaddedCPCA(16))
    assert min(errs.values()) > 1e-3, f'the bias-padded restatement fits the wide fixture: {errs}'
    d = np.load(os.path.join(GOLDEN, 'block_cpca_wide.npz'))
    assert d['x'].shape[2] != d['x'].shape[3] and min(d['x'].shape[2:]) > 21
    one, three = R.CPCA(64), R.ThreeConvCPCA(64)
    count = lambda m: sum(p.numel() for p in m.parameters())      # noqa: E731
    assert count(three) == count(one) + 2 * (64 * 64 + 64)
    assert count(one) == 2 * 64 * 16 + 16 + 64 + 64 * 25 + 64 + 2 * 64 * (7 + 11 + 21) + 6 * 64 + 64 * 64 + 64


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    makes = list(R.BLOCKS.values()) + [lambda M: M.CPCA(512), lambda M: M.CPCA(32, 8), lambda M: M.C3CPCA(32, 64, 3, False),
                                       lambda M: M.CPCABottleneck(32, 32, True, 1, (3, 3), 0.5, 8), lambda M: M.CPCA_ChannelAttention(64, 16)]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # a checkpoint of the restatement loads ...
        a.load_state_dict(b.state_dict())                         # ... and ours loads there
    sd = MB.CPCA(64).state_dict()
    assert list(sd) == ['ca.fc1.weight', 'ca.fc1.bias', 'ca.fc2.weight', 'ca.fc2.bias', 'dconv5_5.weight', 'dconv5_5.bias', 'dconv1_7.weight',
                        'dconv1_7.bias', 'dconv7_1.weight', 'dconv7_1.bias', 'dconv1_11.weight', 'dconv1_11.bias', 'dconv11_1.weight',
                        'dconv11_1.bias', 'dconv1_21.weight', 'dconv1_21.bias', 'dconv21_1.weight', 'dconv21_1.bias', 'conv.weight', 'conv.bias']
    assert tuple(sd['dconv1_7.weight'].shape) == (64, 1, 1, 7) and tuple(sd['dconv21_1.weight'].shape) == (64, 1, 21, 1)
    assert tuple(sd['ca.fc1.weight'].shape) == (16, 64, 1, 1) and tuple(sd['conv.weight'].shape) == (64, 64, 1, 1)
    assert [n for n, _ in MB.CPCABottleneck(64, 64).named_children()][:4] == ['cv1', 'cv2', 'ca', 'dconv5_5']
    blk = MB.C3CPCA(128, 128, 2)
    assert len(blk.m) == 2 and all(type(m) is MB.CPCABottleneck and m.add and m.cv2.conv.kernel_size == (3, 3) for m in blk.m)
    assert blk.m[0].cv1.conv.out_channels == 64 and blk.m[0].cv1.conv.kernel_size == (1, 1)       # e = 1.0 inside, k = ((1, 1), (3, 3))


def test_contract_and_limits_are_explicit():
    from somi_amd import blocks as MB
    for cls in (MB.CPCA_ChannelAttention, MB.CPCA, MB.CPCABottleneck, MB.C3CPCA):     # declared on the class itself, not inherited
        assert (cls.__dict__['accumulates'], cls.__dict__['folds_pooled'], cls.__dict__['reduction']) == (False, False, 1), cls.__name__
        assert list(inspect.signature(cls.backward).parameters)[2:5] == ['dx_out', 'accumulate', 'need_dx'], cls.__name__
    assert issubclass(MB.C3CPCA, MB.C3) and MB.C3.accumulates is True
    with pytest.raises(NotImplementedError, match=r'CPCABottleneck\(64, 128\)'):
        MB.CPCABottleneck(64, 128)
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        MB.CPCA(6).eval()(MB.Act(torch.zeros(1, 4, 4, 8), 0, 6))
    with pytest.raises(NotImplementedError, match='stored unpadded'):
        MB.CPCA(80).eval()(MB.Act(torch.zeros(1, 4, 4, 96), 0, 80))
    with pytest.raises(RuntimeError, match='got a map of 8'):
        MB.CPCA(16).eval()(MB.Act(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.CPCA(8).eval()(MB.Act(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(NotImplementedError, match='at most 1024 channels'):
        MB.CPCA_ChannelAttention(1280, 320).eval()(MB.Act(torch.zeros(1, 2, 2, 1280)))
    from somi_amd import ops
    x = torch.zeros(2, 3, 3, 8)
    for bad, kw in ((torch.zeros(8, 4).t(), {}), (torch.zeros(4, 8, dtype=torch.float64), {}), (torch.zeros(3, 8), {}),
                    (torch.zeros(4, 8), dict(want_max=False))):
        with pytest.raises(RuntimeError, match='contiguous fp32'):
            ops.global_pool(x, c=8, out=bad, **kw)
    blk = MB.C3CPCA(64, 64, 2)
    for m in blk.m:
        m.__dict__['_pk'] = 'stale'
        m.invalidate()
        assert '_pk' not in m.__dict__
    pk = MB.CPCA(64).train()._pack(torch.device('cpu'))
    assert tuple(pk['wp'].shape) == (64, 64) and tuple(pk['wt'].shape) == (64, 64) and tuple(pk['g5'].shape) == (25, 1, 64)
    assert [tuple(w.shape) for w in pk['wh']] == [(64, 1, 1, 7), (64, 1, 1, 11), (64, 1, 1, 21)]
    assert [tuple(w.shape) for w in pk['wv']] == [(64, 1, 7, 1), (64, 1, 11, 1), (64, 1, 21, 1)]


@pytest.mark.parametrize('where', ['c3', 'row'])
def test_cpca_graph_matches_the_oracle(where, monkeypatch):
    """The same layer table, state dict and parameter count as the oracle Model, n > 1 inside C3CPCA included."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cfg, yolov5_cpca_cfg
    from somi_amd.model import Model, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert 'C3CPCA' in _REPEAT_INSIDE and 'CPCA' not in _REPEAT_INSIDE
    cfg = yolov5_cpca_cfg(0.25, 0.33, nc=10, where=where)
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
    if where == 'row':
        assert cfg['backbone'][:10] == base['backbone'] and cfg['backbone'][10] == [-1, 1, 'CPCA', []]
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 15], [-1, 11], [18, 21, 24]]
        assert type(mine.model[10]) is MB.CPCA and mine.model[10].conv.in_channels == 256 and mine.model[10].ca.fc1.out_channels == 64
    else:
        assert cfg['head'] == base['head'] and [r[2] for r in cfg['backbone']].count('C3CPCA') == 4
        assert [r[:2] + r[3:] for r in cfg['backbone']] == [r[:2] + r[3:] for r in base['backbone']]
        assert [type(mine.model[i]) for i in (2, 4, 6, 8)] == [MB.C3CPCA] * 4 and [len(mine.model[i].m) for i in (2, 4, 6, 8)] == [1, 2, 3, 1]
        assert 'model.6.m.2.dconv21_1.bias' in got and 'model.4.m.1.ca.fc2.weight' in got


def test_cfg_defaults_and_the_other_cfgs_are_unchanged():
    from somi_amd.configs import COCO_ANCHORS, yolov5_cfg, yolov5_cpca_cfg
    from somi_amd.model import Model
    cfg = yolov5_cpca_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert [r[2] for r in cfg['backbone']] == ['Conv', 'Conv', 'C3CPCA', 'Conv', 'C3CPCA', 'Conv', 'C3CPCA', 'Conv', 'C3CPCA', 'SPPF']
    assert all('CPCA' not in r[2] for r in yolov5_cfg()['backbone'] + yolov5_cfg()['head'])
    with pytest.raises(ValueError, match="'c3' or 'row'"):
        yolov5_cpca_cfg(where='neck')
    cfg = yolov5_cpca_cfg(0.25, 0.33, nc=10)
    cfg['backbone'][8][2] = 'C3TR'                                # stays outside
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


def test_optimizer_groups_follow_the_reference():
    """train.py:125-133: every .bias in the bias group, BatchNorm weights without decay, every other .weight decayed - no special case."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    for mk in R.BLOCKS.values():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert sorted(g0 + g1 + g2) == sorted(names.values()), 'a parameter is in no group'
        assert all(n.endswith('.bias') for n in g2) and not any(n.endswith('.bias') for n in g0 + g1)
        for leaf in ('dconv1_7.weight', 'dconv21_1.weight', 'dconv5_5.weight', 'conv.weight', 'ca.fc1.weight', 'ca.fc2.weight'):
            assert any(n.endswith(leaf) for n in g1) and not any(n.endswith(leaf) for n in g0 + g2)
        assert all('bn.weight' in n for n in g0)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]


def test_block_seeds_are_the_ones_the_rule_gives():
    """cpca_ref.BLOCK_SEEDS: per block the first of the seeds 0..7 whose fp32-against-fp64 figure is below half the bar and whose smallest
    channel-maximum gap is at least MIN_GAP - computed from the restatement alone."""
    for tag in R.BLOCKS:
        for seed in range(8):
            gap, bars = R.block_figures(tag, seed)
            print(f'{tag} seed {seed}: max gap {gap:.3e}, fp32 against fp64 {bars:.3f} x the bar')
            if bars < 0.5 and gap >= R.MIN_GAP:
                break
        assert R.BLOCK_SEEDS[tag] == seed, f'{tag}: the rule gives seed {seed}'


@pytest.mark.parametrize('where', ['c3', 'row'])
def test_graph_cases_are_ones_the_fp32_oracle_can_be_judged_on(where, monkeypatch):
    """cpca_ref.GRAPH_SEEDS is the FIRST of the candidates (fill 1..4) x (batch 0..3) at which the fp32 CPU oracle's parameter gradients are below
    half check_train_step's bar (2e-3 * scale + 2e-6) against its own fp64 twin's and no channel maximum of the fp64 oracle is closer than
    MIN_GAP to the runner-up: every candidate before it misses one of the two."""
    R.register(monkeypatch)
    for cand in ((fill, batch) for fill in range(1, 5) for batch in range(4)):
        gap, bars = R.graph_figures(where, cand)
        print(f'{where} {cand}: max gap {gap:.3e}, fp32 oracle against fp64 at {bars:.3f} x the bar')
        if gap >= R.MIN_GAP and bars < 0.5:
            break
    assert R.GRAPH_SEEDS[where] == cand, f'{where}: the rule gives {cand}'


def test_new_symbols_are_declared_bound_and_exported():
    from somi_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/somi_hip.h'
        assert name in _lib.SIGNATURES, f'{name} is not bound in _lib.SIGNATURES'
        assert hasattr(L, name), f'{name} is not exported'
        proto = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert not re.search(r'_coff\b', proto), f'{name} takes a slice as loose *_coff parameters'
    assert '#define SOMI_ABI_VERSION 15' in hdr and _lib.lib().somi_abi_version() == _lib.ABI_VERSION == 15
    assert _lib.lib().somi_cpca_strip_desc_bytes() == ctypes.sizeof(_lib.CpcaStripDesc)
    assert _lib.lib().somi_cpca_wgrad_desc_bytes() == ctypes.sizeof(_lib.CpcaWgradDesc)
    for fn in ('cpca_fanout', 'cpca_fanin', 'cpca_wgrad', 'cpca_gate', 'cpca_gate_backward', 'cpca_sigmoid2', 'cpca_sigmoid2_backward', 'argmax_pixel'):
        assert callable(getattr(ops, fn))
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'cpca.hip' in mk
    src = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'cpca.hip')).read()
    assert 'SOMI_REQUIRE_SLICES' in src and not re.search(r'\batomicAdd\b', src)


def _strip_desc(_lib, fanin):
    d = _lib.CpcaStripDesc()
    for i in range(4):
        d.src[i] = _lib.Slice(0x10000 * (i + 1), 16, 4)
    for i in range(3):
        d.dst[i] = _lib.Slice(0x100000 * (i + 1), 16, 4)
        d.w[i], d.bias[i], d.taps[i] = 0x1000000 * (i + 1), None, (7, 11, 21)[i]
    d.B, d.H, d.W, d.C = 1, 4, 6, 8
    return d


def _wgrad_desc(_lib):
    d = _lib.CpcaWgradDesc()
    d.u, d.ds = _lib.Slice(0x10000, 16, 4), _lib.Slice(0x20000, 16, 4)
    for i in range(3):
        d.t[i], d.dt[i], d.taps[i] = _lib.Slice(0x100000 * (i + 1), 16, 4), _lib.Slice(0x1000000 * (i + 1), 16, 4), (7, 11, 21)[i]
    d.B, d.H, d.W, d.C = 1, 4, 6, 8
    d.workspace, d.workspace_floats = 0xA0000, 1 << 30
    return d


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    """Every slice an entry point reads or writes, broken in six ways, is SOMI_EINVAL with a message that names it; C not a multiple of 4 and a
    tap set other than (7, 11, 21) are refused by name; a short workspace is SOMI_EWORKSPACE.  A rejected call launches nothing, so the made-up
    addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    strips = {'fanout': (L.somi_cpca_fanout_nhwc_f32, [('src', 0)] + [('dst', i) for i in range(3)]),
              'fanin': (L.somi_cpca_fanin_nhwc_f32, [('src', i) for i in range(4)] + [('dst', 0)])}
    for key, (fn, fields) in strips.items():
        for field, i in fields:
            for what, brk in BREAKS:
                d = _strip_desc(_lib, key == 'fanin')
                brk(getattr(d, field)[i])
                assert fn(ctypes.byref(d), None) == -1, f'{key}: {field}[{i}]: {what} is let through'
                assert f'{field}[{i}] = ['.encode() in L.somi_last_error(), f'{key}: {field}[{i}]: {what}: {L.somi_last_error()}'
        for attr, value, word in (('C', 6, b'not a multiple of 4'), ('C', 0, b'not a multiple of 4'), ('H', 0, b'bad sizes'), ('B', -1, b'bad sizes'),
                                  ('axis', 2, b'axis')):
            d = _strip_desc(_lib, key == 'fanin')
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and word in L.somi_last_error(), f'{key}: {attr} = {value}: {L.somi_last_error()}'
        d = _strip_desc(_lib, key == 'fanin')
        d.taps[1] = 9
        assert fn(ctypes.byref(d), None) == -1 and b'tap set (7, 9, 21) is not built' in L.somi_last_error()
        d = _strip_desc(_lib, key == 'fanin')
        d.w[2] = None
        assert fn(ctypes.byref(d), None) == -1 and b'three tap tensors' in L.somi_last_error()
        assert fn(None, None) == -1
    fn = L.somi_cpca_wgrad_nhwc_f32
    for field in ('u', 'ds'):
        for what, brk in BREAKS:
            d = _wgrad_desc(_lib)
            brk(getattr(d, field))
            assert fn(ctypes.byref(d), None) == -1 and f'{field} = ['.encode() in L.somi_last_error(), f'wgrad: {field}: {what}'
    for field in ('t', 'dt'):
        for i in range(3):
            for what, brk in BREAKS:
                d = _wgrad_desc(_lib)
                brk(getattr(d, field)[i])
                assert fn(ctypes.byref(d), None) == -1 and f'{field}[{i}] = ['.encode() in L.somi_last_error(), f'wgrad: {field}[{i}]: {what}'
    d = _wgrad_desc(_lib)
    d.C = 6
    assert fn(ctypes.byref(d), None) == -1 and b'not a multiple of 4' in L.somi_last_error()
    d = _wgrad_desc(_lib)
    d.taps[0] = 5
    assert fn(ctypes.byref(d), None) == -1 and b'tap set (5, 11, 21) is not built' in L.somi_last_error()
    d = _wgrad_desc(_lib)
    d.workspace_floats = L.somi_cpca_wgrad_workspace_floats(1, 4, 6, 8) - 1
    assert fn(ctypes.byref(d), None) == -3, 'a short workspace is let through'
    d = _wgrad_desc(_lib)
    d.workspace = None
    assert fn(ctypes.byref(d), None) == -1
    d = _wgrad_desc(_lib)
    d.workspace += 4
    assert fn(ctypes.byref(d), None) == -1
    assert fn(None, None) == -1
    ok, odd = _lib.Slice(0x10000, 16, 4), _lib.Slice(0x10000, 16, 6)
    assert L.somi_cpca_gate_nhwc_f32(ok, ok, odd, 10, 8, None) == -1 and b'out = [' in L.somi_last_error()
    assert L.somi_cpca_gate_nhwc_f32(ok, ok, ok, 10, 6, None) == -1 and b'not a multiple of 4' in L.somi_last_error()
    assert L.somi_cpca_gate_bwd_nhwc_f32(ok, ok, ok, ok, odd, 10, 8, None) == -1 and b'dy = [' in L.somi_last_error()
    assert L.somi_cpca_sigmoid2_f32(None, 0x1000, 2, 8, None) == -1 and L.somi_cpca_sigmoid2_bwd_f32(0x1000, None, 0x1000, 2, 8, None) == -1
    assert L.somi_cpca_argmax_pixel_nhwc_f32(odd, 0x1000, 0x2000, 1, 4, 8, None) == -1 and b'x = [' in L.somi_last_error()


def test_workspace_size_is_host_arithmetic():
    """One row of 42 (along W) and one of 40 (along H) partial sums per stage-1 workgroup and channel: rows = B x tiles along the strip (32
    positions at most) x groups of lines; a workgroup walks up to 32 tiles, halved while fewer than 512 workgroups exist."""
    from somi_amd import _lib
    L = _lib.lib()
    assert L.somi_cpca_wgrad_workspace_floats(1, 4, 6, 8) == (1 * 42 + 1 * 40) * 8               # every line of the map in one tile
    assert L.somi_cpca_wgrad_workspace_floats(1, 3, 130, 8) == (5 * 42 + 8 * 40) * 8             # 130 = 4 x 32 + 2 along W; 17 lines a tile along H
    assert L.somi_cpca_wgrad_workspace_floats(2, 5, 7, 32) == 2 * (2 * 42 + 3 * 40) * 32          # 3 lines of 8 quads fit a tile
    assert L.somi_cpca_wgrad_workspace_floats(1, 4, 4, 6) == 0 and L.somi_cpca_wgrad_workspace_floats(0, 4, 4, 8) == 0
    # tiles a workgroup walks: one at the small shapes, several where the launch has workgroups to spare (the shapes training runs at)
    tiles = L.somi_cpca_tiles_per_workgroup
    assert [tiles(2, 5, 7, 32, ax, wg) for ax in (0, 1) for wg in (0, 1)] == [1, 1, 1, 1]
    assert [tiles(32, 20, 20, 512, ax, 0) for ax in (0, 1)] == [2, 2] and [tiles(32, 20, 20, 512, ax, 1) for ax in (0, 1)] == [16, 16]
    assert tiles(32, 160, 160, 32, 0, 0) == 4 and tiles(1, 4, 4, 6, 0, 0) == 0 and tiles(1, 4, 4, 8, 2, 0) == 0
