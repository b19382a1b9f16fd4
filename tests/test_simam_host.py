"""CPU checks of the SimAM attention family (SimAM, models/common.py:2915-2939; PSSimAM, :2942-2961; SimAMWithSlicing, SimAMWithFlexibleSlicing
and Conv_SWS, :9374-9495): the test restatement (tests/simam_ref.py) reproduces the reference's own classes through the
tests/golden/block_simam*.npz fixtures, and two plausible but wrong restatements do not; the analytic gradient the kernels implement equals
autograd in fp64; state-dict keys, the declared contract and every limit are as specified; the parser treats the five names as the reference
does; and the new entry points are declared, bound, exported and refuse bad descriptors without a launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import simam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_simam_stats_nhwc_f32', 'somi_simam_apply_nhwc_f32', 'somi_simam_bwd_sums_nhwc_f32', 'somi_simam_bwd_input_nhwc_f32',
               'somi_simam_workspace_floats', 'somi_simam_desc_bytes')
FAMILY = ('SimAM', 'SimAMWithSlicing', 'SimAMWithFlexibleSlicing', 'Conv_SWS', 'PSSimAM')


def _fixture(tag):
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    return torch.from_numpy(d['x']), {m: torch.from_numpy(d[f'out_{m}']) for m in ('eval', 'train')}


@pytest.mark.parametrize('tag', R.FIXTURES)
def test_restatement_reproduces_the_reference(tag):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    x, want = _fixture(tag)
    make, shape = R.BLOCKS[tag]
    assert tuple(x.shape) == shape
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        err = (y - want[mode]).abs().max().item()
        assert y.shape == want[mode].shape and err <= 1e-5 * want[mode].abs().max().item(), f'{tag} {mode}: {err:.3e}'


def test_quadrants_share_one_n_and_windows_divide_by_the_running_count():
    """Two wrong restatements miss the fixtures: quadrants with each region's own N - 1 (on 7x5 the regions have 6, 9, 8 and 12 pixels and all
    use n = 5), and windows divided by the final coverage count.  The overlap fixture has both uncovered pixels and pixels under four windows."""
    x, want = _fixture('simam_slicing')
    assert x.shape[2] % 2 == 1 and x.shape[3] % 2 == 1
    scale = want['eval'].abs().max().item()
    assert (R.quadrants(x, 1e-4) - want['eval']).abs().max().item() <= 1e-5 * scale
    wrong = (R.quadrants(x, 1e-4, own_n=True) - want['eval']).abs().max().item()
    print(f'quadrants with their own N - 1: off by {wrong / scale:.3f} of the largest value')
    assert wrong > 1e-2 * scale, f'own-N quadrants are only {wrong:.3e} off: the fixture does not tell the two apart'
    x, want = _fixture('simam_windows_overlap')
    scale = want['eval'].abs().max().item()
    assert (R.windows(x, 4, 2, 1e-4) - want['eval']).abs().max().item() <= 1e-5 * scale
    wrong = (R.windows(x, 4, 2, 1e-4, final_count=True) - want['eval']).abs().max().item()
    print(f'windows over the final count: off by {wrong / scale:.3f} of the largest value')
    assert wrong > 1e-2 * scale, f'final-count windows are only {wrong:.3e} off: the fixture does not tell the two apart'
    cov = R.coverage(11, 13, 4, 2)
    assert int((cov == 0).sum()) == 23 and int(cov.max()) == 4
    assert bool((want['eval'][:, :, cov == 0] == 0).all()), 'a pixel no window covers is not zero in the reference output'
    assert R.window_stride(4, 0.5) == 2 and R.window_stride(5, 0.3) == 3 and R.window_stride(8, 0.0) == 8


@pytest.mark.parametrize('mode,shape,t,st,add', [('map', (2, 3, 5, 7), None, None, False), ('map', (1, 2, 2, 1), None, None, True),
                                                 ('quadrants', (2, 3, 7, 5), None, None, False), ('quadrants', (1, 2, 2, 4), None, None, True),
                                                 ('windows', (2, 3, 11, 13), 4, 4, False), ('windows', (2, 3, 11, 13), 4, 2, True),
                                                 ('windows', (1, 2, 11, 13), 5, 3, False), ('windows', (1, 2, 8, 8), 8, 4, False)])
def test_analytic_gradient_equals_autograd_in_fp64(mode, shape, t, st, add):
    """The formula simam.hip implements, dx = [g +] sum_r (w g s + 2 T d / D - 2 A / (N D) - (8 / n) d B / D^2), against autograd of the
    restatement, fp64, all three modes, with and without the added input."""
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_(True)
    g = torch.randn(*shape, generator=gen, dtype=torch.float64)
    H, W = shape[2:]
    y = {'map': lambda: R.gate(x, H * W - 1, 1e-4), 'quadrants': lambda: R.quadrants(x, 1e-4), 'windows': lambda: R.windows(x, t, st, 1e-4)}[mode]()
    (y + x if add else y).backward(g)
    regions, n = R.region_list(mode, H, W, t, st)
    with torch.no_grad():
        dx = R.analytic_dx(x.detach(), g, regions, n, 1e-4, add_input=add)
    err = (dx - x.grad).abs().max().item()
    print(f'{mode} {shape}: analytic against autograd {err:.3e} (scale {x.grad.abs().max().item():.3e})')
    assert err <= 1e-12 * max(1.0, x.grad.abs().max().item())


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    for tag, (make, _) in R.BLOCKS.items():
        a, b = make(R), make(MB)
        assert list(a.state_dict()) == list(b.state_dict()), tag
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # checkpoints load both ways
        a.load_state_dict(b.state_dict())
    for gate in (MB.SimAM(16), MB.SimAMWithSlicing(16), MB.SimAMWithFlexibleSlicing(16, 4, 0.5)):
        assert list(gate.state_dict()) == [] and list(gate.parameters()) == []
    sws = MB.Conv_SWS(16, 32, 4, 0.5, 1e-4, 3, 2)
    assert [n for n, _ in sws.named_children()] == ['conv', 'bn', 'act', 'att']
    assert list(sws.state_dict()) == ['conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var', 'bn.num_batches_tracked']
    assert sws.conv.kernel_size == (3, 3) and sws.conv.stride == (2, 2) and sws.conv.padding == (1, 1) and sws.att.stride == (2, 2)
    assert not hasattr(sws, 'fuseforward')
    ps = MB.PSSimAM(32, 32)
    assert [n for n, _ in ps.named_children()] == ['cv1', 'cv2', 'attn', 'ffn'] and ps.c == 16 and type(ps.attn) is MB.SimAM
    assert MB.SimAMWithFlexibleSlicing(8, 8).stride == (8, 8) and MB.SimAMWithFlexibleSlicing(8, 5, 0.3).stride == (3, 3)


def test_contract_is_declared_on_each_class_itself():
    from somi_amd import blocks as MB
    for name in FAMILY:
        cls = getattr(MB, name)
        assert cls.__dict__['accumulates'] is False and cls.__dict__['folds_pooled'] is False and 'reduction' in cls.__dict__, name
        assert list(inspect.signature(cls.backward).parameters)[2:5] == ['dx_out', 'accumulate', 'need_dx'], name
        assert 'forward' in cls.__dict__ or name.startswith('SimAM'), name
    assert MB.Conv_SWS(16, 32, 4, 0.5, 1e-4, 3, 2).reduction == 2 and MB.Conv_SWS(16, 32, 4).reduction == 1
    assert MB.SimAM(8).reduction == MB.SimAMWithSlicing(8).reduction == MB.SimAMWithFlexibleSlicing(8, 4).reduction == MB.PSSimAM(8, 8).reduction == 1


def test_every_limit_raises_by_name():
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    from somi_amd.configs import yolov5_simam_cfg
    from somi_amd.model import Model
    z = lambda h, w: Act(torch.zeros(1, h, w, 8))                 # noqa: E731  (CPU tensors: every limit is raised before a launch)
    with pytest.raises(RuntimeError, match='one pixel has no variance'):
        MB.SimAM(8).eval()(z(1, 1))
    for h, w in ((1, 8), (8, 1), (2, 3), (3, 3)):
        with pytest.raises(RuntimeError, match='quadrant of .* has no variance'):
            MB.SimAMWithSlicing(8).eval()(z(h, w))
    with pytest.raises(ValueError, match='target_size 1'):
        MB.SimAMWithFlexibleSlicing(8, 1)
    with pytest.raises(RuntimeError, match='7x9 map is smaller than target_size 8'):
        MB.SimAMWithFlexibleSlicing(8, 8).eval()(z(7, 9))
    with pytest.raises(RuntimeError, match='smaller than target_size 8'):
        MB.Conv_SWS(8, 8, 8, 0.5).eval()(z(9, 7))
    with pytest.raises(ValueError, match='overlap_ratio 0.9'):
        MB.SimAMWithFlexibleSlicing(8, 4, 0.9)                    # int(4 * 0.1) = 0
    with pytest.raises(NotImplementedError, match='overlap_ratio 0.8'):
        MB.SimAMWithFlexibleSlicing(8, 8, 0.8)                    # stride 1: 8 windows over a pixel
    MB.SimAMWithFlexibleSlicing(8, 8, 0.75)                       # stride 2: 4 windows, allowed
    with pytest.raises(ValueError, match='PSSimAM needs c1 == c2'):
        MB.PSSimAM(32, 64)
    with pytest.raises(NotImplementedError, match='multiples of 4'):
        MB.SimAM(6).eval()(Act(torch.zeros(1, 4, 4, 16), 4, 6))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.SimAM(8).eval()(z(4, 4))
    cfg = yolov5_simam_cfg(0.25, 0.33, nc=10, where='row')
    cfg['backbone'][10][0] = 8
    with pytest.raises(NotImplementedError, match="'SimAM' row from 8"):
        Model(cfg)
    cfg = yolov5_simam_cfg(0.25, 0.33, nc=10, where='slicing')
    cfg['backbone'][10][3] = [512]
    with pytest.raises(ValueError, match="'SimAMWithSlicing' row that names 128 channels .* behind 256"):
        Model(cfg)
    cfg['backbone'][10][2:] = ['SimAMWithFlexibleSlicing', [512, 2]]
    with pytest.raises(ValueError, match="'SimAMWithFlexibleSlicing' row that names 128"):
        Model(cfg)
    with pytest.raises(ValueError, match='where must be one of'):
        yolov5_simam_cfg(where='neck')


@pytest.mark.parametrize('where', R.WHERE)
def test_parser_gives_the_oracle_layer_table(where, monkeypatch):
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cfg, yolov5_simam_cfg
    from somi_amd.model import Model, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert not set(FAMILY) & set(_REPEAT_INSIDE)
    cfg = yolov5_simam_cfg(0.25, 0.33, nc=10, where=where)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    mine.load_state_dict(ref.state_dict())
    assert mine.fuse() is mine
    base = yolov5_cfg(0.25, 0.33, nc=10)
    if where == 'sws':
        assert cfg['head'] == base['head'] and [r[2] for r in cfg['backbone']].count('Conv_SWS') == 2
        assert cfg['backbone'][3] == [-1, 1, 'Conv_SWS', [256, 8, 0.5, 1e-4, 3, 2]] and cfg['backbone'][5][3][0] == 512
        assert [i for i, r in enumerate(cfg['backbone']) if r != base['backbone'][i]] == [3, 5]
        m3, m5 = mine.model[3], mine.model[5]
        assert type(m3) is MB.Conv_SWS and (m3.conv.in_channels, m3.conv.out_channels, m3.att.target_size, m3.att.stride) == (32, 64, 8, (4, 4))
        assert type(m5) is MB.Conv_SWS and (m5.conv.in_channels, m5.conv.out_channels) == (64, 128)
    else:
        name = {'row': 'SimAM', 'slicing': 'SimAMWithSlicing', 'ps': 'PSSimAM'}[where]
        assert cfg['backbone'][:10] == base['backbone'] and cfg['backbone'][10][:3] == [-1, 1, name]
        assert cfg['backbone'][10][3] == ([256, 256] if where == 'ps' else [1024])
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 15], [-1, 11], [18, 21, 24]]
        assert type(mine.model[10]).__name__ == name and mine.model[11].conv.in_channels == 256
        if where == 'ps':
            assert mine.model[10].c == 128


def test_cfg_defaults_and_the_stock_cfg_names_none_of_the_family():
    from somi_amd.configs import COCO_ANCHORS, yolov5_cfg, yolov5_simam_cfg
    cfg = yolov5_simam_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert cfg['backbone'][10] == [-1, 1, 'SimAM', [1024]]
    assert yolov5_simam_cfg(where='ps')['backbone'][10] == [-1, 1, 'PSSimAM', [512, 512]]
    assert all(r[2] not in FAMILY for r in yolov5_cfg()['backbone'] + yolov5_cfg()['head'])


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
    assert _lib.lib().somi_simam_desc_bytes() == ctypes.sizeof(_lib.SimamDesc)
    for fn in ('simam_grid', 'simam_stats', 'simam_apply', 'simam_backward_sums', 'simam_backward_input'):
        assert callable(getattr(ops, fn))
    assert 'simam.hip' in open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()


def test_grids_of_the_three_modes():
    from somi_amd import ops
    assert ops.simam_grid('map', 5, 7) == (1, 1, 5, 7, 5, 7, 0, 34.0, 1e-4)
    assert ops.simam_grid('quadrants', 7, 5, 1e-3) == (2, 2, 3, 2, 3, 2, 1, 5.0, 1e-3)
    assert ops.simam_grid('windows', 11, 13, 1e-4, 4, 2) == (4, 5, 2, 2, 4, 4, 0, 15.0, 1e-4)
    assert ops.simam_grid('windows', 160, 160, 1e-4, 8, 4)[:2] == (39, 39)
    assert ops.simam_grid('windows', 8, 8, 1e-4, 8, 4)[:2] == (1, 1)


def _desc(_lib, grid=(4, 5, 2, 2, 4, 4, 0, 15.0, 1e-4)):
    d = _lib.SimamDesc()
    d.x, d.y, d.dx = _lib.Slice(0x10000, 16, 4), _lib.Slice(0x20000, 16, 4), _lib.Slice(0x30000, 16, 4)
    d.stats, d.sums = 0x40000, 0x50000
    d.B, d.H, d.W, d.C = 1, 11, 13, 8
    d.ny, d.nx, d.step_y, d.step_x, d.len_y, d.len_x, d.stretch_last, d.n, d.lam = grid
    d.workspace, d.workspace_floats = 0xA0000, 1 << 30
    return d


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_bad_descriptors_are_refused_without_a_launch():
    """Every slice an entry point reads or writes, broken in six ways, is SOMI_EINVAL with a message that names it; so are bad sizes, bad region
    grids, regions of one pixel, a non-positive n or lambda, missing statistics and a short workspace.  A rejected call launches nothing, so the
    made-up addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    entries = {'stats': (L.somi_simam_stats_nhwc_f32, {'x': 'x'}),
               'apply': (L.somi_simam_apply_nhwc_f32, {'x': 'x', 'y': 'out'}),
               'sums': (L.somi_simam_bwd_sums_nhwc_f32, {'x': 'x', 'y': 'dout'}),
               'input': (L.somi_simam_bwd_input_nhwc_f32, {'x': 'x', 'y': 'dout', 'dx': 'dx'})}
    for key, (fn, fields) in entries.items():
        for field, name in fields.items():
            for what, brk in BREAKS:
                d = _desc(_lib)
                brk(getattr(d, field))
                assert fn(ctypes.byref(d), None) == -1, f'{key}: {name}: {what} is let through'
                assert re.search(r'\b%s = \[' % name, L.somi_last_error().decode()), f'{key}: {name}: {what}: {L.somi_last_error()}'
        for attr, value in (('C', 6), ('C', 0), ('H', 0), ('B', -1)):
            d = _desc(_lib)
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and b'bad sizes' in L.somi_last_error(), f'{key}: {attr} = {value}'
        for attr, value in (('ny', 0), ('ny', 5), ('nx', 6), ('step_y', 0), ('len_x', 0), ('len_y', 6)):
            d = _desc(_lib)
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and b'bad region grid' in L.somi_last_error(), f'{key}: {attr} = {value}'
        d = _desc(_lib, (11, 13, 1, 1, 1, 1, 0, 1.0, 1e-4))
        assert fn(ctypes.byref(d), None) == -1 and b'one pixel' in L.somi_last_error(), key
        d = _desc(_lib, (7, 9, 1, 1, 5, 5, 0, 24.0, 1e-4))
        assert fn(ctypes.byref(d), None) == -2 and b'cover a pixel' in L.somi_last_error(), key
        d = _desc(_lib, (2, 2, 5, 6, 4, 4, 1, 15.0, 1e-4))
        assert fn(ctypes.byref(d), None) == -1 and b'stretch_last' in L.somi_last_error(), key
        for attr, value in (('n', 0.0), ('n', -1.0), ('lam', 0.0), ('lam', -1e-4), ('n', float('inf'))):
            d = _desc(_lib)
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and b'must be positive' in L.somi_last_error(), f'{key}: {attr} = {value}'
        for value in (None, 0x40004):
            d = _desc(_lib)
            d.stats = value
            assert fn(ctypes.byref(d), None) == -1 and b'stats' in L.somi_last_error(), key
        assert fn(None, None) == -1
    for key in ('sums', 'input'):
        d = _desc(_lib)
        d.sums = None
        assert entries[key][0](ctypes.byref(d), None) == -1 and b'sums' in L.somi_last_error()
    whole = (1, 1, 40, 40, 40, 40, 0, 1599.0, 1e-4)               # 1600 pixels, chunks of 8 * 128: two
    for key in ('stats', 'sums'):
        d = _desc(_lib, whole)
        d.H = d.W = 40
        need = L.somi_simam_workspace_floats(ctypes.byref(d))
        assert need == 1 * 1 * 2 * 2 * 8
        d.workspace_floats = need - 1
        assert entries[key][0](ctypes.byref(d), None) == -3, f'{key}: a short workspace is let through'
        d.workspace_floats, d.workspace = need, None
        assert entries[key][0](ctypes.byref(d), None) == -1
        d.workspace = 0xA0004
        assert entries[key][0](ctypes.byref(d), None) == -1


def test_workspace_size_is_host_arithmetic():
    """B * regions * chunks * 2 * C floats when the largest region has more than one chunk of 8 * NL pixels, NL = 256 / min(C / 4, 256); else 0."""
    from somi_amd import _lib, ops
    L = _lib.lib()

    def need(B, H, W, C, grid):
        d = _desc(_lib, grid)
        d.B, d.H, d.W, d.C = B, H, W, C
        return L.somi_simam_workspace_floats(ctypes.byref(d))
    assert need(32, 160, 160, 32, ops.simam_grid('map', 160, 160)) == 32 * 1 * 100 * 2 * 32           # NL 32: 25600 / 256 chunks
    assert need(32, 160, 160, 32, ops.simam_grid('windows', 160, 160, 1e-4, 8, 4)) == 0              # 64 pixels: one chunk
    assert need(2, 33, 18, 16, ops.simam_grid('quadrants', 33, 18)) == 0                             # the largest quadrant: 17 * 9 = 153 <= 512
    assert need(1, 67, 35, 16, ops.simam_grid('map', 67, 35)) == 1 * 1 * 5 * 2 * 16                  # 2345 pixels, chunks of 512
    assert need(1, 3, 2, 1032, ops.simam_grid('map', 3, 2)) == 0                                     # 258 quads: NL 1, one chunk of 8
    assert need(1, 4, 4, 1032, ops.simam_grid('map', 4, 4)) == 1 * 1 * 2 * 2 * 1032
    assert need(1, 4, 4, 6, ops.simam_grid('map', 4, 4)) == 0 and need(0, 4, 4, 8, ops.simam_grid('map', 4, 4)) == 0
