"""CPU checks of coordinate attention (CoorAttention, models/common.py:1399-1450; CABottleneck and C3_CA, :4884-4931): the test restatement
(tests/coordatt_ref.py) reproduces the reference's own classes through the tests/golden/block_coordatt.npz, block_cabottleneck_*.npz and
block_c3_ca.npz fixtures; the parser treats the two names as the reference's does (channel scaling, C3_CA repeated as whole blocks); state-dict
keys, optimizer groups and parameter counts are the oracle's; the seeded cases of the GPU tests are ones the fp32 oracle itself can be judged on;
and the new entry points are declared, bound, exported and check their slices."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import coordatt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_coordatt_means_nhwc_f32', 'somi_coordatt_apply_nhwc_f32', 'somi_coordatt_bwd_gates_nhwc_f32',
               'somi_coordatt_bwd_input_nhwc_f32', 'somi_coordatt_workspace_floats', 'somi_coordatt_desc_bytes')

FIXTURES = {'block_coordatt': lambda M: M.CoorAttention(64, 64), 'block_cabottleneck_sc': lambda M: M.CABottleneck(64, 64, True, 1, 1.0),
            'block_cabottleneck_nosc': lambda M: M.CABottleneck(64, 64, False, 1, 1.0), 'block_c3_ca': lambda M: M.C3_CA(64, 64, 1)}


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_restatement_reproduces_the_reference(name):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    mod = fill_state(FIXTURES[name](R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == R.BLOCK_SHAPE
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        err = (y - want).abs().max().item()
        assert y.shape == want.shape and err <= 1e-5 * want.abs().max().item(), f'{name} {mode}: {err:.3e}'
    if name == 'block_coordatt':                                  # H != W in the fixture: gates swapped between rows and columns do not fit
        assert x.shape[2] != x.shape[3]


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    makes = list(R.BLOCKS.values()) + [lambda M: M.CABottleneck(96, 96), lambda M: M.CoorAttention(512, 512), lambda M: M.C3_CA(32, 64, 2, False)]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())
    ca = MB.CoorAttention(64, 64)
    assert list(ca.state_dict()) == ['conv1.weight', 'conv1.bias', 'bn1.weight', 'bn1.bias', 'bn1.running_mean', 'bn1.running_var',
                                     'bn1.num_batches_tracked', 'conv_h.weight', 'conv_h.bias', 'conv_w.weight', 'conv_w.bias']
    assert [n for n, _ in MB.CABottleneck(64, 64).named_children()] == ['cv1', 'cv2', 'conv1', 'bn1', 'conv_h', 'conv_w']
    assert MB.CoorAttention(512, 512).conv1.out_channels == 16 and ca.conv1.out_channels == 8
    assert MB.CABottleneck(512, 512, ratio=16).conv1.out_channels == 32        # mip from c1 and ratio
    blk = MB.C3_CA(128, 128, 2)
    assert len(blk.m) == 2 and all(type(m) is MB.CABottleneck and m.add and m.cv2.conv.kernel_size == (3, 3) for m in blk.m)
    assert blk.m[0].cv1.conv.out_channels == 64                   # e = 1.0 inside


def test_contract_and_limits_are_explicit():
    from somi_amd import blocks as MB
    with pytest.raises(NotImplementedError, match='inp == oup'):
        MB.CoorAttention(64, 128)
    import inspect
    for cls in (MB.CoorAttention, MB.CABottleneck, MB.C3_CA):     # declared on the class itself, not inherited
        assert (cls.__dict__['accumulates'], cls.__dict__['folds_pooled'], cls.__dict__['reduction']) == (False, False, 1), cls.__name__
        assert list(inspect.signature(cls.backward).parameters)[2:5] == ['dx_out', 'accumulate', 'need_dx'], cls.__name__
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        MB.CoorAttention(6, 6).eval()(MB.Act(torch.zeros(1, 4, 4, 8), 0, 6))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.CoorAttention(8, 8).eval()(MB.Act(torch.zeros(1, 4, 4, 8)))


def test_invalidate_drops_the_packed_gates():
    from somi_amd import blocks as MB
    blk = MB.C3_CA(64, 64, 2)
    for m in blk.m:
        m.__dict__['_pk'] = 'stale'
        m.invalidate()
        assert '_pk' not in m.__dict__
    pk = MB.CoorAttention(64, 64).eval()._pack(torch.device('cpu'))
    assert tuple(pk['w1'].shape) == (8, 64) and tuple(pk['wg'].shape) == (128, 8) and tuple(pk['bg'].shape) == (128,)
    ca = MB.CoorAttention(64, 64).train()
    pk = ca._pack(torch.device('cpu'))
    assert tuple(pk['wt1'].shape) == (64, 8) and tuple(pk['wtg'].shape) == (8, 128) and pk['rm'] is ca.bn1.running_mean


def test_eval_pack_folds_bn1_into_conv1():
    """The eval-mode packed conv1 is the reference's fuse_conv_and_bn of (conv1, bn1)."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    ref = fill_state(R.CoorAttention(64, 64), 3)
    OB.initialize_weights(ref)
    mine = MB.CoorAttention(64, 64)
    mine.load_state_dict(ref.state_dict())
    mine.bn1.eps, mine.bn1.momentum = 1e-3, 0.03
    pk = mine.eval()._pack(torch.device('cpu'))
    fused = OB.fuse_conv_and_bn(ref.conv1, ref.bn1)
    assert torch.allclose(pk['w1'], fused.weight.detach().view(8, 64), rtol=1e-6, atol=1e-7)
    assert torch.allclose(pk['b1'], fused.bias.detach(), rtol=1e-6, atol=1e-7)


def test_parser_scales_channels_and_repeats_c3_ca_as_whole_blocks(monkeypatch):
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_ca_cfg
    from somi_amd.model import Model, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert 'C3_CA' not in _REPEAT_INSIDE and 'CoorAttention' not in _REPEAT_INSIDE
    cfg = yolov5_ca_cfg(0.25, 0.33, nc=10)
    mine, ref = Model(cfg), R.oracle_model(cfg)
    assert [type(mine.model[i]).__name__ for i in (2, 4, 6, 8)] == ['C3_CA', 'Repeat', 'Repeat', 'C3_CA']
    assert len(mine.model[6]) == 3 and all(type(m) is MB.C3_CA and len(m.m) == 1 for m in mine.model[6])
    assert mine.model[6][0].cv1.conv.in_channels == 128 and mine.model[8].cv3.conv.out_channels == 256       # 512 and 1024 at width 0.25
    names = [n for n, _ in mine.named_parameters()]
    assert 'model.6.2.m.0.conv_h.bias' in names and 'model.2.m.0.bn1.weight' in names and 'model.6.1.m.0.cv2.conv.weight' in names
    assert names == [n for n, _ in ref.named_parameters()]
    cfg = yolov5_ca_cfg(0.5, 1.0, nc=10)                          # depth 1.0: rows of 3, 6, 9 and 3 blocks
    assert [len(m) for m in Model(cfg).model if isinstance(m, MB.Repeat)] == [3, 6, 9, 3]


def test_repeated_c3_ca_that_changes_width_is_refused():
    from somi_amd.configs import yolov5_ca_cfg
    from somi_amd.model import Model
    cfg = yolov5_ca_cfg(0.25, 0.33, nc=10)
    cfg['backbone'][4][3] = [512]                                 # 64 -> 128 channels, two blocks in a row
    with pytest.raises(NotImplementedError, match='2 repeats of C3_CA from 64 to 128'):
        Model(cfg)
    cfg['backbone'][4][1] = 1                                     # one block may change the width
    cfg['backbone'][5][3] = [512, 3, 2]
    Model(cfg)
    cfg = yolov5_ca_cfg(0.25, 0.33, nc=10)
    cfg['backbone'][8][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


@pytest.mark.parametrize('where', ['c3', 'row'])
def test_ca_graph_matches_the_oracle(where, monkeypatch):
    from somi_amd.configs import yolov5_ca_cfg, yolov5_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov5_ca_cfg(0.25, 0.33, nc=10, where=where)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    bns = [m for m in mine.modules() if isinstance(m, nn.BatchNorm2d)]
    assert all(m.eps == 1e-3 and m.momentum == 0.03 for m in bns) and any(n.endswith('bn1') for n, _ in mine.named_modules())
    mine.load_state_dict(ref.state_dict())
    assert mine.fuse() is mine
    base = yolov5_cfg(0.25, 0.33, nc=10)
    if where == 'row':
        assert cfg['backbone'][:10] == base['backbone'] and cfg['backbone'][10] == [-1, 1, 'CoorAttention', [1024]]
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 15], [-1, 11], [18, 21, 24]]
        assert type(mine.model[10]).__name__ == 'CoorAttention' and mine.model[10].conv1.in_channels == 256
    else:
        assert cfg['head'] == base['head'] and [r[2] for r in cfg['backbone']].count('C3_CA') == 4
        assert [r[:2] + r[3:] for r in cfg['backbone']] == [r[:2] + r[3:] for r in base['backbone']]


def test_cfg_defaults_and_the_other_cfgs_are_unchanged():
    from somi_amd.configs import COCO_ANCHORS, yolov5_ca_cfg, yolov5_cfg
    cfg = yolov5_ca_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert [r[2] for r in cfg['backbone']] == ['Conv', 'Conv', 'C3_CA', 'Conv', 'C3_CA', 'Conv', 'C3_CA', 'Conv', 'C3_CA', 'SPPF']
    assert all(r[2] != 'C3_CA' and r[2] != 'CoorAttention' for r in yolov5_cfg()['backbone'] + yolov5_cfg()['head'])
    with pytest.raises(ValueError, match="'c3' or 'row'"):
        yolov5_ca_cfg(where='neck')


def test_optimizer_groups_follow_the_reference():
    """train.py:125-133: bn1.weight without decay, the three conv weights decayed, conv1 / conv_h / conv_w and bn1 biases in the bias group."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    for mk in R.BLOCKS.values():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert sorted(g0 + g1 + g2) == sorted(names.values()), 'a parameter is in no group'
        assert [n for n in g0 if 'bn1' in n] == [n for n in names.values() if n.endswith('bn1.weight')] != []
        for leaf in ('conv1.bias', 'conv_h.bias', 'conv_w.bias', 'bn1.bias'):
            assert any(n.endswith(leaf) for n in g2) and not any(n.endswith(leaf) for n in g0 + g1)
        for leaf in ('conv1.weight', 'conv_h.weight', 'conv_w.weight'):
            assert any(n.endswith(leaf) for n in g1) and not any(n.endswith(leaf) for n in g0 + g2)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]


def _bars(ref, ref64, rel, atol):
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    return worst


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_block_cases_are_ones_the_fp32_oracle_can_be_judged_on(tag):
    """The seeded block cases of test_coordatt_gpu: no bn1 output of the fp64 oracle lies within 1e-2 of one of h-swish's kinks - fifty times the
    distance between two correct fp32 training forwards (1e-4 .. 2e-4) -, and the fp32 CPU oracle's parameter gradients meet
    parity.grads_close's bar (1e-3 * scale + 2e-5) against its own fp64 twin."""
    ref, x, gen = R.block_case(tag)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    with R.kink_margin(ref64) as km:
        y64 = ref64(x.double())
    y = ref(x)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    y64.backward(dy.double())
    worst = _bars(ref, ref64, 1e-3, 2e-5)
    print(f'{tag}: kink margin {km.value:.3e}, fp32 oracle against fp64 at {worst:.3f} x the bar')
    assert km.value >= 1e-2, f'{tag}: a bn1 output of the fp64 oracle lies {km.value:.2e} from a kink'
    assert worst <= 1.0, f'{tag}: the fp32 oracle is {worst:.2f} x the bar away from fp64'


@pytest.mark.parametrize('where', ['c3', 'row'])
def test_graph_cases_are_ones_the_fp32_oracle_can_be_judged_on(where, monkeypatch):
    """The graph cases of test_coordatt_gpu (coordatt_ref.graph_case): the fp32 CPU oracle's parameter gradients meet check_train_step's bar
    (2e-3 * scale + 2e-6) against its own fp64 twin's, and no bn1 output of the fp64 oracle lies within 1e-2 of a kink - fifty times the
    distance between two correct fp32 training forwards (1e-4 .. 2e-4)."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(monkeypatch)
    _, ref, imgs, targets = R.graph_case(where)
    ref64 = copy.deepcopy(ref).double()
    ref.train(), ref64.train()
    with R.kink_margin(ref64) as km:
        out64 = ref64(imgs.double() / 255)
    OLoss(ref64)(out64, targets.double())[0].backward()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    worst = _bars(ref, ref64, 2e-3, 2e-6)
    print(f'{where}: kink margin {km.value:.3e}, fp32 oracle against fp64 at {worst:.3f} x the bar')
    assert km.value >= 1e-2, f'{where}: a bn1 output of the fp64 oracle lies {km.value:.2e} from a kink'
    assert worst <= 1.0, f'{where}: the fp32 oracle is {worst:.2f} x the bar away from fp64 on the graph case'


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
    assert 'SOMI_ACT_HSWISH = 6' in hdr and 'SOMI_ACT_LEAKY = 5' in hdr
    assert '#define SOMI_ABI_VERSION 15' in hdr and _lib.lib().somi_abi_version() == _lib.ABI_VERSION == 15
    assert _lib.lib().somi_coordatt_desc_bytes() == ctypes.sizeof(_lib.CoordAttDesc)
    assert ops.ACT['hswish'] == 6 and ops.ACT['leaky'] == 5
    for fn in ('coordatt_means', 'coordatt_apply', 'coordatt_backward_gates', 'coordatt_backward_input'):
        assert callable(getattr(ops, fn))
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'coordatt.hip' in mk


def _desc(_lib):
    d = _lib.CoordAttDesc()
    d.x, d.y, d.res, d.pool = _lib.Slice(0x10000, 16, 4), _lib.Slice(0x20000, 16, 4), _lib.Slice(0x30000, 16, 4), _lib.Slice(0x40000, 16, 4)
    d.a_h, d.a_w, d.r_h, d.r_w = _lib.Slice(0x50000, 24, 4), _lib.Slice(0x60000, 24, 4), _lib.Slice(0x70000, 24, 4), _lib.Slice(0x80000, 24, 4)
    d.dx = _lib.Slice(0x90000, 16, 4)
    d.a_h_rows, d.a_w_rows, d.r_h_rows, d.r_w_rows = 4, 6, 10, 10
    d.B, d.H, d.W, d.C = 1, 4, 6, 8
    d.workspace, d.workspace_floats = 0xA0000, 1 << 30
    return d


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_new_entry_points_check_their_slices_without_a_launch():
    """The slice rule at the four entry points: every slice an entry point reads or writes, broken in six ways, is SOMI_EINVAL with a message
    that names it; a rejected call launches nothing, so the made-up addresses are never touched.  Other argument errors likewise."""
    from somi_amd import _lib
    L = _lib.lib()
    entries = {'means': (L.somi_coordatt_means_nhwc_f32, {'x': 'x', 'pool': 'pool'}),
               'apply': (L.somi_coordatt_apply_nhwc_f32, {'x': 'x', 'y': 'out', 'res': 'res', 'a_h': 'a_h', 'a_w': 'a_w'}),
               'gates': (L.somi_coordatt_bwd_gates_nhwc_f32, {'x': 'x', 'y': 'dout', 'a_h': 'a_h', 'a_w': 'a_w', 'r_h': 'da_h', 'r_w': 'da_w'}),
               'input': (L.somi_coordatt_bwd_input_nhwc_f32, {'y': 'dout', 'a_h': 'a_h', 'a_w': 'a_w', 'r_h': 'gh', 'r_w': 'gw', 'dx': 'dx'})}
    for key, (fn, fields) in entries.items():
        for field, name in fields.items():
            for what, brk in BREAKS:
                if what == 'pointer NULL' and name == 'res':
                    continue                                      # the optional slice: NULL means no shortcut
                d = _desc(_lib)
                brk(getattr(d, field))
                assert fn(ctypes.byref(d), None) == -1, f'{key}: {name}: {what} is let through'
                assert re.search(r'\b%s = \[' % name, L.somi_last_error().decode()), f'{key}: {name}: {what}: {L.somi_last_error()}'
        for attr, value in (('C', 6), ('C', 0), ('H', 0), ('B', -1)):
            d = _desc(_lib)
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and b'bad sizes' in L.somi_last_error(), f'{key}: {attr} = {value}'
        assert fn(None, None) == -1
    for key in ('apply', 'gates', 'input'):
        d = _desc(_lib)
        d.a_w_rows = 5
        assert entries[key][0](ctypes.byref(d), None) == -1 and b'a_w at least W' in L.somi_last_error()
    for key, word in (('gates', b'da_h'), ('input', b'gh')):
        d = _desc(_lib)
        d.r_h_rows = 3
        assert entries[key][0](ctypes.byref(d), None) == -1 and word in L.somi_last_error()
    for key in ('means', 'gates'):
        need = L.somi_coordatt_workspace_floats(1, 4, 6, 8)
        d = _desc(_lib)
        d.workspace_floats = need - 1
        assert entries[key][0](ctypes.byref(d), None) == -3, f'{key}: a short workspace is let through'
        d = _desc(_lib)
        d.workspace = None
        assert entries[key][0](ctypes.byref(d), None) == -1
        d = _desc(_lib)
        d.workspace += 4
        assert entries[key][0](ctypes.byref(d), None) == -1


def test_workspace_size_is_host_arithmetic():
    """Row partials B * H * ceil(W / NL) * C plus column partials B * ceil(H / RH) * W * C floats, NL = 256 / min(C / 4, 256) columns and RH rows
    per workgroup, RH halved from 32 (not below 4) while fewer than 1024 workgroups exist."""
    from somi_amd import _lib
    L = _lib.lib()
    assert L.somi_coordatt_workspace_floats(1, 4, 6, 8) == (4 * 1 + 1 * 6) * 8                    # NL 128, RH 4
    assert L.somi_coordatt_workspace_floats(1, 3, 130, 8) == (3 * 2 + 1 * 130) * 8                # two column chunks
    assert L.somi_coordatt_workspace_floats(1, 130, 3, 8) == (130 * 1 + 33 * 3) * 8               # 33 row chunks of 4
    assert L.somi_coordatt_workspace_floats(32, 160, 160, 32) == 32 * (160 * 5 + 10 * 160) * 32    # NL 32, RH 16
    assert L.somi_coordatt_workspace_floats(64, 160, 160, 32) == 64 * (160 * 5 + 5 * 160) * 32     # enough workgroups at RH 32
    assert L.somi_coordatt_workspace_floats(1, 4, 4, 2048) == (4 * 4 + 1 * 4) * 2048              # C / 4 > 256: one column per workgroup
    assert L.somi_coordatt_workspace_floats(1, 4, 4, 6) == 0 and L.somi_coordatt_workspace_floats(0, 4, 4, 8) == 0
