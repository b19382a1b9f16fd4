"""CPU checks of the ASFF head (ASFF_Detect, models/yolo.py:172-184; ASFF and add_conv, models/common.py:5500-5567, 5322-5343): the test
restatement (tests/asff_ref.py) reproduces the reference's own classes through the tests/golden/block_asff*.npz fixtures - the head's fixture
pins the chain the reference forms by rewriting its input list in place -, the product graph is built like the oracle's (state-dict keys and
shapes, strides, bias init, BatchNorm hyperparameters), the limits of the MI355X path are explicit, and the new entry points are declared, bound,
exported and check their slices."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import asff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_asff_fuse_nhwc_f32', 'somi_asff_fuse_bwd_nhwc_f32', 'somi_asff_fuse_bwd_workspace_floats', 'somi_asff_desc_bytes', 'somi_maxpool3s2_nhwc_f32',
               'somi_maxpool3s2_bwd_nhwc_f32')


def _close(got, want, what):
    err = (got - want).abs().max().item()
    assert got.shape == want.shape and err <= 1e-5 * want.abs().max().item(), f'{what}: {err:.3e}'


@pytest.mark.parametrize('level', [0, 1, 2])
def test_restatement_reproduces_the_reference_asff(level):
    """Eval and train outputs of the reference's ASFF(level) under fill_state weights, fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_asff{level}.npz'))
    mod = fill_state(R.ASFF(level), 0)
    OB.initialize_weights(mod)
    xs = [torch.from_numpy(d[f'in{i}']) for i in range(3)]
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(*(x.clone() for x in xs))
        _close(y, torch.from_numpy(d[f'out_{mode}']), f'asff{level} {mode}')


def test_restatement_reproduces_the_reference_head_chain_quirk_included():
    """ASFF_Detect on [P3, P4, P5]: z and the raws in eval, the raws in training.  A head that fused the ORIGINAL maps at every level (the chain
    'fixed') differs from the fixture by far more than the bar."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, 'block_asff_detect.npz'))
    anchors = torch.from_numpy(d['anchors'])
    head = fill_state(R.ASFF_Detect(3, anchors.view(3, -1).tolist(), (128, 256, 512)), 0)
    OB.initialize_weights(head)
    head.stride = torch.tensor(R.STRIDES)
    xs = [torch.from_numpy(d[f'in{i}']) for i in range(3)]
    head.eval()
    with torch.no_grad():
        z, raws = head([x.clone() for x in xs])
    _close(z, torch.from_numpy(d['z_eval']), 'z')
    for i, t in enumerate(raws):
        _close(t, torch.from_numpy(d[f'raw{i}_eval']), f'raw{i} eval')
    head.train()
    with torch.no_grad():
        raws = head([x.clone() for x in xs])
    for i, t in enumerate(raws):
        _close(t, torch.from_numpy(d[f'raw{i}_train']), f'raw{i} train')
    head.eval()
    with torch.no_grad():
        p3, p4, p5 = xs
        unchained = head.m[0](head.asffs[2](p5, p4, p3))          # level 2 from the original maps instead of (f0, f1, P3)
    want = torch.from_numpy(d['raw0_eval'])
    got = unchained.view(1, 3, 8, 8, 12).permute(0, 1, 3, 4, 2)
    assert (got - want).abs().max().item() > 1e-2 * want.abs().max().item(), 'the fixture does not tell the chain from its repaired form'


def test_asff_graph_matches_the_oracle():
    from somi_amd.configs import yolov5_cfg
    from somi_amd.model import Model
    cfg = yolov5_cfg(nc=10, head='ASFF_Detect')
    assert cfg['head'][-1] == [[17, 20, 23], 1, 'ASFF_Detect', ['nc', 'anchors']]
    assert yolov5_cfg(nc=10)['head'][-1][2] == 'Detect'           # the default is unchanged
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert 'model.24.asffs.2.weight_levels.bias' in got and 'model.24.asffs.0.stride_level_1.batch_norm.running_var' in got
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and mine.model[-1].type == 'ASFF_Detect'
    det = mine.model[-1]
    assert torch.equal(det.anchors, ref.model[-1].anchors)
    for conv, s in zip(det.m, (8, 16, 32)):                       # _initialize_biases ran: obj and cls priors on top of the small default init
        b = conv.bias.detach().view(det.na, -1)
        slack = 1.0 / math.sqrt(conv.in_channels) + 1e-6
        assert (b[:, 4] - math.log(8 / (640 / s) ** 2)).abs().max().item() <= slack
        assert (b[:, 5:] - math.log(0.6 / (10 - 0.999999))).abs().max().item() <= slack
    bns = [m for m in mine.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) > 60 and all(m.eps == 1e-3 and m.momentum == 0.03 for m in bns)
    mine.load_state_dict(ref.state_dict())


def test_graph_case_is_one_the_fp32_oracle_can_be_judged_on():
    """The graph case of test_asff_gpu (asff_ref.graph_case): the fp32 CPU oracle's parameter gradients stay within a quarter of
    check_train_step's bar (2e-3 * scale + 2e-6) of its own fp64 twin's - no pre-activation of a LeakyReLU close enough to zero for the two to
    take different sides of the kink (asff_ref.GRAPH_SEEDS has the figures of the seed pairs where they do)."""
    import copy
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    _, ref, imgs, targets = R.graph_case()
    ref64 = copy.deepcopy(ref).double()
    ref.train(), ref64.train()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
    worst = 0.0
    for (n, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (2e-3 * scale + 2e-6))
    print(f'fp32 oracle against fp64: worst parameter gradient at {worst:.3f} x the bar')
    assert worst <= 0.25, f'the fp32 oracle is {worst:.2f} x the bar away from fp64 on the graph case'


def test_add_conv_keeps_the_reference_layout_and_rides_conv():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    a, b = R.add_conv(16, 24, 3, 2), MB.add_conv(16, 24, 3, 2)
    assert list(a.state_dict()) == list(b.state_dict()) == ['conv.weight', 'batch_norm.weight', 'batch_norm.bias', 'batch_norm.running_mean',
                                                             'batch_norm.running_var', 'batch_norm.num_batches_tracked']
    b.load_state_dict(fill_state(a, 1).state_dict())
    assert isinstance(b, MB.Conv) and b.bn is b.batch_norm and b.act is b.leaky and b.conv.padding == (1, 1) and b.reduction == 2
    assert MB._act_name(b.act) == 'leaky'
    assert [len(g) for g in reference_param_groups(b)] == [len(g) for g in reference_param_groups(a)] == [1, 1, 1]
    for level in range(3):
        x, y = R.ASFF(level), MB.ASFF(level)
        assert list(x.state_dict()) == list(y.state_dict())
        assert {k: v.shape for k, v in x.state_dict().items()} == {k: v.shape for k, v in y.state_dict().items()}
        assert type(y.weight_levels) is nn.Conv2d and y.weight_levels.bias is not None


def test_asff_limits_are_explicit():
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cfg, yolov5_hub_cfg
    from somi_amd.model import Model
    with pytest.raises(NotImplementedError, match=r'three levels of \(128, 256, 512\) channels.*\[512, 256, 128\]'):
        cfg = yolov5_hub_cfg('p6', width=0.5, depth=0.33)         # four levels
        cfg['head'][-1][2] = 'ASFF_Detect'
        Model(cfg)
    with pytest.raises(NotImplementedError, match=r'three levels of \(128, 256, 512\) channels.*\[512, 256, 128\]'):
        Model(yolov5_cfg(0.25, 0.33, nc=10, head='ASFF_Detect'))  # levels of (64, 128, 256) channels
    with pytest.raises(NotImplementedError, match='rfb=True'):
        MB.ASFF(0, rfb=True)
    with pytest.raises(NotImplementedError, match='vis=True'):
        MB.ASFF(2, vis=True)
    with pytest.raises(NotImplementedError, match='ReLU6'):
        MB.add_conv(16, 16, 1, 1, leaky=False)
    with pytest.raises(NotImplementedError, match=r'LeakyReLU\(0.2\).*0.1 only'):
        MB._act_name(nn.LeakyReLU(0.2))
    with pytest.raises(ValueError, match='head must be one of'):
        yolov5_cfg(head='IDetect')
    cfg = yolov5_cfg(nc=10, head='ASFF_Detect')
    cfg['backbone'][8][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)
    for cls in (MB.ASFF, MB.ASFF_Detect):
        assert cls.accumulates is False and cls.folds_pooled is False and cls.reduction == 1


def test_invalidate_reaches_the_asff_children():
    from somi_amd import blocks as MB
    head = MB.ASFF_Detect(3, R.ANCHORS, (128, 256, 512))
    convs = [m for m in head.asffs.modules() if isinstance(m, MB.Conv)]
    assert len(convs) == 3 * 6
    for m in convs + head._runners:
        m.__dict__['_pk'] = 'stale'
    head.invalidate()
    assert not any('_pk' in m.__dict__ for m in convs + head._runners)


def test_new_symbols_are_declared_bound_and_exported():
    from somi_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/somi_hip.h'
        assert name in _lib.SIGNATURES, f'{name} is not bound in _lib.SIGNATURES'
        assert hasattr(L, name), f'{name} is not exported'
    assert 'SOMI_ACT_LEAKY = 5' in hdr and 'SOMI_ACT_SIGMOID = 4' in hdr
    assert '#define SOMI_ABI_VERSION 15' in hdr and _lib.lib().somi_abi_version() == _lib.ABI_VERSION == 15
    assert _lib.lib().somi_asff_desc_bytes() == ctypes.sizeof(_lib.AsffDesc)
    from somi_amd import ops
    assert ops.ACT['leaky'] == 5 and [ops.ACT[k] for k in ('none', 'silu', 'gelu', 'relu', 'sigmoid')] == [0, 1, 2, 3, 4]


def _asff_desc(_lib, bwd):
    d = _lib.AsffDesc()
    for i in range(3):
        d.r[i], d.v[i] = _lib.Slice(0x10000 * (i + 1), 16, 4), _lib.Slice(0x100000 * (i + 1), 24, 4)
        d.dr[i], d.dv[i] = _lib.Slice(0x20000 * (i + 1), 16, 4), _lib.Slice(0x200000 * (i + 1), 24, 4)
    d.w, d.bias, d.out, d.p = 0x1000, 0x2000, _lib.Slice(0x3000, 16, 4), 0x4000
    d.dw, d.db, d.workspace, d.workspace_floats = 0x5000, 0x6000, 0x7000, 1 << 30
    d.B, d.H, d.W, d.C = 1, 4, 4, 8
    return d


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_new_entry_points_check_their_slices_without_a_launch():
    """The slice rule at the entry points that take their slices as somi_slice values: every slice broken in six ways is SOMI_EINVAL with a message
    that names it; a rejected call launches nothing, so the made-up addresses are never touched.  Other argument errors likewise."""
    from somi_amd import _lib
    L = _lib.lib()
    assert L.somi_asff_fuse_bwd_workspace_floats(2, 8, 12) == 3 * 148 and L.somi_asff_fuse_bwd_workspace_floats(1, 1, 1) == 148
    optional = {'dr0', 'dr1', 'dr2'}
    for bwd, fn in ((False, L.somi_asff_fuse_nhwc_f32), (True, L.somi_asff_fuse_bwd_nhwc_f32)):
        fields = [('r', 3), ('v', 3), ('out', 0)] + ([('dr', 3), ('dv', 3)] if bwd else [])
        for field, n in fields:
            for i in range(max(n, 1)):
                name = f'{field}{i}' if n else ('dfused' if bwd else 'fused')
                for what, brk in BREAKS:
                    if what == 'pointer NULL' and name in optional:
                        continue
                    d = _asff_desc(_lib, bwd)
                    brk(getattr(d, field)[i] if n else getattr(d, field))
                    assert fn(ctypes.byref(d), None) == -1, f'{name}: {what} is let through'
                    assert re.search(r'\b%s = \[' % name, L.somi_last_error().decode()), f'{name}: {what}: {L.somi_last_error()}'
        d = _asff_desc(_lib, bwd)
        d.r_up[0] = 3
        assert fn(ctypes.byref(d), None) == -1 and b'up must be 0, 1 or 2' in L.somi_last_error()
        d = _asff_desc(_lib, bwd)
        d.v_up[1], d.H = 2, 6
        assert fn(ctypes.byref(d), None) == -1 and b'multiples of 4' in L.somi_last_error()
        d = _asff_desc(_lib, bwd)
        d.C = 6
        assert fn(ctypes.byref(d), None) == -1
    d = _asff_desc(_lib, True)
    d.workspace_floats = 147
    assert L.somi_asff_fuse_bwd_nhwc_f32(ctypes.byref(d), None) == -3
    mk = lambda: (_lib.Slice(0x10000, 16, 4), _lib.Slice(0x20000, 16, 4))     # noqa: E731
    for which, name_f, name_b in ((0, 'x', 'dy'), (1, 'y', 'dx')):
        for what, brk in BREAKS:
            a, b = mk()
            brk((a, b)[which])
            assert L.somi_maxpool3s2_nhwc_f32(ctypes.byref(a), ctypes.byref(b), None, 1, 4, 4, 8, None) == -1, what
            assert re.search(r'\b%s = \[' % name_f, L.somi_last_error().decode()), what
            a, b = mk()
            brk((a, b)[which])
            assert L.somi_maxpool3s2_bwd_nhwc_f32(ctypes.byref(a), 0x30000, ctypes.byref(b), 1, 4, 4, 8, None) == -1, what
            assert re.search(r'\b%s = \[' % name_b, L.somi_last_error().decode()), what
    a, b = mk()
    assert L.somi_maxpool3s2_bwd_nhwc_f32(ctypes.byref(a), None, ctypes.byref(b), 1, 4, 4, 8, None) == -1      # training codes are required
    assert L.somi_maxpool3s2_nhwc_f32(ctypes.byref(a), ctypes.byref(b), None, 1, 4, 4, 6, None) == -1
