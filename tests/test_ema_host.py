"""CPU checks of efficient multi-scale attention (EMA, models/common.py:5263-5292; iRMB_EMA, iRMB_EMABottleneck and C2f_iRMB_EMA, :5409-5497):
the test restatement (tests/ema_ref.py) reproduces the reference's own classes through the tests/golden/block_ema*.npz fixtures; the parser
builds the four names from the yaml arguments as written, as the reference's generic branch does, and refuses what that branch would get wrong;
state-dict keys, optimizer groups and parameter counts are the oracle's; mean(x1) = gn.bias holds in fp64; the seeded cases of the GPU tests
are ones a plain fp32 computation meets half the bar on; and the new entry points are declared, bound, exported and refuse what they say."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import ema_ref as R
from support_kernels_ref import POINT, REDUCED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_ema_stats_nhwc_f32', 'somi_ema_gate_nhwc_f32', 'somi_ema_bwd_gate_nhwc_f32', 'somi_ema_bwd_norm_nhwc_f32',
               'somi_ema_workspace_floats', 'somi_ema_partials', 'somi_ema_desc_bytes')

FIXTURES = {'block_ema32': 'ema32', 'block_ema16_f4': 'ema16_f4', 'block_ema_irmb32': 'irmb32', 'block_ema_bottleneck32': 'bottleneck32',
            'block_ema_c2f32': 'c2f32', 'block_ema_c2f64_n2': 'c2f64_n2'}

# which results of ema_ref.kernel_reference are sums over pixels (REDUCED) and which pointwise (POINT): the bars of test_ema_gpu
KERNEL_BARS = dict(stats=REDUCED, vec=REDUCED, out=POINT, out_res=POINT, dx=POINT, dw=POINT, sums=REDUCED, dt=POINT, dx2=POINT, dsg=REDUCED,
                   dgamma=REDUCED, dbeta=REDUCED, dx_total=POINT)


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_restatement_reproduces_the_reference(name):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    make, shape = R.BLOCKS[FIXTURES[name]]
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == shape
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        err = (y - want).abs().max().item()
        assert y.shape == want.shape and err <= 1e-5 * want.abs().max().item(), f'{name} {mode}: {err:.3e}'


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    for tag, (mk, _) in R.BLOCKS.items():
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict()), tag
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())
    assert list(MB.EMA(32).state_dict()) == ['gn.weight', 'gn.bias', 'conv1x1.weight', 'conv1x1.bias', 'conv3x3.weight', 'conv3x3.bias']
    assert MB.EMA(32).conv3x3.weight.shape == (4, 4, 3, 3) and MB.EMA(16, 4).gn.num_groups == 4 and MB.EMA(32).gn.eps == 1e-5
    irmb = MB.iRMB_EMA(32)
    assert [n for n, _ in irmb.named_children()] == ['norm', 'ema', 'conv_local', 'proj']
    assert list(irmb.state_dict()) == (['norm.' + k for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')] +
                                       ['ema.' + k for k in MB.EMA(32).state_dict()] + ['conv_local.conv.weight'] +
                                       ['conv_local.norm.' + k for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')] +
                                       ['proj.conv.weight'])
    assert irmb.conv_local.conv.groups == 32 and irmb.conv_local.bn is irmb.conv_local.norm and irmb.proj.conv.bias is None
    assert [n for n, _ in MB.iRMB_EMABottleneck(32, 32).named_children()] == ['cv1', 'cv2', 'iRMB']
    blk = MB.C2f_iRMB_EMA(64, 64, 2, True)
    assert [n for n, _ in blk.named_children()] == ['cv1', 'cv2', 'm'] and len(blk.m) == 2
    assert all(type(m) is MB.iRMB_EMABottleneck and m.add and m.cv1.conv.kernel_size == (3, 3) and m.cv1.conv.out_channels == 32 for m in blk.m)


def test_contract_and_limits_are_explicit():
    import inspect
    from somi_amd import blocks as MB
    for cls in (MB.EMA, MB.iRMB_EMA, MB.iRMB_EMABottleneck, MB.C2f_iRMB_EMA):      # declared on the class itself, not inherited
        assert (cls.__dict__['accumulates'], cls.__dict__['folds_pooled'], cls.__dict__['reduction']) == (False, False, 1), cls.__name__
        assert list(inspect.signature(cls.backward).parameters)[2:5] == ['dx_out', 'accumulate', 'need_dx'], cls.__name__
    assert issubclass(MB.C2f_iRMB_EMA, MB.C2f) and MB.C2f.accumulates is True
    for kw in (dict(attn_s=False), dict(exp_ratio=2.0), dict(se_ratio=0.25), dict(drop=0.1), dict(drop_path=0.1), dict(norm_layer='ln_2d'),
               dict(dw_ks=5), dict(stride=2), dict(norm_in=False), dict(has_skip=False), dict(dilation=2)):
        with pytest.raises(NotImplementedError, match="only the reference's defaults"):
            MB.iRMB_EMA(32, **kw)
    MB.iRMB_EMA(32, act_layer='silu', v_proj=False, qkv_bias=True)          # unused with attn_s=True, in the reference too
    act = lambda c, cs=None: MB.Act(torch.zeros(1, 4, 4, cs or c), 0, c)    # noqa: E731
    with pytest.raises(NotImplementedError, match='channels % factor == 0'):
        MB.EMA(36).eval()(act(36))                                 # 36 % 8 != 0
    with pytest.raises(NotImplementedError, match='2 channels per group'):
        MB.EMA(16).eval()(act(16))                                 # cg = 2
    with pytest.raises(NotImplementedError, match='128 channels per group'):
        MB.EMA(1024).eval()(act(1024))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.EMA(32).eval()(act(32))


def test_parser_builds_the_four_names_from_the_arguments_as_written(monkeypatch):
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_ema_cfg
    from somi_amd.model import Model, _CH, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert not {'EMA', 'iRMB_EMA', 'iRMB_EMABottleneck', 'C2f_iRMB_EMA'} & (set(_CH) | set(_REPEAT_INSIDE))
    cfg = yolov5_ema_cfg(0.5, 0.33, nc=10)
    mine, ref = Model(cfg), R.oracle_model(cfg)
    assert [type(mine.model[i]).__name__ for i in (2, 4, 6, 8)] == ['C2f_iRMB_EMA'] * 4
    assert [len(mine.model[i].m) for i in (2, 4, 6, 8)] == [1, 2, 3, 1] and [mine.model[i].c for i in (2, 4, 6, 8)] == [32, 64, 128, 256]
    assert all(m.add for i in (2, 4, 6, 8) for m in mine.model[i].m)
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert 'model.6.m.2.iRMB.ema.gn.weight' in dict(mine.named_parameters())
    # iRMB_EMA and iRMB_EMABottleneck as rows of their own
    cfg = yolov5_ema_cfg(0.5, 0.33, nc=10, where='row')
    cfg['backbone'][10] = [-1, 1, 'iRMB_EMA', [512]]
    assert type(Model(cfg).model[10]) is MB.iRMB_EMA
    cfg['backbone'][10] = [-1, 1, 'iRMB_EMABottleneck', [512, 512, False]]
    m = Model(cfg).model[10]
    assert type(m) is MB.iRMB_EMABottleneck and not m.add and m.cv1.conv.out_channels == 256


def test_parser_refusals_cite_the_reference():
    from somi_amd.configs import yolov5_ema_cfg
    from somi_amd.model import Model
    cfg = yolov5_ema_cfg(0.5, 0.33, nc=10, where='row')
    assert cfg['backbone'][10] == [-1, 1, 'EMA', [512]]
    cfg['backbone'][10][3] = [1024]                                # the unscaled width: the generic branch scales nothing
    with pytest.raises(ValueError, match=r"'EMA' row that names \[1024\] channels behind 512.*models/yolo.py:1648-1650"):
        Model(cfg)
    for name, args in (('C2f_iRMB_EMA', [512, 256, 1]), ('C2f_iRMB_EMA', [256, 512, 1]), ('iRMB_EMABottleneck', [512, 256]),
                       ('iRMB_EMABottleneck', [256, 512]), ('iRMB_EMA', [256]), ('C2f_iRMB_EMA', [512])):
        cfg['backbone'][10] = [-1, 1, name, args]
        with pytest.raises(ValueError, match=r'models/yolo.py:1648-1650'):
            Model(cfg)
    cfg = yolov5_ema_cfg(0.5, 1.0, nc=10, where='row')
    cfg['backbone'][10][1] = 2                                     # n > 1 would be an nn.Sequential of whole modules: refused as for every such module
    with pytest.raises(NotImplementedError, match="2 repeats of 'EMA'"):
        Model(cfg)
    cfg = yolov5_ema_cfg(0.5, 0.33, nc=10)
    cfg['backbone'][8][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)
    cfg['backbone'][8][2] = 'C2fEMACBAM'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


@pytest.mark.parametrize('where', ['c2f', 'row'])
def test_ema_graph_matches_the_oracle(where, monkeypatch):
    """State dict, parameter count, strides and save list are the oracle Model's; the oracle's forward runs on both configs and the restated
    blocks inside it are the ones the fixtures pin."""
    from somi_amd.configs import yolov5_cfg, yolov5_ema_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov5_ema_cfg(0.5, 0.33, nc=10, where=where)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    bns = [m for m in mine.modules() if isinstance(m, nn.BatchNorm2d)]
    assert all(m.eps == 1e-3 and m.momentum == 0.03 for m in bns)
    assert all(m.eps == 1e-3 and m.momentum == 0.03 for m in ref.modules() if isinstance(m, nn.BatchNorm2d))
    assert all(m.eps == 1e-5 for m in mine.modules() if isinstance(m, nn.GroupNorm))
    mine.load_state_dict(ref.state_dict())
    assert mine.fuse() is mine
    with torch.no_grad():
        z, raw = ref.eval()(torch.rand(1, 3, 64, 64))
    assert z.shape == (1, 3 * (64 + 16 + 4), 15) and len(raw) == 3 and torch.isfinite(z).all()
    base = yolov5_cfg(0.5, 0.33, nc=10)
    if where == 'row':
        assert cfg['backbone'][:10] == base['backbone'] and cfg['backbone'][10] == [-1, 1, 'EMA', [512]]
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 15], [-1, 11], [18, 21, 24]]
        assert type(mine.model[10]).__name__ == 'EMA' and mine.model[10].conv3x3.in_channels == 64
    else:
        assert cfg['head'] == base['head']
        assert [r for r in cfg['backbone'] if r[2] == 'C2f_iRMB_EMA'] == [[-1, 1, 'C2f_iRMB_EMA', [c, c, n, True]]
                                                                          for c, n in ((64, 1), (128, 2), (256, 3), (512, 1))]


def test_cfg_defaults_and_the_other_cfgs_are_unchanged():
    from somi_amd.configs import COCO_ANCHORS, yolov5_cfg, yolov5_ema_cfg
    cfg = yolov5_ema_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert [r[2] for r in cfg['backbone']] == ['Conv', 'Conv', 'C2f_iRMB_EMA', 'Conv', 'C2f_iRMB_EMA', 'Conv', 'C2f_iRMB_EMA', 'Conv',
                                               'C2f_iRMB_EMA', 'SPPF']
    assert not any('EMA' in r[2] for r in yolov5_cfg()['backbone'] + yolov5_cfg()['head'])
    with pytest.raises(ValueError, match="'c2f' or 'row'"):
        yolov5_ema_cfg(where='neck')


def test_optimizer_groups_follow_the_reference():
    """train.py:125-133: gn.weight is NOT a BatchNorm2d weight, so it is decayed; gn.bias and the two conv biases are in the bias group; the two
    BatchNorm weights of iRMB_EMA are in the no-decay group."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    for tag, (mk, _) in R.BLOCKS.items():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert sorted(g0 + g1 + g2) == sorted(names.values()), 'a parameter is in no group'
        assert any(n.endswith('gn.weight') for n in g1) and not any(n.endswith('gn.weight') for n in g0 + g2), tag
        for leaf in ('gn.bias', 'conv1x1.bias', 'conv3x3.bias'):
            assert any(n.endswith(leaf) for n in g2) and not any(n.endswith(leaf) for n in g0 + g1), (tag, leaf)
        for leaf in ('conv1x1.weight', 'conv3x3.weight'):
            assert any(n.endswith(leaf) for n in g1) and not any(n.endswith(leaf) for n in g0 + g2), (tag, leaf)
        if tag.startswith(('irmb', 'bottleneck', 'c2f')):
            assert [n for n in g0 if 'iRMB' in n or tag.startswith('irmb')] and all(n.endswith(('norm.weight', 'bn.weight')) for n in g0)
            assert any(n.endswith('proj.conv.weight') for n in g1) and any(n.endswith('conv_local.conv.weight') for n in g1)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]


def test_mean_of_x1_is_the_bias_in_fp64():
    """agp(x1) = gn.bias: the mean of a normalised map is its shift, so softmax(agp(x1)) does not depend on the input (2e-16 in fp64), and
    kernel_forward(literal=False), which the kernels follow, gives the literal formula's output."""
    for shape in R.KERNEL_SHAPES[:4]:
        t = R.kernel_inputs(shape)
        lit, idn = R.kernel_forward(t, shape[4], literal=True), R.kernel_forward(t, shape[4], literal=False)
        assert (lit['x1'].mean((1, 2)) - t['beta'].double().repeat(shape[4])).abs().max().item() <= 1e-14
        assert (lit['x11'] - idn['x11']).abs().max().item() <= 1e-14 and (lit['out'] - idn['out']).abs().max().item() <= 1e-13
    mod = R.block_case('ema32')[0].double()
    seen = []
    h = mod.gn.register_forward_hook(lambda m, i, o: seen.append(o.mean((2, 3))))
    mod(torch.randn(2, 32, 5, 7, dtype=torch.float64))
    h.remove()
    assert (seen[0] - mod.gn.bias).abs().max().item() <= 1e-14


@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=lambda c: 'x'.join(map(str, c[0])) + '-' + c[1])
def test_kernel_cases_are_ones_fp32_meets_half_the_bar_on(case):
    """Every case of test_ema_gpu's kernel tests: the same formulas in fp32 on the CPU meet HALF the bar the GPU test applies (POINT for pointwise
    results, REDUCED for sums over pixels) against fp64."""
    shape, kind = case
    t = R.kernel_inputs(shape, kind)
    want, got = R.kernel_reference(t, shape[4]), R.kernel_reference(t, shape[4], torch.float32)
    worst = {}
    for k, bar in KERNEL_BARS.items():
        scale = want[k].abs().max().item() + 1e-12
        worst[k] = (got[k].double() - want[k]).abs().max().item() / (bar * scale)
    print(f'{case}: fp32 against fp64 in units of the bar: ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))
    bad = {k: round(v, 3) for k, v in worst.items() if not v <= 0.5}
    assert not bad, f'{case}: the fp32 reference is beyond half the bar in {bad}'
    if kind == 'pooled50':
        assert want['stats'][:, 2].abs().max().item() > 40 and torch.isfinite(got['out']).all()
    if kind == 'mean30':
        assert (want['stats'][:, 0].abs() / torch.sqrt(want['stats'][:, 1] / (shape[1] * shape[2]))).median().item() > 20


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_block_cases_are_ones_the_fp32_oracle_can_be_judged_on(tag):
    """The seeded block cases of test_ema_gpu: the fp32 CPU restatement's parameter gradients meet HALF of parity.grads_close's bar
    (1e-3 * scale + 2e-5) against its own fp64 twin, its output and input gradient half of rel_close's 1e-3."""
    ref, x, gen = R.block_case(tag)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    y, y64 = ref(x32), ref64(x64)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    y64.backward(dy.double())
    worst = R.worst_grad_ratio(ref, ref64, 1e-3, 2e-5)
    eo = (y.double() - y64).abs().max().item() / y64.abs().max().item()
    ex = (x32.grad.double() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
    print(f'{tag}: out {eo:.1e}, dx {ex:.1e}, parameter gradients at {worst:.3f} x the bar')
    assert worst <= 0.5 and eo <= 5e-4 and ex <= 5e-4, f'{tag}: the fp32 oracle is {worst:.2f} x the bar away from fp64 (out {eo:.1e}, dx {ex:.1e})'


@pytest.mark.parametrize('where', ['c2f', 'row'])
def test_graph_cases_are_ones_the_fp32_oracle_can_be_judged_on(where, monkeypatch):
    """The graph cases of test_ema_gpu (ema_ref.graph_case): the fp32 CPU oracle's parameter gradients meet HALF of check_train_step's bar
    (2e-3 * scale + 2e-6) against its own fp64 twin's."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(monkeypatch)
    _, ref, imgs, targets = R.graph_case(where)
    ref64 = copy.deepcopy(ref).double()
    ref.train(), ref64.train()
    OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    worst = R.worst_grad_ratio(ref, ref64, 2e-3, 2e-6)
    print(f'{where}: fp32 oracle against fp64 at {worst:.3f} x the bar')
    assert worst <= 0.5, f'{where}: the fp32 oracle is {worst:.2f} x the bar away from fp64 on the graph case'


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
    assert _lib.lib().somi_ema_desc_bytes() == ctypes.sizeof(_lib.EmaDesc)
    for fn in ('ema_stats', 'ema_gate', 'ema_backward_gate', 'ema_backward_norm', 'ema_partials'):
        assert callable(getattr(ops, fn))
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'ema.hip' in mk and 'ema' not in mk.split('ATOMIC_SRCS :=')[1].splitlines()[0].split()       # no -munsafe-fp-atomics
    src = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'ema.hip')).read()
    assert 'atomicAdd' not in src and 'atomic' not in src.replace('No float atomics', '')


def _desc(_lib, **kw):
    d = _lib.EmaDesc()
    for i, f in enumerate(('x', 'x2', 'sg', 'y', 'res', 'dx', 'dw', 'dsg')):
        setattr(d, f, _lib.Slice(0x10000 * (i + 1), 40, 4))
    for i, f in enumerate(('gamma', 'beta', 'stats', 'vec', 'sums', 'bvec', 'dgamma', 'dbeta')):
        setattr(d, f, 0x100000 * (i + 1))
    d.B, d.H, d.W, d.C, d.factor, d.eps = 1, 4, 6, 32, 8, 1e-5
    d.workspace, d.workspace_floats = 0xA00000, 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_new_entry_points_refuse_without_a_launch():
    """The slice rule at the four entry points (SOMI_EINVAL with a message that names the slice), the refusals the header lists
    (SOMI_ENOTIMPL), the workspace checks; a rejected call launches nothing, so the made-up addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    entries = {'stats': (L.somi_ema_stats_nhwc_f32, {'x': 'x', 'sg': 'sg', 'x2': 'x2'}),
               'gate': (L.somi_ema_gate_nhwc_f32, {'x': 'x', 'sg': 'sg', 'x2': 'x2', 'y': 'out', 'res': 'res'}),
               'bwd gate': (L.somi_ema_bwd_gate_nhwc_f32, {'x': 'x', 'sg': 'sg', 'x2': 'x2', 'y': 'dout', 'dx': 'dx', 'dw': 'dw'}),
               'bwd norm': (L.somi_ema_bwd_norm_nhwc_f32, {'x': 'x', 'sg': 'sg', 'dw': 'dw', 'y': 'dt', 'dsg': 'dsg'})}
    for key, (fn, fields) in entries.items():
        for field, name in fields.items():
            for what, brk in BREAKS:
                if what == 'pointer NULL' and (name == 'res' or (key == 'stats' and name == 'x2')):
                    continue                                      # the optional slices
                d = _desc(_lib)
                brk(getattr(d, field))
                assert fn(ctypes.byref(d), None) == -1, f'{key}: {name}: {what} is let through'
                assert re.search(r'\b%s = \[' % name, L.somi_last_error().decode()), f'{key}: {name}: {what}: {L.somi_last_error()}'
        for kw, word in ((dict(C=36), b'do not divide'), (dict(C=16), b'a multiple of 4 is needed'), (dict(C=1024), b'at most 64'),
                         (dict(C=40, factor=4), b'a multiple of 4 is needed'), (dict(B=1 << 14, H=1 << 8, W=1 << 8), b'2^30 floats')):
            assert fn(ctypes.byref(_desc(_lib, **kw)), None) == -2 and word in L.somi_last_error(), f'{key}: {kw}: {L.somi_last_error()}'
        for kw in (dict(C=0), dict(H=0), dict(B=-1), dict(factor=0)):
            assert fn(ctypes.byref(_desc(_lib, **kw)), None) == -1 and b'bad sizes' in L.somi_last_error(), f'{key}: {kw}'
        assert fn(None, None) == -1
        if key != 'gate':
            need = L.somi_ema_workspace_floats(1, 4, 6, 32)
            assert fn(ctypes.byref(_desc(_lib, workspace_floats=need - 1)), None) == -3, f'{key}: a short workspace is let through'
            assert fn(ctypes.byref(_desc(_lib, workspace=None)), None) == -1
            assert fn(ctypes.byref(_desc(_lib, workspace=0xA00004)), None) == -1


def test_plan_is_host_arithmetic():
    """Partials per (b, c): ceil(H / RH) * ceil(W / NL) with NL = 256 / min(C / 4, 256) columns and RH rows per workgroup, RH halved from 32 (not
    below 4) while fewer than 1024 workgroups exist.  The smallest map with two partials has H = 5; the workspace holds three sums per partial,
    or the row and column partials of the norm backward, whichever is larger."""
    from somi_amd import ops
    L = ops._lib.lib()
    assert [ops.ema_partials(2, h, 7, 32) for h in (1, 4, 5, 8, 9)] == [1, 1, 2, 2, 3]
    assert ops.ema_partials(1, 1, 1, 32) == 1 and ops.ema_partials(2, 1, 3, 32) == 1
    assert ops.ema_partials(1, 5, 7, 256) == 2 * 2                  # NL = 4: two column chunks
    assert ops.ema_partials(1, 9, 70, 16) == 3 * 2                  # NL = 64
    assert ops.ema_partials(32, 160, 160, 32) == 10 * 5 and ops.ema_partials(64, 160, 160, 32) == 5 * 5
    assert ops.ema_partials(1, 4, 4, 6) == 0 and ops.ema_partials(0, 4, 4, 8) == 0
    assert L.somi_ema_workspace_floats(2, 5, 7, 32) == max(2 * 2 * 3 * 32, (2 * 5 * 1 + 2 * 2 * 7) * 32)
    assert L.somi_ema_workspace_floats(32, 160, 160, 32) == max(32 * 50 * 3 * 32, 32 * (160 * 5 + 10 * 160) * 32)
    assert L.somi_ema_workspace_floats(1, 4, 4, 6) == 0
