"""CPU checks of ACmix (models/common.py:7281-7365): the test restatement (tests/acmix_ref.py) reproduces the reference's own class through the
tests/golden/block_acmix*.npz fixtures; state-dict keys, parameter names, initial values, optimizer groups and parameter counts are the
restatement's; the parser builds both yolov5_acmix_cfg graphs as the oracle does and refuses what it says; dep_conv(fc(.)) is one grouped conv and
the position term is two scalars per (pixel, head), both in fp64; the seeded cases of the GPU tests are ones a plain fp32 computation meets half
the bar on; and the new entry points are declared, bound, exported and refuse what they say without a launch."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import acmix_ref as R
from support_kernels_ref import POINT, REDUCED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_acmix_desc_bytes', 'somi_acmix_workspace_floats', 'somi_acmix_plan', 'somi_acmix_attn_nhwc_f32',
               'somi_acmix_attn_bwd_q_nhwc_f32', 'somi_acmix_attn_bwd_kv_nhwc_f32', 'somi_acmix_conv_nhwc_f32', 'somi_acmix_conv_bwd_data_nhwc_f32',
               'somi_acmix_conv_bwd_weight_nhwc_f32', 'somi_acmix_fold_weff_f32', 'somi_acmix_split_dweff_f32')
FIXTURES = {'block_acmix32': 'acmix32', 'block_acmix16to32': 'acmix16to32', 'block_acmix64_min': 'acmix64_min'}
KEYS = ['rate1', 'rate2', 'conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias', 'conv_p.weight', 'conv_p.bias',
        'fc.weight', 'dep_conv.weight']

# which results of acmix_ref.kernel_reference are sums over pixels (REDUCED) and which pointwise (POINT): the bars of test_acmix_gpu
KERNEL_BARS = dict(out=POINT, out_att=POINT, mix=POINT, lse=POINT, weff=POINT, dq=POINT, dk=POINT, dv=POINT, cq=POINT, ck=POINT, cv=POINT,
                   dwp=REDUCED, drate1=REDUCED, drate2=REDUCED, dweff=REDUCED, dfc=REDUCED, ddep=REDUCED, dbias=REDUCED)


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_restatement_reproduces_the_reference(name):
    """The reference's own class under fill_state(., 0), fp32, 1e-5 relative: with the rates fill_state draws and with both at 0.5."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    make, shape = R.BLOCKS[FIXTURES[name]]
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    mod.eval()
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == shape and torch.equal(x * 2, (x * 2).round())
    for key in ('out', 'out_half'):
        if key == 'out_half':
            with torch.no_grad():
                mod.rate1.fill_(0.5)
                mod.rate2.fill_(0.5)
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[key])
        err = (y - want).abs().max().item()
        assert y.shape == want.shape and err <= 1e-5 * want.abs().max().item(), f'{name} {key}: {err:.3e}'
    assert (torch.from_numpy(d['out']) - torch.from_numpy(d['out_half'])).abs().max().item() > 0.1


def test_block_keeps_the_reference_parameter_layout_and_initial_values():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    for tag, (mk, _) in R.BLOCKS.items():
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict()) == KEYS, tag
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()] == KEYS
        for k in ('rate1', 'rate2', 'dep_conv.weight'):           # reset_parameters, models/common.py:7313-7321
            assert torch.equal(a.state_dict()[k], b.state_dict()[k]), (tag, k)
        assert b.dep_conv.bias is None and a.dep_conv.bias is None   # the reference assigns the None its init_rate_0 helper returns
        b.load_state_dict(fill_state(a, 2).state_dict())
    m = MB.ACmix(16, 32)
    assert m.rate1.item() == m.rate2.item() == 0.5 and m.head_dim == 8 and m.dep_conv.groups == 8 and m.dep_conv.weight.shape == (32, 9, 3, 3)
    w = m.dep_conv.weight
    assert all(w[c, i, i // 3, i % 3] == 1 for c in (0, 31) for i in range(9)) and w.sum().item() == 32 * 9        # the shift kernel
    assert m.conv1.weight.shape == (32, 16, 1, 1) and m.conv_p.weight.shape == (8, 2, 1, 1) and m.fc.weight.shape == (9, 12, 1, 1)
    assert m.fc.bias is None and sum(p.numel() for p in m.parameters()) == sum(p.numel() for p in R.ACmix(16, 32).parameters())


def test_contract_and_limits_are_explicit():
    import inspect
    from somi_amd import blocks as MB
    cls = MB.ACmix                                                # declared on the class itself, not inherited
    assert (cls.__dict__['accumulates'], cls.__dict__['folds_pooled'], cls.__dict__['reduction']) == (False, False, 1)
    assert list(inspect.signature(cls.backward).parameters)[1:5] == ['dout', 'dx_out', 'accumulate', 'need_dx']
    assert list(inspect.signature(cls.__init__).parameters)[1:] == ['in_planes', 'out_planes', 'kernel_att', 'head', 'kernel_conv', 'stride',
                                                                    'dilation']
    for kw in (dict(kernel_att=5), dict(head=8), dict(kernel_conv=5), dict(stride=2), dict(dilation=2)):
        with pytest.raises(NotImplementedError, match=next(iter(kw)) + '='):
            MB.ACmix(32, 32, **kw)
    act = lambda c, h=4, w=4: MB.Act(torch.zeros(1, h, w, c), 0, c)    # noqa: E731
    with pytest.raises(NotImplementedError, match=r'out_planes % 16 == 0'):
        MB.ACmix(32, 24).eval()(act(32))
    with pytest.raises(NotImplementedError, match='at most 1024'):
        MB.ACmix(32, 2048).eval()(act(32))
    for h, w in ((3, 8), (8, 3)):                                 # the reference's ReflectionPad2d(3) raises there
        with pytest.raises(RuntimeError, match=r'Padding size should be less than the corresponding input dimension.*models/common.py:7302'):
            MB.ACmix(32, 32).eval()(act(32, h, w))
        with pytest.raises(RuntimeError, match='Padding size should be less than the corresponding input dimension'):
            R.ACmix(32, 32)(torch.zeros(1, 32, h, w))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.ACmix(32, 32).eval()(act(32))


@pytest.mark.parametrize('where', ['row', 'p3'])
def test_acmix_graph_matches_the_oracle(where, monkeypatch):
    """Names, state dict, parameter count, strides and save list at width 0.5 are the oracle Model's; Model places a blocks.ACmix."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_acmix_cfg, yolov5_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov5_acmix_cfg(0.5, 0.33, nc=10, where=where)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    mine.load_state_dict(ref.state_dict())
    with torch.no_grad():
        z, raw = ref.eval()(torch.rand(1, 3, 128, 128))
    assert z.shape == (1, 3 * (256 + 64 + 16), 15) and len(raw) == 3 and torch.isfinite(z).all()
    base = yolov5_cfg(0.5, 0.33, nc=10)
    if where == 'row':
        assert cfg['backbone'][:10] == base['backbone'] and cfg['backbone'][10] == [-1, 1, 'ACmix', [1024]]
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 15], [-1, 11], [18, 21, 24]]
        m = mine.model[10]
        assert type(m) is MB.ACmix and (m.in_planes, m.out_planes) == (512, 512)
    else:
        assert cfg['backbone'] == base['backbone'] and cfg['head'][8] == [-1, 1, 'ACmix', [256]]
        assert cfg['head'][:8] == base['head'][:8] and [r[1:] for r in cfg['head'][9:]] == [r[1:] for r in base['head'][8:]]
        assert [r[0] for r in cfg['head'] if isinstance(r[0], list)] == [[-1, 6], [-1, 4], [-1, 14], [-1, 10], [18, 21, 24]]
        m = mine.model[18]
        assert type(m) is MB.ACmix and (m.in_planes, m.out_planes) == (128, 128) and mine.model[19].f == -1


def test_parser_refusals_and_the_other_cfgs_are_unchanged():
    from somi_amd.configs import COCO_ANCHORS, yolov5_acmix_cfg, yolov5_cfg, yolov5_ema_cfg
    from somi_amd.model import Model
    cfg = yolov5_acmix_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert cfg['backbone'][10] == [-1, 1, 'ACmix', [1024]]
    with pytest.raises(ValueError, match="'row' or 'p3'"):
        yolov5_acmix_cfg(where='neck')
    cfg = yolov5_acmix_cfg(0.5, 1.0, nc=10)
    cfg['backbone'][10][1] = 2                                     # n > 1 would be an nn.Sequential of whole modules: refused as for every such module
    with pytest.raises(NotImplementedError, match="2 repeats of 'ACmix'"):
        Model(cfg)
    cfg = yolov5_acmix_cfg(0.5, 0.33, nc=10)
    cfg['backbone'][10][2] = 'BAM'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)
    cfg['backbone'][10] = [-1, 1, 'ACmix', [1024, 7, 8]]          # head = 8
    with pytest.raises(NotImplementedError, match='head=8'):
        Model(cfg)
    assert not any(r[2] == 'ACmix' for c in (yolov5_cfg(), yolov5_ema_cfg(), yolov5_ema_cfg(where='row')) for r in c['backbone'] + c['head'])
    assert len(yolov5_cfg()['head']) == 15 and yolov5_cfg()['head'][-1][0] == [17, 20, 23]


def test_optimizer_groups_follow_the_reference():
    """train.py:125-133: the conv weights and fc.weight are decayed, the four biases are in the bias group, rate1 and rate2 - neither a .weight
    nor a .bias - are in no group."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    for tag, (mk, _) in R.BLOCKS.items():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert not g0 and sorted(g1) == sorted(k for k in KEYS if k.endswith('.weight')), tag
        assert sorted(g2) == sorted(k for k in KEYS if k.endswith('.bias')) and len(g2) == 4, tag
        assert not {'rate1', 'rate2'} & set(g0 + g1 + g2)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]


def test_the_conv_half_is_one_grouped_conv_in_fp64():
    """dep_conv(fc(.)) = the grouped 3x3 conv with Weff[c, t, tap] = sum_j dep_conv.weight[c, j, tap] * fc.weight[j, t], borders included (zero
    padding commutes with the bias-free fc), at 1e-12."""
    for shape in R.KERNEL_SHAPES[:6]:
        t = {k: v.double() for k, v in R.kernel_inputs(shape).items()}
        q, k, v = (t[n].permute(0, 3, 1, 2) for n in ('q', 'k', 'v'))
        lit = R.conv_half(q, k, v, t['fc'], t['dep'], t['bias'])
        one = R.conv_half_folded(q, k, v, R.fold_weff(t['fc'], t['dep']), t['bias'])
        assert (lit - one).abs().max().item() <= 1e-12 * lit.abs().max().item(), shape
        border = torch.ones_like(lit, dtype=torch.bool)
        border[:, :, 1:-1, 1:-1] = False
        assert (lit - one)[border].abs().max().item() <= 1e-12 * lit.abs().max().item()


def test_the_position_term_is_two_scalars_per_pixel_and_head_in_fp64():
    """s * q . (pe_p - pe_r(p+j)) = s * (q . Wp[:, 0]) * dx_j + s * (q . Wp[:, 1]) * dy_j with dx, dy the differences of the position grid under the
    reflected index, and conv_p.bias drops out."""
    for shape in R.KERNEL_SHAPES[:6]:
        B, H, W, C = shape
        D = C // 4
        t = {k: v.double() for k, v in R.kernel_inputs(shape, 'pe').items()}
        q, k = t['q'].permute(0, 3, 1, 2), t['k'].permute(0, 3, 1, 2)
        loc = R.position(H, W, torch.float64)
        bias = torch.randn(D, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        pe = F.conv2d(loc, t['wp'].reshape(D, 2, 1, 1), bias)
        want = R.scores_from_pe(q, k, pe)
        s = float(D) ** -0.5
        qa = q.reshape(B * 4, D, H, W)
        qk = (qa.unsqueeze(2) * R.window(k.reshape(B * 4, D, H, W))).sum(1)
        dloc = loc.unsqueeze(2) - R.window(loc)                   # (1, 2, 49, H, W)
        qw = torch.einsum('ndhw,dc->nchw', qa, t['wp'])           # (B 4, 2, H, W)
        got = s * (qk + qw[:, 0:1] * dloc[:, 0] + qw[:, 1:2] * dloc[:, 1])
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), shape
        r = lambda i, n: -i if i < 0 else (2 * (n - 1) - i if i > n - 1 else i)     # noqa: E731
        x, y, jx, jy = W - 1, 0, 6, 1                             # a corner pixel: both taps reflect
        assert abs(dloc[0, 0, jy * 7 + jx, y, x].item() - 2.0 * (x - r(x + jx - 3, W)) / (W - 1)) <= 1e-15
        assert abs(dloc[0, 1, jy * 7 + jx, y, x].item() - 2.0 * (y - r(y + jy - 3, H)) / (H - 1)) <= 1e-15


@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=R.CASE_IDS)
def test_kernel_cases_are_ones_fp32_meets_half_the_bar_on(case):
    """Every case of test_acmix_gpu's kernel tests: the same formulas in fp32 on the CPU meet HALF the bar the GPU test applies against fp64."""
    shape, kind = case
    t = R.kernel_inputs(shape, kind)
    want, got = R.kernel_reference(t), R.kernel_reference(t, torch.float32)
    worst = {}
    for k, bar in KERNEL_BARS.items():
        scale = want[k].abs().max().item() + 1e-12
        worst[k] = (got[k].double() - want[k]).abs().max().item() / (bar * scale)
    print(f'{case}: fp32 against fp64 in units of the bar: ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))
    bad = {k: round(v, 3) for k, v in worst.items() if not v <= 0.5}
    assert not bad, f'{case}: the fp32 reference is beyond half the bar in {bad}'
    assert (want['mix'] - want['mix_literal']).abs().max().item() <= 1e-12 * want['mix'].abs().max().item()
    p = torch.softmax(want['scores'], 1)
    if kind == 'peaked':
        assert p.max().item() > 0.99 and want['scores'].max().item() > 89, 'not peaked: exp(score) must overflow in fp32 without the maximum'
        assert torch.isfinite(got['out']).all()
    if kind == 'pe':
        B, H, W, C = shape
        t0 = dict(t, wp=torch.zeros_like(t['wp']))
        assert (want['scores'] - R.kernel_reference(t0)['scores']).abs().max().item() > 5 * R.kernel_reference(t0)['scores'].abs().max().item()
    if kind == 'rate1_0':
        assert not want['dq'].any() and not want['out_att'].any() and want['drate1'].abs().item() > 0
    if kind == 'rate2_0':
        assert not want['cq'].any() and not want['dweff'].any() and want['drate2'].abs().item() > 0


@pytest.mark.parametrize('rates', R.RATES)
@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_block_cases_are_ones_the_fp32_oracle_can_be_judged_on(tag, rates):
    """The seeded block cases of test_acmix_gpu: the fp32 CPU restatement's parameter gradients meet HALF of parity.grads_close's bar
    (1e-3 * scale + 2e-5) against its own fp64 twin - conv_p.bias, whose true gradient is zero, included -, its output and input gradient half
    of rel_close's 1e-3."""
    ref, x, gen = R.block_case(tag, rates)
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
    print(f'{tag} {rates}: out {eo:.1e}, dx {ex:.1e}, parameter gradients at {worst:.3f} x the bar')
    assert worst <= 0.5 and eo <= 5e-4 and ex <= 5e-4, f'{tag}: the fp32 oracle is {worst:.2f} x the bar away from fp64 (out {eo:.1e}, dx {ex:.1e})'
    assert ref64.conv_p.bias.grad.abs().max().item() <= 1e-12 * ref64.conv_p.weight.grad.abs().max().item(), 'conv_p.bias has a gradient in fp64'
    assert ref.conv_p.bias.grad.abs().max().item() <= 1e-5          # half of grads_close's atol: what an exact zero is judged against


@pytest.mark.parametrize('where', ['row', 'p3'])
def test_graph_cases_are_ones_the_fp32_oracle_can_be_judged_on(where, monkeypatch):
    """The graph cases of test_acmix_gpu (acmix_ref.graph_case): the fp32 CPU oracle's parameter gradients meet HALF of check_train_step's bar
    (2e-3 * scale + 2e-6) against its own fp64 twin's; conv_p.bias, judged against an exact zero there, stays below 1e-6."""
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
    row = ref.model[10 if where == 'row' else 18]
    assert type(row) is R.ACmix and row.conv_p.bias.grad.abs().max().item() <= 1e-6
    assert tuple(imgs.shape[2:]) == (R.GRAPH_SIZE[where],) * 2 and row.out_planes == (256 if where == 'row' else 64)


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
    assert _lib.lib().somi_acmix_desc_bytes() == ctypes.sizeof(_lib.AcmixDesc)
    for fn in ('acmix_plan', 'acmix_fold_weff', 'acmix_split_dweff', 'acmix_conv', 'acmix_attn', 'acmix_attn_backward_q', 'acmix_attn_backward_kv',
               'acmix_conv_backward_data', 'acmix_conv_backward_weight'):
        assert callable(getattr(ops, fn))
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'acmix.hip' in mk and 'acmix' not in mk.split('ATOMIC_SRCS :=')[1].splitlines()[0].split()       # no -munsafe-fp-atomics
    assert 'atomic' not in open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'acmix.hip')).read()


SLICES = ('q', 'k', 'v', 'mix', 'out', 'lse', 'aux', 'dq', 'dk', 'dv')


def _desc(_lib, **kw):
    d = _lib.AcmixDesc()
    for i, f in enumerate(SLICES):
        setattr(d, f, _lib.Slice(0x10000 * (i + 1), 40, 4))
    for i, f in enumerate(('wp', 'rate1', 'rate2', 'weff', 'bias', 'dwp', 'drates', 'dweff', 'dbias')):
        setattr(d, f, 0x100000 * (i + 1))
    d.B, d.H, d.W, d.C = 1, 4, 6, 32
    d.workspace, d.workspace_floats = 0xA00000, 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs)),      # lse is 4 wide: cs - 4 fits
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def test_new_entry_points_refuse_without_a_launch():
    """The slice rule at the six descriptor entry points (SOMI_EINVAL with a message that names the slice), the refusals the header lists, the
    workspace checks; a rejected call launches nothing, so the made-up addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    qkv = {'q': 'q', 'k': 'k', 'v': 'v'}
    entries = {'attn': (L.somi_acmix_attn_nhwc_f32, dict(qkv, out='out', mix='mix', lse='lse'), ('mix', 'lse'), False),
               'bwd q': (L.somi_acmix_attn_bwd_q_nhwc_f32, dict(qkv, out='dout', mix='mix', lse='lse', aux='aux', dq='dq'), ('mix',), True),
               'bwd kv': (L.somi_acmix_attn_bwd_kv_nhwc_f32, dict(qkv, out='dout', lse='lse', aux='aux', dk='dk', dv='dv'), (), False),
               'conv': (L.somi_acmix_conv_nhwc_f32, dict(qkv, mix='mix'), (), False),
               'conv bwd data': (L.somi_acmix_conv_bwd_data_nhwc_f32, dict(out='dout', dq='dq', dk='dk', dv='dv'), (), False),
               'conv bwd weight': (L.somi_acmix_conv_bwd_weight_nhwc_f32, dict(qkv, out='dout'), (), True)}
    for key, (fn, fields, optional, workspace) in entries.items():
        for field, name in fields.items():
            for what, brk in BREAKS:
                if what == 'pointer NULL' and field in optional:
                    continue
                d = _desc(_lib)
                brk(getattr(d, field))
                assert fn(ctypes.byref(d), None) == -1, f'{key}: {name}: {what} is let through'
                assert re.search(r'\b%s = \[' % name, L.somi_last_error().decode()), f'{key}: {name}: {what}: {L.somi_last_error()}'
        for kw, word in ((dict(C=24), b'C % 16 == 0'), (dict(C=2048), b'at most 1024'), (dict(B=1 << 14, H=1 << 8, W=1 << 8), b'2^30 floats')):
            assert fn(ctypes.byref(_desc(_lib, **kw)), None) == -2 and word in L.somi_last_error(), f'{key}: {kw}: {L.somi_last_error()}'
        for kw in (dict(C=0), dict(H=0), dict(B=-1)):
            assert fn(ctypes.byref(_desc(_lib, **kw)), None) == -1 and b'bad sizes' in L.somi_last_error(), f'{key}: {kw}'
        for kw in (dict(H=3), dict(W=3)):
            assert fn(ctypes.byref(_desc(_lib, **kw)), None) == -1 and b'reflection pad of 3' in L.somi_last_error(), f'{key}: {kw}'
        assert fn(None, None) == -1
        if workspace:
            need = L.somi_acmix_workspace_floats(1, 4, 6, 32)
            assert need > 0 and fn(ctypes.byref(_desc(_lib, workspace_floats=need - 1)), None) == -3, f'{key}: a short workspace is let through'
            assert fn(ctypes.byref(_desc(_lib, workspace=None)), None) == -1
            assert fn(ctypes.byref(_desc(_lib, workspace=0xA00004)), None) == -1
    for missing in ('wp', 'rate1', 'rate2'):
        assert L.somi_acmix_attn_nhwc_f32(ctypes.byref(_desc(_lib, **{missing: None})), None) == -1
    assert L.somi_acmix_fold_weff_f32(0x1000, 0x2000, 0x3000, 24, None) == -2 and L.somi_acmix_fold_weff_f32(0x1000, None, 0x3000, 32, None) == -1
    assert L.somi_acmix_split_dweff_f32(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 2048, None) == -2
    assert L.somi_acmix_split_dweff_f32(0x1000, 0x2000, 0x3000, 0x4000, 0x5004, 32, None) == -1


def test_plan_and_workspace_are_host_arithmetic():
    """A workgroup of the attention kernels owns an 8x8 tile; the workspace holds two partials per tile and 2 C per block of the dWp reduction,
    or the weight-gradient partials (436 values per head dim and chunk of image rows, at most 256 chunks and 4 Mi floats), whichever is larger."""
    from somi_amd import ops
    L = ops._lib.lib()
    assert ops.acmix_plan(4, 4) == (8, 1, 1) and ops.acmix_plan(11, 13) == (8, 2, 2) and ops.acmix_plan(80, 80) == (8, 10, 10)
    assert ops.acmix_plan(8, 9) == (8, 1, 2)
    with pytest.raises(RuntimeError):
        ops.acmix_plan(3, 8)
    assert L.somi_acmix_workspace_floats(2, 11, 13, 64) == max(16 + 256 * 64 * 2, 22 * 436 * 16)
    assert L.somi_acmix_workspace_floats(1, 4, 4, 16) == max(4 + 16 * 16 * 2, 4 * 436 * 4)
    assert L.somi_acmix_workspace_floats(32, 80, 80, 128) == max(32 * 100 * 2 + 256 * 128 * 2, 256 * 436 * 32)
    assert L.somi_acmix_workspace_floats(1, 4, 5, 1024) == max(4 + 20 * 1024 * 2, 4 * 436 * 256)
    assert L.somi_acmix_workspace_floats(32, 20, 20, 1024) == max(32 * 9 * 2 + 256 * 1024 * 2, ((4 << 20) // (436 * 256)) * 436 * 256)
    for bad in ((1, 3, 4, 32), (1, 4, 4, 24), (1, 4, 4, 2048), (0, 4, 4, 32)):
        assert L.somi_acmix_workspace_floats(*bad) == 0
