"""CPU checks of MultiSEAM (models/common.py:8508-8555), SEAM with n > 1 stages (:8448-8505) and the patch-embedding geometry (kernel = stride,
no padding) of the dense conv entries: the test restatement (tests/seam_ref.py) reproduces the reference's own classes through the three
tests/golden/block_*seam*.npz fixtures; state-dict layouts, parser, strides and parameter groups are the restatement's; every limit raises by
name; the C ABI's three conv entries check Ho / Wo of a patch descriptor; and the fp32 CPU restatement meets each GPU test's gradient bar
against its fp64 copy at the seeds those tests use."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':                                       # the child (below) runs this file as a script: the oracle lives at the root
    sys.path.insert(0, ROOT)

import seam_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EINVAL = -1
SEAM_ROWS = [[-1, 1, 'SEAM', [256, 1, 16]]] * 3                   # what somi_cfg() has always returned at head rows 6, 10 and 14


# ---------------------------------------------------------------------------------------------------------------- the restatement and the blocks
@pytest.mark.parametrize('tag', R.FIXTURES)
def test_restatement_reproduces_the_reference(tag):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    assert sorted(d.files) == ['out_eval', 'out_train', 'x']
    make, shape = R.BLOCKS[tag]
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == shape == (2, 64, 15, 17)
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        err = (y - want).abs().max().item()
        assert y.shape == want.shape and err <= 1e-5 * want.abs().max().item(), f'{tag} {mode}: {err:.3e}'


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    makes = [mk for mk, _ in R.BLOCKS.values()] + [lambda M: M.MultiSEAM(32, 64, 1, 3, [2, 4, 8], 8), lambda M: M.SEAM(32, 16, 3, 8)]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())
    m = MB.MultiSEAM(64, 64, 2)
    keys = list(m.state_dict())
    for k in ('DCovN0.0.weight', 'DCovN0.0.bias', 'DCovN1.2.running_var', 'DCovN2.3.0.fn.0.weight', 'DCovN2.4.0.fn.0.weight', 'DCovN2.4.3.weight',
              'fc.0.weight', 'fc.2.weight'):
        assert k in keys, k
    assert [tuple(getattr(m, f'DCovN{j}')[0].weight.shape) for j in range(3)] == [(64, 64, 3, 3), (64, 64, 5, 5), (64, 64, 7, 7)]
    assert [getattr(m, f'DCovN{j}')[0].stride for j in range(3)] == [(3, 3), (5, 5), (7, 7)] and m.DCovN0[0].padding == (0, 0)
    assert tuple(m.fc[0].weight.shape) == (4, 64) and m.fc[0].bias is None
    assert MB.MultiSEAM(32, 64, 1).DCovN0[0].out_channels == 32, 'c1 != c2 sets c2 = c1'
    s = MB.SEAM(64, 64, 3)
    assert len(s.DCovN) == 6 and all(isinstance(s.DCovN[i][0], MB.Residual) for i in (3, 4, 5))
    # torch's default initialisation: SEAM's xavier initialiser sets every BatchNorm weight to 1 and draws conv weights from another range
    torch.manual_seed(0)
    mine = MB.MultiSEAM(64, 64, 1)
    torch.manual_seed(0)
    want = R.MultiSEAM(64, 64, 1)
    assert all(torch.equal(a, b) for a, b in zip(mine.state_dict().values(), want.state_dict().values()))


def test_new_blocks_declare_the_walk_contract_themselves():
    from somi_amd import blocks as MB
    for cls in (MB.MultiSEAM, MB.SEAM):
        assert cls.__dict__['accumulates'] is False and cls.__dict__['folds_pooled'] is False and cls.__dict__['reduction'] == 1, cls.__name__
    import inspect
    assert list(inspect.signature(MB.MultiSEAM.backward).parameters)[2:5] == ['dx_out', 'accumulate', 'need_dx']
    assert list(inspect.signature(MB.MultiSEAM.__init__).parameters) == ['self', 'c1', 'c2', 'depth', 'kernel_size', 'patch_size', 'reduction']


def test_limits_are_explicit():
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    with pytest.raises(NotImplementedError, match='kernel_size 5'):
        MB.MultiSEAM(64, 64, 1, 5)
    for bad in ([3, 5], [3, 5, 0], [3, 5, 7.0], 3, [3, -5, 7]):
        with pytest.raises(NotImplementedError, match='three positive ints'):
            MB.MultiSEAM(64, 64, 1, 3, bad)
    with pytest.raises(NotImplementedError, match='quarter divides 256'):
        MB.MultiSEAM(96, 96, 1)                                     # 24 does not divide 256
    with pytest.raises(NotImplementedError, match='quarter divides 256'):
        MB.MultiSEAM(2048, 2048, 1, reduction=512)
    with pytest.raises(NotImplementedError, match='depth'):
        MB.MultiSEAM(64, 64, 0)
    with pytest.raises(NotImplementedError, match='stages'):
        MB.SEAM(64, 64, 0)
    m = MB.MultiSEAM(64, 64, 1)
    with pytest.raises(NotImplementedError, match='whole tensor'):
        m(Act(torch.zeros(1, 16, 16, 72), 4, 64))
    with pytest.raises(NotImplementedError, match='whole tensor'):
        MB.MultiSEAM(8, 8, 1, reduction=2)(Act(torch.zeros(1, 16, 16, 8), 0, 6))
    with pytest.raises(RuntimeError, match='6 x 9 map is smaller than its largest patch, 7 x 7'):
        m(Act(torch.zeros(1, 6, 9, 64)))
    with pytest.raises(RuntimeError, match='12 x 9 map is smaller than its largest patch, 11 x 11'):
        MB.MultiSEAM(64, 64, 1, 3, [11, 2, 3])(Act(torch.zeros(1, 12, 9, 64)))
    for kw in (dict(dx_out=Act(torch.zeros(1, 16, 16, 64))), dict(accumulate=True)):
        with pytest.raises(NotImplementedError, match='writes its own input gradient'):
            m.backward(Act(torch.zeros(1, 16, 16, 64)), **kw)
        with pytest.raises(NotImplementedError, match='writes its own input gradient'):
            MB.SEAM(64, 64, 2).backward(Act(torch.zeros(1, 16, 16, 64)), **kw)


def test_param_groups_follow_the_reference():
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    for tag in ('multiseam_d2', 'seam_n2'):
        mk = R.BLOCKS[tag][0]
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert sorted(g0 + g1 + g2) == sorted(names.values()), 'a parameter is in no group'
        bns = [n + '.weight' for n, mod in m.named_modules() if isinstance(mod, nn.BatchNorm2d)]
        assert sorted(g0) == sorted(bns) and len(bns) == (15 if tag == 'multiseam_d2' else 5)
        assert sorted(g1) == sorted(n + '.weight' for n, mod in m.named_modules() if isinstance(mod, (nn.Conv2d, nn.Linear)))
        assert all(n.endswith('.bias') for n in g2) and 'fc.0.bias' not in g2
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]


# ---------------------------------------------------------------------------------------------------------------- configs and the parser
@pytest.mark.parametrize('how', ['multi', 'seam2'])
def test_seam_graph_matches_the_oracle(how, monkeypatch):
    from somi_amd import blocks as MB
    from somi_amd.configs import somi_cfg
    from somi_amd.model import Model, _CH, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert _CH['MultiSEAM'] is MB.MultiSEAM and 'MultiSEAM' not in _REPEAT_INSIDE and 'SEAM' not in _REPEAT_INSIDE
    cfg = R.graph_cfg(how)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert mine.stride.tolist() == ref.stride.tolist() == [4.0, 8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    mine.load_state_dict(ref.state_dict())
    for m in mine.model:                                          # what the graph walk reads of every layer
        assert isinstance(m.accumulates, bool) and isinstance(m.folds_pooled, bool) and m.reduction in (0.5, 1, 2), m.type
    base = somi_cfg(0.25, 0.33, nc=10)
    assert cfg['backbone'] == base['backbone'] and [r[:2] for r in cfg['head']] == [r[:2] for r in base['head']]
    changed = [i for i, (a, b) in enumerate(zip(cfg['head'], base['head'])) if a != b]
    assert changed == [6, 10, 14]
    for i in changed:
        layer = mine.model[10 + i]
        if how == 'multi':
            assert cfg['head'][i] == [-1, 1, 'MultiSEAM', [256, 1]] and type(layer) is MB.MultiSEAM and layer.patch_size == (3, 5, 7)
            assert layer.DCovN2[0].in_channels == 64 and len(layer.DCovN0) == 4
        else:
            assert cfg['head'][i] == [-1, 1, 'SEAM', [256, 2, 16]] and type(layer) is MB.SEAM and len(layer.DCovN) == 5
    assert somi_cfg(seam='multi', seam_depth=3)['head'][6] == [-1, 1, 'MultiSEAM', [256, 3]]


def test_cfg_defaults_are_unchanged():
    from somi_amd.configs import somi_cfg
    from oracle.somi_ref.testing import somi_cfg as oracle_cfg
    import inspect
    assert list(inspect.signature(somi_cfg).parameters)[-2:] == ['seam', 'seam_depth']
    cfg = somi_cfg()
    assert [cfg['head'][i] for i in (6, 10, 14)] == SEAM_ROWS
    assert cfg == somi_cfg(seam='seam', seam_depth=1)
    assert all(r[2] != 'MultiSEAM' for r in cfg['backbone'] + cfg['head'])
    o = oracle_cfg(1.0, 1.0)
    assert cfg['backbone'] == o['backbone'] and cfg['head'] == o['head']
    for kw in (dict(dcn=True), dict(upsample='carafe')):
        a, b = somi_cfg(0.25, 0.33, **kw), somi_cfg(0.25, 0.33, seam='multi', **kw)
        assert [r[2] for r in a['head']].count('SEAM') == 3 == [r[2] for r in b['head']].count('MultiSEAM')
        assert [r[:2] for r in a['head']] == [r[:2] for r in b['head']]
    with pytest.raises(ValueError, match="'seam' or 'multi'"):
        somi_cfg(seam='multiseam')
    with pytest.raises(ValueError, match='seam_depth'):
        somi_cfg(seam_depth=0)


def test_c3tr_stays_outside():
    from somi_amd.configs import somi_cfg
    from somi_amd.model import Model
    cfg = somi_cfg(0.25, 0.33, seam='multi')
    cfg['head'][7][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


# ---------------------------------------------------------------------------------------------------------------- the seeds, judged by the reference alone
def _bars(ref, ref64, rel, atol):
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        if q.grad is None:                                        # ODConv_3rd's conv.reduction: unused in the reference's forward
            assert p.grad is None
            continue
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    return worst


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_block_seeds_meet_the_bar_in_fp32(tag):
    """The fp32 CPU restatement against its fp64 copy at the seed tests/test_seam_gpu.py uses, under parity.grads_close's bar and with room to spare
    (a quarter of it): what the GPU result is held to is then the kernels' error, not the conditioning of the case."""
    ref, x, gen = R.block_case(tag)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    y64, y = ref64(x.double()), ref(x)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    y64.backward(dy.double())
    worst = _bars(ref, ref64, 1e-3, 2e-5)
    print(f'{tag}: fp32 against fp64 {worst:.3f} x the bar')
    assert worst <= 0.25


@pytest.mark.parametrize('how', sorted(R.GRAPH_SEEDS))
def test_graph_seeds_meet_the_bar_in_fp32(how, monkeypatch):
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    R.register(monkeypatch)
    _, ref, imgs, targets = R.graph_case(how)
    ref64 = copy.deepcopy(ref).double().train()
    ref.train()
    OLoss(ref64)(ref64(imgs.double() / 255), targets.double())[0].backward()
    OLoss(ref)(ref(imgs.float() / 255), targets)[0].backward()
    worst = _bars(ref, ref64, 2e-3, 2e-6)
    print(f'{how}: fp32 against fp64 {worst:.3f} x the bar')
    assert worst <= 0.25


# ---------------------------------------------------------------------------------------------------------------- the C ABI, in a child without a device
GEO = {'d.w': 0, 'd.B': 2, 'd.H': 15, 'd.W': 17, 'd.Cin': 32, 'd.Cout': 32, 'd.pad': 0, 'd.dil': 1, 'd.x': 0, 'd.y': 0,
       'd.x_cs': 32, 'd.y_cs': 32, 'dy_cs': 32, 'dx_cs': 32, 'x_cs': 32, 'accumulate': None, 'workspace_bytes': 1 << 40}
ENTRIES = {'fwd': 'somi_conv2d_nhwc_f32', 'dgrad': 'somi_conv2d_dgrad_nhwc_f32', 'wgrad': 'somi_conv2d_wgrad_nhwc_f32'}
CASES = {}
for _e, _fn in ENTRIES.items():
    for _p in (3, 5, 7):
        _g = {'d.kh': _p, 'd.kw': _p, 'd.stride': _p}
        CASES[f'{_e} p{_p}'] = (_fn, dict(_g, **{'d.Ho': 15 // _p, 'd.Wo': 17 // _p}))
        # the sizes a ceiling division would give: the last, partial patch does not exist
        CASES[f'{_e} p{_p} wrong size'] = (_fn, dict(_g, **{'d.Ho': -(-15 // _p), 'd.Wo': -(-17 // _p)}))
    CASES[f'{_e} p7 generic'] = (_fn, {'d.kh': 7, 'd.kw': 7, 'd.stride': 7, 'd.Ho': 2, 'd.Wo': 2, 'd.Cin': 8, 'd.Cout': 12, 'd.x_cs': 8, 'd.y_cs': 12,
                                       'dy_cs': 12, 'dx_cs': 8, 'x_cs': 8})
    CASES[f'{_e} p7 map smaller than the patch'] = (_fn, {'d.kh': 7, 'd.kw': 7, 'd.stride': 7, 'd.H': 6, 'd.Ho': 0, 'd.Wo': 2})
VALID = [n for n in CASES if 'wrong' not in n and 'smaller' not in n]
INVALID = [n for n in CASES if n not in VALID]


def _child():
    import torch
    n = torch.cuda.device_count()
    if n != 0:                                               # the guard: with a device visible nothing is called
        print(json.dumps({'devices': n}))
        return
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_slice_args_host as S                         # its caller of an entry point from made-up addresses, and the header's prototypes
    from somi_amd import _lib
    L = _lib.lib()
    protos = S.prototypes()
    out = {}
    for name, (fn, geo) in CASES.items():
        rc, err = S._call(L, _lib, protos[fn], dict(GEO, fn=fn, **geo))
        out[name] = {'rc': rc, 'error': err}
    print(json.dumps({'devices': 0, 'results': out}))


_cache = {}


def child_results():
    if 'run' not in _cache:
        env = dict(os.environ, HIP_VISIBLE_DEVICES='-1')
        _cache['run'] = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    r = _cache['run']
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out['devices'] != 0:
        pytest.skip(f"{out['devices']} GPU(s) visible to the child despite HIP_VISIBLE_DEVICES=-1: made-up addresses are never handed to a process "
                    "that could launch on them")
    return out['results']


@pytest.mark.parametrize('name', VALID)
def test_abi_accepts_the_patch_geometry(name):
    c = child_results()[name]
    assert c['rc'] > 0, f'{name}: returned {c["rc"]}, "{c["error"]}" - without a device an accepted call ends in the launch failure'


@pytest.mark.parametrize('name', INVALID)
def test_abi_checks_the_output_size_of_a_patch_descriptor(name):
    c = child_results()[name]
    assert c['rc'] == EINVAL, f'{name}: returned {c["rc"]}, "{c["error"]}"'


if __name__ == '__main__':
    _child()
