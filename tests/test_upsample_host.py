"""CPU checks of the two learned 2x upsamplers of the neck (models/common.py:4450 CARAFE, :4246 DySample): the test restatement
(tests/upsample_ref.py) reproduces the reference's own classes through the tests/golden/block_{carafe,carafe_k3,dysample,dysample_g2}.npz fixtures
(tools/gen_upsample_golden.py), the product blocks keep the reference's parameter and buffer layout, the graphs build with either module in the
nn.Upsample rows at unchanged strides, and the limits of the MI355X path are explicit."""
import os
import re

import numpy as np
import pytest
import torch

import upsample_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIXTURES = {'carafe': (lambda M: M.CARAFE(32, 3, 5), (2, 32, 7, 9)), 'carafe_k3': (lambda M: M.CARAFE(16, 1, 3, 16), (2, 16, 6, 5)),
            'dysample': (lambda M: M.DySample(32), (2, 32, 7, 9)), 'dysample_g2': (lambda M: M.DySample(24, 2, 'lp', 2), (2, 24, 6, 5))}

# the reference's own state dicts for the four configurations (models/common.py:4465-4469, 4264-4270): names in order, shapes
REF_STATE = {
    'carafe': [('comp.conv.weight', (64, 32, 1, 1)), ('comp.bn.weight', (64,)), ('comp.bn.bias', (64,)), ('comp.bn.running_mean', (64,)),
               ('comp.bn.running_var', (64,)), ('comp.bn.num_batches_tracked', ()), ('enc.conv.weight', (100, 64, 3, 3)), ('enc.bn.weight', (100,)),
               ('enc.bn.bias', (100,)), ('enc.bn.running_mean', (100,)), ('enc.bn.running_var', (100,)), ('enc.bn.num_batches_tracked', ())],
    'carafe_k3': [('comp.conv.weight', (16, 16, 1, 1)), ('comp.bn.weight', (16,)), ('comp.bn.bias', (16,)), ('comp.bn.running_mean', (16,)),
                  ('comp.bn.running_var', (16,)), ('comp.bn.num_batches_tracked', ()), ('enc.conv.weight', (36, 16, 1, 1)), ('enc.bn.weight', (36,)),
                  ('enc.bn.bias', (36,)), ('enc.bn.running_mean', (36,)), ('enc.bn.running_var', (36,)), ('enc.bn.num_batches_tracked', ())],
    'dysample': [('init_pos', (1, 32, 1, 1)), ('offset.weight', (32, 32, 1, 1)), ('offset.bias', (32,))],
    'dysample_g2': [('init_pos', (1, 16, 1, 1)), ('offset.weight', (16, 24, 1, 1)), ('offset.bias', (16,))]}


@pytest.mark.parametrize('tag', list(FIXTURES))
def test_restatement_reproduces_the_reference_blocks(tag):
    """Eval and train outputs of the reference's classes under fill_state weights (oracle.gen_golden.run_block), fp32 on both sides, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    mk, shape = FIXTURES[tag]
    mod = fill_state(mk(R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['in0'])
    assert tuple(x.shape) == shape
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        assert y.shape == want.shape == (shape[0], shape[1], 2 * shape[2], 2 * shape[3])
        err = (y - want).abs().max().item()
        assert err <= 1e-5 * want.abs().max().item(), f'{tag} {mode}: {err:.3e}'


@pytest.mark.parametrize('tag', list(FIXTURES))
def test_blocks_keep_the_reference_state_dict(tag):
    """Names (in order) and shapes of parameters and buffers: the reference's, for the restatement and for the product block, so reference
    checkpoints load; init_pos is the reference's buffer (+-0.25, x in the first half following dx, y in the second following dy)."""
    from somi_amd import blocks as MB
    mk, _ = FIXTURES[tag]
    a, b = mk(R), mk(MB)
    for mod in (a, b):
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == REF_STATE[tag]
    assert [n for n, _ in b.named_buffers()] == [n for n, _ in a.named_buffers()]
    assert [n for n, _ in b.named_parameters()] == [n for n, _ in a.named_parameters()]
    b.load_state_dict(a.state_dict())
    if tag.startswith('dysample'):
        G = b.groups
        want = torch.tensor([-0.25, 0.25, -0.25, 0.25] * G + [-0.25, -0.25, 0.25, 0.25] * G).view(1, -1, 1, 1)
        assert torch.equal(mk(MB).init_pos, want) and torch.equal(mk(R).init_pos, want)
        assert mk(MB).offset.weight.std().item() < 2e-3 and not mk(MB).offset.bias.any()    # normal_init(std=0.001), bias 0


@pytest.mark.parametrize('up', ['carafe', 'dysample'])
@pytest.mark.parametrize('graph', ['somi', 'yolov5', 'yolov10'])
def test_graphs_build_with_the_learned_upsamplers(graph, up, monkeypatch):
    """Model builds the tables with the nn.Upsample rows rewritten; Detect.stride is what upsample='nearest' gives; for the graphs the oracle parses,
    names, shapes and the save list equal the oracle Model's built through the upsample_ref registration."""
    from oracle.somi_ref import Model as OModel
    from somi_amd import blocks as MB
    from somi_amd import configs
    from somi_amd.model import Model
    mk = {'somi': lambda **kw: configs.somi_cfg(0.25, 0.33, **kw), 'yolov5': lambda **kw: configs.yolov5_cfg(**kw),
          'yolov10': lambda **kw: configs.yolov10_cfg(0.25, 0.33, **kw)}[graph]
    plain, cfg = mk(), mk(upsample=up)
    rows, prows = cfg['backbone'] + cfg['head'], plain['backbone'] + plain['head']
    want_row = {'carafe': ['CARAFE', [3, 5]], 'dysample': ['DySample', []]}[up]
    n_up = sum(r[2] == 'nn.Upsample' for r in prows)
    assert n_up == (3 if graph == 'somi' else 2)
    for r, p in zip(rows, prows):
        assert r == ([p[0], p[1], *want_row] if p[2] == 'nn.Upsample' else p)
    assert mk(upsample='nearest') == plain
    base, mine = Model(plain), Model(cfg)
    assert mine.stride.tolist() == base.stride.tolist() and mine.model[-1].stride.tolist() == base.model[-1].stride.tolist()
    cls = MB.CARAFE if up == 'carafe' else MB.DySample
    ups = [m for m in mine.model if isinstance(m, cls)]
    assert len(ups) == n_up and not any(isinstance(m, MB.Upsample) for m in mine.model)
    assert mine.save == base.save
    if graph == 'yolov10':
        return                                                    # its other modules need tests/yolov10_ref.py; the rows are checked above
    R.register(monkeypatch)
    ref = OModel(cfg)
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert list(mine.state_dict()) == list(ref.state_dict())
    assert mine.stride.tolist() == ref.stride.tolist() and mine.save == ref.save
    assert [m.type for m in mine.model] == [m.type for m in ref.model]
    assert [m.np for m in mine.model] == [m.np for m in ref.model]
    mine.load_state_dict(ref.state_dict())


def test_unknown_upsample_choice_is_an_error():
    from somi_amd.configs import somi_cfg, yolov5_cfg, yolov10_cfg
    for fn in (somi_cfg, yolov5_cfg, yolov10_cfg):
        with pytest.raises(ValueError, match="upsample='bilinear'"):
            fn(upsample='bilinear')


LIMITS = [(lambda M: M.CARAFE(32, 3, 5, 64, 4), 'scale 2 only'), (lambda M: M.CARAFE(32, 3, 7), 'k_up 3 or 5'),
          (lambda M: M.CARAFE(32, 5, 5), 'k_enc 1 or 3'), (lambda M: M.CARAFE(30), r'c % 4 == 0'),
          (lambda M: M.DySample(32, 4), 'scale 2 only'), (lambda M: M.DySample(32, 2, 'pl'), "style 'lp' only"),
          (lambda M: M.DySample(32, 2, 'lp', 4, True), 'dyscope=True'), (lambda M: M.DySample(30, 2, 'lp', 2), r'c % 4 == 0'),
          (lambda M: M.DySample(24, 2, 'lp', 4), r'\(c / groups\) % 4 == 0')]


@pytest.mark.parametrize('i', range(len(LIMITS)))
def test_limits_are_explicit(i):
    from somi_amd import blocks as MB
    mk, msg = LIMITS[i]
    with pytest.raises(NotImplementedError, match=msg):
        mk(MB)


def test_a_limit_reaches_the_user_through_model():
    from somi_amd.configs import yolov5_cfg
    from somi_amd.model import Model
    cfg = yolov5_cfg(0.25, 0.33, upsample='carafe')
    cfg['head'][1] = [-1, 1, 'CARAFE', [3, 7]]
    with pytest.raises(NotImplementedError, match='k_up 3 or 5'):
        Model(cfg)


def test_symbols_are_declared_and_bound():
    """The four entry points are in the header, in the binding and in the built library; the ABI version did not move."""
    from somi_amd import _lib
    names = ['somi_carafe_nhwc_f32', 'somi_carafe_bwd_nhwc_f32', 'somi_dysample_nhwc_f32', 'somi_dysample_bwd_nhwc_f32']
    header = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    L = _lib.lib()
    for n in names:
        m = re.search(r'\bint ' + n + r'\(([^;]*)\);', header)
        assert m, f'{n} is not declared in include/somi_hip.h'
        assert n in _lib.SIGNATURES and hasattr(L, n)
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[n][1]), f'{n}: the binding and the header disagree on the argument count'
    assert _lib.ABI_VERSION == 15 and L.somi_abi_version() == 15
    assert '#define SOMI_ABI_VERSION 15' in header


def test_ops_are_public_and_refuse_cpu_tensors():
    from somi_amd import ops
    for n in ('carafe', 'carafe_backward', 'dysample', 'dysample_backward', 'dysample_far_taps'):
        assert callable(getattr(ops, n))
    x = torch.zeros(1, 2, 2, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.carafe(x, torch.zeros(1, 2, 2, 36), 4, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.dysample(x, torch.zeros(1, 2, 2, 8), torch.zeros(8), 4, 1)
