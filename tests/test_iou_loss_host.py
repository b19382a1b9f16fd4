"""The box-regression rules of the fused loss, host side: the plain-torch restatement (tests/iou_loss_ref.py) against the fixture the
reference's own functions produced (tests/golden/iou_loss.npz, tools/gen_iou_loss_golden.py), what ComputeLoss refuses, the binding's mirror
of somi_loss_box_rule, and TrainStep handing its loss_kwargs on."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import iou_loss_ref as R

T = torch.from_numpy
CASE_RULE = [(c, tag) for c, (_, _, tags) in R.CASES.items() for tag in tags]


def _hyp(case):
    from oracle.somi_ref.testing import HYP_VISDRONE
    return dict(HYP_VISDRONE, **R.CASES[case][1])


def _inputs(g, case):
    src = R.CASES[case][0]
    nl = g[f'{src}_anchors'].shape[0]
    return T(g[f'{src}_anchors']), [T(g[f'{src}_p{i}']) for i in range(nl)], T(g[f'{src}_targets'])


def test_fixture_holds_the_cases_it_should(golden):
    g = golden('iou_loss')
    for case, (src, _, tags) in R.CASES.items():
        grids, nt, dup = R.SHAPES[src]
        anchors, p, tg = R.make_inputs(grids, nt, int(g[f'{src}_seed']), dup)     # the committed recipe gives the committed inputs
        assert np.array_equal(anchors.numpy(), g[f'{src}_anchors']) and np.array_equal(tg.numpy(), g[f'{src}_targets'])
        assert all(np.array_equal(t.numpy(), g[f'{src}_p{i}']) for i, t in enumerate(p))
        assert g[f'{case}_margin'] >= 64, f'case {case}: a branch within {g[f"{case}_margin"]} spacings of flipping'
        assert all(f'{case}_{tag}_loss' in g for tag in tags)
    assert set(R.CASES['a'][2]) == set(R.RULES) and len(R.RULES) == 19
    assert R.CASES['g'][0] == 'b' and R.CASES['g'][1]['slide_ratio'] > 0 and g['g_entries'].min() == 0 < g['g_entries'].max()
    assert (g['a_entries'] > 0).all() and (g['d_entries'] > 0).all() and len(g['d_entries']) == 5
    assert g['b_entries'].min() == 0 < g['b_entries'].max() and g['c_entries'].sum() == 0
    # case e: cells hit by more than one entry (what the gradient's list walk is for)
    anchors, p, tg = _inputs(g, 'e')
    crit = R.restated_loss(anchors, _hyp('e'), R.RULES['GIoU'])
    _, _, indices, _ = crit.build_targets(p, tg)
    cells = torch.stack(indices[0], 1)
    assert len(torch.unique(cells, dim=0)) < len(cells)


@pytest.mark.parametrize('case,tag', CASE_RULE)
def test_restatement_matches_reference_fixture(golden, case, tag):
    """fp64 against fp64: loss and items to 1e-9, gradients to the fp32 rounding of the stored ones."""
    g = golden('iou_loss')
    anchors, p, tg = _inputs(g, case)
    state = R.WIoUState()
    crit = R.restated_loss(anchors, _hyp(case), R.RULES[tag], state)
    pd = [t.double().requires_grad_(True) for t in p]
    loss, items = crit(pd, tg)
    loss.backward()
    np.testing.assert_allclose(loss.detach().numpy(), g[f'{case}_{tag}_loss'], rtol=1e-9)
    np.testing.assert_allclose(items.numpy(), g[f'{case}_{tag}_items'], rtol=1e-9, atol=1e-12)
    for i, t in enumerate(pd):
        want = g[f'{case}_{tag}_g{i}']
        np.testing.assert_allclose(t.grad.numpy(), want, rtol=2e-7, atol=1e-7 * np.abs(want).max() + 1e-30, err_msg=f'd loss / d p[{i}]')
    if R.RULES[tag].get('wiou_scale'):
        means = [state.mean]
        for _ in range(2):
            crit([t.double() for t in p], tg)
            means.append(state.mean)
        np.testing.assert_allclose(means, g[f'{case}_{tag}_wiou_mean'], rtol=1e-12)
        if g[f'{case}_entries'].sum():
            assert means[0] != 1.0 and means[0] != means[1] != means[2]
        else:
            assert means == [1.0, 1.0, 1.0]


def test_default_rule_is_the_oracles_ciou(golden):
    """The restated CIoU rule through RuleLoss is oracle.somi_ref.loss.ComputeLoss itself."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    g = golden('iou_loss')
    anchors, p, tg = _inputs(g, 'e')
    a, ai = OLoss(R.Model(anchors, _hyp('e')))(p, tg)
    b, bi = R.restated_loss(anchors, _hyp('e'), {})(p, tg)
    assert torch.equal(a, b) and torch.equal(ai, bi)


@pytest.mark.parametrize('kw,word', [
    (dict(iou='SIoU', focal=True), 'name clash'), (dict(iou='EfficiCIoU', focal=True), 'Focal'), (dict(iou='WIoU', focal=True), 'Focal'),
    (dict(iou='shape', focal=True), 'Focal'), (dict(iou='CIoU', alpha=0.5), 'alpha'), (dict(iou='GIoU', alpha=float('nan')), 'alpha'),
    (dict(iou='CIoU', inner_ratio=0.7, focal=True), 'inner_ratio'), (dict(iou='EIoU', inner_ratio=0.7, alpha=2.0), 'inner_ratio'),
    (dict(iou='WIoU', inner_ratio=0.7), 'inner_ratio'), (dict(iou='EfficiCIoU', inner_ratio=0.7), 'inner_ratio'),
    (dict(iou='shape', inner_ratio=0.7), 'inner_ratio'), (dict(iou='ciou'), 'unknown'), (dict(iou='MPDIoU'), 'unknown'),
    (dict(iou='EfficiCIoU', alpha=2.0), 'alpha'), (dict(iou='WIoU', alpha=2.0), 'alpha'), (dict(iou='shape', alpha=2.0), 'alpha'),
    (dict(iou='CIoU', wiou_scale=True), 'wiou_scale')])
def test_compute_loss_refuses(kw, word):
    """ValueError that names the reason, from the constructor: nothing is launched (the model here lives on the CPU)."""
    from somi_amd.loss import ComputeLoss
    mdl = R.Model(torch.rand(3, 3, 2) + 0.5, {'label_smoothing': 0.0})
    with pytest.raises(ValueError, match=word):
        ComputeLoss(mdl, **kw)


def test_train_step_hands_loss_kwargs_to_compute_loss(monkeypatch):
    """TrainStep(loss_kwargs=...) builds its ComputeLoss with exactly those keywords (and with none by default).  The model is a stand-in
    that claims to live on the device and the optimizer is stubbed out: nothing of the GPU is needed to see what is handed on."""
    from somi_amd import train

    class FakeModel:
        def parameters(self):
            return iter([type('P', (), {'is_cuda': True})()])

        def train(self):
            return self
    seen = []

    class Recorder:
        def __init__(self, model, **kw):
            seen.append((model, kw))
    monkeypatch.setattr(train, 'ComputeLoss', Recorder)
    monkeypatch.setattr(train, 'build_optimizer', lambda *a, **k: None)
    m = FakeModel()
    kw = dict(iou='WIoU', wiou_scale=True)
    tr = train.TrainStep(m, {'some': 'hyp'}, 2, loss_kwargs=kw)
    assert seen == [(m, kw)] and isinstance(tr.compute_loss, Recorder)
    train.TrainStep(m, {}, 2)
    assert seen[1] == (m, {})
    # and the real ComputeLoss in that place refuses what it refuses
    monkeypatch.undo()
    monkeypatch.setattr(train, 'build_optimizer', lambda *a, **k: None)
    m.model = R.Model(torch.rand(3, 3, 2) + 0.5, {}).model
    with pytest.raises(ValueError, match='name clash'):
        train.TrainStep(m, {}, 2, loss_kwargs=dict(iou='SIoU', focal=True))


@pytest.mark.parametrize('tag', list(R.RULES))
def test_compute_loss_accepts_every_rule_of_the_table(tag):
    from somi_amd._lib import LossBoxRule
    from somi_amd.loss import IOU_KINDS, ComputeLoss
    kw = dict(R.DEFAULTS, **R.RULES[tag])
    crit = ComputeLoss(R.Model(torch.rand(3, 3, 2) + 0.5, {}), **R.RULES[tag])
    r = crit.rule
    assert isinstance(r, LossBoxRule) and r.kind == IOU_KINDS[kw['iou']]
    assert (r.focal, r.inner, r.wiou_scaled) == (int(kw['focal']), int(kw['inner_ratio'] is not None), int(kw['wiou_scale']))
    assert (r.alpha, r.gamma, r.shape_scale) == (kw['alpha'], kw['gamma'], kw['shape_scale'])
    assert r.inner_ratio == np.float32(kw['inner_ratio'] or 0.0)
    assert crit.wiou_mean.dtype == torch.float64 and crit.wiou_mean.tolist() == [1.0] and crit.wiou_train is True


def test_signatures():
    from somi_amd.loss import WIOU_MOMENTUM, ComputeLoss
    from somi_amd.train import TrainStep
    sig = inspect.signature(ComputeLoss.__init__)
    assert list(sig.parameters)[1:] == ['model', 'autobalance', 'iou', 'focal', 'alpha', 'gamma', 'inner_ratio', 'shape_scale', 'wiou_scale']
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [False, 'CIoU', False, 1.0, 0.5, None, 0.5, False]
    assert inspect.signature(TrainStep.__init__).parameters['loss_kwargs'].default is None
    assert WIOU_MOMENTUM == 1 - 0.5 ** (1 / 7000) == R.WIOU_MOMENTUM


def test_box_rule_mirror_matches_the_library():
    from somi_amd import _lib
    from somi_amd._lib import LossBoxRule, LossDesc
    L = _lib.lib()
    assert L.somi_sizeof_desc(2) == ctypes.sizeof(LossBoxRule) == 4 * 4 + 4 * 4 + 8 + 4 + 4           # ... + tail padding to the pointer's alignment
    assert L.somi_sizeof_desc(1) == ctypes.sizeof(LossDesc) and L.somi_sizeof_desc(3) == 0           # the earlier indices stay
    assert [n for n, _ in LossBoxRule._fields_] == ['kind', 'focal', 'inner', 'wiou_scaled', 'alpha', 'gamma', 'inner_ratio', 'shape_scale',
                                                    'wiou_mean', 'wiou_train']
    assert LossBoxRule.wiou_mean.offset == 32 and LossBoxRule.wiou_train.offset == 40
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib._HERE)), 'include', 'somi_hip.h')).read()
    for name in ('somi_loss_box_rule', 'somi_loss_rule_workspace_bytes', 'somi_yolo_loss_rule_f32'):
        assert name in header and (name == 'somi_loss_box_rule' or hasattr(L, name))
    from somi_amd.loss import IOU_KINDS
    enum = header[header.index('enum somi_loss_iou_kind'):]
    enum = enum[:enum.index('}')]
    for name, val in IOU_KINDS.items():
        assert f'SOMI_LOSS_{name.upper()} = {val}' in enum
