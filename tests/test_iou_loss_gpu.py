"""The box-regression rules of the fused loss on the MI355X: every case x rule of tests/golden/iou_loss.npz (the reference's own functions,
tools/gen_iou_loss_golden.py), the WIoU running mean as device state, run-to-run bits, the default rule's bits, one differential case per
rule against the plain-torch restatement, and a TrainStep that was handed a rule.  Tolerances are those of tests/test_loss_wbf_gpu.py:
loss and items rel 1e-4, gradients per level |g - g_ref|_max <= 1e-3 |g_ref|_max + 1e-9."""
import numpy as np
import pytest
import torch

import iou_loss_ref as R
from parity import rel_close

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CASE_RULE = [(c, tag) for c, (_, _, tags) in R.CASES.items() for tag in tags]


def _hyp(case='a'):
    from somi_amd.configs import HYP_VISDRONE
    return dict(HYP_VISDRONE, **R.CASES[case][1])


def _inputs(g, case):
    src = R.CASES[case][0]
    nl = g[f'{src}_anchors'].shape[0]
    return T(g[f'{src}_anchors']), [T(g[f'{src}_p{i}']) for i in range(nl)], T(g[f'{src}_targets'])


def _grad_close(got, want, what):
    got, want = got.detach().cpu().double(), torch.as_tensor(want).double()
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    print(f'{what}: max err {err:.3e}, scale {scale:.3e}')
    assert torch.isfinite(got).all() and err <= 1e-3 * scale + 1e-9, f'{what}: max err {err:.3e} vs scale {scale:.3e}'


@pytest.mark.parametrize('case,tag', CASE_RULE)
def test_rule_matches_reference_fixture(golden, case, tag):
    from somi_amd.loss import ComputeLoss
    g = golden('iou_loss')
    anchors, p, tg = _inputs(g, case)
    crit = ComputeLoss(R.Model(anchors, _hyp(case)), **R.RULES[tag])
    scaled = bool(R.RULES[tag].get('wiou_scale'))
    pm = [t.cuda().requires_grad_(True) for t in p]
    loss, items = crit(pm, tg.cuda())
    rel_close(loss, g[f'{case}_{tag}_loss'], rel=1e-4, what=f'{case} {tag}: loss')
    rel_close(items, g[f'{case}_{tag}_items'], rel=1e-4, what=f'{case} {tag}: loss_items')
    loss.backward()
    for i, t in enumerate(pm):
        _grad_close(t.grad, g[f'{case}_{tag}_g{i}'], f'{case} {tag}: d loss / d p[{i}]')
    if scaled:                                                   # the running mean after each of three calls from 1.0, no host value in between
        means = [crit.wiou_mean.clone()]
        for _ in range(2):
            with torch.no_grad():                                # value-only calls move it too while wiou_train is set
                crit([t.detach() for t in pm], tg.cuda())
            means.append(crit.wiou_mean.clone())
        assert crit.wiou_mean.is_cuda and crit.wiou_mean.dtype == torch.float64
        np.testing.assert_allclose(torch.cat(means).cpu().numpy(), g[f'{case}_{tag}_wiou_mean'], rtol=1e-9)
        crit.wiou_mean.fill_(1.0)
    with torch.no_grad():                                        # value-only path (val.py:159-160)
        l2, it2 = crit([t.detach() for t in pm], tg.cuda())
    rel_close(l2, g[f'{case}_{tag}_loss'], rel=1e-4, what=f'{case} {tag}: loss (no grad)')
    rel_close(it2, g[f'{case}_{tag}_items'], rel=1e-4, what=f'{case} {tag}: loss_items (no grad)')
    if not scaled:
        assert crit.wiou_mean.tolist() == [1.0]                  # only scaled WIoU touches the state


@pytest.mark.parametrize('case', ['a', 'b', 'f'])
def test_wiou_state_frozen_when_not_training(golden, case):
    """wiou_train = False (WIoU_Scale._is_train): the mean keeps its bits, in gradient and value-only calls, and the factor is formed from it."""
    from somi_amd.loss import ComputeLoss
    g = golden('iou_loss')
    anchors, p, tg = _inputs(g, case)
    crit = ComputeLoss(R.Model(anchors, _hyp(case)), iou='WIoU', wiou_scale=True)
    crit.wiou_train = False
    crit.wiou_mean = torch.tensor([0.8125], dtype=torch.float64, device='cuda')
    before = crit.wiou_mean.clone()
    pm = [t.cuda().requires_grad_(True) for t in p]
    loss, items = crit(pm, tg.cuda())
    loss.backward()
    with torch.no_grad():
        l2, _ = crit([t.detach() for t in pm], tg.cuda())
    assert torch.equal(crit.wiou_mean, before)
    rel_close(l2, loss.detach(), rel=1e-6, what='value-only call against the call with gradients')
    state = R.WIoUState()
    state.mean, state.train = 0.8125, False
    pr = [t.double().requires_grad_(True) for t in p]
    want, want_items = R.restated_loss(anchors, _hyp(case), R.RULES['WIoU_scaled'], state)(pr, tg)
    want.backward()
    rel_close(loss, want.detach(), rel=1e-4, what='loss')
    rel_close(items, want_items, rel=1e-4, what='loss_items')
    for i, t in enumerate(pm):
        _grad_close(t.grad, pr[i].grad, f'd loss / d p[{i}]')


@pytest.mark.parametrize('tag', ['GIoU', 'EIoU_focal', 'SIoU_a3', 'CIoU_in0.7', 'shape', 'WIoU', 'WIoU_scaled'])
def test_two_calls_from_equal_state_give_equal_bits(golden, tag):
    """Case e (cells hit more than once): loss, items, every gradient and the WIoU state after the call."""
    from somi_amd.loss import ComputeLoss
    g = golden('iou_loss')
    anchors, p, tg = _inputs(g, 'e')
    runs = []
    for _ in range(2):
        crit = ComputeLoss(R.Model(anchors, _hyp('e')), **R.RULES[tag])
        pm = [t.cuda().requires_grad_(True) for t in p]
        loss, items = crit(pm, tg.cuda())
        loss.backward()
        runs.append([loss.detach(), items, crit.wiou_mean] + [t.grad for t in pm])
    assert torch.isfinite(runs[0][0]).all()
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_default_rule_keeps_its_bits(golden):
    """ComputeLoss(m), ComputeLoss(m, iou='CIoU') and an explicit alpha=1.0 are one computation: loss, items and gradients bit for bit on the
    loss family's own vector (four levels), on case d (five) and on case f's inputs with the NWD branch on."""
    from somi_amd.configs import HYP_VISDRONE
    from somi_amd.loss import ComputeLoss
    ga, gi = golden('loss_a'), golden('iou_loss')
    sets = [(T(ga['anchors']), [T(ga[f'p{i}']) for i in range(4)], T(ga['targets']), dict(HYP_VISDRONE), 10)]
    sets += [_inputs(gi, 'd') + (_hyp('d'), R.NC), _inputs(gi, 'f') + (_hyp('f'), R.NC)]
    for anchors, p, tg, hyp, nc in sets:
        runs = []
        for kw in ({}, dict(iou='CIoU'), dict(alpha=1.0), dict(iou='CIoU', focal=False, alpha=1.0, gamma=0.5, inner_ratio=None)):
            crit = ComputeLoss(R.Model(anchors, hyp, nc), **kw)
            pm = [t.cuda().requires_grad_(True) for t in p]
            loss, items = crit(pm, tg.cuda())
            loss.backward()
            with torch.no_grad():
                l2, it2 = crit([t.detach() for t in pm], tg.cuda())
            runs.append([loss.detach(), items, l2, it2] + [t.grad for t in pm])
        for other in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


@pytest.mark.parametrize('tag', list(R.RULES))
def test_rule_random_against_restatement(tag):
    """Differential: fresh random inputs at case (a)'s shape with near-duplicated targets, label smoothing and SlideLoss on (the level mean of
    the clamped similarity feeds both BCE terms), against the restatement in fp64."""
    from somi_amd.loss import ComputeLoss
    seed = 1000 + list(R.RULES).index(tag)
    anchors, p, tg = R.make_inputs((8, 4, 2), 40, seed, near_duplicates=True)
    hyp = dict(_hyp(), label_smoothing=0.1, slide_ratio=1.0)
    pr = [t.double().requires_grad_(True) for t in p]
    want, want_items = R.restated_loss(anchors, hyp, R.RULES[tag], R.WIoUState())(pr, tg)
    want.backward()
    pm = [t.cuda().requires_grad_(True) for t in p]
    got, items = ComputeLoss(R.Model(anchors, hyp), **R.RULES[tag])(pm, tg.cuda())
    rel_close(got, want.detach(), rel=1e-4, what=f'{tag}: loss')
    rel_close(items, want_items, rel=1e-4, what=f'{tag}: loss_items')
    got.backward()
    for i, t in enumerate(pm):
        _grad_close(t.grad, pr[i].grad, f'{tag}: d loss / d p[{i}]')


def test_train_step_forwards_its_rule():
    """TrainStep(loss_kwargs=dict(iou='SIoU')): the step's loss is ComputeLoss(iou='SIoU') on the same forward, and not the default rule's."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import fill_state, synthetic_batch
    from somi_amd.configs import HYP_VISDRONE, tiny_somi_cfg
    from somi_amd.loss import ComputeLoss
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    cfg = tiny_somi_cfg()
    state = fill_state(OModel(cfg), 4).state_dict()
    imgs, targets = synthetic_batch(2, 64, seed=3)
    losses = {}
    for name, kw in (('SIoU', dict(iou='SIoU')), ('default', {})):
        twin = Model(cfg)
        twin.load_state_dict(state)
        twin = twin.cuda().train()
        twin.hyp = dict(HYP_VISDRONE)
        losses[name] = ComputeLoss(twin, **kw)(twin(imgs.cuda()), targets.cuda())
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2, loss_kwargs=dict(iou='SIoU'))
    assert tr.compute_loss.rule.kind == 5
    loss, items = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all()
    assert torch.equal(loss, losses['SIoU'][0].detach()) and torch.equal(items, losses['SIoU'][1])
    assert not torch.equal(loss, losses['default'][0].detach())
