"""Efficient multi-scale attention on the MI355X (EMA, iRMB_EMA, iRMB_EMABottleneck, C2f_iRMB_EMA; ema.hip): the four kernels against the fp64
references of tests/ema_ref.py under the channel-slice contract (tests/slices.py: offsets and strides wider than the layer, three launches held
bit-identical, the accumulate forms), at POINT for pointwise results and REDUCED for sums over pixels; the blocks against torch autograd on the
CPU restatement; the yolov5s graphs of configs.yolov5_ema_cfg against the oracle Model.  The backward references are autograd of the LITERAL
formula (x11 = softmax(mean x1)); the kernels use mean x1 = gn.bias."""
import copy

import pytest
import torch

import ema_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nhwc,
                    rel_close)
from slices import In, Out, check_slice_op
from support_kernels_ref import POINT, REDUCED

pytestmark = pytest.mark.gpu

CASE_IDS = ['x'.join(map(str, c[0])) + '-' + c[1] for c in R.KERNEL_CASES]
_REFS = {}


def _case(case):
    """(inputs, fp64 reference) of a kernel case, computed once and shared; sg and the small vectors as the fp32 tensors the kernels read."""
    if case not in _REFS:
        shape, kind = case
        t = R.kernel_inputs(shape, kind)
        want = R.kernel_reference(t, shape[4])
        t['sg'], t['vec'] = want['sg'].float(), want['vec'].float().contiguous()
        N = shape[1] * shape[2]
        x21, x11 = want['vec'][:, 2], want['vec'][:, 3]
        c2 = (want['dx2'] - want['dw'] * x11[:, None, None])[:, 0, 0]
        want['bvec'] = torch.stack([c2, x21 * want['sums'][:, 1] / N, x21 * want['sums'][:, 0] / N], 1)
        t['bvec'], t['dw'] = want['bvec'].float().contiguous(), want['dw'].float()
        if N == 1:                                                # one pixel: the mean of t IS t and mean dx1 IS dx1, as fp32 numbers too - what the kernels in front leave
            t['vec'][:, 0] = t['x'][:, 0, 0] * t['sg'][:, 0] * t['sg'][:, 1]
            t['bvec'][:, 1], t['bvec'][:, 2] = t['vec'][:, 2] * t['dw'][:, 0, 0], 0.0
        _REFS[case] = (t, want)
    return _REFS[case]


@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=CASE_IDS)
def test_stats_and_gate_against_fp64(case):
    """ema_stats (mean and sum of squared deviations of t, the mean of x2; rstd and the two softmaxes) and ema_gate with a residual, every map a
    slice of a wider tensor.  'pooled50': the x2 means are ~50, a softmax without the maximum overflows; 'mean30': the mean of t is ~30 spreads."""
    from somi_amd import ops
    (B, H, W, C, g), kind = case
    t, want = _case(case)
    if (H, W) == (5, 7):                                          # the smallest map at which one (b, c) has two partials (two row chunks of 4)
        assert ops.ema_partials(B, H, W, C) == (4 if C == 256 else 2) and ops.ema_partials(B, 4, W, C) == (2 if C == 256 else 1)

    def run(b):
        stats, vec = ops.ema_stats(b['x'], b['sg'], C, g, b['gamma'], b['beta'], R.EPS, 4, sg_coff=4, x2=b['x2'], x2_coff=8)
        ops.ema_gate(b['x'], b['x2'], b['sg'], vec, C, g, b['gamma'], b['beta'], 4, x2_coff=8, sg_coff=4, res=b['res'], res_coff=0, out=b['out'],
                     o_coff=8)
        return dict(mean=stats[:, 0], m2=stats[:, 1], mx2=stats[:, 2], rstd=vec[:, 1], x21=vec[:, 2], x11=vec[:, 3], vec_mean=vec[:, 0])

    got = check_slice_op(run, dict(x=In(t['x'], C + 8, 4), x2=In(t['x2'], C + 16, 8), sg=In(t['sg'], C + 8, 4), res=In(t['res'], C + 4, 0),
                                   gamma=t['gamma'], beta=t['beta']),
                         dict(out=Out((B, H, W), C + 12, 8, C)),
                         dict(out=want['out_res'], mean=want['stats'][:, 0], m2=want['stats'][:, 1], mx2=want['stats'][:, 2], rstd=want['vec'][:, 1],
                              x21=want['vec'][:, 2], x11=want['vec'][:, 3], vec_mean=want['vec'][:, 0]),
                         rel=REDUCED, bars=dict(out=POINT), what=f'ema forward {CASE_IDS[R.KERNEL_CASES.index(case)]}')
    if H * W == 1:
        assert not got['m2'].any(), '1x1 map: the sum of squared deviations is not exactly zero'


def test_gate_without_a_residual_and_stats_without_x2():
    from somi_amd import ops
    case = R.KERNEL_CASES[0]
    (B, H, W, C, g), _ = case
    t, want = _case(case)
    d = {k: v.cuda() for k, v in t.items()}
    stats, vec = ops.ema_stats(d['x'], d['sg'], C, g, d['gamma'], d['beta'], R.EPS)
    assert not stats[:, 2].any(), 'no x2: its mean is zero'
    rel_close(stats[:, 1], want['stats'][:, 1], rel=REDUCED, what='m2 without x2')
    rel_close(ops.ema_gate(d['x'], d['x2'], d['sg'], d['vec'], C, g, d['gamma'], d['beta']), want['out'], rel=POINT, what='out without a residual')


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=CASE_IDS)
def test_backward_gate_against_fp64(case, accumulate):
    """ema_backward_gate: the direct part of dx (written, or added to what dx held), dwgt over the group's channels, the three sums per (b, c), the
    constants of the norm backward, and dgamma / dbeta added to what they held.  The constants are differences of the sums (c2 is a softmax
    backward over a group's S1 = gamma P + beta Q), so besides REDUCED of their own largest value they are allowed what they can inherit from sums
    that are right at their own bar, on the scale of the tensor they are added to: c2 lands on every pixel of dx2 = dwgt * x11 + c2 and gets
    POINT of max |dx2|; k1 and k2 land in dx1 - k1 - that * k2 and get POINT of max |dx1|, dx1 = dwgt * x21."""
    from somi_amd import ops
    (B, H, W, C, g), kind = case
    t, want = _case(case)
    cg = C // g
    gen = torch.Generator().manual_seed(5)
    dg0, db0 = torch.randn(cg, generator=gen), torch.randn(cg, generator=gen)
    dx1 = POINT * (want['dw'] * want['vec'][:, 2, None, None]).abs().max().item()

    def run(b):
        dg, db = dg0.clone().cuda(), db0.clone().cuda()
        _, _, sums, bvec = ops.ema_backward_gate(b['dout'], b['x'], b['x2'], b['sg'], b['vec'], C, g, b['gamma'], b['beta'], dg, db, 4, 4, x2_coff=8,
                                                 sg_coff=4, dx=b['dx'], dx_coff=8, accumulate=accumulate, dw=b['dw'], dw_coff=4)
        return dict(P=sums[:, 0], Q=sums[:, 1], R=sums[:, 2], c2=bvec[:, 0], k1=bvec[:, 1], k2=bvec[:, 2], dgamma=dg, dbeta=db)

    check_slice_op(run, dict(dout=In(t['dout'], C + 8, 4), x=In(t['x'], C + 8, 4), x2=In(t['x2'], C + 16, 8), sg=In(t['sg'], C + 8, 4),
                             vec=t['vec'], gamma=t['gamma'], beta=t['beta']),
                   dict(dx=Out((B, H, W), C + 12, 8, C, prev=t['have'] if accumulate else None, accumulate=accumulate),
                        dw=Out((B, H, W), C + 8, 4, C)),
                   dict(dx=want['dx'], dw=want['dw'], P=want['sums'][:, 0], Q=want['sums'][:, 1], R=want['sums'][:, 2], c2=want['bvec'][:, 0],
                        k1=want['bvec'][:, 1], k2=want['bvec'][:, 2], dgamma=want['dgamma'] + dg0.double(), dbeta=want['dbeta'] + db0.double()),
                   rel=REDUCED, bars=dict(dx=POINT, dw=POINT, c2=dict(rel=REDUCED, atol=POINT * want['dx2'].abs().max().item()),
                                          k1=dict(rel=REDUCED, atol=dx1), k2=dict(rel=REDUCED, atol=dx1)),
                   what=f'ema backward gate {CASE_IDS[R.KERNEL_CASES.index(case)]}')


@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=CASE_IDS)
def test_backward_norm_against_fp64(case):
    """ema_backward_norm: dt (the instance-norm backward), dx2 written over dwgt in place, and the gradient of conv1x1's output.  On a 1x1 map the
    variance is zero and dt and dsg are exactly zero."""
    from somi_amd import ops
    (B, H, W, C, g), kind = case
    t, want = _case(case)

    def run(b):
        ops.ema_backward_norm(b['x'], b['sg'], b['dw'], b['vec'], b['bvec'], C, g, b['gamma'], b['beta'], 4, sg_coff=4, dw_coff=8, dt=b['dt'],
                              dt_coff=4, dsg=b['dsg'], dsg_coff=0)

    got = check_slice_op(run, dict(x=In(t['x'], C + 8, 4), sg=In(t['sg'], C + 8, 4), vec=t['vec'], bvec=t['bvec'], gamma=t['gamma'], beta=t['beta']),
                         dict(dw=Out((B, H, W), C + 12, 8, C, prev=t['dw']), dt=Out((B, H, W), C + 8, 4, C), dsg=Out((B, H + W), C + 4, 0, C)),
                         dict(dw=want['dx2'], dt=want['dt'], dsg=want['dsg']),
                         rel=POINT, bars=dict(dsg=REDUCED), what=f'ema backward norm {CASE_IDS[R.KERNEL_CASES.index(case)]}')
    if H * W == 1:
        assert not got['dt'].any() and not got['dsg'].any(), '1x1 map: the norm\'s input gradient is not exactly zero'


@pytest.mark.parametrize('case', [((1, 9, 70, 16, 4), 'plain'), ((2, 1, 1, 32, 8), 'plain')], ids=['9x70', '1x1'])
def test_backward_chain_from_the_kernels_own_forward(case):
    """stats -> backward gate -> backward norm chained on the device (each kernel reading what the one before wrote): dx + dt * gates is
    autograd's input gradient, dx2 and dsg are autograd's, two chains are bit-identical.  On the 1x1 map dt and dsg are exactly zero."""
    from somi_amd import ops
    (B, H, W, C, g), _ = case
    t, want = _case(case)
    d = {k: v.cuda() for k, v in t.items()}
    runs = []
    for _ in range(2):
        _, vec = ops.ema_stats(d['x'], d['sg'], C, g, d['gamma'], d['beta'], R.EPS, x2=d['x2'])
        dg, db = torch.zeros(C // g, device='cuda'), torch.zeros(C // g, device='cuda')
        dx, dw, _, bvec = ops.ema_backward_gate(d['dout'], d['x'], d['x2'], d['sg'], vec, C, g, d['gamma'], d['beta'], dg, db)
        dt, dx2, dsg = ops.ema_backward_norm(d['x'], d['sg'], dw, vec, bvec, C, g, d['gamma'], d['beta'])
        runs.append(dict(dx_total=dx + dt * d['sg'][:, :H, None] * d['sg'][:, None, H:], dx2=dx2, dsg=dsg, dgamma=dg, dbeta=db))
        if H * W == 1:
            assert not dt.any() and not dsg.any(), '1x1 map: the norm\'s input gradient is not exactly zero'
    torch.cuda.synchronize()
    for k, v in runs[0].items():
        assert torch.equal(v, runs[1][k]), f'two chains differ in {k}'
        rel_close(v, want[k], rel=REDUCED if k in ('dsg', 'dgamma', 'dbeta') else POINT, what=f'chain {k}')


def test_refusals_raise_not_implemented():
    from somi_amd import ops
    z = lambda *s: torch.zeros(*s, device='cuda')                 # noqa: E731
    for C, g, word in ((36, 8, 'do not divide'), (16, 8, 'multiple of 4'), (1024, 8, 'at most 64')):
        with pytest.raises(NotImplementedError, match=word):
            ops.ema_stats(z(1, 2, 2, C), z(1, 4, C), C, g, z(max(C // g, 1)), z(max(C // g, 1)), 1e-5)


@pytest.mark.parametrize('tag', R.GPU_BLOCKS)
def test_blocks_eval_train_backward(tag):
    """EMA at 32 channels (cg = 4), 16 with factor 4 and 256 with factor 4 (cg = 64, the widest group), iRMB_EMA,
    the bottleneck with and without its shortcut and C2f_iRMB_EMA with two bottlenecks: eval forward, training forward, dx, every parameter
    gradient and the running statistics (parity.check_block)."""
    make, shape = R.BLOCKS[tag]
    check_block(make, R, shape, tag, seed=R.BLOCK_SEEDS[tag])


@pytest.mark.parametrize('tag', ['ema32', 'ema256_f4', 'irmb32', 'bottleneck32', 'c2f64_n2'])
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`, R what it held and dx what a plain backward of the same forward returns."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case(tag)
    c = x.shape[1]
    mine = R.BLOCKS[tag][0](MB)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda().train()
    xd = nhwc(x).cuda()
    y = mine(Act(xd.clone()))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    dx = mine.backward(Act(dy.clone()))
    dx = dx.t[..., dx.coff:dx.coff + c].clone()
    mine(Act(xd.clone()))
    have = torch.randn(xd.shape, generator=gen).cuda()
    before = have.clone()
    got = mine.backward(Act(dy.clone()), dx_out=Act(have), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have, before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')


@pytest.mark.parametrize('where', ['c2f', 'row'])
def test_ema_graph_training_step_eval_and_checkpoint(where, monkeypatch):
    """yolov5s 6.0 at width 0.5 with C2f_iRMB_EMA in the backbone ('c2f': 1, 2, 3 and 1 bottlenecks at hidden widths 32 .. 256) or an EMA row behind
    SPPF ('row', 512 channels, cg = 64), nc 10, batch 2, 64x64, against the oracle Model: one training forward, ComputeLoss and backward, the eval
    forward; two fresh TrainStep.step runs bit-identical; a pickled oracle model loads; a step moves EMA's parameters."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-ema-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-ema-{where}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'ema_ref'), f'yolov5s-ema-{where}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    moved = [k for k in state if k.endswith(('gn.weight', 'gn.bias', 'conv1x1.weight', 'conv1x1.bias', 'conv3x3.weight', 'conv3x3.bias'))]
    assert len(moved) == (6 * 7 if where == 'c2f' else 6)
    for k in moved:
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
