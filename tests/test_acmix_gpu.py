"""ACmix on the MI355X (acmix.hip): the attention kernels (forward, query-centred and key-centred backward) and the conv half (forward, data
and weight gradient, the fold of fc and dep_conv into one grouped weight and the split of its gradient) against the fp64 references of
tests/acmix_ref.py under the channel-slice contract (tests/slices.py: operands inside wider tensors at non-zero offsets, three launches held
bit-identical, the accumulate forms), at POINT for pointwise results and REDUCED for sums over pixels; the block against torch autograd on the CPU
restatement, with the rates fill_state draws and with both at 0.5; the yolov5s graphs of configs.yolov5_acmix_cfg against the oracle Model."""
import copy

import pytest
import torch

import acmix_ref as R
from parity import (bn_hyper, check_built_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nhwc,
                    rel_close)
from slices import In, Out, check_slice_op
from support_kernels_ref import POINT, REDUCED

pytestmark = pytest.mark.gpu

_REFS = {}


def _case(case):
    """(inputs, fp64 reference) of a kernel case, computed once and shared."""
    if case not in _REFS:
        t = R.kernel_inputs(*case)
        _REFS[case] = (t, R.kernel_reference(t))
    return _REFS[case]


def _qkv(t, C):
    """q, k, v as slices of ONE wider tensor, the way the block holds them: [8, 8 + C), [12 + C, 12 + 2 C), [16 + 2 C, 16 + 3 C) of 3 C + 16
    channels; the gaps between them hold NaN under every neighbour fill.  -> (In, (q_coff, k_coff, v_coff))."""
    gap = torch.full(tuple(t['q'].shape[:3]) + (4,), float('nan'))
    return In(torch.cat([gap, t['q'], gap, t['k'], gap, t['v']], -1), 3 * C + 16, 4), (8, 12 + C, 16 + 2 * C)


def test_the_tiled_case_has_two_ragged_tiles_on_both_axes():
    from somi_amd import ops
    _, H, W, _ = R.TILED_SHAPE
    tile, ny, nx = ops.acmix_plan(H, W)
    assert ny >= 2 and nx >= 2 and H % tile and W % tile, f'{R.TILED_SHAPE}: tile {tile}, {ny} x {nx} tiles'
    assert ops.acmix_plan(4, 4) == (tile, 1, 1)


@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=R.CASE_IDS)
def test_conv_half_and_attention_forward_against_fp64(case):
    """acmix_fold_weff, acmix_conv (the mix, with a bias) and acmix_attn with the mix in its epilogue and the log-sum-exp written."""
    from somi_amd import ops
    (B, H, W, C), kind = case
    t, want = _case(case)
    qkv, (qo, ko, vo) = _qkv(t, C)

    def run(b):
        weff = ops.acmix_fold_weff(b['fc'], b['dep'], C)
        ops.acmix_conv((b['qkv'], qo, ko, vo), C, weff, b['bias'], out=b['mix'], o_coff=4)
        ops.acmix_attn((b['qkv'], qo, ko, vo), C, b['wp'], b['rate1'], b['rate2'], mix=b['mix'], mix_coff=4, out=b['out'], o_coff=8, lse=b['lse'],
                       lse_coff=4)
        return dict(weff=weff)

    check_slice_op(run, dict(qkv=qkv, wp=t['wp'], fc=t['fc'], dep=t['dep'], bias=t['bias'], rate1=t['rate1'], rate2=t['rate2']),
                   dict(mix=Out((B, H, W), C + 8, 4, C), out=Out((B, H, W), C + 12, 8, C), lse=Out((B, H, W), 12, 4, 4)),
                   dict(mix=want['mix'], out=want['out'], lse=want['lse'], weff=want['weff']), rel=POINT,
                   what=f'acmix forward {R.CASE_IDS[R.KERNEL_CASES.index(case)]}')


def test_attention_without_a_mix_and_without_lse():
    from somi_amd import ops
    case = R.KERNEL_CASES[3]
    C = case[0][3]
    t, want = _case(case)
    d = {k: v.cuda() for k, v in t.items()}
    qkv = torch.cat([d['q'], d['k'], d['v']], -1)
    out, lse = ops.acmix_attn(qkv, C, d['wp'], d['rate1'], d['rate2'])
    assert lse is None
    rel_close(out, want['out_att'], rel=POINT, what='rate1 * att without a mix')


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('case', R.KERNEL_CASES, ids=R.CASE_IDS)
def test_attention_backward_against_fp64(case, accumulate):
    """acmix_attn_backward_q then acmix_attn_backward_kv (which reads what the first left in aux): dq, dk, dv written or added to what they held,
    dWp, drate1 = sum dout . att and drate2 = sum dout . mix."""
    from somi_amd import ops
    (B, H, W, C), kind = case
    t, want = _case(case)
    qkv, (qo, ko, vo) = _qkv(t, C)
    lse, mix = want['lse'].float(), want['mix'].float()
    prev = (lambda n: t['have_' + n] if accumulate else None)

    def run(b):
        src = (b['qkv'], qo, ko, vo)
        _, aux, dwp, drates = ops.acmix_attn_backward_q(b['dout'], src, C, b['wp'], b['rate1'], b['rate2'], b['lse'], do_coff=4, lse_coff=4,
                                                        mix=b['mix'], mix_coff=8, dq=b['dq'], dq_coff=4, accumulate=accumulate, aux=b['aux'],
                                                        aux_coff=4)
        ops.acmix_attn_backward_kv(b['dout'], src, C, b['wp'], b['rate1'], b['rate2'], b['lse'], aux, do_coff=4, lse_coff=4, aux_coff=4,
                                   dk=b['dk'], dk_coff=8, dv=b['dv'], dv_coff=0, accumulate=accumulate)
        return dict(dwp=dwp, drate1=drates[0:1], drate2=drates[1:2])

    got = check_slice_op(run, dict(qkv=qkv, dout=In(t['dout'], C + 8, 4), lse=In(lse, 12, 4), mix=In(mix, C + 12, 8), wp=t['wp'],
                                   rate1=t['rate1'], rate2=t['rate2']),
                         dict(dq=Out((B, H, W), C + 8, 4, C, prev=prev('q'), accumulate=accumulate),
                              dk=Out((B, H, W), C + 12, 8, C, prev=prev('k'), accumulate=accumulate),
                              dv=Out((B, H, W), C + 4, 0, C, prev=prev('v'), accumulate=accumulate),
                              aux=Out((B, H, W), 32, 4, 24)),
                         dict(dq=want['dq'], dk=want['dk'], dv=want['dv'], dwp=want['dwp'], drate1=want['drate1'],
                              drate2=(t['dout'].double() * want['mix']).sum().view(1), aux=lambda res: res['aux']),
                         rel=POINT, bars=dict(dwp=REDUCED, drate1=REDUCED, drate2=REDUCED),
                         what=f'acmix attention backward {R.CASE_IDS[R.KERNEL_CASES.index(case)]}')
    if kind == 'rate1_0' and not accumulate:
        assert not got['dq'].any() and not got['dk'].any() and not got['dv'].any(), 'rate1 = 0: the attention passes no gradient to q, k, v'


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('case', [c for c in R.KERNEL_CASES if c[1] in ('plain', 'rate2_0')], ids=lambda c: 'x'.join(map(str, c[0])) + '-' + c[1])
def test_conv_half_backward_against_fp64(case, accumulate):
    """acmix_conv_backward_data (into the three slices of one tensor), acmix_conv_backward_weight (the gradient of the folded weight and of the
    bias, rate2 included) and acmix_split_dweff (the gradients of fc.weight and dep_conv.weight)."""
    from somi_amd import ops
    (B, H, W, C), kind = case
    t, want = _case(case)
    qkv, (qo, ko, vo) = _qkv(t, C)
    have = torch.cat([t['have_q'], t['have_k'], t['have_v']], -1)

    def run(b):
        weff = ops.acmix_fold_weff(b['fc'], b['dep'], C)
        ops.acmix_conv_backward_data(b['dout'], C, weff, b['rate2'], (b['dqkv'], 4, 4 + C, 4 + 2 * C), do_coff=4, accumulate=accumulate)
        dweff, dbias = ops.acmix_conv_backward_weight(b['dout'], (b['qkv'], qo, ko, vo), C, b['rate2'], do_coff=4)
        dfc, ddep = ops.acmix_split_dweff(dweff, b['fc'], b['dep'], C)
        return dict(dweff=dweff, dbias=dbias, dfc=dfc, ddep=ddep)

    check_slice_op(run, dict(qkv=qkv, dout=In(t['dout'], C + 8, 4), fc=t['fc'], dep=t['dep'], rate2=t['rate2']),
                   dict(dqkv=Out((B, H, W), 3 * C + 8, 4, 3 * C, prev=have if accumulate else None, accumulate=accumulate)),
                   dict(dqkv=torch.cat([want['cq'], want['ck'], want['cv']], -1), dweff=want['dweff'], dbias=want['dbias'], dfc=want['dfc'],
                        ddep=want['ddep']),
                   rel=REDUCED, bars=dict(dqkv=POINT), what=f'acmix conv half backward {case}')


def test_refusals_raise():
    from somi_amd import ops
    z = lambda *s: torch.zeros(*s, device='cuda')                 # noqa: E731
    for C, word in ((24, 'C % 16 == 0'), (2048, 'at most 1024')):
        with pytest.raises(NotImplementedError, match=word):
            ops.acmix_attn(z(1, 4, 4, 3 * C), C, z(C // 4, 2), z(1), z(1))
    with pytest.raises(RuntimeError, match='reflection pad of 3'):
        ops.acmix_attn(z(1, 3, 5, 96), 32, z(8, 2), z(1), z(1))


def _built_pair(tag, rates):
    from somi_amd import blocks as MB
    ref, x, gen = R.block_case(tag, rates)
    mine = R.BLOCKS[tag][0](MB)
    mine.load_state_dict(ref.state_dict())
    return ref, mine, x, gen


@pytest.mark.parametrize('rates', R.RATES)
@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_block_eval_train_backward(tag, rates):
    """ACmix(32, 32) at 5x7, ACmix(16, 32) at 9x4 and ACmix(64, 64) on the minimal 4x4 map: eval forward, training forward, dx and every
    parameter gradient (parity.check_built_block) - conv_p.bias included, whose gradient is exactly zero here and rounding noise in autograd."""
    ref, mine, x, gen = _built_pair(tag, rates)
    check_built_block(ref, mine, x, gen, f'{tag}-{rates}')
    assert not mine.conv_p.bias.grad.any(), 'conv_p.bias cancels out of the scores: its gradient is exactly zero'


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`, R what it held and dx what a plain backward of the same forward
    returns (the procedure of parity.check_accumulate_contract, which itself takes only classes that declare `accumulates`)."""
    from somi_amd.blocks import Act
    _, mine, x, gen = _built_pair(tag, 'half')
    c = x.shape[1]
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
    mine(Act(xd.clone()))
    assert mine.backward(Act(dy.clone()), need_dx=False) is None


@pytest.mark.parametrize('where', ['row', 'p3'])
def test_acmix_graph_training_step_eval_and_checkpoint(where, monkeypatch):
    """yolov5s 6.0 at width 0.25, nc 4, batch 2 with an ACmix row behind SPPF ('row', 128x128: 256 channels on the minimal 4x4 map) or behind the P3
    head C3 ('p3', 64x64: 64 channels at 8x8), against the oracle Model: one training forward, ComputeLoss and backward, the eval forward; two
    fresh TrainStep.step runs bit-identical; a pickled oracle model loads; a step moves conv1, fc and conv_p and leaves the rates where they were."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-acmix-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-acmix-{where}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'acmix_ref'), f'yolov5s-acmix-{where}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    row = 10 if where == 'row' else 18
    for leaf in ('conv1.weight', 'fc.weight', 'conv_p.weight'):
        k = f'model.{row}.{leaf}'
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
    for leaf in ('rate1', 'rate2'):
        k = f'model.{row}.{leaf}'
        assert torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step moved {k}: the reference puts it in no optimizer group (train.py:125-133)'
