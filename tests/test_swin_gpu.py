"""The Swin module set on the MI355X (C3STR, SwinTransformerBlock / Layer, WindowAttention, Mlp; swin.hip): the window attention kernels and
the plain LayerNorm backward against fp64 on the CPU, the blocks against torch autograd on the CPU restatement (tests/swin_ref.py), the
whole yolov5s-transformer graph with C3STR against the oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import swin_ref as R
from parity import check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, rel_close

pytestmark = pytest.mark.gpu


def _attn64(qkv, table, heads, shift, dout):
    """fp64 einsum restatement of one layer's attention on the (B,H,W,3C) qkv map (channel = which*C + head*32 + d), padding, cyclic shift and
    shift mask included -> o (B,H,W,C), the largest score, d qkv, d table."""
    qkv, table = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    B, H, W, c3 = qkv.shape
    C = c3 // 3
    t = qkv.permute(0, 2, 1, 3)                                   # the layer's frame: (B, W, H, .)
    P1, P2 = -(-W // 8) * 8, -(-H // 8) * 8
    t = F.pad(t, (0, 0, 0, P2 - H, 0, P1 - W))                    # zero tokens: q = k = v = 0 (no qkv bias), still keys
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    w = R.to_windows(t)
    q, k, v = w.view(-1, 64, 3, heads, 32).permute(2, 0, 3, 1, 4)
    index = R.WindowAttention(32, (8, 8), 1).relative_position_index
    s = torch.einsum('bhid,bhjd->bhij', q * 32 ** -0.5, k) + table[index.view(-1)].view(64, 64, heads).permute(2, 0, 1)
    if shift:
        m = R.shift_mask(P1, P2, 8, shift).double()
        s = (s.view(B, m.shape[0], heads, 64, 64) + m[None, :, None]).view(-1, heads, 64, 64)
    o = torch.einsum('bhij,bhjd->bihd', s.softmax(-1), v).reshape(-1, 64, C)
    o = R.from_windows(o, B, P1, P2)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    o = o[:, :W, :H].permute(0, 2, 1, 3)
    o.backward(dout.double())
    return o.detach(), s.detach().max().item(), qkv.grad, table.grad


# (B, heads, H, W, shift, factor on q and k)
ACASES = [(1, 1, 8, 8, 0, 1.0), (1, 1, 8, 8, 4, 1.0), (2, 2, 12, 20, 4, 6.0), (1, 3, 5, 3, 4, 1.0), (2, 2, 16, 8, 0, 1.0), (1, 4, 20, 20, 4, 1.0)]


@pytest.mark.parametrize('case', ACASES, ids=lambda c: 'x'.join(map(str, c)))
def test_window_attention_kernels(case):
    """Forward and backward against fp64 with a random, asymmetric bias table: o, dq, dk, dv and the table gradient at 1e-3 of each
    quantity's largest value, no absolute slack (nothing here is analytically zero: every relative offset occurs in every window, padded keys
    included).  In the 6.0 case the largest score is beyond 88.7, where a naive exp(score) is inf in fp32.  Two launches are bit-identical."""
    from somi_amd import ops
    from somi_amd.blocks import swin_region_ids
    B, heads, H, W, shift, factor = case
    C = 32 * heads
    gen = torch.Generator().manual_seed(sum(case[:5]))
    qkv = torch.randn(B, H, W, 3 * C, generator=gen)
    qkv[..., :2 * C] *= factor
    table = torch.randn(225, heads, generator=gen)
    dout = torch.randn(B, H, W, C, generator=gen)
    o64, smax, g64, gt64 = _attn64(qkv, table, heads, shift, dout)
    if factor > 1:
        assert smax > 88.73, f'largest score {smax:.1f}: a naive exp would not overflow'
    ids = swin_region_ids((W + 7) // 8 * 8, (H + 7) // 8 * 8).cuda() if shift else None
    qd, td, dd = qkv.cuda(), table.cuda(), dout.cuda()

    def run():
        o, lse = ops.window_attention(qd, td, heads, shift, ids, lse=True)
        gt = torch.zeros(225, heads, device='cuda')
        g = ops.window_attention_backward(qd, td, dd, lse, heads, shift, ids, dtable=gt)
        return o, lse, g, gt

    first, second = run(), run()
    torch.cuda.synchronize()
    for a_, b_, name in zip(first, second, ('output', 'log-sum-exp', 'qkv gradient', 'table gradient')):
        assert torch.equal(a_, b_), f'two launches differ: {name}'
    o, _, g, gt = first
    rel_close(o, o64, what='output')
    for i, name in enumerate(('dq', 'dk', 'dv')):
        rel_close(g[..., i * C:(i + 1) * C], g64[..., i * C:(i + 1) * C], what=name)
    rel_close(gt, gt64, what='table gradient')
    o_eval, none = ops.window_attention(qd, td, heads, shift, ids)
    assert none is None and torch.equal(o_eval, o), 'the forward without the log-sum-exp differs'
    gt2 = torch.ones(225, heads, device='cuda')                   # the table gradient is accumulated
    ops.window_attention_backward(qd, td, dd, first[1], heads, shift, ids, dtable=gt2)
    rel_close(gt2, gt64 + 1, what='table gradient accumulated onto ones')


def test_window_attention_rejects_what_the_kernels_do_not_do():
    from somi_amd import ops
    t = torch.zeros(225, 1, device='cuda')
    with pytest.raises(NotImplementedError, match='head_dim 32'):
        ops.window_attention(torch.zeros(1, 8, 8, 3 * 48, device='cuda'), t, 1)
    with pytest.raises(RuntimeError, match='region-id'):
        ops.window_attention(torch.zeros(1, 8, 8, 96, device='cuda'), t, 1, 4)
    with pytest.raises(RuntimeError, match=r'\(225, 2\)'):
        ops.window_attention(torch.zeros(1, 8, 8, 192, device='cuda'), t, 2)


@pytest.mark.parametrize('C', [32, 256])
@pytest.mark.parametrize('npix', [1, 15, 1000])
def test_plain_layernorm_backward(C, npix):
    """du (with and without the added residual gradient), dgamma and dbeta against fp64 autograd; accumulated; two launches bit-identical."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(C + npix)
    u = torch.randn(1, 1, npix, C, generator=gen) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1
    dy, add = torch.randn(1, 1, npix, C, generator=gen), torch.randn(1, 1, npix, C, generator=gen)
    u64, g64, b64 = u.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(u64, (C,), g64, b64, 1e-5).backward(dy.double())
    ud, gd, dyd, addd = u.cuda(), gamma.cuda(), dy.cuda(), add.cuda()

    def run(add_):
        dg, db = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
        return ops.layernorm_backward(ud, gd, 1e-5, dyd, dg, db, add=add_), dg, db

    a, b = run(None), run(None)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two launches differ'
    rel_close(a[0], u64.grad, what='du')
    rel_close(a[1], g64.grad + 1, what='dgamma accumulated onto ones')
    rel_close(a[2], b64.grad, what='dbeta')
    rel_close(run(addd)[0], u64.grad + add.double(), what='du + add')


def test_gelu_backward():
    from somi_amd import ops
    gen = torch.Generator().manual_seed(3)
    u, dy = torch.randn(3, 5, 7, 128, generator=gen) * 2, torch.randn(3, 5, 7, 128, generator=gen)
    u64 = u.double().requires_grad_(True)
    F.gelu(u64).backward(dy.double())
    rel_close(ops.gelu_backward_(u.cuda(), dy.cuda()), u64.grad, what='gelu backward')


BLOCKS = {'c3str': (lambda M: M.C3STR(64, 64, 2), (1, 64, 12, 20)),
          'c3str_h2': (lambda M: M.C3STR(128, 128, 2, False), (1, 128, 16, 8)),
          'swinblock_small': (lambda M: M.SwinTransformerBlock(32, 32, 1, 2), (2, 32, 5, 3)),
          'c3str_n1': (lambda M: M.C3STR(64, 64, 1), (2, 64, 8, 8))}


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_swin_blocks_eval_train_backward(tag):
    """Eval forward, training forward, hand-written backward against torch autograd on the CPU restatement: output, dx, every parameter
    gradient (the bias tables' and the LayerNorms' included) and the BatchNorm statistics of the C3 shell."""
    mk, shape = BLOCKS[tag]
    check_block(mk, R, shape, tag)


def test_swin_graph_training_step_eval_and_checkpoint(monkeypatch):
    """yolov5s-transformer with C3STR at width 0.25 / depth 0.67 (two Swin layers, four heads), batch 2, 96x64 (P5 is 3x2: one heavily padded
    window) against the oracle Model: one training forward, ComputeLoss and backward, the eval forward; two fresh TrainStep.step runs
    bit-identical; a step leaves the bias tables where they were, as the reference's optimizer does; a pickled oracle model loads."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_swin_cfg
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg = yolov5_swin_cfg(0.25, 0.67, nc=10)
    ref = fill_state(OModel(cfg), 3)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    ref.hyp = mine.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 96, nc=10, seed=2)
    imgs = imgs[..., :64].contiguous()
    check_train_step(ref, mine, imgs, targets, 'yolov5-swin')
    check_eval(ref, mine, imgs, 'yolov5-swin')
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'swin_ref'), 'yolov5-swin')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    for _ in range(2):
        tr.step(imgs.cuda(), targets.cuda())
    tables = [k for k in state if k.endswith('relative_position_bias_table')]
    assert len(tables) == 2
    ema = tr.optimizer.ema_state_dict()
    for k in tables:
        assert torch.equal(m.state_dict()[k].cpu(), state[k]), f'{k} moved in an optimizer step'
        assert torch.equal(ema[k].cpu(), state[k]), f'the EMA of {k} is not the table'
    assert all(p.grad is None for p in tr.optimizer._ungrouped), 'zero_grad left the gradient of a parameter outside the groups'
    k = 'model.9.m.tr.1.norm1.weight'
    assert not torch.equal(m.state_dict()[k].cpu(), state[k]), 'the step left a LayerNorm weight where it was'
