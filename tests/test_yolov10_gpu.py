"""The YOLOv10 module set on the MI355X (C2f, SCDown, CIB, C2fCIB, AttentionPSA, PSA; models/hub/yolov10.yaml): the PSA attention kernels
against fp64 on the CPU, the blocks against torch autograd on the CPU restatement (tests/yolov10_ref.py), the whole graph against the
oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch

import yolov10_ref as R
from parity import check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, rel_close

pytestmark = pytest.mark.gpu


def _attn64(qkv, heads, dout=None, dv_add=None):
    """fp64 reference on (B, N, 128*heads) token rows: -> o (B, N, 64*heads), lse (B, heads, N) and, given dout, the qkv gradient."""
    qkv = qkv.double().requires_grad_(dout is not None)
    B, N, _ = qkv.shape
    t = qkv.view(B, N, heads, 128)
    q, k, v = t[..., :32], t[..., 32:64], t[..., 64:]
    s = torch.einsum('bihd,bjhd->bhij', q, k) * 32 ** -0.5
    lse = torch.logsumexp(s, -1)
    o = torch.einsum('bhij,bjhd->bihd', s.softmax(-1), v).reshape(B, N, 64 * heads)
    g = None
    if dout is not None:
        o.backward(dout.double())
        g = qkv.grad.clone()
        if dv_add is not None:
            g.view(B, N, heads, 128)[..., 64:] += dv_add.double().view(B, N, heads, 64)
    return o.detach(), lse.detach(), g


ACASES = [(1, 1, 1, 1), (2, 2, 5, 5), (1, 4, 13, 17), (2, 8, 20, 20), (1, 2, 40, 40), (3, 1, 7, 3)]


@pytest.mark.parametrize('case', ACASES, ids=lambda c: 'x'.join(map(str, c)))
def test_psa_attention_kernels(case):
    """Forward (output, log-sum-exp, the contiguous v copy) and backward (dq, dk, dv with the dv addend) against fp64, read from and
    written into channel slices of wider tensors; channels outside the written slices stay as they were; two launches are bit-identical."""
    from somi_amd import ops
    B, heads, H, W = case
    N = H * W
    gen = torch.Generator().manual_seed(sum(case))
    cq, co = 128 * heads, 64 * heads
    qkv_all = torch.randn(B, H, W, cq + 12, generator=gen)
    dout_all = torch.randn(B, H, W, co + 8, generator=gen)
    dv_add = torch.randn(B, H, W, co, generator=gen)
    qkv = qkv_all[..., 4:4 + cq].reshape(B, N, cq)
    o64, lse64, g64 = _attn64(qkv, heads, dout_all[..., 8:].reshape(B, N, co), dv_add.reshape(B, N, co))
    dev = 'cuda'
    qa, da, dva = qkv_all.to(dev), dout_all.to(dev), dv_add.to(dev)
    o_fill = torch.randn(B, H, W, co + 4, generator=gen)
    g_fill = torch.randn(B, H, W, cq + 8, generator=gen)

    def run():
        o = o_fill.clone().to(dev)
        _, lse, v = ops.psa_attention(qa, heads, qkv_coff=4, out=o, o_coff=4, lse=True, v_out=True)
        g = g_fill.clone().to(dev)
        ops.psa_attention_backward(qa, o, da, lse, heads, qkv_coff=4, o_coff=4, do_coff=8, out=g, g_coff=8, dv_add=dva)
        return o, lse, v, g

    o, lse, v, g = run()
    o2, lse2, v2, g2 = run()
    torch.cuda.synchronize()
    for a_, b_ in ((o, o2), (lse, lse2), (v, v2), (g, g2)):
        assert torch.equal(a_, b_), 'two launches differ'
    rel_close(o[..., 4:].reshape(B, N, co), o64, what='output')
    rel_close(lse, lse64, what='log-sum-exp')
    rel_close(v.reshape(B, N, heads, 64), qkv.view(B, N, heads, 128)[..., 64:], rel=0, what='v copy')
    gg = g[..., 8:].reshape(B, N, heads, 128).cpu()
    want = g64.view(B, N, heads, 128)
    for name, sl in (('dq', slice(0, 32)), ('dk', slice(32, 64)), ('dv', slice(64, 128))):
        rel_close(gg[..., sl], want[..., sl], what=name, atol=1e-5)   # N = 1: dq, dk are exactly 0, fp32 leaves P (dP - D) roundings
    assert torch.equal(o[..., :4].cpu(), o_fill[..., :4]), 'output channels outside the slice changed'
    assert torch.equal(g[..., :8].cpu(), g_fill[..., :8]), 'gradient channels outside the slice changed'


def test_psa_attention_large_logits():
    """q and k scaled so that exp of a raw score overflows fp32: the online max keeps everything finite and right."""
    from somi_amd import ops
    B, heads, H, W = 2, 2, 9, 11
    N = H * W
    gen = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, H, W, 128 * heads, generator=gen)
    t = qkv.view(B, H, W, heads, 128)
    t[..., :64] *= 12.0                                           # scores up to a few thousand: exp() of them is inf in fp32
    dout = torch.randn(B, H, W, 64 * heads, generator=gen)
    o64, lse64, g64 = _attn64(qkv.reshape(B, N, -1), heads, dout.reshape(B, N, -1))
    assert lse64.abs().max() > 200                                # a naive exp(score) overflows
    o, lse, _ = ops.psa_attention(qkv.cuda(), heads, lse=True)
    g = ops.psa_attention_backward(qkv.cuda(), o, dout.cuda(), lse, heads)
    rel_close(o.reshape(B, N, -1), o64, what='output')
    rel_close(lse, lse64, what='log-sum-exp')
    rel_close(g.reshape(B, N, -1), g64, rel=2e-3, what='qkv gradient')


BLOCKS = {'c2f_n1_sc': (lambda M: M.C2f(32, 32, 1, True), (2, 32, 9, 11)),
          'c2f_n2_sc': (lambda M: M.C2f(32, 32, 2, True), (2, 32, 10, 10)),
          'c2f_n1_nosc': (lambda M: M.C2f(24, 32, 1, False), (2, 24, 7, 9)),
          'c2f_n2_nosc': (lambda M: M.C2f(16, 48, 2, False), (3, 16, 8, 11)),
          'scdown_k3s2': (lambda M: M.SCDown(16, 32, 3, 2), (2, 16, 13, 17)),
          'cib': (lambda M: M.CIB(32, 32, True, e=1.0), (2, 32, 9, 7)),
          'cib_noadd': (lambda M: M.CIB(16, 32, True, e=1.0), (2, 16, 9, 7)),
          'c2fcib': (lambda M: M.C2fCIB(32, 32, 1, True), (2, 32, 9, 11)),
          'c2fcib_n2_nosc': (lambda M: M.C2fCIB(24, 32, 2, False), (2, 24, 8, 8)),
          'attnpsa': (lambda M: M.AttentionPSA(128, 2), (2, 128, 5, 7)),
          'psa': (lambda M: M.PSA(256, 256), (1, 256, 5, 7)),
          'psa_n156': (lambda M: M.PSA(128, 128), (2, 128, 12, 13))}


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_yolov10_blocks_eval_train_backward(tag):
    """Eval forward (BatchNorm folded), training forward, hand-written backward against torch autograd on the CPU restatement: output,
    dx, every parameter gradient (BatchNorm's included) and the updated running statistics."""
    mk, shape = BLOCKS[tag]
    check_block(mk, R, shape, tag)


def test_yolov10_graph_training_step_eval_and_checkpoint(monkeypatch):
    """yolov10 at width 0.25 / depth 0.33, batch 2, 160x160 (PSA sees N = 25) against the oracle Model: one training forward, ComputeLoss
    and backward (outputs, loss, every parameter gradient, BatchNorm statistics), the eval forward; two fresh TrainStep.step runs
    bit-identical; attempt_load of a pickled oracle model reproduces the eval forward."""
    from oracle.somi_ref import Model as OModel
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov10_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov10_cfg(0.25, 0.33)
    ref = fill_state(OModel(cfg), 3)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    ref.hyp = mine.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 160, nc=10, seed=2)
    check_train_step(ref, mine, imgs, targets, 'yolov10')
    check_eval(ref, mine, imgs, 'yolov10')
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'yolov10_ref'), 'yolov10')
