"""tests/odconv_ref.py held to the oracle's ODConv2d_3rd (forward values and autograd through get_weight_bias, float64), and the condition on
the inputs of tests/test_odconv_gpu.py: for every case of that file the restatement evaluated in float32 on the CPU stays within half the
kernels' bar (8 of the 16 roundings), so the inputs themselves leave the kernels room.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import odconv_ref as R
from parity import rel_close


def close12(got, want, what):
    rel_close(got, want, rel=1e-12, what=what, atol=1e-14)


def packed(w, lead):
    """(lead.., Cout, Cin, k, k) -> (lead.., Cout, kk, Cin): the kernels' tap-major layout."""
    w = w.movedim(-3, -1)
    return w.reshape(*w.shape[:lead + 1], -1, w.shape[-1])


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('K', [1, 4])
@pytest.mark.parametrize('k', [1, 3])
def test_restatement_equals_the_oracle(k, K, B):
    """heads / synth / synth_grads / linear_grads against ODConv2d_3rd.attentions, get_weight_bias and autograd through both, with non-zero biases.
    The module runs in eval mode: its squeeze BatchNorm (skipped for one sample) is the fold the eval entry is handed."""
    from oracle.somi_ref import blocks as OB
    Cin, Cout, kk, H, W = 8, 12, k * k, 5, 6
    g = torch.Generator().manual_seed(100 * k + 10 * K + B)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                         # noqa: E731
    m = OB.ODConv2d_3rd(Cin, Cout, k, 1, k // 2, K=K).double().eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(rnd(*p.shape) * 0.5)
        m.bn.running_mean.copy_(rnd(*m.bn.running_mean.shape) * 0.2)
        m.bn.running_var.copy_(torch.rand(m.bn.running_var.shape, generator=g, dtype=torch.float64) + 0.5)
    hid = m.fc.weight.shape[0]
    if B > 1:
        s = (m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)).detach()
        t = (m.bn.bias - m.bn.running_mean * s).detach()
    else:
        s, t = torch.ones(hid, dtype=torch.float64), None
    x = rnd(B, Cin, H, W).requires_grad_(True)
    gap = x.detach().mean(dim=(2, 3))
    fcw = m.fc.weight.detach().flatten(1) * s[:, None]
    lins = (m.fc_f, m.fc_s, m.fc_c, m.fc_w)
    attn, a_attn = R.heads(gap, fcw, t, *(v.detach() for lin in lins for v in (lin.weight, lin.bias)))
    assert (a_attn > 0).all()
    a = m.attentions(x)
    for v in a:
        v.retain_grad()
    close12(attn, torch.cat(a, dim=1), 'heads')
    m.attentions = lambda context: a                               # get_weight_bias on the very tensors whose gradients are read below
    weight, bias = m.get_weight_bias(x)
    Wk = packed(m.weight.detach(), 1)
    (Wb, _), (bb, _) = R.synth(attn, Wk, m.bias.detach())
    close12(Wb, packed(weight.view(B, Cout, Cin, k, k), 1), 'synth W_b')
    close12(bb, bias.view(B, Cout), 'synth bias_b')
    dWb, dbb = rnd(B, Cout, kk, Cin), rnd(B, Cout)
    ((packed(weight.view(B, Cout, Cin, k, k), 1) * dWb).sum() + (bias.view(B, Cout) * dbb).sum()).backward()
    r = R.synth_grads(dWb, attn, Wk, m.bias.detach(), dbb)
    close12(r['dWk'][0], packed(m.weight.grad, 1), 'synth_grads dWk')
    close12(r['dbiask'][0], m.bias.grad, 'synth_grads dbiask')
    z = R.squeeze(gap, fcw, t)[0]
    dz = torch.zeros_like(z)
    for lin, n, y, act in zip(lins, ('da_f', 'da_s', 'da_c', 'da_w'), a, ('sigmoid', 'sigmoid', 'sigmoid', 'softmax')):
        close12(r[n][0], y.grad, f'synth_grads {n}')
        (dW, _), (db, _), (dx, _) = R.linear_grads(z, lin.weight.detach(), r[n][0], y.detach(), act)
        close12(dW, lin.weight.grad, f'linear_grads {act} dW ({n})')
        close12(db, lin.bias.grad, f'linear_grads {act} db ({n})')
        dz += dx
    (dfc, _), (dfb, _), (dgap, _) = R.linear_grads(gap, fcw, dz, z, 'relu')
    close12(dfc * s[:, None], m.fc.weight.grad.flatten(1), 'linear_grads relu dW through the fold')
    if B > 1:
        close12(dfb, m.bn.bias.grad, 'linear_grads relu db')
    close12((dgap / (H * W))[:, :, None, None].expand(B, Cin, H, W), x.grad, 'linear_grads relu dx, spread over the pixels')


def test_linear_and_its_gradients_equal_autograd_for_every_activation():
    g = torch.Generator().manual_seed(3)
    x, W, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((5, 7), (6, 7), (6,)))
    dy = torch.randn(5, 6, generator=g, dtype=torch.float64)
    fn = {'none': lambda v: v, 'relu': F.relu, 'sigmoid': torch.sigmoid, 'softmax': lambda v: torch.softmax(v, -1)}
    for act in R.ACTS:
        xl, Wl, bl = (v.clone().requires_grad_(True) for v in (x, W, b))
        y = fn[act](F.linear(xl, Wl, bl))
        y.backward(dy)
        got, absum = R.linear(x, W, b, act)
        close12(got, y, f'linear {act}')
        assert (absum >= 0).all()
        (dW, aW), (db, ab), (dx, ax) = R.linear_grads(x, W, dy, y.detach(), act)
        close12(dW, Wl.grad, f'{act} dW'), close12(db, bl.grad, f'{act} db'), close12(dx, xl.grad, f'{act} dx')
        assert (aW >= dW.abs() * (1 - 1e-12)).all() and (ab >= db.abs() * (1 - 1e-12)).all() and (ax >= dx.abs() * (1 - 1e-12)).all()


def test_abs_term_sums_equal_the_values_on_positive_inputs_and_the_fold_is_a_batchnorm():
    g = torch.Generator().manual_seed(4)
    B, Cin, Cout, kk, K = 2, 6, 5, 9, 3
    pos = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) + 0.1                      # noqa: E731
    attn, Wk, biask, dWb, dbb = pos(B, Cout + kk + Cin + K), pos(K, Cout, kk, Cin), pos(K, Cout), pos(B, Cout, kk, Cin), pos(B, Cout)
    for v, a in R.synth(attn, Wk, biask) + tuple(R.synth_grads(dWb, attn, Wk, biask, dbb).values()):
        assert torch.equal(v, a)
    assert R.synth_grads(dWb, attn, Wk, None, None)['dbiask'] is None
    assert not R.synth(attn, Wk, None)[1][0].any()
    # signs in: the sums dominate, and the fold is the eval BatchNorm behind the conv
    Wk, biask = Wk - 0.5, biask - 0.5
    s, t = pos(Cout), pos(Cout) - 0.5
    (Wb, aW), (bb, ab) = R.synth(attn, Wk, biask)
    (Wf, aWf), (bf, abf) = R.synth(attn, Wk, biask, bn=(s, t))
    assert (aW >= Wb.abs()).all() and (ab >= bb.abs()).all() and (aWf >= Wf.abs()).all() and (abf >= bf.abs() * (1 - 1e-12)).all()
    x = torch.randn(1, Cin, 4, 4, generator=g, dtype=torch.float64)
    w4 = lambda w: w[0].view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)                                 # noqa: E731
    close12(F.conv2d(x, w4(Wf), bf[0], 1, 1), F.conv2d(x, w4(Wb), bb[0], 1, 1) * s[None, :, None, None] + t[None, :, None, None], 'fold')
    # an attention buffer with sums of its own widens the output's sums, by the first-order term of each factor
    (_, aW2), (_, ab2) = R.synth(attn, Wk, biask, attn_absum=attn * 1e-3)
    close12(aW2, aW * (1 + 4e-3), 'first-order carry of the attention sums, W_b')
    close12(ab2, ab * (1 + 1e-3), 'first-order carry of the attention sums, bias_b')


# ------------------------------------------------------------------------------------------------------------- the condition on the inputs
HALF = 8                                                           # half of the kernels' 16 roundings


def within_half(got, pair, what):
    assert R.within(got, pair[0], pair[1], what, k=HALF) <= HALF


@pytest.mark.parametrize('case', R.LINEAR_CASES, ids=R.ident)
def test_inputs_linear(case):
    c = R.linear_inputs(case)
    within_half(R.linear(c.x, c.W, c.bias, c.act, dtype=torch.float32)[0], R.linear(c.x, c.W, c.bias, c.act), f'linear {case}')


def test_inputs_softmax_at_extreme_logits():
    c = R.softmax_extreme_inputs()
    ref = R.linear(c.x, c.W, c.bias, c.act)
    assert float(F.linear(c.x.double(), c.W.double(), c.bias.double()).abs().max()) > 88, 'the logits do not reach the range where expf overflows'
    within_half(R.linear(c.x, c.W, c.bias, c.act, dtype=torch.float32)[0], ref, 'softmax at logits near +-90')


@pytest.mark.parametrize('case', R.LINEAR_BWD_CASES, ids=R.ident)
def test_inputs_linear_backward(case):
    c = R.linear_bwd_inputs(case)
    f32, f64 = R.linear_grads(c.x, c.W, c.dy, c.y, c.act, dtype=torch.float32), R.linear_grads(c.x, c.W, c.dy, c.y, c.act)
    for n, a, b in zip(('dW', 'db', 'dx'), f32, f64):
        within_half(a[0], b, f'linear_grads {case} {n}')


@pytest.mark.parametrize('case', R.SYNTH_CASES, ids=R.ident)
def test_inputs_synthesis(case):
    c = R.synth_inputs(case)
    for n, a, b in zip(('W_b', 'bias_b'), R.synth(c.attn, c.Wk, c.biask, dtype=torch.float32), R.synth(c.attn, c.Wk, c.biask)):
        within_half(a[0], b, f'synth {case} {n}')
    e = R.eval_inputs(case)
    attn32 = R.heads(*R.eval_head_args(e, True), dtype=torch.float32)[0]
    attn, a_attn = R.heads(*R.eval_head_args(e, True))
    within_half(attn32, (attn, a_attn), f'heads {case}')
    B = case[0]
    if B > 1:                                                      # the samples' sigmoid rows differ by the factor the GPU test relies on
        ratio = attn[0, :-case[5]] / attn[1, :-case[5]]
        assert ratio.min() > 4 and ratio.max() < 16, f'sample 0 / sample 1 attention ratios {float(ratio.min()):.2f} .. {float(ratio.max()):.2f}'
    for n, a, b in zip(('W_b', 'bias_b'), R.synth(attn32, e.Wk, e.biask, bn=(e.bn_s, e.bn_t), dtype=torch.float32),
                       R.synth(attn, e.Wk, e.biask, bn=(e.bn_s, e.bn_t), attn_absum=a_attn)):
        within_half(a[0], b, f'heads + synth + fold {case} {n}')


@pytest.mark.parametrize('name', list(R.SYNTH_BWD_CASES))
def test_inputs_synthesis_backward(name):
    c = R.synth_bwd_inputs(R.SYNTH_BWD_CASES[name])
    f32, f64 = R.synth_grads(c.dWb, c.attn, c.Wk, c.biask, c.dbias_b, dtype=torch.float32), R.synth_grads(c.dWb, c.attn, c.Wk, c.biask, c.dbias_b)
    for n, b in f64.items():
        if b is not None:
            within_half(f32[n][0], b, f'synth_grads {name} {n}')


@pytest.mark.parametrize('case', R.CONV_CASES, ids=R.ident)
def test_inputs_per_sample_conv(case):
    c = R.conv_inputs(case)
    f32, f64 = R.conv_per_sample(c.x, c.w, c.bias, c.dy, c.k, c.s, dtype=torch.float32), R.conv_per_sample(c.x, c.w, c.bias, c.dy, c.k, c.s)
    for n, b in f64.items():
        within_half(f32[n][0], b, f'per-sample conv {case} {n}')
