"""tests/attention_ref.py held to the oracle's own modules, to autograd's tie rule and to the step-by-step backward of csrc/train_blocks.hip.
CPU only, float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as R
from parity import nhwc, rel_close

# the size classes of tests/test_attention_kernels_gpu.py (B, H, W, C)
SIZES = [(1, 1, 1, 4), (2, 1, 7, 12), (2, 16, 16, 32), (3, 1, 257, 64), (2, 37, 29, 256), (8, 37, 29, 256), (1, 129, 129, 8), (1, 5, 7, 1028),
         (1, 3, 11, 2048)]


def close12(got, want, what):
    rel_close(got, want, rel=1e-12, what=what, atol=1e-13)


def params(g, C, mid, k):
    W1, b1 = torch.randn(mid, C, generator=g, dtype=torch.float64) / C ** 0.5, torch.randn(mid, generator=g, dtype=torch.float64) * 0.1
    W2, b2 = torch.randn(C, mid, generator=g, dtype=torch.float64) * 0.3, torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    w, b = torch.randn(k, k, 2, generator=g, dtype=torch.float64) * 0.2, torch.randn(1, generator=g, dtype=torch.float64) * 0.1
    return W1, b1, W2, b2, w, b


@pytest.mark.parametrize('B,H,W,C,mid,k', [(2, 9, 7, 32, 4, 7), (3, 5, 6, 16, 2, 3), (1, 4, 4, 8, 1, 5)])
def test_cbam_equals_the_oracle_modules_on_tie_free_inputs(B, H, W, C, mid, k):
    """Forward values and every gradient of attention_ref.cbam against ChannelAttentionModule / SpatialAttentionModule (amax there, single-index
    maxima here: the same function and gradient where no maximum is tied)."""
    from oracle.somi_ref import blocks as OB
    g = torch.Generator().manual_seed(C + k)
    t = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    dt2 = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    W1, b1, W2, b2, w, b = params(g, C, mid, k)
    cam, sam = OB.ChannelAttentionModule(C, C // mid).double(), OB.SpatialAttentionModule(k).double()
    with torch.no_grad():
        cam.shared_MLP[0].weight.copy_(W1), cam.shared_MLP[0].bias.copy_(b1)
        cam.shared_MLP[2].weight.copy_(W2), cam.shared_MLP[2].bias.copy_(b2)
        sam.cv1.weight.copy_(w.permute(2, 0, 1)[None]), sam.cv1.bias.copy_(b)
    x = t.permute(0, 3, 1, 2).clone().requires_grad_(True)
    ca = cam(x)
    x1 = ca * x
    sa = sam(x1)
    x2 = sa * x1
    x2.backward(dt2.permute(0, 3, 1, 2))
    r = R.cbam_grads(t, dt2, W1, b1, W2, b2, w, b, k)
    close12(R.cbam(t, W1, b1, W2, b2, w, b, k), nhwc(x2), 'cbam forward')
    close12(r['t2'], nhwc(x2), 't2')
    close12(r['ca'], ca[:, :, 0, 0], 'ca')
    close12(r['sa'], sa[:, 0], 'sa')
    close12(r['dt'], nhwc(x.grad), 'dt')
    close12(r['dW1'], cam.shared_MLP[0].weight.grad, 'dW1')
    close12(r['db1'], cam.shared_MLP[0].bias.grad, 'db1')
    close12(r['dW2'], cam.shared_MLP[2].weight.grad, 'dW2')
    close12(r['db2'], cam.shared_MLP[2].bias.grad, 'db2')
    close12(r['dw'], sam.cv1.weight.grad[0].permute(1, 2, 0), 'dw')
    close12(r['db'], sam.cv1.bias.grad, 'db')
    avg, mx = R.global_pools(t)
    close12(avg, x.detach().mean((2, 3)), 'avg')
    assert torch.equal(mx, x.detach().amax((2, 3))), 'max over pixels'
    st = R.spatial_stats(r['t1'])
    close12(st[..., 0], x1.detach().mean(1), 'mean over channels')
    assert torch.equal(st[..., 1], x1.detach().amax(1)), 'max over channels'


@pytest.mark.parametrize('B,H,W,C,red', [(2, 9, 7, 32, 16), (3, 4, 5, 16, 4)])
def test_seam_tail_equals_the_oracle_squeeze(B, H, W, C, red):
    """attention_ref.seam_tail_grads against SEAM's own avg_pool -> fc -> exp -> multiply (oracle.somi_ref.blocks.SEAM.forward, the DCovN output
    given), forward and every gradient."""
    from oracle.somi_ref import blocks as OB
    g = torch.Generator().manual_seed(C)
    seam = OB.SEAM(C, C, 1, red).double()
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    u = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    dout = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    with torch.no_grad():
        seam.fc[0].weight.copy_(torch.randn(seam.fc[0].weight.shape, generator=g, dtype=torch.float64) * 0.4)
        seam.fc[2].weight.copy_(torch.randn(seam.fc[2].weight.shape, generator=g, dtype=torch.float64) * 0.4)
    y = x * torch.exp(seam.fc(seam.avg_pool(u).view(B, C)).view(B, C, 1, 1))
    y.backward(dout)
    r = R.seam_tail_grads(nhwc(x.detach()), nhwc(u.detach()), nhwc(dout), seam.fc[0].weight, seam.fc[2].weight)
    close12(r['y'], nhwc(y), 'seam y')
    close12(r['dx'], nhwc(x.grad), 'seam dx')
    close12(r['du'], nhwc(u.grad), 'seam du')
    close12(r['dW1'], seam.fc[0].weight.grad, 'seam dW1')
    close12(r['dW2'], seam.fc[2].weight.grad, 'seam dW2')
    close12(r['du'], (r['davg'] / (H * W))[:, None, None, :].expand(B, H, W, C), 'du = davg / HW at every pixel')
    close12(r['dsc'], (nhwc(dout) * nhwc(x.detach())).sum((1, 2)), 'dsc')
    m = R.attn_mlp_grads(1, r['avg'], None, seam.fc[0].weight, None, seam.fc[2].weight, None, r['dsc'])
    close12(m['out'], r['sc'], 'mode 1 out')
    close12(m['davg'], r['davg'], 'mode 1 davg')
    close12(m['dW1'], r['dW1'], 'mode 1 dW1')
    close12(m['dW2'], r['dW2'], 'mode 1 dW2')


@pytest.mark.parametrize('B,H,W,C', SIZES, ids=[str(s) for s in SIZES])
def test_autograd_routes_a_tied_maximum_to_numpy_argmax(B, H, W, C):
    """On quantised inputs - round(clamp(randn, -1.5, 1.5)): three values, ties everywhere - the gradient of F.adaptive_max_pool2d(., 1) and of
    torch.max(., dim=1) is one-hot at numpy.argmax (first occurrence).  The GPU tests of the arg-max kernels rest on this."""
    g = torch.Generator().manual_seed(B * 1000 + C)
    t = torch.round(torch.clamp(torch.randn(B, H, W, C, generator=g), -1.5, 1.5)).double().requires_grad_(True)
    _, mx = R.global_pools(t)
    mx.sum().backward()
    want = F.one_hot(R.argmax_pixels(t).long(), H * W).permute(0, 2, 1).reshape(B, H, W, C)
    assert torch.equal(t.grad, want.double()), 'adaptive_max_pool2d: gradient not one-hot at the first maximal pixel'
    assert np.array_equal(R.argmax_pixels(t).numpy(), np.argmax(t.detach().numpy().reshape(B, H * W, C), axis=1))
    t.grad = None
    R.spatial_stats(t)[..., 1].sum().backward()
    want = F.one_hot(R.argmax_channels(t).long(), C)
    assert torch.equal(t.grad, want.double()), 'torch.max(dim=1): gradient not one-hot at the first maximal channel'
    if H * W > 1:
        assert (t.detach().reshape(B, H * W, C) == mx.detach()[:, None, :]).sum(1).max() > 1, 'the quantised input has no tied spatial maximum'


@pytest.mark.parametrize('kind', ['rand', 'ties'])
@pytest.mark.parametrize('B,H,W,C,mid,k', [(2, 9, 7, 32, 4, 7), (3, 1, 5, 12, 3, 3), (1, 1, 1, 4, 1, 5), (2, 18, 15, 8, 2, 5)])
def test_steps_a_to_f_reproduce_autograd(B, H, W, C, mid, k, kind):
    """The formulas A-F in the header of csrc/train_blocks.hip, in fp64, against autograd through attention_ref.cbam: every step's quantity, ties
    included (there the steps' numpy.argmax and autograd's routing must name the same index)."""
    g = torch.Generator().manual_seed(H * W + C)
    t = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    if kind == 'ties':
        t = torch.round(torch.clamp(t, -1.5, 1.5))
    dt2 = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    W1, b1, W2, b2, w, b = params(g, C, mid, k)
    if kind == 'ties':                                           # a constant ca: the channel ties survive the product
        W2, b2 = torch.zeros_like(W2), torch.full_like(b2, 0.25)
    want = R.cbam_grads(t, dt2, W1, b1, W2, b2, w, b, k)
    got = R.cbam_backward_steps(t, dt2, W1, b1, W2, b2, w, b, k)
    for name in ('amaxc', 'amaxp'):
        assert torch.equal(got[name], want[name]), name
    for name in ('dlogit', 'dstats', 'dw', 'db', 'dt_c', 'dca', 'davg', 'dmax', 'dW1', 'db1', 'dW2', 'db2', 'dt'):
        close12(got[name], want[name], name)


@pytest.mark.parametrize('act,order', [('silu', 0), ('gelu', 1)])
def test_fused_and_pooled_batchnorm_references_agree(act, order):
    """bn_silu_cbam_grads is cbam_grads behind a BatchNorm + SiLU: feeding its dt (all of steps A-F) to a plain BatchNorm backward gives its dy;
    bn_act_pooled_grads with (dt_c, davg, dmax, amaxp) gives the same dy - the two routes the kernels take."""
    g = torch.Generator().manual_seed(5 + order)
    B, H, W, C, mid, k, eps = 2, 6, 5, 16, 2, 3, 1e-3
    y = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 1.3 + 0.2
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    dt2 = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    W1, b1, W2, b2, w, b = params(g, C, mid, k)
    if (act, order) == ('silu', 0):
        r = R.bn_silu_cbam_grads(y, gamma, beta, eps, dt2, W1, b1, W2, b2, w, b, k)
        plain = R.cbam_grads(r['t'], dt2, W1, b1, W2, b2, w, b, k)
        close12(plain['dt'], r['dt'], 'dt')
        p = R.bn_act_pooled_grads(y, gamma, beta, eps, 'silu', 0, r['dt_c'], r['davg'], r['dmax'], r['amaxp'])
        for name in ('dy', 'dgamma', 'dbeta'):
            close12(p['dx' if name == 'dy' else name], r[name], name)
        mean, rstd, scale, shift = R.batchnorm_stats(y, gamma, beta, eps)
        close12(F.silu(y * scale + shift), r['t'], 't from scale / shift')
    else:
        dz = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
        davg, dmax = torch.randn(B, C, generator=g, dtype=torch.float64), torch.randn(B, C, generator=g, dtype=torch.float64)
        amaxp = torch.randint(0, H * W, (B, C), generator=g, dtype=torch.int32)
        p = R.bn_act_pooled_grads(y, gamma, beta, eps, act, order, dz, davg, dmax, amaxp)
        full = dz + davg[:, None, None, :] / (H * W) + F.one_hot(amaxp.long(), H * W).permute(0, 2, 1).reshape(B, H, W, C) * dmax[:, None, None, :]
        q = R.bn_act_pooled_grads(y, gamma, beta, eps, act, order, full, torch.zeros_like(davg), None, None)
        for name in ('dx', 'dgamma', 'dbeta'):
            close12(p[name], q[name], name)
