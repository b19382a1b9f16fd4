"""fp64 restatement of the pooling and attention pieces of the SOMI blocks for the tests: the global pools, the channel attention's MLP
(CBAM, models/common.py:339-358), SEAM's squeeze (:8483-8490), the spatial attention (:392-405) and the CBAM bottleneck's t -> t*ca*sa
(:686-688), plain PyTorch on NHWC tensors so that torch autograd runs through it.  tests/test_attention_ref_host.py pins it to the oracle's
own modules.  What the oracle's modules do not show and this keeps:
  - the maxima are taken the way the reference takes them: F.adaptive_max_pool2d(., 1) over pixels (nn.AdaptiveMaxPool2d(1)) and
    torch.max(., dim=1) over channels.  Autograd routes the gradient of a tied maximum to ONE index with both (the first one, which is
    numpy.argmax's documented rule); `amax`, which the oracle uses, splits it evenly among the ties.  The kernels implement the single-index rule.
  - every intermediate gradient of the backward steps A-F (the header of csrc/train_blocks.hip) is returned by name, so a kernel-level test can
    hold each step to autograd on its own.
Layouts are the kernels': tensors (B,H,W,C); pooled vectors (B,C); W1 (mid,C), W2 (C,mid) like nn.Linear; the k x k weight [k][k][2] (channel 0
the mean, 1 the max), its bias (1,); stats (B,H,W,2); sa / dlogit (B,H,W)."""
import numpy as np
import torch
import torch.nn.functional as F

ACTS = {'none': lambda v: v, 'silu': F.silu, 'gelu': F.gelu, 'relu': F.relu, 'sigmoid': torch.sigmoid, 'leaky': lambda v: F.leaky_relu(v, 0.1)}


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().double()


def _leaf(t):
    return None if t is None else f64(t).clone().requires_grad_(True)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------- forward
def global_pools(t):
    """(B,H,W,C) -> mean and max over pixels, (B,C) each."""
    x = _nchw(t.double())
    return x.mean(dim=(2, 3)), F.adaptive_max_pool2d(x, 1)[:, :, 0, 0]


def _mlp(v, W1, b1, W2, b2):
    return F.linear(F.relu(F.linear(v, W1, b1)), W2, b2)


def channel_attention(avg, mx, W1, b1, W2, b2):
    """mode 0: sigmoid(MLP(avg) + MLP(max)); the biases may be None."""
    return torch.sigmoid(_mlp(avg, W1, b1, W2, b2) + _mlp(mx, W1, b1, W2, b2))


def seam_scale(avg, W1, W2):
    """mode 1: exp(sigmoid(W2 relu(W1 avg)))."""
    return torch.exp(torch.sigmoid(_mlp(avg, W1, None, W2, None)))


def spatial_stats(t1):
    """(B,H,W,C) -> (B,H,W,2): [mean over channels, max over channels]."""
    x = _nchw(t1.double())
    return torch.stack([x.mean(dim=1), torch.max(x, dim=1).values], dim=-1)


def spatial_logit(stats, w, b, k):
    return F.conv2d(_nchw(stats), w.permute(2, 0, 1)[None].contiguous(), b, padding=k // 2)[:, 0]


def spatial_attention(stats, w, b, k):
    """sigmoid(conv_kxk(stats) + b) -> (B,H,W)."""
    return torch.sigmoid(spatial_logit(stats, w, b, k))


def cbam(t, W1, b1, W2, b2, w, b, k):
    """t -> t2 = t * ca * sa."""
    avg, mx = global_pools(t)
    ca = channel_attention(avg, mx, W1, b1, W2, b2)
    t1 = t.double() * ca[:, None, None, :]
    return t1 * spatial_attention(spatial_stats(t1), w, b, k)[..., None]


# ---------------------------------------------------------------------------------------------------------------- backward
def _cbam_graph(t, W1, b1, W2, b2, w, b, k):
    """cbam() with every intermediate kept (and its gradient retained)."""
    n = {}
    n['avg'], n['max'] = global_pools(t)
    n['ca'] = channel_attention(n['avg'], n['max'], W1, b1, W2, b2)
    n['t1'] = t * n['ca'][:, None, None, :]
    n['stats'] = spatial_stats(n['t1'])
    n['logit'] = spatial_logit(n['stats'], w, b, k)
    for v in n.values():
        v.retain_grad()
    n['sa'] = torch.sigmoid(n['logit'])
    n['t2'] = n['t1'] * n['sa'][..., None]
    return n


def argmax_channels(t1):
    """(B,H,W) int32: numpy.argmax over the channels (first occurrence)."""
    return torch.from_numpy(np.argmax(f64(t1).numpy(), axis=3).astype(np.int32))


def argmax_pixels(t):
    """(B,C) int32: numpy.argmax over the pixels h*W + w (first occurrence)."""
    a = f64(t).numpy()
    return torch.from_numpy(np.argmax(a.reshape(a.shape[0], -1, a.shape[3]), axis=1).astype(np.int32))


def _collect(n, t, W1, b1, W2, b2, w, b):
    g = lambda v: None if v is None else v.grad                                     # noqa: E731
    out = {k_: v.detach() for k_, v in n.items()}
    out.update(dlogit=n['logit'].grad, dstats=n['stats'].grad, dw=w.grad, db=b.grad, dt_c=n['t1'].grad * n['ca'].detach()[:, None, None, :],
               dca=n['ca'].grad, dW1=W1.grad, db1=g(b1), dW2=W2.grad, db2=g(b2), davg=n['avg'].grad, dmax=n['max'].grad, dt=t.grad,
               amaxc=argmax_channels(n['t1']), amaxp=argmax_pixels(t))
    return out


def cbam_grads(t, dt2, W1, b1, W2, b2, w, b, k):
    """One autograd run of cbam() under the output gradient dt2.  -> dict: the forward values avg, max, ca, t1, stats, logit, sa, t2 and
    dlogit (B,H,W); amaxc (B,H,W) int32 = numpy.argmax over channels of t*ca; amaxp (B,C) int32 = numpy.argmax over pixels of t; dstats; dw, db
    (the k x k conv's); dt_c = dt1 * ca (what step C writes); dca; dW1, db1, dW2, db2; davg, dmax; dt (after step F)."""
    t, W1, b1, W2, b2, w, b = (_leaf(v) for v in (t, W1, b1, W2, b2, w, b))
    n = _cbam_graph(t, W1, b1, W2, b2, w, b, k)
    n['t2'].backward(f64(dt2))
    return _collect(n, t, W1, b1, W2, b2, w, b)


def cbam_backward_steps(t, dt2, W1, b1, W2, b2, w, b, k):
    """dt by the step-by-step formulas A-F of csrc/train_blocks.hip, written out in fp64 without autograd (the forward values are recomputed
    from t).  -> dict with dlogit, amaxc, dstats, dw, db, dt_c, dca, amaxp, davg, dmax, dW1, db1, dW2, db2, dt."""
    t, dt2, W1, b1, W2, b2, w, b = (f64(v) for v in (t, dt2, W1, b1, W2, b2, w, b))
    B, H, W, C = t.shape
    avg, mx = global_pools(t)
    ca = channel_attention(avg, mx, W1, b1, W2, b2)
    t1 = t * ca[:, None, None, :]
    stats = spatial_stats(t1)
    sa = spatial_attention(stats, w, b, k)
    # A
    dlogit = (dt2 * t1).sum(-1) * sa * (1 - sa)
    amaxc = argmax_channels(t1)
    # B: the transposed conv, and the weight gradient tap by tap
    pad = k // 2
    wc = w.permute(2, 0, 1)[None]                                                  # (1,2,k,k)
    dstats = F.conv_transpose2d(dlogit[:, None], wc, padding=pad).permute(0, 2, 3, 1)
    sp = F.pad(_nchw(stats), (pad, pad, pad, pad))
    dw = torch.zeros(k, k, 2, dtype=torch.float64)
    for r in range(k):
        for q in range(k):
            dw[r, q] = (dlogit[:, None] * sp[:, :, r:r + H, q:q + W]).sum(dim=(0, 2, 3))
    db = dlogit.sum().reshape(1)
    # C
    onehot_c = F.one_hot(amaxc.long(), C).double()
    dt1 = dt2 * sa[..., None] + dstats[..., 0:1] / C + onehot_c * dstats[..., 1:2]
    dca = (dt1 * t).sum(dim=(1, 2))
    dt_c = dt1 * ca[:, None, None, :]
    # D
    amaxp = argmax_pixels(t)
    # E
    dpre = dca * ca * (1 - ca)                                                     # the gradient of BOTH MLP outputs (they are added)
    zero1 = torch.zeros(W1.shape[0], dtype=torch.float64) if b1 is None else b1
    ha, hm = F.linear(avg, W1, zero1), F.linear(mx, W1, zero1)
    dha, dhm = (dpre @ W2) * (ha > 0), (dpre @ W2) * (hm > 0)
    dW2 = dpre.t() @ (F.relu(ha) + F.relu(hm))
    db2 = 2 * dpre.sum(0)
    dW1 = dha.t() @ avg + dhm.t() @ mx
    db1 = (dha + dhm).sum(0)
    davg, dmax = dha @ W1, dhm @ W1
    # F
    onehot_p = F.one_hot(amaxp.long(), H * W).double().permute(0, 2, 1).reshape(B, H, W, C)
    dt = dt_c + davg[:, None, None, :] / (H * W) + onehot_p * dmax[:, None, None, :]
    return dict(dlogit=dlogit, amaxc=amaxc, dstats=dstats, dw=dw, db=db, dt_c=dt_c, dca=dca, amaxp=amaxp, davg=davg, dmax=dmax, dW1=dW1,
                db1=db1, dW2=dW2, db2=db2, dt=dt)


def attn_mlp_grads(mode, avg, mx, W1, b1, W2, b2, dout):
    """The MLP alone under the gradient dout of its output.  -> dict out, davg, dmax (None in mode 1), dW1, db1, dW2, db2."""
    avg, mx, W1, b1, W2, b2 = (_leaf(v) for v in (avg, mx, W1, b1, W2, b2))
    out = channel_attention(avg, mx, W1, b1, W2, b2) if mode == 0 else seam_scale(avg, W1, W2)
    out.backward(f64(dout))
    g = lambda v: None if v is None else v.grad                                     # noqa: E731
    return dict(out=out.detach(), davg=avg.grad, dmax=g(mx) if mode == 0 else None, dW1=W1.grad, db1=g(b1), dW2=W2.grad, db2=g(b2))


def seam_tail_grads(x, u, dout, W1, W2):
    """SEAM's tail: avg = mean over pixels of u (the DCovN output), sc = seam_scale(avg), y = x * sc.  -> dict avg, sc, y, dx (through the
    product only), dsc, dW1, dW2, davg and du = davg / HW at every pixel (the average-only pool backward)."""
    x, u, W1, W2 = (_leaf(v) for v in (x, u, W1, W2))
    avg = _nchw(u).mean(dim=(2, 3))
    sc = seam_scale(avg, W1, W2)
    avg.retain_grad(), sc.retain_grad()
    y = x * sc[:, None, None, :]
    y.backward(f64(dout))
    return dict(avg=avg.detach(), sc=sc.detach(), y=y.detach(), dx=x.grad, dsc=sc.grad, dW1=W1.grad, dW2=W2.grad, davg=avg.grad, du=u.grad)


def batchnorm_stats(y, gamma, beta, eps):
    """Training-mode BatchNorm over (B,H,W) as the kernels carry it: mean, rstd (biased variance), scale = gamma * rstd, shift = beta - mean * scale."""
    y, gamma, beta = f64(y), f64(gamma), f64(beta)
    mean = y.mean(dim=(0, 1, 2))
    rstd = 1.0 / torch.sqrt(y.var(dim=(0, 1, 2), unbiased=False) + eps)
    return mean, rstd, gamma * rstd, beta - mean * gamma * rstd


def _bn(y, gamma, beta, eps):
    mean = y.mean(dim=(0, 1, 2))
    var = ((y - mean) ** 2).mean(dim=(0, 1, 2))
    return (y - mean) / torch.sqrt(var + eps) * gamma + beta


def bn_silu_cbam_grads(y, gamma, beta, eps, dt2, W1, b1, W2, b2, w, b, k):
    """The fused form: t = silu(BatchNorm_batchstats(y)) in front of cbam().  -> cbam_grads' dict (of that t) plus t, dy, dgamma, dbeta."""
    y, gamma, beta, W1, b1, W2, b2, w, b = (_leaf(v) for v in (y, gamma, beta, W1, b1, W2, b2, w, b))
    t = F.silu(_bn(y, gamma, beta, eps))
    t.retain_grad()
    n = _cbam_graph(t, W1, b1, W2, b2, w, b, k)
    n['t2'].backward(f64(dt2))
    out = _collect(n, t, W1, b1, W2, b2, w, b)
    out.update(t=t.detach(), dy=y.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return out


def bn_act_pooled_grads(x, gamma, beta, eps, act, order, dz, davg, dmax, amaxp):
    """z = act(BN(x)) (order 0) or BN(act(x)) (order 1) with batch statistics, under dz (or None) plus the gradient of global pools over z:
    davg (B,C) of the mean over pixels, dmax (B,C) (or None) of the value at pixel amaxp (B,C).  -> dict dx, dgamma, dbeta."""
    x, gamma, beta = (_leaf(v) for v in (x, gamma, beta))
    z = ACTS[act](_bn(x, gamma, beta, eps)) if order == 0 else _bn(ACTS[act](x), gamma, beta, eps)
    B, H, W, C = z.shape
    zf = z.reshape(B, H * W, C)
    loss = (zf.mean(dim=1) * f64(davg)).sum()
    if dz is not None:
        loss = loss + (z * f64(dz)).sum()
    if dmax is not None:
        loss = loss + (torch.gather(zf, 1, torch.as_tensor(amaxp).long()[:, None, :])[:, 0] * f64(dmax)).sum()
    loss.backward()
    return dict(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
