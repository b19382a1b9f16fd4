"""fp64 restatement of ODConv's own arithmetic for the tests (models/common.py:4557-4590): the small dense layers of the attention heads
and their backward (csrc/train_odconv.hip), the per-sample weight synthesis and its backward, and the eval entry's heads + synthesis + fold
(csrc/layers.hip).  Plain torch, no import from somi_amd; tests/test_odconv_host.py pins it to the oracle's ODConv2d_3rd.

Every output comes as a pair (value, abs-term sum): the abs-term sum is the same expression with |.| of every factor and addend, the quantity
the README's gradient rule ("16 fp32 roundings of the gradient's own terms") is written in, so `within(got, value, abssum)` holds a kernel to
k = 16 roundings of 2^-24 of it, element by element.  Because every expression here is sums of products, the abs-term sum is the same code
run on the absolute values of its inputs.
  Behind an activation the pre-activation's sum is carried through the activation's Lipschitz constant (relu 1, sigmoid 1/4, softmax output o
2 y_o max_j of the pre-activation sums: |dy_o/dpre_j| = y_o |delta_oj - y_j| sums to 2 y_o (1 - y_o) over j), plus |y| / 4 for expf and the
division, which is 4 * 2^-24 |y| at k = 16.  Where an input carries a bar of its own (z behind the squeeze, the attention buffer inside the eval
entry) its sum is carried to the output to first order the same way: through |W| for a dense layer, through the other factors for a product.

Layouts are the kernels': rows (B, features); W (nout, nin) like nn.Linear; the attention row [a_f (Cout) | a_s (kk) | a_c (Cin) | a_w (K)];
Wk (K, Cout, kk, Cin), W_b / dW_b (B, Cout, kk, Cin), biask (K, Cout), bias_b (B, Cout).  The storage pad Cin_pad is the caller's (pad_c).

The case tables of tests/test_odconv_gpu.py live here with their seeded inputs, so that tests/test_odconv_host.py can hold the inputs themselves
to half the bar in fp32 on the CPU."""
import functools
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24                                                     # the unit of every bar: one fp32 rounding
ACTS = ('none', 'relu', 'sigmoid', 'softmax')


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().double()


def _cast(dtype, *ts):
    return [None if t is None else torch.as_tensor(t).detach().to(dtype) for t in ts]


def _abs(*ts):
    return [None if t is None else t.abs() for t in ts]


def within(got, ref, absum, what, k=16):
    """`got` finite and of `ref`'s shape, and |got - ref| <= k 2^-24 absum + 1e-30 at every element.  Prints and returns the worst error in
    units of 2^-24 absum (the bar is k of them) and where it is."""
    got, ref, absum = (torch.as_tensor(v).detach().cpu().double() for v in (got, ref, absum))
    assert got.shape == ref.shape == absum.shape, f'{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)} (abs-term sums {tuple(absum.shape)})'
    assert torch.isfinite(got).all(), f'{what}: not finite'
    err = (got - ref).abs()
    units = err / (U * absum + 1e-30 / k)
    worst = float(units.max()) if units.numel() else 0.0
    at = tuple(int(i) for i in torch.unravel_index(units.argmax(), units.shape)) if units.numel() else ()
    print(f'{what}: worst {worst:.2f} of {k} roundings at {at}')
    bad = err > k * U * absum + 1e-30
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.numel()} elements beyond {k} roundings of their terms, the worst {worst:.2f} at {at}: '
                           f'got {float(got[at]):.9e}, want {float(ref[at]):.9e}, abs-term sum {float(absum[at]):.3e}')
    return worst


# ---------------------------------------------------------------------------------------------------------------- the dense layers
def _activate(pre, a_pre, act):
    """(y, abs-term sum of y) from the pre-activation and its sum."""
    if act == 'none':
        return pre, a_pre
    if act == 'relu':
        return F.relu(pre), a_pre
    if act == 'sigmoid':
        y = torch.sigmoid(pre)
        return y, a_pre / 4 + y / 4
    if act == 'softmax':
        y = torch.softmax(pre, dim=-1)
        return y, 2 * y * a_pre.amax(dim=-1, keepdim=True) + y / 4
    raise ValueError(act)


def linear(x, W, bias, act, x_absum=None, dtype=torch.float64):
    """y = act(x W^T + bias) on rows.  x_absum: the abs-term sum of an x that is itself a rounded result."""
    x, W, bias, x_absum = _cast(dtype, x, W, bias, x_absum)
    pre = F.linear(x, W, bias)
    a_pre = F.linear(x.abs(), W.abs(), None if bias is None else bias.abs())
    if x_absum is not None:
        a_pre = a_pre + F.linear(x_absum, W.abs())
    return _activate(pre, a_pre, act)


def act_grad(dy, y, act):
    """d(pre-activation) by the kernels' rules, from the OUTPUT y: sigmoid y (1 - y), relu [y > 0], softmax y (dy - sum dy y).  -> (value, sum)."""
    if act == 'none':
        return dy, dy.abs()
    if act == 'relu':
        return dy * (y > 0), dy.abs() * (y > 0)
    if act == 'sigmoid':
        return dy * y * (1 - y), dy.abs() * y.abs() * (1 + y.abs())
    if act == 'softmax':
        return y * (dy - (dy * y).sum(-1, keepdim=True)), y.abs() * (dy.abs() + (dy.abs() * y.abs()).sum(-1, keepdim=True))
    raise ValueError(act)


def linear_grads(x, W, dy, y, act, dtype=torch.float64):
    """-> (dW, sum), (db, sum), (dx, sum) of y = act(x W^T + b) under dy, with the activation's gradient taken from the given y."""
    x, W, dy, y = _cast(dtype, x, W, dy, y)
    dpre, a_dpre = act_grad(dy, y, act)
    return ((dpre.t() @ x, a_dpre.t() @ x.abs()), (dpre.sum(0), a_dpre.sum(0)), (dpre @ W, a_dpre @ W.abs()))


# ---------------------------------------------------------------------------------------------------------------- the synthesis
def split_attn(attn, Cout, kk, Cin, K):
    assert attn.shape[-1] == Cout + kk + Cin + K
    return attn[..., :Cout], attn[..., Cout:Cout + kk], attn[..., Cout + kk:Cout + kk + Cin], attn[..., Cout + kk + Cin:]


def _outer(f, s, c):
    return f[:, :, None, None] * s[:, None, :, None] * c[:, None, None, :]


def fold(W, b, bn):
    """A following BatchNorm (bn_s, bn_t) folded into (value, sum) pairs of W_b and bias_b: W_b bn_s[n], bias_b bn_s + bn_t."""
    s, t = _cast(W[0].dtype, *bn)
    return (W[0] * s[None, :, None, None], W[1] * s.abs()[None, :, None, None]), (b[0] * s + t, b[1] * s.abs() + t.abs())


def synth(attn, Wk, biask, bn=None, attn_absum=None, dtype=torch.float64):
    """W_b[b,n,t,c] = a_f a_s a_c sum_q a_w[b,q] Wk[q,n,t,c], bias_b = a_w @ biask (zeros without biask); bn = (bn_s, bn_t): see fold.
    attn_absum: the sums of an attention buffer that is itself a rounded result, carried to first order (one factor at a time replaced by its
    own sum).  -> (W_b, sum), (bias_b, sum)."""
    attn, Wk, biask, attn_absum = _cast(dtype, attn, Wk, biask, attn_absum)
    K, Cout, kk, Cin = Wk.shape
    af, as_, ac, aw = split_attn(attn, Cout, kk, Cin, K)
    Wb = _outer(af, as_, ac) * torch.einsum('bq,qntc->bntc', aw, Wk)
    Ma = torch.einsum('bq,qntc->bntc', aw.abs(), Wk.abs())
    aWb = _outer(af.abs(), as_.abs(), ac.abs()) * Ma
    bb = abb = torch.zeros_like(af)
    if biask is not None:
        bb, abb = aw @ biask, aw.abs() @ biask.abs()
    if attn_absum is not None:
        Af, As, Ac, Aw = split_attn(attn_absum, Cout, kk, Cin, K)
        aWb = aWb + (_outer(Af, as_.abs(), ac.abs()) + _outer(af.abs(), As, ac.abs()) + _outer(af.abs(), as_.abs(), Ac)) * Ma
        aWb = aWb + _outer(af.abs(), as_.abs(), ac.abs()) * torch.einsum('bq,qntc->bntc', Aw, Wk.abs())
        if biask is not None:
            abb = abb + Aw @ biask.abs()
    W, b = (Wb, aWb), (bb, abb)
    return (W, b) if bn is None else fold(W, b, bn)


def _synth_grads_core(G, af, as_, ac, aw, Wk, biask, dbb):
    fb, sb, cb = af[:, :, None, None], as_[:, None, :, None], ac[:, None, None, :]
    GP = G * (fb * sb * cb)
    GM = G * torch.einsum('bq,qntc->bntc', aw, Wk)
    dWk = torch.einsum('bq,bntc->qntc', aw, GP)
    da_f = (GM * (sb * cb)).sum(dim=(2, 3))
    da_s = (GM * (fb * cb)).sum(dim=(1, 3))
    da_c = (GM * (fb * sb)).sum(dim=(1, 2))
    da_w = torch.einsum('bntc,qntc->bq', GP, Wk)
    dbiask = None
    if biask is not None:
        da_w = da_w + dbb @ biask.t()
        dbiask = aw.t() @ dbb
    return dWk, dbiask, da_f, da_s, da_c, da_w


def synth_grads(dWb, attn, Wk, biask, dbias_b, dtype=torch.float64):
    """The synthesis under dW_b (B, Cout, kk, Cin) and dbias_b (B, Cout; read only with biask).
    -> dict name -> (value, sum) for dWk, dbiask (None without biask), da_f, da_s, da_c, da_w."""
    dWb, attn, Wk, biask, dbias_b = _cast(dtype, dWb, attn, Wk, biask, dbias_b)
    K, Cout, kk, Cin = Wk.shape
    parts = split_attn(attn, Cout, kk, Cin, K)
    if biask is None:
        dbias_b = None
    val = _synth_grads_core(dWb, *parts, Wk, biask, dbias_b)
    ab = _synth_grads_core(*_abs(dWb, *parts, Wk, biask, dbias_b))
    return {n: (None if v is None else (v, a)) for n, v, a in zip(('dWk', 'dbiask', 'da_f', 'da_s', 'da_c', 'da_w'), val, ab)}


def squeeze(gap, fc_w, fc_b, dtype=torch.float64):
    """z = relu(fc_w gap + fc_b): the eval entry's first stage (a squeeze BatchNorm is folded into fc_w / fc_b by the caller)."""
    return linear(gap, fc_w, fc_b, 'relu', dtype=dtype)


def heads(gap, fc_w, fc_b, Wf, bf, Ws, bs, Wc, bc, Ww, bw, dtype=torch.float64):
    """The attention buffer of the eval entry: relu squeeze, three sigmoid heads, softmax over K.  -> (attn (B, Cout+kk+Cin+K), sum)."""
    z, a_z = squeeze(gap, fc_w, fc_b, dtype)
    outs = [linear(z, W, b, act, x_absum=a_z, dtype=dtype) for W, b, act in ((Wf, bf, 'sigmoid'), (Ws, bs, 'sigmoid'), (Wc, bc, 'sigmoid'),
                                                                             (Ww, bw, 'softmax'))]
    return torch.cat([o[0] for o in outs], dim=1), torch.cat([o[1] for o in outs], dim=1)


def pad_c(t, Cin_pad, fill=0.0):
    """(..., Cin) -> (..., Cin_pad) with `fill` in the pad channels."""
    out = torch.full(t.shape[:-1] + (Cin_pad,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


# ---------------------------------------------------------------------------------------------------------------- the per-sample conv
def conv_per_sample(x, w, bias, dy, k, s, dtype=torch.float64):
    """x (B,Cin,H,W), w (B,Cout,Cin,k,k), bias (B,Cout), dy (B,Cout,Ho,Wo): sample b convolved with its own weight set, pad k // 2, and autograd
    through it.  -> dict name -> (value, sum) for y, dx, dw; the sums are the same conv of the absolute values (+ |bias|)."""
    x, w, bias, dy = _cast(dtype, x, w, bias, dy)

    def run(x, w, bias, dy):
        x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = torch.cat([F.conv2d(x[b:b + 1], w[b], bias[b], s, k // 2) for b in range(x.shape[0])])
        y.backward(dy)
        return y.detach(), x.grad, w.grad
    val, ab = run(x, w, bias, dy), run(*_abs(x, w, bias, dy))
    return {n: (v, a) for n, v, a in zip(('y', 'dx', 'dw'), val, ab)}


# ---------------------------------------------------------------------------------------------------------------- case tables and inputs
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 3) * int(v) for i, v in enumerate(key)) + 1009)


def ident(case):
    return '-'.join(str(v) for v in case)


# a. linear forward: (B, nin, nout, act, bias)
LINEAR_CASES = [
    (3, 1, 1, 'none', True),                # one input, one output
    (1, 16, 255, 'sigmoid', True),          # thread per output: a workgroup not quite full
    (3, 16, 1024, 'sigmoid', True),         # the channel head at Cin = 1024: four 256-output trips, the upper limit
    (3, 32, 256, 'sigmoid', True),          # nin = 32: the last width of the thread-per-output path (hidden width at Cin = 512)
    (3, 32, 257, 'relu', True),             # ... one output in the second trip
    (3, 33, 257, 'sigmoid', True),          # nin = 33: first width of the wave-per-output path, 33 of 64 lanes busy
    (1, 33, 1, 'none', False),              # ... one output: three waves idle
    (3, 64, 1024, 'sigmoid', False),        # exactly one input per lane (hidden width at Cin = 1024), no bias
    (3, 65, 255, 'relu', True),             # a second lane trip with one input
    (3, 1000, 256, 'none', True),           # the squeeze at a wide input: 15 full lane trips and a tail of 40
    (1, 1000, 64, 'relu', False),
    (3, 16, 1, 'softmax', True),            # K = 1: the softmax of one logit
    (3, 32, 4, 'softmax', True),            # K = 4, the product's
    (1, 33, 8, 'softmax', False),
    (3, 64, 64, 'softmax', True),           # the softmax's upper limit
]


@functools.lru_cache(maxsize=None)
def linear_inputs(case):
    B, nin, nout, act, has_bias = case
    g = _gen(B, nin, nout, ACTS.index(act), has_bias)
    return types.SimpleNamespace(x=torch.randn(B, nin, generator=g), W=torch.randn(nout, nin, generator=g) / nin ** 0.5,
                                 bias=torch.randn(nout, generator=g) * 0.3 if has_bias else None, act=act)


def softmax_extreme_inputs():
    """Logits near +-90: exp of them overflows / underflows fp32 unless the row maximum is subtracted first."""
    g = torch.Generator().manual_seed(90)
    return types.SimpleNamespace(x=torch.randn(3, 16, generator=g), W=torch.randn(8, 16, generator=g) * 0.1,
                                 bias=torch.tensor([90.0, -90.0, 89.5, -88.0, 0.0, 45.0, 90.25, -90.0]), act='softmax')


# b. linear backward: (B, nin, nout, act, db, dx) with dx in None / 'write' / 'add'
LINEAR_BWD_CASES = [
    (1, 16, 256, 'sigmoid', True, 'write'),
    (3, 16, 9, 'sigmoid', True, 'add'),             # the spatial head
    (3, 32, 4, 'softmax', True, 'add'),             # the candidate head
    (17, 64, 64, 'softmax', True, 'write'),         # two 8-sample trips and a tail of one; softmax rows of a whole wave
    (17, 33, 257, 'relu', True, 'write'),           # exact zeros planted in y
    (3, 16, 32, 'none', False, None),               # neither db nor dx
    (3, 1000, 64, 'none', False, 'write'),          # the squeeze's own layer: no bias
    (3, 1024, 1024, 'sigmoid', True, 'add'),        # nin nout + nout > 2048 * 256: the weight kernel's second grid-stride trip
    (16, 1024, 16, 'relu', True, 'write'),          # B nin > 8192: the data kernel's second grid-stride trip
    (8, 65, 130, 'sigmoid', False, 'add'),          # exactly one 8-sample trip; dx sums of three lane trips
]


@functools.lru_cache(maxsize=4)
def linear_bwd_inputs(case):
    """x, W, dy and the fp32 y the backward reads (the fp64 forward, rounded; relu: exact zeros where the pre-activation is negative, and
    every seventh output planted to zero on top)."""
    B, nin, nout, act, _, _ = case
    g = _gen(B, nin, nout, ACTS.index(act), 77)
    c = types.SimpleNamespace(x=torch.randn(B, nin, generator=g), W=torch.randn(nout, nin, generator=g) / nin ** 0.5,
                              dy=torch.randn(B, nout, generator=g), act=act)
    c.y = linear(c.x, c.W, None, act)[0].float()
    if act == 'relu':
        c.y[:, ::7] = 0.0
        assert (c.y == 0).any() and (c.y > 0).any()
    return c


def attn_rows(g, B, Cout, kk, Cin, K):
    """An attention buffer whose rows differ by a factor of 8 from sample to sample: reading another sample's row is off by a factor."""
    return (0.1 + 0.8 * torch.rand(B, Cout + kk + Cin + K, generator=g)) * (0.125 ** torch.arange(B, dtype=torch.float32))[:, None]


# c. synthesis forward: (B, Cin, Cin_pad, Cout, kk, K)
SYNTH_CASES = [
    (1, 4, 4, 4, 1, 1),                     # smallest possible
    (3, 16, 16, 32, 9, 4),                  # the block test's shape
    (2, 12, 12, 20, 9, 4),
    (2, 10, 12, 8, 9, 4),                   # pad channels
    (2, 512, 512, 256, 1, 4),               # kk = 1
    (2, 1024, 1024, 256, 9, 4),             # widest: the grid-stride loop's second trip
    (2, 8, 8, 8, 49, 8),                    # kk = 49, K = 8
    (1, 8, 8, 8, 9, 16),                    # K = 16, the forward entries' upper limit
]
HIDDEN = dict(zip(SYNTH_CASES, (16, 32, 64, 16, 32, 64, 64, 16)))   # the eval entry's hidden width per case: each of 16 / 32 / 64 with a pad-free,
#                                                                     a wide and a small case


@functools.lru_cache(maxsize=2)
def synth_inputs(case):
    B, Cin, Cin_pad, Cout, kk, K = case
    g = _gen(*case)
    return types.SimpleNamespace(attn=attn_rows(g, B, Cout, kk, Cin, K), Wk=torch.randn(K, Cout, kk, Cin, generator=g) * (2.0 / (kk * Cout)) ** 0.5,
                                 biask=torch.randn(K, Cout, generator=g) * 0.2)


@functools.lru_cache(maxsize=2)
def eval_inputs(case):
    """The eval entry's inputs.  Sample b's pooled vector carries b along the all-ones direction, the first squeeze row reads it (z_0 ~ b, the
    other rows sum to zero), and every sigmoid head weighs z_0 by about -ln 8 below a bias of about -2: the samples' attention vectors differ by a
    factor of about 8 (test_odconv_host.py holds it between 4 and 16)."""
    B, Cin, Cin_pad, Cout, kk, K = case
    hid = HIDDEN[case]
    g = _gen(*case, hid)
    c = types.SimpleNamespace(hid=hid)
    c.gap = 0.3 * torch.randn(B, Cin, generator=g) + torch.arange(B, dtype=torch.float32)[:, None]
    c.fc_w = torch.randn(hid, Cin, generator=g) / Cin ** 0.5
    c.fc_w -= c.fc_w.mean(dim=1, keepdim=True)
    c.fc_w[0] = 1.0 / Cin
    c.fc_b = torch.randn(hid, generator=g) * 0.1
    c.fc_b[0] = 0.0
    for n, rows in (('f', Cout), ('s', kk), ('c', Cin), ('w', K)):
        W = torch.randn(rows, hid, generator=g) * 0.3 / hid ** 0.5
        if n != 'w':
            W[:, 0] = -2.08 + 0.1 * torch.randn(rows, generator=g)
        setattr(c, 'W' + n, W)
        setattr(c, 'b' + n, torch.randn(rows, generator=g) * 0.2 - (2.0 if n != 'w' else 0.0))
    c.Wk = torch.randn(K, Cout, kk, Cin, generator=g) * (2.0 / (kk * Cout)) ** 0.5
    c.biask = torch.randn(K, Cout, generator=g) * 0.2
    c.bn_s, c.bn_t = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3
    return c


def eval_head_args(c, with_fc_b):
    return (c.gap, c.fc_w, c.fc_b if with_fc_b else None, c.Wf, c.bf, c.Ws, c.bs, c.Wc, c.bc, c.Ww, c.bw)


# d. synthesis backward: name -> (B, Cin, Cin_pad, Cout, kk, K, biask)
SYNTH_BWD_CASES = {
    'smallest': (1, 4, 4, 1, 1, 1, True),
    'block': (3, 16, 16, 32, 9, 4, True),               # the block test's shape
    'cin12': (3, 12, 12, 4, 9, 4, False),
    'pad': (2, 10, 12, 4, 9, 4, True),                  # Cin_pad > Cin
    'cin252_K8': (1, 252, 252, 4, 9, 8, True),          # slot 0 not quite full; K at its limit
    'cin256_kk1': (3, 256, 256, 4, 1, 4, False),        # slot 0 exactly full
    'cin260_kk25': (1, 260, 260, 1, 25, 4, True),       # slot 1 with four lanes; one filter
    'cin512': (3, 512, 512, 256, 9, 4, True),           # slots 0 and 1 full: the 512 -> 256 site
    'cin1024': (2, 1024, 1024, 256, 9, 4, True),        # all four slots: the 1024 -> 256 site; the candidate kernel's grid-stride loop
    'kk49_K1': (3, 12, 12, 4, 49, 1, True),
    'cin1024_K8': (1, 1024, 1024, 4, 1, 8, False),
    'cin772_kk25': (3, 772, 772, 4, 25, 4, False),      # slot 3 with four lanes
}


@functools.lru_cache(maxsize=2)
def synth_bwd_inputs(case):
    B, Cin, Cin_pad, Cout, kk, K, has_bias = case
    g = _gen(*case, 5)
    c = types.SimpleNamespace(attn=attn_rows(g, B, Cout, kk, Cin, K), Wk=torch.randn(K, Cout, kk, Cin, generator=g) * (2.0 / (kk * Cout)) ** 0.5,
                              dWb=torch.randn(B, Cout, kk, Cin, generator=g), biask=None, dbias_b=None)
    if has_bias:
        c.biask, c.dbias_b = torch.randn(K, Cout, generator=g) * 0.2, torch.randn(B, Cout, generator=g) * 3.0
    return c


# e. per-sample conv: (B, H, W, Cin, Cout, k, s)
CONV_CASES = [
    (2, 27, 25, 64, 128, 3, 2),             # Ho Wo = 182: a full 128-row tile plus a ragged one per sample
    (5, 33, 31, 16, 32, 3, 1),              # 1023 rows per sample
    (3, 10, 10, 64, 64, 1, 1),              # ODConv_3rd's default k = 1
    (2, 9, 9, 512, 256, 3, 2),              # real site width
    (1, 7, 7, 1024, 256, 3, 2),             # real site width
    (3, 12, 12, 32, 48, 3, 2),              # the case of test_kernels_gpu.py, now also with the data gradient
]


@functools.lru_cache(maxsize=2)
def conv_inputs(case):
    """NCHW inputs; sample b's weight set is scaled by 4^b: a tile that takes another sample's set is off by a factor, not by noise."""
    B, H, W, Cin, Cout, k, s = case
    g = _gen(*case)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    scale = (4.0 ** torch.arange(B, dtype=torch.float32))[:, None, None, None, None]
    return types.SimpleNamespace(x=torch.randn(B, Cin, H, W, generator=g), w=torch.randn(B, Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5 * scale,
                                 bias=torch.randn(B, Cout, generator=g), dy=torch.randn(B, Cout, Ho, Wo, generator=g), k=k, s=s)
