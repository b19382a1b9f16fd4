"""ODConv's own kernels one by one - the dense layers of the attention heads and their backward, the per-sample weight synthesis and its
backward (csrc/train_odconv.hip), the eval entry (heads + synthesis + fold, csrc/layers.hip) - and the per-sample-weight mode of the
implicit-GEMM conv, against tests/odconv_ref.py in fp64 at the sizes where their thread mappings change, then the block at the product's widths.
The bar is odconv_ref.within: every element within 16 fp32 roundings of its own abs-term sum.  Every call runs twice from equal inputs and must
repeat bit for bit; buffers a call overwrites start as NaN, buffers it adds to start from noise of the gradient's size and the added part is
compared (its abs-term sum then has the start as one more addend); a slice of a wider row leaves the rest of the row bit-unchanged.
The cases and their inputs live in odconv_ref.py; tests/test_odconv_host.py holds those inputs to half the bar in fp32 on the CPU."""
import pytest
import torch

import odconv_ref as R
from parity import check_built_block, nhwc

pytestmark = pytest.mark.gpu
EINVAL = -1
NAN = float('nan')


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def nans(*shape):
    return torch.full(shape, NAN, device=dev())


def twice(fn):
    """fn() twice from equal inputs: every output tensor bit-identical; -> the first run's outputs."""
    a = fn()
    torch.cuda.synchronize()
    b = fn()
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert (p is None and q is None) or torch.equal(p, q), f'output {i} differs between two runs from equal inputs'
    return a


def same_bits(a, b, what):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: bits changed'


def like_scaled(ref, seed, per_sample=False):
    """A non-zero start for an accumulated gradient, of the gradient's own size (per sample where the samples' sizes differ on purpose)."""
    ref = R.f64(ref)
    scale = ref.abs().amax(dim=tuple(range(1, ref.dim())), keepdim=True) if per_sample else ref.abs().max()
    return (torch.randn(ref.shape, generator=torch.Generator().manual_seed(seed)).double() * (scale + 1e-6)).float()


def added(buf, start, pair, what):
    """The part a kernel added to a buffer that started at `start`, against (value, sum): the start is one more addend of the expression."""
    return R.within(buf.cpu().double() - start.double(), pair[0], pair[1] + start.double().abs(), what)


def wide_rows(t, off, after, fill=NAN):
    """t (B, n) in columns [off, off + n) of wider rows of `fill`."""
    out = torch.full((t.shape[0], off + t.shape[1] + after), fill)
    out[:, off:off + t.shape[1]] = t
    return out


def api():
    from somi_amd import _lib
    from somi_amd.ops import ACT, _ptr, _stream
    return _lib.lib(), ACT, _ptr, _stream


# ------------------------------------------------------------------------------------------------------------------- a. linear forward
def raw_linear(x, ldx, W, bias, act, y, ldy, y_off, B, nin, nout):
    L, ACT, p, stream = api()
    return L.somi_linear_f32(p(x), ldx, p(W), p(bias), ACT[act], p(y), ldy, y_off, B, nin, nout, stream())


@pytest.mark.parametrize('case', R.LINEAR_CASES, ids=R.ident)
def test_linear(case):
    from somi_amd import ops
    d = dev()
    B, nin, nout, act, _ = case
    c = R.linear_inputs(case)
    ref = R.linear(c.x, c.W, c.bias, act)
    xd, Wd, bd = c.x.to(d), c.W.to(d), None if c.bias is None else c.bias.to(d)
    y, = twice(lambda: (ops.linear(xd, Wd, bd, act, out=nans(B, nout)),))
    R.within(y, *ref, f'linear {case}')
    if act == 'softmax':
        assert (y.cpu().double().sum(1) - 1).abs().max() <= 4 * R.U * nout, 'softmax rows do not sum to 1'
    # x read from wider rows (NaN behind nin), y written into columns [7, 7 + nout) of wider rows
    xw, start = wide_rows(c.x, 0, 3).to(d), torch.randn(B, 7 + nout + 5, generator=torch.Generator().manual_seed(nout))

    def run():
        out = start.to(d)
        assert raw_linear(xw, nin + 3, Wd, bd, act, out, out.shape[1], 7, B, nin, nout) == 0
        return (out,)
    out, = twice(run)
    same_bits(out[:, 7:7 + nout], y, 'the slice form against the plain one')
    same_bits(out[:, :7], start[:, :7], 'columns in front of the slice')
    same_bits(out[:, 7 + nout:], start[:, 7 + nout:], 'columns behind the slice')


def test_linear_softmax_subtracts_the_maximum():
    """Logits near +-90: exp of them overflows / underflows fp32 unless the row maximum is subtracted first."""
    from somi_amd import ops
    d = dev()
    c = R.softmax_extreme_inputs()
    x, W, bias = c.x, c.W, c.bias
    y, = twice(lambda: (ops.linear(x.to(d), W.to(d), bias.to(d), 'softmax', out=nans(3, 8)),))
    R.within(y, *R.linear(x, W, bias, 'softmax'), 'softmax at logits near +-90')
    assert (y.cpu().double().sum(1) - 1).abs().max() <= 4 * R.U * 8, 'softmax rows do not sum to 1'
    assert (y[:, [0, 2, 6]] > 0.05).all()


def test_linear_rejections_write_nothing():
    L = api()[0]
    d = dev()
    x, W, b = torch.randn(2, 16, device=d), torch.randn(1025, 16, device=d), torch.randn(1025, device=d)
    for what, act, ldy, y_off, nout in (('nout = 1025', 'sigmoid', 1100, 0, 1025), ('softmax with nout = 65', 'softmax', 1100, 0, 65),
                                        ('ldy < y_off + nout', 'sigmoid', 40, 9, 32)):
        y = nans(2, 1100)
        assert raw_linear(x, 16, W, b, act, y, ldy, y_off, 2, 16, nout) == EINVAL, what
        assert L.somi_last_error().decode().startswith('linear: bad'), what
        torch.cuda.synchronize()
        assert torch.isnan(y).all(), f'{what}: rejected, but y was written'


# ------------------------------------------------------------------------------------------------------------------- b. linear backward
def raw_linear_bwd(x, W, dy, y, ld, off, act, dW, db, dx, accumulate, ws, B, nin, nout):
    L, ACT, p, stream = api()
    return L.somi_linear_bwd_f32(p(x), nin, p(W), p(dy), p(y), ld, off, ACT[act], p(dW), p(db), p(dx), nin, int(accumulate), p(ws), B, nin, nout, stream())


@pytest.mark.parametrize('case', R.LINEAR_BWD_CASES, ids=R.ident)
def test_linear_backward(case):
    """dy and y are read at columns [5, 5 + nout) of wider rows (NaN elsewhere), as the block reads dattn / attn."""
    from somi_amd import ops
    d = dev()
    B, nin, nout, act, has_db, dx_mode = case
    c = R.linear_bwd_inputs(case)
    dW, db, dx = R.linear_grads(c.x, c.W, c.dy, c.y, act)
    xd, Wd, dyw, yw = c.x.to(d), c.W.to(d), wide_rows(c.dy, 5, 3).to(d), wide_rows(c.y, 5, 3).to(d)
    dW0, db0 = like_scaled(dW[0], 1), like_scaled(db[0], 2) if has_db else None
    dx0 = like_scaled(dx[0], 3) if dx_mode == 'add' else None

    def start():
        return (dW0.to(d), None if db0 is None else db0.to(d), None if dx_mode is None else nans(B, nin) if dx0 is None else dx0.to(d))

    def run():
        gW, gb, gx = start()
        ws = nans(B * nout)
        assert raw_linear_bwd(xd, Wd, dyw, yw, yw.shape[1], 5, act, gW, gb, gx, dx_mode == 'add', ws, B, nin, nout) == 0
        return gW, gb, gx, ws
    gW, gb, gx, ws = twice(run)
    tag = f'linear_backward {case}'
    R.within(ws.view(B, nout), *R.act_grad(c.dy.double(), c.y.double(), act), f'{tag} d(pre-activation), the workspace')
    added(gW, dW0, dW, f'{tag} dW')
    if has_db:
        added(gb, db0, db, f'{tag} db')
    if dx_mode == 'write':
        R.within(gx, *dx, f'{tag} dx')
    elif dx_mode == 'add':
        added(gx, dx0, dx, f'{tag} dx, added')
    if act == 'relu':                                              # where y is exactly 0 nothing flows: not a small number, nothing
        dead = c.y == 0
        assert not ws.view(B, nout).cpu()[dead].any(), 'relu: a gradient where y == 0'
        cols = dead.all(dim=0)
        assert cols.any()
        same_bits(gW[cols], dW0[cols], 'relu: dW rows of outputs that are 0 for every sample')
        same_bits(gb[cols], db0[cols], 'relu: db of outputs that are 0 for every sample')
    # the same through ops.linear_backward (its own workspace)
    oW, ob, ox = start()
    ops.linear_backward(xd, Wd, dyw, yw, 5, act, oW, ob, ox, accumulate=dx_mode == 'add')
    for a, b, n in ((oW, gW, 'dW'), (ob, gb, 'db'), (ox, gx, 'dx')):
        assert (a is None and b is None) or torch.equal(a, b), f'{tag}: ops.linear_backward {n} differs from the direct call'


# ------------------------------------------------------------------------------------------------------------------- c. synthesis forward
JUNK = 3.0                                                         # what the pad channels of Wk / dW_b hold: finite, and never to be seen


def packed_k(t, Cin_pad, fill=0.0):
    """(K or B, Cout, kk, Cin) -> (., Cout, kk * Cin_pad) with `fill` in the pad channels."""
    return R.pad_c(t, Cin_pad, fill).flatten(2).contiguous()


def raw_synth(attn, Wk, biask, wout, bout, B, Cin, Cin_pad, Cout, kk, K):
    L, _, p, stream = api()
    return L.somi_odconv_synth_f32(p(attn), p(Wk), p(biask), p(wout), p(bout), B, Cin, Cin_pad, Cout, kk, K, stream())


def check_wout(wout, bout, W, b, case, tag):
    """W_b against (value, sum) with pad channels exactly 0; bias_b against (value, sum), or exactly 0 where b is None."""
    B, Cin, Cin_pad, Cout, kk, K = case
    w4 = wout.view(B, Cout, kk, Cin_pad)
    R.within(w4[..., :Cin], *W, f'{tag} W_b')
    assert not w4[..., Cin:].cpu().view(torch.int32).any(), f'{tag}: the pad channels of W_b are not exactly 0'
    if b is None:
        assert not bout.cpu().view(torch.int32).any(), f'{tag}: bias_b without biask is not exactly 0'
    else:
        R.within(bout, *b, f'{tag} bias_b')


@pytest.mark.parametrize('case', R.SYNTH_CASES, ids=R.ident)
def test_odconv_synth(case):
    from somi_amd import ops
    d = dev()
    B, Cin, Cin_pad, Cout, kk, K = case
    c = R.synth_inputs(case)
    attn, Wk = c.attn.to(d), packed_k(c.Wk, Cin_pad, JUNK).to(d)
    for has_bias in (True, False):
        biask = c.biask.to(d) if has_bias else None
        W, b = R.synth(c.attn, c.Wk, c.biask if has_bias else None)

        def run():
            wout, bout = nans(B, Cout, kk * Cin_pad), nans(B, Cout)
            assert raw_synth(attn, Wk, biask, wout, bout, B, Cin, Cin_pad, Cout, kk, K) == 0
            return wout, bout
        wout, bout = twice(run)
        check_wout(wout, bout, W, b if has_bias else None, case, f'odconv_synth {case} biask={has_bias}')
        ow, ob = ops.odconv_synth(attn, Wk, biask, Cin, Cin_pad, Cout, kk, K)
        assert torch.equal(ow, wout) and torch.equal(ob, bout), 'ops.odconv_synth differs from the direct call'


def raw_weights(e, with_fc_b, Wk, biask, bn, wout, bout, ws, case):
    L, _, p, stream = api()
    B, Cin, Cin_pad, Cout, kk, K = case
    return L.somi_odconv_weights_f32(p(e['gap']), p(e['fc_w']), p(e['fc_b'] if with_fc_b else None), p(e['Wf']), p(e['bf']), p(e['Ws']), p(e['bs']),
                                     p(e['Wc']), p(e['bc']), p(e['Ww']), p(e['bw']), p(Wk), p(biask), p(bn[0] if bn else None),
                                     p(bn[1] if bn else None), p(wout), p(bout), p(ws), B, Cin, Cin_pad, Cout, kk, K, e['fc_w'].shape[0], stream())


@pytest.mark.parametrize('case', R.SYNTH_CASES, ids=R.ident)
def test_odconv_weights(case):
    """The eval entry: heads, synthesis and fold in one call, against the restatement (the attention buffer it leaves in its workspace too) and
    against the train pair on the same inputs: linear x 5, then odconv_synth."""
    from somi_amd import ops
    d = dev()
    B, Cin, Cin_pad, Cout, kk, K = case
    na = Cout + kk + Cin + K
    c = R.eval_inputs(case)
    e = {n: v.to(d) for n, v in vars(c).items() if torch.is_tensor(v)}
    Wk = packed_k(c.Wk, Cin_pad, JUNK).to(d)
    small = Cout * kk * Cin <= 1 << 16
    for has_bias, with_fc_b in ((True, True), (True, False), (False, True), (False, False)) if small else ((True, True), (False, False)):
        biask = e['biask'] if has_bias else None
        attn_ref = R.heads(*R.eval_head_args(c, with_fc_b))
        plain = R.synth(attn_ref[0], c.Wk, c.biask if has_bias else None, attn_absum=attn_ref[1])
        # the train pair
        z = ops.linear(e['gap'], e['fc_w'], e['fc_b'] if with_fc_b else None, 'relu', out=nans(B, c.hid))
        attn = nans(B, na)
        for n, off, act in (('f', 0, 'sigmoid'), ('s', Cout, 'sigmoid'), ('c', Cout + kk, 'sigmoid'), ('w', Cout + kk + Cin, 'softmax')):
            ops.linear(z, e['W' + n], e['b' + n], act, attn, off)
        R.within(attn, *attn_ref, f'the train pair\'s attention buffer {case}')
        tw, tb = ops.odconv_synth(attn, Wk, biask, Cin, Cin_pad, Cout, kk, K)
        for bn in (None, (e['bn_s'], e['bn_t'])):
            W, b = plain if bn is None else R.fold(*plain, (c.bn_s, c.bn_t))
            tag = f'odconv_weights {case} hid={c.hid} biask={has_bias} fc_b={with_fc_b} bn={bn is not None}'

            def run():
                wout, bout, ws = nans(B, Cout, kk * Cin_pad), nans(B, Cout), nans(B * na)
                assert raw_weights(e, with_fc_b, Wk, biask, bn, wout, bout, ws, case) == 0
                return wout, bout, ws
            wout, bout, ws = twice(run)
            R.within(ws.view(B, na), *attn_ref, f'{tag} attention buffer')
            check_wout(wout, bout, W, b if has_bias or bn is not None else None, case, tag)
            w4 = wout.view(B, Cout, kk, Cin_pad)
            # against the train pair, under the same bar
            pair = ((tw.view(B, Cout, kk, Cin_pad)[..., :Cin].cpu().double(), None), (tb.cpu().double(), None))
            if bn is not None:
                pair = R.fold((pair[0][0], pair[0][0]), (pair[1][0], pair[1][0]), (c.bn_s, c.bn_t))
            R.within(w4[..., :Cin], pair[0][0], W[1], f'{tag} W_b against the train pair')
            R.within(bout, pair[1][0], b[1], f'{tag} bias_b against the train pair')
            ow, ob = ops.odconv_weights(e['gap'], e['fc_w'], e['fc_b'] if with_fc_b else None,
                                        dict(e, Wk=Wk, biask=biask, bn_s=bn and bn[0], bn_t=bn and bn[1]), nans(B, Cout, kk * Cin_pad), nans(B, Cout),
                                        Cin, Cin_pad, Cout, kk, K)
            assert torch.equal(ow, wout) and torch.equal(ob, bout), 'ops.odconv_weights differs from the direct call'


# ------------------------------------------------------------------------------------------------------------------- d. synthesis backward
def raw_synth_bwd(dWb, attn, Wk, biask, dbias_b, dWk, dbiask, dattn, ws, B, Cin, Cin_pad, Cout, kk, K):
    L, _, p, stream = api()
    return L.somi_odconv_synth_bwd_f32(p(dWb), p(attn), p(Wk), p(biask), p(dbias_b), p(dWk), p(dbiask), p(dattn), p(ws), B, Cin, Cin_pad, Cout, kk, K,
                                       stream())


@pytest.mark.parametrize('name', list(R.SYNTH_BWD_CASES))
def test_odconv_synth_backward(name):
    from somi_amd import ops
    L = api()[0]
    d = dev()
    case = R.SYNTH_BWD_CASES[name]
    B, Cin, Cin_pad, Cout, kk, K, has_bias = case
    c = R.synth_bwd_inputs(case)
    r = R.synth_grads(c.dWb, c.attn, c.Wk, c.biask, c.dbias_b)
    dWb, attn, Wk = packed_k(c.dWb, Cin_pad, JUNK).to(d), c.attn.to(d), packed_k(c.Wk, Cin_pad, JUNK).to(d)
    biask, dbias_b = (c.biask.to(d), c.dbias_b.to(d)) if has_bias else (None, None)
    dWk0 = packed_k(like_scaled(r['dWk'][0], 1), Cin_pad, 0.0)
    dWk0.view(K, Cout, kk, Cin_pad)[..., Cin:] = 0.5               # the pad lanes of dWk: must come back bit-unchanged
    dbk0 = like_scaled(r['dbiask'][0], 2) if has_bias else None
    nws = L.somi_odconv_synth_bwd_workspace_floats(B, Cin, Cout, kk, K)
    assert nws == B * Cout * (kk + Cin + K)

    def run():
        dWk, dbk, dattn, ws = dWk0.to(d), None if dbk0 is None else dbk0.to(d), nans(*attn.shape), nans(nws)
        assert raw_synth_bwd(dWb, attn, Wk, biask, dbias_b, dWk, dbk, dattn, ws, B, Cin, Cin_pad, Cout, kk, K) == 0
        return dWk, dbk, dattn, ws
    dWk, dbk, dattn, ws = twice(run)
    tag = f'odconv_synth_backward {name}'
    assert torch.isfinite(ws).all(), f'{tag}: the workspace keeps a NaN, so a partial sum was never written'
    for n, seg in zip(('da_f', 'da_s', 'da_c', 'da_w'), R.split_attn(dattn, Cout, kk, Cin, K)):
        R.within(seg, *r[n], f'{tag} {n}')
    g4, s4 = dWk.view(K, Cout, kk, Cin_pad), dWk0.view(K, Cout, kk, Cin_pad)
    added(g4[..., :Cin], s4[..., :Cin], r['dWk'], f'{tag} dWk')
    same_bits(g4[..., Cin:], s4[..., Cin:], f'{tag}: the pad lanes of dWk')
    if has_bias:
        added(dbk, dbk0, r['dbiask'], f'{tag} dbiask')
    oWk, obk = dWk0.to(d), None if dbk0 is None else dbk0.to(d)
    oattn = ops.odconv_synth_backward(dWb.view(B, Cout, kk * Cin_pad), attn, Wk, biask, dbias_b, oWk, obk, Cin, Cin_pad, Cout, kk, K)
    assert torch.equal(oattn, dattn) and torch.equal(oWk, dWk) and (obk is None or torch.equal(obk, dbk)), 'ops.odconv_synth_backward differs'


def test_odconv_synth_backward_rejections():
    L = api()[0]
    d = dev()
    n = 1 << 18                                                   # every buffer holds every shape below
    buf = lambda: torch.zeros(n, device=d)                         # noqa: E731
    dWb, attn, Wk, biask, dbias_b = buf(), buf(), buf(), buf(), buf()
    # (B, Cin, Cin_pad, Cout, kk, K), biask, dbias_b / dbiask
    cases = {'K = 9': ((1, 4, 4, 4, 1, 9), True, True), 'kk = 65': ((1, 4, 4, 4, 65, 4), True, True), 'Cin = 1028': ((1, 1028, 1028, 1, 1, 1), True, True),
             'Cin_pad % 4 != 0': ((1, 6, 6, 4, 1, 1), True, True), 'biask without dbias_b': ((1, 4, 4, 4, 1, 1), True, False)}
    for what, (shape, with_bias, with_grads) in cases.items():
        dWk, dbk, dattn, ws = buf(), buf(), nans(n), nans(n)
        rc = raw_synth_bwd(dWb, attn, Wk, biask if with_bias else None, dbias_b if with_grads else None, dWk, dbk if with_grads else None, dattn, ws,
                           *shape)
        assert rc == EINVAL, f'{what}: returned {rc}'
        assert L.somi_last_error().decode().startswith('odconv synth bwd:'), what
        torch.cuda.synchronize()
        assert torch.isnan(dattn).all() and torch.isnan(ws).all() and not dWk.any() and not dbk.any(), f'{what}: rejected, but something was written'


# ------------------------------------------------------------------------------------------------------------------- e. per-sample conv
@pytest.mark.parametrize('case', R.CONV_CASES, ids=R.ident)
def test_per_sample_conv(case):
    """Forward with a per-sample bias, data gradient and weight gradient (each plain and added onto a non-zero tensor) of the conv whose
    grid.z is the sample, in fp32, against a per-sample F.conv2d and its autograd in fp64."""
    from somi_amd import ops
    d = dev()
    B, H, W, Cin, Cout, k, s = case
    c = R.conv_inputs(case)
    r = R.conv_per_sample(c.x, c.w, c.bias, c.dy, k, s)
    kw = dict(kh=k, kw=k, stride=s, pad=k // 2, per_sample_w=True)
    x, dy, bias = nhwc(c.x).to(d), nhwc(c.dy).to(d), c.bias.to(d)
    wp = c.w.permute(0, 1, 3, 4, 2).reshape(B, Cout, k * k * Cin).contiguous().to(d)           # [b][Cout][kk Cin]
    wt = c.w.permute(0, 2, 3, 4, 1).reshape(B, Cin, k * k * Cout).contiguous().to(d)           # [b][Cin][kk Cout]: the data gradient's operand
    tag = f'per-sample conv {case}'
    y, = twice(lambda: (ops.conv2d_nhwc(x, wp, bias, act='none', out=nans(*dy.shape), **kw),))
    R.within(y, *(nhwc(v) for v in r['y']), f'{tag} forward')
    geo = dict(B=B, H=H, W=W, cin=Cin, **kw)
    dx, = twice(lambda: (ops.conv2d_dgrad_nhwc(dy, wt, out=nans(B, H, W, Cin), **geo),))
    dxr = tuple(nhwc(v) for v in r['dx'])
    R.within(dx, *dxr, f'{tag} data gradient')
    dx0 = like_scaled(dxr[0], 1, per_sample=True)
    dx0d = dx0.to(d)
    got, = twice(lambda: (ops.conv2d_dgrad_nhwc(dy, wt, out=nans(B, H, W, Cin), accumulate=dx0d, **geo),))
    added(got, dx0, dxr, f'{tag} data gradient, added')
    same_bits(dx0d, dx0, 'the tensor the data gradient is added to')
    dwr = tuple(v.permute(0, 1, 3, 4, 2).reshape(B, Cout, k * k * Cin) for v in r['dw'])
    dw, = twice(lambda: (ops.conv2d_wgrad_nhwc(x, dy, out=nans(B, Cout, k * k * Cin), **kw),))
    R.within(dw, *dwr, f'{tag} weight gradient')
    dw0 = like_scaled(dwr[0], 2)

    def run():
        acc = dw0.to(d)
        return (ops.conv2d_wgrad_nhwc(x, dy, out=acc, accumulate=acc, **kw),)
    got, = twice(run)
    added(got, dw0, dwr, f'{tag} weight gradient, added')


# ------------------------------------------------------------------------------------------------------------------- f. the block
@pytest.mark.parametrize('c1,c2,k,s,H,W,B', [(64, 128, 3, 2, 12, 12, 3), (512, 256, 3, 2, 6, 6, 3), (1024, 256, 3, 2, 4, 4, 3), (32, 32, 1, 1, 9, 7, 3),
                                             (512, 256, 3, 2, 6, 6, 1)])
def test_odconv_block_at_the_product_widths(c1, c2, k, s, H, W, B):
    """Eval forward, train forward, dx, every parameter gradient and the running statistics of ODConv_3rd(c1, c2, k, s, 4) at the sites of the
    default graph (hidden width 16, 32 and 64) and at k = 1.  B = 3: a squeeze BatchNorm over two samples is degenerate."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    ref = fill_state(OB.ODConv_3rd(c1, c2, k, s, 4), 12)
    OB.initialize_weights(ref)
    mine = MB.ODConv_3rd(c1, c2, k, s, 4)
    mine.load_state_dict(ref.state_dict())
    x = torch.randn(B, c1, H, W, generator=torch.Generator().manual_seed(B + c1))
    # conv.reduction is unused in the reference (and here); one sample skips the squeeze BatchNorm, so its parameters get nothing either
    no_grad = ('conv.reduction.weight', 'conv.reduction.bias') + (('conv.bn.weight', 'conv.bn.bias') if B == 1 else ())
    check_built_block(ref, mine, x, torch.Generator().manual_seed(41 + B), f'ODConv {c1}->{c2} k{k}s{s} B={B}', eval_too=True, no_grad=no_grad)
