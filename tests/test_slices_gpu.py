"""The channel-slice contract (tests/slices.py) on the kernels every layer calls with offsets: dense conv forward / data gradient / weight
gradient, the fused twin-branch 1x1 pattern of blocks.py, the BatchNorm training sweeps and the copy kernels.  Every slice sits between live
neighbour channels at an offset that is 16-byte but not 64-byte aligned; references are torch on the CPU in fp64, computed from the slices'
contents only; the bars are the ones the sibling tests of each kernel use (test_kernels_gpu.py, test_train_gpu.py)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from parity import nchw, nhwc, rel_close
from slices import (In, Out, check_slice_op, depth_to_space_ref, embed, resample_copy_ref, resample_reduce_ref, space_to_depth_ref)

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(v) for i, v in enumerate(key)) + 17)


# ------------------------------------------------------------------------------------------------ dense conv forward
FWD = {
    # name: B, H, W, Cin, Cout, k, s, x_cs, x_coff, y_cs, y_coff, extras
    'a': (2, 9, 11, 20, 36, 3, 1, 36, 4, 52, 12, {}),                                   # K tail and N tail together, generic tap path
    'b': (2, 12, 12, 100, 20, 1, 1, 140, 28, 36, 4, {}),                                # 128x32 tile
    'c': (3, 20, 20, 128, 256, 3, 2, 160, 20, 300, 28, {'res': (280, 12), 'post': True}),
    'd': (4, 40, 40, 128, 256, 3, 1, 152, 12, 288, 20, {'res': (276, 12)}),             # stream-K: cut tiles finish in the fix-up kernel
    'f177': (2, 17, 13, 32, 177, 3, 1, 48, 12, 188, 4, {}),                             # ragged Cout: [y_coff + Cout, y_cs) stays untouched
    'f20': (2, 12, 12, 100, 20, 1, 1, 112, 4, 28, 4, {}),
}


@functools.lru_cache(maxsize=None)
def _fwd_case(name):
    """The dense tensors of one forward case and its fp64 reference (shared by the plain and the statistics test)."""
    B, H, W, Cin, Cout, k, s, x_cs, x_coff, y_cs, y_coff, ex = FWD[name]
    g = _gen(B, H, Cin, Cout, k, s)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    bias = torch.randn(Cout, generator=g)
    want = F.silu(F.conv2d(x.double(), w.double(), bias.double(), s, k // 2))
    t = {'x': nhwc(x), 'w': w, 'bias': bias}
    if ex.get('post'):
        t['ps'], t['pt'] = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        want = want * t['ps'].double()[None, :, None, None] + t['pt'].double()[None, :, None, None]
    if ex.get('res'):
        t['res'] = torch.randn(nhwc(want).shape, generator=g)
        want = want + nchw(t['res']).double()
    return t, nhwc(want)


def _fwd_call(name, bufs, **more):
    from somi_amd import ops
    B, H, W, Cin, Cout, k, s, x_cs, x_coff, y_cs, y_coff, ex = FWD[name]
    kw = dict(more)
    if ex.get('post'):
        kw.update(post_scale=bufs['ps'], post_shift=bufs['pt'])
    if ex.get('res'):
        kw.update(residual=bufs['res'], res_coff=ex['res'][1])
    return ops.conv2d_nhwc(bufs['x'], bufs['w'], bufs['bias'], kh=k, kw=k, stride=s, pad=k // 2, act='silu', cin=Cin, x_coff=x_coff,
                           out=bufs['y'], cout=Cout, y_coff=y_coff, **kw)


def _fwd_specs(name):
    from somi_amd.pack import pack_conv_weight
    B, H, W, Cin, Cout, k, s, x_cs, x_coff, y_cs, y_coff, ex = FWD[name]
    t, want = _fwd_case(name)
    inputs = {'x': In(t['x'], x_cs, x_coff), 'w': pack_conv_weight(t['w'], cin_pad=Cin), 'bias': t['bias']}
    if ex.get('post'):
        inputs.update(ps=t['ps'], pt=t['pt'])
    if ex.get('res'):
        inputs['res'] = In(t['res'], ex['res'][0], ex['res'][1])
    return inputs, {'y': Out(want.shape[:3], y_cs, y_coff, Cout)}, want


@pytest.mark.parametrize('name', list(FWD))
def test_conv_forward_into_a_slice(name, monkeypatch):
    from somi_amd import ops
    inputs, outputs, want = _fwd_specs(name)
    check_slice_op(lambda b: _fwd_call(name, b), inputs, outputs, {'y': want}, what=f'conv forward {name}')
    if name == 'd':                                             # the schedule under test was taken: bitwise unlike one workgroup per tile
        o = outputs['y']
        bufs = {n: (embed(s.t, s.cs, s.coff, 'rand_a') if isinstance(s, In) else s).to(dev()) for n, s in inputs.items()}
        y1, y0 = torch.zeros(*o.shape, o.cs, device=dev()), torch.zeros(*o.shape, o.cs, device=dev())
        _fwd_call(name, dict(bufs, y=y1))
        with monkeypatch.context() as mp:
            mp.setattr(ops, '_conv_workspace', lambda d, dev: None)
            _fwd_call(name, dict(bufs, y=y0))
        assert not torch.equal(y0, y1), 'the stream-K schedule was not taken for a shape it is meant for'
        rel_close(y1, y0, rel=1e-5, what='stream-K vs one workgroup per tile, in slices')


@pytest.mark.parametrize('name', ['a', 'd'])
def test_conv_epilogue_statistics_of_a_slice(name):
    """bn_stats={'pivot': ...} with every offset non-zero: the output is bitwise what it is without statistics, and the statistics from the
    epilogue's partial sums equal the separate pass over the output slice (bars of test_conv_epilogue_batchnorm_statistics) and fp64."""
    from somi_amd import ops
    B, H, W, Cin, Cout, k, s, x_cs, x_coff, y_cs, y_coff, ex = FWD[name]
    inputs, outputs, want = _fwd_specs(name)
    g = _gen(Cout, 3)
    inputs.update(gam=torch.rand(Cout, generator=g) + 0.5, bet=torch.randn(Cout, generator=g), rm0=torch.randn(Cout, generator=g) * 0.3,
                  rv0=torch.rand(Cout, generator=g) + 0.5)
    npix = want.shape[0] * want.shape[1] * want.shape[2]

    def run(b):
        st = {'pivot': b['rm0']}
        _fwd_call(name, b, bn_stats=st)
        plain = b['y'].clone()
        _fwd_call(name, dict(b, y=plain))
        assert torch.equal(_bits_view(plain), _bits_view(b['y'])), 'the output changes when the epilogue takes statistics'
        rm1, rv1, rm2, rv2 = b['rm0'].clone(), b['rv0'].clone(), b['rm0'].clone(), b['rv0'].clone()
        got = ops.bn_stats_from_partials(st['part'], st['rows'], npix, Cout, b['gam'], b['bet'], 1e-3, 0.03, rm1, rv1)
        sep = ops.bn_stats(b['y'], Cout, y_coff, b['gam'], b['bet'], 1e-3, 0.03, rm2, rv2)
        if not torch.isnan(b['y'][..., 0]).any():               # (under the NaN fill the comparison is the helper's: bitwise the same)
            for a_, b_, what in zip(got, sep, ('mean', 'rstd', 'scale', 'shift')):
                rel_close(a_, b_, rel=1e-5, what=f'{what}: partial sums vs the separate pass')
            rel_close(rm1, rm2, rel=1e-6, what='running mean: partial sums vs the separate pass')
            rel_close(rv1, rv2, rel=1e-5, what='running var: partial sums vs the separate pass')
        return {'mean': got[0], 'var': 1.0 / got[1].double() ** 2 - 1e-3, 'scale': got[2], 'shift': got[3], 'rm': rm1, 'rv': rv1,
                'mean_sep': sep[0], 'rstd_sep': sep[1]}
    y64 = lambda r: r['y'].double().reshape(-1, Cout)            # noqa: E731  statistics of the output the kernel itself wrote
    refs = {'y': want, 'mean': lambda r: y64(r).mean(0), 'var': lambda r: y64(r).var(0, unbiased=False),
            'mean_sep': lambda r: y64(r).mean(0), 'rstd_sep': lambda r: 1.0 / torch.sqrt(y64(r).var(0, unbiased=False) + 1e-3),
            'scale': lambda r: inputs['gam'].double() / torch.sqrt(y64(r).var(0, unbiased=False) + 1e-3),
            'shift': lambda r: inputs['bet'].double() - y64(r).mean(0) * inputs['gam'].double() / torch.sqrt(y64(r).var(0, unbiased=False) + 1e-3),
            'rm': lambda r: 0.97 * inputs['rm0'].double() + 0.03 * y64(r).mean(0),
            'rv': lambda r: 0.97 * inputs['rv0'].double() + 0.03 * y64(r).var(0, unbiased=True)}
    check_slice_op(run, inputs, outputs, refs, bars={'mean': 1e-5, 'var': 1e-4, 'mean_sep': 1e-5, 'rstd_sep': 1e-5},
                   what=f'conv forward {name} with epilogue statistics')


def _bits_view(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ dense data gradient
DGRAD = [(2, 9, 11, 20, 36, 3, 1),         # ragged channels
         (2, 17, 13, 32, 64, 3, 2),        # stride-2 parity classes
         (2, 9, 12, 16, 32, 1, 2),         # three of the four parity classes have no tap
         (2, 14, 14, 16, 32, 6, 2),        # 6x6 stride-2 stem
         (2, 11, 13, 8, 32, 5, 3),         # stride 3
         (6, 40, 40, 128, 128, 3, 1)]      # stream-K
DY_COFF, DX_COFF, ACC_COFF, ACC2_COFF = 12, 4, 20, 28


@functools.lru_cache(maxsize=None)
def _dgrad_case(case):
    B, H, W, Cin, Cout, k, s = case
    g = _gen(*case)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    y = F.conv2d(x, w.double(), None, s, k // 2)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    acc, acc2 = torch.randn(B, H, W, Cin, generator=g), torch.randn(B, H, W, Cin, generator=g)
    return nhwc(dy), w, nhwc(x.grad), acc, acc2


@pytest.mark.parametrize('form', ['plain', 'in_place', 'two_sources'])
@pytest.mark.parametrize('case', DGRAD, ids=lambda c: 'x'.join(str(v) for v in c))
def test_conv_dgrad_between_slices(case, form):
    """dy read at dy_coff, dx written at dx_coff; accumulate=out in place (the skip connection), or accumulate from another buffer at acc_coff
    plus accumulate2 at acc2_coff (the shortcut's gradient): four different non-zero offsets."""
    from somi_amd import ops
    from somi_amd.pack import pack_dgrad_weight
    B, H, W, Cin, Cout, k, s = case
    dy, w, want, acc, acc2 = _dgrad_case(case)
    inputs = {'dy': In(dy, Cout + 24, DY_COFF), 'wt': pack_dgrad_weight(w, cin_pad=Cin, cout_pad=Cout)}
    out = Out((B, H, W), Cin + 12, DX_COFF, Cin)
    added = torch.zeros_like(acc)
    if form == 'in_place':
        out, added = Out((B, H, W), Cin + 12, DX_COFF, Cin, prev=acc, accumulate=True), acc
    elif form == 'two_sources':
        inputs.update(acc=In(acc, Cin + 32, ACC_COFF), acc2=In(acc2, Cin + 40, ACC2_COFF))
        want, added = want + acc.double() + acc2.double(), acc + acc2

    def run(b):
        kw = {}
        if form == 'in_place':
            kw = dict(accumulate=b['dx'], acc_coff=DX_COFF)
        elif form == 'two_sources':
            kw = dict(accumulate=b['acc'], acc_coff=ACC_COFF, accumulate2=b['acc2'], acc2_coff=ACC2_COFF)
        ops.conv2d_dgrad_nhwc(b['dy'], b['wt'], B=B, H=H, W=W, cin=Cin, kh=k, kw=k, stride=s, pad=k // 2, cout=Cout, dy_coff=DY_COFF,
                              out=b['dx'], dx_coff=DX_COFF, **kw)
    got = check_slice_op(run, inputs, {'dx': out}, {'dx': want}, what=f'dgrad {form}')['dx']
    if k == 1 and s == 2:                                       # pixels no tap reaches hold 0, or the accumulate sources, and nothing else
        no_tap = torch.ones(H, W, dtype=torch.bool)
        no_tap[::2, ::2] = False
        assert torch.equal(got[:, no_tap], added[:, no_tap]), 'a pixel of a parity class without a tap holds something else than its sources'


# ------------------------------------------------------------------------------------------------ dense weight gradient
WGRAD = [(2, 9, 11, 20, 36, 3, 1, False),
         (3, 33, 31, 4, 64, 3, 2, False),       # the stem
         (2, 12, 12, 96, 68, 1, 1, False),
         (16, 20, 20, 256, 132, 1, 1, False),   # several pixel splits
         (2, 8, 8, 16, 32, 3, 1, False),        # a single pixel split
         (3, 12, 12, 32, 48, 3, 2, True)]       # per-sample weight sets
WX_COFF, WDY_COFF, DW_PAD = 12, 20, 16


@functools.lru_cache(maxsize=None)
def _wgrad_case(case):
    B, H, W, Cin, Cout, k, s, ps = case
    g = _gen(*case)
    x = torch.randn(B, Cin, H, W, generator=g)
    Ho = (H + 2 * (k // 2) - k) // s + 1
    Wo = (W + 2 * (k // 2) - k) // s + 1
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    want = []
    for b in (range(B) if ps else [slice(None)]):
        xb, dyb = (x[b:b + 1], dy[b:b + 1]) if ps else (x, dy)
        w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(xb.double(), w, None, s, k // 2).backward(dyb.double())
        want.append(w.grad.movedim(-3, -1).reshape(Cout, k * k * Cin))      # the forward packing [Cout][kh*kw*Cin], in fp64
    want = torch.stack(want) if ps else want[0]
    return nhwc(x), nhwc(dy), want, torch.randn(want.shape, generator=g)


@pytest.mark.parametrize('form', ['plain', 'accumulate'])
@pytest.mark.parametrize('case', WGRAD, ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_conv_wgrad_from_slices(case, form):
    """x read at x_coff, dy at dy_coff (different, both with live neighbours).  The packed dW lies inside a larger allocation: it has exactly
    its own shape and nothing around it is touched.  accumulate: out=acc, accumulate=acc adds onto the gradient that is there."""
    from somi_amd import ops
    B, H, W, Cin, Cout, k, s, ps = case
    x, dy, want, prev = _wgrad_case(case)
    n = want.numel()
    out = Out((1,), n + 2 * DW_PAD, DW_PAD, n, prev=prev.reshape(1, n) if form == 'accumulate' else None, accumulate=form == 'accumulate')

    def run(b):
        dw = b['dw'][0, DW_PAD:DW_PAD + n].view(want.shape)
        kw = dict(kh=k, kw=k, stride=s, pad=k // 2, cin=Cin, x_coff=WX_COFF, cout=Cout, dy_coff=WDY_COFF, per_sample_w=ps)
        ops.conv2d_wgrad_nhwc(b['x'], b['dy'], out=dw, accumulate=dw if form == 'accumulate' else None, **kw)
        if form == 'plain':
            fresh = ops.conv2d_wgrad_nhwc(b['x'], b['dy'], **kw)
            assert fresh.shape == want.shape, f'dW allocated as {tuple(fresh.shape)}, expected {tuple(want.shape)}'
            return {'fresh': fresh}
    refs = {'dw': want.reshape(1, n)}
    if form == 'plain':
        refs['fresh'] = want
    check_slice_op(run, {'x': In(x, Cin + 24, WX_COFF), 'dy': In(dy, Cout + 28, WDY_COFF)}, {'dw': out}, refs, what=f'wgrad {form}')


# ------------------------------------------------------------------------------------------------ the twin-branch 1x1 pattern of blocks.py
def test_twin_branch_1x1_pattern():
    """Two 1x1 convs read one input slice and write adjacent slices of one buffer; backward takes each branch's weight gradient from
    dy_coff = o and lets branch 2's data gradient accumulate in place onto branch 1's.  Against autograd on torch.cat of two F.conv2d."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    B, H, W, c1, c_ = 2, 7, 9, 20, 12
    x_cs, x_coff, y_cs, o1, dx_cs, dx_coff = 32, 4, 40, 8, 28, 4
    o2 = o1 + c_
    g = _gen(c1, c_)
    x = torch.randn(B, c1, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w1 = (torch.randn(c_, c1, 1, 1, generator=g) / math.sqrt(c1)).double().requires_grad_(True)
    w2 = (torch.randn(c_, c1, 1, 1, generator=g) / math.sqrt(c1)).double().requires_grad_(True)
    b1, b2 = torch.randn(c_, generator=g), torch.randn(c_, generator=g)
    y = torch.cat([F.conv2d(x, w1, b1.double()), F.conv2d(x, w2, b2.double())], 1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    xs = In(nhwc(x.detach()), x_cs, x_coff)
    packed = {'w1': pack_conv_weight(w1.detach().float(), cin_pad=c1), 'w2': pack_conv_weight(w2.detach().float(), cin_pad=c1)}

    def forward(b):
        for w, bias, o in ((b['w1'], b['b1'], o1), (b['w2'], b['b2'], o2)):
            ops.conv2d_nhwc(b['x'], w, bias, kh=1, kw=1, cin=c1, x_coff=x_coff, out=b['y'], cout=c_, y_coff=o)
    check_slice_op(forward, dict(packed, x=xs, b1=b1, b2=b2), {'y': Out((B, H, W), y_cs, o1, 2 * c_)}, {'y': nhwc(y.detach())},
                   what='twin 1x1 forward')
    wts = {'wt1': pack_dgrad_weight(w1.detach().float(), cin_pad=c1, cout_pad=c_), 'wt2': pack_dgrad_weight(w2.detach().float(), cin_pad=c1, cout_pad=c_)}

    def backward(b):
        dws = {}
        for i, (wt, o) in enumerate(((b['wt1'], o1), (b['wt2'], o2))):
            dws[f'dw{i + 1}'] = ops.conv2d_wgrad_nhwc(b['x'], b['dy'], kh=1, kw=1, cin=c1, x_coff=x_coff, cout=c_, dy_coff=o)
            ops.conv2d_dgrad_nhwc(b['dy'], wt, B=B, H=H, W=W, cin=c1, kh=1, kw=1, cout=c_, dy_coff=o, out=b['dx'], dx_coff=dx_coff,
                                  accumulate=b['dx'] if i else None, acc_coff=dx_coff)
        return dws
    check_slice_op(backward, dict(wts, x=xs, dy=In(nhwc(dy), y_cs, o1)), {'dx': Out((B, H, W), dx_cs, dx_coff, c1)},
                   {'dx': nhwc(x.grad), 'dw1': w1.grad.view(c_, c1), 'dw2': w2.grad.view(c_, c1)}, what='twin 1x1 backward')


# ------------------------------------------------------------------------------------------------ training sweeps
SWEEP_SIZES = [(1, 4), (7, 12), (353, 1028)]          # the sizes test_elementwise_sweeps_cover_every_pixel_and_channel chose for the thread mapping
S_COFF, S_PAD = 12, 24                                # the slice sits at coff 12 of C + 24 channels


def _silu_grad(u):
    sg = torch.sigmoid(u)
    return sg * (1 + u * (1 - sg))


@pytest.mark.parametrize('npix,C', SWEEP_SIZES)
def test_bn_stats_of_a_slice(npix, C):
    """mean, rstd, scale / shift and the running statistics of the slice only, against fp64.  Bars: the mean 1e-5 and the variance 1 / rstd^2 - eps
    1e-4 of the largest, as test_conv_epilogue_batchnorm_statistics holds them against fp64; everything else 1e-3 as in
    test_bn_act_forward_backward.  The variance bar has one absolute term: the kernel sums fp32 squares t^2 of t = x - pivot (the running mean),
    each rounded by up to 2^-24 t^2 on top of t's own rounding, so s2 / n - mean^2 carries up to ~4 * 2^-24 * mean(t^2) whatever the spread is.
    A single pixel has variance 0 exactly: there that term is the whole bar (against 1e-4 * 0)."""
    from somi_amd import ops
    g = _gen(npix, C)
    x = torch.randn(1, 1, npix, C, generator=g) * 1.5 + 0.3
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    x64 = x.double().reshape(npix, C)
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-3)
    unb = var * npix / (npix - 1) if npix > 1 else var         # one pixel has no unbiased variance: the kernel keeps the biased one
    sq_round = 4 * 2.0 ** -24 * ((x64 - rm0.double()) ** 2).mean(0).max().item()
    want = {'mean': mean, 'rstd': rstd, 'var': var, 'scale': gam.double() * rstd, 'shift': bet.double() - mean * gam.double() * rstd,
            'rm': 0.97 * rm0.double() + 0.03 * mean, 'rv': 0.97 * rv0.double() + 0.03 * unb}

    def run(b):
        m, r, sc, sh = ops.bn_stats(b['x'], C, S_COFF, b['gam'], b['bet'], 1e-3, 0.03, b['rm'], b['rv'])
        return {'mean': m, 'rstd': r, 'var': 1.0 / r.double() ** 2 - 1e-3, 'scale': sc, 'shift': sh, 'rm': b['rm'], 'rv': b['rv']}
    check_slice_op(run, {'x': In(x, C + S_PAD, S_COFF), 'gam': gam, 'bet': bet, 'rm': rm0, 'rv': rv0}, {}, want,
                   bars={'mean': 1e-5, 'var': {'rel': 1e-4, 'atol': sq_round}}, what='bn_stats')


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('npix,C', SWEEP_SIZES)
def test_chan_affine_act_between_slices(npix, C, in_place):
    from somi_amd import ops
    g = _gen(npix, C, 1)
    x, res = torch.randn(1, 1, npix, C, generator=g), torch.randn(1, 1, npix, C, generator=g)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    u = x.double() * sc.double() + sh.double()
    want = u * torch.sigmoid(u) + res.double()
    inputs = {'res': In(res, C + 28, 20), 'sc': sc, 'sh': sh}
    if in_place:
        outputs = {'x': Out((1, 1, npix), C + S_PAD, S_COFF, C, prev=x)}
        run = lambda b: ops.chan_affine_act(b['x'], C, S_COFF, b['sc'], b['sh'], 'silu', 0, b['x'], S_COFF, residual=b['res'], res_coff=20)   # noqa: E731
        refs = {'x': want}
    else:
        inputs['x'] = In(x, C + S_PAD, S_COFF)
        outputs = {'out': Out((1, 1, npix), C + 16, 4, C)}
        run = lambda b: ops.chan_affine_act(b['x'], C, S_COFF, b['sc'], b['sh'], 'silu', 0, b['out'], 4, residual=b['res'], res_coff=20)   # noqa: E731
        refs = {'out': want}
    check_slice_op(run, inputs, outputs, refs, rel=1e-5, what='affine + silu + residual')


@pytest.mark.parametrize('batch_stats', [False, True])
@pytest.mark.parametrize('npix,C', SWEEP_SIZES)
def test_bn_act_backward_between_slices(npix, C, batch_stats):
    """dz, x and dx at three different offsets; dgamma / dbeta accumulate onto what they held.  Frozen statistics at the bars of
    test_elementwise_sweeps_cover_every_pixel_and_channel (dx 1e-5, dgamma / dbeta 1e-4), batch statistics at those of
    test_bn_act_forward_backward (1e-3), against fp64 autograd."""
    from somi_amd import ops
    g = _gen(npix, C, 2)
    x = torch.randn(1, 1, npix, C, generator=g) * 1.5 + 0.3
    dz = torch.randn(1, 1, npix, C, generator=g)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    if batch_stats:
        mean, var = x64.mean((0, 1, 2)), x64.var((0, 1, 2), unbiased=False)
    else:
        mean, var = (torch.randn(C, generator=g) * 0.1).double(), (torch.rand(C, generator=g) + 0.5).double()
    rstd = 1.0 / torch.sqrt(var + 1e-3)
    F.silu((x64 - mean) * rstd * g64 + b64).backward(dz.double())
    mean, rstd = mean.detach().float(), rstd.detach().float()
    scale = gam * rstd
    shift = bet - mean * scale

    def run(b):
        ops.bn_act_backward(b['dz'], 4, b['x'], S_COFF, C, b['mean'], b['rstd'], b['scale'], b['shift'], 'silu', 0, batch_stats, b['dx'], 20,
                            b['dg'], b['db'])
        return {'dgamma': b['dg'], 'dbeta': b['db']}
    inputs = {'dz': In(dz, C + 16, 4), 'x': In(x, C + S_PAD, S_COFF), 'mean': mean, 'rstd': rstd, 'scale': scale, 'shift': shift, 'dg': dg0, 'db': db0}
    want = {'dx': x64.grad, 'dgamma': dg0.double() + g64.grad, 'dbeta': db0.double() + b64.grad}
    bars = {} if batch_stats else {'dx': 1e-5, 'dgamma': 1e-4, 'dbeta': 1e-4}
    check_slice_op(run, inputs, {'dx': Out((1, 1, npix), C + 28, 20, C)}, want, bars=bars, what=f'bn_act_backward batch_stats={batch_stats}')


@pytest.mark.parametrize('npix,C', SWEEP_SIZES)
def test_add_and_chan_sum_between_slices(npix, C):
    """add_ with three different offsets, bit-exact; chan_sum_ accumulates the slice's channel sums (it is the bias gradient: dbeta's 1e-4)."""
    from somi_amd import ops
    g = _gen(npix, C, 3)
    a, b_ = torch.randn(1, 1, npix, C, generator=g), torch.randn(1, 1, npix, C, generator=g)
    check_slice_op(lambda b: ops.add_(b['a'], 4, b['b'], S_COFF, C, out=b['out'], out_coff=20),
                   {'a': In(a, C + 16, 4), 'b': In(b_, C + S_PAD, S_COFF)}, {'out': Out((1, 1, npix), C + 28, 20, C)}, {'out': a + b_},
                   bars={'out': 'exact'}, what='add_')
    check_slice_op(lambda b: ops.add_(b['a'], S_COFF, b['b'], 4, C), {'b': In(b_, C + 16, 4)},
                   {'a': Out((1, 1, npix), C + S_PAD, S_COFF, C, prev=a)}, {'a': a + b_}, bars={'a': 'exact'}, what='add_ in place')
    s0 = torch.randn(C, generator=g)
    check_slice_op(lambda b: {'sum': ops.chan_sum_(b['a'], C, S_COFF, b['s'])}, {'a': In(a, C + S_PAD, S_COFF), 's': s0}, {},
                   {'sum': s0.double() + a.double().sum((0, 1, 2))}, rel=1e-4, what='chan_sum_')


# ------------------------------------------------------------------------------------------------ copy kernels
@pytest.mark.parametrize('form', ['copy', 'reduce', 'reduce_accumulate'])
@pytest.mark.parametrize('up', [0, 1, 2, 3])
def test_resample_slice_between_slices(up, form):
    """Concat's copy with the nearest upsample folded in, and its reducing adjoint, bit-exact.  The reducing direction sums 4^up values in
    an order that is not part of the contract: the inputs are small integers, so every partial sum is exact in fp32 whatever the order."""
    from somi_amd import ops
    B, Hs, Ws, n = 2, 3, 5, 1 << up
    for C in (4, 12, 68):
        g = _gen(up, C, len(form))
        lo = torch.randint(-8, 9, (B, Hs, Ws, C), generator=g).float()
        hi = torch.randint(-8, 9, (B, Hs * n, Ws * n, C), generator=g).float()
        assert torch.equal(hi, hi.round()) and hi.abs().max() * n * n + 8 < 2 ** 24, 'the exactness condition of the block sums'
        if form == 'copy':
            check_slice_op(lambda b: ops.resample_slice(b['src'], 12, b['dst'], 4, C, up=up), {'src': In(lo, C + 20, 12)},
                           {'dst': Out((B, Hs * n, Ws * n), C + 12, 4, C)}, {'dst': resample_copy_ref(lo, up)}, bars={'dst': 'exact'},
                           what=f'resample copy up={up} C={C}')
        else:
            acc = form == 'reduce_accumulate'
            check_slice_op(lambda b: ops.resample_slice(b['src'], 12, b['dst'], 4, C, up=up, reduce=True, accumulate=acc),
                           {'src': In(hi, C + 20, 12)}, {'dst': Out((B, Hs, Ws), C + 12, 4, C, prev=lo if acc else None, accumulate=acc)},
                           {'dst': resample_reduce_ref(hi, up)}, bars={'dst': 'exact'}, what=f'resample {form} up={up} C={C}')


@pytest.mark.parametrize('C,x_cs,x_coff,y_cs,y_coff', [(3, 4, 0, 20, 4), (8, 16, 4, 48, 8)])
def test_space_to_depth_between_slices(C, x_cs, x_coff, y_cs, y_coff):
    """Focus and its inverse: the image's 3 channels in a 4-channel buffer, and 8 channels at x_coff 4 / y_coff 8.  inverse(forward(x)) == x
    on the slice, neighbours untouched in both directions."""
    from somi_amd import ops
    B, H, W = 2, 6, 10
    x = torch.randn(B, H, W, C, generator=_gen(C))

    def run(b):
        ops.space_to_depth(b['x'], x_coff, C, out=b['y'], y_coff=y_coff)
        ops.space_to_depth(b['y'], y_coff, C, out=b['back'], inverse=True, y_coff=x_coff)
    assert torch.equal(depth_to_space_ref(space_to_depth_ref(x)), x)
    check_slice_op(run, {'x': In(x, x_cs, x_coff)}, {'y': Out((B, H // 2, W // 2), y_cs, y_coff, 4 * C), 'back': Out((B, H, W), x_cs, x_coff, C)},
                   {'y': space_to_depth_ref(x), 'back': x}, bars={'y': 'exact', 'back': 'exact'}, what=f'space_to_depth C={C}')
