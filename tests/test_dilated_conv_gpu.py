"""Dilated convolution on the MI355X: forward, data gradient and weight gradient of the dense implicit-GEMM family (conv_igemm.hip,
conv_wgrad.hip) with dil > 1, through `ops`, against fp64 F.conv2d / torch.nn.grad.conv2d_input / conv2d_weight on the CPU.  Bar:
parity.rel_close's default, 1e-3 of the result's largest value (the fp32 matrix instruction is exact fp32 arithmetic: ~1e-6 in practice).  Every
launch runs twice and must be bit-identical.  The dilated data gradient exists at stride 1 only (the library refuses it at stride > 1)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from parity import nhwc, rel_close

pytestmark = pytest.mark.gpu

CASES = [
    # B, H, W, Cin, Cout, k, d, pad, stride
    (2, 7, 9, 32, 32, 3, 2, 2, 1),            # FAST path, H != W, one ragged row tile
    (1, 4, 4, 32, 16, 3, 5, 5, 1),            # the footprint exceeds the map: only the centre tap lands inside
    (2, 13, 11, 64, 40, 3, 3, 3, 1),          # three row tiles with a ragged last one, two channel chunks, Cout not a multiple of 32
    (1, 9, 7, 8, 12, 3, 2, 2, 1),             # the generic path, Cin % 32 != 0
    (1, 9, 7, 32, 32, 3, 2, 0, 1),            # pad 0, output 5x3
    (2, 12, 12, 32, 32, 5, 2, 4, 1),          # 25 taps
    (1, 16, 16, 256, 32, 3, 3, 3, 1),         # stream-K: 72 K-tiles over two tiles get cut
    (1, 10, 10, 32, 32, 3, 2, 2, 2),          # stride 2: forward and weight gradient only
]
SLICE_CASE = CASES[2]
STREAMK_CASE = CASES[6]


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _id(c):
    return 'x'.join(map(str, c[:5])) + f'-k{c[5]}d{c[6]}p{c[7]}s{c[8]}'


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fp32 tensors and the fp64 results, computed once and shared (nobody writes to them)."""
    B, H, W, Cin, Cout, k, d, p, s = case
    g = torch.Generator().manual_seed(sum(v * (i + 1) for i, v in enumerate(case)))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    x64, w64 = x.double(), w.double()
    y = F.conv2d(x64, w64, None, s, p, d)
    dy = torch.randn(y.shape, generator=g)
    dx = torch.nn.grad.conv2d_input(x64.shape, w64, dy.double(), s, p, d) if s == 1 else None
    dw = torch.nn.grad.conv2d_weight(x64, w64.shape, dy.double(), s, p, d)
    return dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw)


def _operands(case):
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    B, H, W, Cin, Cout, k, d, p, s = case
    r = reference(case)
    dv = dev()
    return (r, nhwc(r['x']).to(dv), nhwc(r['dy']).to(dv), pack_conv_weight(r['w'], cin_pad=Cin).to(dv),
            pack_dgrad_weight(r['w'], cin_pad=Cin, cout_pad=Cout).to(dv))


def _twice(fn, what):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b), f'{what}: two launches differ'
    return a


def _check_all(case, tag):
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight
    B, H, W, Cin, Cout, k, d, p, s = case
    r, xd, dyd, wp, wt = _operands(case)
    geo = dict(kh=k, kw=k, stride=s, pad=p, dil=d)
    y = _twice(lambda: ops.conv2d_nhwc(xd, wp, None, act='none', **geo), f'{tag} forward')
    rel_close(y, nhwc(r['y']), what=f'{tag} forward')
    dw = _twice(lambda: ops.conv2d_wgrad_nhwc(xd, dyd, **geo), f'{tag} wgrad')
    rel_close(dw, pack_conv_weight(r['dw'], cin_pad=Cin), what=f'{tag} wgrad')
    if s == 1:
        dx = _twice(lambda: ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, **geo), f'{tag} dgrad')
        rel_close(dx, nhwc(r['dx']), what=f'{tag} dgrad')
    else:
        with pytest.raises(RuntimeError, match='stride 1 only'):
            ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, **geo)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_dilated_forward_dgrad_wgrad(case):
    _check_all(case, _id(case))


def test_dilated_conv_without_the_streamk_workspace(monkeypatch):
    """The stream-K case again on the one-workgroup-per-tile schedule (a descriptor without the workspace), against the same reference; the
    parametrised run above takes the stream-K schedule (ops attaches the workspace)."""
    from somi_amd import ops
    monkeypatch.setattr(ops, '_conv_workspace', lambda d, dev: None)
    _check_all(STREAMK_CASE, _id(STREAMK_CASE) + ' no workspace')


def test_dilated_dgrad_into_a_channel_slice_and_accumulating():
    """dx into channels [4, 4 + Cin) of a tensor 8 wider filled with a sentinel; the same with accumulate (dx's own slice) and accumulate2 (a second
    tensor's slice): nothing outside the slice changes, the slice holds the sum."""
    from somi_amd import ops
    case = SLICE_CASE
    B, H, W, Cin, Cout, k, d, p, s = case
    r, xd, dyd, wp, wt = _operands(case)
    geo = dict(kh=k, kw=k, stride=s, pad=p, dil=d)
    want = nhwc(r['dx'])

    def outside_untouched(t, what):
        assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + Cin:] == 7.0).all()), f'{what}: wrote outside the slice'

    def plain():
        out = torch.full((B, H, W, Cin + 8), 7.0, device=dev())
        ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, out=out, dx_coff=4, **geo)
        return out
    out = _twice(plain, 'dgrad into a slice')
    outside_untouched(out, 'dgrad into a slice')
    rel_close(out[..., 4:4 + Cin], want, what='dgrad into a slice')

    g = torch.Generator().manual_seed(11)
    have, other = torch.randn(B, H, W, Cin, generator=g), torch.randn(B, H, W, Cin, generator=g)
    other_wide = torch.full((B, H, W, Cin + 8), 7.0)
    other_wide[..., 4:4 + Cin] = other
    other_wide = other_wide.to(dev())

    def accumulating():
        out = torch.full((B, H, W, Cin + 8), 7.0, device=dev())
        out[..., 4:4 + Cin] = have.to(dev())
        ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, out=out, dx_coff=4, accumulate=out, acc_coff=4, accumulate2=other_wide, acc2_coff=4,
                              **geo)
        return out
    out = _twice(accumulating, 'dgrad accumulate + accumulate2')
    outside_untouched(out, 'dgrad accumulate + accumulate2')
    rel_close(out[..., 4:4 + Cin], want + have.double() + other.double(), what='dgrad accumulate + accumulate2')
    assert bool((other_wide[..., :4] == 7.0).all()) and torch.equal(other_wide[..., 4:4 + Cin].cpu(), other), 'accumulate2 was written'


def test_dilated_conv_bf16x3():
    """prec='bf16x3' (two bf16 values per operand, three products, fp32 accumulate) goes through the same dilated addresses: against the exact
    fp32 HIP result at 1e-4, the bar tests/test_kernels_gpu.py states for that mode."""
    from somi_amd import ops
    case = SLICE_CASE
    B, H, W, Cin, Cout, k, d, p, s = case
    r, xd, dyd, wp, wt = _operands(case)
    geo = dict(kh=k, kw=k, stride=s, pad=p, dil=d)

    def run():
        return (ops.conv2d_nhwc(xd, wp, None, act='none', **geo), ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, **geo),
                ops.conv2d_wgrad_nhwc(xd, dyd, **geo))
    want = run()
    ops.CONV_PREC = ops.PREC['bf16x3']
    try:
        got, again = run(), run()
    finally:
        ops.CONV_PREC = 0
    torch.cuda.synchronize()
    for a, a2, b, what in zip(got, again, want, ('forward', 'dgrad', 'wgrad')):
        assert torch.equal(a, a2), f'bf16x3 {what}: two launches differ'
        rel_close(a, b, rel=1e-4, what=f'bf16x3 {what} against the fp32 kernels')
