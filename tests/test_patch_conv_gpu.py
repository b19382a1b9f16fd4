"""Patch-embedding convolutions (kernel = stride = p, no padding: MultiSEAM's DcovN stems, models/common.py:8508-8511) on the MI355X: forward,
data gradient and weight gradient of the dense implicit-GEMM family (conv_igemm.hip, conv_wgrad.hip) through `ops`, against fp64 F.conv2d /
torch.nn.grad.conv2d_input / conv2d_weight on the CPU.  Bar: parity.rel_close's default, 1e-3 of the result's largest value (the fp32 matrix
instruction is exact fp32 arithmetic: ~1e-6 in practice).  Every launch runs twice and must be bit-identical.

p = 3 and 5 (9 / 25 taps) run the FAST instantiations with p^2 parity classes in the data gradient; p = 7 (49 taps) with Cin % 32 == 0 runs the
PATCH instantiation; Cin % 32 != 0 runs the generic path.  The rows and columns of dx beyond Ho * p / Wo * p, which no tap reaches, are exact zeros
when written and keep what they held with `accumulate`."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from parity import nhwc, rel_close

pytestmark = pytest.mark.gpu

# B, H, W, Cin, Cout, k, stride, pad
GRID = [(2, 15, 17, cin, cout, p, p, 0) for p in (3, 5, 7) for cin, cout in ((32, 32), (8, 12))]
P7 = [
    (1, 7, 7, 32, 32, 7, 7, 0),               # one patch: Ho = Wo = 1
    (2, 14, 21, 32, 32, 7, 7, 0),             # no remainder
    (1, 84, 91, 32, 32, 7, 7, 0),             # 156 output rows: more than one 128-row tile and a ragged last one
    (1, 84, 91, 32, 160, 7, 7, 0),            # two N tiles
]
CONTROLS = [(2, 15, 17, 32, 32, 3, 1, 1), (2, 15, 17, 32, 32, 3, 2, 1)]     # the old paths, through the same calls
CASES = GRID + P7 + CONTROLS


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _id(c):
    return 'x'.join(map(str, c[:5])) + f'-k{c[5]}s{c[6]}p{c[7]}'


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fp32 tensors and the fp64 results, computed once and shared (nobody writes to them)."""
    B, H, W, Cin, Cout, k, s, p = case
    g = torch.Generator().manual_seed(sum(v * (i + 1) for i, v in enumerate(case)))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    x64, w64 = x.double(), w.double()
    y = F.conv2d(x64, w64, None, s, p)
    dy = torch.randn(y.shape, generator=g)
    dx = torch.nn.grad.conv2d_input(x64.shape, w64, dy.double(), s, p)
    dw = torch.nn.grad.conv2d_weight(x64, w64.shape, dy.double(), s, p)
    return dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw)


def _operands(case):
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    B, H, W, Cin, Cout, k, s, p = case
    r = reference(case)
    dv = dev()
    return (r, nhwc(r['x']).to(dv), nhwc(r['dy']).to(dv), pack_conv_weight(r['w'], cin_pad=Cin).to(dv),
            pack_dgrad_weight(r['w'], cin_pad=Cin, cout_pad=Cout).to(dv))


def _twice(fn, what):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b), f'{what}: two launches differ'
    return a


def _run(case):
    """-> (forward, data gradient, weight gradient) of the case, each launched twice."""
    from somi_amd import ops
    B, H, W, Cin, Cout, k, s, p = case
    r, xd, dyd, wp, wt = _operands(case)
    geo = dict(kh=k, kw=k, stride=s, pad=p)
    tag = _id(case)
    return (_twice(lambda: ops.conv2d_nhwc(xd, wp, None, act='none', **geo), f'{tag} forward'),
            _twice(lambda: ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, **geo), f'{tag} dgrad'),
            _twice(lambda: ops.conv2d_wgrad_nhwc(xd, dyd, **geo), f'{tag} wgrad'))


def _remainder(case, t):
    """The rows and columns of an NHWC dx that no tap of a k = s conv reaches, flattened (empty when the map is a whole number of patches)."""
    B, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = H // k, W // k
    return torch.cat([t[:, Ho * k:].reshape(-1), t[:, :Ho * k, Wo * k:].reshape(-1)])


def _check_all(case, tag):
    from somi_amd.pack import pack_conv_weight
    B, H, W, Cin, Cout, k, s, p = case
    r = reference(case)
    y, dx, dw = _run(case)
    rel_close(y, nhwc(r['y']), what=f'{tag} forward')
    rel_close(dx, nhwc(r['dx']), what=f'{tag} dgrad')
    rel_close(dw, pack_conv_weight(r['dw'], cin_pad=Cin), what=f'{tag} wgrad')
    if k == s and p == 0:
        assert not _remainder(case, dx).any(), f'{tag} dgrad: a pixel beyond Ho * p / Wo * p is not exactly zero'


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_patch_forward_dgrad_wgrad(case):
    _check_all(case, _id(case))


@pytest.mark.parametrize('case', [GRID[4], P7[2], P7[3]], ids=_id)
def test_patch_conv_without_the_streamk_workspace(case, monkeypatch):
    """p = 7 again on the one-workgroup-per-tile schedule (a descriptor without the workspace), against the same reference; the parametrised run
    above takes the stream-K schedule (ops attaches the workspace, and 49 K-tiles per channel chunk over one or two tiles get cut)."""
    from somi_amd import ops
    monkeypatch.setattr(ops, '_conv_workspace', lambda d, dev: None)
    _check_all(case, _id(case) + ' no workspace')


@pytest.mark.parametrize('case', GRID, ids=_id)
def test_patch_dgrad_into_a_channel_slice_and_accumulating(case):
    """dx into channels [4, 4 + Cin) of a tensor 8 wider filled with the sentinel 7.0: nothing outside the slice changes; inside it the pixels no
    tap reaches are exactly 0.0 when written and exactly what they held with `accumulate` (dx's own slice)."""
    from somi_amd import ops
    B, H, W, Cin, Cout, k, s, p = case
    r, xd, dyd, wp, wt = _operands(case)
    geo = dict(kh=k, kw=k, stride=s, pad=p)
    want = nhwc(r['dx'])
    tag = _id(case)
    assert _remainder(case, want).numel() > 0, 'the shape leaves a remainder for every patch size'

    def outside_untouched(t, what):
        assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + Cin:] == 7.0).all()), f'{what}: wrote outside the slice'

    def plain():
        out = torch.full((B, H, W, Cin + 8), 7.0, device=dev())
        ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, out=out, dx_coff=4, **geo)
        return out
    out = _twice(plain, f'{tag} dgrad into a slice')
    outside_untouched(out, f'{tag} dgrad into a slice')
    rel_close(out[..., 4:4 + Cin], want, what=f'{tag} dgrad into a slice')
    assert bool((_remainder(case, out[..., 4:4 + Cin]) == 0.0).all()), f'{tag}: an unreached pixel of the slice is not exactly 0.0'

    have = torch.randn(B, H, W, Cin, generator=torch.Generator().manual_seed(11))

    def accumulating():
        out = torch.full((B, H, W, Cin + 8), 7.0, device=dev())
        out[..., 4:4 + Cin] = have.to(dev())
        ops.conv2d_dgrad_nhwc(dyd, wt, B=B, H=H, W=W, cin=Cin, out=out, dx_coff=4, accumulate=out, acc_coff=4, **geo)
        return out
    out = _twice(accumulating, f'{tag} dgrad accumulate')
    outside_untouched(out, f'{tag} dgrad accumulate')
    rel_close(out[..., 4:4 + Cin], want + have.double(), what=f'{tag} dgrad accumulate')
    assert torch.equal(_remainder(case, out[..., 4:4 + Cin]).cpu(), _remainder(case, have)), f'{tag}: accumulate changed an unreached pixel'


@pytest.mark.parametrize('prec', ['bf16', 'bf16x3'])
def test_patch_conv_reduced_precision_requests_run_fp32(prec):
    """prec requested at p = 7: the PATCH instantiation of the forward and the data gradient has no reduced-precision form and answers with the
    fp32 result, bit for bit.  (The weight gradient keeps its own bf16 forms: checked against the fp32 kernel at the bars tests/test_kernels_gpu.py
    states for them, 2e-2 and 1e-4.)"""
    from somi_amd import ops
    case = P7[3]
    want = _run(case)
    ops.CONV_PREC = ops.PREC[prec]
    try:
        got = _run(case)
    finally:
        ops.CONV_PREC = 0
    assert torch.equal(got[0], want[0]), f'{prec} forward at p = 7 differs from fp32'
    assert torch.equal(got[1], want[1]), f'{prec} dgrad at p = 7 differs from fp32'
    rel_close(got[2], want[2], rel=2e-2 if prec == 'bf16' else 1e-4, what=f'{prec} wgrad against the fp32 kernel')
