"""The premises of tests/test_conv_amp_gpu.py, on the CPU: the rounding of conv_amp_ref is round-to-nearest-even and its split reconstructs the
operand; the three restated products are torch's; and at every case and product the GPU tests use, the bf16 model lies far enough from the
exact result that agreeing with it proves the bf16 form ran, while the bf16x3 model lies far enough from it that the quarter rule leaves an
fp32-accumulating kernel room."""
import pytest
import torch
import torch.nn.functional as F

import conv_amp_ref as R
from support_kernels_ref import POINT

CASE_PRODUCTS = [(name, which) for name, c in R.CASES.items() for which in c.reduced]


def test_rounding_is_to_nearest_even_at_exact_ties():
    """Every element of the tensor lies exactly half-way between two bf16 values.  There the two wrong conversions - truncation and
    round-half-up - give the two different neighbours, and r() gives the one with the even mantissa: truncation's on the elements drawn from an
    even bf16 value (where half-up is wrong), half-up's on the others (where truncation is wrong).  Either wrong conversion is therefore told
    from r() on about half of the tensor, and no element fails to tell the two apart."""
    t = R.ties((4096,), torch.Generator().manual_seed(5))
    got, down, up = R.r(t), R.trunc_bf16(t), R.half_up_bf16(t)
    for v in (got, down, up):
        assert torch.equal(v.bfloat16().float(), v), 'not a bf16 value'
    assert ((t.double() - down.double()).abs() == (up.double() - t.double()).abs()).all(), 'an element is not an exact tie'
    assert (down != up).all()
    even = (R._bits(down) >> 16) & 1 == 0
    assert 0.4 < even.float().mean().item() < 0.6, 'ties of both parities'
    assert torch.equal(got[even], down[even]) and torch.equal(got[~even], up[~even]), 'r() is not round-to-nearest-even'
    assert (got[even] != up[even]).all() and (got[~even] != down[~even]).all()
    assert ((R._bits(got) >> 16) & 1 == 0).all(), 'a tie went to the odd neighbour'
    assert not torch.equal(got, up) and not torch.equal(got, down)


def test_split_reconstructs_the_operand_to_16_bits():
    g = torch.Generator().manual_seed(6)
    t = torch.cat([torch.randn(1 << 16, generator=g), torch.randn(1 << 12, generator=g) * 1e-3, R.ties((1 << 12,), g)])
    hi, lo = R.split(t)
    assert torch.equal(hi, R.r(t)) and torch.equal(lo, R.r(t - hi))
    err = ((hi.double() + lo.double() - t.double()).abs() / t.double().abs()).max().item()
    print(f'hi + lo reproduces the operand to {err:.3e} relative')
    assert err <= 2.0 ** -16


@pytest.mark.parametrize('geom', [(2, 7, 6, 8, 12, 3, 1, 1, 1), (2, 9, 7, 8, 12, 3, 2, 1, 1), (1, 9, 8, 4, 8, 3, 1, 2, 2), (2, 5, 5, 8, 4, 1, 1, 0, 1)],
                         ids=lambda c: 'x'.join(str(v) for v in c))
@pytest.mark.parametrize('per_sample', [False, True], ids=['shared', 'per_sample'])
def test_products_restate_autograd(geom, per_sample):
    """The three products against F.conv2d and its autograd in fp64 (per image with per-sample weights)."""
    B, H, W, Cin, Cout, k, s, p, dil = geom
    g = torch.Generator().manual_seed(sum(geom))
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(((B,) if per_sample else ()) + (Cout, Cin, k, k), generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.cat([F.conv2d(x[b:b + 1], w[b], None, s, p, dil) for b in range(B)]) if per_sample else F.conv2d(x, w, None, s, p, dil)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xd, wd = x.detach(), w.detach()
    for got, want, what in ((R.product('forward', xd, wd, geom, per_sample), y.detach(), 'forward'),
                            (R.product('dgrad', dy, wd, geom, per_sample), x.grad, 'dgrad'),
                            (R.product('wgrad', xd, dy, geom, per_sample), w.grad, 'wgrad')):
        assert got.shape == want.shape, what
        assert R.rel_err(got, want) <= 1e-12, (what, R.rel_err(got, want))


def test_model_modes_are_what_they_say():
    """exact / bf16 / bf16x3 of model() spelled out with r() on one small product; the autograd Function returns the same three products."""
    geom = (2, 6, 5, 8, 8, 3, 1, 1, 1)
    g = torch.Generator().manual_seed(9)
    x, w = torch.randn(2, 8, 6, 5, generator=g), torch.randn(8, 8, 3, 3, generator=g)
    m = R.model('forward', x, w, geom)
    conv = lambda a, b: F.conv2d(a.double(), b.double(), None, 1, 1)                                        # noqa: E731
    xh, wh = R.r(x), R.r(w)
    xl, wl = R.r(x - xh), R.r(w - wh)
    assert torch.equal(m['exact'], conv(x, w)) and torch.equal(m['bf16'], conv(xh, wh))
    assert torch.equal(m['bf16x3'], conv(xh, wh) + conv(xh, wl) + conv(xl, wh))
    for mode in (None, 'bf16', 'bf16x3'):
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = R.AmpConv2d.apply(xa, wa, mode, 1, 1, 1)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(10))
        y.backward(dy)
        key = mode or 'exact'
        assert y.dtype == torch.float32 and torch.equal(y.detach(), m[key].float())
        assert torch.equal(xa.grad, R.model('dgrad', dy, w, geom)[key].float())
        assert torch.equal(wa.grad, R.model('wgrad', x, dy, geom)[key].float())


def test_use_amp_convs_replaces_every_conv_of_a_reference_block():
    from oracle.somi_ref import blocks as OB
    blk = OB.Bottleneck(8, 8)
    assert R.use_amp_convs(blk, 'bf16') == 2
    x = torch.randn(1, 8, 5, 5, generator=torch.Generator().manual_seed(1))
    want = blk.cv2.act(blk.cv2.bn(F.conv2d(R.r(blk.cv1(x)), R.r(blk.cv2.conv.weight), None, 1, 1))) + x
    assert R.rel_err(blk(x), want) <= 1e-6


def test_inputs_stay_in_the_normal_range():
    for name in R.CASES:
        for tied in ((False, True) if name == 'A' else (False,)):        # the ties test runs case A
            inp = R.inputs(name, tied)
            for t in (inp.x, inp.w, inp.dy):
                a = t.abs()
                assert torch.isfinite(t).all() and a.max() < 16.0
                assert (a[a > 0] >= 2.0 ** -100).all(), 'an operand near the subnormal range'
                lo = R.split(t)[1].abs()
                assert (lo[lo > 0] >= 2.0 ** -110).all(), 'a low part near the subnormal range'


@pytest.mark.parametrize('name,which', CASE_PRODUCTS, ids=[f'{n}-{w}' for n, w in CASE_PRODUCTS])
def test_bf16_model_is_separable_from_the_exact_result(name, which):
    """err(model_bf16, exact) >= 100 x POINT of the output range: a result within POINT of the bf16 model cannot have come from the fp32 kernel."""
    _, m = R.case(name)
    d1 = R.rel_err(m[which]['bf16'], m[which]['exact'])
    print(f'{name} {which}: bf16 model {d1:.3e} from exact')
    assert d1 >= 100 * POINT


@pytest.mark.parametrize('name,which', CASE_PRODUCTS, ids=[f'{n}-{w}' for n, w in CASE_PRODUCTS])
def test_bf16x3_model_is_separable_from_fp32_accumulation(name, which):
    """d3 = err(model_x3, exact), n3 = distance between the fp32 and the fp64 accumulation of the same three products on the CPU: n3 <= d3 / 8,
    so the quarter rule of the GPU test (err(got, model_x3) <= d3 / 4) leaves a kernel that accumulates in fp32 room.
    Measured: d3 4.1e-6 ... 6.1e-6, n3 1.1e-7 ... 3.2e-7, d3 / n3 15 ... 45."""
    _, m = R.case(name)
    d3 = R.rel_err(m[which]['bf16x3'], m[which]['exact'])
    n3 = R.rel_err(R.case_fp32(name)[which], m[which]['bf16x3'])
    print(f'{name} {which}: d3 {d3:.3e}, n3 {n3:.3e}, d3 / n3 {d3 / n3:.1f}')
    assert n3 <= d3 / 8
