"""tests/slices.py on the CPU: check_slice_op must pass a correct op and fail each way an op can break the channel-slice contract, and the
references of the copy kernels must be what torch autograd says they are."""
import pytest
import torch
import torch.nn.functional as F

from parity import nchw, nhwc
from slices import (In, Out, check_slice_op, depth_to_space_ref, embed, resample_copy_ref, resample_reduce_ref, space_to_depth_ref)

B, H, W, C = 2, 3, 5, 8
X_CS, X_COFF, ACC_CS, ACC_COFF, Y_CS, Y_COFF = 20, 4, 16, 8, 24, 12


def _case():
    g = torch.Generator().manual_seed(5)
    x, acc = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)
    scale = torch.rand(C, generator=g) + 0.5
    want = {'y': x.double() * scale.double() + acc.double()}
    inputs = {'x': In(x, X_CS, X_COFF), 'acc': In(acc, ACC_CS, ACC_COFF), 'scale': scale}
    return inputs, {'y': Out((B, H, W), Y_CS, Y_COFF, C)}, want


def _op(fault=None):
    """y[slice] = x[slice] * scale + acc[slice] in torch, with one deliberate fault."""
    def run(b):
        x = b['x'][..., X_COFF:X_COFF + C]
        a0 = 0 if fault == 'acc_coff' else ACC_COFF
        y = x * b['scale'] + b['acc'][..., a0:a0 + C]
        if fault == 'read':                                   # one neighbour channel leaks in, weighted by zero: invisible unless it is NaN / Inf
            y = y + 0.0 * b['x'][..., X_COFF + C:X_COFF + C + 1]
        if fault == 'read_finite':                            # ... and one that changes the values a little
            y = y + 1e-6 * b['x'][..., X_COFF - 1:X_COFF]
        if fault == 'nan':
            y = torch.where(torch.isnan(b['x'][..., :1]), torch.full_like(y, float('nan')), y)
        n = C + 1 if fault == 'write' else C
        b['y'][..., Y_COFF:Y_COFF + n] = F.pad(y, (0, n - C))
    return run


def test_check_slice_op_passes_a_correct_op(capsys):
    inputs, outputs, want = _case()
    got = check_slice_op(_op(), inputs, outputs, want, rel=1e-5, what='probe', device='cpu')
    assert got['y'].shape == (B, H, W, C) and got['y'].dtype == torch.float32        # the dense content of the output slice
    assert 'probe: worst ratio to the bar' in capsys.readouterr().out


@pytest.mark.parametrize('fault,message', [('write', 'values outside the slice'),
                                           ('read', 'not finite when the channels around the slices hold nan'),
                                           ('read_finite', 'depends on channels outside the input slices'),
                                           ('acc_coff', 'probe: y: max err'),
                                           ('nan', 'not finite when the channels around the slices hold nan')])
def test_check_slice_op_fails_each_broken_contract(fault, message):
    inputs, outputs, want = _case()
    with pytest.raises(AssertionError, match=message):
        check_slice_op(_op(fault), inputs, outputs, want, rel=1e-5, what='probe', device='cpu')


def test_check_slice_op_accumulates_onto_the_previous_content():
    g = torch.Generator().manual_seed(6)
    x, prev = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)

    def run(b, keep=True):
        b['y'][..., Y_COFF:Y_COFF + C] = 2.0 * b['x'][..., X_COFF:X_COFF + C] + (b['y'][..., Y_COFF:Y_COFF + C] if keep else 0.0)
    outputs = {'y': Out((B, H, W), Y_CS, Y_COFF, C, prev=prev, accumulate=True)}
    check_slice_op(run, {'x': In(x, X_CS, X_COFF)}, outputs, {'y': 2.0 * x.double()}, rel=1e-6, what='probe', device='cpu')
    with pytest.raises(AssertionError, match='probe: y: max err'):
        check_slice_op(lambda b: run(b, keep=False), {'x': In(x, X_CS, X_COFF)}, outputs, {'y': 2.0 * x.double()}, rel=1e-6, what='probe',
                       device='cpu')


def test_check_slice_op_exact_bar_and_missed_writes():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, C, generator=g)

    def copy(b, eps=0.0, rows=B):
        b['y'][:rows, ..., Y_COFF:Y_COFF + C] = b['x'][:rows, ..., X_COFF:X_COFF + C] * (1.0 + eps)
    args = ({'x': In(x, X_CS, X_COFF)}, {'y': Out((B, H, W), Y_CS, Y_COFF, C)}, {'y': x})
    check_slice_op(copy, *args, bars={'y': 'exact'}, what='probe', device='cpu')
    with pytest.raises(AssertionError, match='not bit-exact'):
        check_slice_op(lambda b: copy(b, eps=1e-7), *args, bars={'y': 'exact'}, what='probe', device='cpu')
    with pytest.raises(AssertionError, match='not bit-exact'):                   # the last image is left as it was: stale values, not zeros
        check_slice_op(lambda b: copy(b, rows=B - 1), *args, bars={'y': 'exact'}, what='probe', device='cpu')


def test_check_slice_op_bars_per_result_and_references_from_results():
    """A dense result returned by run is held to its own bar (rel, or rel + atol), and a reference may be a function of the run's results."""
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(8))

    def run(b, off=0.0):
        b['y'][..., Y_COFF:Y_COFF + C] = b['x'][..., X_COFF:X_COFF + C]
        return {'sum': b['y'][..., Y_COFF:Y_COFF + C].sum((0, 1, 2)) + off}
    args = ({'x': In(x, X_CS, X_COFF)}, {'y': Out((B, H, W), Y_CS, Y_COFF, C)}, {'y': x, 'sum': lambda r: r['y'].double().sum((0, 1, 2))})
    check_slice_op(run, *args, bars={'y': 'exact', 'sum': 1e-5}, what='probe', device='cpu')
    check_slice_op(lambda b: run(b, 0.01), *args, bars={'y': 'exact', 'sum': {'rel': 1e-5, 'atol': 0.02}}, what='probe', device='cpu')
    with pytest.raises(AssertionError, match='probe: sum: max err'):
        check_slice_op(lambda b: run(b, 0.01), *args, bars={'y': 'exact', 'sum': 1e-5}, what='probe', device='cpu')
    with pytest.raises(AssertionError, match='differ in names'):
        check_slice_op(run, args[0], args[1], {'y': x}, what='probe', device='cpu')


def test_embed_fills():
    t = torch.arange(24.0).view(1, 2, 3, 4)
    a, a2, b_ = embed(t, 12, 4, 'rand_a'), embed(t, 12, 4, 'rand_a'), embed(t, 12, 4, 'rand_b')
    for buf in (a, b_, embed(t, 12, 4, 'nan'), embed(t, 12, 4, 7.0)):
        assert buf.shape == (1, 2, 3, 12) and torch.equal(buf[..., 4:8], t)
    assert torch.equal(a, a2) and torch.isfinite(a).all() and torch.isfinite(b_).all()
    assert (a[..., :4] != b_[..., :4]).all() and (a[..., 8:] != b_[..., 8:]).all()
    assert not torch.equal(a, embed(t, 12, 4, 'rand_a', salt=1))
    assert torch.isnan(embed(t, 12, 4, 'nan')[..., :4]).all() and torch.isnan(embed(t, 12, 4, 'nan')[..., 8:]).all()
    assert (embed(t, 12, 4, 7.0)[..., 8:] == 7.0).all()
    with pytest.raises(AssertionError, match='does not fit'):
        embed(t, 6, 4, 'nan')


@pytest.mark.parametrize('up', [0, 1, 2, 3])
def test_resample_references_are_nearest_upsampling_and_its_adjoint(up):
    g = torch.Generator().manual_seed(up)
    lo = torch.randn(2, 3, 5, 4, generator=g, dtype=torch.float64)
    x = nchw(lo).clone().requires_grad_(True)
    y = F.interpolate(x, scale_factor=2 ** up, mode='nearest')
    assert torch.equal(resample_copy_ref(lo, up), nhwc(y.detach()))
    dy = torch.randint(-8, 9, y.shape, generator=g).double()                      # integers: the block sums are exact in any order
    y.backward(dy)
    assert torch.equal(resample_reduce_ref(nhwc(dy), up), nhwc(x.grad))


@pytest.mark.parametrize('c', [3, 8])
def test_space_to_depth_references_are_the_focus_cat_order_and_its_gradient(c):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(2, c, 6, 10, generator=g, dtype=torch.float64).requires_grad_(True)
    y = torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)      # models/common.py:1996
    assert torch.equal(space_to_depth_ref(nhwc(x.detach())), nhwc(y.detach()))
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    assert torch.equal(depth_to_space_ref(nhwc(dy)), nhwc(x.grad))
    assert torch.equal(depth_to_space_ref(space_to_depth_ref(nhwc(x.detach()))), nhwc(x.detach()))
