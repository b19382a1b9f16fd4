"""tests/parity.py on the CPU: the comparison bar and the block procedure must actually fail what they are there to fail."""
import pytest
import torch

from parity import check_block, nchw, nhwc, rel_close


def test_rel_close_rejects_a_shape_mismatch():
    with pytest.raises(AssertionError, match='probe: shape'):
        rel_close(torch.zeros(2, 3), torch.zeros(3, 2), what='probe')


def test_rel_close_rejects_a_nan():
    got = torch.tensor([1.0, float('nan')])
    with pytest.raises(AssertionError, match='probe: not finite'):
        rel_close(got, torch.ones(2), rel=1e30, atol=1e30, what='probe')


@pytest.mark.parametrize('atol', [0.0, 2e-5])
def test_rel_close_bar_is_rel_times_scale_plus_atol(atol):
    want = torch.tensor([4.0, -1.0, 0.0], dtype=torch.float64)
    bar = 1e-3 * 4.0 + atol
    rel_close(want + torch.tensor([0.0, 0.0, 0.999 * bar], dtype=torch.float64), want, atol=atol, what='below')
    with pytest.raises(AssertionError, match='above: max err'):
        rel_close(want + torch.tensor([0.0, 0.0, 1.001 * bar], dtype=torch.float64), want, atol=atol, what='above')


def test_rel_close_floor_and_plain_numbers():
    zero = torch.zeros(3, dtype=torch.float64)
    rel_close(zero + 1e-16, zero, what='default floor')           # bar 1e-3 * 1e-12
    with pytest.raises(AssertionError):
        rel_close(zero + 1e-14, zero, what='default floor')
    with pytest.raises(AssertionError):
        rel_close(zero + 1e-16, zero, what='tight floor', floor=1e-30)
    rel_close(1.0005, 1.0, what='python floats')                  # as_tensor on both operands


def _autograd_block(corrupt):
    """`Ours` for check_block on the CPU: the oracle Conv under torch autograd behind the Act protocol of the hand-written blocks, its
    gradient of the parameter `corrupt` pushed past the bar."""
    from oracle.somi_ref import blocks as OB
    from somi_amd.blocks import Act

    class Block(OB.Conv):
        def forward(self, a):
            self._x = nchw(a.t[..., a.coff:a.coff + a.c]).clone().requires_grad_(self.training)
            self._y = super().forward(self._x)
            return Act(nhwc(self._y.detach()))

        def backward(self, d):
            self._y.backward(nchw(d.t))
            if corrupt:
                g = dict(self.named_parameters())[corrupt].grad
                g.view(-1)[0] += 0.01 * g.abs().max() + 1e-3
            return Act(nhwc(self._x.grad))
    return Block


@pytest.mark.parametrize('corrupt', [None, 'conv.weight', 'bn.bias'])
def test_check_block_names_the_parameter_whose_gradient_is_off(corrupt):
    from oracle.somi_ref import blocks as OB
    mine = _autograd_block(corrupt)

    def make(M):
        return (OB.Conv if M is OB else mine)(8, 16, 3, 1)
    if corrupt is None:
        check_block(make, OB, (2, 8, 7, 9), 'fake', device='cpu')
    else:
        with pytest.raises(AssertionError, match=f'fake: d{corrupt}: max err'):
            check_block(make, OB, (2, 8, 7, 9), 'fake', device='cpu')


def test_check_block_insists_on_every_gradient():
    from oracle.somi_ref import blocks as OB
    mine = _autograd_block(None)

    class Forgetful(mine):
        def backward(self, d):
            dx = super().backward(d)
            self.bn.weight.grad = None
            return dx

    def make(M):
        return (OB.Conv if M is OB else Forgetful)(8, 16, 3, 1)
    with pytest.raises(AssertionError, match='fake: bn.weight has no gradient'):
        check_block(make, OB, (2, 8, 7, 9), 'fake', device='cpu')
