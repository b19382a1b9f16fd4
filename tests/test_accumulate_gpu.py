"""The accumulate contract the graph walk relies on (Model._backward_walk): every block class that declares `accumulates` adds its input
gradient into a tensor that already holds another consumer's.  One case per declaring class (tests/test_blocks_contract_host.py checks that
none is missing) at the smallest sizes the blocks take: batch 2, maps of at most 8 x 8.  A dropped add or a wrong channel offset is an error
of order one here; the bar is parity.rel_close's default, the one the plain path is held to against the oracle."""
import pytest
import torch
import torch.nn as nn

from parity import check_accumulate_contract

# (constructor arguments, input channels, map size).  GhostBottleneck and C3Ghost start at 16 / 32 channels: below that a GhostConv inside
# gets a hidden width under 4.  ODConv_3rd's input is an unpadded tensor (8 channels); Conv(6, 8, 1) reads a padded one (6 of 8).
CASES = [('Conv', (8, 16, 3), 8, 7), ('Conv', (8, 8, 3, 2), 8, 7), ('Conv', (6, 8, 1), 6, 5), ('DWConv', (8, 8, 3), 8, 7), ('C3', (8, 8), 8, 6),
         ('C3Ghost', (32, 32), 32, 6), ('BottleneckCSP', (8, 8), 8, 6), ('SPPF', (8, 8), 8, 7), ('SPP', (8, 8, (3, 5)), 8, 7), ('SPP', (8, 8), 8, 7),
         ('C2fCBAM', (32, 32), 32, 7), ('ODConv_3rd', (8, 8, 3), 8, 7), ('GhostConv', (8, 8), 8, 7), ('GhostBottleneck', (16, 16, 3, 1), 16, 7),
         ('GhostBottleneck', (16, 16, 3, 2), 16, 7), ('C2f', (8, 8), 8, 6), ('C2fCIB', (8, 8), 8, 6), ('SCDown', (8, 8, 3, 2), 8, 7),
         ('PSA', (128, 128), 128, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,args,c,hw', CASES, ids=[f'{n}{a}'.replace(' ', '') for n, a, _, _ in CASES])
def test_backward_adds_into_a_tensor_that_holds_another_gradient(name, args, c, hw):
    from somi_amd import blocks as MB
    gen = torch.Generator().manual_seed(len(name) + 7 * c + hw)
    blk = getattr(MB, name)(*args)
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn(p_.shape, generator=gen) * (0.5 if p_.dim() < 2 else (2.0 / max(1, p_[0].numel())) ** 0.5))
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
    x = torch.randn(2, hw, hw - 1, MB.pad4(c), generator=gen)
    x[..., c:] = 0
    check_accumulate_contract(blk, x, c, gen, f'{name}{args}')
