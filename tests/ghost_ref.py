"""CPU reference of the Ghost module set for the tests (models/common.py:2001-2029, 1798-1803, 9580-9583), built from the oracle's
Conv / C3.  The oracle's Conv takes `act` by keyword, so act=False is no activation - what the build implements."""
import math

import torch
import torch.nn as nn

from oracle.somi_ref import blocks as OB


class DWConv(OB.Conv):
    def __init__(self, c1, c2, k=1, s=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), act=act)


class GhostConv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = OB.Conv(c1, c_, k, s, None, g, act=act)
        self.cv2 = OB.Conv(c_, c_, 5, 1, None, c_, act=act)

    def forward(self, x):
        y = self.cv1(x)
        return torch.cat([y, self.cv2(y)], 1)


class GhostBottleneck(nn.Module):
    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1), DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), OB.Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    def forward(self, x):
        return self.conv(x) + self.shortcut(x)


class C3Ghost(OB.C3):
    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(GhostBottleneck(c_, c_) for _ in range(n)))


def register(monkeypatch):
    """The four names in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    chm = dict(OM._CH_MODULES, GhostConv=GhostConv, GhostBottleneck=GhostBottleneck, DWConv=DWConv, C3Ghost=C3Ghost)
    monkeypatch.setattr(OM, '_CH_MODULES', chm)
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'C3Ghost'})
