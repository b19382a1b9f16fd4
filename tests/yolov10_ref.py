"""CPU restatement of the YOLOv10 module set for the tests (models/common.py:2638-2658 C2f, 7192-7255 SCDown / AttentionPSA / PSA,
8981-9013 CIB / C2fCIB), built from the oracle's Conv / Bottleneck and written from their semantics: torch autograd runs through it.
tests/test_yolov10_host.py pins it to the reference's own classes through the tests/golden/block_*.npz fixtures."""
import torch
import torch.nn as nn

from oracle.somi_ref import blocks as OB


class C2f(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = OB.Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = OB.Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(OB.Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        for m in self.m:
            y.append(m(y[-1]))
        return self.cv2(torch.cat(y, 1))


class SCDown(nn.Module):
    def __init__(self, c1, c2, k, s):
        super().__init__()
        self.cv1 = OB.Conv(c1, c2, 1, 1)
        self.cv2 = OB.Conv(c2, c2, k=k, s=s, g=c2, act=False)

    def forward(self, x):
        return self.cv2(self.cv1(x))


class CIB(nn.Module):
    def __init__(self, c1, c2, shortcut=True, e=0.5, lk=False):
        super().__init__()
        if lk:
            raise NotImplementedError('RepVGGDW is not restated')
        c_ = int(c2 * e)
        self.cv1 = nn.Sequential(OB.Conv(c1, c1, 3, g=c1), OB.Conv(c1, 2 * c_, 1), OB.Conv(2 * c_, 2 * c_, 3, g=2 * c_), OB.Conv(2 * c_, c2, 1),
                                 OB.Conv(c2, c2, 3, g=c2))
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv1(x) if self.add else self.cv1(x)


class C2fCIB(C2f):
    def __init__(self, c1, c2, n=1, shortcut=False, lk=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(CIB(self.c, self.c, shortcut, e=1.0, lk=lk) for _ in range(n))


class AttentionPSA(nn.Module):
    """Per head h of the qkv output: channels h*(2*key_dim + head_dim) + [0, key_dim) q, then key_dim of k, then head_dim of v."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim ** -0.5
        self.qkv = OB.Conv(dim, dim + 2 * self.key_dim * num_heads, 1, act=False)
        self.proj = OB.Conv(dim, dim, 1, act=False)
        self.pe = OB.Conv(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x):
        B, C, H, W = x.shape
        kd, hd = self.key_dim, self.head_dim
        t = self.qkv(x).reshape(B, self.num_heads, 2 * kd + hd, H * W)
        q, k, v = t[:, :, :kd], t[:, :, kd:2 * kd], t[:, :, 2 * kd:]
        p = (torch.einsum('bhdi,bhdj->bhij', q, k) * self.scale).softmax(-1)
        o = torch.einsum('bhij,bhdj->bhdi', p, v).reshape(B, C, H, W)
        return self.proj(o + self.pe(v.reshape(B, C, H, W)))


class PSA(nn.Module):
    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = OB.Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = OB.Conv(2 * self.c, c1, 1)
        self.attn = AttentionPSA(self.c, attn_ratio=0.5, num_heads=self.c // 64)
        self.ffn = nn.Sequential(OB.Conv(self.c, self.c * 2, 1), OB.Conv(self.c * 2, self.c, 1, act=False))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), dim=1)
        b = b + self.attn(b)
        b = b + self.ffn(b)
        return self.cv2(torch.cat((a, b), 1))


def register(monkeypatch):
    """The four yaml names in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    chm = dict(OM._CH_MODULES, C2f=C2f, SCDown=SCDown, C2fCIB=C2fCIB, PSA=PSA)
    monkeypatch.setattr(OM, '_CH_MODULES', chm)
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'C2f', 'C2fCIB'})
