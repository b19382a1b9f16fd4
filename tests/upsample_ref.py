"""CPU restatement of the two learned 2x upsamplers of the neck (models/common.py:4450-4490 CARAFE, 4246-4309 DySample with style='lp' and no
dyscope) on the oracle's Conv, written from their semantics so that torch autograd runs through them without nn.Unfold of the upsampled map or
grid_sample, and a parse_model that takes the two names.  tests/test_upsample_host.py pins the restatement to the reference's own classes through
the tests/golden/block_{carafe,carafe_k3,dysample,dysample_g2}.npz fixtures."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


def carafe_reassemble(x, logits, k):
    """out[c, 2h+dy, 2w+dx] = sum_{a,b} softmax_t(logits[t*4 + dy*2 + dx, h, w])[a*k+b] * x[c, h+a-r, w+b-r], x zero outside the map.
    x (B,C,H,W), logits (B,4*k*k,H,W) -> (B,C,2H,2W)."""
    B, C, H, W = x.shape
    r = k // 2
    p = torch.softmax(logits.view(B, k * k, 4, H, W), 1)
    xp = F.pad(x, [r, r, r, r])
    out = x.new_zeros(B, C, 4, H, W)
    for a in range(k):
        for b in range(k):
            out = out + p[:, a * k + b].unsqueeze(1) * xp[:, :, a:a + H, b:b + W].unsqueeze(2)
    return F.pixel_shuffle(out.reshape(B, C * 4, H, W), 2)


class CARAFE(nn.Module):
    def __init__(self, c, k_enc=3, k_up=5, c_mid=64, scale=2):
        super().__init__()
        assert scale == 2
        self.scale, self.k_up = scale, k_up
        self.comp = OB.Conv(c, c_mid)
        self.enc = OB.Conv(c_mid, (scale * k_up) ** 2, k=k_enc, act=False)

    def forward(self, x):
        return carafe_reassemble(x, self.enc(self.comp(x)), self.k_up)


def dysample_coords(o, init_pos, groups):
    """Sampling positions in pixels BEFORE the border clamp: o (B,8G,H,W) the raw offset conv output -> sx, sy (B,G,4,H,W), sub-pixel s = dy*2+dx."""
    B, _, H, W = o.shape
    off = (o * 0.25 + init_pos).view(B, 2, groups, 4, H, W)
    sx = off[:, 0] + torch.arange(W, dtype=o.dtype).view(1, 1, 1, 1, W)
    sy = off[:, 1] + torch.arange(H, dtype=o.dtype).view(1, 1, 1, H, 1)
    return sx, sy


def dysample_sample(x, o, init_pos, groups):
    """Bilinear sample of x[g*C/G:(g+1)*C/G] at (sx, sy) clamped to the map (gradient zero where clamped, like grid_sample's border padding)."""
    B, C, H, W = x.shape
    G, Cg = groups, C // groups
    sx, sy = dysample_coords(o, init_pos, G)
    sx, sy = sx.clamp(0, W - 1), sy.clamp(0, H - 1)
    x0, y0 = sx.detach().floor().clamp(0, max(W - 2, 0)), sy.detach().floor().clamp(0, max(H - 2, 0))
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    xg = x.view(B, G, Cg, H * W)

    def tap(yy, xx):
        idx = (yy * W + xx).view(B, G, 1, 4 * H * W).expand(B, G, Cg, 4 * H * W)
        return xg.gather(3, idx).view(B, G, Cg, 4, H, W)
    fx, fy = fx.unsqueeze(2), fy.unsqueeze(2)
    v = (tap(y0, x0) * (1 - fx) + tap(y0, x1) * fx) * (1 - fy) + (tap(y1, x0) * (1 - fx) + tap(y1, x1) * fx) * fy
    return F.pixel_shuffle(v.reshape(B, C * 4, H, W), 2)


class DySample(nn.Module):
    def __init__(self, in_channels, scale=2, style='lp', groups=4, dyscope=False):
        super().__init__()
        assert scale == 2 and style == 'lp' and not dyscope and in_channels % groups == 0
        self.scale, self.style, self.groups = scale, style, groups
        self.offset = nn.Conv2d(in_channels, 2 * groups * scale ** 2, 1)
        nn.init.normal_(self.offset.weight, 0, 0.001)
        nn.init.constant_(self.offset.bias, 0)
        h = torch.tensor([-0.25, 0.25])
        px, py = h.view(1, 1, 2).expand(groups, 2, 2), h.view(1, 2, 1).expand(groups, 2, 2)     # x follows dx, y follows dy
        self.register_buffer('init_pos', torch.stack([px, py]).reshape(1, -1, 1, 1).clone())

    def forward(self, x):
        return dysample_sample(x, self.offset(x), self.init_pos, self.groups)


_NAMES = {'CARAFE': CARAFE, 'DySample': DySample}


def _row_channels(d, ch):
    """Output channels of every row, by the parser's own bookkeeping (models/yolo.py:1480-1648 for the names the oracle takes)."""
    from oracle.somi_ref import model as OM
    anchors, nc, gw = d['anchors'], d['nc'], d['width_multiple']
    no = ((len(anchors[0]) // 2) if isinstance(anchors, list) else anchors) * (nc + 5)
    chs, c2 = list(ch), ch[-1]
    for i, (f, n, name, args) in enumerate(d['backbone'] + d['head']):
        name = OM._ALIASES.get(name, name)
        if name in OM._CH_MODULES or name == 'ODConv_3rd':
            c2 = args[0] if args[0] == no else OB.make_divisible(args[0] * gw, 8)
        elif name == 'Concat':
            c2 = sum(chs[x] for x in f)
        elif name not in ('BiFPN', 'DecoupledDetect', 'Detect'):  # channels pass through (BiFPN keeps the parser's last value)
            c2 = chs[f]
        if i == 0:
            chs = []
        chs.append(c2)
    return chs


def register(monkeypatch):
    """A CARAFE / DySample row stands in the oracle's parse_model as an nn.Upsample row, which takes the same branch (c2 = ch[f]); the module itself
    is built here on the channel count of its source and put in its place (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    inner = OM.parse_model

    def parse_model(d, ch):
        rows = d['backbone'] + d['head']
        chs = _row_channels(d, ch)
        swapped = dict(d, backbone=[], head=[[f, n, 'nn.Upsample', [None, 2, 'nearest']] if name in _NAMES else [f, n, name, args]
                                             for f, n, name, args in rows])
        seq, save = inner(swapped, ch)
        layers = list(seq)
        for i, (f, n, name, args) in enumerate(rows):
            if name in _NAMES:
                m_ = _NAMES[name](chs[i], *args)                  # c2 = ch[f]: the row's own output channels
                m_.i, m_.f, m_.type = i, f, name
                m_.np = sum(p.numel() for p in m_.parameters())
                layers[i] = m_
        return nn.Sequential(*layers), save
    monkeypatch.setattr(OM, 'parse_model', parse_model)
