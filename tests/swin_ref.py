"""CPU restatement of the Swin module set for the tests (models/common.py:1184-1264 WindowAttention, 1147-1168 Mlp, 1267-1358
SwinTransformerLayer, 1361-1378 SwinTransformerBlock, 1632-1637 C3STR), plain PyTorch written from their semantics: torch autograd runs
through it.  tests/test_swin_host.py pins it to the reference's own classes through the tests/golden/block_*.npz fixtures.  What a textbook
Swin would get wrong and this keeps:
  - the frame is transposed: the layer names b, c, w, h = x.shape of an NCHW map and works on (b, h, w, c), so its window rows run along the
    map's W axis, and the relative-position index is (offset along W) * 15 + (offset along H) after the +7 shifts;
  - create_mask's first row group is the index pair (0, -window), not a slice (region_ids below);
  - the mask adds -100, not -inf; padding (zeros, after norm1, no qkv bias) gives tokens with q = k = v = 0 that still are keys of every
    softmax, in shifted and unshifted layers; q is scaled before q k^T and the bias is added after;
  - stochastic depth (drop_path 0.1 when num_heads > 10) is left out: such a layer is restated for eval only."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB

WS = 8


def region_ids(hp, wp, ws=WS, shift=WS // 2):
    """img_mask of create_mask on the padded (hp, wp) map of the layer's own frame.  Along the first axis the first group is the two rows
    0 and hp - ws only (rows between keep id 0; row hp - ws is overwritten by the second group)."""
    ids = torch.zeros(hp, wp, dtype=torch.long)
    row_groups = (torch.tensor([0, hp - ws]), torch.arange(hp - ws, hp - shift), torch.arange(hp - shift, hp))
    col_groups = (torch.arange(0, wp - ws), torch.arange(wp - ws, wp - shift), torch.arange(wp - shift, wp))
    n = 0
    for rows in row_groups:
        for cols in col_groups:
            ids[rows[:, None], cols[None, :]] = n
            n += 1
    return ids


def to_windows(t, ws=WS):
    """(B, A1, A2, C) -> (B * windows, ws * ws, C), windows in (A1 block, A2 block) order, tokens row-major inside a window."""
    B, A1, A2, C = t.shape
    return t.view(B, A1 // ws, ws, A2 // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def from_windows(w, B, A1, A2, ws=WS):
    return w.view(B, A1 // ws, A2 // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, A1, A2, -1)


def shift_mask(hp, wp, ws=WS, shift=WS // 2):
    """(windows, N, N): -100 where the two tokens' region ids differ, else 0."""
    ids = to_windows(region_ids(hp, wp, ws, shift).view(1, hp, wp, 1).float(), ws).squeeze(-1)
    return (ids[:, None, :] != ids[:, :, None]).float() * -100.0


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads, qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = (dim // num_heads) ** -0.5
        wh, ww = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        r, c = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing='ij')
        r, c = r.flatten(), c.flatten()
        index = (r[:, None] - r[None, :] + wh - 1) * (2 * ww - 1) + (c[:, None] - c[None, :] + ww - 1)
        self.register_buffer('relative_position_index', index)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    def forward(self, x, mask=None):
        """x (windows * B, N, C); mask (windows, N, N) or None."""
        n_, N, C = x.shape
        h = self.num_heads
        q, k, v = self.qkv(x).view(n_, N, 3, h, C // h).permute(2, 0, 3, 1, 4)
        s = torch.einsum('bhid,bhjd->bhij', q * self.scale, k)
        s = s + self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, h).permute(2, 0, 1)
        if mask is not None:
            s = (s.view(-1, mask.shape[0], h, N, N) + mask[None, :, None]).view(-1, h, N, N)
        o = torch.einsum('bhij,bhjd->bihd', s.softmax(-1), v).reshape(n_, N, C)
        return self.proj(o)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class SwinTransformerLayer(nn.Module):
    def __init__(self, c, num_heads, window_size=7, shift_size=0, mlp_ratio=4, qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.window_size, self.shift_size, self.mlp_ratio = window_size, shift_size, mlp_ratio
        self.norm1 = norm_layer(c)
        self.attn = WindowAttention(c, (window_size, window_size), num_heads, qkv_bias=qkv_bias)
        self.norm2 = norm_layer(c)
        self.mlp = Mlp(c, int(c * mlp_ratio), act_layer=act_layer)

    def forward(self, x):
        ws, sh = self.window_size, self.shift_size
        t = x.permute(0, 3, 2, 1)                                 # (B, W, H, C): the layer's frame
        B, A1, A2, C = t.shape
        P1, P2 = -(-A1 // ws) * ws, -(-A2 // ws) * ws
        n = F.pad(self.norm1(t), (0, 0, 0, P2 - A2, 0, P1 - A1))
        mask = None
        if sh > 0:
            n = torch.roll(n, (-sh, -sh), (1, 2))
            mask = shift_mask(P1, P2, ws, sh).to(n.device)
        a = from_windows(self.attn(to_windows(n, ws), mask), B, P1, P2, ws)
        if sh > 0:
            a = torch.roll(a, (sh, sh), (1, 2))
        t = t + a[:, :A1, :A2]
        t = t + self.mlp(self.norm2(t))
        return t.permute(0, 3, 2, 1).contiguous()


class SwinTransformerBlock(nn.Module):
    def __init__(self, c1, c2, num_heads, num_layers, window_size=8):
        super().__init__()
        self.conv = OB.Conv(c1, c2) if c1 != c2 else None
        self.window_size, self.shift_size = window_size, window_size // 2
        self.tr = nn.Sequential(*(SwinTransformerLayer(c2, num_heads, window_size, 0 if i % 2 == 0 else self.shift_size)
                                  for i in range(num_layers)))

    def forward(self, x):
        return self.tr(x if self.conv is None else self.conv(x))


class C3STR(OB.C3):
    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = SwinTransformerBlock(c_, c_, c_ // 32, n)


def register(monkeypatch):
    """C3STR in the oracle's parse_model tables (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, C3STR=C3STR))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'C3STR'})
