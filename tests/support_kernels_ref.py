"""Cases, inputs and references of tests/test_support_kernels_gpu.py: the depthwise 3x3 backward, LayerNorm+GELU backward, BiFPN, centre-feature-scale
blend, the two detect decodes and their raw backwards, the test-time-augmentation resample / descale and the image ingest.

Every reference is the same operation in plain torch (autograd for the gradients) or the oracle module, evaluated in the dtype it is handed: float64
is what the kernels are compared with, float32 is what tests/test_support_kernels_host.py holds to half the kernels' bar, so that the inputs
themselves leave the kernels room.  The hand-written restatements (scale_img, descale_pred, the NHWC / anchor plumbing around the oracle's detect
heads) are held to the oracle at 1e-12 there.  A plain module, imported like odconv_ref; inputs are float32 CPU tensors drawn from a generator seeded
by the case, so both test files see the same numbers."""
import math
import re
import zlib
from types import SimpleNamespace as NS

import torch
import torch.nn as nn
import torch.nn.functional as F

POINT = 1e-5          # pointwise results, of max |want|
REDUCED = 2e-5        # sums over pixels (dw, dbias, dgamma, dbeta, BiFPN dw, dlogit), of max |want|
DESCALE = 1e-6
RESAMPLE_FLOOR = 1e-6
EPS_LN = 1e-6


def ident(case):
    return re.sub(r'[^0-9A-Za-z.]+', '-', str(case)).strip('-')


def gen(name, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((name, case)).encode()))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def leaf(t, dtype):
    """A fresh leaf of autograd in `dtype` (the inputs themselves stay as they are)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def rel_err(got, want):
    got, want = got.detach().double(), want.detach().double()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-12)


# ------------------------------------------------------------------------------------------------------------------- depthwise 3x3
# (B, C, H, W).  The weight-gradient kernel gives a workgroup 256 (column, channel quad) items, B * W * C/4 of them in all ("chunks" of 256):
# C/4 = 1 (256 lanes share a quad), C/4 = 256 (none do), a single partly filled chunk, W = H = 1, 16-row segments of the data gradient (H >= 64)
# with a last segment of 6 rows and of one row, 8-row segments with a last one of one row (H = 9), 20 chunks (one trip of the final reduction's
# two-way loop for some groups only) and 34 chunks (a second trip).
DW_BWD_CASES = [(2, 4, 9, 7), (1, 1024, 5, 3), (2, 32, 1, 1), (2, 32, 64, 5), (1, 8, 65, 3), (2, 256, 9, 40), (3, 256, 70, 45)]
DW_BWD_REFUSED = (2, 24, 5, 3)                       # C/4 = 6 does not divide 256
DW_FWD_CASES = [(2, 32, 70, 5, True), (2, 32, 9, 7, True), (2, 32, 70, 5, False), (2, 32, 9, 7, False)]     # (B, C, H, W, bias)


def dw_chunks(case):
    B, C, H, W = case[:4]
    return -(-B * W * (C // 4) // 256)


def dw_pack(w):
    """(C, 1, 3, 3) -> the kernels' tap-major (9, C)."""
    return w[:, 0].permute(1, 2, 0).reshape(9, w.shape[0]).contiguous()


def dw_inputs(case):
    B, C, H, W = case[:4]
    g = gen('dw', case)
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    return NS(x=r(B, C, H, W), w=r(C, 1, 3, 3) * 0.4, b=r(C) * 0.3, dy=r(B, C, H, W), acc=r(B, C, H, W), dw0=r(9, C), db0=r(C),
              ps=torch.rand(C, generator=g) + 0.5, pt=r(C) * 0.5, res=r(B, C, H, W))


def dw_backward(c, dtype):
    """-> dx (NHWC), dw (9, C), db (C) of y = conv2d(x, w, b, padding=1, groups=C) under dy."""
    x, w, b = (leaf(v, dtype) for v in (c.x, c.w, c.b))
    F.conv2d(x, w, b, 1, 1, groups=x.shape[1]).backward(c.dy.to(dtype))
    return NS(dx=nhwc(x.grad), dw=dw_pack(w.grad), db=b.grad)


def dw_forward(c, dtype, bias):
    """gelu(conv(x) + b) * post_scale + post_shift + residual, NHWC."""
    t = lambda v: v.to(dtype)                                                                     # noqa: E731
    y = F.gelu(F.conv2d(t(c.x), t(c.w), t(c.b) if bias else None, 1, 1, groups=c.x.shape[1]))
    return nhwc(y * t(c.ps)[None, :, None, None] + t(c.pt)[None, :, None, None] + t(c.res))


# ------------------------------------------------------------------------------------------------------------------- LayerNorm + GELU backward
# (npix, C): one wave per row, at most 1024 workgroups = 4096 waves.  C = 4 (60 idle lanes), 260 (a second trip of the lane loop for one lane),
# 64, 2048 (the limit: 64 KiB of dynamic LDS); > 448 rows = > 112 partial rows for the parameter kernel's eight-loads loop; 4100 rows make a
# few waves take a second row, 9000 a third - at C = 256 / 512 in the register-resident form (its prefetch), at 768 in the generic one.
LN_CASES = [(3, 4), (453, 260), (1000, 64), (130, 2048), (4100, 256), (9000, 512), (4100, 768)]
LN_REFUSED = (5, 2052)


def ln_inputs(case):
    """Rows of standard deviation in [0.5, 2] around a mean of size [0.3, 1.3] (no constant rows: there rstd = 1 / sqrt(eps) and the comparison would
    test cancellation), gamma in [0.5, 3]."""
    n, C = case
    g = gen('ln', case)
    r = torch.randn(n, C, generator=g, dtype=torch.float64)
    r = (r - r.mean(1, keepdim=True)) / r.std(1, unbiased=False, keepdim=True)
    std = 0.5 + 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    mean = (0.3 + torch.rand(n, 1, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (n, 1), generator=g) * 2 - 1)
    return NS(u=(r * std + mean).float(), gamma=0.5 + 2.5 * torch.rand(C, generator=g), beta=torch.randn(C, generator=g) * 0.3,
              dz=torch.randn(n, C, generator=g), dgamma0=torch.randn(C, generator=g), dbeta0=torch.randn(C, generator=g))


def ln_backward(c, dtype):
    u, gamma, beta = (leaf(v, dtype) for v in (c.u, c.gamma, c.beta))
    F.gelu(F.layer_norm(u, (u.shape[1],), gamma, beta, EPS_LN)).backward(c.dz.to(dtype))
    return NS(du=u.grad, dgamma=gamma.grad, dbeta=beta.grad)


# ------------------------------------------------------------------------------------------------------------------- BiFPN
# (ups, B, C, H, W): the 2x nearest upsample folded into the fusion, in every position, twice, not at all, with two inputs.  The last case has
# 589 824 (pixel, channel quad) items: more than the 2048 x 256 the grid is capped at, and all 3 x 2048 floats of the backward's workspace.
BIFPN_CASES = [(ups, 2, 16, 10, 12) for ups in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 0, 0), (1, 0), (0, 1))] + \
              [((0, 1, 0), 2, 4, 10, 12), ((1, 0), 1, 4, 2, 2), ((1, 0, 0), 2, 256, 72, 64)]
BIFPN_W = {3: [0.3, 1.5, -0.7], 2: [1.2, -0.4]}            # raw fusion parameters, one negative


def bifpn_inputs(case):
    ups, B, C, H, W = case
    g = gen('bifpn', case)
    return NS(srcs=[torch.randn(B, C, H >> u, W >> u, generator=g) for u in ups], w=torch.tensor(BIFPN_W[len(ups)]),
              dout=torch.randn(B, C, H, W, generator=g), dw0=torch.randn(len(ups), generator=g) * 3)


def bifpn_ref(c, ups, dtype):
    """The oracle's BiFPN on the sources (nn.Upsample(2, 'nearest') in front of the flagged ones) -> out, dsrcs (NHWC), dw."""
    from oracle.somi_ref.blocks import BiFPN
    m = BiFPN(len(ups)).to(dtype)
    with torch.no_grad():
        m.weight.copy_(c.w)
    srcs = [leaf(s, dtype) for s in c.srcs]
    out = m([F.interpolate(s, scale_factor=2, mode='nearest') if u else s for s, u in zip(srcs, ups)])
    out.backward(c.dout.to(dtype))
    return NS(out=nhwc(out.detach()), dsrcs=[nhwc(s.grad) for s in srcs], dw=m.weight.grad)


# ------------------------------------------------------------------------------------------------------------------- centre-feature-scale blend
# (npix, G, Gc): one wave per pixel, lanes over a group's channels: Gc = 100 takes the lane loop twice, 6 and 16 leave lanes idle; 8200 pixels are
# more than the 2048 x 4 waves of the grid.  The logits sit in columns [0, G) of rows CFS_EXTRA wider.
CFS_CASES = [(50, 4, 16), (50, 3, 6), (50, 2, 100), (8200, 4, 16)]
CFS_EXTRA = 3


def cfs_inputs(case):
    n, G, Gc = case
    g = gen('cfs', case)
    return NS(x=torch.randn(n, G * Gc, generator=g), xproj=torch.randn(n, G * Gc, generator=g),
              logit=(torch.rand(n, G + CFS_EXTRA, generator=g) * 16 - 8), dout=torch.randn(n, G * Gc, generator=g))


def cfs_ref(c, G, Gc, dtype):
    """out = x * (1 - s) + xproj * s, s = sigmoid(logit[:, g]) over the channels of group g (modules/dcnv3.py:370-376) -> out, dx, dxproj, dlogit."""
    x, xp, lg = (leaf(v, dtype) for v in (c.x, c.xproj, c.logit))
    s = torch.sigmoid(lg[:, :G]).repeat_interleave(Gc, dim=1)
    out = x * (1 - s) + xp * s
    out.backward(c.dout.to(dtype))
    return NS(out=out.detach(), dx=x.grad, dxproj=xp.grad, dlogit=lg.grad)


# ------------------------------------------------------------------------------------------------------------------- detect decode
# (B, na, nc, ((ny, nx, stride), ...)): the levels of one case are decoded into one z at consecutive row offsets.  816 000 items are more than
# the 2048 x 256 the decoupled decode's grid is capped at, 1 224 000 more than the 4096 x 256 of the plain decode and its raw backward.
DETECT_CASES = [(2, 1, 3, ((5, 7, 8),)), (2, 3, 3, ((6, 4, 8), (3, 2, 16))), (2, 8, 3, ((5, 7, 8),)), (2, 3, 80, ((40, 40, 8),)),
                (3, 3, 80, ((40, 40, 8),))]
DETECT_PAD = NS(t=3, box=2, cls=5, rows_before=2, rows_after=3)


def detect_inputs(case):
    """Per level: t (B, ny, nx, na * no + 3), box (.., na * 5 + 2), cls (.., na * nc + 5) - the columns behind the used ones hold noise - the
    anchors in pixels (multiples of 0.5: anchors / stride * stride is exact) and a gradient of raw (B, na, ny, nx, no)."""
    B, na, nc, levels = case
    no = nc + 5
    g = gen('detect', case)
    out = []
    for ny, nx, stride in levels:
        out.append(NS(ny=ny, nx=nx, stride=float(stride), t=torch.randn(B, ny, nx, na * no + DETECT_PAD.t, generator=g) * 2,
                      box=torch.randn(B, ny, nx, na * 5 + DETECT_PAD.box, generator=g) * 2,
                      cls=torch.randn(B, ny, nx, na * nc + DETECT_PAD.cls, generator=g) * 2,
                      anchors_px=(torch.randint(8, 120, (na * 2,), generator=g).float() / 2).tolist(),
                      draw=torch.randn(B, na, ny, nx, no, generator=g)))
    return out


def _oracle_head(kind, case, lv, dtype):
    """The oracle's Detect / DecoupledDetect with the per-level convs taken out (nn.Identity): what is left is the view / permute and the decode."""
    from oracle.somi_ref import blocks as OB
    _, na, nc, _ = case
    det = (OB.Detect if kind == 'plain' else OB.DecoupledDetect)(nc, [[v / l.stride for v in l.anchors_px] for l in lv], ch=())
    det.m = nn.ModuleList(nn.Identity() for _ in lv)
    det = det.to(dtype)
    det.stride = torch.tensor([l.stride for l in lv], dtype=dtype)
    return det


def _oracle_feed(kind, case, l, dtype):
    """-> (the leaves whose gradients are the raw backward, the NCHW tensor the head's (absent) conv would have produced)."""
    B, na, nc, _ = case
    if kind == 'plain':
        t = leaf(l.t[..., :na * (nc + 5)], dtype)
        return (t,), t.permute(0, 3, 1, 2)
    box, cls = leaf(l.box[..., :na * 5], dtype), leaf(l.cls[..., :na * nc], dtype)
    b, c = box.permute(0, 3, 1, 2), cls.permute(0, 3, 1, 2)
    return (box, cls), torch.cat((b.reshape(B, na, 5, l.ny, l.nx), c.reshape(B, na, nc, l.ny, l.nx)), 2).reshape(B, -1, l.ny, l.nx)   # Decouple.forward


def detect_ref(kind, case, lv, dtype):
    """kind 'plain' (Detect on t) or 'decoupled' (DecoupledDetect on box / cls) -> raw per level, z of all levels (eval), and per level the
    gradients of the inputs under draw (training mode: raw is the output), zero-padded to the inputs' widths."""
    det = _oracle_head(kind, case, lv, dtype).eval()
    with torch.no_grad():
        z, raw = det([_oracle_feed(kind, case, l, dtype)[1] for l in lv])
    det = _oracle_head(kind, case, lv, dtype).train()
    feeds = [_oracle_feed(kind, case, l, dtype) for l in lv]
    outs = det([f[1] for f in feeds])
    sum((o * l.draw.to(dtype)).sum() for o, l in zip(outs, lv)).backward()
    pads = (DETECT_PAD.t,) if kind == 'plain' else (DETECT_PAD.box, DETECT_PAD.cls)
    grads = [tuple(F.pad(leaf.grad, (0, p)) for leaf, p in zip(f[0], pads)) for f in feeds]
    return NS(raw=list(raw), z=z, grads=grads)


def decode_plain(t, anchors_px, stride, na, nc):
    """By hand: t (B, ny, nx, >= na * no) -> raw (B, na, ny, nx, no), z rows (B, na * ny * nx, no) (models/yolo.py:84-98)."""
    B, ny, nx, _ = t.shape
    no = nc + 5
    raw = t[..., :na * no].reshape(B, ny, nx, na, no).permute(0, 3, 1, 2, 4)
    y = torch.sigmoid(raw)
    yv, xv = torch.meshgrid(torch.arange(ny, dtype=t.dtype), torch.arange(nx, dtype=t.dtype), indexing='ij')
    xy = (y[..., :2] * 2 - 0.5 + torch.stack((xv, yv), -1)) * stride
    wh = (y[..., 2:4] * 2) ** 2 * torch.tensor(anchors_px, dtype=t.dtype).view(1, na, 1, 1, 2)
    return raw.contiguous(), torch.cat((xy, wh, y[..., 4:]), -1).reshape(B, -1, no)


def decode_decoupled(box, cls, anchors_px, stride, na, nc):
    """By hand: box (.., >= na * 5), cls (.., >= na * nc) -> the same two (models/yolo.py:948-965: the cell origin carries the -0.5)."""
    B, ny, nx, _ = box.shape
    t = torch.cat((box[..., :na * 5].reshape(B, ny, nx, na, 5), cls[..., :na * nc].reshape(B, ny, nx, na, nc)), -1).reshape(B, ny, nx, -1)
    raw, _ = decode_plain(t, anchors_px, stride, na, nc)
    y = torch.sigmoid(raw)
    yv, xv = torch.meshgrid(torch.arange(ny, dtype=t.dtype), torch.arange(nx, dtype=t.dtype), indexing='ij')
    xy = (y[..., :2] * 2 + (torch.stack((xv, yv), -1) - 0.5)) * stride
    wh = (y[..., 2:4] * 2) ** 2 * torch.tensor(anchors_px, dtype=t.dtype).view(1, na, 1, 1, 2)
    return raw, torch.cat((xy, wh, y[..., 4:]), -1).reshape(B, -1, nc + 5)


Z_GROUPS = (('xy', slice(0, 2)), ('wh', slice(2, 4)), ('obj and classes', slice(4, None)))          # each held to the bar at its own scale


# ------------------------------------------------------------------------------------------------------------------- TTA resample / descale
# (B, channels, H, W, ratio, gs, flip): scale_img of the augmented forward.  96 x 128 at the three ratios with and without the flip, a non-square
# 70 x 50 (58 x 41 padded to 64 x 64) with one and three channels, three 448 x 448 images.
TTA_CASES = [(2, 3, 96, 128, r, 32, f) for r in (1.0, 0.83, 0.67) for f in (0, 1)] + \
            [(2, 3, 70, 50, 0.83, 32, 0), (2, 1, 70, 50, 0.83, 32, 1), (2, 1, 96, 128, 0.67, 32, 1), (3, 3, 448, 448, 0.67, 32, 1)]
# (B, channels, H, W, Hn, Wn): F.interpolate to a size; the last has 1 105 000 output pixels, more than the 4096 x 256 the grid is capped at
RESIZE_CASES = [(2, 3, 40, 56, 60, 84), (2, 1, 40, 56, 60, 84), (2, 3, 70, 50, 33, 77), (2, 3, 300, 400, 650, 850)]
TTA_PAD = 0.447


def image_inputs(case):
    """A noise image in [0, 1] (B, channels, H, W) and its ingested form (B, H, W, 4) with noise in the unused channels."""
    B, ch, H, W = case[:4]
    g = gen('image', case)
    img = torch.rand(B, ch, H, W, generator=g)
    x4 = torch.rand(B, H, W, 4, generator=g) + 2
    x4[..., :ch] = nhwc(img)
    return NS(img=img, x4=x4.contiguous())


def scale_img(img, ratio, gs, flip, pad=TTA_PAD):
    """By hand: utils/torch_utils.py:270-282 after the left-right flip of models/yolo.py:1260, in img's dtype."""
    x = img.flip(3) if flip else img
    if ratio == 1.0:
        return x
    h, w = x.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    x = F.interpolate(x, size=s, mode='bilinear', align_corners=False)
    hp, wp = (math.ceil(v * ratio / gs) * gs for v in (h, w))
    return F.pad(x, [0, wp - s[1], 0, hp - s[0]], value=pad)


def to_nhwc4(y, ch):
    """(B, ch, H, W) -> (B, H, W, 4), the channels behind ch zero."""
    return F.pad(nhwc(y), (0, 4 - ch))


def tta_want(c, case, dtype):
    B, ch, H, W, ratio, gs, flip = case
    y = scale_img(c.img.to(dtype), ratio, gs, flip)
    hs, ws = (H, W) if ratio == 1.0 else (int(H * ratio), int(W * ratio))
    return to_nhwc4(y, ch), (hs, ws)


def resize_want(c, case, dtype):
    return to_nhwc4(F.interpolate(c.img.to(dtype), size=case[4:6], mode='bilinear', align_corners=False), case[1])


def resample_bar(want32, want64):
    """Four times what torch's own float32 evaluation on the CPU is off by (float32 source coordinates move a sample by about size * 2^-24 pixels;
    four covers another equally valid rounding of the coordinate; a wrong neighbour or weight is off by O(1)), at least 1e-6."""
    return max(4 * rel_err(want32, want64), RESAMPLE_FLOOR)


# (B, n, no, scale, flip, img_w); the last has more rows than the 4096 x 256 the grid is capped at
DESCALE_CASES = [(2, 50, 4, 0.83, 0, 640.0), (2, 50, 85, 0.83, 1, 640.0), (2, 37, 85, 0.67, 0, 512.0), (2, 37, 4, 0.67, 1, 512.0),
                 (1, 1100000, 4, 0.67, 1, 640.0)]


def descale_inputs(case):
    B, n, no, _, _, img_w = case
    z = torch.rand(B, n, no, generator=gen('descale', case))
    z[..., :4] *= img_w
    return z


def descale_pred(p, scale, flip, img_w):
    """By hand: models/yolo.py:1292-1308 (not in place): xywh / scale, x mirrored after a left-right flip."""
    px, py, pwh = p[..., 0:1] / scale, p[..., 1:2] / scale, p[..., 2:4] / scale
    if flip:
        px = img_w - px
    return torch.cat((px, py, pwh, p[..., 4:]), -1)


# ------------------------------------------------------------------------------------------------------------------- image ingest
INGEST_CASES = [(3, 3, 448, 448), (3, 1, 448, 448)]         # 602 112 pixels: more than the 2048 x 256 the grid is capped at
