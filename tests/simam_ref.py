"""Plain-PyTorch restatement of the reference's SimAM attention family, the CPU oracle of tests/test_simam_host.py and tests/test_simam_gpu.py:
SimAM (models/common.py:2915-2939), SimAMWithSlicing (:9374-9408), SimAMWithFlexibleSlicing (:9411-9480), Conv_SWS (:9483-9495) and PSSimAM
(:2942-2961), written from their semantics:

  * the gate of a region (a set of pixels of one image and channel): with mu the mean over the region's own pixels, d = x - mu and S = sum d^2,
    every pixel is multiplied by sigmoid(d^2 / (4 (S / n + e_lambda)) + 0.5); n is GIVEN, not derived from the region's size;
  * SimAM: one region, the whole map, n = H W - 1;
  * SimAMWithSlicing: rows split at H // 2 and columns at W // 2 (on odd sizes the second region is the larger one); all four regions share
    n = (H // 2)(W // 2) - 1;
  * SimAMWithFlexibleSlicing: t x t windows starting at range(0, H - t + 1, st) x range(0, W - t + 1, st), st = t without overlap, else
    int(t (1 - overlap_ratio)); n = t t - 1.  A pixel no window covers is zero.  A pixel covered by the windows Iy x Jx gets
    sum_(i, j) gate_(i, j) / k with k = rank(i in Iy) |Jx| + rank(j in Jx) + 1: the k-th window to reach it, row-major, counts 1 / k (the reference
    divides by the coverage count at the time a window is added).  Written here in that closed form, one vectorised pass per (rank_y, rank_x);
  * Conv_SWS: act(bn(conv(att(x)))), att the window form; PSSimAM: PSA's shape around SimAM, b + SimAM(b) then b + ffn(b).
tests/golden/block_simam*.npz, generated from the reference's own classes, pin all of that.

register(monkeypatch) puts the names into the oracle's parser for the length of a test: Conv_SWS into the (c1, c2, ...) table, not repeated
inside; the four rows that pass their channels through stand in the oracle's pass as nn.Upsample rows (the same branch, c2 = ch[f]) and are
built here with their arguments as written - the three gates ignore c1, PSSimAM's row carries the scaled count."""
import copy
import sys

import torch
import torch.nn as nn

from oracle.somi_ref import blocks as OB


def gate(x, n, lam):
    """x: (..., h, w), one region per leading index."""
    d = x - x.mean((-2, -1), keepdim=True)
    d2 = d * d
    return x * torch.sigmoid(d2 / (4 * (d2.sum((-2, -1), keepdim=True) / n + lam)) + 0.5)


def quadrants(x, lam, own_n=False):
    """own_n=True is the WRONG form the host tests rule out: every region with its own N - 1."""
    H, W = x.shape[-2:]
    bh, bw = H // 2, W // 2
    out = torch.empty_like(x)
    for ys in (slice(0, bh), slice(bh, H)):
        for xs in (slice(0, bw), slice(bw, W)):
            blk = x[..., ys, xs]
            out[..., ys, xs] = gate(blk, blk.shape[-2] * blk.shape[-1] - 1 if own_n else bh * bw - 1, lam)
    return out


def window_stride(t, r):
    return t if r == 0.0 else int(t * (1 - r))


def cover(size, t, st):
    """Per coordinate of an axis: the first window over it and how many are (0: none)."""
    nwin = (size - t) // st + 1
    p = torch.arange(size)
    hi = torch.clamp(p // st, max=nwin - 1)
    lo = torch.where(p >= t, (p - t) // st + 1, torch.zeros_like(p))
    return lo, torch.clamp(hi - lo + 1, min=0), nwin


def windows(x, t, st, lam, final_count=False):
    """final_count=True is the WRONG form the host tests rule out: every contribution divided by the pixel's final coverage count."""
    B, C, H, W = x.shape
    (ylo, yn, ny), (xlo, xn, nx) = cover(H, t, st), cover(W, t, st)
    if ny < 1 or nx < 1:
        return torch.zeros_like(x)
    e = gate(x.unfold(2, t, st).unfold(3, t, st), t * t - 1, lam)                  # (B, C, ny, nx, t, t): every window's gated pixels
    hh, ww = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    out = torch.zeros_like(x)
    for ry in range(int(yn.max())):
        for rx in range(int(xn.max())):
            on = (ry < yn)[:, None] & (rx < xn)[None, :]                            # pixels that have a (ry, rx)-th window
            i, j = (ylo[:, None] + ry).expand(H, W)[on], (xlo[None, :] + rx).expand(H, W)[on]
            h, w = hh[on], ww[on]
            k = (yn[:, None] * xn[None, :])[on] if final_count else ry * xn[None, :].expand(H, W)[on] + rx + 1
            i, j, h, w, k = (v.to(x.device) for v in (i, j, h, w, k))
            out[:, :, h, w] += e[:, :, i, j, h - i * st, w - j * st] / k.to(x.dtype)
    return out


def coverage(H, W, t, st):
    """How many windows cover each pixel."""
    (_, yn, _), (_, xn, _) = cover(H, t, st), cover(W, t, st)
    return yn[:, None] * xn[None, :]


class SimAM(nn.Module):
    def __init__(self, c1, e_lambda=1e-4):
        super().__init__()
        self.e_lambda = e_lambda

    def forward(self, x):
        return gate(x, x.shape[2] * x.shape[3] - 1, self.e_lambda)


class SimAMWithSlicing(nn.Module):
    def __init__(self, c1, e_lambda=1e-4):
        super().__init__()
        self.e_lambda = e_lambda

    def forward(self, x):
        return quadrants(x, self.e_lambda)


class SimAMWithFlexibleSlicing(nn.Module):
    def __init__(self, c1, target_size, overlap_ratio=0.0, e_lambda=1e-4):
        super().__init__()
        self.target_size, self.overlap_ratio, self.e_lambda = target_size, overlap_ratio, e_lambda
        self.stride = (window_stride(target_size, overlap_ratio),) * 2

    def forward(self, x):
        return windows(x, self.target_size, self.stride[0], self.e_lambda)


class Conv_SWS(nn.Module):
    def __init__(self, c1, c2, target_size, overlap_ratio=0.0, e_lambda=1e-4, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, OB.autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())
        self.att = SimAMWithFlexibleSlicing(c1, target_size, overlap_ratio, e_lambda)

    def forward(self, x):
        return self.act(self.bn(self.conv(self.att(x))))


class PSSimAM(nn.Module):
    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = OB.Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = OB.Conv(2 * self.c, c1, 1)
        self.attn = SimAM(self.c)
        self.ffn = nn.Sequential(OB.Conv(self.c, self.c * 2, 1), OB.Conv(self.c * 2, self.c, 1, act=False))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), 1)
        b = b + self.attn(b)
        b = b + self.ffn(b)
        return self.cv2(torch.cat((a, b), 1))


# ---------------------------------------------------------------------------------------------- the analytic gradient the kernels implement
def analytic_dx(x, g, regions, n, lam, add_input=False):
    """dx of out = [x +] sum_r w_r x s_r by the closed formula (fp of x): regions = [(ys, xs, w)] with w the (h, w) weight map of the region
    (1, or 1 / k).  T = w g x s (1 - s), A = sum T d, B = sum T d^2 over the region,
    dx = [g +] sum_r ( w g s + 2 T d / D - 2 A / (N D) - (8 / n) d B / D^2 )."""
    dx = g.clone() if add_input else torch.zeros_like(x)
    for ys, xs, w in regions:
        xr, gr = x[..., ys, xs], g[..., ys, xs]
        N = xr.shape[-2] * xr.shape[-1]
        d = xr - xr.mean((-2, -1), keepdim=True)
        D = 4 * ((d * d).sum((-2, -1), keepdim=True) / n + lam)
        s = torch.sigmoid(d * d / D + 0.5)
        T = w * gr * xr * s * (1 - s)
        A, Bs = (T * d).sum((-2, -1), keepdim=True), (T * d * d).sum((-2, -1), keepdim=True)
        dx[..., ys, xs] += w * gr * s + 2 * T * d / D - 2 * A / (N * D) - (8 / n) * d * Bs / (D * D)
    return dx


def region_list(mode, H, W, t=None, st=None):
    """-> (regions of analytic_dx, n) of the three modes; the window weights (fp64) are 1 / k in the reference's visiting order."""
    one = torch.ones(1, 1, dtype=torch.float64)
    if mode == 'map':
        return [(slice(0, H), slice(0, W), one)], H * W - 1
    if mode == 'quadrants':
        bh, bw = H // 2, W // 2
        return [(ys, xs, one) for ys in (slice(0, bh), slice(bh, H)) for xs in (slice(0, bw), slice(bw, W))], bh * bw - 1
    count, regions = torch.zeros(H, W, dtype=torch.float64), []
    for i in range(0, H - t + 1, st):
        for j in range(0, W - t + 1, st):
            count[i:i + t, j:j + t] += 1
            regions.append((slice(i, i + t), slice(j, j + t), 1 / count[i:i + t, j:j + t].clone()))
    return regions, t * t - 1


# ---------------------------------------------------------------------------------------------- the parser tables
_ROWS = {'SimAM': SimAM, 'SimAMWithSlicing': SimAMWithSlicing, 'SimAMWithFlexibleSlicing': SimAMWithFlexibleSlicing, 'PSSimAM': PSSimAM}


def register(monkeypatch):
    """The five names in the oracle's parse_model (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, Conv_SWS=Conv_SWS))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) - {'Conv_SWS'})
    inner = OM.parse_model

    def parse_model(d, ch):
        rows = d['backbone'] + d['head']
        swapped = dict(d, backbone=[], head=[[f, n, 'nn.Upsample', [None, 1, 'nearest']] if name in _ROWS else [f, n, name, args]
                                             for f, n, name, args in rows])
        seq, save = inner(swapped, ch)
        layers = list(seq)
        for i, (f, n, name, args) in enumerate(rows):
            if name in _ROWS:
                m_ = _ROWS[name](*args)
                m_.i, m_.f, m_.type = i, f, name
                m_.np = sum(p.numel() for p in m_.parameters())
                layers[i] = m_
        return nn.Sequential(*layers), save
    monkeypatch.setattr(OM, 'parse_model', parse_model)


# ---------------------------------------------------------------------------------------------- the cases
# Nothing in the family has a kink or a discrete choice: the gate is a sigmoid of a smooth function of the input, the blocks add SiLU and
# BatchNorm only - no max pool, no h-swish, no arg-max.  Two correct fp32 implementations cannot fall on different sides of anything, so the
# seeds below are the first ones (parity.check_block's default rule, fill 1 / batch 0) and need no selection.
BLOCKS = {                        # tag -> (constructor over a namespace, NCHW input shape); the first six are the fixtures' blocks and shapes
    'simam': (lambda ns: ns.SimAM(16), (2, 16, 5, 7)),
    'simam_slicing': (lambda ns: ns.SimAMWithSlicing(16), (2, 16, 7, 5)),
    'simam_windows': (lambda ns: ns.SimAMWithFlexibleSlicing(16, 4, 0.0), (2, 16, 11, 13)),
    'simam_windows_overlap': (lambda ns: ns.SimAMWithFlexibleSlicing(16, 4, 0.5), (2, 16, 11, 13)),
    'simam_conv_sws': (lambda ns: ns.Conv_SWS(16, 32, 4, 0.5, 1e-4, 3, 2), (2, 16, 11, 13)),
    'simam_pssimam': (lambda ns: ns.PSSimAM(32, 32), (2, 32, 5, 7)),
    'simam_conv_sws_r0': (lambda ns: ns.Conv_SWS(16, 32, 4, 0.0, 1e-4, 3, 2), (2, 16, 11, 13)),
}
FIXTURES = [t for t in BLOCKS if t != 'simam_conv_sws_r0']       # tests/golden/block_<tag>.npz
WHERE = ('row', 'slicing', 'sws', 'ps')
# 'slicing' at 64 x 64 would put the row on a 2 x 2 map: quadrants of ONE pixel, which the reference turns into 0 / 0 and the blocks refuse by
# name.  128 x 128 gives it a 4 x 4 map, quadrants of 2 x 2.  The other three run at 64 x 64.
GRAPH_SIZE = {'row': 64, 'slicing': 128, 'sws': 64, 'ps': 64}


def block_case(tag):
    """-> (the filled oracle block, the input, the generator for the output gradient) of a block test, exactly as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    make, shape = BLOCKS[tag]
    ref = make(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    gen = torch.Generator().manual_seed(len(tag))
    return ref, torch.randn(*shape, generator=gen), gen


def oracle_model(cfg):
    """The oracle Model of a yolov5_simam_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


def graph_case(where):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_simam_cfg at width 0.25, nc 10, batch 2, GRAPH_SIZE[where]."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_simam_cfg
    cfg = yolov5_simam_cfg(0.25, 0.33, nc=10, where=where)
    ref = fill_state(oracle_model(cfg), 1)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, GRAPH_SIZE[where], nc=10, seed=0)
    return cfg, ref, imgs, targets
