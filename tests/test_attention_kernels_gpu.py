"""The global pools and the CBAM / SEAM attention kernels (csrc/layers.hip, csrc/train_blocks.hip, the pooled and CBAM entries of
csrc/train_ops.hip), kernel by kernel, against tests/attention_ref.py in fp64 at the sizes where their thread mappings change: chunked two-stage
reductions, channel quads that do not fill a workgroup, lanes per pixel, image-aligned sweeps at their grid cap, and the two arg-max tie rules.
Inputs and outputs live in channel slices of wider tensors wherever the entry point takes one; every sequence runs twice and must repeat bit
for bit.  Bars: 1e-5 point-wise and pooled values, 2e-5 the k x k weight gradient, 1e-4 per-channel sums over pixels, exact maxima and indices."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import attention_ref as R
from parity import rel_close

pytestmark = pytest.mark.gpu

# (B, H, W, C): each class exists for one mapping edge
SHAPES = [
    (1, 1, 1, 4),          # one pixel, one channel quad, a map smaller than every k
    (2, 1, 7, 12),         # C/4 = 3 does not divide 256: idle rows in stage 1, an idle fourth lane per pixel; affine_silu_pool does not cover it
    (2, 16, 16, 32),       # exactly one full 256-pixel chunk per image
    (3, 1, 257, 64),       # the second chunk holds one pixel; W larger than a chunk
    (2, 37, 29, 256),      # 5 chunks with a ragged tail; C/4 = 64: a whole wave per pixel
    (8, 37, 29, 256),      # the image-aligned grids at their per-batch cap (5*256/B, 7*256/B, 4*256/B workgroups per image)
    (1, 129, 129, 8),      # 66 chunks per image: stage 2 (global_pool_stage2, img_partial_sum_kernel) takes its second 64-chunk trip
    (16, 37, 37, 256),     # capped grids with more than three pixel steps per thread: the four-deep pixel loop of the image-aligned sweeps, then its tail
    #                        (at B = 8 above a thread's step is 640 / 896 / 512 pixels of 1073: the cap is hit, the four-deep loop is not entered)
    (1, 5, 7, 1028),       # C/4 = 257: a second channel pass with one quad; attn_mlp_backward refuses it (C > 1024); affine_silu_pool does not cover it
    (1, 3, 11, 2048),      # C/4 = 512: the multiple-of-256 branch of affine_silu_pool, two workgroups per row; forward kernels and pool_backward_add_ only
]
DEEP = SHAPES[7]
EVERY = SHAPES                                     # forward kernels that pool, pool_backward_add_
FORWARD = SHAPES[:7] + SHAPES[8:]                  # forward kernels without an image-aligned sweep
BACKWARD = SHAPES[:7] + SHAPES[8:9]                # steps A - F one by one
POOLED = SHAPES[:9]                                # the pooled BatchNorm backward
FUSED = SHAPES[:8]                                 # step C inside the BatchNorm backward: C <= 1024 (the MLP backward is part of the sequence)
MID, K, EPS = 4, 7, 1e-3


def shapes(which):
    return pytest.mark.parametrize('shape', which, ids=['x'.join(map(str, s)) for s in which], scope='module')


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def planted_pixels(HW):
    """Where the 'planted' kind writes channel 0's maximum (the first one must win) - 255, 256 and HW - 1: the last pixel of the first chunk, the
    first of the second, the last of the map; a smaller map takes its middle and its last pixel."""
    if HW > 256:
        return [255, 256, HW - 1]
    return sorted({HW // 2, HW - 1})


def draw(shape, kind, g):
    """rand: N(0,1) plus a per-channel offset in [-2, 2] (means O(1)); neg: every value below -1 (a reduction identity of 0 instead of -inf
    shows); ties: round(clamp(randn, -1.5, 1.5)); planted: rand with channel 0's maximum written at planted_pixels and channel 1's at HW - 1."""
    B, H, W, C = shape
    x = torch.randn(B, H, W, C, generator=g)
    off = torch.rand(C, generator=g) * 4 - 2
    if kind == 'ties':
        return torch.round(torch.clamp(x, -1.5, 1.5))
    if kind == 'neg':
        return -1.0625 - 3 * torch.rand(B, H, W, C, generator=g) - off.abs()
    x = x + off
    if kind == 'planted':
        flat = x.view(B, H * W, C)
        top = float(x.max()) + 1.0
        flat[:, planted_pixels(H * W), 0] = top
        flat[:, H * W - 1, 1] = top + 0.5
    return x


def mlp_params(g, C, mid):
    return (torch.randn(mid, C, generator=g) * (0.5 / C ** 0.5), torch.randn(mid, generator=g) * 0.1, torch.randn(C, mid, generator=g) * 0.3,
            torch.randn(C, generator=g) * 0.1)


@functools.lru_cache(maxsize=4)
def tensor(shape, kind):
    """One input tensor of a size class and kind, drawn once."""
    return draw(shape, kind, torch.Generator().manual_seed(sum(shape) * 13 + len(kind)))


@functools.lru_cache(maxsize=4)
def case(shape, kind, k=K):
    """The fp32 inputs of one CBAM (t, dt2, the MLP, the k x k conv) and attention_ref.cbam_grads of them in fp64, computed once and shared."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape) * 31 + len(kind) + k)
    c = types.SimpleNamespace(shape=shape, kind=kind, k=k, t=tensor(shape, kind), dt2=torch.randn(B, H, W, C, generator=g))
    c.W1, c.b1, c.W2, c.b2 = mlp_params(g, C, MID)
    if kind == 'ties':                                           # a constant ca: the channel ties survive the product
        c.W2, c.b2 = torch.zeros(C, MID), torch.full((C,), 0.25)
    c.w, c.b = torch.randn(k, k, 2, generator=g) * 0.2, torch.randn(1, generator=g) * 0.1
    c.ref = R.cbam_grads(c.t, c.dt2, c.W1, c.b1, c.W2, c.b2, c.w, c.b, k)
    return c


@functools.lru_cache(maxsize=2)
def fused_case(shape, k=K):
    """y, gamma, beta in front of a CBAM and attention_ref.bn_silu_cbam_grads of them."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape) * 17 + k)
    c = types.SimpleNamespace(shape=shape, k=k, y=draw(shape, 'rand', g) * 0.7, gamma=torch.rand(C, generator=g) + 0.5,
                              beta=torch.randn(C, generator=g) * 0.3, dt2=torch.randn(B, H, W, C, generator=g))
    c.W1, c.b1, c.W2, c.b2 = mlp_params(g, C, MID)
    c.w, c.b = torch.randn(k, k, 2, generator=g) * 0.2, torch.randn(1, generator=g) * 0.1
    c.ref = R.bn_silu_cbam_grads(c.y, c.gamma, c.beta, EPS, c.dt2, c.W1, c.b1, c.W2, c.b2, c.w, c.b, k)
    c.stats = [v.float() for v in R.batchnorm_stats(c.y, c.gamma, c.beta, EPS)]              # mean, rstd, scale, shift
    return c


def widen(x, coff, after, seed=1):
    """x in channels [coff, coff + C) of a wider tensor of noise."""
    B, H, W, C = x.shape
    wide = torch.randn(B, H, W, coff + C + after, generator=torch.Generator().manual_seed(seed))
    wide[..., coff:coff + C] = x
    return wide


def outside_untouched(got, wide, coff, C, what):
    got = got.cpu()
    assert torch.equal(got[..., :coff], wide[..., :coff]) and torch.equal(got[..., coff + C:], wide[..., coff + C:]), \
        f'{what}: channels outside the slice changed'


def twice(fn):
    """fn() twice from equal inputs: every output tensor bit-identical; -> the first run's outputs."""
    a = fn()
    torch.cuda.synchronize()
    b = fn()
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert (p is None and q is None) or torch.equal(p, q), f'output {i} differs between two runs from equal inputs'
    return a


def accumulated(buf, buf0):
    """What a kernel added to a buffer that started at buf0."""
    return buf.cpu().double() - buf0.double()


def like_scaled(ref, seed):
    """A non-zero start for an accumulated gradient, of the gradient's own size (so that fp32 accumulation does not decide the comparison)."""
    ref = R.f64(ref)
    return (torch.randn(ref.shape, generator=torch.Generator().manual_seed(seed)) * float(ref.abs().max() + 1e-6)).float()


# ------------------------------------------------------------------------------------------------------------------- 1, 2, 3: the pools
@shapes(FORWARD)
@pytest.mark.parametrize('kind', ['rand', 'neg', 'ties'])
def test_global_pool(shape, kind):
    from somi_amd import ops
    d = dev()
    C = shape[3]
    t = tensor(shape, kind)
    want_avg, want_max = R.global_pools(t)
    wd = widen(t, 8, 4).to(d)
    avg, mx = twice(lambda: ops.global_pool(wd, c=C, x_coff=8))
    rel_close(avg, want_avg, rel=1e-5, what=f'global_pool avg {kind}')
    assert torch.equal(mx.cpu().double(), want_max), f'global_pool max {kind}'
    avg2, none = twice(lambda: ops.global_pool(wd, c=C, x_coff=8, want_max=False))
    assert none is None and torch.equal(avg2, avg), 'global_pool(want_max=False)'


@shapes(FORWARD)
def test_global_pool_act(shape):
    from somi_amd import ops
    d = dev()
    C = shape[3]
    c = types.SimpleNamespace(t=tensor(shape, 'rand'))
    g = torch.Generator().manual_seed(C)
    ps, pt = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    wd = widen(c.t, 4, 8).to(d)
    for act in ('none', 'silu', 'gelu', 'relu', 'sigmoid'):
        want = R.ACTS[act](c.t.double()).mean(dim=(1, 2))
        got, = twice(lambda: (ops.global_pool_act(wd, act, c=C, x_coff=4),))
        rel_close(got, want, rel=1e-5, what=f'global_pool_act {act}')
        psd, ptd = ps.to(d), pt.to(d)
        got, = twice(lambda: (ops.global_pool_act(wd, act, psd, ptd, c=C, x_coff=4),))
        rel_close(got, want * ps.double() + pt.double(), rel=1e-5, what=f'global_pool_act {act} + post scale / shift')


@shapes(EVERY)
def test_affine_silu_pool(shape):
    from somi_amd import _lib, ops
    d = dev()
    B, H, W, C = shape
    c = types.SimpleNamespace(t=tensor(shape, 'rand'))
    g = torch.Generator().manual_seed(C + 1)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(d), (torch.randn(C, generator=g) * 0.3).to(d)
    xw, ow = widen(c.t, 4, 4).to(d), widen(torch.zeros(shape), 8, 4, seed=2)
    covered = (256 % (C // 4) == 0) or ((C // 4) % 256 == 0)
    rows = _lib.lib().somi_affine_silu_pool_rows(B, H * W, C)
    if not covered:
        assert rows == 0, f'somi_affine_silu_pool_rows: {rows} for C / 4 = {C // 4}'
        assert ops.affine_silu_pool(xw, C, 4, sc, sh, ow.to(d), 8) is None
        return
    assert rows > 0

    def run():
        out = ow.to(d)
        avg, mx = ops.affine_silu_pool(xw, C, 4, sc, sh, out, 8)
        return out, avg, mx
    out, avg, mx = twice(run)
    plain = ops.chan_affine_act(xw, C, 4, sc, sh, 'silu', 0, ow.to(d), 8)
    assert torch.equal(out, plain), 'z differs from chan_affine_act(silu, order 0)'
    outside_untouched(out, ow, 8, C, 'affine_silu_pool z')
    assert torch.equal(mx, ops.global_pool(out, c=C, x_coff=8)[1]), 'max differs from global_pool of z'
    u = c.t.double() * sc.cpu().double() + sh.cpu().double()
    rel_close(avg, (u * torch.sigmoid(u)).mean(dim=(1, 2)), rel=1e-5, what='affine_silu_pool avg')


# ------------------------------------------------------------------------------------------------------------------- 4: the MLPs
@shapes(FORWARD)
def test_attn_mlp(shape):
    from somi_amd import ops
    d = dev()
    C = shape[3]
    avg, mx = (v.float() for v in R.global_pools(tensor(shape, 'rand')))
    for mid in (1, 3, 4, 64):                                    # fewer and more hidden units than the workgroup's four waves
        W1, b1, W2, b2 = mlp_params(torch.Generator().manual_seed(C + mid), C, mid)
        dv = [v.to(d) for v in (avg, mx, W1, b1, W2, b2)]
        got, = twice(lambda: (ops.attn_mlp(0, *dv),))
        rel_close(got, R.channel_attention(avg.double(), mx.double(), W1.double(), b1.double(), W2.double(), b2.double()), rel=1e-5,
                  what=f'attn_mlp mode 0 mid {mid}')
        got, = twice(lambda: (ops.attn_mlp(0, dv[0], dv[1], dv[2], None, dv[4], None),))
        rel_close(got, R.channel_attention(avg.double(), mx.double(), W1.double(), None, W2.double(), None), rel=1e-5,
                  what=f'attn_mlp mode 0 without biases mid {mid}')
        got, = twice(lambda: (ops.attn_mlp(1, dv[0], None, dv[2], None, dv[4], None),))
        rel_close(got, R.seam_scale(avg.double(), W1.double(), W2.double()), rel=1e-5, what=f'attn_mlp mode 1 mid {mid}')


# ------------------------------------------------------------------------------------------------------------------- 5, 6, 7: the spatial branch
@shapes(FORWARD)
@pytest.mark.parametrize('kind', ['rand', 'neg', 'ties'])
def test_chan_stats(shape, kind):
    from somi_amd import ops
    d = dev()
    C = shape[3]
    c = case(shape, kind)
    ca = c.ref['ca'].float()
    wd = widen(c.t, 8, 8).to(d)
    cad = ca.to(d)
    stats, = twice(lambda: (ops.chan_stats(wd, cad, c=C, x_coff=8),))
    want = R.spatial_stats(c.t.double() * ca.double()[:, None, None, :])
    rel_close(stats[..., 0], want[..., 0], rel=1e-5, what=f'chan_stats mean {kind}')
    assert torch.equal(stats[..., 1].cpu(), (c.t * ca[:, None, None, :]).amax(dim=3)), f'chan_stats max {kind}: not the maximum of the fp32 products'
    rel_close(stats[..., 1], want[..., 1], rel=1e-5, what=f'chan_stats max {kind}')


@shapes(FORWARD)
@pytest.mark.parametrize('k', [3, 5, 7])
def test_spatial_attn_and_cbam_apply(shape, k):
    from somi_amd import ops
    d = dev()
    C = shape[3]
    c = case(shape, 'rand')
    g = torch.Generator().manual_seed(C + k)
    w, b = torch.randn(k, k, 2, generator=g) * 0.2, torch.randn(1, generator=g) * 0.1
    ca, stats = c.ref['ca'].float(), c.ref['stats'].float()
    want_sa = R.spatial_attention(stats.double(), w.double(), b.double(), k)
    cad, std, wdv, bd = ca.to(d), stats.to(d), w.to(d), b.to(d)
    sa, = twice(lambda: (ops.spatial_attn(std, wdv, bd, k),))
    rel_close(sa, want_sa, rel=1e-5, what=f'spatial_attn k {k}')
    wide = widen(c.t, 8, 4)

    def run():
        x = wide.to(d)
        return (ops.cbam_apply_(x, cad, std, wdv, bd, k, c=C, x_coff=8),)
    got, = twice(run)
    rel_close(got[..., 8:8 + C], c.t.double() * ca.double()[:, None, None, :] * want_sa[..., None], rel=1e-5, what=f'cbam_apply_ k {k}')
    outside_untouched(got, wide, 8, C, 'cbam_apply_')


@shapes(FORWARD)
def test_scale_channels(shape):
    from somi_amd import ops
    d = dev()
    c = case(shape, 'rand')
    s, pix = c.ref['ca'].float(), c.ref['sa'].float()
    xd, sd, pd = c.t.to(d), s.to(d), pix.to(d)
    x64 = c.t.double()
    for what, a, b, want in (('s', sd, None, x64 * s.double()[:, None, None, :]), ('pix', None, pd, x64 * pix.double()[..., None]),
                             ('s and pix', sd, pd, x64 * s.double()[:, None, None, :] * pix.double()[..., None])):
        got, = twice(lambda: (ops.scale_channels(xd, a, b),))
        rel_close(got, want, rel=1e-5, what=f'scale_channels with {what}')


# ------------------------------------------------------------------------------------------------------------------- 8: steps A - D
def steps_abc(dt2w, d_coff, tw, t_coff, C, ca, sa, stats, w, k, dw, db, t_max):
    """Steps A - C entry by entry (ops.cbam_backward keeps dlogit, amaxc and dstats to itself and fixes the gradient's channel offset at 0)."""
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream, check
    L, d = _lib.lib(), tw.device
    B, H, W, _ = tw.shape
    dlogit = torch.empty(B, H, W, device=d)
    amaxc = torch.empty(B, H, W, device=d, dtype=torch.int32)
    amaxp = torch.empty(B, C, device=d, dtype=torch.int32)
    check(L.somi_cbam_bwd_pixel_argmax_f32(_ptr(dt2w), dt2w.shape[3], d_coff, _ptr(tw), tw.shape[3], t_coff, _ptr(ca), _ptr(sa), _ptr(t_max),
                                           _ptr(dlogit), _ptr(amaxc), _ptr(amaxp), B, H * W, C, _stream()), 'cbam_bwd_pixel')
    dstats = torch.empty(B, H, W, 2, device=d)
    ws = torch.empty(((B * H * W + 511) // 512) * (2 * k * k + 1), device=d)
    check(L.somi_spatial_attn_bwd_f32(_ptr(dlogit), _ptr(stats), _ptr(w), _ptr(dstats), _ptr(dw), _ptr(db), _ptr(ws), B, H, W, k, 0, _stream()),
          'spatial_attn_bwd')
    dca = torch.empty(B, C, device=d)
    ws2 = torch.empty(B * L.somi_img_nchunk(H * W) * C, device=d)
    check(L.somi_cbam_bwd_chan_f32(_ptr(dt2w), dt2w.shape[3], d_coff, _ptr(tw), tw.shape[3], t_coff, _ptr(ca), _ptr(sa), _ptr(dstats), _ptr(amaxc),
                                   _ptr(dca), _ptr(ws2), B, H * W, C, _stream()), 'cbam_bwd_chan')
    return dlogit, amaxc, amaxp, dstats, dca


@shapes(BACKWARD)
@pytest.mark.parametrize('kind', ['rand', 'neg', 'ties', 'planted'])
def test_cbam_backward_steps_a_to_d(shape, kind):
    from somi_amd import ops
    d = dev()
    B, H, W, C = shape
    c = case(shape, kind)
    r = c.ref
    ca, sa, stats, wk = (v.float().to(d) for v in (r['ca'], r['sa'], r['stats'], c.w))
    tw = widen(c.t, 8, 4).to(d)
    _, t_max = ops.global_pool(tw, c=C, x_coff=8)
    dw0, db0 = like_scaled(r['dw'], 3), like_scaled(r['db'], 4)
    for d_coff, after, direct in ((4, 8, True), (0, 4, False)):
        wide = widen(c.dt2, d_coff, after, seed=5)

        def run():
            dt2w, dw, db = wide.to(d), dw0.to(d), db0.to(d)
            if direct:
                return (dt2w, dw, db) + steps_abc(dt2w, d_coff, tw, 8, C, ca, sa, stats, wk, c.k, dw, db, t_max)
            dca, amaxp = ops.cbam_backward(dt2w, tw, 8, C, ca, sa, stats, wk, c.k, dw, db, t_max)
            return dt2w, dw, db, None, None, amaxp, None, dca
        dt, dw, db, dlogit, amaxc, amaxp, dstats, dca = twice(run)
        tag = f'{kind} ' + ('entry by entry' if direct else 'ops.cbam_backward')
        assert torch.equal(amaxp.cpu(), r['amaxp']), f'{tag}: amaxp is not the first pixel of every channel\'s maximum'
        if kind == 'planted':
            assert (amaxp[:, 0].cpu() == planted_pixels(H * W)[0]).all() and (amaxp[:, 1].cpu() == H * W - 1).all(), f'{tag}: planted amaxp'
        if direct:
            assert torch.equal(amaxc.cpu(), r['amaxc']), f'{tag}: amaxc is not the lowest channel that holds the pixel\'s maximum'
            rel_close(dlogit, r['dlogit'], rel=1e-5, what=f'{tag} dlogit')
            rel_close(dstats, r['dstats'], rel=1e-5, what=f'{tag} dstats')
        rel_close(accumulated(dw, dw0), r['dw'], rel=2e-5, what=f'{tag} dw')
        rel_close(accumulated(db, db0), r['db'], rel=2e-5, what=f'{tag} db')
        rel_close(dt[..., d_coff:d_coff + C], r['dt_c'], rel=1e-5, what=f'{tag} dt after step C')
        outside_untouched(dt, wide, d_coff, C, f'{tag} dt')
        rel_close(dca, r['dca'], rel=1e-4, what=f'{tag} dca')


# ------------------------------------------------------------------------------------------------------------------- 9: step E
@shapes(BACKWARD)
def test_attn_mlp_backward(shape):
    from somi_amd import ops
    d = dev()
    B, _, _, C = shape
    c = case(shape, 'rand')
    avg, mx = c.ref['avg'].float(), c.ref['max'].float()
    g = torch.Generator().manual_seed(C + 7)
    dout = torch.randn(B, C, generator=g)
    for mode in (0, 1):
        for mid in (1, 3, 4, 64):
            W1, b1, W2, b2 = mlp_params(torch.Generator().manual_seed(C + mid + mode), C, mid)
            if mode == 1:
                b1 = b2 = None
            want = R.attn_mlp_grads(mode, avg, mx if mode == 0 else None, W1, b1, W2, b2, dout)
            out = want['out'].float()
            starts = [None if want[n] is None else like_scaled(want[n], i) for i, n in enumerate(('dW1', 'db1', 'dW2', 'db2'))]
            dv = [None if v is None else v.to(d) for v in (dout, out, avg, mx if mode == 0 else None, W1, b1, W2)]

            def run():
                bufs = [None if s is None else s.to(d) for s in starts]
                return tuple(ops.attn_mlp_backward(mode, *dv, *bufs)) + tuple(bufs)
            if C > 1024:
                with pytest.raises(RuntimeError, match=r'attn mlp bwd: bad arguments \(C <= 1024'):
                    run()
                continue
            davg, dmax, *bufs = twice(run)
            tag = f'attn_mlp_backward mode {mode} mid {mid}'
            rel_close(davg, want['davg'], rel=1e-5, what=f'{tag} davg')
            if mode == 0:
                rel_close(dmax, want['dmax'], rel=1e-5, what=f'{tag} dmax')
            else:
                assert dmax is None
            for n, buf, s in zip(('dW1', 'db1', 'dW2', 'db2'), bufs, starts):
                if s is not None:
                    rel_close(accumulated(buf, s), want[n], rel=1e-4, what=f'{tag} {n}')


# ------------------------------------------------------------------------------------------------------------------- 10: step F
@shapes(EVERY)
@pytest.mark.parametrize('kind', ['rand', 'planted'])
def test_pool_backward_add(shape, kind):
    from somi_amd import ops
    d = dev()
    B, H, W, C = shape
    amaxp = R.argmax_pixels(tensor(shape, kind))
    g = torch.Generator().manual_seed(C + 11)
    c = types.SimpleNamespace(dt2=torch.randn(B, H, W, C, generator=g))
    davg, dmax = torch.randn(B, C, generator=g) * (H * W) ** 0.5, torch.randn(B, C, generator=g)
    wide = widen(c.dt2, 4, 8, seed=6)
    onehot = F.one_hot(amaxp.long(), H * W).permute(0, 2, 1).reshape(B, H, W, C).double()
    dad, dmd, apd = davg.to(d), dmax.to(d), amaxp.to(d)
    got, = twice(lambda: (ops.pool_backward_add_(wide.to(d), 4, C, dad, dmd, apd),))
    rel_close(got[..., 4:4 + C], c.dt2.double() + davg.double()[:, None, None, :] / (H * W) + onehot * dmax.double()[:, None, None, :], rel=1e-5,
              what=f'pool_backward_add_ {kind}')
    outside_untouched(got, wide, 4, C, 'pool_backward_add_')
    got, = twice(lambda: (ops.pool_backward_add_(wide.to(d), 4, C, dad),))
    rel_close(got[..., 4:4 + C], c.dt2.double() + davg.double()[:, None, None, :] / (H * W), rel=1e-5, what=f'pool_backward_add_ {kind}, average only')
    # dmax alone onto zeros: exactly one pixel of every (image, channel) receives it, the arg-max
    zeros, ones = torch.zeros(B, H, W, C, device=d), torch.ones(B, C, device=d)
    got = ops.pool_backward_add_(zeros, 0, C, torch.zeros(B, C, device=d), ones, apd).cpu()
    assert torch.equal(got.double(), onehot), 'dmax reached another pixel than amaxp, or more than one'
    if kind == 'planted':
        assert (got.view(B, H * W, C)[:, planted_pixels(H * W)[0], 0] == 1).all() and (got.view(B, H * W, C)[:, :, 0].sum(1) == 1).all()


# ------------------------------------------------------------------------------------------------------------------- 11: SEAM's tail
@shapes(BACKWARD)
def test_scale_channels_backward(shape):
    from somi_amd import ops
    d = dev()
    C = shape[3]
    c = case(shape, 'rand')
    W1, _, W2, _ = mlp_params(torch.Generator().manual_seed(C + 13), C, MID)
    u = c.dt2 + 0.5                                                # the tensor SEAM pools: any tensor of the shape
    r = R.seam_tail_grads(c.t, u, c.dt2, W1, W2)
    sc = r['sc'].float()
    dod, xd, sd = c.dt2.to(d), c.t.to(d), sc.to(d)
    dx, ds = twice(lambda: ops.scale_channels_backward(dod, xd, sd))
    rel_close(dx, c.dt2.double() * sc.double()[:, None, None, :], rel=1e-5, what='scale_channels_backward dx')
    rel_close(ds, r['dsc'], rel=1e-4, what='scale_channels_backward ds')
    if C <= 1024:                                                  # the rest of the tail: MLP mode 1 backward, then the average-only pool backward
        gW1, gW2 = like_scaled(r['dW1'], 1), like_scaled(r['dW2'], 2)
        b1, b2 = gW1.to(d), gW2.to(d)
        davg, none = ops.attn_mlp_backward(1, ds, sd, r['avg'].float().to(d), None, W1.to(d), None, W2.to(d), b1, None, b2, None)
        assert none is None
        rel_close(davg, r['davg'], rel=1e-5, what='SEAM davg')
        rel_close(accumulated(b1, gW1), r['dW1'], rel=1e-4, what='SEAM dW1')
        rel_close(accumulated(b2, gW2), r['dW2'], rel=1e-4, what='SEAM dW2')
        du = ops.pool_backward_add_(torch.zeros(shape, device=d), 0, C, davg)
        rel_close(du, r['du'], rel=1e-5, what='SEAM du = davg / HW')


# ------------------------------------------------------------------------------------------------------------------- 12: step C inside the BatchNorm backward
@shapes(FUSED)
def test_cbam_step_c_in_the_batchnorm_backward(shape):
    from somi_amd import ops
    d = dev()
    B, H, W, C = shape
    c = fused_case(shape)
    r = c.ref
    mean, rstd, scale, shift = (v.to(d) for v in c.stats)
    ca, sa, stats, wk = (v.float().to(d) for v in (r['ca'], r['sa'], r['stats'], c.w))
    avg, mx = r['avg'].float().to(d), r['max'].float().to(d)
    mlp = [v.to(d) for v in (c.W1, c.b1, c.W2, c.b2)]
    yw = widen(c.y, 0, 4, seed=7).to(d)
    # t and its spatial maximum as the forward pass leaves them: the fused pass where it covers the width, else the two separate ones
    t = torch.empty(B, H, W, C, device=d)
    pooled = ops.affine_silu_pool(yw, C, 0, scale, shift, t, 0)
    if pooled is None:
        ops.chan_affine_act(yw, C, 0, scale, shift, 'silu', 0, t, 0)
    t_max_pool = ops.global_pool(t)[1]
    rel_close(t, r['t'], rel=1e-5, what='t')
    starts = {n: like_scaled(r[n], i) for i, n in enumerate(('dw', 'db', 'dW1', 'db1', 'dW2', 'db2', 'dgamma', 'dbeta'))}
    wide = widen(c.dt2, 0, 8, seed=8)

    def run(t_max):
        buf = {n: s.to(d) for n, s in starts.items()}
        dt2w = wide.to(d)
        dca, amaxp, state = ops.cbam_backward(dt2w, t, 0, C, ca, sa, stats, wk, c.k, buf['dw'], buf['db'], t_max, bn=(yw, scale, shift, mean))
        davg, dmax = ops.attn_mlp_backward(0, dca, ca, avg, mx, *mlp[:3], buf['dW1'], buf['db1'], buf['dW2'], buf['db2'])
        dy = ops.cbam_bn_backward_apply(state, rstd, davg, dmax, torch.full((B, H, W, C), 9.0, device=d), buf['dgamma'], buf['dbeta'])
        return (dy, dca, amaxp, davg, dmax, dt2w) + tuple(buf[n] for n in starts)
    dy, dca, amaxp, davg, dmax, dt2w, *bufs = twice(lambda: run(t_max_pool))
    assert torch.equal(amaxp.cpu(), R.argmax_pixels(t.cpu())), 'amaxp is not the first pixel of every channel\'s maximum of t'
    if pooled is not None:
        assert torch.equal(pooled[1], t_max_pool), 'affine_silu_pool max differs from global_pool of z'
        assert torch.equal(run(pooled[1])[2], amaxp), 'amaxp from affine_silu_pool\'s maximum differs from global_pool\'s'
    assert torch.equal(dt2w.cpu(), wide), 'the fused form must leave dt2 alone'
    # one pixel in the batch: dy is analytically 0 (every term of the BatchNorm backward cancels), and the reduction and the apply kernel add the
    # pooled terms in different orders - the bar is then 1e-5 of the cancelling terms' size, max |scale * dt * silu'(u)|, from the fp64 reference
    atol = 0.0
    if B * H * W == 1:
        u = c.y.double() * c.stats[2].double() + c.stats[3].double()
        sg = torch.sigmoid(u)
        atol = 1e-5 * float((c.stats[2].double() * r['dt'] * sg * (1 + u * (1 - sg))).abs().max())
    rel_close(dy, r['dy'], rel=1e-5, atol=atol, what='fused dy')
    rel_close(dca, r['dca'], rel=1e-4, what='fused dca')
    rel_close(davg, r['davg'], rel=1e-4, what='fused davg (of dca)')
    rel_close(dmax, r['dmax'], rel=1e-4, what='fused dmax (of dca)')
    for (n, s), buf in zip(starts.items(), bufs):
        rel_close(accumulated(buf, s), r[n], rel=2e-5 if n in ('dw', 'db') else 1e-4, what=f'fused {n}')


# ------------------------------------------------------------------------------------------------------------------- 13: the pooled BatchNorm backward
@shapes(POOLED)
@pytest.mark.parametrize('act,order', [('silu', 0), ('gelu', 1)])
def test_bn_act_backward_pooled(shape, act, order):
    from somi_amd import ops
    d = dev()
    B, H, W, C = shape
    HW = H * W
    g = torch.Generator().manual_seed(sum(shape) + order)
    x = draw(shape, 'rand', g) * 0.7
    dz = torch.randn(B, H, W, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    davg, dmax = torch.randn(B, C, generator=g) * HW ** 0.5, torch.randn(B, C, generator=g)
    amaxp = torch.randint(0, HW, (B, C), generator=g, dtype=torch.int32)
    for j, p in enumerate((min(255, HW - 1), min(256, HW - 1), HW - 1, 0)):       # chunk edges, the last pixel, the first
        amaxp[:, j] = p
    xw, dzw, dxw = widen(x, 8, 4, seed=9).to(d), widen(dz, 4, 4, seed=10), widen(torch.zeros(shape), 4, 8, seed=11)
    dad, dmd, apd = davg.to(d), dmax.to(d), amaxp.to(d)
    # the statistics from their producer in the training pass (of act(x) when the activation comes first), held to fp64 here
    mean, rstd, scale, shift = ops.bn_stats(xw, C, 8, gamma.to(d), beta.to(d), EPS, 0.03, act=act if order == 1 else 'none')
    for got, want, name in zip((mean, rstd, scale, shift), R.batchnorm_stats(x.double() if order == 0 else R.ACTS[act](x.double()), gamma, beta, EPS),
                               ('mean', 'rstd', 'scale', 'shift')):
        rel_close(got, want, rel=1e-5, what=f'bn_stats {name}')
    for form in ('dz + avg + max', 'no dz', 'no max'):
        has_dz, has_max = form != 'no dz', form != 'no max'
        want = R.bn_act_pooled_grads(x, gamma, beta, EPS, act, order, dz if has_dz else None, davg, dmax if has_max else None, amaxp)
        dg0, db0 = like_scaled(want['dgamma'], 1), like_scaled(want['dbeta'], 2)
        pooled = (dad, dmd if has_max else None, apd if has_max else None)

        def run():
            dg, db, dx = dg0.to(d), db0.to(d), dxw.to(d)
            ops.bn_act_backward(dzw.to(d) if has_dz else None, 4, xw, 8, C, mean, rstd, scale, shift, act, order, True, dx, 4, dg, db, pooled=pooled)
            return dx, dg, db
        dx, dg, db = twice(run)
        tag = f'pooled bn_act_backward {act} order {order}, {form}'
        rel_close(dx[..., 4:4 + C], want['dx'], rel=1e-5, what=f'{tag} dx')
        outside_untouched(dx, dxw, 4, C, tag)
        rel_close(accumulated(dg, dg0), want['dgamma'], rel=1e-4, what=f'{tag} dgamma')
        rel_close(accumulated(db, db0), want['dbeta'], rel=1e-4, what=f'{tag} dbeta')
        # the un-fused route: the pooled part added to dz by a pass of its own, then the plain BatchNorm backward
        full = dzw.to(d) if has_dz else torch.zeros(B, H, W, C + 8, device=d)
        ops.pool_backward_add_(full, 4, C, *pooled)
        dg2, db2, dx2 = dg0.to(d), db0.to(d), dxw.to(d)
        ops.bn_act_backward(full, 4, xw, 8, C, mean, rstd, scale, shift, act, order, True, dx2, 4, dg2, db2)
        rel_close(dx[..., 4:4 + C], dx2[..., 4:4 + C], rel=1e-5, what=f'{tag} dx against the un-fused route')
        rel_close(accumulated(dg, dg0), accumulated(dg2, dg0), rel=1e-4, what=f'{tag} dgamma against the un-fused route')
        rel_close(accumulated(db, db0), accumulated(db2, db0), rel=1e-4, what=f'{tag} dbeta against the un-fused route')
