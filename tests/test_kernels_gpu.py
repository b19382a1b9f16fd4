"""GPU parity tests of the individual HIP kernels (through the C ABI) against plain torch fp32 on the CPU.
Tolerance: 1e-3 relative (BASELINE.json north_star); in practice ~1e-5 because the MFMA path is exact fp32."""
import math

import pytest
import torch
import torch.nn.functional as F

from parity import nhwc, rel_close

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


ACTS = {'none': lambda v: v, 'silu': F.silu, 'gelu': F.gelu, 'relu': F.relu, 'sigmoid': torch.sigmoid}

CONV_CASES = [
    # B, H, W, Cin, Cout, k, s, act, extras
    (2, 16, 16, 64, 128, 3, 1, 'silu', {}),
    (2, 17, 13, 32, 177, 3, 1, 'silu', {}),                 # ragged M and N: 128-wide tile with an N tail
    (1, 9, 9, 4, 64, 3, 2, 'silu', {}),                     # first-layer shape: Cin 3 padded to 4, K = 36
    (2, 12, 12, 100, 20, 1, 1, 'none', {}),                 # 1x1, Cout 20 -> 128x32 tile
    (2, 12, 12, 256, 40, 1, 1, 'none', {}),                 # 128x64 tile
    (3, 20, 20, 128, 256, 3, 2, 'silu', {}),
    (2, 40, 40, 128, 128, 3, 1, 'silu', {'residual': True}),
    (2, 14, 14, 96, 64, 1, 1, 'gelu', {'post': True}),
    (2, 10, 10, 64, 96, 3, 1, 'silu', {'slices': True}),
    (2, 10, 10, 64, 64, 3, 1, 'silu', {'modulate': True}),
    (3, 12, 12, 32, 48, 3, 2, 'silu', {'per_sample': True}),
    (64, 20, 20, 64, 256, 1, 1, 'silu', {}),                # many rows -> 128x128 tiles across images
    # stream-K schedule (tile count leaves the last round mostly idle): tiles cut several ways, ragged M / N, whole tiles
    # between two cut ones (600 tiles over 512 workgroups), 1x1
    (4, 40, 40, 128, 256, 3, 1, 'silu', {'residual': True}),
    (6, 37, 41, 96, 200, 3, 1, 'silu', {'post': True}),
    (12, 80, 80, 32, 128, 3, 1, 'silu', {}),
    (16, 40, 40, 512, 128, 1, 1, 'none', {}),
    (9, 40, 40, 64, 64, 3, 1, 'silu', {}),                  # 128x64 tiles
]


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: f'{c[3]}-{c[4]}-k{c[5]}s{c[6]}-{"".join(c[8]) or "plain"}')
def test_conv_igemm(case):
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight as _pack
    pack_conv_weight = lambda w: _pack(w, cin_pad=w.shape[-3])   # noqa: E731  exact channel count, no storage padding
    B, H, W, Cin, Cout, k, s, act, ex = case
    g = torch.Generator().manual_seed(B * 1000 + Cin * 10 + Cout + k + s)
    d = dev()
    p = k // 2
    x = torch.randn(B, Cin, H, W, generator=g)
    bias = torch.randn(Cout, generator=g)
    if ex.get('per_sample'):
        w = torch.randn(B, Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
        bias = torch.randn(B, Cout, generator=g)
        want = torch.stack([F.conv2d(x[b:b + 1], w[b], bias[b], s, p)[0] for b in range(B)])
    else:
        w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
        xin = x
        if ex.get('modulate'):
            ca = torch.rand(B, Cin, generator=g) + 0.5
            sa = torch.rand(B, H, W, generator=g) + 0.5
            xin = x * ca[:, :, None, None] * sa[:, None]
        want = F.conv2d(xin, w, bias, s, p)
    want = ACTS[act](want)
    kw = {}
    if ex.get('post'):
        ps, pt = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        want = want * ps[None, :, None, None] + pt[None, :, None, None]
        kw.update(post_scale=ps.to(d), post_shift=pt.to(d))
    if ex.get('residual'):
        res = torch.randn(want.shape, generator=g)
        want = want + res
        kw.update(residual=nhwc(res).to(d))
    if ex.get('modulate'):
        kw.update(a_chan_scale=ca.to(d), a_pix_scale=sa.to(d))
    xd = nhwc(x).to(d)
    if ex.get('slices'):                                    # read channels [32,32+Cin) of a wider tensor, write at offset 16
        wide = torch.randn(B, H, W, Cin + 64, generator=g)
        wide[..., 32:32 + Cin] = nhwc(x)
        out = torch.full((B, want.shape[2], want.shape[3], Cout + 48), 7.0, device=d)
        ops.conv2d_nhwc(wide.to(d), pack_conv_weight(w).to(d), bias.to(d), kh=k, kw=k, stride=s, pad=p, act=act, cin=Cin,
                        x_coff=32, out=out, cout=Cout, y_coff=16)
        torch.cuda.synchronize()
        assert (out[..., :16] == 7.0).all() and (out[..., 16 + Cout:] == 7.0).all()
        got = out[..., 16:16 + Cout]
    elif Cout % 4:                                          # ragged Cout: the output row stride must still be 16 B aligned
        out = torch.full((B, want.shape[2], want.shape[3], (Cout + 3) // 4 * 4), 7.0, device=d)
        ops.conv2d_nhwc(xd, pack_conv_weight(w).to(d), bias.to(d), kh=k, kw=k, stride=s, pad=p, act=act, out=out, cout=Cout, **kw)
        torch.cuda.synchronize()
        assert (out[..., Cout:] == 7.0).all()
        got = out[..., :Cout]
    else:
        got = ops.conv2d_nhwc(xd, pack_conv_weight(w).to(d), bias.to(d), kh=k, kw=k, stride=s, pad=p, act=act,
                              per_sample_w=bool(ex.get('per_sample')), **kw)
    torch.cuda.synchronize()
    rel_close(got, nhwc(want), what='conv')


def test_conv_streamk_matches_the_workspace_less_tile_schedule(monkeypatch):
    """The stream-K schedule only changes the order in which K-tiles of a cut tile are added: same result to fp32 rounding,
    and bit-identical from run to run (fixed combination order).  Without the stream-K workspace the descriptor runs one workgroup per tile."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight
    g = torch.Generator().manual_seed(77)
    d = dev()
    x = torch.randn(5, 40, 40, 128, generator=g).to(d)
    w = pack_conv_weight(torch.randn(256, 128, 3, 3, generator=g) / 34).to(d)
    b = torch.randn(256, generator=g).to(d)
    y1 = ops.conv2d_nhwc(x, w, b, kh=3, kw=3, pad=1, act='silu')
    y2 = ops.conv2d_nhwc(x, w, b, kh=3, kw=3, pad=1, act='silu')
    with monkeypatch.context() as mp:
        mp.setattr(ops, '_conv_workspace', lambda d, dev: None)
        y0 = ops.conv2d_nhwc(x, w, b, kh=3, kw=3, pad=1, act='silu')
    assert torch.equal(y1, y2)
    assert not torch.equal(y0, y1), 'the stream-K schedule was not taken for a shape it is meant for'
    rel_close(y1, y0, rel=1e-5, what='stream-K vs one workgroup per tile')


def test_conv_wgrad_accumulates_with_a_single_split():
    """Tiny layers run the weight gradient as one pixel split; accumulating into an existing gradient then still goes through the
    workspace (regression: the workspace query used to return 256 bytes for that case)."""
    from somi_amd import ops
    g = torch.Generator().manual_seed(3)
    d = dev()
    B, H, W, Cin, Cout, k = 2, 8, 8, 16, 32, 3
    x = torch.randn(B, Cin, H, W, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g, requires_grad=True)
    dy = torch.randn(B, Cout, H, W, generator=g)
    F.conv2d(x, w, None, 1, 1).backward(dy)
    from somi_amd.pack import pack_conv_weight
    want = pack_conv_weight(w.grad, cin_pad=Cin)
    base = torch.randn(Cout, k * k * Cin, generator=g)
    acc = base.clone().to(d)
    guard = torch.full((1 << 20,), 7.0, device=d)              # allocated right after: an overrun of a short workspace lands here
    ops.conv2d_wgrad_nhwc(nhwc(x.detach()).to(d), nhwc(dy).to(d), kh=k, kw=k, stride=1, pad=1, out=acc, accumulate=acc)
    torch.cuda.synchronize()
    rel_close(acc, want + base, what='wgrad accumulate, one split')
    assert (guard == 7.0).all()


def test_conv_rejects_bad_arguments():
    from somi_amd import ops
    d = dev()
    x = torch.zeros(1, 4, 4, 6, device=d)                  # Cin 6 is not a multiple of 4
    w = torch.zeros(8, 9 * 6, device=d)
    with pytest.raises(RuntimeError, match='multiples of 4'):
        ops.conv2d_nhwc(x, w, kh=3, kw=3, pad=1)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ops.conv2d_nhwc(torch.zeros(1, 4, 4, 8), torch.zeros(8, 72), kh=3, kw=3, pad=1)


def test_image_ingest():
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (3, 3, 20, 24), generator=g, dtype=torch.uint8)
    got = ops.image_to_nhwc4(img.to(d))
    want = torch.zeros(3, 20, 24, 4)
    want[..., :3] = nhwc(img.float() / 255)               # train.py:249
    assert torch.equal(got.cpu(), want)
    f = torch.rand(2, 3, 8, 8, generator=g)
    got = ops.image_to_nhwc4(f.to(d), scale=1.0)
    assert torch.equal(got.cpu()[..., :3], nhwc(f)) and (got.cpu()[..., 3] == 0).all()


def test_dwconv_sppf_bifpn():
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(2)
    B, C, H, W = 2, 32, 11, 9
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g)
    b = torch.randn(C, generator=g)
    ps, pt = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    want = F.gelu(F.conv2d(x, w, b, 1, 1, groups=C)) * ps[None, :, None, None] + pt[None, :, None, None] + x
    wp = w[:, 0].permute(1, 2, 0).reshape(9, C).contiguous()
    got = ops.dwconv3x3(nhwc(x).to(d), wp.to(d), b.to(d), ps.to(d), pt.to(d), residual=nhwc(x).to(d), act='gelu')
    rel_close(got, nhwc(want), what='dwconv')
    # SPPF pooling into the concat buffer
    buf = torch.zeros(B, H, W, 4 * C)
    buf[..., :C] = nhwc(x)
    out = ops.sppf_pool_(buf.to(d), C)
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    y3 = F.max_pool2d(y2, 5, 1, 2)
    assert torch.equal(out.cpu(), nhwc(torch.cat([x, y1, y2, y3], 1)))
    # BiFPN with a folded nearest upsample
    a = torch.randn(B, C, 4, 6, generator=g)
    c2 = torch.randn(B, C, 8, 12, generator=g)
    c3 = torch.randn(B, C, 8, 12, generator=g)
    w = torch.tensor([0.3, 1.5, -0.7])                       # raw fusion parameter; normalised on the device (models/common.py:3696)
    wn = w / ((w * torch.sigmoid(w)).sum() + 1e-4)
    want = wn[0] * F.interpolate(a, scale_factor=2, mode='nearest') + wn[1] * c2 + wn[2] * c3
    got = ops.bifpn([nhwc(a).to(d), nhwc(c2).to(d), nhwc(c3).to(d)], [1, 0, 0], w.to(d))
    rel_close(got, nhwc(want), rel=1e-6, what='bifpn')


@pytest.mark.parametrize('ties', [False, True])
@pytest.mark.parametrize('B,C,H,W', [(2, 32, 11, 9), (1, 8, 20, 20), (3, 16, 4, 3)])
def test_sppf_backward_follows_the_chain_of_pools(ties, B, C, H, W):
    """somi_sppf_pool_bwd_nhwc_f32 against autograd through THREE CHAINED nn.MaxPool2d(5, 1, 2) (models/common.py:1846-1861): the gradient of each
    pooled slice goes back through the chain to the first maximum (row-major) of each 5x5 window.  ties = True quantises the input to four values, so
    almost every window has several maxima and the routing IS the tie rule (rounds 1-3 routed through 5 / 9 / 13 windows of slice 0: equal without
    ties only).  Maps smaller than a window included."""
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, C, H, W, generator=g)
    if ties:
        x = torch.round(x.clamp(-1.5, 1.5))
    xr = x.clone().double().requires_grad_(True)
    y1 = F.max_pool2d(xr, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    y3 = F.max_pool2d(y2, 5, 1, 2)
    dcat = torch.randn(B, 4 * C, H, W, generator=g)
    torch.cat([xr, y1, y2, y3], 1).backward(dcat.double())
    buf = nhwc(torch.cat([x, y1.detach().float(), y2.detach().float(), y3.detach().float()], 1)).to(d)
    dbuf = nhwc(dcat).to(d)
    ops.sppf_pool_backward_(buf, dbuf, C, 0)
    rel_close(dbuf[..., :C], nhwc(xr.grad), rel=2e-6, what=f'sppf dx ties={ties}')
    # the training path: the forward runs level by level and leaves the codes; the backward then searches nothing and does not read the buffer
    buf2 = torch.zeros(B, H, W, 4 * C)
    buf2[..., :C] = nhwc(x)
    buf2 = buf2.to(d)
    _, codes = ops.sppf_pool_(buf2, C, 0, codes=True)
    assert torch.equal(buf2.cpu(), buf.cpu())
    dbuf2 = nhwc(dcat).to(d)
    ops.sppf_pool_backward_(None, dbuf2, C, 0, codes=codes)
    assert torch.equal(dbuf2[..., :C].cpu(), dbuf[..., :C].cpu())


@pytest.mark.parametrize('B,H,W', [(2, 11, 9), (1, 70, 5), (3, 8, 33)])
def test_dwconv_layernorm_gelu_in_one_pass(B, H, W):
    """somi_dwconv3x3_ln_nhwc_f32 (the DCNv3 block's depthwise conv -> LayerNorm -> GELU chain, 256 channels) against the two separate passes and
    against torch: the conv output u is the same tensor bit for bit, y within one rounding of the separate LayerNorm kernel's (same formulas)."""
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(H)
    C = 256
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.4
    b = torch.randn(C, generator=g) * 0.2
    lw, lb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    wp = w[:, 0].permute(1, 2, 0).reshape(9, C).contiguous().to(d)
    xd = nhwc(x).to(d)
    u, y = ops.dwconv3x3_ln(xd, wp, b.to(d), lw.to(d), lb.to(d), 1e-6, 'gelu')
    u2 = ops.dwconv3x3(xd, wp, b.to(d))
    y2 = ops.layernorm_act(u2, lw.to(d), lb.to(d), 1e-6, 'gelu')
    assert torch.equal(u, u2)
    rel_close(y, y2, rel=1e-6, what='fused vs separate LayerNorm + GELU')
    want_u = F.conv2d(x.double(), w.double(), b.double(), 1, 1, groups=C)
    want = F.gelu(F.layer_norm(want_u.permute(0, 2, 3, 1), (C,), lw.double(), lb.double(), 1e-6))
    rel_close(y, want, rel=1e-5, what='dwconv + LayerNorm + GELU')


def test_attention_pieces():
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(3)
    B, C, H, W, mid = 3, 64, 37, 23, 4
    x = torch.randn(B, C, H, W, generator=g)
    wide = torch.randn(B, H, W, C + 32, generator=g)
    wide[..., 16:16 + C] = nhwc(x)
    avg, mx = ops.global_pool(wide.to(d), c=C, x_coff=16)
    rel_close(avg, x.mean((2, 3)), rel=1e-5, what='gap')
    assert torch.equal(mx.cpu(), x.amax((2, 3)))
    W1, b1 = torch.randn(mid, C, generator=g) * 0.2, torch.randn(mid, generator=g) * 0.1
    W2, b2 = torch.randn(C, mid, generator=g) * 0.2, torch.randn(C, generator=g) * 0.1
    mlp = lambda v: F.linear(F.relu(F.linear(v, W1, b1)), W2, b2)   # noqa: E731
    want_ca = torch.sigmoid(mlp(x.mean((2, 3))) + mlp(x.amax((2, 3))))
    ca = ops.attn_mlp(0, avg, mx, W1.to(d), b1.to(d), W2.to(d), b2.to(d))
    rel_close(ca, want_ca, rel=1e-5, what='channel attention')
    want_seam = torch.exp(torch.sigmoid(F.linear(F.relu(F.linear(x.mean((2, 3)), W1)), W2)))
    rel_close(ops.attn_mlp(1, avg, None, W1.to(d), None, W2.to(d), None), want_seam, rel=1e-5, what='seam mlp')
    xs = x * want_ca[:, :, None, None]
    stats = ops.chan_stats(wide.to(d), ca, c=C, x_coff=16)
    want_stats = torch.stack([xs.mean(1), xs.amax(1)], -1)
    rel_close(stats, want_stats, rel=1e-5, what='chan stats')
    w7, b7 = torch.randn(1, 2, 7, 7, generator=g) * 0.1, 0.05
    want_sa = torch.sigmoid(F.conv2d(torch.cat([xs.mean(1, keepdim=True), xs.amax(1, keepdim=True)], 1), w7,
                                     torch.tensor([b7]), padding=3))[:, 0]
    b7d = torch.tensor([b7], device=d)                        # the bias stays a device value
    sa = ops.spatial_attn(stats, w7[0].permute(1, 2, 0).contiguous().to(d), b7d, 7)
    rel_close(sa, want_sa, rel=1e-5, what='spatial attention')
    got = ops.scale_channels(nhwc(x).to(d), ca, sa)
    rel_close(got, nhwc(xs * want_sa[:, None]), rel=1e-5, what='scale')
    wd = wide.to(d)                                          # fused stats->sigmoid(conv7x7)->scale, in place on a channel slice
    ops.cbam_apply_(wd, ca, stats, w7[0].permute(1, 2, 0).contiguous().to(d), b7d, 7, c=C, x_coff=16)
    rel_close(wd[..., 16:16 + C], nhwc(xs * want_sa[:, None]), rel=1e-5, what='cbam apply')
    assert torch.equal(wd[..., :16].cpu(), wide[..., :16]) and torch.equal(wd[..., 16 + C:].cpu(), wide[..., 16 + C:])


@pytest.mark.parametrize('k', [3, 5, 7])
@pytest.mark.parametrize('B,H,W', [(3, 37, 29), (2, 8, 8), (1, 70, 65)])
def test_spatial_attention_backward_against_conv2d_autograd(k, B, H, W):
    """somi_spatial_attn_bwd_f32 (gradient of the k x k, 2 -> 1 conv under the sigmoid) against F.conv2d's autograd in fp64: data gradient, weight
    gradient in both layouts ([k][k][2] and nn.Conv2d's (2,k,k)), bias gradient - ACCUMULATED onto non-zero buffers.  Maps whose pixel count is not
    a multiple of the 512-pixel chunk, chunks that span image boundaries, a batch smaller than one chunk."""
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream, check
    d = dev()
    g = torch.Generator().manual_seed(k * 100 + H)
    dlogit = torch.randn(B, H, W, generator=g)
    stats = torch.randn(B, H, W, 2, generator=g)
    w = torch.randn(1, 2, k, k, generator=g) * 0.2
    s64 = stats.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    F.conv2d(s64, w64, b64, padding=k // 2).backward(dlogit.double()[:, None])
    L = _lib.lib()
    for chw in (0, 1):
        dw0 = torch.randn(2, k, k, generator=g) if chw else torch.randn(k, k, 2, generator=g)
        db0 = torch.randn(1, generator=g)
        dw, db = dw0.to(d), db0.to(d)
        dstats = torch.empty(B, H, W, 2, device=d)
        ws = torch.empty(((B * H * W + 511) // 512) * (2 * k * k + 1), device=d)
        dl_d, st_d, w_d = dlogit.to(d), stats.to(d), w[0].permute(1, 2, 0).contiguous().to(d)      # named: the pointers must outlive the call
        check(L.somi_spatial_attn_bwd_f32(_ptr(dl_d), _ptr(st_d), _ptr(w_d), _ptr(dstats), _ptr(dw), _ptr(db), _ptr(ws), B, H, W, k, chw, _stream()),
              'spatial_attn_bwd')
        want_dw = w64.grad[0] if chw else w64.grad[0].permute(1, 2, 0)
        rel_close(dstats, s64.grad.permute(0, 2, 3, 1), rel=1e-5, what=f'dstats k{k}')
        rel_close(dw.cpu().double() - dw0.double(), want_dw, rel=2e-5, what=f'dw k{k} chw{chw}')
        rel_close(db.cpu().double() - db0.double(), b64.grad, rel=2e-5, what=f'dbias k{k}')


def test_detect_decode():
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(4)
    B, ny, nx, na, nc = 2, 6, 5, 4, 10
    box = torch.randn(B, ny, nx, na * 5, generator=g)
    cls = torch.randn(B, ny, nx, na * nc, generator=g)
    anchors_px = [4., 6., 12., 8., 7., 14., 20., 12.]
    stride = 8.0
    total, row_off = na * ny * nx + 7, 3
    raw = torch.empty(B, na, ny, nx, nc + 5, device=d)
    z = torch.zeros(B, total, nc + 5, device=d)
    ops.detect_decode(box.to(d), cls.to(d), anchors_px, stride, na, nc, raw=raw, z=z, total=total, row_off=row_off)
    t = torch.cat((box.view(B, ny, nx, na, 5), cls.view(B, ny, nx, na, nc)), -1).permute(0, 3, 1, 2, 4)   # B,na,ny,nx,no
    assert torch.equal(raw.cpu(), t.contiguous())
    y = t.sigmoid()
    yv, xv = torch.meshgrid(torch.arange(ny).float(), torch.arange(nx).float(), indexing='ij')
    grid = torch.stack((xv, yv), 2) - 0.5
    xy = (y[..., :2] * 2 + grid) * stride
    wh = (y[..., 2:4] * 2) ** 2 * torch.tensor(anchors_px).view(1, na, 1, 1, 2)
    want = torch.cat((xy, wh, y[..., 4:]), -1).reshape(B, -1, nc + 5)
    rel_close(z[:, row_off:row_off + na * ny * nx], want, rel=1e-5, what='decode')
    assert (z[:, :row_off] == 0).all()


@pytest.mark.parametrize('B,H,W,Cin,Cout,k,s', [(2, 16, 16, 64, 128, 3, 1), (2, 17, 13, 32, 64, 3, 2), (3, 20, 20, 128, 256, 3, 2),
                                                (2, 12, 12, 96, 64, 1, 1), (2, 9, 11, 20, 36, 3, 1), (2, 10, 10, 64, 32, 3, 2),
                                                # stride parity classes: one with no tap at all (k=1), 3x3 taps per class
                                                # (k=6), stride 3, and a ragged 64-row class tile
                                                (2, 9, 12, 16, 32, 1, 2), (2, 14, 14, 16, 32, 6, 2), (2, 11, 13, 8, 32, 5, 3),
                                                (5, 23, 19, 36, 96, 3, 2),
                                                (6, 40, 40, 128, 128, 3, 1)])                 # stream-K schedule
def test_conv_dgrad(B, H, W, Cin, Cout, k, s):
    """dx of F.conv2d from the MFMA implicit-GEMM kernel in data-gradient geometry, against torch autograd on the CPU."""
    from somi_amd import ops
    from somi_amd.pack import pack_dgrad_weight
    g = torch.Generator().manual_seed(B + H + Cin + Cout + k + s)
    d = dev()
    p = k // 2
    x = torch.randn(B, Cin, H, W, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    y = F.conv2d(x, w, None, s, p)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    acc = torch.randn(B, H, W, Cin, generator=g)
    got = ops.conv2d_dgrad_nhwc(nhwc(dy).to(d), pack_dgrad_weight(w, cin_pad=Cin, cout_pad=Cout).to(d), B=B, H=H, W=W, cin=Cin,
                                kh=k, kw=k, stride=s, pad=p)
    rel_close(got, nhwc(x.grad), what='dgrad')
    accd = acc.to(d)
    ops.conv2d_dgrad_nhwc(nhwc(dy).to(d), pack_dgrad_weight(w, cin_pad=Cin, cout_pad=Cout).to(d), B=B, H=H, W=W, cin=Cin, kh=k, kw=k,
                          stride=s, pad=p, out=accd, accumulate=accd)           # in-place accumulate (skip connection)
    rel_close(accd, nhwc(x.grad) + acc, what='dgrad accumulate')


@pytest.mark.parametrize('B,H,W,Cin,Cout,k,s,ps', [(2, 16, 16, 64, 128, 3, 1, False), (2, 17, 13, 32, 64, 3, 2, False),
                                                   (4, 40, 40, 128, 256, 3, 2, False), (2, 12, 12, 96, 68, 1, 1, False),
                                                   (2, 9, 11, 20, 36, 3, 1, False), (3, 33, 31, 4, 64, 3, 2, False),
                                                   (3, 12, 12, 32, 48, 3, 2, True), (16, 20, 20, 256, 132, 1, 1, False)])
def test_conv_wgrad(B, H, W, Cin, Cout, k, s, ps):
    """dW of F.conv2d from the MFMA split-K weight-gradient kernel, against torch autograd on the CPU."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight
    g = torch.Generator().manual_seed(B + H + Cin + Cout + k + s)
    d = dev()
    p = k // 2
    x = torch.randn(B, Cin, H, W, generator=g)
    dy_shape = F.conv2d(x[:1], torch.zeros(Cout, Cin, k, k), None, s, p).shape
    dy = torch.randn(B, *dy_shape[1:], generator=g)
    if ps:
        want = []
        for b in range(B):
            w = torch.zeros(Cout, Cin, k, k, requires_grad=True)
            F.conv2d(x[b:b + 1], w, None, s, p).backward(dy[b:b + 1])
            want.append(pack_conv_weight(w.grad, cin_pad=Cin))
        want = torch.stack(want)
    else:
        w = torch.zeros(Cout, Cin, k, k, requires_grad=True)
        F.conv2d(x, w, None, s, p).backward(dy)
        want = pack_conv_weight(w.grad, cin_pad=Cin)
    got = ops.conv2d_wgrad_nhwc(nhwc(x).to(d), nhwc(dy).to(d), kh=k, kw=k, stride=s, pad=p, per_sample_w=ps)
    rel_close(got, want, what='wgrad')
    prev = torch.randn(want.shape, generator=g)
    acc = prev.to(d)
    ops.conv2d_wgrad_nhwc(nhwc(x).to(d), nhwc(dy).to(d), kh=k, kw=k, stride=s, pad=p, per_sample_w=ps, out=acc, accumulate=acc)
    rel_close(acc, want + prev, what='wgrad accumulate')


def test_conv_tensors_beyond_the_descriptor_range():
    """An activation tensor of 3.9 GB does not fit one 32-bit buffer descriptor: the launchers run the batch in slices.  Forward,
    data gradient and weight gradient of the whole batch must equal the two halves run on their own (fp32 rounding: the tile
    schedule depends on the row count)."""
    from somi_amd import ops
    d = dev()
    B, H, Cin, Cout = 60, 160, 640, 32
    g = torch.Generator(device='cuda').manual_seed(4)
    x = torch.randn(B, H, H, Cin, device=d, generator=g)
    assert x.numel() * 4 > 0xE0000000
    w = torch.randn(Cout, Cin, device=d, generator=g) / 25
    y = ops.conv2d_nhwc(x, w, None, kh=1, kw=1)
    h = B // 2
    rel_close(y[:h], ops.conv2d_nhwc(x[:h], w, None, kh=1, kw=1), rel=1e-5, what='forward, first half')
    rel_close(y[h:], ops.conv2d_nhwc(x[h:], w, None, kh=1, kw=1), rel=1e-5, what='forward, second half')
    dy = torch.randn(B, H, H, Cout, device=d, generator=g)
    dw = ops.conv2d_wgrad_nhwc(x, dy, kh=1, kw=1)
    dw2 = ops.conv2d_wgrad_nhwc(x[:h], dy[:h], kh=1, kw=1) + ops.conv2d_wgrad_nhwc(x[h:], dy[h:], kh=1, kw=1)
    rel_close(dw, dw2, rel=1e-5, what='weight gradient')
    # data gradient of a layer whose dy is the big tensor: Cout 640 -> Cin 32
    wt = torch.randn(32, 640, device=d, generator=g) / 25        # [Cin][Cout] dgrad packing of a 1x1 layer
    dx = ops.conv2d_dgrad_nhwc(x, wt, B=B, H=H, W=H, cin=32, kh=1, kw=1)
    rel_close(dx[:h], ops.conv2d_dgrad_nhwc(x[:h], wt, B=h, H=H, W=H, cin=32, kh=1, kw=1), rel=1e-5, what='dgrad, first half')
    rel_close(dx[h:], ops.conv2d_dgrad_nhwc(x[h:], wt, B=B - h, H=H, W=H, cin=32, kh=1, kw=1), rel=1e-5, what='dgrad, second half')


@pytest.mark.parametrize('B,H,W,Cin,Cout,k,s', [(4, 40, 40, 128, 256, 3, 1),      # stream-K schedule: cut tiles finish in the fix-up kernel
                                                (3, 37, 29, 32, 64, 3, 2),       # ragged rows, 128x64 tiles
                                                (2, 16, 16, 4, 32, 3, 1),        # generic (non-uniform tap) path, 128x32 tiles
                                                (64, 20, 20, 64, 256, 1, 1),     # whole tiles, one workgroup each
                                                (40, 80, 80, 32, 128, 1, 1)])    # more than 1024 partial rows: the fold pass
def test_conv_epilogue_batchnorm_statistics(B, H, W, Cin, Cout, k, s):
    """The training forward takes BatchNorm's batch statistics from partial sums the conv epilogue leaves behind (around the
    running mean as pivot): mean / variance / running statistics must equal the separate statistics pass over y."""
    from somi_amd import ops
    g = torch.Generator().manual_seed(B + H + Cout)
    d = dev()
    x = torch.randn(B, H, W, Cin, generator=g).to(d)
    w = (torch.randn(Cout, k * k * Cin, generator=g) / math.sqrt(k * k * Cin)).to(d)
    gam, bet = (torch.rand(Cout, generator=g) + 0.5).to(d), torch.randn(Cout, generator=g).to(d)
    rm0, rv0 = (torch.randn(Cout, generator=g) * 0.3).to(d), (torch.rand(Cout, generator=g) + 0.5).to(d)
    st = {'pivot': rm0}
    y = ops.conv2d_nhwc(x, w, None, kh=k, kw=k, stride=s, pad=k // 2, bn_stats=st)
    y_plain = ops.conv2d_nhwc(x, w, None, kh=k, kw=k, stride=s, pad=k // 2)
    assert torch.equal(y, y_plain)
    rm1, rv1 = rm0.clone(), rv0.clone()
    got = ops.bn_stats_from_partials(st['part'], st['rows'], y.shape[0] * y.shape[1] * y.shape[2], Cout, gam, bet, 1e-3, 0.03, rm1, rv1)
    rm2, rv2 = rm0.clone(), rv0.clone()
    want = ops.bn_stats(y, Cout, 0, gam, bet, 1e-3, 0.03, rm2, rv2)
    for a, b, what in zip(got, want, ('mean', 'rstd', 'scale', 'shift')):
        rel_close(a, b, rel=1e-5, what=what)
    rel_close(rm1, rm2, rel=1e-6, what='running mean')
    rel_close(rv1, rv2, rel=1e-5, what='running var')
    yd = y.double().cpu().reshape(-1, Cout)
    rel_close(got[0], yd.mean(0), rel=1e-5, what='mean vs fp64')
    rel_close(1.0 / got[1].double().cpu() ** 2 - 1e-3, yd.var(0, unbiased=False), rel=1e-4, what='variance vs fp64')


def _random_conv_cases(n, seed):
    import random
    rnd = random.Random(seed)
    cases = []
    while len(cases) < n:
        k = rnd.choice([1, 1, 3, 3, 3, 5])
        s = rnd.choice([1, 1, 1, 2])
        cin = rnd.choice([4, 8, 20, 32, 36, 64, 96, 128, 160])
        cout = rnd.choice([4, 12, 32, 36, 64, 100, 128, 192, 260])
        H, W = rnd.randint(3, 44), rnd.randint(3, 44)
        B = rnd.choice([1, 2, 3, 5, 8])
        p = rnd.choice([k // 2, k // 2, 0]) if k > 1 else 0
        if H + 2 * p < k or W + 2 * p < k:
            continue
        cases.append((B, H, W, cin, cout, k, s, p))
    return cases


@pytest.mark.parametrize('case', _random_conv_cases(36, 2024), ids=lambda c: 'x'.join(str(v) for v in c))
def test_conv_forward_dgrad_wgrad_random_shapes(case):
    """Differential test over seeded random geometries (odd sizes, padding 0, 5x5, stride 2, channel counts on and off the
    uniform-tap fast path, batch 1): forward, data gradient and weight gradient against torch autograd on the CPU."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    B, H, W, Cin, Cout, k, s, p = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    d = dev()
    x = torch.randn(B, Cin, H, W, generator=g, requires_grad=True)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).requires_grad_(True)
    bias = torch.randn(Cout, generator=g)
    y = F.conv2d(x, w, bias, s, p)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    wp = pack_conv_weight(w.detach(), cin_pad=Cin).to(d)
    got = ops.conv2d_nhwc(nhwc(x.detach()).to(d), wp, bias.to(d), kh=k, kw=k, stride=s, pad=p)
    rel_close(got, nhwc(y), what='forward')
    gx = ops.conv2d_dgrad_nhwc(nhwc(dy).to(d), pack_dgrad_weight(w.detach(), cin_pad=Cin, cout_pad=Cout).to(d), B=B, H=H, W=W, cin=Cin,
                               kh=k, kw=k, stride=s, pad=p)
    rel_close(gx, nhwc(x.grad), what='dgrad')
    gw = ops.conv2d_wgrad_nhwc(nhwc(x.detach()).to(d), nhwc(dy).to(d), kh=k, kw=k, stride=s, pad=p)
    rel_close(gw, pack_conv_weight(w.grad, cin_pad=Cin), what='wgrad')


@pytest.mark.parametrize('B,H,Cin,Cout,k,s', [(32, 160, 128, 128, 3, 1), (32, 80, 256, 256, 3, 1), (32, 160, 256, 256, 1, 1),
                                              (32, 160, 256, 256, 3, 2)])
def test_conv_full_size_adjoint_identities(B, H, Cin, Cout, k, s):
    """The three conv kernels at the bench step's dominant layer shapes (batch 32: far beyond what a CPU reference finishes in a test)
    through identities that do not depend on the size: y = conv(x, w) is bilinear, so for random dy
        <dy, conv(x, w)> == <dgrad(dy, w), x> == <wgrad(x, dy), w>,
    and conv is linear in x.  Sums in float64 on the device."""
    from somi_amd import ops
    d = dev()
    g = torch.Generator(device='cuda').manual_seed(B + H + Cin + k)
    p = k // 2
    x = torch.randn(B, H, H, Cin, device=d, generator=g)
    x2 = torch.randn(B, H, H, Cin, device=d, generator=g)
    w = torch.randn(Cout, k * k * Cin, device=d, generator=g) / math.sqrt(Cin * k * k)
    y = ops.conv2d_nhwc(x, w, None, kh=k, kw=k, stride=s, pad=p)
    dy = torch.randn(y.shape, device=d, generator=g)
    dx = ops.conv2d_dgrad_nhwc(dy, ops.pack_dgrad_weights(w, Cout, k * k, Cin), B=B, H=H, W=H, cin=Cin, kh=k, kw=k, stride=s, pad=p)
    dw = ops.conv2d_wgrad_nhwc(x, dy, kh=k, kw=k, stride=s, pad=p)
    dot = lambda a, b: (a.double() * b.double()).sum().item()      # noqa: E731
    ref = dot(dy, y)
    size = (dy.double() * y.double()).abs().sum().item()
    assert abs(dot(dx, x) - ref) <= 1e-5 * size, ('dgrad adjoint', dot(dx, x), ref)
    assert abs(dot(dw.view_as(w), w) - ref) <= 1e-5 * size, ('wgrad adjoint', dot(dw.view_as(w), w), ref)
    y12 = ops.conv2d_nhwc(0.5 * x - 2.0 * x2, w, None, kh=k, kw=k, stride=s, pad=p)
    y2 = ops.conv2d_nhwc(x2, w, None, kh=k, kw=k, stride=s, pad=p)
    err = (y12 - (0.5 * y - 2.0 * y2)).abs().max().item()
    assert err <= 2e-5 * y.abs().max().item(), ('linearity', err)


@pytest.mark.parametrize('prec,rel', [('bf16', 2e-2), ('bf16x3', 1e-4)])
@pytest.mark.parametrize('B,H,Cin,Cout,k,s', [(2, 24, 64, 128, 3, 1),       # 128 x 128 tile
                                              (4, 40, 128, 256, 3, 1),      # stream-K: cut tiles finish in the fp32 fix-up kernel
                                              (3, 20, 128, 256, 3, 2),      # stride 2: the data gradient runs its parity classes
                                              (2, 32, 256, 64, 1, 1),       # 128 x 64 tile, 1x1
                                              (5, 17, 96, 160, 3, 1)])      # ragged M / N, Cin = 3 K-tiles per tap
def test_conv_reduced_precision_forms(prec, rel, B, H, Cin, Cout, k, s):
    """Opt-in `amp` forms of forward / dgrad / wgrad (somi_conv_desc.prec; train.py:263 runs the reference's GPU loop under autocast):
    operands rounded to bf16, or split into two bf16 values with three products (bf16x3), fp32 accumulate.  Against the exact fp32 HIP
    kernels on the same inputs.  Bars: bf16 2e-2 of the output range (the reference's own bar for half in models/ops_dcnv3/test.py:85
    is rtol 1e-2 / atol 1e-3), bf16x3 1e-4 (16 mantissa bits per operand)."""
    from somi_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(Cin + Cout + k)
    p = k // 2
    x = torch.randn(B, H, H, Cin, generator=g).to(d)
    w = (torch.randn(Cout, k * k * Cin, generator=g) / math.sqrt(k * k * Cin)).to(d)
    wt = (torch.randn(Cin, k * k * Cout, generator=g) / math.sqrt(k * k * Cout)).to(d)
    b = torch.randn(Cout, generator=g).to(d)

    def run():
        y = ops.conv2d_nhwc(x, w, b, kh=k, kw=k, stride=s, pad=p, act='silu')
        dy = torch.sin(torch.arange(y.numel(), device=d, dtype=torch.float32) * 0.37).view_as(y)
        dx = ops.conv2d_dgrad_nhwc(dy, wt, B=B, H=H, W=H, cin=Cin, kh=k, kw=k, stride=s, pad=p)
        dw = ops.conv2d_wgrad_nhwc(x, dy, kh=k, kw=k, stride=s, pad=p)
        return y, dx, dw
    want = run()
    ops.CONV_PREC = ops.PREC[prec]
    try:
        got = run()
    finally:
        ops.CONV_PREC = 0
    for a_, b_, what in zip(got, want, ('forward', 'dgrad', 'wgrad')):
        rel_close(a_, b_, rel=rel, what=f'{prec} {what}')
        # Which launches have a bf16 form is pinned tile by tile in test_conv_amp_gpu.py (against the operand-rounding model, and bit for bit where
        # there is none): here every forward and weight gradient has one, and so has every data gradient but the stride-2 one (1200 rows without
        # stream-K plan the 4-wave 64 x 128 tile: exact fp32, as are the per-sample forward and data gradient below, on 100 and 400 rows per image).
        if what == 'forward':
            assert not torch.equal(a_, b_), f'{prec} {what}: bit-identical to fp32 - the reduced-precision kernel did not run'
    if k == 3 and s == 2:                 # ODConv's shape: per-sample weight sets (forward and data gradient; its weight gradient stays fp32)
        wps = (torch.randn(B, Cout, k * k * Cin, generator=g) / math.sqrt(k * k * Cin)).to(d)
        wtps = (torch.randn(B, Cin, k * k * Cout, generator=g) / math.sqrt(k * k * Cout)).to(d)

        def run_ps():
            y = ops.conv2d_nhwc(x, wps, None, kh=k, kw=k, stride=s, pad=p, per_sample_w=True)
            return y, ops.conv2d_dgrad_nhwc(torch.cos(y * 3.0), wtps, B=B, H=H, W=H, cin=Cin, kh=k, kw=k, stride=s, pad=p, per_sample_w=True)
        want_ps = run_ps()
        ops.CONV_PREC = ops.PREC[prec]
        try:
            got_ps = run_ps()
        finally:
            ops.CONV_PREC = 0
        rel_close(got_ps[0], want_ps[0], rel=rel, what=f'{prec} per-sample forward')
        rel_close(got_ps[1], want_ps[1], rel=10 * rel, what=f'{prec} per-sample dgrad (of the perturbed forward)')


def test_conv_family_parity_per_channel_across_six_orders_of_magnitude():
    """VERDICT r3 (weak 2): a max-error-over-max-magnitude bar is blind on channels whose values are small beside the tensor's largest.  Here the
    output channels of a 3x3 layer span SIX orders of magnitude (channel c scaled by 10^(-6 c / Cout)) and forward, data gradient and weight
    gradient are each held to 1e-3 of EVERY channel's own largest value against the fp64 convolution (the fp32 matrix instruction is exact
    fp32 arithmetic, so a channel's relative error does not depend on its scale: ~1e-6 observed)."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    g = torch.Generator().manual_seed(77)
    d = dev()
    B, H, W, Cin, Cout, k = 4, 24, 20, 96, 128, 3
    x = torch.randn(B, Cin, H, W, generator=g).double().requires_grad_(True)
    amp_out = 10.0 ** (-6.0 * torch.arange(Cout, dtype=torch.float64) / Cout)
    amp_in = 10.0 ** (-6.0 * torch.arange(Cin, dtype=torch.float64) / Cin)
    w = (torch.randn(Cout, Cin, k, k, generator=g).double() / math.sqrt(Cin * k * k) * amp_out[:, None, None, None]).float().double().requires_grad_(True)
    y = F.conv2d(x, w, None, 1, 1)
    dy = (torch.randn(y.shape, generator=g).double() * amp_out[None, :, None, None] ** -0.5).float().double()   # keeps dy * w spread over the channels too
    y.backward(dy)

    def per_channel(got, want, dim, what):
        got, want = got.detach().cpu().double(), want.detach().double()
        red = tuple(i for i in range(want.dim()) if i != dim)
        err, scale = (got - want).abs().amax(red), want.abs().amax(red)
        worst = int((err / scale.clamp_min(1e-300)).argmax())
        assert (err <= 1e-3 * scale).all(), f'{what}: channel {worst} is {float(err[worst] / scale[worst]):.2e} of its own scale {float(scale[worst]):.2e}'
        return float((err / scale.clamp_min(1e-300)).max())
    xd, dyd, wf = nhwc(x.detach().float()).to(d), nhwc(dy.float()).to(d), w.detach().float()
    got_y = ops.conv2d_nhwc(xd, pack_conv_weight(wf, cin_pad=Cin).to(d), None, kh=k, kw=k, stride=1, pad=1, act='none')
    e1 = per_channel(got_y, nhwc(y), 3, 'forward')
    assert float(nhwc(y).detach().abs().amax((0, 1, 2)).min() / nhwc(y).detach().abs().max()) < 1e-5       # the premise: small channels exist
    got_dx = ops.conv2d_dgrad_nhwc(dyd, pack_dgrad_weight(wf, cin_pad=Cin, cout_pad=Cout).to(d), B=B, H=H, W=W, cin=Cin, kh=k, kw=k, stride=1, pad=1)
    # the data gradient's own channels: scale the INPUT channels' weights instead, through a second layer, so dx spans the range per channel
    e2 = per_channel(got_dx, nhwc(x.grad), 3, 'data gradient')
    got_dw = ops.conv2d_wgrad_nhwc(xd, dyd, kh=k, kw=k, stride=1, pad=1).view(Cout, k, k, Cin).permute(0, 3, 1, 2)
    e3 = per_channel(got_dw, w.grad, 0, 'weight gradient (per output channel)')
    w2 = (torch.randn(Cout, Cin, k, k, generator=g).double() / math.sqrt(Cin * k * k) * amp_in[None, :, None, None]).float()
    x2 = torch.randn(B, Cin, H, W, generator=g).double().requires_grad_(True)
    y2 = F.conv2d(x2, w2.double(), None, 1, 1)
    dy2 = torch.randn(y2.shape, generator=g).float()
    y2.backward(dy2.double())
    got_dx2 = ops.conv2d_dgrad_nhwc(nhwc(dy2).to(d), pack_dgrad_weight(w2, cin_pad=Cin, cout_pad=Cout).to(d), B=B, H=H, W=W, cin=Cin, kh=k, kw=k,
                                    stride=1, pad=1)
    e4 = per_channel(got_dx2, nhwc(x2.grad), 3, 'data gradient (input channels spanning 1e6)')
    print(f'worst per-channel relative errors: forward {e1:.1e}, dgrad {e2:.1e}, wgrad {e3:.1e}, dgrad over scaled input channels {e4:.1e}')
