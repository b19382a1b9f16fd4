"""The entry points that only block and model tests used to reach, one by one through their ops wrappers against the same operation in float64
on the CPU (torch autograd or the oracle module; tests/support_kernels_ref.py): depthwise 3x3 backward and forward, LayerNorm+GELU backward, BiFPN
forward and backward, the centre-feature-scale blend and its backward, both detect decodes and their raw backwards, the test-time-augmentation
resample / resize / descale and the image ingest - at the sizes where their loops and thread mappings change (the case lists say which).

Bars: 1e-5 of max |want| for pointwise results, 2e-5 for sums over pixels, torch.equal for permutations; bilinear resampling four times what
torch's float32 evaluation on the CPU is off by.  Accumulated outputs start from noise and the added part is compared; what a call must not touch
starts as a NaN sentinel and is compared bit for bit.  tests/test_support_kernels_host.py holds the same inputs to half these bars in float32."""
import pytest
import torch

import support_kernels_ref as R
from parity import nhwc, rel_close

pytestmark = pytest.mark.gpu
NAN = float('nan')
F64 = torch.float64


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def sentinel(*shape):
    return torch.full(shape, NAN, device=dev())


def same_bits(a, b, what):
    a, b = a.cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: bits changed'


def untouched(t, what):
    same_bits(t, torch.full(t.shape, NAN), what)


def added(buf, start, want, what):
    rel_close(buf.cpu().double() - start.double(), want, rel=R.REDUCED, what=what)


def api():
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream, check
    return _lib.lib(), _ptr, _stream, check


# ------------------------------------------------------------------------------------------------------------------- depthwise 3x3
@pytest.mark.parametrize('case', R.DW_BWD_CASES, ids=R.ident)
def test_dwconv3x3_backward(case):
    """dx (plain and added onto dx_accumulate), dw and dbias (added onto noise; dbias=None leaves dw as it is) against F.conv2d(groups=C) autograd."""
    from somi_amd import ops
    d = dev()
    c = R.dw_inputs(case)
    want = R.dw_backward(c, F64)
    x, dy, wp, acc = nhwc(c.x).to(d), nhwc(c.dy).to(d), R.dw_pack(c.w).to(d), nhwc(c.acc)
    acc_d = acc.to(d)
    print(f'{case}: {R.dw_chunks(case)} chunks')
    for accumulate, with_bias in ((False, True), (True, True), (False, False)):
        tag = f'dwconv bwd {case} accumulate={accumulate} dbias={with_bias}'
        dw, db = c.dw0.to(d), c.db0.to(d) if with_bias else None
        dx = ops.dwconv3x3_backward(dy, x, wp, dw, db, dx_accumulate=acc_d if accumulate else None)
        rel_close(dx, want.dx + acc.double() if accumulate else want.dx, rel=R.POINT, what=f'{tag}: dx')
        added(dw, c.dw0, want.dw, f'{tag}: dw')
        if with_bias:
            added(db, c.db0, want.db, f'{tag}: dbias')
    same_bits(acc_d, acc, 'dx_accumulate is read only')


def test_dwconv3x3_backward_refuses_a_width_whose_quads_do_not_divide_256():
    from somi_amd import ops
    L, p, stream, check = api()
    d = dev()
    B, Cc, H, W = R.DW_BWD_REFUSED
    c = R.dw_inputs(R.DW_BWD_REFUSED)
    x, dy, wp = nhwc(c.x).to(d), nhwc(c.dy).to(d), R.dw_pack(c.w).to(d)
    dx, dw, db = sentinel(B, H, W, Cc), sentinel(9, Cc), sentinel(Cc)
    ws = torch.empty(max(L.somi_dwconv3x3_bwd_workspace_floats(B, W, Cc), 1), device=d)
    rc = L.somi_dwconv3x3_bwd_nhwc_f32(p(dy), p(x), p(wp), p(dx), None, p(dw), p(db), p(ws), B, H, W, Cc, stream())
    with pytest.raises(RuntimeError, match='must divide 256'):
        check(rc, 'dwconv3x3_bwd')
    torch.cuda.synchronize()
    for t, n in ((dx, 'dx'), (dw, 'dw'), (db, 'dbias')):
        untouched(t, f'{n} after the refusal')
    dw, db = c.dw0.to(d), c.db0.to(d)
    with pytest.raises(RuntimeError, match='must divide 256'):
        ops.dwconv3x3_backward(dy, x, wp, dw, db)
    same_bits(dw, c.dw0, 'dw after the refusal')
    same_bits(db, c.db0, 'dbias after the refusal')


@pytest.mark.parametrize('case', R.DW_FWD_CASES, ids=R.ident)
def test_dwconv3x3_forward(case):
    """gelu(conv + bias) * post_scale + post_shift + residual with 16-row (H = 70) and 8-row (H = 9) segments, with and without the bias."""
    from somi_amd import ops
    d = dev()
    c = R.dw_inputs(case)
    B, Cc, H, W, bias = case
    got = ops.dwconv3x3(nhwc(c.x).to(d), R.dw_pack(c.w).to(d), c.b.to(d) if bias else None, c.ps.to(d), c.pt.to(d), residual=nhwc(c.res).to(d),
                        act='gelu', out=sentinel(B, H, W, Cc))
    rel_close(got, R.dw_forward(c, F64, bias), rel=R.POINT, what=f'dwconv forward {case}')


# ------------------------------------------------------------------------------------------------------------------- LayerNorm + GELU backward
@pytest.mark.parametrize('case', R.LN_CASES, ids=R.ident)
def test_layernorm_gelu_backward(case):
    """du, and dgamma / dbeta added onto noise, against F.gelu(F.layer_norm(u)) autograd."""
    from somi_amd import ops
    d = dev()
    c = R.ln_inputs(case)
    want = R.ln_backward(c, F64)
    dgamma, dbeta = c.dgamma0.to(d), c.dbeta0.to(d)
    du = ops.layernorm_gelu_backward(c.u.to(d), c.gamma.to(d), c.beta.to(d), R.EPS_LN, c.dz.to(d), dgamma, dbeta)
    rel_close(du, want.du, rel=R.POINT, what=f'LN+GELU bwd {case}: du')
    added(dgamma, c.dgamma0, want.dgamma, f'LN+GELU bwd {case}: dgamma')
    added(dbeta, c.dbeta0, want.dbeta, f'LN+GELU bwd {case}: dbeta')


def test_layernorm_gelu_backward_refuses_more_than_2048_channels():
    from somi_amd import ops
    d = dev()
    n, Cc = R.LN_REFUSED
    g = torch.Generator().manual_seed(n)
    u, dz = torch.randn(n, Cc, generator=g).to(d), torch.randn(n, Cc, generator=g).to(d)
    dg0, db0 = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    dgamma, dbeta = dg0.to(d), db0.to(d)
    with pytest.raises(RuntimeError, match='C up to 2048'):
        ops.layernorm_gelu_backward(u, torch.ones(Cc, device=d), torch.zeros(Cc, device=d), R.EPS_LN, dz, dgamma, dbeta)
    same_bits(dgamma, dg0, 'dgamma after the refusal')
    same_bits(dbeta, db0, 'dbeta after the refusal')


# ------------------------------------------------------------------------------------------------------------------- BiFPN
@pytest.mark.parametrize('case', R.BIFPN_CASES, ids=R.ident)
def test_bifpn_forward_and_backward(case):
    """The fusion, the gradient of every source (2x2 sums for an upsampled one) and dw added onto noise against the oracle's BiFPN under autograd,
    with a negative fusion weight."""
    from somi_amd import ops
    d = dev()
    ups, B, Cc, H, W = case
    c = R.bifpn_inputs(case)
    want = R.bifpn_ref(c, ups, F64)
    srcs, w, dout = [nhwc(s).to(d) for s in c.srcs], c.w.to(d), nhwc(c.dout).to(d)
    rel_close(ops.bifpn(srcs, list(ups), w, out=sentinel(B, H, W, Cc)), want.out, rel=R.POINT, what=f'bifpn {case}')
    dw = c.dw0.to(d)
    dsrcs = ops.bifpn_backward(srcs, list(ups), w, dout, dw)
    for i, (a, b) in enumerate(zip(dsrcs, want.dsrcs)):
        rel_close(a, b, rel=R.POINT, what=f'bifpn bwd {case}: dsrc {i}')
    added(dw, c.dw0, want.dw, f'bifpn bwd {case}: dw')


# ------------------------------------------------------------------------------------------------------------------- centre-feature-scale blend
@pytest.mark.parametrize('case', R.CFS_CASES, ids=R.ident)
def test_cfs_blend_forward_and_backward(case):
    """Logits out to +-8 in rows wider than G: out, dx, dxproj, dlogit; the columns of dlogit behind G are zero from the wrapper and are not
    written by the kernel."""
    from somi_amd import ops
    L, p, stream, check = api()
    d = dev()
    n, G, Gc = case
    c = R.cfs_inputs(case)
    want = R.cfs_ref(c, G, Gc, F64)
    x, xp, lg, dout = c.x.to(d), c.xproj.to(d), c.logit.to(d), c.dout.to(d)
    rel_close(ops.cfs_blend(x, xp, lg, G, Gc), want.out, rel=R.POINT, what=f'cfs {case}: out')
    dx, dxp, dlogit = ops.cfs_blend_backward(x, xp, lg, dout, G, Gc)
    rel_close(dx, want.dx, rel=R.POINT, what=f'cfs bwd {case}: dx')
    rel_close(dxp, want.dxproj, rel=R.POINT, what=f'cfs bwd {case}: dxproj')
    rel_close(dlogit, want.dlogit, rel=R.REDUCED, what=f'cfs bwd {case}: dlogit')
    assert dlogit.shape == lg.shape and not dlogit[:, G:].any(), 'dlogit behind the G logits is not zero'
    dx2, dxp2, dl2 = sentinel(n, G * Gc), sentinel(n, G * Gc), sentinel(n, G + R.CFS_EXTRA)
    check(L.somi_dcnv3_cfs_blend_bwd_f32(p(x), p(xp), p(lg), G + R.CFS_EXTRA, p(dout), p(dx2), p(dxp2), p(dl2), G + R.CFS_EXTRA, n, G, Gc, stream()),
          'cfs_blend_bwd')
    same_bits(dl2[:, :G], dlogit[:, :G], 'dlogit written into sentinel rows')
    untouched(dl2[:, G:], 'the columns of dlogit behind G')
    same_bits(dx2, dx, 'dx')
    same_bits(dxp2, dxp, 'dxproj')


# ------------------------------------------------------------------------------------------------------------------- detect decode
def run_decode(kind, l, na, nc, **kw):
    from somi_amd import ops
    d = dev()
    if kind == 'plain':
        ops.detect_plain_decode(l.t.to(d), l.anchors_px, l.stride, na, nc, **kw)
    else:
        ops.detect_decode(l.box.to(d), l.cls.to(d), l.anchors_px, l.stride, na, nc, **kw)


@pytest.mark.parametrize('case', R.DETECT_CASES, ids=R.ident)
@pytest.mark.parametrize('kind', ['plain', 'decoupled'])
def test_detect_decode_and_raw_backward(kind, case):
    """Detect on t / DecoupledDetect on box and cls, inputs wider than the used columns: raw alone, z alone and both, every level of the case into
    one z at its row offset (the rows around them untouched), against the oracle head in float64; the raw backward is the exact adjoint of raw."""
    from somi_amd import ops
    d = dev()
    B, na, nc, _ = case
    no = nc + 5
    lv = R.detect_inputs(case)
    want = R.detect_ref(kind, case, lv, F64)
    rows = [na * l.ny * l.nx for l in lv]
    lo = R.DETECT_PAD.rows_before
    total = lo + sum(rows) + R.DETECT_PAD.rows_after
    for mode in ('raw', 'z', 'both'):
        z = sentinel(B, total, no) if mode != 'raw' else None
        off = lo
        for i, l in enumerate(lv):
            raw = sentinel(B, na, l.ny, l.nx, no) if mode != 'z' else None
            run_decode(kind, l, na, nc, raw=raw, z=z, total=total if z is not None else 0, row_off=off if z is not None else 0)
            off += rows[i]
            if raw is not None:
                assert torch.equal(raw.cpu().double(), want.raw[i]), f'{kind} {case} {mode}: raw of level {i}'
        if z is not None:
            for name, cols in R.Z_GROUPS:
                rel_close(z[:, lo:lo + sum(rows), cols], want.z[..., cols], rel=R.POINT, what=f'{kind} {case} {mode}: z {name}')
            untouched(z[:, :lo], 'the rows of z in front of the levels')
            untouched(z[:, lo + sum(rows):], 'the rows of z behind the levels')
    for i, l in enumerate(lv):
        draw = l.draw.to(d)
        if kind == 'plain':
            got = (ops.detect_plain_raw_backward(draw, l.t.shape[3], na, nc),)
        else:
            got = ops.detect_raw_backward(draw, l.box.shape[3], l.cls.shape[3], na, nc)
        for a, b in zip(got, want.grads[i]):
            assert a.shape == b.shape and torch.equal(a.cpu().double(), b), f'{kind} {case}: the raw backward of level {i} is not the adjoint of raw'


@pytest.mark.parametrize('kind', ['plain', 'decoupled'])
def test_detect_decode_refuses_nine_anchors_and_rows_past_the_end(kind):
    d = dev()
    B, ny, nx, nc = 1, 2, 3, 2
    g = torch.Generator().manual_seed(9)

    def level(na):
        return R.NS(t=torch.randn(B, ny, nx, na * (nc + 5), generator=g), box=torch.randn(B, ny, nx, na * 5, generator=g),
                    cls=torch.randn(B, ny, nx, na * nc, generator=g), anchors_px=[float(v + 4) for v in range(2 * na)], stride=8.0)
    with pytest.raises(RuntimeError, match='na <= 8'):
        run_decode(kind, level(9), 9, nc, raw=sentinel(B, 9, ny, nx, nc + 5))
    n = 3 * ny * nx
    z = sentinel(B, n + 1, nc + 5)
    with pytest.raises(RuntimeError, match='rows out of range'):
        run_decode(kind, level(3), 3, nc, z=z, total=n + 1, row_off=2)
    with pytest.raises(RuntimeError, match='rows out of range'):
        run_decode(kind, level(3), 3, nc, z=z, total=n + 1, row_off=-1)
    torch.cuda.synchronize()
    untouched(z, 'z after the refusals')
    run_decode(kind, level(3), 3, nc, z=z, total=n + 1, row_off=1)                       # the last rows that fit
    assert torch.isfinite(z[:, 1:]).all()
    untouched(z[:, :1], 'the row of z in front')


# ------------------------------------------------------------------------------------------------------------------- TTA resample / resize / descale
def check_resampled(got, want32, want64, hs, ws, ch, pad, what):
    bar = R.resample_bar(want32, want64)
    print(f'{what}: float32 F.interpolate on the CPU is off by {R.rel_err(want32, want64):.3e} -> bar {bar:.3e}')
    rel_close(got, want64, rel=bar, what=what)
    g = got.cpu()
    assert not g[..., ch:].any(), f'{what}: the channels behind {ch} are not zero'
    padv = torch.tensor(pad, dtype=torch.float32)
    assert (g[:, hs:, :, :ch] == padv).all() and (g[:, :, ws:, :ch] == padv).all(), f'{what}: the padded region is not exactly {pad}'


@pytest.mark.parametrize('case', R.TTA_CASES, ids=R.ident)
def test_tta_resample(case):
    """scale_img after the optional flip: bilinear resize to int(size * ratio), 0.447 up to the next multiple of gs (none at ratio 1)."""
    from somi_amd import ops
    B, ch, H, W, ratio, gs, flip = case
    c = R.image_inputs(case)
    (w32, _), (w64, (hs, ws)) = R.tta_want(c, case, torch.float32), R.tta_want(c, case, F64)
    got = ops.tta_resample(c.x4.to(dev()), ratio, gs, flip, channels=ch, pad=R.TTA_PAD)
    check_resampled(got, w32, w64, hs, ws, ch, R.TTA_PAD, f'tta_resample {case}')
    if ratio == 1.0:
        assert torch.equal(got.cpu()[..., :ch], nhwc(c.img.flip(3) if flip else c.img)), 'ratio 1 is a copy (mirrored under the flip)'


@pytest.mark.parametrize('case', R.RESIZE_CASES, ids=R.ident)
def test_resize_bilinear_nhwc4(case):
    """F.interpolate(size=..., mode='bilinear', align_corners=False): up, down and mixed."""
    from somi_amd import ops
    B, ch, H, W, Hn, Wn = case
    c = R.image_inputs(case)
    got = ops.resize_bilinear_nhwc4(c.x4.to(dev()), Hn, Wn, channels=ch)
    check_resampled(got, R.resize_want(c, case, torch.float32), R.resize_want(c, case, F64), Hn, Wn, ch, 0.0, f'resize {case}')


@pytest.mark.parametrize('case', R.DESCALE_CASES, ids=R.ident)
def test_tta_descale(case):
    """_descale_pred in place: columns 0..3 against float64, every column from 4 on bit-unchanged."""
    from somi_amd import ops
    B, n, no, scale, flip, img_w = case
    z0 = R.descale_inputs(case)
    z = z0.to(dev())
    assert ops.tta_descale_(z, scale, flip, img_w) is z
    rel_close(z[..., :4], R.descale_pred(z0.double(), scale, flip, img_w)[..., :4], rel=R.DESCALE, what=f'tta_descale {case}')
    if no > 4:
        same_bits(z[..., 4:], z0[..., 4:], 'the columns of z from 4 on')


# ------------------------------------------------------------------------------------------------------------------- image ingest
@pytest.mark.parametrize('case', R.INGEST_CASES, ids=R.ident)
def test_image_ingest_beyond_the_grid_cap(case):
    from somi_amd import ops
    d = dev()
    B, ch, H, W = case
    g = R.gen('ingest', case)
    img = torch.randint(0, 256, case, generator=g, dtype=torch.uint8)
    want = torch.zeros(B, H, W, 4)
    want[..., :ch] = nhwc(img.float() / 255)
    assert torch.equal(ops.image_to_nhwc4(img.to(d)).cpu(), want), 'uint8 ingest'
    f = torch.rand(case, generator=g)
    for scale in (1.0, 0.5):
        want[..., :ch] = nhwc(f * scale)
        assert torch.equal(ops.image_to_nhwc4(f.to(d), scale=scale).cpu(), want), f'float ingest, scale {scale}'
