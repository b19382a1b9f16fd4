"""tests/support_kernels_ref.py held to the oracle (float64, 1e-12), the condition on the inputs of tests/test_support_kernels_gpu.py - for every
case of that file the reference evaluated in float32 on the CPU stays within half the kernels' bar, so the inputs themselves leave the kernels
room - and the guard that keeps every public function of somi_amd/ops.py named in a GPU test file.  CPU only."""
import ast
import glob
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

import support_kernels_ref as R
from parity import rel_close

HERE = os.path.dirname(os.path.abspath(__file__))


def close12(got, want, what):
    rel_close(got, want, rel=1e-12, what=what, atol=1e-14)


def half(got32, want64, bar, what):
    assert got32.dtype == torch.float32 and want64.dtype == torch.float64, what
    rel_close(got32, want64, rel=bar / 2, what=f'{what}: float32 on the CPU against float64, half the bar')


# ------------------------------------------------------------------------------------------------------------------- restatements
def test_scale_img_and_descale_pred_equal_the_oracles_augmented_forward():
    """Model._forward_augment (the oracle's TTA) on a stand-in whose single-scale forward records its input and returns given predictions: the six
    inputs are scale_img at ratios 1 / 0.83 / 0.67 with and without the flip, the six outputs descale_pred of the predictions (the first pass loses
    its last n // 5 rows and the last its first 4 * (n // 5) with two levels: the rest is compared)."""
    from oracle.somi_ref.model import Model
    g = torch.Generator().manual_seed(7)
    H, W, gs, n, no = 70, 50, 32, 23, 9
    x = torch.rand(2, 3, H, W, generator=g, dtype=torch.float64)
    preds = [torch.rand(2, n, no, generator=g, dtype=torch.float64) * 100 for _ in range(6)]
    seen, feed = [], iter(preds)

    def forward_once(xi):
        seen.append(xi)
        return (next(feed),)
    y, _ = Model._forward_augment(NS(stride=torch.tensor([8.0, float(gs)]), model=[NS(nl=2)], _forward_once=forward_once), x)
    combos = [(1.0, 0), (1.0, 1), (0.83, 0), (0.83, 1), (0.67, 0), (0.67, 1)]
    assert len(seen) == 6
    want = []
    for i, ((ratio, flip), xi, p) in enumerate(zip(combos, seen, preds)):
        mine = R.scale_img(x, ratio, gs, flip)
        close12(mine, xi, f'scale_img ratio {ratio} flip {flip}')
        d = R.descale_pred(p, ratio, flip, float(W))
        want.append(d[:, :n - n // 5] if i == 0 else d[:, (n // 5) * 4:] if i == 5 else d)
    close12(torch.cat(want, 1), y, 'descale_pred of the six passes')
    assert seen[2].shape[2:] == (64, 64) and (seen[2][:, :, 58:] == 0.447).all() and (seen[2][:, :, :, 41:] == 0.447).all()


@pytest.mark.parametrize('case', R.DETECT_CASES, ids=R.ident)
@pytest.mark.parametrize('kind', ['plain', 'decoupled'])
def test_detect_reference_equals_the_decode_formulas(kind, case):
    """The oracle heads with their convs taken out (detect_ref: what the GPU tests compare with) against the decode written out by hand on the NHWC
    inputs the kernels read: raw is the same permutation, z the same rows level after level, the raw backward the inverse permutation with zero in
    the columns behind the used ones."""
    B, na, nc, _ = case
    lv = R.detect_inputs(case)
    ref = R.detect_ref(kind, case, lv, torch.float64)
    zs = []
    for i, l in enumerate(lv):
        if kind == 'plain':
            raw, z = R.decode_plain(l.t.double(), l.anchors_px, l.stride, na, nc)
        else:
            raw, z = R.decode_decoupled(l.box.double(), l.cls.double(), l.anchors_px, l.stride, na, nc)
        assert torch.equal(raw, ref.raw[i]), f'raw of level {i}'
        zs.append(z)
        d = l.draw.double().permute(0, 2, 3, 1, 4)                                          # B, ny, nx, na, no
        if kind == 'plain':
            want = (torch.nn.functional.pad(d.reshape(B, l.ny, l.nx, -1), (0, R.DETECT_PAD.t)),)
        else:
            want = (torch.nn.functional.pad(d[..., :5].reshape(B, l.ny, l.nx, -1), (0, R.DETECT_PAD.box)),
                    torch.nn.functional.pad(d[..., 5:].reshape(B, l.ny, l.nx, -1), (0, R.DETECT_PAD.cls)))
        for a, b in zip(ref.grads[i], want):
            assert torch.equal(a, b), f'raw backward of level {i}'
    close12(torch.cat(zs, 1), ref.z, f'{kind} z')


# ------------------------------------------------------------------------------------------------------------------- the inputs leave room
@pytest.mark.parametrize('case', R.DW_BWD_CASES, ids=R.ident)
def test_dwconv_backward_inputs(case):
    c = R.dw_inputs(case)
    r32, r64 = R.dw_backward(c, torch.float32), R.dw_backward(c, torch.float64)
    half(r32.dx, r64.dx, R.POINT, f'dwconv dx {case}')
    half(r32.dx + R.nhwc(c.acc), r64.dx + R.nhwc(c.acc).double(), R.POINT, f'dwconv dx + accumulate {case}')
    half(r32.dw, r64.dw, R.REDUCED, f'dwconv dw {case}')
    half(r32.db, r64.db, R.REDUCED, f'dwconv dbias {case}')


def test_dwconv_backward_cases_reach_the_final_reduction_loops():
    chunks = [R.dw_chunks(c) for c in R.DW_BWD_CASES]
    assert any(16 < n <= 32 for n in chunks) and any(n > 32 for n in chunks) and R.dw_chunks((3, 256, 70, 45)) == 34, chunks
    assert (R.DW_BWD_REFUSED[1] // 4) and 256 % (R.DW_BWD_REFUSED[1] // 4) != 0


@pytest.mark.parametrize('case', R.DW_FWD_CASES, ids=R.ident)
def test_dwconv_forward_inputs(case):
    c = R.dw_inputs(case)
    half(R.dw_forward(c, torch.float32, case[4]), R.dw_forward(c, torch.float64, case[4]), R.POINT, f'dwconv forward {case}')


@pytest.mark.parametrize('case', R.LN_CASES, ids=R.ident)
def test_layernorm_gelu_backward_inputs(case):
    c = R.ln_inputs(case)
    u = c.u.double()
    assert (u.std(1, unbiased=False) >= 0.499).all() and (u.mean(1).abs() >= 0.29).all(), 'rows: standard deviation >= 0.5 around a non-zero mean'
    assert (c.gamma >= 0.5).all() and (c.gamma <= 3).all()
    r32, r64 = R.ln_backward(c, torch.float32), R.ln_backward(c, torch.float64)
    half(r32.du, r64.du, R.POINT, f'LN+GELU du {case}')
    half(r32.dgamma, r64.dgamma, R.REDUCED, f'LN+GELU dgamma {case}')
    half(r32.dbeta, r64.dbeta, R.REDUCED, f'LN+GELU dbeta {case}')


@pytest.mark.parametrize('case', R.BIFPN_CASES, ids=R.ident)
def test_bifpn_inputs(case):
    c = R.bifpn_inputs(case)
    assert min(R.BIFPN_W[len(case[0])]) < 0
    r32, r64 = R.bifpn_ref(c, case[0], torch.float32), R.bifpn_ref(c, case[0], torch.float64)
    half(r32.out, r64.out, R.POINT, f'bifpn {case}')
    for i, (a, b) in enumerate(zip(r32.dsrcs, r64.dsrcs)):
        half(a, b, R.POINT, f'bifpn dsrc {i} {case}')
    half(r32.dw, r64.dw, R.REDUCED, f'bifpn dw {case}')


@pytest.mark.parametrize('case', R.CFS_CASES, ids=R.ident)
def test_cfs_blend_inputs(case):
    c = R.cfs_inputs(case)
    assert c.logit[:, :case[1]].abs().max() > 7.5
    r32, r64 = R.cfs_ref(c, case[1], case[2], torch.float32), R.cfs_ref(c, case[1], case[2], torch.float64)
    for n, bar in (('out', R.POINT), ('dx', R.POINT), ('dxproj', R.POINT), ('dlogit', R.REDUCED)):
        half(getattr(r32, n), getattr(r64, n), bar, f'cfs {n} {case}')
    assert not r64.dlogit[:, case[1]:].any()


@pytest.mark.parametrize('case', R.DETECT_CASES, ids=R.ident)
@pytest.mark.parametrize('kind', ['plain', 'decoupled'])
def test_detect_inputs(kind, case):
    lv = R.detect_inputs(case)
    r32, r64 = R.detect_ref(kind, case, lv, torch.float32), R.detect_ref(kind, case, lv, torch.float64)
    for name, cols in R.Z_GROUPS:
        half(r32.z[..., cols], r64.z[..., cols], R.POINT, f'{kind} z {name} {case}')
    for a, b in zip(r32.raw, r64.raw):
        assert torch.equal(a.double(), b)
    for ga, gb in zip(r32.grads, r64.grads):
        for a, b in zip(ga, gb):
            assert torch.equal(a.double(), b)


@pytest.mark.parametrize('case', R.TTA_CASES, ids=R.ident)
def test_tta_resample_inputs(case):
    c = R.image_inputs(case)
    (w32, _), (w64, (hs, ws)) = R.tta_want(c, case, torch.float32), R.tta_want(c, case, torch.float64)
    bar = R.resample_bar(w32, w64)
    print(f'tta_resample {case}: float32 F.interpolate is off by {R.rel_err(w32, w64):.3e}, bar {bar:.3e}')
    assert bar < 1e-4, 'a bar this wide would pass a wrong weight'
    half(w32, w64, bar, f'tta_resample {case}')
    ch = case[1]
    assert (w64[:, hs:, :, :ch] == R.TTA_PAD).all() and (w64[:, :, ws:, :ch] == R.TTA_PAD).all() and not w64[..., ch:].any()


@pytest.mark.parametrize('case', R.RESIZE_CASES, ids=R.ident)
def test_resize_inputs(case):
    c = R.image_inputs(case)
    w32, w64 = R.resize_want(c, case, torch.float32), R.resize_want(c, case, torch.float64)
    bar = R.resample_bar(w32, w64)
    print(f'resize {case}: float32 F.interpolate is off by {R.rel_err(w32, w64):.3e}, bar {bar:.3e}')
    assert bar < 1e-4, 'a bar this wide would pass a wrong weight'
    half(w32, w64, bar, f'resize {case}')


@pytest.mark.parametrize('case', R.DESCALE_CASES, ids=R.ident)
def test_descale_inputs(case):
    z = R.descale_inputs(case)
    half(R.descale_pred(z, *case[3:]), R.descale_pred(z.double(), *case[3:]), R.DESCALE, f'descale {case}')


# ------------------------------------------------------------------------------------------------------------------- the guard
# Public functions of somi_amd/ops.py that no GPU test file has to name, each with its reason.  No kernel wrapper belongs here: a wrapper that
# launches a kernel gets a direct test instead.
NOT_NAMED_IN_A_GPU_TEST = {
    'conv_out_size': 'size helper: integer arithmetic on the host, no launch',
    'maxpool2_out_size': 'size helper: integer arithmetic on the host, no launch',
    'free_workspaces': 'drops the cached scratch tensors; launches nothing',
    'reset_dcn_overflow_taps': 'counter reset: zeroes the running far-tap totals with torch; no kernel of the library runs',
}


def public_ops():
    with open(os.path.join(HERE, '..', 'yolo-somi_amd', 'somi_amd', 'ops.py')) as f:
        tree = ast.parse(f.read())
    return [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and not n.name.startswith('_')]


def test_every_public_op_is_named_in_a_gpu_test_file():
    """`ops.NAME` (or `from somi_amd.ops import ... NAME`) appears in at least one tests/test_*_gpu.py for every public function of ops.py, apart
    from the table above: a new wrapper that only block or model tests reach fails here."""
    files = sorted(glob.glob(os.path.join(HERE, 'test_*_gpu.py')))
    assert len(files) > 10
    text = {}
    for p in files:
        with open(p) as f:
            text[os.path.basename(p)] = f.read()
    names = public_ops()
    assert len(names) > 80 and 'dwconv3x3_backward' in names and 'conv2d_nhwc' in names

    def named(n):
        return any(re.search(rf'\bops\.{n}\b', t) or re.search(rf'from somi_amd\.ops import[^\n]*\b{n}\b', t) for t in text.values())
    missing = [n for n in names if n not in NOT_NAMED_IN_A_GPU_TEST and not named(n)]
    assert not missing, f'public functions of somi_amd/ops.py that no tests/test_*_gpu.py names: {missing}'
    stale = [n for n in NOT_NAMED_IN_A_GPU_TEST if n not in names or named(n)]
    assert not stale, f'entries of the exemption table that are gone from ops.py or named by a GPU test by now: {stale}'
    assert all(len(r) > 10 for r in NOT_NAMED_IN_A_GPU_TEST.values())
