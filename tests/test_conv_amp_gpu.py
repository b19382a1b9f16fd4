"""The opt-in reduced-precision forms of the dense conv kernels (somi_conv_desc.prec, ops.CONV_PREC: bf16 and bf16x3; forward, data gradient,
weight gradient) against their operand-rounding model (tests/conv_amp_ref.py): operands rounded as the LDS staging rounds them, the product in
fp64.  A kernel differs from that model only by its fp32 accumulation, so the bars are the project's fp32 bars - POINT (1e-5 of max |want|) for
forward and data gradient, REDUCED (2e-5) for the weight gradient - some 200 x below what test_conv_reduced_precision_forms asks of bf16, and
for bf16x3 a quarter of the model's own distance from the exact result, which the exact fp32 kernel (1 x that distance) and a split with a
wrong low part (6 x) both miss.

Every launch is taken under ops.PROFILE, which records the kernel name the library's own planner reports: each test asserts the tile it claims,
and a bf16 form exists for the 8-wave tiles only (forward / data gradient 128 x 128 and 128 x 64, weight gradient 128 | 64 x 128 with shared
weights).  Every other launch computes exact fp32 whatever `prec` asks for, which test_launches_without_a_bf16_form_are_exact_fp32 pins bit for
bit.

Measured on one MI355X, the worst launch of this file per product (distance to the model over max |model|, its ratio to the bar; bf16x3 also as
a fraction of d3, the model's own distance from the exact result, which the rule holds to 0.25):

    bf16    forward 3.5e-7 (0.035 x POINT, case P2)    dgrad 4.2e-7 (0.042 x POINT, C2)    wgrad 2.2e-7 (0.011 x REDUCED, W)
    bf16x3  forward 7.6e-7 (0.076 x, 0.16 d3, P2)      dgrad 6.2e-7 (0.062 x, 0.15 d3, A without workspace)
            wgrad 4.1e-7 (0.020 x, 0.094 d3, T)

The bf16x3 results lie 4.0e-6 ... 6.1e-6 from the exact product (d3: 4.1e-6 ... 6.1e-6), the bf16 model 2.1e-3 ... 3.3e-3.  With a library
whose conversions truncate instead of rounding, bf16 lies 6.6e-3 ... 9.1e-3 from its model (360 ... 910 x the bar) and bf16x3 2.5e-5 ... 3.5e-5
(1.4 ... 3.5 x the bar, 5.6 ... 7.5 x d3): 50 of the 80 tests here fail (the other 30 are the exact-fp32 contracts and the bf16x3 blocks), while
test_conv_reduced_precision_forms passes.
"""
import math
from types import SimpleNamespace as NS

import pytest
import torch

import conv_amp_ref as R
from parity import check_built_block, rel_close
from slices import In, Out, check_slice_op
from support_kernels_ref import POINT, REDUCED

pytestmark = pytest.mark.gpu

PRECS = ('bf16', 'bf16x3')
BAR = {'forward': POINT, 'dgrad': POINT, 'wgrad': REDUCED}
NO_WS = 'no_ws'

# The tile every launch of a case plans: with the stream-K workspace (ops attaches it to every forward and stride-1 data gradient), and, for the
# cases the schedule test runs, without it.  conv_igemm_f32_kernel<BM,BN,WAVES_M,WAVES_N,...> / conv_wgrad_f32_kernel<BM,BN,waves>.
TILES = {
    'A': dict(forward='128,128,2,4', dgrad='128,64,4,2', wgrad='128,128,8'),
    'B': dict(forward='128,64,4,2', dgrad='128,128,2,4', wgrad='64,128,8'),
    'C': dict(forward='128,128,2,4', dgrad='64,128,1,4', wgrad='128,128,8'),
    'C2': dict(forward='128,128,2,4', dgrad='128,64,4,2', wgrad='128,128,8'),
    'D': dict(forward='128,128,2,4', dgrad='128,128,2,4', wgrad='64,128,8'),
    'E': dict(forward='128,64,4,2', dgrad='128,32,4,1', wgrad='64,128,8'),
    'G': dict(forward='128,128,2,4', dgrad='128,64,4,2', wgrad='128,128,8'),
    'S': dict(forward='128,128,2,4', dgrad='128,128,2,4', wgrad='128,128,8'),
    'T': dict(forward='128,64,4,2', dgrad='128,64,4,2', wgrad='64,128,8'),
    'U': dict(forward='128,128,2,4'),
    'P': dict(forward='64,128,1,4', dgrad='128,64,4,2', wgrad='128,128,8'),
    'P2': dict(forward='128,64,4,2', dgrad='128,64,4,2', wgrad='64,128,8'),
    'W': dict(forward='64,128,1,4', dgrad='128,32,4,1', wgrad='128,128,8'),
    (NO_WS, 'A'): dict(forward='64,128,1,4', dgrad='128,64,4,2'),
    (NO_WS, 'S'): dict(forward='64,128,1,4', dgrad='64,128,1,4'),
    (NO_WS, 'T'): dict(forward='128,64,4,2', dgrad='128,64,4,2'),
    (NO_WS, 'U'): dict(forward='128,128,2,4'),
}
EIGHT_WAVES = ('128,128,2,4', '128,64,4,2')


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def has_bf16_form(which, name, per_sample=False):
    """The rule the launchers follow (launch() in conv_igemm.hip, somi_conv2d_wgrad_nhwc_f32), on a kernel name."""
    if which == 'wgrad':
        return name.startswith('conv_wgrad_f32_kernel<') and name.endswith(',128,8>') and not per_sample
    return any(name == f'conv_igemm_f32_kernel<{t},false,true>' for t in EIGHT_WAVES)


def packed(which, t, geom):
    """A product of conv_amp_ref in the layout its kernel writes."""
    from somi_amd.pack import pack_conv_weight
    return pack_conv_weight(t, cin_pad=geom[3]) if which == 'wgrad' else R.nhwc(t)


_DEV = {}


def device_inputs(name, tied=False):
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    if (name, tied) not in _DEV:
        inp, d = R.inputs(name, tied), dev()
        Cin, Cout = inp.geom[3], inp.geom[4]
        wt = (torch.stack([pack_dgrad_weight(w, cin_pad=Cin, cout_pad=Cout) for w in inp.w]) if inp.per_sample
              else pack_dgrad_weight(inp.w, cin_pad=Cin, cout_pad=Cout))
        _DEV[name, tied] = NS(geom=inp.geom, per_sample=inp.per_sample, x=R.nhwc(inp.x).to(d), dy=R.nhwc(inp.dy).to(d),
                              wp=pack_conv_weight(inp.w, cin_pad=Cin).to(d), wt=wt.to(d))
    return _DEV[name, tied]


def launch(which, di, **kw):
    from somi_amd import ops
    B, H, W, Cin, Cout, k, s, p, dil = di.geom
    conv = dict(kh=k, kw=k, stride=s, pad=p, dil=dil, per_sample_w=di.per_sample)
    if which == 'forward':
        return ops.conv2d_nhwc(di.x, di.wp, kw.pop('bias', None), **conv, **kw)
    if which == 'dgrad':
        return ops.conv2d_dgrad_nhwc(di.dy, di.wt, B=B, H=H, W=W, cin=Cin, **conv, **kw)
    return ops.conv2d_wgrad_nhwc(di.x, di.dy, **conv, **kw)


def traced(monkeypatch, prec, fn, workspace=True):
    """fn() under CONV_PREC = prec, optionally without the stream-K workspace -> (its result, the kernel names of its conv launches)."""
    from somi_amd import ops
    with monkeypatch.context() as mp:
        log = []
        mp.setattr(ops, 'CONV_PREC', ops.PREC[prec])
        mp.setattr(ops, 'PROFILE', log)
        if not workspace:
            mp.setattr(ops, '_conv_workspace', lambda d, dev: None)
        out = fn()
        torch.cuda.synchronize()
    assert ops.CONV_PREC == 0 and ops.PROFILE is None
    return out, [e[0] for e in log]


def run(monkeypatch, which, di, prec, workspace=True, **kw):
    out, names = traced(monkeypatch, prec, lambda: launch(which, di, **kw), workspace)
    assert len(names) == 1, names
    return out, names[0]


def kernel_name(which, tile, fast=True):
    return f'conv_wgrad_f32_kernel<{tile}>' if which == 'wgrad' else f'conv_igemm_f32_kernel<{tile},false,{"true" if fast else "false"}>'


def against_model(got, m, which, prec, what):
    """The bar of the product against the model of `prec`; bf16x3: the quarter rule as well.  Prints both figures.  -> (distance to the model,
    its ratio to the bar, distance / d3 or None)."""
    got = got.detach().cpu()
    err = R.rel_err(got, m[prec])
    line = f'{what}: {err:.3e} from the {prec} model = {err / BAR[which]:.3f} x the bar {BAR[which]:.0e}'
    frac = None
    if prec == 'bf16x3':
        scale = m['bf16x3'].abs().max().item()
        d3 = (m['exact'] - m['bf16x3']).abs().max().item() / scale
        frac = err / d3
        line += f'; {R.rel_err(got, m["exact"]):.3e} from exact; d3 {d3:.3e}, err / d3 {frac:.3f} (rule: 0.25)'
    print(line)
    rel_close(got, m[prec], rel=BAR[which], what=what)
    if prec == 'bf16x3':
        assert frac <= 0.25, f'{what}: {err:.3e} from the bf16x3 model, more than a quarter of the model\'s {d3:.3e} from the exact result'
    return err, err / BAR[which], frac


def layouts(name, tied=False):
    """The models of a case in the kernels' layouts (computed once)."""
    key = ('layout', name, tied)
    if key not in _DEV:
        inp, m = R.case(name, tied)
        _DEV[key] = {which: {mode: packed(which, t, inp.geom) for mode, t in modes.items()} for which, modes in m.items()}
    return _DEV[key]


CASE_PREC = [(n, p) for n in R.CASES for p in PRECS]


# ------------------------------------------------------------------------------------------------------------------------ 1. - 4.
@pytest.mark.parametrize('name,prec', CASE_PREC, ids=[f'{n}-{p}' for n, p in CASE_PREC])
def test_reduced_products_match_their_model(monkeypatch, name, prec):
    """Every product of the case that has a bf16 form: the planned tile (by name); the bar against the model (and the quarter rule, bf16x3); not
    bit-identical to the exact fp32 launch (the bf16 form ran); two launches bit-identical.
    Measured over the cases, distance to the model: bf16 forward 1.4e-7 ... 3.5e-7, dgrad 9.1e-8 ... 4.2e-7, wgrad 1.3e-7 ... 2.2e-7;
    bf16x3 forward 2.4e-7 ... 7.6e-7 (0.05 ... 0.16 of d3), dgrad 1.4e-7 ... 5.7e-7 (0.02 ... 0.13), wgrad 2.0e-7 ... 4.1e-7 (0.04 ... 0.09)."""
    di, want = device_inputs(name), layouts(name)
    for which in R.CASES[name].reduced:
        what = f'{name} {prec} {which}'
        got, kname = run(monkeypatch, which, di, prec)
        assert kname == kernel_name(which, TILES[name][which]), f'{what}: the planner chose {kname}'
        assert has_bf16_form(which, kname, di.per_sample), f'{what}: {kname} has no bf16 form'
        against_model(got, want[which], which, prec, what)
        exact, _ = run(monkeypatch, which, di, None)
        assert not torch.equal(got, exact), f'{what}: bit-identical to the fp32 launch - the reduced-precision kernel did not run'
        again, _ = run(monkeypatch, which, di, prec)
        assert torch.equal(got, again), f'{what}: two launches differ'


# ------------------------------------------------------------------------------------------------------------------------ 5. schedules
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name,which', [('A', 'dgrad'), ('T', 'forward'), ('T', 'dgrad'), ('U', 'forward')], ids=lambda v: v)
def test_both_schedules_match_the_model(monkeypatch, name, which, prec):
    """Stream-K (with the workspace: cut tiles are finished by the fp32 fix-up kernel) and one workgroup per tile (without it) run the same bf16
    form of the same tile: both against the model, and not bit-identical (stream-K was taken)."""
    di, want = device_inputs(name), layouts(name)
    sk, n1 = run(monkeypatch, which, di, prec)
    plain, n0 = run(monkeypatch, which, di, prec, workspace=False)
    assert n1 == kernel_name(which, TILES[name][which]) and n0 == kernel_name(which, TILES[NO_WS, name][which]), (n1, n0)
    assert has_bf16_form(which, n0) and has_bf16_form(which, n1)
    against_model(sk, want[which], which, prec, f'{name} {prec} {which} stream-K')
    against_model(plain, want[which], which, prec, f'{name} {prec} {which} one workgroup per tile')
    assert not torch.equal(sk, plain), f'{name} {which}: the stream-K schedule was not taken for a shape it is meant for'
    fp32, _ = run(monkeypatch, which, di, None, workspace=False)
    assert not torch.equal(plain, fp32), f'{name} {prec} {which}: the workspace-less launch is bit-identical to fp32'


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('name,which', [('A', 'forward'), ('S', 'forward'), ('S', 'dgrad')], ids=lambda v: v)
def test_workspace_less_small_launches_plan_a_tile_without_a_bf16_form(monkeypatch, name, which, prec):
    """Without the workspace a small forward / data gradient of more than 64 output channels takes the 4-wave 64 x 128 tile to fill the chip:
    exact fp32 whatever `prec` asks for."""
    di = device_inputs(name)
    got, kname = run(monkeypatch, which, di, prec, workspace=False)
    assert kname == kernel_name(which, TILES[NO_WS, name][which]) and not has_bf16_form(which, kname), kname
    fp32, _ = run(monkeypatch, which, di, None, workspace=False)
    assert torch.equal(got, fp32), f'{name} {prec} {which} without the workspace: not the fp32 launch\'s bits'


# ------------------------------------------------------------------------------------------------------------------------ 6. ties
@pytest.mark.parametrize('prec', PRECS)
def test_operands_at_exact_ties_round_to_even(monkeypatch, prec):
    """Case A with x and dy built from values half-way between two bf16 neighbours (test_conv_amp_host.py shows that ties-to-even differs there
    from truncation and from round-half-up on half of the elements each, by a whole bf16 ulp of the operand): a conversion that is not
    round-to-nearest-even lies ~1e-3 of the range from the model, which random data cannot show."""
    di, want = device_inputs('A', tied=True), layouts('A', tied=True)
    for which in R.PRODUCTS:
        got, kname = run(monkeypatch, which, di, prec)
        assert kname == kernel_name(which, TILES['A'][which])
        against_model(got, want[which], which, prec, f'A at ties {prec} {which}')


# ------------------------------------------------------------------------------------------------------------------------ 7. epilogue
@pytest.mark.parametrize('prec', PRECS)
def test_epilogue_terms_stay_fp32(monkeypatch, prec):
    """Case A's forward with bias + SiLU + residual and case D's data gradient with accumulate + accumulate2, against the model pushed through
    the same terms in fp64, at POINT."""
    d = dev()
    inp, m = R.case('A')
    want = R.nhwc(R.forward_epilogue(m['forward'][prec], inp.bias, inp.res))
    got, _ = run(monkeypatch, 'forward', device_inputs('A'), prec, bias=inp.bias.to(d), act='silu', residual=R.nhwc(inp.res).to(d))
    rel_close(got, want, rel=POINT, what=f'A {prec} forward + bias + SiLU + residual')
    inp, m = R.case('D')
    want = R.nhwc(R.dgrad_epilogue(m['dgrad'][prec], inp.acc, inp.acc2))
    got, _ = run(monkeypatch, 'dgrad', device_inputs('D'), prec, accumulate=R.nhwc(inp.acc).to(d), accumulate2=R.nhwc(inp.acc2).to(d))
    rel_close(got, want, rel=POINT, what=f'D {prec} dgrad + accumulate + accumulate2')


# ------------------------------------------------------------------------------------------------------------------------ the fallbacks
def _random_layer(geom, per_sample=False):
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    B, H, W, Cin, Cout, k, s, p, dil = geom
    g, d = R._gen('fallback', geom), dev()
    Ho, Wo = R.out_size(H, k, s, p, dil), R.out_size(W, k, s, p, dil)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    return NS(geom=geom, per_sample=False, x=torch.randn(B, H, W, Cin, generator=g).to(d), dy=torch.randn(B, Ho, Wo, Cout, generator=g).to(d),
              wp=pack_conv_weight(w, cin_pad=Cin).to(d), wt=pack_dgrad_weight(w, cin_pad=Cin, cout_pad=Cout).to(d),
              ca=(torch.rand(B, Cin, generator=g) + 0.5).to(d), sa=(torch.rand(B, H, W, generator=g) + 0.5).to(d))


NARROW = (2, 9, 9, 64, 32, 3, 1, 1, 1)            # Cout <= 32: the 4-wave 128 x 32 tile
SHORT_K = (2, 9, 9, 64, 128, 1, 1, 0, 1)          # wgrad with K = 64: a 64-column tile
FALLBACKS = [(name, which, {}) for name, c in R.CASES.items() for which in c.fallback] + [
    (NARROW, 'forward', {}), (SHORT_K, 'wgrad', {}), (R.CASES['A'].shape, 'forward', {'modulated': True})]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('case,which,extra', FALLBACKS, ids=[f'{c if isinstance(c, str) else "x".join(map(str, c))}-{w}{"-modulated" if e else ""}'
                                                              for c, w, e in FALLBACKS])
def test_launches_without_a_bf16_form_are_exact_fp32(monkeypatch, case, which, extra, prec):
    """The fallback contract of somi_conv_desc.prec, bit for bit: a forward / data gradient that plans a 4-wave tile (64 x 128: small launches
    without stream-K, among them the stride-2 data gradient of case C and the per-sample forward of case P; 128 x 32: Cout <= 32, the data
    gradients of cases E and W), a forward with Cin % 32 != 0 (case W), a modulated forward, a weight gradient with K <= 64 or per-sample
    weights (cases P, P2) give the bits of prec = 0.  (The patch conv: test_patch_conv_reduced_precision_requests_run_fp32.)"""
    di = device_inputs(case) if isinstance(case, str) else _random_layer(case)
    kw = dict(a_chan_scale=di.ca, a_pix_scale=di.sa) if extra else {}
    got, kname = run(monkeypatch, which, di, prec, **kw)
    if isinstance(case, str):
        fast = not (case == 'W' and which == 'forward')
        assert kname == kernel_name(which, TILES[case][which], fast), kname
    elif extra:
        assert kname == 'conv_igemm_f32_kernel<128,128,2,4,true,true>', kname
    else:
        assert kname == {NARROW: 'conv_igemm_f32_kernel<128,32,4,1,false,true>', SHORT_K: 'conv_wgrad_f32_kernel<128,64,4>'}[case], kname
    assert not has_bf16_form(which, kname, di.per_sample), f'{kname} has a bf16 form'
    fp32, _ = run(monkeypatch, which, di, None, **kw)
    assert torch.isfinite(got).all() and got.abs().max() > 0
    assert torch.equal(got, fp32), f'{case} {prec} {which}: differs from the fp32 launch in {int((got != fp32).sum())} values'


@pytest.mark.parametrize('prec', PRECS)
def test_grouped_conv_ignores_the_precision_switch(monkeypatch, prec):
    """gconv2d_nhwc and its two gradients are fp32 always (the comment above ops.gconv2d_nhwc)."""
    from somi_amd import ops
    from somi_amd.pack import pack_gconv_weight
    B, H, W, c1, c2, groups, k = 2, 9, 11, 64, 96, 4, 3
    g, d = R._gen('gconv'), dev()
    x, dy = torch.randn(B, H, W, c1, generator=g).to(d), torch.randn(B, H, W, c2, generator=g).to(d)
    w = pack_gconv_weight(torch.randn(c2, c1 // groups, k, k, generator=g) / math.sqrt(c1 // groups * k * k)).to(d)

    def three():
        kw = dict(c1=c1, c2=c2, groups=groups, k=k)
        return (ops.gconv2d_nhwc(x, w, None, **kw), ops.gconv2d_dgrad_nhwc(dy, w, H=H, W=W, **kw), ops.gconv2d_wgrad_nhwc(x, dy, **kw))
    got, _ = traced(monkeypatch, prec, three)
    fp32, _ = traced(monkeypatch, None, three)
    for a, b, what in zip(got, fp32, R.PRODUCTS):
        assert a.abs().max() > 0 and torch.equal(a, b), f'grouped conv {what} under {prec}: not the fp32 bits'


# ------------------------------------------------------------------------------------------------------------------------ slices
X_COFF, Y_COFF, DY_COFF, DX_COFF, DW_PAD = 32, 16, 8, 12, 40


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('form', ['forward', 'dgrad', 'dgrad_accumulate', 'dgrad_stride2', 'wgrad'])
def test_slice_contract_under_reduced_precision(monkeypatch, form, prec):
    """The channel-slice contract (tests/slices.py) on the staging path of the bf16 forms: case A's forward, data gradient (written, and
    accumulated in place) and weight gradient, and the stride-2 data gradient of case C2, with every operand at a non-zero channel offset
    inside a wider tensor, under random and NaN neighbours, against the model at the bars of the kernel tests."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight, pack_dgrad_weight
    name = 'C2' if form == 'dgrad_stride2' else 'A'
    which = form.split('_')[0]
    inp, m = R.case(name)
    B, H, W, Cin, Cout, k, s, p, dil = inp.geom
    want = layouts(name)[which][prec]
    conv = dict(kh=k, kw=k, stride=s, pad=p, dil=dil)
    bars = {'rel': BAR[which]}
    if which == 'forward':
        ins = {'x': In(R.nhwc(inp.x), Cin + 64, X_COFF), 'w': pack_conv_weight(inp.w, cin_pad=Cin)}
        outs = {'y': Out((B, inp.Ho, inp.Wo), Cout + 48, Y_COFF, Cout)}
        call = lambda b: ops.conv2d_nhwc(b['x'], b['w'], None, cin=Cin, x_coff=X_COFF, out=b['y'], cout=Cout, y_coff=Y_COFF, **conv)   # noqa: E731
        refs = {'y': want}
    elif which == 'dgrad':
        acc = form == 'dgrad_accumulate'
        ins = {'dy': In(R.nhwc(inp.dy), Cout + 24, DY_COFF), 'wt': pack_dgrad_weight(inp.w, cin_pad=Cin, cout_pad=Cout)}
        outs = {'dx': Out((B, H, W), Cin + 20, DX_COFF, Cin, prev=R.nhwc(inp.acc) if acc else None, accumulate=acc)}
        call = lambda b: ops.conv2d_dgrad_nhwc(b['dy'], b['wt'], B=B, H=H, W=W, cin=Cin, cout=Cout, dy_coff=DY_COFF, out=b['dx'],   # noqa: E731
                                               dx_coff=DX_COFF, accumulate=b['dx'] if acc else None, acc_coff=DX_COFF, **conv)
        refs = {'dx': want}
    else:
        n = want.numel()
        ins = {'x': In(R.nhwc(inp.x), Cin + 64, X_COFF), 'dy': In(R.nhwc(inp.dy), Cout + 28, DY_COFF)}
        outs = {'dw': Out((1,), n + 2 * DW_PAD, DW_PAD, n)}
        call = lambda b: ops.conv2d_wgrad_nhwc(b['x'], b['dy'], cin=Cin, x_coff=X_COFF, cout=Cout, dy_coff=DY_COFF,                  # noqa: E731
                                               out=b['dw'][0, DW_PAD:DW_PAD + n].view(want.shape), **conv)
        refs = {'dw': want.reshape(1, n)}
    names = []

    def op(b):
        names.extend(traced(monkeypatch, prec, lambda: call(b))[1])
    check_slice_op(op, ins, outs, refs, bars={k_: bars for k_ in refs}, what=f'{name} {prec} {form}')
    assert names == [kernel_name(which, TILES[name][which])] * 3, names


# ------------------------------------------------------------------------------------------------------------------------ one block
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('block', ['Conv', 'Bottleneck'])
def test_block_trains_on_the_model_of_its_convs(monkeypatch, block, prec):
    """Conv(128, 128, 3, 1) and Bottleneck(128, 128) at (2, 128, 12, 10), training forward and backward under CONV_PREC, by the block procedure
    (1e-3; atol 2e-5 on gradients) against the CPU reference whose nn.Conv2d products are the model's (conv_amp_ref.AmpConv2d): under plain
    bf16 more than two orders below the band test_amp_training_step_stays_in_its_band holds a graph to.  Every conv of the two blocks runs all
    three products in a bf16 form (asserted from the kernel names)."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    make = {'Conv': lambda ns: ns.Conv(128, 128, 3, 1), 'Bottleneck': lambda ns: ns.Bottleneck(128, 128)}[block]
    ref, mine = make(OB), make(MB)
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    mine.load_state_dict(ref.state_dict())
    nconv = R.use_amp_convs(ref, prec)
    gen = torch.Generator().manual_seed(len(block))
    x = torch.randn(2, 128, 12, 10, generator=gen)
    _, names = traced(monkeypatch, prec, lambda: check_built_block(ref, mine, x, gen, f'{block} {prec}', eval_too=False))
    kinds = {'forward': [n for n in names if 'igemm' in n], 'wgrad': [n for n in names if 'wgrad' in n]}
    assert len(kinds['forward']) == 2 * nconv and len(kinds['wgrad']) == nconv, names          # forward + data gradient, weight gradient
    for which, ns in kinds.items():
        for n in ns:
            assert has_bf16_form(which, n), f'{block}: {n} has no bf16 form'
