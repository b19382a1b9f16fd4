"""The CBAM C3 family on the MI355X (C3_CBAM, C3_CBAMS, C3_CBAM_DWC, C3_CBAMS_DWC, C3_SCBAM, C3CBAM and their bottlenecks; cbam_c3.hip): the
gate-combine pass and its two backward passes and the depthwise-separable gate against an fp64 restatement, the blocks against torch autograd on the CPU restatement (tests/cbam_c3_ref.py), the yolov5s
graphs of configs.yolov5_cbam_cfg against the oracle Model.  Bar 1e-3 relative (BASELINE)."""
import copy

import pytest
import torch

import cbam_c3_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step,
                    check_two_steps_bit_identical, nhwc, rel_close)

pytestmark = pytest.mark.gpu

MODES = ('product', 'sigmoid_sum')
# the fixtures' map; more than one 256-pixel chunk of the per-image reduction (390 pixels); three quads (no power of two); 128 quads: two
# channel trips of a pixel's 64 lanes; 260 quads: a second trip of the per-element pass's quad loop (256 quads a trip), four quads wide
SHAPES = [(2, 5, 7, 32), (1, 3, 130, 8), (2, 24, 22, 12), (1, 9, 11, 512), (1, 2, 3, 1040)]
# the per-pixel pass is a grid-stride loop: at this shape its first waves take a second trip (somi_gate_combine_pixel_trips == 2, asserted in
# tests/test_cbam_c3_host.py against the library's own plan)
WALK_SHAPE = (1, 512, 520, 8)
IDS = lambda s: 'x'.join(map(str, s))     # noqa: E731


def _case(shape, seed, grid=False):
    """t, the two gates, a shortcut, an output gradient, a gradient of the channel statistics and a start value for dt (NHWC fp32, CPU)."""
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    t = r(B, H, W, C)
    ca = torch.sigmoid(r(B, C))
    if grid:                                                      # a grid of 1/2 under one gate value: the channel maximum has ties
        t, ca = (t * 2).round() / 2, torch.full((B, C), 0.5)
    return dict(t=t, ca=ca, sa=torch.sigmoid(r(B, H, W)), res=r(B, H, W, C), dout=r(B, H, W, C), dstats=r(B, H, W, 2), have=r(B, H, W, C))


def _want(c, mode, residual):
    """fp64: the output, and through L = <out, dout> + <[mean_c, max_c](t * ca), dstats> the gradients the two backward passes leave."""
    t, ca, sa = (c[k].double().requires_grad_(True) for k in ('t', 'ca', 'sa'))
    t1 = t * ca[:, None, None, :]
    if mode == 'product':
        out = t1 * sa[..., None]
    else:
        out = torch.sigmoid(t * (ca[:, None, None, :] + sa[..., None]))
    if residual:
        out = out + c['res'].double()
    mx, amaxc = t1.max(dim=3)                                     # the first index on ties, and the gradient goes there
    stats = torch.stack([t1.mean(dim=3), mx], dim=3)
    dsa, = torch.autograd.grad((out * c['dout'].double()).sum(), sa, retain_graph=True)
    dt, dca = torch.autograd.grad((out * c['dout'].double()).sum() + (stats * c['dstats'].double()).sum(), [t, ca])
    flat = c['t'].reshape(t.shape[0], -1, t.shape[3])
    hit = flat == flat.max(1)[0][:, None]
    pix = torch.arange(flat.shape[1])[None, :, None].expand_as(hit)
    amaxp = torch.where(hit, pix, torch.full_like(pix, flat.shape[1])).min(1)[0]      # the FIRST pixel of the maximum, spelled out
    return dict(out=out.detach(), dsa=dsa, dt=dt, dca=dca, amaxc=amaxc, amaxp=amaxp, t_max=flat.max(1)[0])


def _wide(t, dev='cuda'):
    """t as channels [4, 4 + c) of a tensor 8 channels wider, the rest 7.0 (a sentinel the kernels must leave)."""
    out = torch.full((*t.shape[:-1], t.shape[-1] + 8), 7.0)
    out[..., 4:4 + t.shape[-1]] = t
    return out.to(dev)


def _untouched(t, c, what):
    assert bool((t[..., :4] == 7.0).all()) and bool((t[..., 4 + c:] == 7.0).all()), f'{what}: a kernel wrote outside its slice'


def _run(ops, c, mode, residual, sliced, C):
    """One forward and both backward passes on the device -> dict of results (slices cut out, the wide tensors kept for the sentinel check)."""
    off = 4 if sliced else 0
    put = _wide if sliced else (lambda v: v.cuda())
    cut = lambda v: v[..., off:off + C]                           # noqa: E731
    t, dout, ca, sa = put(c['t']), put(c['dout']), c['ca'].cuda(), c['sa'].cuda()
    res = put(c['res']) if residual else None
    out = torch.full((*c['t'].shape[:3], C + 2 * off), 7.0, device='cuda')
    ops.gate_combine(t, ca, sa, C, mode, off, residual=res, res_coff=off, out=out, o_coff=off)
    t_max = c['t'].reshape(c['t'].shape[0], -1, C).max(1)[0].cuda()
    dsa, amaxc, amaxp = ops.gate_combine_backward_pixel(dout, t, ca, sa, C, mode, off, off, t_max=t_max)
    dlogit, amaxc2, none = ops.gate_combine_backward_pixel(dout, t, ca, sa, C, mode, off, off, logit=True)
    assert none is None and torch.equal(amaxc, amaxc2)
    dt = torch.full_like(out, 7.0)
    _, dca = ops.gate_combine_backward_chan(dout, t, ca, sa, c['dstats'].cuda(), amaxc, C, mode, off, off, dt=dt, dt_coff=off)
    acc = put(c['have'])
    _, dca2 = ops.gate_combine_backward_chan(dout, t, ca, sa, c['dstats'].cuda(), amaxc, C, mode, off, off, dt=acc, dt_coff=off, accumulate=True)
    torch.cuda.synchronize()
    return dict(out=cut(out), dsa=dsa, dlogit=dlogit, amaxc=amaxc, amaxp=amaxp, dt=cut(dt), dca=dca, acc=cut(acc), dca2=dca2,
                wide=dict(out=out, dt=dt, acc=acc) if sliced else {})


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES + [WALK_SHAPE], ids=IDS)
def test_gate_combine_against_fp64(shape, mode):
    """Forward with and without the shortcut, the per-pixel pass (raw and times sa (1 - sa), both arg-maxima), the per-element pass written and
    accumulated; every tensor a slice at offset 4 of a tensor 8 channels wider filled with 7.0, nothing outside the slice written; two
    launches bit-identical.  The first shape also runs on whole tensors."""
    from somi_amd import ops
    B, H, W, C = shape
    c = _case(shape, 5 + sum(shape))
    for residual, sliced in ((True, True), (False, True)) + (((True, False),) if shape == SHAPES[0] else ()):
        what = f'{shape} {mode} residual {residual} sliced {sliced}'
        want = _want(c, mode, residual)
        a, b = (_run(ops, c, mode, residual, sliced, C) for _ in range(2))
        for k in ('out', 'dsa', 'dlogit', 'amaxc', 'amaxp', 'dt', 'dca', 'acc'):
            assert torch.equal(a[k], b[k]), f'{what}: two launches differ in {k}'
        assert torch.equal(a['dca'], a['dca2'])
        rel_close(a['out'], want['out'], what=f'{what} out')
        rel_close(a['dsa'], want['dsa'], what=f'{what} dsa')
        sa = c['sa'].double()
        rel_close(a['dlogit'], want['dsa'] * sa * (1 - sa), what=f'{what} dsa sa (1 - sa)')
        rel_close(a['dt'], want['dt'], what=f'{what} dt')
        rel_close(a['acc'], want['dt'] + c['have'].double(), what=f'{what} dt accumulated')
        rel_close(a['dca'], want['dca'], what=f'{what} dca')
        assert torch.equal(a['amaxc'].cpu().long(), want['amaxc']), f'{what}: channel arg-max'
        assert torch.equal(a['amaxp'].cpu().long(), want['amaxp']), f'{what}: pixel arg-max'
        for k, v in a['wide'].items():
            _untouched(v, C, f'{what} {k}')


@pytest.mark.parametrize('mode', MODES)
def test_gate_combine_ties_take_the_first_index(mode):
    """Inputs on a grid of 1/2 under one gate value: the channel maximum of most pixels and the spatial maximum of most channels are tied, and
    the FIRST index wins, as in torch.max."""
    from somi_amd import ops
    shape = (2, 9, 11, 12)
    c = _case(shape, 21, grid=True)
    want = _want(c, mode, False)
    t1 = c['t'] * 0.5
    assert bool(((t1 == t1.max(3, keepdim=True)[0]).sum(3) > 1).any()), 'the case has no tied channel maximum'
    flat = c['t'].reshape(2, -1, 12)
    assert bool(((flat == flat.max(1, keepdim=True)[0]).sum(1) > 1).any()), 'the case has no tied pixel maximum'
    a = _run(ops, c, mode, False, True, 12)
    assert torch.equal(a['amaxc'].cpu().long(), want['amaxc']) and torch.equal(a['amaxp'].cpu().long(), want['amaxp'])
    rel_close(a['dt'], want['dt'], what=f'tied {mode} dt')
    rel_close(a['dca'], want['dca'], what=f'tied {mode} dca')


# the depthwise-separable gate: a map smaller than the 7x7 window; degenerate axes; ragged; more than one workgroup, reduction partial and
# weight-gradient chunk (17420 pixels: 69 workgroups, 5 chunks); and one that makes every grid-stride loop take a second trip (33800 pixels
# over the plan's 128 workgroups: somi_dwc_gate_trips == 2, asserted in the test)
DWC_MAPS = [(2, 5, 7), (1, 1, 23), (1, 23, 1), (1, 67, 35), (2, 130, 67), (2, 130, 130)]


def _dwc_case(k, shape):
    """The first seed at which no value entering a ReLU of the fp64 gate is closer to zero than 1e-5 (an fp32 run cannot flip it: its error
    there is of the order of 1e-6) -> (fp64 module, stats NHWC fp32, dsa, parameter start values, flat fp32 parameter vector, running vector)."""
    B, H, W = shape
    for seed in range(64):
        gen = torch.Generator().manual_seed(1000 * k + seed)
        mod = R.DepthWiseConv(2, 1, k, padding=k // 2)
        with torch.no_grad():
            for p_ in mod.parameters():
                p_.copy_(torch.randn(p_.shape, generator=gen) * 0.5)
            for bn in (mod.bn, mod.bn1):
                bn.weight.copy_(torch.rand(bn.weight.shape, generator=gen) + 0.5)
                bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen) * 0.1)
                bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen) + 0.5)
                bn.eps, bn.momentum = 1e-3, 0.03
        stats, dsa = torch.randn(B, H, W, 2, generator=gen), torch.randn(B, H, W, generator=gen)
        start = torch.randn(2 * k * k + 11, generator=gen)
        m64 = copy.deepcopy(mod).double().train()
        seen = []
        hook = m64.relu.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().abs().min().item()))
        m64(stats.double().permute(0, 3, 1, 2))
        hook.remove()
        if min(seen) >= 1e-5:
            break
    else:
        raise AssertionError(f'no seed keeps the ReLUs of k = {k}, {shape} away from zero')
    order = (mod.depth_conv.weight, mod.depth_conv.bias, mod.bn.weight, mod.bn.bias, mod.point_conv.weight, mod.point_conv.bias, mod.bn1.weight,
             mod.bn1.bias)
    params = torch.cat([p_.detach().reshape(-1) for p_ in order])
    run = torch.cat([mod.bn.running_mean, mod.bn.running_var, mod.bn1.running_mean, mod.bn1.running_var]).detach().clone()
    return copy.deepcopy(mod).double(), stats, dsa, start, params, run


@pytest.mark.parametrize('k', [3, 7])
@pytest.mark.parametrize('shape', DWC_MAPS, ids=IDS)
def test_dwc_gate_against_fp64(shape, k):
    """The depthwise-separable gate: training and inference forward, dstats and the eight parameter gradients (accumulated onto a non-zero
    start, in the layout of the parameters) against fp64 autograd of the restatement at 1e-3 of each result's scale (+ check_block's 2e-5 per
    parameter, + one fp32 rounding per summed term for the two analytically zero bias gradients); the running statistics after one training
    forward are torch's BatchNorm2d's; two launches are bit-identical."""
    from somi_amd import _lib, ops
    B, H, W = shape
    assert _lib.lib().somi_dwc_gate_trips(B, H, W) == (2 if shape == DWC_MAPS[-1] else 1)
    m64, stats, dsa, start, params, run0 = _dwc_case(k, shape)
    x64 = stats.double().permute(0, 3, 1, 2).requires_grad_(True)
    m64.eval()
    with torch.no_grad():
        want_eval = torch.sigmoid(m64(x64))[:, 0]
    m64.train()
    kept = {}
    def keep(name):
        def hook(mod, inp, out):
            out.retain_grad()
            kept[name] = out
        return hook
    hooks = [m64.depth_conv.register_forward_hook(keep('u')), m64.point_conv.register_forward_hook(keep('p'))]
    sa64 = torch.sigmoid(m64(x64))[:, 0]
    sa64.backward(dsa.double())
    for h in hooks:
        h.remove()
    # The two conv biases stand in front of a BatchNorm: their gradients, sum_p du_p and sum_p dp_p, are analytically ZERO, so a bar relative
    # to their size has no size to hold on to, and an fp32 implementation leaves the roundings of the N terms it adds.  Their bar is ONE fp32
    # rounding (2^-24) of every term, from the fp64 terms themselves - fixed here from the number format, not from any run.
    zero_bars = {'depth_conv.bias': 2.0 ** -24 * kept['u'].grad.abs().sum(dim=(0, 2, 3)).max().item(),
                 'point_conv.bias': 2.0 ** -24 * kept['p'].grad.abs().sum().item()}
    order = (m64.depth_conv.weight, m64.depth_conv.bias, m64.bn.weight, m64.bn.bias, m64.point_conv.weight, m64.point_conv.bias, m64.bn1.weight,
             m64.bn1.bias)
    want_grads = torch.cat([p_.grad.reshape(-1) for p_ in order])
    want_run = torch.cat([m64.bn.running_mean, m64.bn.running_var, m64.bn1.running_mean, m64.bn1.running_var])
    assert int(m64.bn.num_batches_tracked) == 1
    sd, pd, dd = stats.cuda(), params.cuda(), dsa.cuda()
    rel_close(ops.dwc_gate_eval(sd, pd, run0.cuda(), k, 1e-3), want_eval, what=f'{shape} k {k} eval sa')
    runs = []
    for _ in range(2):
        run = run0.clone().cuda()
        sa, u, p, st = ops.dwc_gate_train(sd, pd, run, k, 1e-3, 0.03)
        dparams = start.clone().cuda()
        dstats = ops.dwc_gate_backward(dd, sd, u, p, st, pd, k, dparams)
        torch.cuda.synchronize()
        runs.append((sa, run, dstats, dparams))
    for a, b in zip(*runs):
        assert torch.equal(a, b), f'{shape} k {k}: two launches differ'
    sa, run, dstats, dparams = runs[0]
    assert bool((sa >= 0.5).all()), 'the ReLU comes before the sigmoid: the gate lies in [0.5, 1)'
    rel_close(sa, sa64, what=f'{shape} k {k} train sa')
    rel_close(run, want_run, what=f'{shape} k {k} running statistics')
    rel_close(dstats.permute(0, 3, 1, 2), x64.grad, what=f'{shape} k {k} dstats')
    rel_close(dparams, want_grads + start.double(), what=f'{shape} k {k} parameter gradients, accumulated')
    names = ('depth_conv.weight',) * (2 * k * k) + ('depth_conv.bias',) * 2 + ('bn.weight',) * 2 + ('bn.bias',) * 2 + ('point_conv.weight',) * 2 + \
        ('point_conv.bias', 'bn1.weight', 'bn1.bias')
    got = dparams.cpu().double() - start.double()
    for name in dict.fromkeys(names):
        idx = [i for i, n in enumerate(names) if n == name]
        rel_close(got[idx], want_grads[idx], what=f'{shape} k {k} d{name}', atol=zero_bars.get(name, 0.0) + 2e-5)


def test_dwc_gate_module_moves_the_buffers_like_batchnorm():
    """SpatialAttentionModuleDWC.gate in training: running_mean / running_var of both BatchNorms and num_batches_tracked as nn.BatchNorm2d."""
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    ref = bn_hyper(fill_state(R.SpatialAttentionModuleDWC(7), 3)).train()
    mine = MB.SpatialAttentionModuleDWC(7)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda().train()
    stats = torch.randn(2, 9, 11, 2, generator=torch.Generator().manual_seed(1))
    want = torch.sigmoid(ref.cv1(stats.permute(0, 3, 1, 2)))[:, 0]
    rel_close(mine.gate(stats.cuda()), want, what='gate module sa')
    for (n, a), (_, b) in zip(mine.named_buffers(), ref.named_buffers()):
        if 'num_batches' in n:
            assert int(a) == int(b) == 1, n
        else:
            rel_close(a, b, what=n)


@pytest.mark.parametrize('k', [3, 5, 7])
def test_spatial_gate_backward_on_its_own(k):
    """ops.spatial_attn_backward - step B of the CBAM backward as a call of its own, between the two combine passes: dstats and the weight and
    bias gradients in nn.Conv2d's (1, 2, k, k) layout, accumulated onto a non-zero start, against fp64 autograd of the k x k conv."""
    import torch.nn.functional as F
    from somi_amd import ops
    gen = torch.Generator().manual_seed(k)
    B, H, W = 2, 9, 11                                            # smaller than two 7x7 windows: every tap meets the border
    stats, dlogit = torch.randn(B, H, W, 2, generator=gen), torch.randn(B, H, W, generator=gen)
    w, dw0, db0 = torch.randn(1, 2, k, k, generator=gen), torch.randn(1, 2, k, k, generator=gen), torch.randn(1, generator=gen)
    s64, w64, b64 = stats.double().requires_grad_(True), w.double().requires_grad_(True), torch.zeros(1, dtype=torch.float64, requires_grad=True)
    F.conv2d(s64.permute(0, 3, 1, 2), w64, b64, padding=k // 2)[:, 0].backward(dlogit.double())
    packed = w[0].permute(1, 2, 0).contiguous().cuda()            # [k][k][2], as SpatialAttentionModule packs it
    dw, db = dw0.clone().cuda(), db0.clone().cuda()
    dstats = ops.spatial_attn_backward(dlogit.cuda(), stats.cuda(), packed, k, dw, db)
    rel_close(dstats, s64.grad, what=f'k = {k} dstats')
    rel_close(dw, w64.grad + dw0.double(), what=f'k = {k} dw accumulated')
    rel_close(db, b64.grad + db0.double(), what=f'k = {k} db accumulated')


@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """C3_CBAM, C3_CBAMS and C3_SCBAM with two bottlenecks, C3CBAM, SCBAMBottleneck with and without the shortcut, C3_CBAM(64, 32, 1, False):
    eval forward, training forward, dx, every parameter gradient and buffer.  The input seeds are cbam_c3_ref.BLOCK_SEEDS."""
    check_block(R.BLOCKS[tag], R, R.block_shape(tag), tag, seed=R.BLOCK_SEEDS[tag])


@pytest.mark.parametrize('tag', ['c3_cbam_dwc', 'c3_scbam', 'c3cbam', 'scbam_bneck_sc'])
def test_backward_into_a_given_tensor(tag):
    """backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`, R what it held and dx what a plain backward of the same forward
    returns."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case(tag)
    mine = R.BLOCKS[tag](MB)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda().train()
    xd = nhwc(x).cuda()
    y = mine(Act(xd.clone()))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    dx = mine.backward(Act(dy.clone()))
    dx = dx.t[..., dx.coff:dx.coff + 64].clone()
    mine(Act(xd.clone()))
    have = torch.randn(xd.shape, generator=gen).cuda()
    before = have.clone()
    got = mine.backward(Act(dy.clone()), dx_out=Act(have), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have, before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')


def test_c3cbam_writes_a_slice_and_skips_dx():
    """C3CBAM: backward(dx_out=) WRITES a channel slice of a wider tensor without accumulate and leaves the rest; need_dx=False returns None
    with the gates' gradients taken; the input is never written."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case('c3cbam')
    mine = MB.C3CBAM(64, 64)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda().train()
    xd = nhwc(x).cuda()
    keep = xd.clone()
    y = mine(Act(xd))
    assert y.t.data_ptr() != xd.data_ptr() and torch.equal(xd, keep), 'C3CBAM ran in place on its input'
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    dx = mine.backward(Act(dy)).t.clone()
    mine(Act(xd))
    wide = torch.full((*xd.shape[:3], 72), 7.0, device='cuda')
    got = mine.backward(Act(dy), dx_out=Act(wide, 4, 64))
    assert got.t.data_ptr() == wide.data_ptr() and got.coff == 4
    assert torch.equal(wide[..., 4:68], dx) and bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 68:] == 7.0).all())
    mine(Act(xd))
    before = mine.spatial_attention.cv1.weight.grad.clone()
    assert mine.backward(Act(dy), need_dx=False) is None and not torch.equal(mine.spatial_attention.cv1.weight.grad, before)


@pytest.mark.parametrize('shortcut', [True, False])
def test_cbam_bottleneck_returning_form_equals_its_accumulate_form(shortcut):
    """CBAMBottleneck.backward(dout) returns what backward(dout, dx_out=zeros, accumulate=True) leaves, with the same parameter gradients."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    make = lambda ns: ns.CBAMBottleneck(64, 64, shortcut, 1, k=((1, 1), (3, 3)), e=1.0, kernel_size=7)      # noqa: E731
    ref = fill_state(make(OB), 5)
    gen = torch.Generator().manual_seed(3)
    xd = torch.randn(2, 5, 7, 64, generator=gen).cuda()
    dy = torch.randn(2, 5, 7, 64, generator=gen).cuda()
    runs = []
    for returning in (True, False):
        mine = make(MB)
        mine.load_state_dict(ref.state_dict())
        mine = bn_hyper(mine).cuda().train()
        mine(Act(xd.clone()))
        if returning:
            dx = mine.backward(Act(dy.clone()))
        else:
            dx = mine.backward(Act(dy.clone()), dx_out=Act(torch.zeros_like(xd)), accumulate=True)
        runs.append((dx.t[..., dx.coff:dx.coff + 64].clone(), {n: p.grad.clone() for n, p in mine.named_parameters()}))
    rel_close(runs[0][0], runs[1][0], rel=1e-6, what='CBAMBottleneck returned dx against the accumulate form on zeros')
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), f'd{n} differs between the two forms'


@pytest.mark.parametrize('variant', R.VARIANTS)
def test_cbam_graph_training_step_eval_and_checkpoint(variant, monkeypatch):
    """yolov5s 6.0 at width 0.25 with C3_CBAM / C3_CBAMS / C3_SCBAM in the backbone (1, 2, 3 and 1 bottlenecks) or a C3CBAM row behind SPPF,
    nc 10, batch 2, 64x64, against the oracle Model: one training forward, ComputeLoss and backward, the eval forward, fuse(); two fresh
    TrainStep.step runs bit-identical; a pickled oracle model loads; a step moves the gates.  Seeds: cbam_c3_ref.GRAPH_SEEDS."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(variant)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, f'yolov5s-{variant}')
    check_eval(ref, mine, imgs, f'yolov5s-{variant}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'cbam_c3_ref'), f'yolov5s-{variant}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    gate = ('depth_conv.weight', 'bn1.weight') if variant.endswith('dwc') else ('spatial_attention.cv1.weight', 'spatial_attention.cv1.bias')
    moved = [k for k in state if k.endswith(('shared_MLP.0.weight', 'shared_MLP.2.bias') + gate)]
    assert len(moved) == (4 if variant == 'row' else 4 * 7)
    for k in moved:
        assert not torch.equal(m.state_dict()[k].cpu(), state[k]), f'a step left {k} where it was'
