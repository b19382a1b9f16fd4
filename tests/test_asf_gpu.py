"""The ASF-YOLO neck on the MI355X (Zoom_cat, ScalSeq, attention_model; asf.hip): every kernel against fp64 of the restatement
(tests/asf_ref.py), run twice and bit-identical, and once under the channel-slice contract (slices.check_slice_op); the blocks against torch
autograd on the restatement; the yolov5_asf_cfg graph against the oracle Model.  Bar 1e-3 of each result's largest value (BASELINE).

Arg-max inputs are seeded and, before anything runs on the GPU, checked in fp64: at every element the two largest candidates (the four pixels
of a Zoom_cat window, the three branches of ScalSeq after affine and LeakyReLU) differ by more than 1e-4 of the largest magnitude; where a
draw violates that the winning input is moved 0.05 further away and everything is recomputed.  With that margin the kernels' codes must
equal the fp64 arg-max at EVERY element.  Exact ties are pinned separately on constant maps."""
import copy

import pytest
import torch

import asf_ref as R
from parity import (check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, rel_close)
from slices import In, Out, check_slice_op

pytestmark = pytest.mark.gpu

MARGIN, PUSH = 1e-4, 0.05


def _unpack(codes, c):
    """(B,H,W,c/4) code bytes -> (B,H,W,c) two-bit codes, channel 4q + j in bits 2j, 2j + 1 of byte q."""
    b = codes.cpu().to(torch.int64)
    return torch.stack([(b >> (2 * j)) & 3 for j in range(4)], -1).reshape(*b.shape[:3], c)


def _gap(cands):
    """cands: list of equal-shape candidates -> (largest minus second largest, index of the first largest)."""
    top = torch.stack(cands).topk(2, 0).values
    return top[0] - top[1], R.first_max(cands)[1]


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        if x is not None:
            assert torch.equal(x, y), 'two launches on the same input differ'
    return a


# ================================================================================================ Zoom_cat
def _zoom_inputs(B, H, W, cl, cm, cs, seed):
    """fp64 NHWC inputs with the margin enforced on every 2x2 window of l."""
    from somi_amd import ops
    gen = torch.Generator().manual_seed(seed)
    l = torch.randn(B, 2 * H, 2 * W, cl, generator=gen, dtype=torch.float64)
    m = torch.randn(B, H, W, cm, generator=gen, dtype=torch.float64)
    s = torch.randn(B, ops.zoomcat_small_size(H), ops.zoomcat_small_size(W), cs, generator=gen, dtype=torch.float64)
    dout = torch.randn(B, H, W, cl + cm + cs, generator=gen, dtype=torch.float64)
    for _ in range(20):
        win = R.windows2(l)
        gap, first = _gap(win)
        bad = gap <= MARGIN * l.abs().max()
        if not bad.any():
            break
        for k, (i, j) in enumerate((i, j) for i in (0, 1) for j in (0, 1)):
            l[:, i::2, j::2] += PUSH * (bad & (first == k))
    gap, _ = _gap(R.windows2(l))
    assert bool((gap > MARGIN * l.abs().max()).all()), 'a Zoom_cat window is still on a near-tie'
    return l.float().double(), m.float().double(), s.float().double(), dout.float().double()      # fp32-representable


# a workgroup is 256 lanes = consecutive (pixel, quad) pairs, quads fastest, of the Q = (Cl + Cm + Cs) / 4 output quads per pixel (forward) or
# of the three gradient segments one after the other (backward): 256 // Q pixels per workgroup when Q <= 256
ZOOM_SHAPES = [(2, 1, 1, 8, 8, 8),              # the smallest case
               (1, 3, 5, 4, 8, 12),             # odd m, unequal widths
               (1, 7, 11, 8, 8, 8),             # 77 pixels x 6 quads = 462 lanes: two workgroups, the last ragged (206), a pixel split over both
               (1, 1, 2, 1032, 8, 8)]           # 262 quads per pixel: more than one workgroup per pixel


@pytest.mark.parametrize('shape', ZOOM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_zoomcat_kernels_against_fp64(shape):
    from somi_amd import ops
    B, H, W, cl, cm, cs = shape
    l, m, s, dout = _zoom_inputs(*shape, seed=sum(shape))
    want, codes = R.zoomcat_ref(l, m, s)
    wl, wm, ws = R.zoomcat_bwd_ref(dout, codes, cl, cm)
    g = [t.float().cuda() for t in (l, m, s, dout)]
    out, cg = _twice(lambda: ops.zoomcat(g[0], g[1], g[2], cl, cm, cs, codes=True))
    rel_close(out, want, what=f'zoomcat {shape} out')
    assert torch.equal(_unpack(cg, cl), codes), f'zoomcat {shape}: {int((_unpack(cg, cl) != codes).sum())} codes differ from the fp64 arg-max'
    # m passed in place: its slice of the output is already written
    pre = torch.full((B, H, W, cl + cm + cs), float('nan'), device='cuda')
    pre[..., cl:cl + cm] = g[1]
    assert torch.equal(ops.zoomcat(g[0], None, g[2], cl, cm, cs, out=pre), out), 'm in place differs from m copied'
    dl, dm, ds = _twice(lambda: ops.zoomcat_backward(g[3], cg, cl, cm, cs, dm=True))
    rel_close(dl, wl, what=f'zoomcat {shape} dl')
    rel_close(dm, wm, what=f'zoomcat {shape} dm')
    rel_close(ds, ws, what=f'zoomcat {shape} ds')
    gen = torch.Generator().manual_seed(1)
    have = [torch.randn(t.shape, generator=gen) for t in (wl, wm, ws)]
    acc = [h.cuda() for h in have]
    ops.zoomcat_backward(g[3], cg, cl, cm, cs, dl=(acc[0], 0), dm=(acc[1], 0), ds=(acc[2], 0), accumulate=(True, True, True))
    for a, h, w_, n in zip(acc, have, (wl, wm, ws), ('dl', 'dm', 'ds')):
        rel_close(a, h.double() + w_, what=f'zoomcat {shape} {n} accumulated')
    skip = ops.zoomcat_backward(g[3], cg, cl, cm, cs, dl=None, dm=None)
    assert skip[0] is None and skip[1] is None and torch.equal(skip[2], ds)


def test_zoomcat_exact_ties_go_to_the_first_pixel():
    from somi_amd import ops
    l = torch.full((1, 4, 6, 8), 1.5, device='cuda')
    l[0, 2:4, 0:2, :] = torch.tensor([[0.0, 2.0], [2.0, 2.0]], device='cuda')[:, :, None]       # window (1, 0): the first of three equal maxima is position 1
    m, s = torch.zeros(1, 2, 3, 8, device='cuda'), torch.zeros(1, 1, 2, 8, device='cuda')
    out, codes = ops.zoomcat(l, m, s, 8, 8, 8, codes=True)
    c = _unpack(codes, 8)
    assert int(c[0, 1, 0].min()) == int(c[0, 1, 0].max()) == 1
    c[0, 1, 0] = 0
    assert int(c.abs().max()) == 0, 'a constant window does not send its maximum to the first pixel'
    dl, _, _ = ops.zoomcat_backward(torch.ones(1, 2, 3, 24, device='cuda'), codes, 8, 8, 8)
    want = torch.full((4, 6), 0.25)
    want[0::2, 0::2] += 1
    want[2, 0], want[2, 1] = 0.25, 1.25
    assert torch.equal(dl.cpu()[0, :, :, 0], want) and torch.equal(dl.cpu()[0, :, :, 7], want)


def test_zoomcat_under_the_slice_contract():
    from somi_amd import ops
    B, H, W, cl, cm, cs = 1, 3, 5, 8, 4, 12
    l, m, s, dout = _zoom_inputs(B, H, W, cl, cm, cs, seed=5)
    want, codes = R.zoomcat_ref(l, m, s)
    wl, wm, ws = R.zoomcat_bwd_ref(dout, codes, cl, cm)
    ct = cl + cm + cs
    state = {}

    def fwd(b):
        _, state['codes'] = ops.zoomcat(b['l'], b['m'], b['s'], cl, cm, cs, 4, 8, 0, out=b['out'], o_coff=4, codes=True)
    check_slice_op(fwd, dict(l=In(l, 16, 4), m=In(m, 16, 8), s=In(s, 12, 0)), dict(out=Out((B, H, W), ct + 8, 4, ct)), dict(out=want),
                   what='zoomcat forward')
    prev = [torch.randn(t.shape, generator=torch.Generator().manual_seed(9 + i)) for i, t in enumerate((wl, wm, ws))]

    def bwd(b):
        ops.zoomcat_backward(b['dout'], state['codes'], cl, cm, cs, 8, dl=(b['dl'], 4), dm=(b['dm'], 0), ds=(b['ds'], 4),
                             accumulate=(False, True, True))
    check_slice_op(bwd, dict(dout=In(dout, ct + 12, 8)),
                   dict(dl=Out(wl.shape[:3], cl + 8, 4, cl), dm=Out(wm.shape[:3], cm + 4, 0, cm, prev=prev[1], accumulate=True),
                        ds=Out(ws.shape[:3], cs + 4, 4, cs, prev=prev[2], accumulate=True)), dict(dl=wl, dm=wm, ds=ws), what='zoomcat backward')


# ================================================================================================ ScalSeq's tail
def _scalseq_inputs(B, H, W, C, seed, negative_gamma):
    """fp64 NHWC maps, gamma, beta and dout, the margin enforced on the three candidates of every output element."""
    gen = torch.Generator().manual_seed(seed)
    us = [torch.randn(B, H // n, W // n, C, generator=gen, dtype=torch.float64) + 0.3 * i for i, n in enumerate((1, 2, 4))]
    gamma = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    if negative_gamma:
        gamma[::2] *= -1                                          # every other channel: the affine reverses the order there
    beta = torch.randn(C, generator=gen, dtype=torch.float64) * 0.1
    dout = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)
    us = [u.float().double() for u in us]
    gamma, beta, dout = gamma.float().double(), beta.float().double(), dout.float().double()
    sign = torch.sign(gamma)
    for _ in range(20):
        r = R.scalseq_tail_ref(us, gamma, beta, 1e-5)
        gap, first = _gap(r['candidates'])
        bad = gap <= MARGIN * torch.stack(r['candidates']).abs().max()
        if not bad.any():
            break
        for i, n in enumerate((1, 2, 4)):                         # the winner's input moves so that its candidate grows
            hit = (bad & (first == i)).reshape(B, H // n, n, W // n, n, C).any(4).any(2)
            us[i] = (us[i] + PUSH * sign * hit).float().double()
    r = R.scalseq_tail_ref(us, gamma, beta, 1e-5)
    gap, _ = _gap(r['candidates'])
    assert bool((gap > MARGIN * torch.stack(r['candidates']).abs().max()).all()), 'a ScalSeq element is still on a near-tie'
    return us, gamma, beta, dout


# statistics: a workgroup takes 16 * NL pixels of the list [u3 | u4 | u5], NL = 256 / min(C / 4, 256) pixel lanes; route: NL 4x4 tiles per
# workgroup; the second stage of both walks the workgroups' rows 256 at a time
SCALSEQ_SHAPES = [(1, 4, 4, 8),                 # one tile, one u5 pixel
                  (2, 8, 12, 32),
                  (1, 20, 28, 16),              # u5 is 5 x 7; 735 pixels, one ragged chunk of 1024
                  (1, 36, 44, 32),              # 99 tiles in workgroups of 32, the last one of 3; 2079 pixels in five chunks of 512, the last ragged
                  (1, 8, 8, 1032),              # 258 quads: two quad chunks, the second of 2; one pixel lane per workgroup
                  (1, 96, 88, 512)]             # 347 rows of statistics partials (the last chunk ragged) and 264 of the route's: more than 256


@pytest.mark.parametrize('negative_gamma', [False, True], ids=['gamma_pos', 'gamma_neg'])
@pytest.mark.parametrize('shape', SCALSEQ_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_scalseq_tail_kernels_against_fp64(shape, negative_gamma):
    """Statistics and running buffers; the forward, with positive and with negative gamma (the arg-max is taken after the affine); pass 1's
    g_i and sums; du_i, dgamma and dbeta."""
    from somi_amd import ops
    B, H, W, C = shape
    us, gamma, beta, dout = _scalseq_inputs(B, H, W, C, 11 + sum(shape), negative_gamma)
    eps, mom = 1e-5, 0.1
    r = R.scalseq_tail_ref(us, gamma, beta, eps, dout)
    gen = torch.Generator().manual_seed(2)
    rm0, rv0 = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    gu = tuple(u.float().cuda() for u in us)
    gg, gb, gd = gamma.float().cuda(), beta.float().cuda(), dout.float().cuda()

    def stats():
        rm, rv = rm0.cuda(), rv0.cuda()
        return (*ops.scalseq_stats(gu, C, gg, gb, eps, mom, rm, rv), rm, rv)
    mean, rstd, scale, shift, rm, rv = _twice(stats)
    what = f'scalseq {shape} gamma{"-" if negative_gamma else "+"}'
    for got, key in ((mean, 'mean'), (rstd, 'rstd'), (scale, 'scale'), (shift, 'shift')):
        rel_close(got, r[key], what=f'{what} {key}')
    rel_close(rm, (1 - mom) * rm0.double() + mom * r['mean'], what=f'{what} running_mean')
    rel_close(rv, (1 - mom) * rv0.double() + mom * r['var_unbiased'], what=f'{what} running_var')
    st = (mean, rstd, scale, shift)
    out, codes = _twice(lambda: ops.scalseq_fuse(gu, C, scale, shift, codes=True))
    rel_close(out, r['out'], what=f'{what} out')
    cg = _unpack(codes, C)
    assert torch.equal(cg, r['codes']), f'{what}: {int((cg != r["codes"]).sum())} codes differ from the fp64 arg-max'
    if B * H * W >= 96:
        assert len(set(r['codes'].flatten().tolist())) == 3, 'a branch never wins: the case does not exercise the routing'

    def route():
        dg, db = torch.ones(C, device='cuda'), torch.full((C,), 2.0, device='cuda')
        gs, sums = ops.scalseq_route_backward(gd, codes, gu, C, st, dgamma=dg, dbeta=db)
        return (*gs, sums, dg, db)
    g3, g4, g5, sums, dg, db = _twice(route)
    for got, want, n in zip((g3, g4, g5), r['g'], '345'):
        rel_close(got, want, what=f'{what} g{n}')
    rel_close(sums[0], r['sum_g'], what=f'{what} sum g')
    rel_close(sums[1], r['sum_gx'], what=f'{what} sum g xhat')
    rel_close(dg, r['dgamma'] + 1, what=f'{what} dgamma (added to 1)')
    rel_close(db, r['dbeta'] + 2, what=f'{what} dbeta (added to 2)')
    rel_close(sums[1], r['dgamma'], what=f'{what} dgamma itself (sum g xhat)')
    rel_close(sums[0], r['dbeta'], what=f'{what} dbeta itself (sum g)')

    def apply():
        return ops.scalseq_apply_backward(tuple(g.clone() for g in (g3, g4, g5)), gu, C, st, sums)
    for got, want, n in zip(_twice(apply), r['du'], '345'):
        rel_close(got, want, what=f'{what} du{n}')


def test_scalseq_eval_form_and_exact_ties():
    """scale / shift left out: scale 1, shift 0 (eval, the BatchNorm folded into the conv).  Equal maps: the first depth index wins everywhere,
    and where u4 == u5 > u3 the second one does."""
    from somi_amd import ops
    B, H, W, C = 1, 8, 8, 8
    gen = torch.Generator().manual_seed(3)
    us = [torch.randn(B, H // n, W // n, C, generator=gen) for n in (1, 2, 4)]
    want = R.first_max([torch.nn.functional.leaky_relu(u.double(), 0.1) if n == 1 else
                        R.up(torch.nn.functional.leaky_relu(u.double(), 0.1).permute(0, 3, 1, 2), n).permute(0, 2, 3, 1) for u, n in zip(us, (1, 2, 4))])[0]
    rel_close(ops.scalseq_fuse(tuple(u.cuda() for u in us), C), want, what='scalseq eval form')
    const = tuple(torch.full((B, H // n, W // n, C), -0.75, device='cuda') for n in (1, 2, 4))
    one, zero = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    out, codes = ops.scalseq_fuse(const, C, one, zero, codes=True)
    assert int(_unpack(codes, C).abs().max()) == 0 and bool((out == -0.075).all())
    gs, _ = ops.scalseq_route_backward(torch.ones(B, H, W, C, device='cuda'), codes, const, C, (zero, one, one, zero))
    assert bool((gs[0] == 0.1).all()) and not gs[1].any() and not gs[2].any()
    higher = (const[0], const[1] + 1, const[2] + 1)
    _, codes = ops.scalseq_fuse(higher, C, one, zero, codes=True)
    assert int(_unpack(codes, C).min()) == int(_unpack(codes, C).max()) == 1


def test_scalseq_under_the_slice_contract():
    from somi_amd import ops
    B, H, W, C = 1, 8, 12, 8
    us, gamma, beta, dout = _scalseq_inputs(B, H, W, C, 21, True)
    r = R.scalseq_tail_ref(us, gamma, beta, 1e-5, dout)
    ins = dict(u3=In(us[0], 16, 4), u4=In(us[1], 12, 0), u5=In(us[2], 16, 8))
    coffs = (4, 0, 8)
    gg, gb = gamma.float(), beta.float()
    state = {}

    def stats(b):
        st = ops.scalseq_stats((b['u3'], b['u4'], b['u5']), C, gg.cuda(), gb.cuda(), 1e-5, 0.1, coffs=coffs)
        state['st'] = st
        return dict(mean=st[0], rstd=st[1], scale=st[2], shift=st[3])
    check_slice_op(stats, ins, {}, {k: r[k] for k in ('mean', 'rstd', 'scale', 'shift')}, what='scalseq stats')

    def fuse(b):
        _, state['codes'] = ops.scalseq_fuse((b['u3'], b['u4'], b['u5']), C, state['st'][2], state['st'][3], coffs, out=b['out'], o_coff=8, codes=True)
    check_slice_op(fuse, ins, dict(out=Out((B, H, W), 20, 8, C)), dict(out=r['out']), what='scalseq fuse')
    assert torch.equal(_unpack(state['codes'], C), r['codes'])

    def route(b):
        gs, sums = ops.scalseq_route_backward(b['dout'], state['codes'], (b['u3'], b['u4'], b['u5']), C, state['st'], coffs, do_coff=4)
        state['sums'] = sums
        return dict(g3=gs[0], g4=gs[1], g5=gs[2], sum_g=sums[0], sum_gx=sums[1])
    check_slice_op(route, dict(ins, dout=In(dout, 12, 4)), {}, dict(g3=r['g'][0], g4=r['g'][1], g5=r['g'][2], sum_g=r['sum_g'], sum_gx=r['sum_gx']),
                   what='scalseq route')

    def apply(b):
        ops.scalseq_apply_backward((b['g3'], b['g4'], b['g5']), (b['u3'], b['u4'], b['u5']), C, state['st'], state['sums'], coffs, (0, 4, 8))
    outs = dict(g3=Out(us[0].shape[:3], 12, 0, C, prev=r['g'][0]), g4=Out(us[1].shape[:3], 12, 4, C, prev=r['g'][1]),
                g5=Out(us[2].shape[:3], 16, 8, C, prev=r['g'][2]))
    check_slice_op(apply, ins, outs, dict(g3=r['du'][0], g4=r['du'][1], g5=r['du'][2]), what='scalseq apply (in place)')


# ================================================================================================ attention_model
@pytest.mark.parametrize('B,C,k', [(2, 8, 3), (3, 8, 9), (2, 64, 3), (2, 1032, 5)], ids=str)
def test_eca_gate_forward_and_backward(B, C, k):
    """C = 8 with k = 9: the taps reach past both edges from every channel.  k = 3 at 8 and 64 and 5 at 1032 channels are the reference's sizes."""
    from somi_amd import ops
    assert (B, C, k) == (3, 8, 9) or ops.eca_kernel_size(C) == k
    gen = torch.Generator().manual_seed(B * C + k)
    avg, w, dgate = (torch.randn(*s, generator=gen) for s in ((B, C), (k,), (B, C)))
    gate, davg, dw = R.eca_ref(avg.double(), w.double(), dgate.double())
    a, wg, dgt = avg.cuda(), w.cuda(), dgate.cuda()
    got, = _twice(lambda: (ops.eca_gate(a, wg),))
    rel_close(got, gate, what=f'eca gate {B}x{C} k={k}')
    gda, gdw = _twice(lambda: ops.eca_gate_backward(a, wg, got, dgt))
    rel_close(gda, davg, what=f'eca davg {B}x{C} k={k}')
    rel_close(gdw, dw, what=f'eca dw {B}x{C} k={k}')


def _mix_case(shape, seed):
    B, H, W, C = shape
    gen = torch.Generator().manual_seed(seed)
    x1, x2, dt, have = (torch.randn(B, H, W, C, generator=gen) for _ in range(4))
    gate, davg = torch.rand(B, C, generator=gen), torch.randn(B, C, generator=gen)
    t = x1.double() * gate.double()[:, None, None, :] + x2.double()
    want = dict(t=t, pool=torch.cat([t.mean(2), t.mean(1)], 1)[:, :, None, :], ds=(dt.double() * x1.double()).sum((1, 2)),
                dx1=dt.double() * gate.double()[:, None, None, :] + davg.double()[:, None, None, :] / (H * W))
    return dict(x1=x1, x2=x2, dt=dt, have=have, gate=gate, davg=davg), want


# the coordinate-attention geometry: a workgroup takes RH rows x NL columns, NL = 256 / min(C / 4, 256)
@pytest.mark.parametrize('shape', [(2, 5, 7, 32), (1, 2, 1, 8), (1, 67, 35, 16), (1, 3, 2, 1032)], ids=lambda s: 'x'.join(map(str, s)))
def test_mix_means_and_its_backward_passes(shape):
    from somi_amd import ops
    B, H, W, C = shape
    c32, want = _mix_case(shape, 5 + sum(shape))
    g = {k: v.cuda() for k, v in c32.items()}
    t, pool = _twice(lambda: ops.asf_mix_means(g['x1'], g['x2'], g['gate'], C))
    rel_close(t, want['t'], what=f'mix {shape} t')
    rel_close(pool, want['pool'], what=f'mix {shape} pool')
    ds, = _twice(lambda: (ops.asf_mix_backward_sums(g['dt'], g['x1'], C),))
    rel_close(ds, want['ds'], what=f'mix {shape} ds')
    dx1, = _twice(lambda: (ops.asf_mix_backward_input(g['dt'], g['gate'], g['davg'], C),))
    rel_close(dx1, want['dx1'], what=f'mix {shape} dx1')
    acc = g['have'].clone()
    ops.asf_mix_backward_input(g['dt'], g['gate'], g['davg'], C, out=acc, accumulate=True)
    rel_close(acc, want['dx1'] + c32['have'].double(), what=f'mix {shape} dx1 accumulated')


def test_mix_under_the_slice_contract():
    from somi_amd import ops
    shape = (2, 5, 7, 8)
    B, H, W, C = shape
    c32, want = _mix_case(shape, 77)
    gate, davg = c32['gate'], c32['davg']

    def mix(b):
        ops.asf_mix_means(b['x1'], b['x2'], gate.cuda(), C, 4, 0, t=b['t'], t_coff=8, pool=b['pool'], p_coff=4)
    check_slice_op(mix, dict(x1=In(c32['x1'], 16, 4), x2=In(c32['x2'], 12, 0)),
                   dict(t=Out((B, H, W), 16, 8, C), pool=Out((B, H + W, 1), 12, 4, C)), dict(t=want['t'], pool=want['pool']), what='asf mix means')

    def sums(b):
        return dict(ds=ops.asf_mix_backward_sums(b['dt'], b['x1'], C, 8, 4))
    check_slice_op(sums, dict(dt=In(c32['dt'], 16, 8), x1=In(c32['x1'], 16, 4)), {}, dict(ds=want['ds']), what='asf mix bwd sums')

    def inp(b):
        ops.asf_mix_backward_input(b['dt'], gate.cuda(), davg.cuda(), C, 8, out=b['dx1'], dx_coff=4, accumulate=True)
    check_slice_op(inp, dict(dt=In(c32['dt'], 16, 8)), dict(dx1=Out((B, H, W), 12, 4, C, prev=c32['have'], accumulate=True)),
                   dict(dx1=want['dx1']), what='asf mix bwd input')


# ================================================================================================ blocks and the graph
@pytest.mark.parametrize('tag', list(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """The four fixture blocks at the fixtures' shapes and attention_model(256) at 2x256x6x10, behind the one-tensor face of asf_ref.Packed:
    eval forward, training forward, the gradient of every input, every parameter gradient and the running statistics (parity.check_block).
    Seeds: the default rule (len(tag)); none had to be changed."""
    make, shape = R.packed_case(tag)
    check_block(make, R, shape, tag)


def test_asf_graph_training_step_eval_and_checkpoint(monkeypatch):
    """yolov5_asf_cfg(depth=0.33, nc=4) at 128 x 128, batch 2, against the oracle Model with the three names registered: one training
    forward, ComputeLoss and backward, the eval forward; two fresh TrainStep.step runs bit-identical; a pickled oracle model loads.
    Seeds tried: synthetic_batch seed 0 (asf_ref.GRAPH_SEED), the first one."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case()
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    check_train_step(ref, mine, imgs, targets, 'yolov5-asf')
    check_eval(ref, mine, imgs, 'yolov5-asf')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'asf_ref'), 'yolov5-asf')
