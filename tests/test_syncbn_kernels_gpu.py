"""The four sync-BN entry points rank by rank against float64 (tests/syncbn_ref.py): somi_bn_local_sums_f64 (x form and partial-row form),
somi_bn_stats_from_sums_f64, somi_bn_act_backward_sums_f64 and somi_bn_act_backward_apply_sync_f32 through the C ABI, and their Python routes
(ops.bn_stats, ops.bn_stats_from_partials, ops.bn_act_backward with and without pooled=) under a stand-in for torch.distributed.  A rank is a shard of
pixels with its own running buffers and the exchange a concatenation of records, so one process plays world sizes 1, 2, 3 and 8 with unequal
shards (syncbn_ref.CASES says what each case reaches).

Bars (syncbn_ref.bars): dx, scale, shift 1e-5 of max |want|; the records' sums, M2, dgamma, dbeta 2e-5; mean 1e-5; var (derived from rstd) 1e-4 plus
4 * 2^-24 * max mean((x - pivot)^2); rstd and the running buffers what follows from those.  None was set by measurement.  Accumulated outputs start
from noise and the added part is compared; what a call must not touch starts as a NaN sentinel and is compared bit for bit.
tests/test_syncbn_host.py holds the same inputs to half these bars in float32 and shows that five deliberate errors exceed ten times a bar."""
from types import SimpleNamespace as NS

import pytest
import torch

import syncbn_ref as S
from parity import rel_close

pytestmark = pytest.mark.gpu
NAN = float('nan')
F64 = torch.float64


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def api():
    from somi_amd import _lib
    from somi_amd.ops import _ptr, _stream, check
    return _lib.lib(), _ptr, _stream, check


def same_bits(a, b, what):
    a, b = a.detach().cpu().contiguous(), torch.as_tensor(b).detach().cpu().contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: bits changed'


def untouched(t, what):
    same_bits(t, torch.full(t.shape, NAN), what)


def inputs_unchanged(o, what):
    for r in range(len(o.x_buf)):
        same_bits(o.x_buf[r], o.x_buf0[r], f'{what}: x of rank {r}')
        same_bits(o.v_buf[r], o.v_buf0[r], f'{what}: the normalised tensor of rank {r}')
        same_bits(o.dz_buf[r], o.dz_buf0[r], f'{what}: dz of rank {r}')


def ranks_agree(o, what):
    """mean / rstd / scale / shift: the same doubles in the same order on every rank."""
    for r in range(1, len(o.stats)):
        for name in ('mean', 'rstd', 'scale', 'shift'):
            same_bits(getattr(o.stats[r], name), getattr(o.stats[0], name), f'{what}: {name} of rank {r} against rank 0')


def counts_exact(o, c, what):
    assert o.n == [float(n) for n in c.counts], f'{what}: pixel counts {o.n} vs {c.counts}'


# ------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize('case', S.FORWARD_CASES)
def test_forward_records_and_statistics(case):
    """Per rank the record {mean_r, M2_r, n_r} of somi_bn_local_sums_f64 (x form, the rank's own pivot), then somi_bn_stats_from_sums_f64 once per
    rank with that rank's running buffers: mean, var, rstd, scale, shift and both running buffers against the whole batch in float64 (Chan
    combination with unequal counts, the between-rank term, the unbiased variance over the global count); bit-identical between ranks."""
    c, want = S.inputs(case), S.reference(case)
    o = S.simulate(api(), c, 'none', 0, dev())
    counts_exact(o, c, case)
    ranks_agree(o, case)
    inputs_unchanged(o, case)
    S.hold(S.compare(o, want, c, only=S.forward_names(len(c.counts))), f'forward {case}')


@pytest.mark.parametrize('case', S.FORWARD_CASES)
def test_forward_argument_forms(case):
    """gamma = beta = NULL (scale = rstd, shift = -mean * rstd); no running buffers (the given ones keep their bits); one running buffer only: the
    'go together' error, and every output keeps its NaN sentinel."""
    L, p, stream, check = api()
    d = dev()
    c = S.inputs(case)
    W, C = len(c.counts), c.C
    plain = NS(**vars(c))
    plain.gamma, plain.beta = torch.ones(C), torch.zeros(C)
    o = S.simulate(api(), c, 'none', 0, d, affine=False)
    ranks_agree(o, f'{case} without gamma / beta')
    S.hold(S.compare(o, S.evaluate(plain, 'none', 0), plain, only=S.forward_names(W)), f'forward {case} without gamma / beta')
    o = S.simulate(api(), c, 'none', 0, d, running=False)
    ranks_agree(o, f'{case} without running buffers')
    for r in range(W):
        same_bits(o.rm[r], c.rm[r], 'running mean that was not passed')
        same_bits(o.rv[r], c.rv[r], 'running var that was not passed')
    S.hold(S.compare(o, S.reference(case), c, only=list(S.FORWARD_NAMES) + [f'rec_mean{r}' for r in range(W)] + [f'rec_M2_{r}' for r in range(W)]),
           f'forward {case} without running buffers')
    allrec = torch.cat(o.recs)
    for which in ('mean', 'var'):
        out = [torch.full((C,), NAN, device=d) for _ in range(4)]
        rm, rv = c.rm[0].to(d), c.rv[0].to(d)
        rc = L.somi_bn_stats_from_sums_f64(p(allrec), W, C, S.EPS, S.MOM, p(c.gamma.to(d)), p(c.beta.to(d)), *(p(t) for t in out),
                                           p(rm) if which == 'mean' else None, p(rv) if which == 'var' else None, stream())
        with pytest.raises(RuntimeError, match='go together'):
            check(rc, 'bn_stats_from_sums')
        torch.cuda.synchronize()
        for t in out:
            untouched(t, f'an output after the refusal (running {which} only)')
        same_bits(rm, c.rm[0], 'running mean after the refusal')
        same_bits(rv, c.rv[0], 'running var after the refusal')


# ------------------------------------------------------------------------------------------------------------------- partial rows
def _record_of_rows(part, pivot, npix, C):
    L, p, stream, check = api()
    rows = part.shape[1]
    rec = torch.full((2 * C + 1,), NAN, device=part.device, dtype=F64)
    ws = torch.full((2 * 1024 * C,), NAN, device=part.device)
    check(L.somi_bn_local_sums_f64(None, 0, 0, npix, C, p(pivot), p(part[0]), p(part[1]), rows, p(rec), p(ws), stream()), 'bn_local_sums')
    return rec.cpu()


@pytest.mark.parametrize('C', S.PARTIAL_C)
@pytest.mark.parametrize('rows', S.PARTIAL_ROWS)
def test_local_sums_from_partial_rows(rows, C):
    """somi_bn_local_sums_f64 with part_sum / part_sumsq: rows_fold_kernel beyond 1024 rows (1025: per = 2 and 513 folded rows; C = 260: a second
    channel block), then the walk of stage2_sums.  The rows are float32 roundings of float64 group sums and the reference is their float64 sum."""
    d = dev()
    pr = S.partial_rows(rows, C)
    part = pr.part.to(d)
    rec = _record_of_rows(part, pr.pivot.to(d), pr.npix, C)
    assert rec[2 * C].item() == pr.npix
    rel_close(rec[:C], pr.mean, rel=S.MEAN_BAR, what=f'{rows} rows, C = {C}: mean_r')
    rel_close(rec[C:2 * C], pr.M2, rel=S.REDUCED, what=f'{rows} rows, C = {C}: M2_r')
    same_bits(part, pr.part, 'the partial rows are read only')


def test_local_sums_from_a_convolutions_epilogue():
    """The rows a real convolution leaves (conv2d_nhwc(bn_stats={'pivot': rm})): their record agrees with the x-form record of the conv's output, and
    both with float64 statistics of that output."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight
    L, p, stream, check = api()
    d = dev()
    B, H, W, Cin, Cout = 2, 9, 11, 20, 36
    g = S.gen('conv epilogue', (B, H, W, Cin, Cout))
    x = torch.randn(B, H, W, Cin, generator=g).to(d)
    w = pack_conv_weight(torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5, cin_pad=Cin).to(d)
    bias, rm = torch.randn(Cout, generator=g).to(d), (torch.randn(Cout, generator=g) * 0.3).to(d)
    st = {'pivot': rm}
    y = ops.conv2d_nhwc(x, w, bias, kh=3, kw=3, stride=1, pad=1, act='none', cin=Cin, cout=Cout, bn_stats=st)
    npix = B * H * W
    from_rows = _record_of_rows(st['part'], rm, npix, Cout)
    from_x = torch.full((2 * Cout + 1,), NAN, device=d, dtype=F64)
    ws = torch.empty(2 * max(1024, L.somi_red_nchunk(npix)) * Cout, device=d)
    assert tuple(y.shape) == (B, H, W, Cout)
    check(L.somi_bn_local_sums_f64(p(y), Cout, 0, npix, Cout, p(rm), None, None, 0, p(from_x), p(ws), stream()), 'bn_local_sums')
    from_x = from_x.cpu()
    y64 = y.cpu().double().reshape(npix, Cout)
    mean, M2 = y64.mean(0), ((y64 - y64.mean(0)) ** 2).sum(0)
    atol = npix * S.SQ_ROUND * ((y64 - rm.cpu().double()) ** 2).mean(0).max().item()
    assert from_rows[2 * Cout].item() == from_x[2 * Cout].item() == npix
    for name, rec in (('from the epilogue rows', from_rows), ('from the output', from_x)):
        rel_close(rec[:Cout], mean, rel=S.MEAN_BAR, what=f'mean_r {name}')
        rel_close(rec[Cout:2 * Cout], M2, rel=S.REDUCED, atol=atol, what=f'M2_r {name}')
    rel_close(from_rows[:Cout], from_x[:Cout], rel=S.MEAN_BAR, what='mean_r: epilogue rows against the x form')
    rel_close(from_rows[Cout:2 * Cout], from_x[Cout:2 * Cout], rel=S.REDUCED, atol=atol, what='M2_r: epilogue rows against the x form')


# ------------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize('case,act,order', S.BACKWARD_RUNS, ids=S.ident)
def test_backward_records_and_apply(case, act, order):
    """Per rank the record {S1, S2, n_r} of somi_bn_act_backward_sums_f64, then ..._apply_sync_f32: dx against the rank's slice of the whole-batch
    gradient (global count in coefB / coefC), dgamma / dbeta added onto noise against the rank's LOCAL part, their sum over the ranks against the
    whole-batch parameter gradient; dgamma = dbeta = NULL gives the same dx.  The forward in front of it (the statistics of act(x) under order 1)
    is held to its bars too."""
    c, want = S.inputs(case, act, order), S.reference(case, act, order)
    W = len(c.counts)
    o = S.simulate(api(), c, act, order, dev())
    counts_exact(o, c, case)
    ranks_agree(o, case)
    inputs_unchanged(o, case)
    S.hold(S.compare(o, want, c, only=S.forward_names(W) + S.backward_names(W)), f'backward {case} {act}/{order}')
    bare = S.simulate(api(), c, act, order, dev(), param_grads=False)
    for r in range(W):
        same_bits(bare.dx[r], o.dx[r], f'dx of rank {r} without dgamma / dbeta')


@pytest.mark.parametrize('case,act,order', S.TWIN_RUNS, ids=S.ident)
def test_nonsync_backward_through_the_same_kernels(case, act, order):
    """ops.bn_act_backward(batch_stats=True) without sync-BN - bn_act_bwd_stage1<false> and bn_act_bwd_apply<false>, the kernels the sync pair
    shares with it - for every activation and both orders against the same reference."""
    from somi_amd import ops
    d = dev()
    assert ops.SYNC_BN is None
    c, want = S.inputs(case, act, order), S.reference(case, act, order)
    assert len(c.counts) == 1
    dz, x = c.dzs[0].to(d), c.xs[0].to(d)
    dx = torch.full_like(x, NAN)
    dg, db = c.dg0[0].to(d), c.db0[0].to(d)
    mean, rstd, scale, shift = (t.float().to(d) for t in (want.mean, want.rstd, want.scale, want.shift))
    ops.bn_act_backward(dz, 0, x, 0, c.C, mean, rstd, scale, shift, act, order, True, dx, 0, dg, db)
    got = NS(mean=mean, rstd=rstd, scale=scale, shift=shift, dx=[dx], dgamma=[dg.cpu().double() - c.dg0[0].double()],
             dbeta=[db.cpu().double() - c.db0[0].double()])
    S.hold(S.compare(got, want, c, only=['dx0', 'dgamma0', 'dbeta0']), f'non-sync backward {case} {act}/{order}')
    same_bits(dz, c.dzs[0], 'dz')
    same_bits(x, c.xs[0], 'x')


# ------------------------------------------------------------------------------------------------------------------- slices
def test_channel_slices_of_wider_tensors():
    """Case B with x, dz and dx as channel slices: x and dz at coff 12 of C + 24 channels (tests/test_slices_gpu.py), dx at coff 20 of C + 28.  Same
    bars, the same bits as the dense call, everything outside the dx slice keeps its NaN sentinel, x and dz keep theirs."""
    case, act, order = 'B', 'silu', 0
    c, want = S.inputs(case, act, order), S.reference(case, act, order)
    W, C = len(c.counts), c.C
    o = S.simulate(api(), c, act, order, dev(), pad=24, x_coff=12, dz_coff=12, dx_pad=28, dx_coff=20)
    dense = S.simulate(api(), c, act, order, dev())
    counts_exact(o, c, 'slices')
    ranks_agree(o, 'slices')
    inputs_unchanged(o, 'slices')
    S.hold(S.compare(o, want, c, only=S.forward_names(W) + S.backward_names(W)), 'slices of B')
    for r in range(W):
        assert S.same_bits64(o.recs[r].cpu(), dense.recs[r].cpu()) and S.same_bits64(o.brecs[r].cpu(), dense.brecs[r].cpu()), 'records of a slice'
        same_bits(o.dx[r], dense.dx[r], f'dx of rank {r}: slice against dense')
        untouched(o.dx_buf[r][..., :20], 'channels in front of the dx slice')
        untouched(o.dx_buf[r][..., 20 + C:], 'channels behind the dx slice')
    o = S.simulate(api(), c, act, order, dev(), pad=24, x_coff=12, dz_coff=4, dx_pad=28, dx_coff=20)       # dz at an offset of its own
    S.hold(S.compare(o, want, c, only=S.backward_names(W)), 'slices of B, dz at coff 4')
    inputs_unchanged(o, 'slices, dz at coff 4')


# ------------------------------------------------------------------------------------------------------------------- wrappers under FakeDist
WORLD, WB, WH, WW, WC = S.WORLD, S.WB, S.WH, S.WW, S.WC


def _two_passes(monkeypatch, fn):
    """fn(rank) under a FakeDist: once per rank recording (world 1), once per rank replaying (world WORLD) -> the replay's results, rank by rank."""
    from somi_amd import ops
    fd = S.FakeDist(WORLD)
    monkeypatch.setattr(ops, 'SYNC_BN', fd)
    for rank in range(WORLD):
        fd.record(rank)
        fn(rank)
    calls = [len(fd.kept[rank]) for rank in range(WORLD)]
    assert min(calls) == max(calls) >= 1, 'every rank gathers the same number of records'
    out = []
    for rank in range(WORLD):
        fd.replay(rank)
        out.append(fn(rank))
        assert fd.cursor == calls[rank]
    return out


def _forward_result(c, res):
    """res: per rank (mean, rstd, scale, shift, rm, rv) -> the layout `compare` reads."""
    for r in range(1, WORLD):
        for k, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
            same_bits(res[r][k], res[0][k], f'{name} of rank {r} against rank 0')
    return NS(mean=res[0][0], rstd=res[0][1], scale=res[0][2], shift=res[0][3], rm=[t[4] for t in res], rv=[t[5] for t in res])


WRAPPER_FORWARD = ['mean', 'var', 'rstd', 'scale', 'shift'] + [f'{n}{r}' for r in range(WORLD) for n in ('rm', 'rv')]


def test_bn_stats_wrapper_under_sync(monkeypatch):
    """ops.bn_stats -> ops._bn_stats_sync: forward record, forward replay; bn_stats(act=...) raises and leaves the running buffers alone."""
    from somi_amd import ops
    d = dev()
    t = S.wrapper_inputs()
    c = S.batch_of(t.xs, t.dzs, t.gamma, t.beta, t.rm, t.rv, t.dg0, t.db0)
    gamma, beta = t.gamma.to(d), t.beta.to(d)

    def forward(rank):
        rm, rv = t.rm[rank].to(d), t.rv[rank].to(d)
        return (*ops.bn_stats(t.xs[rank].to(d), WC, 0, gamma, beta, S.EPS, S.MOM, rm, rv), rm, rv)
    got = _forward_result(c, _two_passes(monkeypatch, forward))
    S.hold(S.compare(got, S.evaluate(c, 'none', 0), c, only=WRAPPER_FORWARD), 'ops.bn_stats under sync')
    rm, rv = t.rm[0].to(d), t.rv[0].to(d)
    with pytest.raises(RuntimeError, match='no sync-BN form'):
        ops.bn_stats(t.xs[0].to(d), WC, 0, gamma, beta, S.EPS, S.MOM, rm, rv, act='silu')
    same_bits(rm, t.rm[0], 'running mean after the refusal')
    same_bits(rv, t.rv[0], 'running var after the refusal')


def test_bn_stats_from_partials_wrapper_under_sync(monkeypatch):
    """ops.bn_stats_from_partials under sync: each rank's rows come from its own convolution (pivot = its running mean); the statistics are those of
    the outputs of both ranks."""
    from somi_amd import ops
    from somi_amd.pack import pack_conv_weight
    d = dev()
    t = S.wrapper_inputs()
    gamma, beta = t.gamma.to(d), t.beta.to(d)
    w, bias = pack_conv_weight(t.w, cin_pad=16).to(d), t.bias.to(d)
    ys = {}

    def forward(rank):
        rm, rv = t.rm[rank].to(d), t.rv[rank].to(d)
        st = {'pivot': rm}
        ys[rank] = ops.conv2d_nhwc(t.xin[rank].to(d), w, bias, kh=3, kw=3, stride=1, pad=1, act='none', cin=16, cout=WC, bn_stats=st).cpu()
        return (*ops.bn_stats_from_partials(st['part'], st['rows'], WB * WH * WW, WC, gamma, beta, S.EPS, S.MOM, rm, rv), rm, rv)
    res = _two_passes(monkeypatch, forward)
    c = S.batch_of([ys[r] for r in range(WORLD)], t.dzs, t.gamma, t.beta, t.rm, t.rv, t.dg0, t.db0)
    S.hold(S.compare(_forward_result(c, res), S.evaluate(c, 'none', 0), c, only=WRAPPER_FORWARD), 'ops.bn_stats_from_partials under sync')


@pytest.mark.parametrize('form', S.WRAPPER_FORMS)
def test_bn_act_backward_wrapper_under_sync(monkeypatch, form):
    """ops.bn_act_backward under sync, plain and through the pooled= detour (pool_backward_add_ onto dz, then the sync pair; dmax = amaxp = None;
    dz = None): forward record, forward replay, backward record with the replayed statistics, backward replay.  The pooled reference is the plain
    one on dz_eff = dz + davg / HW + [p == amaxp] * dmax."""
    from somi_amd import ops
    d = dev()
    t = S.wrapper_inputs()
    pooled, avg_only, no_dz = form.startswith('pooled'), form == 'pooled, average only', form == 'pooled, dz=None'
    c, act, order = S.wrapper_batch(form, t)
    dzs = [dz.reshape(WB, WH, WW, WC) for dz in c.dzs]
    want = S.reference_of(c, act, order)
    gamma, beta = t.gamma.to(d), t.beta.to(d)
    vs = [v.reshape(WB, WH, WW, WC).to(d) for v in c.vs]

    def forward(rank):
        rm, rv = t.rm[rank].to(d), t.rv[rank].to(d)
        return (*ops.bn_stats(vs[rank], WC, 0, gamma, beta, S.EPS, S.MOM, rm, rv), rm, rv)
    stats = _two_passes(monkeypatch, forward)

    def backward(rank):
        mean, rstd, scale, shift = stats[rank][:4]
        x = t.xs[rank].to(d)
        dz = None if no_dz else t.dzs[rank].to(d)
        dx = torch.full_like(x, NAN)
        dg, db = t.dg0[rank].to(d), t.db0[rank].to(d)
        pl = (t.davg[rank].to(d), None if avg_only else t.dmax[rank].to(d), None if avg_only else t.amaxp[rank].to(d)) if pooled else None
        out = ops.bn_act_backward(dz, 0, x, 0, WC, mean, rstd, scale, shift, act, order, True, dx, 0, dg, db, pooled=pl)
        assert out is dx
        same_bits(x, t.xs[rank], 'x')
        if dz is not None and pooled:                         # dz becomes dz_eff in place (the docstring says so)
            rel_close(dz, dzs[rank], rel=S.POINT, what='dz_eff left in dz')
        elif dz is not None:
            same_bits(dz, t.dzs[rank], 'dz is read only')
        return dx, dg.cpu().double() - t.dg0[rank].double(), db.cpu().double() - t.db0[rank].double()
    res = _two_passes(monkeypatch, backward)
    got = _forward_result(c, stats)
    got.dx, got.dgamma, got.dbeta = [r_[0].reshape(1, 1, -1, WC) for r_ in res], [r_[1] for r_ in res], [r_[2] for r_ in res]
    got.dgamma_sum, got.dbeta_sum = sum(got.dgamma), sum(got.dbeta)
    names = WRAPPER_FORWARD + ['dgamma_sum', 'dbeta_sum'] + [f'{n}{r}' for r in range(WORLD) for n in ('dx', 'dgamma', 'dbeta')]
    S.hold(S.compare(got, want, c, only=names), f'ops.bn_act_backward under sync, {form}')
