"""tests/syncbn_ref.py held to torch: its closed forms (per-rank records, Chan combination, the coefficients A / B / C of dx, the local parameter
gradients) reproduce nn.BatchNorm2d under autograd in float64 on the concatenated batch, for every activation x order and every case; the
condition on the inputs of tests/test_syncbn_kernels_gpu.py - the same formulas in float32 on the CPU stay within half of every bar of that file, on
exactly its inputs, and the absolute term of the variance bar is at most 1e-3 of the smallest channel variance - the teeth of those bars (five
deliberate errors, each beyond ten times a bar on the cases listed), the kink rule of the input builder, and FakeDist.  CPU only."""
import pytest
import torch

import syncbn_ref as S
from parity import rel_close

F64 = torch.float64


def close(got, want, what):
    rel_close(got, want, rel=1e-9, what=what, atol=1e-11)


# ------------------------------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize('act,order', S.FULL_MATRIX, ids=S.ident)
@pytest.mark.parametrize('case', list(S.CASES))
def test_closed_forms_equal_batchnorm2d_autograd(case, act, order):
    """Records combined by Chan's formula = the statistics of the concatenated batch = what nn.BatchNorm2d normalised with and left in its running
    buffers; A d + B (v - mean) + C = autograd's dx; rstd S2_r / S1_r = the parameter gradients under the output gradient of rank r alone."""
    c = S.inputs(case, act, order)
    o, a = S.evaluate(c, act, order), S.autograd(c, act, order)
    v = torch.cat([t.reshape(-1, c.C) for t in c.xs]).double()
    v = v if order == 0 else S.act_f(v, act)
    close(o.mean, v.mean(0), 'mean of the batch')
    close(o.var, v.var(0, unbiased=False), 'biased variance of the batch')
    assert [float(n) for n in o.n] == [float(n) for n in c.counts]
    close(o.rm[0], a.rm, 'running mean')
    close(o.rv[0], a.rv, 'running var (unbiased over the global count)')
    for r in range(len(c.counts)):
        close(o.dx[r], a.dx[r], f'dx of rank {r}')
        close(o.dgamma[r], a.dgamma[r], f'local dgamma of rank {r}')
        close(o.dbeta[r], a.dbeta[r], f'local dbeta of rank {r}')
    close(o.dgamma_sum, a.dgamma_sum, 'dgamma over the ranks')
    close(o.dbeta_sum, a.dbeta_sum, 'dbeta over the ranks')


@pytest.mark.parametrize('act', S.ACTS)
def test_activation_derivatives_equal_autograd(act):
    u = torch.linspace(-6, 6, 2401, dtype=F64) + 1.234e-3        # off 0 and +-3
    u.requires_grad_(True)
    S.act_f(u, act).sum().backward()
    close(S.act_g(u.detach(), act), u.grad, f"{act}'")


def test_case_table():
    """Every row of the case table, and that it reaches what its comment says."""
    red_chunk = lambda n: min(max((-(-n // 1024) + 31) // 32 * 32, 32), 4096)                     # noqa: E731  red_chunk() of train_ops.hip
    nchunk = lambda n: -(-n // red_chunk(n))                                                       # noqa: E731
    want = {'A': ((353,), 24), 'B': ((280, 280), 32), 'C': ((1, 33, 400), 12), 'D': ((7, 5), 1028), 'E': ((40, 41, 42, 43, 44, 45, 46, 47), 64),
            'F': ((20001, 37), 8), 'G': ((64, 64), 16), 'H': ((200, 120), 16), 'I': ((1,), 4)}
    assert S.CASES == want
    assert nchunk(20001) == 626 and 626 > 512 and 1028 // 4 == 257 and 256 % (12 // 4) != 0
    g = S.inputs('G')
    m = [x.double().mean((0, 1, 2)) for x in g.xs]
    assert ((m[0] - m[1]).abs() > 9).all() and all((x.double().reshape(-1, g.C).std(0) < 1.3).all() for x in g.xs)
    h = S.inputs('H')
    hm = torch.cat(h.xs, 2).double().mean((0, 1, 2))
    assert ((hm - 30).abs() < 0.3).all()
    for r in range(2):
        rel_close(h.rm[r], hm + 0.2 + 0.37 * r, rel=1e-6, what=f'pivot of rank {r} of H')
    assert set(c for c, _, _ in S.BACKWARD_RUNS) >= {'A', 'B', 'C', 'E', 'F'}
    assert set((a, o) for c, a, o in S.BACKWARD_RUNS if c == 'B') == set(S.FULL_MATRIX) and len(S.FULL_MATRIX) == 14
    assert set((a, o) for c, a, o in S.TWIN_RUNS if c == 'A') == set(S.FULL_MATRIX)


# ------------------------------------------------------------------------------------------------------------------- bars
@pytest.mark.parametrize('case,act,order', S.ALL_RUNS, ids=S.ident)
def test_float32_on_the_cpu_stays_within_half_of_every_bar(case, act, order):
    """On exactly the inputs of the GPU file: so the bars are reachable in float32, and the inputs do not make them vacuous."""
    c = S.inputs(case, act, order)
    want = S.reference(case, act, order)
    got = S.evaluate(c, act, order, torch.float32)
    assert got.dx[0].dtype == torch.float32 and got.var.dtype == torch.float32
    S.hold(S.compare(got, want, c), f'{case} {act}/{order}: float32 on the CPU against float64, half the bar', factor=0.5)


@pytest.mark.parametrize('form', S.WRAPPER_FORMS)
def test_wrapper_batch_in_float32_stays_within_half_of_every_bar(form):
    """The batch of the ops wrapper tests (world 2, two images of 5 x 7 per rank, C = 24), every form of pooled=: closed forms against autograd, the
    float32 evaluation against half the bars, and the absolute term of the variance bar against the variance."""
    c, act, order = S.wrapper_batch(form)
    assert c.counts == (70, 70) and c.C == 24
    want = S.reference_of(c, act, order)
    closed = S.evaluate(c, act, order)
    for r in range(S.WORLD):
        close(closed.dx[r], want.dx[r], f'{form}: dx of rank {r}')
        close(closed.dgamma[r], want.dgamma[r], f'{form}: local dgamma of rank {r}')
    S.hold(S.compare(S.evaluate(c, act, order, torch.float32), want, c), f'{form}: float32 on the CPU against float64, half the bar', factor=0.5)
    assert S.var_atol(c) <= 1e-3 * want.var.min().item()
    if form == 'pooled':                                      # dz_eff by hand for one element of each kind
        t = S.wrapper_inputs()
        eff = S.dz_eff(t.dzs[1], t.davg[1], t.dmax[1], t.amaxp[1])
        b, ch = 1, 5
        p = t.amaxp[1][b, ch].item()
        q = (p + 1) % (S.WH * S.WW)
        flat = lambda a: a.reshape(S.WB, S.WH * S.WW, S.WC)                                        # noqa: E731
        assert flat(eff)[b, p, ch].item() == pytest.approx(flat(t.dzs[1])[b, p, ch].item() + t.davg[1][b, ch].item() / 35 + t.dmax[1][b, ch].item(), abs=1e-12)
        assert flat(eff)[b, q, ch].item() == pytest.approx(flat(t.dzs[1])[b, q, ch].item() + t.davg[1][b, ch].item() / 35, abs=1e-12)


@pytest.mark.parametrize('case,act,order', S.ALL_RUNS, ids=S.ident)
def test_absolute_term_of_the_variance_bar_is_small_against_the_variance(case, act, order):
    """4 * 2^-24 * max_c mean((v - pivot)^2) is at most 1e-3 of the smallest channel variance of the case: the bar on the variance stays a
    relative one.  (Case I has variance 0: its pivot is the pixel itself and the term is exactly 0.)"""
    c = S.inputs(case, act, order)
    want = S.reference(case, act, order)
    term, vmin = S.var_atol(c), want.var.min().item()
    print(f'{case} {act}/{order}: absolute term {term:.3e}, smallest channel variance {vmin:.3e}')
    assert term <= 1e-3 * vmin


# Where each deliberate error must show (world 1 cannot show any of them; 2 needs a rank much smaller than the batch: 0.03 * var / n_r against 1e-4 of
# the running variance)
TEETH = {1: ('B', 'C', 'D', 'E', 'G', 'H'), 2: ('D', 'G'), 3: ('B', 'C', 'D', 'E', 'F'), 4: ('B', 'C', 'D', 'E', 'F'), 5: ('B', 'E', 'G', 'H')}


@pytest.mark.parametrize('bug,case', [(b, c) for b, cs in TEETH.items() for c in cs], ids=S.ident)
def test_every_deliberate_error_is_beyond_ten_times_a_bar(bug, case):
    c = S.inputs(case, 'silu', 0)
    want = S.reference(case, 'silu', 0)
    errs = S.compare(S.evaluate(c, 'silu', 0, F64, bug=bug), want, c)
    worst = max(errs, key=lambda n: errs[n][0] / max(errs[n][1], 1e-300))
    print(f'{S.BUGS[bug]} on {case}: {worst} off by {errs[worst][0]:.3e}, bar {errs[worst][1]:.3e}')
    assert errs[worst][0] > 10 * errs[worst][1], f'{S.BUGS[bug]} passes on case {case}'
    clean = S.compare(S.evaluate(c, 'silu', 0, F64), want, c)
    assert all(e <= 1e-3 * b or e < 1e-12 for e, b in clean.values()), 'the copy without the error is not the reference'


def test_each_of_the_five_errors_has_a_case_that_shows_it():
    assert sorted(TEETH) == sorted(S.BUGS) == [1, 2, 3, 4, 5] and all(TEETH.values())


# ------------------------------------------------------------------------------------------------------------------- kinks
@pytest.mark.parametrize('case,act,order', [r for r in S.ALL_RUNS if r[1] in S.KINKS], ids=S.ident)
def test_no_preactivation_within_1e_3_of_a_kink(case, act, order):
    c = S.inputs(case, act, order)
    u = S.preact(c, order)
    for k in S.KINKS[act]:
        d = (u - k).abs().min().item()
        print(f'{case} {act}/{order}: nearest pre-activation to {k}: {d:.3e}')
        assert d >= S.KINK_MARGIN
    base = S.inputs(case)                                     # the builder moved elements, it drew no others
    moved = sum((a != b).sum().item() for a, b in zip(c.xs, base.xs))
    assert moved <= 0.02 * c.N * c.C + 4


# ------------------------------------------------------------------------------------------------------------------- partial rows
@pytest.mark.parametrize('C', S.PARTIAL_C)
@pytest.mark.parametrize('rows', S.PARTIAL_ROWS)
def test_partial_rows_folded_in_float32_stay_within_half_the_bars(rows, C):
    pr = S.partial_rows(rows, C)
    assert pr.part.shape == (2, rows, C) and sum(pr.group_lengths) == pr.npix == 3 * rows + 1 and min(pr.group_lengths) >= 1
    assert rows < 3 or len(set(pr.group_lengths)) > 1, 'groups of uneven length'
    per = -(-rows // 1024)
    s = S.rows_fold_f32(pr.part, per)
    mean, M2 = pr.pivot.double() + s[0] / pr.npix, s[1] - s[0] * s[0] / pr.npix
    rel_close(mean, pr.mean, rel=S.MEAN_BAR / 2, what='mean from float32-folded rows')
    rel_close(M2, pr.M2, rel=S.REDUCED / 2, what='M2 from float32-folded rows')
    if rows > 1:                                              # teeth: the last row left out is beyond ten times both bars
        s = S.rows_fold_f32(pr.part[:, :-1], per)
        mean, M2 = pr.pivot.double() + s[0] / pr.npix, s[1] - s[0] * s[0] / pr.npix
        assert (mean - pr.mean).abs().max() > 10 * S.MEAN_BAR * pr.mean.abs().max() or (M2 - pr.M2).abs().max() > 10 * S.REDUCED * pr.M2.abs().max()


# ------------------------------------------------------------------------------------------------------------------- FakeDist
def test_fakedist_records_then_replays():
    fd = S.FakeDist(3)
    recs = {r: [torch.arange(5, dtype=F64) + 10 * r, torch.tensor([float('nan'), -0.0, 1e-300, float(r), 2.0], dtype=F64)] for r in range(3)}
    for r in range(3):
        fd.record(r)
        assert fd.get_world_size(None) == 1
        for rec in recs[r]:
            out = torch.empty(5, dtype=F64)
            fd.all_gather_into_tensor(out, rec, group=None)
            assert S.same_bits64(out, rec)
    recs[1][0][0] = 99.0                                      # the kept records are clones
    assert fd.kept[1][0][0].item() == 10.0
    recs[1][0][0] = 10.0
    for r in range(3):
        fd.replay(r)
        assert fd.get_world_size(None) == 3
        for k, rec in enumerate(recs[r]):
            out = torch.empty(15, dtype=F64)
            fd.all_gather_into_tensor(out, rec.clone(), group=None)
            assert S.same_bits64(out, torch.cat([recs[q][k] for q in range(3)]))


def test_fakedist_refuses_a_record_that_changed_and_a_replay_without_all_ranks():
    fd = S.FakeDist(2)
    fd.record(0)
    fd.all_gather_into_tensor(torch.empty(3, dtype=F64), torch.tensor([0.0, 1.0, 2.0], dtype=F64))
    with pytest.raises(AssertionError, match='every rank'):
        fd.replay(0)
    fd.record(1)
    fd.all_gather_into_tensor(torch.empty(3, dtype=F64), torch.tensor([3.0, 4.0, 5.0], dtype=F64))
    fd.replay(0)
    with pytest.raises(AssertionError, match='differs'):
        fd.all_gather_into_tensor(torch.empty(6, dtype=F64), torch.tensor([-0.0, 1.0, 2.0], dtype=F64))     # -0.0 is not 0.0 bit for bit
    fd.replay(1)
    out = torch.empty(6, dtype=F64)
    fd.all_gather_into_tensor(out, torch.tensor([3.0, 4.0, 5.0], dtype=F64))
    assert out.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(AssertionError, match='never recorded'):
        fd.all_gather_into_tensor(out, torch.tensor([3.0, 4.0, 5.0], dtype=F64))
