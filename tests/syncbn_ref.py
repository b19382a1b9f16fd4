"""Cases, inputs, the float64 reference and the single-process stand-ins of tests/test_syncbn_kernels_gpu.py and tests/test_syncbn_host.py: the
four sync-BN entry points (somi_bn_local_sums_f64, somi_bn_stats_from_sums_f64, somi_bn_act_backward_sums_f64, somi_bn_act_backward_apply_sync_f32)
rank by rank.  A "rank" is a shard of pixels (1, 1, n_r, C) plus its own running buffers, the exchange a concatenation of [2C + 1] double records, so
one process plays any world size.

`evaluate` is the operation in closed form (per-rank records, Chan et al.'s combination, the coefficients A / B / C of dx) in the dtype it is handed:
float64 is what the kernels are compared with, float32 is what the host file holds to half the kernels' bars.  `autograd` is torch's own BatchNorm2d
under autograd in float64 on the concatenated batch; the host file holds `evaluate` to it, the GPU file takes dx and the parameter gradients from it.
`bars` gives every compared quantity its bar, `compare` the (error, bar) pairs; both test files go through them, so they cannot drift apart.

A plain module, imported like support_kernels_ref; inputs are float32 CPU tensors drawn from a generator seeded by the case."""
import functools
import math
from types import SimpleNamespace as NS

import torch
import torch.nn as nn
import torch.nn.functional as F

from support_kernels_ref import POINT, REDUCED, gen, ident  # noqa: F401  (ident: the test files' parametrize ids)

F64 = torch.float64
EPS = torch.tensor(1e-3, dtype=torch.float32).item()      # the entry points take eps as a float: this is the value they receive
MOM = 0.03
MEAN_BAR, VAR_REL = 1e-5, 1e-4
SQ_ROUND = 4 * 2.0 ** -24         # x mean((x - pivot)^2): the fp32 squares of the sums around the pivot (test_bn_stats_of_a_slice)
F32_DERIVED = 2.0 ** -21          # rstd arrives as a float32: half an ulp (2^-24) of rstd is 2^-23 of the variance 1 / rstd^2 - eps derived from it;
#                                   four such roundings are allowed (the square root, the reciprocal, the store, eps itself)

ACTS = ('none', 'silu', 'gelu', 'relu', 'sigmoid', 'leaky', 'hswish')      # all of ops.ACT that an activation kernel reads
KINKS = {'relu': (0.0,), 'leaky': (0.0,), 'hswish': (-3.0, 3.0)}           # where the derivative is a convention
KINK_MARGIN = 1e-3

# name: (pixels per rank, C)
CASES = {
    'A': ((353,), 24),                              # sync with one rank = plain BatchNorm
    'B': ((280, 280), 32),                          # the rehearsal's shape, now at kernel bars
    'C': ((1, 33, 400), 12),                        # a one-pixel rank (M2 = 0), very unequal counts, C/4 = 3 does not divide 256
    'D': ((7, 5), 1028),                            # second channel-quad trip of chunk_reduce2 (C/4 = 257)
    'E': (tuple(40 + r for r in range(8)), 64),     # eight ranks, all counts different
    'F': ((20001, 37), 8),                          # 626 chunks: second trip of stage2_sums; a count ratio of 540
    'G': ((64, 64), 16),                            # rank means +5 and -5, spread 1: the between-rank term carries the variance
    'H': ((200, 120), 16),                          # common channel mean 30, spread 1, pivots = mean + 0.2 + 0.37 r (drifted running means)
    'I': ((1,), 4),                                 # whole batch of one pixel: var 0, rstd = 1 / sqrt(eps), running_var takes var, dx zero up to rounding
}
FORWARD_CASES = list(CASES)
FULL_MATRIX = [(a, o) for a in ACTS for o in (0, 1)]
SHORT_MATRIX = [('silu', 0), ('gelu', 1), ('leaky', 0)]
# backward: the whole activation x order matrix at B; A, C, E, F (and D for chunk_reduce2's second trip in the backward's stage 1, I for dx = 0) take three
BACKWARD_RUNS = [('B', a, o) for a, o in FULL_MATRIX] + [(c, a, o) for c in ('A', 'C', 'D', 'E', 'F', 'I') for a, o in SHORT_MATRIX]
TWIN_RUNS = [('A', a, o) for a, o in FULL_MATRIX]         # the non-sync path through the same stage 1 / apply kernels
ALL_RUNS = sorted(set(BACKWARD_RUNS + TWIN_RUNS + [(c, 'none', 0) for c in CASES]))

# partial rows: 1024 is the last size without the fold, 1025 gives per = 2 and 513 folded rows; C = 260 gives rows_fold_kernel a second channel block
# with four live threads
PARTIAL_ROWS = (1, 7, 1024, 1025, 3000)
PARTIAL_C = (8, 260)


# ------------------------------------------------------------------------------------------------------------------- activations
def act_f(u, act):
    return {'none': lambda t: t, 'silu': F.silu, 'gelu': F.gelu, 'relu': F.relu, 'sigmoid': torch.sigmoid,
            'leaky': lambda t: F.leaky_relu(t, 0.1), 'hswish': F.hardswish}[act](u)


def act_g(u, act):
    """The derivative in closed form (the host file holds it to autograd)."""
    one = torch.ones_like(u)
    if act == 'silu':
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    if act == 'gelu':
        return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    if act == 'relu':
        return torch.where(u > 0, one, 0 * one)
    if act == 'sigmoid':
        s = torch.sigmoid(u)
        return s * (1 - s)
    if act == 'leaky':
        return torch.where(u > 0, one, 0.1 * one)
    if act == 'hswish':
        return torch.where(u <= -3, 0 * one, torch.where(u >= 3, one, (2 * u + 3) / 6))
    return one


# ------------------------------------------------------------------------------------------------------------------- inputs
def _stats64(v):
    mean, var = v.mean(0), v.var(0, unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def preact(c, order):
    """The float64 pre-activations of the whole batch (N, C): x * scale + shift under the batch's own statistics (order 0), x itself (order 1)."""
    x = torch.cat([t.reshape(-1, c.C) for t in c.xs]).double()
    if order == 1:
        return x
    mean, _, rstd = _stats64(x)
    return (x - mean) * rstd * c.gamma.double() + c.beta.double()


def _off_the_kinks(x, gamma, beta, act, order):
    """Moves every element of the float32 batch x (N, C) whose pre-activation lies within 2 * KINK_MARGIN of a kink to 4 * KINK_MARGIN from it, on its
    own side (moving elements moves the statistics a little: repeated until it holds)."""
    for _ in range(20):
        x64 = x.double()
        if order == 0:
            mean, _, rstd = _stats64(x64)
            scale = rstd * gamma.double()
            shift = beta.double() - mean * scale
        else:
            scale, shift = torch.ones(x.shape[1], dtype=F64), torch.zeros(x.shape[1], dtype=F64)
        u = x64 * scale + shift
        moved = False
        for k in KINKS[act]:
            near = (u - k).abs() < 2 * KINK_MARGIN
            if near.any():
                side = torch.where(u >= k, 1.0, -1.0).double()
                x = torch.where(near, ((k + side * 4 * KINK_MARGIN - shift) / scale).expand_as(u), x64).float()
                x64, u, moved = x.double(), x.double() * scale + shift, True
        if not moved:
            return x
    raise AssertionError(f'{act}/{order}: pre-activations stay at a kink')


@functools.lru_cache(maxsize=None)
def inputs(case, act='none', order=0):
    """-> xs, dzs (per rank, (1, 1, n_r, C) float32), vs (what the norm sees: xs, or act(xs) rounded to float32 under order 1 - sync-BN materialises it),
    gamma, beta, per rank the running buffers rm / rv (rm is the rank's pivot) and the noise dg0 / db0 the parameter gradients are added onto.
    The draw depends on the case only; (act, order) only move elements off the activation's kinks."""
    counts, C = CASES[case]
    g = gen('syncbn', case)
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    off = r(C) * 1.5 + 0.3
    if case == 'G':
        xs = [r(n, C) + off + (5.0 if k == 0 else -5.0) for k, n in enumerate(counts)]
    elif case == 'H':
        xs = [r(n, C) + 30.0 for n in counts]
    else:
        xs = [r(n, C) * 1.5 + 0.3 for n in counts]
    gamma, beta = torch.rand(C, generator=g) + 0.5, r(C) * 0.2
    dzs = [r(1, 1, n, C) for n in counts]
    rm = [r(C) * 0.1 for _ in counts]
    rv = [torch.rand(C, generator=g) + 0.5 for _ in counts]
    dg0, db0 = [r(C) for _ in counts], [r(C) for _ in counts]
    if act in KINKS:
        xs = list(_off_the_kinks(torch.cat(xs), gamma, beta, act, order).split(list(counts)))
    vs = xs if order == 0 else [act_f(x.double(), act).float() for x in xs]
    if case == 'H':                                       # running means that drifted apart, around a mean far from zero
        m = torch.cat(vs).double().mean(0)
        rm = [(m + 0.2 + 0.37 * k).float() for k in range(len(counts))]
    if case == 'I':                                       # the pivot is the pixel: the absolute term of the variance bar is 0, like the variance
        rm = [vs[0][0].clone()]
    shape = lambda t: t.reshape(1, 1, -1, C).contiguous()                                          # noqa: E731
    return NS(case=case, C=C, counts=counts, N=sum(counts), xs=[shape(x) for x in xs], vs=[shape(v) for v in vs], dzs=dzs, gamma=gamma, beta=beta,
              rm=rm, rv=rv, dg0=dg0, db0=db0)


# ------------------------------------------------------------------------------------------------------------------- closed forms
BUGS = {1: 'the between-rank term dropped', 2: "the rank's own count in the unbiased variance", 3: 'per-rank count in coefB / coefC',
        4: 'dgamma / dbeta from the all-rank sums', 5: 'sums around different pivots added without re-centring'}


def combine(recs, bug=None):
    """Chan et al.: records (mean_r, M2_r, n_r) in rank order -> (mean, biased var) of the union."""
    N = sum(n for _, _, n in recs)
    mean = sum(m * n for m, _, n in recs) / N
    m2 = sum(M2 + (0 if bug == 1 else n * (m - mean) ** 2) for m, M2, n in recs)
    return mean, m2 / N


def evaluate(c, act, order, dtype=F64, bug=None):
    """Everything the four entry points produce, in closed form in `dtype`.  `bug` (1-5, BUGS) plants one deliberate error (the host file's teeth)."""
    t = lambda a: a.to(dtype)                                                                     # noqa: E731
    C, W, N = c.C, len(c.counts), c.N
    xs = [t(x).reshape(-1, C) for x in c.xs]
    vs = xs if order == 0 else [act_f(x, act) for x in xs]
    gamma, beta = t(c.gamma), t(c.beta)
    o = NS(rec_mean=[v.mean(0) for v in vs], n=list(c.counts))
    o.rec_M2 = [((v - m) ** 2).sum(0) for v, m in zip(vs, o.rec_mean)]
    o.mean, o.var = combine(list(zip(o.rec_mean, o.rec_M2, o.n)), bug)
    if bug == 5:                    # {sum (v - pivot_r), sum (v - pivot_r)^2} of every rank added as if all were taken around rank 0's pivot
        s1 = sum((v - t(p)).sum(0) for v, p in zip(vs, c.rm))
        s2 = sum(((v - t(p)) ** 2).sum(0) for v, p in zip(vs, c.rm))
        o.mean, o.var = t(c.rm[0]) + s1 / N, s2 / N - (s1 / N) ** 2
    o.rstd = 1.0 / torch.sqrt(o.var + EPS)
    o.scale = gamma * o.rstd
    o.shift = beta - o.mean * o.scale
    o.rm, o.rv = [], []
    for r in range(W):
        cnt = c.counts[r] if bug == 2 else N
        unb = o.var * cnt / (cnt - 1) if cnt > 1 else o.var            # one pixel has no unbiased variance: the kernel keeps the biased one
        o.rm.append((1 - MOM) * t(c.rm[r]) + MOM * o.mean)
        o.rv.append((1 - MOM) * t(c.rv[r]) + MOM * unb)
    # backward (header comment of bn_act_bwd_stage1): order 0: d = dz * act'(x * scale + shift), v = x; order 1: d = dz, v = act(x)
    dzs = [t(d).reshape(-1, C) for d in c.dzs]
    ds = [dz * act_g(x * o.scale + o.shift, act) for dz, x in zip(dzs, xs)] if order == 0 else dzs
    o.S1 = [d.sum(0) for d in ds]
    o.S2 = [(d * (v - o.mean)).sum(0) for d, v in zip(ds, vs)]
    S1, S2 = sum(o.S1), sum(o.S2)
    o.dx, o.dgamma, o.dbeta = [], [], []
    for r in range(W):
        cnt = c.counts[r] if bug == 3 else N
        A, B, Cc = o.scale, -o.scale * o.rstd * o.rstd * S2 / cnt, -o.scale * S1 / cnt
        dx = A * ds[r] + B * (vs[r] - o.mean) + Cc
        o.dx.append((dx * act_g(xs[r], act) if order == 1 else dx).reshape(1, 1, -1, C))
        o.dgamma.append(o.rstd * (S2 if bug == 4 else o.S2[r]))
        o.dbeta.append(S1 if bug == 4 else o.S1[r])
    o.dgamma_sum, o.dbeta_sum = sum(o.dgamma), sum(o.dbeta)
    o.d_scale = max((o.scale * d).abs().max().item() for d in ds)      # case I: the scale of a dx that is analytically zero
    o.dv_scale = max(d.abs().max().item() for d in ds) * max(v.abs().max().item() for v in vs)
    return o


def autograd(c, act, order):
    """torch's nn.BatchNorm2d (training mode, eps 1e-3, momentum 0.03) in float64 on the concatenated batch, act after it (order 0) or before it
    (order 1) -> mean / var it normalised with, its running buffers after the step (from rank 0's), dx per rank, the whole-batch parameter gradients
    and per rank the local ones: the output gradient restricted to that rank's pixels.  A batch of one pixel is refused by torch: there the norm is
    written out (var = 0, so z = beta)."""
    C, N = c.C, c.N
    x = torch.cat([t.reshape(-1, C) for t in c.xs]).double().requires_grad_(True)
    dz = torch.cat([t.reshape(-1, C) for t in c.dzs]).double()
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double()
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        bn.running_mean.copy_(c.rm[0])
        bn.running_var.copy_(c.rv[0])
    norm = (lambda v: bn(v.t().reshape(1, C, N, 1)).reshape(C, N).t()) if N > 1 else (lambda v: (v - v.mean(0)) / math.sqrt(EPS) * bn.weight + bn.bias)
    z = act_f(norm(x), act) if order == 0 else norm(act_f(x, act))
    if N == 1:                                                 # running_var takes the (biased) variance itself: 0
        with torch.no_grad():
            bn.running_mean.mul_(1 - MOM).add_(MOM * (x if order == 0 else act_f(x, act))[0])
            bn.running_var.mul_(1 - MOM)
    o = NS(rm=bn.running_mean.clone(), rv=bn.running_var.clone(), dgamma=[], dbeta=[])
    bounds = [0]
    for n in c.counts:
        bounds.append(bounds[-1] + n)
    dx, dg, db = torch.autograd.grad(z, (x, bn.weight, bn.bias), dz, retain_graph=True)
    o.dx = [dx[a:b].reshape(1, 1, -1, C) for a, b in zip(bounds, bounds[1:])]
    o.dgamma_sum, o.dbeta_sum = dg, db
    for a, b in zip(bounds, bounds[1:]):
        local = torch.zeros_like(dz)
        local[a:b] = dz[a:b]
        g_, b_ = torch.autograd.grad(z, (bn.weight, bn.bias), local, retain_graph=True)
        o.dgamma.append(g_)
        o.dbeta.append(b_)
    return o


@functools.lru_cache(maxsize=None)
def reference(case, act='none', order=0):
    """What the GPU file compares with: `evaluate` in float64 for the records and statistics, torch autograd for dx and the parameter gradients."""
    return reference_of(inputs(case, act, order), act, order)


def reference_of(c, act, order):
    o, a = evaluate(c, act, order), autograd(c, act, order)
    o.dx, o.dgamma, o.dbeta, o.dgamma_sum, o.dbeta_sum = a.dx, a.dgamma, a.dbeta, a.dgamma_sum, a.dbeta_sum
    return o


def batch_of(xs, dzs, gamma, beta, rm, rv, dg0, db0, case='wrapper'):
    """The layout of `inputs` around tensors a test made itself: per rank x and dz (B, H, W, C) float32 (order 0)."""
    C = xs[0].shape[3]
    flat = lambda t: t.reshape(1, 1, -1, C).contiguous()                                           # noqa: E731
    counts = tuple(x.numel() // C for x in xs)
    return NS(case=case, C=C, counts=counts, N=sum(counts), xs=[flat(x) for x in xs], vs=[flat(x) for x in xs], dzs=[flat(d) for d in dzs], gamma=gamma,
              beta=beta, rm=rm, rv=rv, dg0=dg0, db0=db0)


# ------------------------------------------------------------------------------------------------------------------- the wrapper tests' batch
WORLD, WB, WH, WW, WC = 2, 2, 5, 7, 24                    # world 2, two images of 5 x 7 per rank, C = 24
WRAPPER_FORMS = ['plain', 'plain gelu/1', 'pooled', 'pooled, average only', 'pooled, dz=None']


def wrapper_inputs():
    g = gen('syncbn wrappers', (WORLD, WB, WH, WW, WC))
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    return NS(xs=[r(WB, WH, WW, WC) * 1.5 + 0.3 for _ in range(WORLD)], dzs=[r(WB, WH, WW, WC) for _ in range(WORLD)],
              gamma=torch.rand(WC, generator=g) + 0.5, beta=r(WC) * 0.2, rm=[r(WC) * 0.1 for _ in range(WORLD)],
              rv=[torch.rand(WC, generator=g) + 0.5 for _ in range(WORLD)], dg0=[r(WC) for _ in range(WORLD)], db0=[r(WC) for _ in range(WORLD)],
              davg=[r(WB, WC) for _ in range(WORLD)], dmax=[r(WB, WC) for _ in range(WORLD)],
              amaxp=[torch.randint(0, WH * WW, (WB, WC), generator=g, dtype=torch.int32) for _ in range(WORLD)],
              xin=[r(WB, WH, WW, 16) for _ in range(WORLD)], w=r(WC, 16, 3, 3) / 12.0, bias=r(WC))


def dz_eff(dz, davg, dmax, amaxp):
    """dz + davg / HW + [p == amaxp] * dmax (the docstring of ops.bn_act_backward), in float64."""
    B, H, W_, C = dz.shape
    out = dz.double().reshape(B, H * W_, C) + davg.double()[:, None, :] / (H * W_)
    if dmax is not None:
        out.scatter_add_(1, amaxp.long()[:, None, :], dmax.double()[:, None, :])
    return out.reshape(B, H, W_, C)


def wrapper_batch(form, t=None):
    """-> (c, act, order): the batch of one form of the ops.bn_act_backward test in the layout of `inputs`.  Under pooled= the reference is the plain
    one on dz_eff, rounded to float32 once - as pool_backward_add_ leaves it in dz."""
    t = t or wrapper_inputs()
    act, order = ('gelu', 1) if form == 'plain gelu/1' else ('silu', 0)
    pooled, avg_only, no_dz = form.startswith('pooled'), form == 'pooled, average only', form == 'pooled, dz=None'
    dzs = []
    for r in range(WORLD):
        dz = torch.zeros_like(t.dzs[r]) if no_dz else t.dzs[r]
        dzs.append(dz_eff(dz, t.davg[r], None if avg_only else t.dmax[r], t.amaxp[r]).float() if pooled else dz)
    c = batch_of(t.xs, dzs, t.gamma, t.beta, t.rm, t.rv, t.dg0, t.db0)
    if order == 1:
        c.vs = [act_f(x.double(), act).float() for x in c.xs]
    return c, act, order


# ------------------------------------------------------------------------------------------------------------------- bars
def sq_terms(c):
    """Per rank 4 * 2^-24 * max_c mean((v - pivot_r)^2): what the fp32 squares around the rank's pivot leave in a variance whatever the spread is."""
    return [SQ_ROUND * ((v.double().reshape(-1, c.C) - p.double()) ** 2).mean(0).max().item() for v, p in zip(c.vs, c.rm)]


def var_atol(c):
    """The absolute term of the variance bar: the largest rank's (every rank's sums are taken around its own pivot)."""
    return max(sq_terms(c))


def bars(c, want):
    """name -> (rel of max |want|, atol).  Pointwise results POINT, sums over pixels REDUCED, mean 1e-5, var 1e-4 + the absolute term; rstd and the
    running buffers follow from those: d rstd = rstd^3 / 2 * d var, running = 0.97 * old + 0.03 * (mean | var * N / (N - 1)), each plus the float32
    they are stored as."""
    W, N = len(c.counts), c.N
    sq, va = sq_terms(c), var_atol(c)
    vmax = want.var.abs().max().item()
    var_bar = VAR_REL * vmax + va
    f32 = 2.0 ** -23
    b = {'mean': (MEAN_BAR, 0.0), 'var': (VAR_REL, va + F32_DERIVED * (vmax + EPS)), 'scale': (POINT, 0.0), 'shift': (POINT, 0.0),
         'rstd': (2 * f32, 0.5 * (want.rstd ** 3).max().item() * var_bar), 'dgamma_sum': (REDUCED, 0.0), 'dbeta_sum': (REDUCED, 0.0)}
    unb = N / (N - 1) if N > 1 else 1.0
    one = N == 1                       # analytically zero results are held to the scale of the terms that cancel
    if one:
        b['dgamma_sum'] = (REDUCED, REDUCED * want.rstd.max().item() * want.dv_scale)
    for r in range(W):
        b[f'rec_mean{r}'] = (MEAN_BAR, 0.0)
        b[f'rec_M2_{r}'] = (REDUCED, c.counts[r] * sq[r])
        b[f'rm{r}'] = (MEAN_BAR, 0.0)
        b[f'rv{r}'] = (VAR_REL, MOM * va * unb)
        b[f'S1_{r}'] = (REDUCED, 0.0)
        b[f'S2_{r}'] = (REDUCED, REDUCED * want.dv_scale if one else 0.0)
        b[f'dx{r}'] = (POINT, POINT * want.d_scale if one else 0.0)
        b[f'dgamma{r}'] = (REDUCED, REDUCED * want.rstd.max().item() * want.dv_scale if one else 0.0)
        b[f'dbeta{r}'] = (REDUCED, 0.0)
    return b


def quantities(o):
    """The compared quantities of an `evaluate` / `reference` / `simulate` result, by name.  `var` of a result that carries none is derived from its rstd."""
    q = {'mean': o.mean, 'var': o.var if getattr(o, 'var', None) is not None else 1.0 / o.rstd.double() ** 2 - EPS, 'rstd': o.rstd, 'scale': o.scale,
         'shift': o.shift, 'dgamma_sum': getattr(o, 'dgamma_sum', None), 'dbeta_sum': getattr(o, 'dbeta_sum', None)}
    for attr, key in (('rec_mean', 'rec_mean'), ('rec_M2', 'rec_M2_'), ('rm', 'rm'), ('rv', 'rv'), ('S1', 'S1_'), ('S2', 'S2_'), ('dx', 'dx'),
                      ('dgamma', 'dgamma'), ('dbeta', 'dbeta')):
        for r, t in enumerate(getattr(o, attr, [])):
            q[f'{key}{r}'] = t
    return {k: v for k, v in q.items() if v is not None}


def compare(got, want, c, only=None):
    """-> {name: (max |got - want|, bar)} over every element of every compared quantity (`only`: a subset of the names)."""
    b, g, w = bars(c, want), quantities(got), quantities(want)
    out = {}
    for name in (only or w):
        gv, wv = g[name].detach().cpu().double(), w[name].detach().cpu().double()
        assert gv.shape == wv.shape, f'{name}: shape {tuple(gv.shape)} vs {tuple(wv.shape)}'
        assert torch.isfinite(gv).all(), f'{name}: not finite'
        rel, atol = b[name]
        out[name] = ((gv - wv).abs().max().item(), rel * wv.abs().max().item() + atol)
    return out


def hold(errs, what, factor=1.0):
    """Prints every figure, then asserts every one within factor x its bar."""
    for name, (err, bar) in errs.items():
        print(f'{what}: {name}: max err {err:.3e}, bar {factor * bar:.3e}')
    bad = {n: (e, factor * b) for n, (e, b) in errs.items() if not e <= factor * b}
    assert not bad, f'{what}: beyond the bar (error, bar): {bad}'


FORWARD_NAMES = ('mean', 'var', 'rstd', 'scale', 'shift')


def forward_names(W):
    return list(FORWARD_NAMES) + [f'{n}{r}' for r in range(W) for n in ('rec_mean', 'rec_M2_', 'rm', 'rv')]


def backward_names(W):
    return ['dgamma_sum', 'dbeta_sum'] + [f'{n}{r}' for r in range(W) for n in ('S1_', 'S2_', 'dx', 'dgamma', 'dbeta')]


# ------------------------------------------------------------------------------------------------------------------- partial rows
def partial_rows(R_, C):
    """3R + 1 pixels split into R contiguous groups of uneven length; each group's sum (x - pivot) and sum (x - pivot)^2 formed in float64 and rounded to
    float32 - what a convolution's epilogue leaves - and the record of the float64 sum of those float32 rows: only the kernel's own additions are
    left to bound.  -> part (2, R, C) float32, pivot, npix, want (mean, M2), the absolute term of M2's bar."""
    g = gen('partial rows', (R_, C))
    npix = 3 * R_ + 1
    x = torch.randn(npix, C, generator=g, dtype=F64) * 1.5 + 0.3
    pivot = torch.randn(C, generator=g) * 0.1
    cuts = torch.sort(torch.randperm(npix - 1, generator=g)[:R_ - 1] + 1).values.tolist()
    t = x - pivot.double()
    rows1, rows2 = [], []
    for a, b in zip([0] + cuts, cuts + [npix]):
        rows1.append(t[a:b].sum(0))
        rows2.append((t[a:b] ** 2).sum(0))
    part = torch.stack((torch.stack(rows1), torch.stack(rows2))).float().contiguous()
    s1, s2 = part[0].double().sum(0), part[1].double().sum(0)
    return NS(part=part, pivot=pivot, npix=npix, mean=pivot.double() + s1 / npix, M2=s2 - s1 * s1 / npix, group_lengths=[b - a for a, b in zip([0] + cuts, cuts + [npix])])


def rows_fold_f32(part, per):
    """rows_fold_kernel in float32 on the CPU: `per` consecutive rows added in order; then the float64 sum over the folded rows (stage2_sums)."""
    rows = part.shape[1]
    folded = []
    for a in range(0, rows, per):
        acc = torch.zeros_like(part[:, 0])
        for k in range(a, min(a + per, rows)):
            acc = acc + part[:, k]
        folded.append(acc)
    return torch.stack(folded, 1).double().sum(1)


# ------------------------------------------------------------------------------------------------------------------- one process, any world size
def same_bits64(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


class FakeDist:
    """Stands in for torch.distributed behind ops.SYNC_BN.  record(rank): world 1 - an all-gather copies the caller's record out and keeps a clone.
    replay(rank): world W - the k-th all-gather of a rank writes the k-th kept records of all ranks, the caller's own at its rank index, and asserts
    that the caller's record equals the one it kept, bit for bit."""

    def __init__(self, world):
        self.world, self.kept, self.mode, self.rank, self.cursor = world, {}, None, None, 0

    def record(self, rank):
        assert 0 <= rank < self.world
        self.mode, self.rank, self.kept[rank] = 'record', rank, []

    def replay(self, rank):
        assert sorted(self.kept) == list(range(self.world)), 'replay needs the records of every rank'
        self.mode, self.rank, self.cursor = 'replay', rank, 0

    def get_world_size(self, group=None):
        return 1 if self.mode == 'record' else self.world

    def all_gather_into_tensor(self, out, rec, group=None):
        assert self.mode in ('record', 'replay') and out.dtype == rec.dtype and out.numel() == self.get_world_size() * rec.numel()
        if self.mode == 'record':
            out.copy_(rec)
            self.kept[self.rank].append(rec.detach().clone())
            return
        k, self.cursor = self.cursor, self.cursor + 1
        assert k < len(self.kept[self.rank]), f'rank {self.rank}: all-gather {k} was never recorded'
        assert same_bits64(rec, self.kept[self.rank][k]), f'rank {self.rank}: the record of all-gather {k} differs from the recorded pass'
        out.copy_(torch.cat([rec if q == self.rank else self.kept[q][k] for q in range(self.world)]))


def embed(t, cs, coff, key):
    """(1, 1, n, C) -> the channels [coff, coff + C) of a (1, 1, n, cs) tensor of noise."""
    if cs == t.shape[3] and coff == 0:
        return t.clone()
    buf = torch.randn(*t.shape[:3], cs, generator=gen('embed', key)) * 3
    buf[..., coff:coff + t.shape[3]] = t
    return buf


def simulate(api, c, act, order, dev, *, pad=0, x_coff=0, dz_coff=0, dx_pad=0, dx_coff=0, affine=True, running=True, param_grads=True):
    """The four entry points in the order of a real step, every rank of c in turn in one process: per rank somi_bn_local_sums_f64 (the rank's running
    mean as its pivot), the records concatenated, per rank somi_bn_stats_from_sums_f64 with that rank's own running buffers; then per rank
    somi_bn_act_backward_sums_f64 with the statistics that rank received, the records concatenated, per rank ..._apply_sync_f32 (dgamma / dbeta
    added onto the rank's noise).  x and dz sit at x_coff / dz_coff of C + pad channels, dx at dx_coff of C + dx_pad channels that start as NaN.
    Compares nothing; returns everything it saw (the layout of `evaluate`, plus the buffers themselves)."""
    from somi_amd.ops import ACT
    L, p, stream, check = api
    C, W = c.C, len(c.counts)
    cs, nan = C + pad, float('nan')
    f32 = lambda *s: torch.full(s, nan, device=dev)                                                 # noqa: E731
    o = NS(rec_mean=[], rec_M2=[], n=[], rm=[], rv=[], S1=[], S2=[], dx=[], dgamma=[], dbeta=[], stats=[], recs=[], brecs=[], dx_buf=[], x_buf=[],
           v_buf=[], dz_buf=[], x_buf0=[], v_buf0=[], dz_buf0=[], var=None)
    gamma, beta = (c.gamma.to(dev), c.beta.to(dev)) if affine else (None, None)
    for r in range(W):
        n = c.counts[r]
        for name, t, off in (('x', c.xs[r], x_coff), ('v', c.vs[r], x_coff), ('dz', c.dzs[r], dz_coff)):
            host = embed(t, cs, off, (c.case, name, r))
            getattr(o, name + '_buf0').append(host)
            getattr(o, name + '_buf').append(host.to(dev))
        rec = torch.full((2 * C + 1,), nan, device=dev, dtype=F64)
        ws = torch.empty(2 * max(1024, L.somi_red_nchunk(n)) * C, device=dev)
        o.rm.append(c.rm[r].to(dev))
        o.rv.append(c.rv[r].to(dev))
        check(L.somi_bn_local_sums_f64(p(o.v_buf[r]), cs, x_coff, n, C, p(o.rm[r]), None, None, 0, p(rec), p(ws), stream()), 'bn_local_sums')
        o.recs.append(rec)
    allrec = torch.cat(o.recs)
    for r in range(W):
        st = NS(mean=f32(C), rstd=f32(C), scale=f32(C), shift=f32(C))
        check(L.somi_bn_stats_from_sums_f64(p(allrec), W, C, EPS, MOM, p(gamma), p(beta), p(st.mean), p(st.rstd), p(st.scale), p(st.shift),
                                            p(o.rm[r]) if running else None, p(o.rv[r]) if running else None, stream()), 'bn_stats_from_sums')
        o.stats.append(st)
    for r in range(W):
        n, st = c.counts[r], o.stats[r]
        rec = torch.full((2 * C + 1,), nan, device=dev, dtype=F64)
        ws = torch.empty(2 * L.somi_red_nchunk(n) * C + 3 * ((C + 3) // 4 * 4), device=dev)
        check(L.somi_bn_act_backward_sums_f64(p(o.dz_buf[r]), cs, dz_coff, p(o.x_buf[r]), cs, x_coff, p(st.mean), p(st.scale), p(st.shift), ACT[act],
                                              order, n, C, p(rec), p(ws), stream()), 'bn_act_backward_sums')
        o.brecs.append(rec)
    allb = torch.cat(o.brecs)
    for r in range(W):
        n, st = c.counts[r], o.stats[r]
        dx = f32(1, 1, n, C + dx_pad)
        dg, db = (c.dg0[r].to(dev), c.db0[r].to(dev)) if param_grads else (None, None)
        ws = torch.empty(3 * ((C + 3) // 4 * 4), device=dev)
        check(L.somi_bn_act_backward_apply_sync_f32(p(o.dz_buf[r]), cs, dz_coff, p(o.x_buf[r]), cs, x_coff, p(st.mean), p(st.rstd), p(st.scale),
                                                    p(st.shift), ACT[act], order, p(o.brecs[r]), p(allb), W, p(dx), C + dx_pad, dx_coff, p(dg), p(db),
                                                    n, C, p(ws), stream()), 'bn_act_backward_apply_sync')
        o.dx_buf.append(dx)
        o.dx.append(dx[..., dx_coff:dx_coff + C])
        if param_grads:
            o.dgamma.append(dg.cpu().double() - c.dg0[r].double())            # the added part
            o.dbeta.append(db.cpu().double() - c.db0[r].double())
    for r in range(W):
        rec = o.recs[r].cpu()
        o.rec_mean.append(rec[:C])
        o.rec_M2.append(rec[C:2 * C])
        o.n.append(rec[2 * C].item())
        b = o.brecs[r].cpu()
        o.S1.append(b[:C])
        o.S2.append(b[C:2 * C])
        assert b[2 * C].item() == c.counts[r], 'the backward record carries the pixel count'
    st = o.stats[0]
    o.mean, o.rstd, o.scale, o.shift = st.mean, st.rstd, st.scale, st.shift
    if param_grads:
        o.dgamma_sum, o.dbeta_sum = sum(o.dgamma), sum(o.dbeta)
    return o
