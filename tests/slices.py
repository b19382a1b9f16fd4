"""The channel-slice contract of the NHWC kernels, once.  Every block passes activations as a slice [coff, coff + c) of a wider buffer: a kernel
reads its input slices and nothing else, writes its output slice and nothing else, and accumulates onto what its slice held.  embed() builds
such buffers, check_slice_op() drives one op under the contract, and the fp64 references of the copy kernels live here too.  A plain module,
imported like parity.py; pytest does not rewrite its asserts, so every assert carries its own message."""
import torch

from parity import rel_close

FILLS = ('rand_a', 'rand_b', 'nan')
_SEEDS = {'rand_a': 0xA11CE, 'rand_b': 0xB0B}


def embed(t, cs, coff, fill, salt=0):
    """A (..., cs) float32 buffer that holds t's channels at [coff, coff + C).  The other channels hold what `fill` names: 'rand_a' / 'rand_b'
    seeded random finite values (two seeds; `salt` tells buffers of one call apart), 'nan', or a number (a constant canary)."""
    C = t.shape[-1]
    assert 0 <= coff and coff + C <= cs, f'embed: slice [{coff}, {coff + C}) does not fit {cs} channels'
    shape = tuple(t.shape[:-1]) + (cs,)
    if fill in _SEEDS:
        buf = torch.randn(shape, generator=torch.Generator().manual_seed(_SEEDS[fill] + 7919 * salt)) * 3.0 + 0.5
    elif fill == 'nan':
        buf = torch.full(shape, float('nan'))
    else:
        buf = torch.full(shape, float(fill))
    buf[..., coff:coff + C] = t
    return buf


class In:
    """An input slice: the dense content t (..., C) as channels [coff, coff + C) of a (..., cs) buffer."""

    def __init__(self, t, cs, coff):
        self.t, self.cs, self.coff, self.c = t.float(), cs, coff, t.shape[-1]


class Out:
    """An output slice [coff, coff + c) of a (*shape, cs) buffer.  prev: what the slice holds before the call (seeded random values when None; an
    op that writes must replace them).  accumulate: the op adds onto prev, so the expected content is reference + prev."""

    def __init__(self, shape, cs, coff, c, prev=None, accumulate=False):
        assert not accumulate or prev is not None, 'an accumulating output needs its previous content'
        self.shape, self.cs, self.coff, self.c, self.prev, self.accumulate = tuple(shape), cs, coff, c, prev, accumulate


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outside(buf, coff, c):
    return torch.cat([buf[..., :coff], buf[..., coff + c:]], -1)


def _ratio(got, want, rel, atol=0.0):
    got, want = got.double(), want.double()
    if got.shape != want.shape or not want.numel():
        return float('nan')
    return ((got - want).abs().max() / (rel * (want.abs().max() + 1e-12) + atol)).item()


def check_slice_op(run, inputs, outputs, want, *, rel=1e-3, bars=None, what='', device='cuda'):
    """One op under the slice contract.
    run(bufs): performs the op on the device buffers bufs[name] (full width; inputs and outputs by name); a dict it returns holds dense
        results (weight gradients, statistics) that are compared like slices, any other return value is ignored.
    inputs: name -> In, or a plain tensor that is handed over as it is (weights, per-channel vectors).
    outputs: name -> Out.  An op that works in place lists the buffer here, with its content as `prev`.
    want: name -> the fp64 reference, computed by the caller from the dense contents only (without `prev` for accumulating outputs); a
        function there is called with the results of the run (name -> dense tensor) for references that follow from another result.
    bars: name -> relative bar of rel_close, a dict of rel_close's arguments (rel, atol), or 'exact' (torch.equal); names left out take `rel`.
    Asserted: parity at the bar (plus prev where the output accumulates); every result finite and bitwise the same whether the channels
    around the slices hold one set of random values, another one, or NaN; every channel of an output buffer outside its slice bitwise
    unchanged.  Prints one report line."""
    bars = dict(bars or {})
    runs = {}
    for fill in FILLS:
        bufs, before = {}, {}
        for i, (name, s) in enumerate(inputs.items()):
            bufs[name] = (embed(s.t, s.cs, s.coff, fill, salt=i) if isinstance(s, In) else s.detach().clone()).to(device)
        for i, (name, o) in enumerate(outputs.items()):
            stale = torch.randn(o.shape + (o.c,), generator=torch.Generator().manual_seed(1234 + i)) * 5.0 - 1.0
            before[name] = embed(stale if o.prev is None else o.prev.float(), o.cs, o.coff, fill, salt=100 + i)
            bufs[name] = before[name].clone().to(device)
        extra = run(bufs)
        extra = extra if isinstance(extra, dict) else {}
        if torch.device(device).type == 'cuda':
            torch.cuda.synchronize()
        got = {name: bufs[name].detach().cpu() for name in outputs}
        for name, o in outputs.items():                            # 3. writes stay inside
            same = _bits(_outside(got[name], o.coff, o.c)) == _bits(_outside(before[name], o.coff, o.c))
            assert same.all(), (f'{what}: {name}: {int((~same).sum())} values outside the slice [{o.coff}, {o.coff + o.c}) of {o.cs} channels '
                                f'were written (neighbour fill {fill})')
        res = {name: got[name][..., o.coff:o.coff + o.c].clone() for name, o in outputs.items()}
        for name, v in extra.items():
            assert name not in res, f'{what}: {name} is both an output slice and a returned result'
            res[name] = v.detach().cpu().clone()
        runs[fill] = res
    missing = set(runs['rand_a']) ^ set(want)
    assert not missing, f'{what}: results and references differ in names: {sorted(missing)}'
    worst = 0.0
    for name, got in runs['rand_a'].items():                       # 1. parity, 4. accumulate semantics
        o = outputs.get(name)
        exp = (want[name](runs['rand_a']) if callable(want[name]) else want[name]).detach().cpu()
        if o is not None and o.accumulate:
            exp = exp.double() + o.prev.double()
        bar = bars.get(name, rel)
        if bar == 'exact':
            assert got.shape == exp.shape, f'{what}: {name}: shape {tuple(got.shape)} vs {tuple(exp.shape)}'
            assert torch.equal(got, exp.to(got.dtype)), f'{what}: {name} is not bit-exact ({int((got != exp.to(got.dtype)).sum())} values differ)'
        else:
            kw = dict(bar) if isinstance(bar, dict) else {'rel': bar}
            rel_close(got, exp, what=f'{what}: {name}', **kw)
            worst = max(worst, _ratio(got, exp, **kw))
    for fill in FILLS[1:]:                                         # 2. reads stay inside
        for name, got in runs[fill].items():
            assert torch.isfinite(got).all(), f'{what}: {name} is not finite when the channels around the slices hold {fill}'
            same = _bits(got) == _bits(runs['rand_a'][name])
            assert same.all(), (f'{what}: {name} depends on channels outside the input slices: {int((~same).sum())} values changed with the '
                                f'neighbour fill ({fill} vs rand_a)')
    print(f'{what}: worst ratio to the bar {worst:.3f} over {len(want)} results; bitwise the same under {len(FILLS)} neighbour fills; '
          f'{sum(o.cs - o.c for o in outputs.values())} neighbour channels untouched')
    return runs['rand_a']


# ------------------------------------------------------------------------------------------------ references of the copy kernels (NHWC)
def resample_copy_ref(lo, up):
    """Nearest upsample by 2^up: hi[b, h, w] = lo[b, h >> up, w >> up]."""
    n = 1 << up
    return lo.repeat_interleave(n, 1).repeat_interleave(n, 2)


def resample_reduce_ref(hi, up):
    """The adjoint: lo[b, h, w] = sum of the 2^up x 2^up block of hi."""
    n = 1 << up
    B, H, W, C = hi.shape
    return hi.reshape(B, H // n, n, W // n, n, C).sum((2, 4))


def space_to_depth_ref(x):
    """Focus: the cat order [::2,::2], [1::2,::2], [::2,1::2], [1::2,1::2] over (row, column), channels last."""
    return torch.cat([x[:, ::2, ::2], x[:, 1::2, ::2], x[:, ::2, 1::2], x[:, 1::2, 1::2]], -1)


def depth_to_space_ref(y):
    """The inverse (and the gradient) of space_to_depth_ref."""
    B, Ho, Wo, C4 = y.shape
    C = C4 // 4
    x = y.new_zeros(B, 2 * Ho, 2 * Wo, C)
    x[:, ::2, ::2], x[:, 1::2, ::2], x[:, ::2, 1::2], x[:, 1::2, 1::2] = y[..., :C], y[..., C:2 * C], y[..., 2 * C:3 * C], y[..., 3 * C:]
    return x
