"""The operand-rounding model of the opt-in reduced-precision conv forms (somi_conv_desc.prec / ops.CONV_PREC: 1 = bf16, 2 = bf16x3), for
tests/test_conv_amp_host.py and tests/test_conv_amp_gpu.py.  A plain CPU module without device code, imported like odconv_ref.

A reduced-precision kernel has an exact model: round the two operands of a product the way the kernel's LDS staging does (store_split /
store_bf16 in conv_igemm.hip and conv_wgrad.hip), then convolve in fp64.

    r(t)  = t.float().bfloat16().float()          round to nearest, ties to even
    hi(t) = r(t),  lo(t) = r(t - hi(t))           the difference in fp32, as in (__bf16)(v - (float)h)

For a product f(a, b) of the three a training step has (forward x * w, data gradient dy * w, weight gradient x * dy):

    exact  = f(a, b)
    bf16   = f(hi a, hi b)
    bf16x3 = f(hi a, hi b) + f(hi a, lo b) + f(lo a, hi b)

A bf16 x bf16 product has 16 significant bits and is exact in fp32, so a kernel differs from its model only by its fp32 accumulation.  Bias,
activation, residual and accumulate terms are fp32 in the kernels; here they are applied in fp64 after the product.

Tensors are in torch's layouts (NCHW activations, (Cout, Cin, k, k) weights, a leading batch dimension on per-sample weights)."""
import functools
import math
import warnings
import zlib
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

PRODUCTS = ('forward', 'dgrad', 'wgrad')
MODES = ('exact', 'bf16', 'bf16x3')

# (B, H, W, Cin, Cout, k, stride, pad, dil) -> what the launch planners (plan_tiles in conv_igemm.hip, plan in conv_wgrad.hip) make of it; the GPU
# tests assert every tile named here from somi_conv2d_kernel_name / somi_conv2d_wgrad_kernel_name.  `reduced`: the products whose launch has a
# bf16 form; the others run exact fp32 whatever `prec` asks for (`fallback`) and are not modelled.  The forward / data-gradient bf16 forms exist
# for the two 8-wave tiles (128 x 128, 128 x 64) only: a launch that plans 64 x 128 or 128 x 32 (4 waves) is a fallback.
CASES = {
    # forward 128 x 128 stream-K over 2 tiles (M = 240: one ragged); dgrad 128 x 64 stream-K; wgrad 128 x 128, one split of 240 pixels
    # (240 % 32 = 16), last K-tile 64 wide
    'A': NS(shape=(2, 12, 10, 64, 128, 3, 1, 1, 1), per_sample=False, reduced=PRODUCTS, fallback=()),
    # forward 128 x 64, 1x1; dgrad 128 x 128 without stream-K (2 K-tiles); wgrad 64 x 128 (64-channel dy tile), 2 splits + reduce
    'B': NS(shape=(2, 16, 16, 256, 64, 1, 1, 0, 1), per_sample=False, reduced=PRODUCTS, fallback=()),
    # stride 2: forward 128 x 128, wgrad 128 x 128 with K = 1152; the data gradient (no stream-K at stride 2, 663 rows) plans 64 x 128: fallback
    'C': NS(shape=(3, 17, 13, 128, 256, 3, 2, 1, 1), per_sample=False, reduced=('forward', 'wgrad'), fallback=('dgrad',)),
    # ... and with Cin = 64 the stride-2 data gradient plans 128 x 64: the bf16 forms over four parity classes of unequal size (9 / 8 rows,
    # 7 / 6 columns)
    'C2': NS(shape=(3, 17, 13, 64, 256, 3, 2, 1, 1), per_sample=False, reduced=PRODUCTS, fallback=()),
    # 3 K-tiles per tap, ragged N (second N tile 32 wide); dgrad with 5 K-tiles per tap; wgrad 64 x 128, 6 splits, K = 864 (last tile 96 wide)
    'D': NS(shape=(5, 17, 17, 96, 160, 3, 1, 1, 1), per_sample=False, reduced=PRODUCTS, fallback=()),
    # forward: the 128 x 64 variant for Cout > 64 (M >= 32768), one K-tile per tap; wgrad 64 x 128 with ~100 splits through wgrad_reduce_kernel;
    # dgrad plans 128 x 32: fallback
    'E': NS(shape=(2, 128, 128, 32, 192, 3, 1, 1, 1), per_sample=False, reduced=('forward', 'wgrad'), fallback=('dgrad',)),
    # dilated: the DILBWD NS = 1 | 2 data gradient (128 x 64), forward and wgrad with dil = 2
    'G': NS(shape=(2, 14, 14, 64, 128, 3, 1, 2, 2), per_sample=False, reduced=PRODUCTS, fallback=()),
    # the stream-K shape of test_conv_reduced_precision_forms: cut tiles finished by the fix-up kernel, 25 wgrad splits
    'S': NS(shape=(4, 40, 40, 128, 256, 3, 1, 1, 1), per_sample=False, reduced=PRODUCTS, fallback=()),
    # 64 output channels: the forward plans the 8-wave 128 x 64 tile with and without the stream-K workspace (two schedules of one bf16 form)
    'T': NS(shape=(2, 12, 10, 64, 64, 3, 1, 1, 1), per_sample=False, reduced=PRODUCTS, fallback=()),
    # 32768 rows: the forward plans 128 x 128 with the workspace (stream-K over 256 tiles) and without it (one tile per workgroup): the two
    # schedules of the other 8-wave tile.  Forward only
    'U': NS(shape=(2, 128, 128, 32, 128, 3, 1, 1, 1), per_sample=False, reduced=('forward',), fallback=()),
    # per-sample weights, stride 2: dgrad 128 x 64 in the bf16 forms; the forward (25 rows per image, no stream-K) plans 64 x 128 and the
    # per-sample wgrad has no bf16 form: fallbacks
    'P': NS(shape=(3, 10, 10, 64, 128, 3, 2, 1, 1), per_sample=True, reduced=('dgrad',), fallback=('forward', 'wgrad')),
    # ... and with Cout = 64 the per-sample forward plans 128 x 64 too
    'P2': NS(shape=(3, 10, 10, 64, 64, 3, 2, 1, 1), per_sample=True, reduced=('forward', 'dgrad'), fallback=('wgrad',)),
    # Cin % 32 != 0: wgrad runs reduced (K = 180, last K-tile 52 wide) while forward (generic path) and dgrad (128 x 32) fall back
    'W': NS(shape=(2, 9, 9, 20, 128, 3, 1, 1, 1), per_sample=False, reduced=('wgrad',), fallback=('forward', 'dgrad')),
}


def out_size(size, k, s, p, d=1):
    return (size + 2 * p - (d * (k - 1) + 1)) // s + 1


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def rel_err(got, want):
    """max |got - want| over max |want|: the distance every bar here is stated in."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-12)


# ------------------------------------------------------------------------------------------------------------------------ the rounding
def r(t):
    """fp32 -> bf16 -> fp32, round to nearest, ties to even; keeps t's dtype."""
    return t.float().bfloat16().float().to(t.dtype)


def split(t):
    """(hi, lo) of the bf16x3 form, in t's dtype."""
    f = t.float()
    hi = f.bfloat16().float()
    lo = (f - hi).bfloat16().float()
    return hi.to(t.dtype), lo.to(t.dtype)


def _bits(t):
    return t.float().contiguous().view(torch.int32)


def trunc_bf16(t):
    """The wrong conversion that drops the low 16 bits."""
    return (_bits(t) & -65536).view(torch.float32)


def half_up_bf16(t):
    """The wrong conversion that adds half an ulp and drops the low 16 bits (ties away from zero)."""
    return ((_bits(t) + 0x8000) & -65536).view(torch.float32)


def ties(shape, gen):
    """fp32 values that each lie exactly half-way between two neighbouring bf16 values: a bf16-representable N(0, 1) draw plus half a bf16 ulp of
    its magnitude (bit 15 of the fp32 pattern: exact).  About half of the draws have an even bf16 mantissa, where ties-to-even keeps the value
    (as truncation does); the others round away (as half-up does)."""
    v = torch.randn(shape, generator=gen).bfloat16().float()
    v = torch.where(v.abs() < 2.0 ** -20, torch.ones_like(v), v)          # keeps every value normal and non-zero
    return (_bits(v) | 0x8000).view(torch.float32)


# ------------------------------------------------------------------------------------------------------------------- the three products
def _per_sample(f, a, b):
    return torch.cat([f(a[i:i + 1], b[i]) for i in range(a.shape[0])])


def product(which, a, b, geom, per_sample=False):
    """One bilinear product in the dtype of its operands.  forward: a = x, b = w -> y.  dgrad: a = dy, b = w -> dx.  wgrad: a = x, b = dy -> dw
    ((B, Cout, Cin, k, k) with per-sample weights)."""
    B, H, W, Cin, Cout, k, s, p, dil = geom
    if which == 'forward':
        f = lambda x, w: F.conv2d(x, w, None, s, p, dil)                                                    # noqa: E731
        return _per_sample(f, a, b) if per_sample else f(a, b)
    if which == 'dgrad':
        f = lambda dy, w: torch.nn.grad.conv2d_input((dy.shape[0], Cin, H, W), w, dy, s, p, dil)            # noqa: E731
        return _per_sample(f, a, b) if per_sample else f(a, b)
    assert which == 'wgrad', which
    f = lambda x, dy: torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), dy, s, p, dil)                      # noqa: E731
    return torch.stack([f(a[i:i + 1], b[i:i + 1]) for i in range(B)]) if per_sample else f(a, b)


def model(which, a, b, geom, per_sample=False, dtype=torch.float64):
    """{exact, bf16, bf16x3} of one product, accumulated in `dtype` (fp64: the reference; fp32: how far an fp32 accumulation of the same
    rounded operands lies from it)."""
    ah, al = (t.to(dtype) for t in split(a))
    bh, bl = (t.to(dtype) for t in split(b))
    f = lambda u, v: product(which, u, v, geom, per_sample)                                                 # noqa: E731
    hh = f(ah, bh)
    return {'exact': f(a.to(dtype), b.to(dtype)), 'bf16': hh, 'bf16x3': hh + f(ah, bl) + f(al, bh)}


def operands(which, inp):
    return {'forward': (inp.x, inp.w), 'dgrad': (inp.dy, inp.w), 'wgrad': (inp.x, inp.dy)}[which]


def forward_epilogue(y, bias, res):
    """bias -> SiLU -> residual, the order of conv_epilogue."""
    return F.silu(y + bias.to(y.dtype)[None, :, None, None]) + res.to(y.dtype)


def dgrad_epilogue(dx, acc, acc2):
    return dx + acc.to(dx.dtype) + acc2.to(dx.dtype)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def inputs(name, tied=False):
    """fp32 inputs of a case, from a generator seeded by the case: x and dy N(0, 1) (or exact ties of the bf16 rounding), w N(0, 1) / sqrt(K), and
    the epilogue terms (bias, forward residual, the data gradient's two accumulate sources).  Everything is in the normal range."""
    c = CASES[name]
    B, H, W, Cin, Cout, k, s, p, dil = c.shape
    Ho, Wo = out_size(H, k, s, p, dil), out_size(W, k, s, p, dil)
    g = _gen('conv_amp', name, tied)
    draw = (lambda shape: ties(shape, g)) if tied else (lambda shape: torch.randn(shape, generator=g))
    x, dy = draw((B, Cin, H, W)), draw((B, Cout, Ho, Wo))
    w = torch.randn(((B,) if c.per_sample else ()) + (Cout, Cin, k, k), generator=g) / math.sqrt(Cin * k * k)
    return NS(name=name, geom=c.shape, per_sample=c.per_sample, x=x, w=w, dy=dy, Ho=Ho, Wo=Wo,
              bias=torch.randn(Cout, generator=g), res=torch.randn(B, Cout, Ho, Wo, generator=g),
              acc=torch.randn(B, Cin, H, W, generator=g), acc2=torch.randn(B, Cin, H, W, generator=g))


@functools.lru_cache(maxsize=None)
def case(name, tied=False):
    """-> (inputs, {product: {exact, bf16, bf16x3}}) in fp64, for the products of the case that run reduced.  Computed once; nobody writes to it."""
    inp = inputs(name, tied)
    return inp, {which: model(which, *operands(which, inp), inp.geom, inp.per_sample) for which in CASES[name].reduced}


@functools.lru_cache(maxsize=None)
def case_fp32(name):
    """The bf16x3 model of every reduced product accumulated in fp32 on the CPU (n3 of the host test is its distance from case()).  On
    torch's own blocked-GEMM convolution: oneDNN's fp32 weight gradient adds the pixels of a channel pair in one long chain and lies
    7.5e-7 ... 9.8e-7 from fp64 at 1445 ... 32768 pixels (cases D, S, E; 2.2e-7 ... 2.3e-7 here), which says nothing about the
    accumulation of a tiled GEMM such as the kernels'."""
    inp = inputs(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with torch.backends.mkldnn.flags(enabled=False):
            return {which: model(which, *operands(which, inp), inp.geom, inp.per_sample, dtype=torch.float32)['bf16x3']
                    for which in CASES[name].reduced}


# ------------------------------------------------------------------------------------------------------- the conv of a CPU reference block
class AmpConv2d(torch.autograd.Function):
    """conv2d without bias whose three products follow the model: mode None (exact), 'bf16' or 'bf16x3'.  The products are taken in fp64 and
    returned in the dtype of the input."""

    @staticmethod
    def forward(ctx, x, w, mode, stride, pad, dil):
        ctx.save_for_backward(x, w)
        ctx.conf = (mode, stride, pad, dil)
        geom = (x.shape[0], x.shape[2], x.shape[3], w.shape[1], w.shape[0], w.shape[2], stride, pad, dil)
        return model('forward', x.detach(), w.detach(), geom)[mode or 'exact'].to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        mode, stride, pad, dil = ctx.conf
        geom = (x.shape[0], x.shape[2], x.shape[3], w.shape[1], w.shape[0], w.shape[2], stride, pad, dil)
        dx = model('dgrad', dy, w.detach(), geom)[mode or 'exact'].to(x.dtype)
        dw = model('wgrad', x.detach(), dy, geom)[mode or 'exact'].to(w.dtype)
        return dx, dw, None, None, None, None


def use_amp_convs(module, mode):
    """Replace the forward (and with it the backward) of every dense bias-free nn.Conv2d of a CPU reference block by AmpConv2d in `mode`.
    -> the number of convs replaced."""
    n = 0
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d):
            assert m.groups == 1 and m.bias is None and m.kernel_size[0] == m.kernel_size[1], 'a dense square conv without bias'
            m.forward = functools.partial(_amp_forward, m, mode)
            n += 1
    return n


def _amp_forward(m, mode, x):
    return AmpConv2d.apply(x, m.weight, mode, m.stride[0], m.padding[0], m.dilation[0])
