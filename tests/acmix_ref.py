"""Plain-PyTorch restatement of the reference's ACmix (models/common.py:7281-7365), the CPU oracle of tests/test_acmix_host.py and
tests/test_acmix_gpu.py, written from its semantics - the literal formula, with unfold:

  * q, k, v are three 1x1 convs (with bias) of the input; 4 heads, head h owns the channels [h D, (h + 1) D), D = out_planes / 4;
  * pe = conv_p(position map), the position map being the 2-channel (x, y) grid of linspace(-1, 1); it is built in the module's dtype here (the
    reference's helper is fp32 only, so the reference class cannot run in fp64);
  * per head and pixel the 49 scores s * q . (k_j + pe_p - pe_j) over the 7x7 window, reflection-padded by 3, are soft-maxed and weigh v_j;
  * fc, a bias-free 1x1 conv over the 12 maps (q heads, k heads, v heads) of every head dim, feeds dep_conv, a 3x3 conv with D groups of 9 inputs and
    4 outputs; the reference's reset_parameters leaves dep_conv without a bias (it assigns the None its init_rate_0 helper returns);
  * out = rate1 * att + rate2 * conv.
tests/golden/block_acmix*.npz, generated from the reference's own class, pin all of that.

register(monkeypatch) teaches the oracle's parse_model the name for the length of a test.  The kernel-level references (fp64, or fp32 for the host
test's half-bar check) of acmix.hip, the block cases and the graph cases follow."""
import copy
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


def position(H, W, dtype=torch.float32, device=None):
    loc_w = torch.linspace(-1.0, 1.0, W, dtype=dtype, device=device).unsqueeze(0).repeat(H, 1)
    loc_h = torch.linspace(-1.0, 1.0, H, dtype=dtype, device=device).unsqueeze(1).repeat(1, W)
    return torch.stack([loc_w, loc_h], 0).unsqueeze(0)


def window(t):
    """(N, D, H, W) -> (N, D, 49, H, W): the 7x7 window around every pixel, reflection-padded."""
    N, D, H, W = t.shape
    return F.unfold(F.pad(t, (3, 3, 3, 3), mode='reflect'), 7).view(N, D, 49, H, W)


def scores_from_pe(q, k, pe, head=4):
    """The reference's scores: (B head, 49, H, W) from q, k (B, C, H, W) and pe (1, D, H, W)."""
    B, C, H, W = q.shape
    D = C // head
    qa = q.reshape(B * head, D, H, W) * float(D) ** -0.5
    return (qa.unsqueeze(2) * (window(k.reshape(B * head, D, H, W)) + pe.unsqueeze(2) - window(pe))).sum(1)


def attention(q, k, v, wp, head=4):
    """-> (att (B, C, H, W), scores (B head, 49, H, W)); wp: conv_p.weight as (D, 2) - conv_p.bias cancels in pe_p - pe_j."""
    B, C, H, W = q.shape
    D = C // head
    pe = F.conv2d(position(H, W, q.dtype, q.device), wp.reshape(D, 2, 1, 1))
    sc = scores_from_pe(q, k, pe, head)
    a = F.softmax(sc, 1)
    return (a.unsqueeze(1) * window(v.reshape(B * head, D, H, W))).sum(2).view(B, C, H, W), sc


def conv_half(q, k, v, fc, dep, bias=None, head=4):
    """dep_conv(fc(.)) the reference's way: fc (9, 12), dep (C, 9, 3, 3)."""
    B, C, H, W = q.shape
    D = C // head
    f_all = F.conv2d(torch.cat([t.reshape(B, head, D, H * W) for t in (q, k, v)], 1), fc.reshape(9, 3 * head, 1, 1))
    return F.conv2d(f_all.permute(0, 2, 1, 3).reshape(B, -1, H, W), dep, bias, padding=1, groups=D)


def fold_weff(fc, dep):
    """(9, 12), (C, 9, 3, 3) -> the grouped 3x3 weight (C, 12, 3, 3) of D groups: Weff[c, t, tap] = sum_j dep[c, j, tap] * fc[j, t]."""
    return torch.einsum('cjyx,jt->ctyx', dep, fc.reshape(9, 12))


def conv_half_folded(q, k, v, weff, bias=None, head=4):
    """The conv half as ONE grouped conv: group d reads the d-th dim of the 12 sources."""
    B, C, H, W = q.shape
    D = C // head
    src = torch.cat([t.reshape(B, head, D, H, W) for t in (q, k, v)], 1)           # (B, 12, D, H, W)
    return F.conv2d(src.permute(0, 2, 1, 3, 4).reshape(B, 12 * D, H, W), weff, bias, padding=1, groups=D)


def weff_kernel_layout(weff):
    """(C, 12, 3, 3) -> (12, 9, D, 4), what acmix.hip reads."""
    C = weff.shape[0]
    return weff.reshape(C // 4, 4, 12, 9).permute(2, 3, 0, 1).contiguous()


class ACmix(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_att=7, head=4, kernel_conv=3, stride=1, dilation=1):
        super().__init__()
        assert (kernel_att, head, kernel_conv, stride, dilation) == (7, 4, 3, 1, 1)
        self.out_planes, self.head, self.head_dim = out_planes, head, out_planes // head
        self.rate1 = nn.Parameter(torch.Tensor(1))
        self.rate2 = nn.Parameter(torch.Tensor(1))
        self.conv1 = nn.Conv2d(in_planes, out_planes, 1)
        self.conv2 = nn.Conv2d(in_planes, out_planes, 1)
        self.conv3 = nn.Conv2d(in_planes, out_planes, 1)
        self.conv_p = nn.Conv2d(2, self.head_dim, 1)
        self.fc = nn.Conv2d(3 * head, 9, 1, bias=False)
        self.dep_conv = nn.Conv2d(9 * self.head_dim, out_planes, 3, bias=True, groups=self.head_dim, padding=1)
        self.rate1.data.fill_(0.5)
        self.rate2.data.fill_(0.5)
        kernel = torch.zeros(9, 3, 3)
        for i in range(9):
            kernel[i, i // 3, i % 3] = 1.
        self.dep_conv.weight = nn.Parameter(kernel.repeat(out_planes, 1, 1, 1))
        self.dep_conv.bias = None

    def forward(self, x):
        q, k, v = self.conv1(x), self.conv2(x), self.conv3(x)
        B, C, H, W = q.shape
        pe = self.conv_p(position(H, W, x.dtype, x.device))
        a = F.softmax(scores_from_pe(q, k, pe, self.head), 1)
        att = (a.unsqueeze(1) * window(v.reshape(B * self.head, self.head_dim, H, W))).sum(2).view(B, C, H, W)
        conv = conv_half(q, k, v, self.fc.weight, self.dep_conv.weight, self.dep_conv.bias, self.head)
        return self.rate1 * att + self.rate2 * conv


def register(monkeypatch):
    """'ACmix' in the oracle's parse_model (test-time only: nothing under oracle/ changes).  The reference's branch (models/yolo.py:1496-1501)
    scales the named width; in both yolov5_acmix_cfg graphs that is the input's width too, so the row stands in the oracle's pass as an nn.Upsample
    row of scale 1 (c2 = ch[f]) and is then replaced by ACmix(c2, c2, ...)."""
    from oracle.somi_ref import model as OM
    inner = OM.parse_model

    def parse_model(d, ch):
        rows = d['backbone'] + d['head']
        swapped = dict(d, backbone=[], head=[[f, n, 'nn.Upsample', [None, 1, 'nearest']] if name == 'ACmix' else [f, n, name, args]
                                             for f, n, name, args in rows])
        seq, save = inner(swapped, ch)
        layers = list(seq)
        for i, (f, n, name, args) in enumerate(rows):
            if name == 'ACmix':
                c2 = -(-args[0] * d['width_multiple'] // 8) * 8
                c2 = int(c2)
                m_ = ACmix(c2, c2, *args[1:])
                m_.i, m_.f, m_.type = i, f, name
                m_.np = sum(p.numel() for p in m_.parameters())
                layers[i] = m_
        return nn.Sequential(*layers), save
    monkeypatch.setattr(OM, 'parse_model', parse_model)


def oracle_model(cfg):
    """The oracle Model of a yolov5_acmix_cfg; the caller has run register(monkeypatch)."""
    from oracle.somi_ref import Model as OModel
    return OModel(copy.deepcopy(cfg))


# ---------------------------------------------------------------------------------------------- the seeded cases
# tools/gen_acmix_golden.py --seeds prints, per candidate, the fp32 CPU restatement's worst parameter gradient against its fp64 twin in units of the
# bar its test applies; tests/test_acmix_host.py asserts half the bar on the ones taken here.  conv_p.bias is the parameter to watch: its true
# gradient is zero, autograd leaves rounding noise there and the path leaves an exact zero.  Blocks, input seeds 0..2, both rate settings: 0.002 ..
# 0.039 of 1e-3 * scale + 2e-5, outputs <= 6.8e-7 and dx <= 5.6e-7 of their largest value; seed 0 is taken.  Graphs, (fill, batch) in (1..3) x (0, 1):
# 'row' 0.026 .. 0.050 of 2e-3 * scale + 2e-6, 'p3' 0.084 .. 0.226; (1, 0) and (3, 0) are taken (0.032 and 0.084).
BLOCKS = {                         # tag -> (constructor over a namespace, NCHW shape)
    'acmix32': (lambda ns: ns.ACmix(32, 32), (2, 32, 5, 7)),
    'acmix16to32': (lambda ns: ns.ACmix(16, 32), (1, 16, 9, 4)),
    'acmix64_min': (lambda ns: ns.ACmix(64, 64), (2, 64, 4, 4)),
}
RATES = ('filled', 'half')         # the rates fill_state draws (small: the conv half nearly vanishes from the output), and both at 0.5
BLOCK_SEEDS = {'acmix32': 0, 'acmix16to32': 0, 'acmix64_min': 0}
GRAPH_SEEDS = {'row': (1, 0), 'p3': (3, 0)}         # where -> (fill_state seed, synthetic_batch seed)
GRAPH_SIZE = {'row': 128, 'p3': 64}                 # 'row': 256 channels on the minimal 4x4 map; 'p3': 64 channels at 8x8
GRAPH_WIDTH, GRAPH_NC = 0.25, 4


def block_case(tag, rates='filled', seed=None):
    """-> (the filled oracle block, the input, the generator for the output gradient), as parity.check_block forms them."""
    from oracle.somi_ref.testing import fill_state
    make, shape = BLOCKS[tag]
    ref = make(sys.modules[__name__])
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    if rates == 'half':
        with torch.no_grad():
            ref.rate1.fill_(0.5)
            ref.rate2.fill_(0.5)
    gen = torch.Generator().manual_seed(BLOCK_SEEDS[tag] if seed is None else seed)
    return ref, torch.randn(*shape, generator=gen), gen


def graph_case(where, seeds=None):
    """-> (cfg, the filled oracle model, images, targets) of the graph test: yolov5_acmix_cfg at width 0.25, nc 4, batch 2."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_acmix_cfg
    fill, batch = GRAPH_SEEDS[where] if seeds is None else seeds
    cfg = yolov5_acmix_cfg(GRAPH_WIDTH, 0.33, nc=GRAPH_NC, where=where)
    ref = fill_state(oracle_model(cfg), fill)
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, GRAPH_SIZE[where], nc=GRAPH_NC, seed=batch)
    return cfg, ref, imgs, targets


def worst_grad_ratio(ref, ref64, rel, atol):
    """The fp32 module's worst parameter gradient against its fp64 twin's, in units of rel * scale + atol."""
    worst = 0.0
    for (_, p), (_, q) in zip(ref.named_parameters(), ref64.named_parameters()):
        scale = q.grad.abs().max().item() + 1e-9
        worst = max(worst, (p.grad.double() - q.grad).abs().max().item() / (rel * scale + atol))
    return worst


# ---------------------------------------------------------------------------------------------- kernel-level references (NHWC)
# (B, H, W, C): the smallest legal map with D = 4 (most taps reflect); one axis minimal, the other with interior pixels; odd sizes; the window equal
# to the map; two 8x8 workgroup tiles with a ragged edge on both axes; D = 128 and 256, the chunked-d path (16 values of d per head at a time);
# D = 20, a last chunk of 4.  'peaked' runs at D = 20 and not at D = 128: there the fp32 restatement itself is at 0.6 of POINT in dq and dk
KERNEL_SHAPES = [(2, 4, 4, 16), (1, 4, 9, 32), (1, 9, 4, 32), (2, 5, 7, 32), (1, 7, 7, 64), (2, 11, 13, 64), (1, 5, 6, 512), (1, 4, 5, 1024),
                 (1, 5, 6, 80)]
TILED_SHAPE = (2, 11, 13, 64)
KERNEL_CASES = ([(s, 'plain') for s in KERNEL_SHAPES] +
                [(s, 'peaked') for s in ((2, 5, 7, 32), TILED_SHAPE, (1, 5, 6, 80))] + [(s, 'pe') for s in ((2, 5, 7, 32), TILED_SHAPE, (1, 5, 6, 512))] +
                [((2, 5, 7, 32), 'rate1_0'), ((2, 5, 7, 32), 'rate2_0')])
CASE_IDS = ['x'.join(map(str, c[0])) + '-' + c[1] for c in KERNEL_CASES]
PEAKED_SCORE, PE_SCALE = 100.0, 30.0          # 'peaked': the largest q . k score; exp overflows in fp32 beyond 88.7


def kernel_inputs(shape, kind='plain', seed=None):
    """The fp32 inputs of the kernels.  kind: 'plain'; 'peaked': q and k scaled so that the largest probability exceeds 0.99 and a softmax without
    the maximum subtracted overflows; 'pe': Wp scaled so that the position term dominates the scores; 'rate1_0' / 'rate2_0': that rate is zero."""
    B, H, W, C = shape
    D = C // 4
    gen = torch.Generator().manual_seed(sum(shape) * 7 + len(kind) if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    t = dict(q=r(B, H, W, C), k=r(B, H, W, C), v=r(B, H, W, C), dout=r(B, H, W, C), wp=0.5 * r(D, 2), fc=r(9, 12) / 12 ** 0.5,
             dep=r(C, 9, 3, 3) / 3.0, bias=0.1 * r(C), rate1=torch.tensor([0.7]), rate2=torch.tensor([-0.4]),
             have_q=r(B, H, W, C), have_k=r(B, H, W, C), have_v=r(B, H, W, C))
    if kind == 'peaked':
        top = scores_from_pe(_nchw(t['q']), _nchw(t['k']), torch.zeros(1, D, H, W)).max().item()
        f = (PEAKED_SCORE / top) ** 0.5
        t['q'], t['k'] = f * t['q'], f * t['k']
    if kind == 'pe':
        t['wp'] = PE_SCALE * t['wp']
    if kind == 'rate1_0':
        t['rate1'] = torch.zeros(1)
    if kind == 'rate2_0':
        t['rate2'] = torch.zeros(1)
    return t


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def kernel_reference(t, dtype=torch.float64):
    """Results of the kernels in `dtype`, the backward by autograd of the literal formula (unfold; pe from conv_p's weight):
    att half: out_att = rate1 * att, out = rate1 * att + rate2 * mix, lse (B, H, W, 4), dq / dk / dv (the attention's share), dwp, drate1;
    conv half: weff (12, 9, D, 4), mix (with bias), cq / ck / cv (its data gradient), dweff (kernel layout), dbias, dfc, ddep, drate2."""
    lv = {n: t[n].to(dtype).clone().requires_grad_(True) for n in ('q', 'k', 'v', 'wp', 'fc', 'dep', 'bias', 'rate1', 'rate2')}
    q, k, v = (_nchw(lv[n]) for n in ('q', 'k', 'v'))
    B, C, H, W = q.shape
    dout = _nchw(t['dout'].to(dtype))
    att, sc = attention(q, k, v, lv['wp'])
    weff = fold_weff(lv['fc'], lv['dep'])
    mix = conv_half_folded(q, k, v, weff, lv['bias'])
    names = ('q', 'k', 'v', 'wp', 'rate1')
    ga = dict(zip(names, torch.autograd.grad(lv['rate1'] * att, [lv[n] for n in names], dout, retain_graph=True)))
    names = ('q', 'k', 'v', 'fc', 'dep', 'bias', 'rate2')
    gs = torch.autograd.grad(lv['rate2'] * mix, [lv[n] for n in names] + [weff], dout)
    gc, dweff = dict(zip(names, gs)), gs[-1]
    with torch.no_grad():
        literal = conv_half(q, k, v, lv['fc'], lv['dep'], lv['bias'])
        want = dict(out_att=_nhwc(lv['rate1'] * att), out=_nhwc(lv['rate1'] * att + lv['rate2'] * mix), mix=_nhwc(mix), mix_literal=_nhwc(literal),
                    lse=torch.logsumexp(sc, 1).view(B, 4, H, W).permute(0, 2, 3, 1).contiguous(), scores=sc,
                    dq=ga['q'], dk=ga['k'], dv=ga['v'], dwp=ga['wp'], drate1=ga['rate1'],
                    cq=gc['q'], ck=gc['k'], cv=gc['v'], dfc=gc['fc'], ddep=gc['dep'], dbias=gc['bias'], drate2=gc['rate2'],
                    weff=weff_kernel_layout(weff), dweff=weff_kernel_layout(dweff))
    return {n: x.detach() for n, x in want.items()}
