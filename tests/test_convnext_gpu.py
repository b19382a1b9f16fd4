"""The large-kernel depthwise kernels (dwlk.hip) and the blocks on them on the MI355X: forward, data gradient and weight gradient for k = 7 and 9
under the channel-slice contract (tests/slices.py) against fp64 at the project's kernel bars (POINT / REDUCED, tests/support_kernels_ref.py),
every epilogue piece on and off, the statistics partials against fp64 sums, accumulation into dx / dw / db; LayerNorm_s, ConvNextBlock, CNeB,
ConvMix and CSPCM against torch autograd on the CPU restatement (tests/convnext_ref.py); the graphs of configs.yolov5_convnext_cfg against the
oracle Model.  tests/test_convnext_host.py holds the fp32 CPU reference to half of every kernel bar at every case used here."""
import copy

import pytest
import torch

import convnext_ref as R
from parity import (bn_hyper, check_block, check_checkpoint_roundtrip, check_eval, check_train_step, check_two_steps_bit_identical, nhwc, rel_close)
from slices import In, Out, check_slice_op
from support_kernels_ref import POINT, REDUCED

pytestmark = pytest.mark.gpu

IDS = lambda s: s if isinstance(s, str) else 'x'.join(map(str, s))     # noqa: E731
CASES = R.SHAPES + ['walk', 'walk_wgrad']


def test_walk_shapes_walk():
    """Every walking shape makes a workgroup walk two rows of strips under its plan, every plain shape one - so both forms of the loops are
    under test (tests/test_convnext_host.py holds that the walking shapes are the smallest that do)."""
    from somi_amd import ops
    assert ops.dwlk_strip_length() == R.STRIP
    for c in R.WIDTHS:
        assert ops.dwlk_strips_per_workgroup(*R.WALK_FWD[c], c) == 2 and ops.dwlk_strips_per_workgroup(*R.WALK_WGRAD[c], c, True) == 2, c
        assert all(ops.dwlk_strips_per_workgroup(*s, c) == 1 and ops.dwlk_strips_per_workgroup(*s, c, True) == 1 for s in R.SHAPES), c


def _case(c, k, shape):
    shape = {'walk': R.WALK_FWD[c], 'walk_wgrad': R.WALK_WGRAD[c]}.get(shape, shape)
    t = R.kernel_case(c, k, shape)
    return shape, t, {n: v.double() for n, v in t.items()}


def _packed(w, w_cs):
    from somi_amd.pack import pack_gconv_weight
    return pack_gconv_weight(w, w_cs)


@pytest.mark.parametrize('c', R.WIDTHS)
@pytest.mark.parametrize('shape', [s for s in CASES if s != 'walk_wgrad'], ids=IDS)
@pytest.mark.parametrize('k', R.KS)
def test_forward(k, shape, c):
    """y = post_scale * act(conv + bias) + post_shift + residual from a slice into a slice (the weights' row stride wider than the layer), every
    epilogue piece on its own, none and all of them; with statistics the pre-activation is written and the partial rows sum to the fp64 sums of
    (gelu(conv + bias) - pivot) and its square.  check_slice_op launches every form three times and holds the results bit-identical."""
    from somi_amd import ops
    (B, H, W), t, d = _case(c, k, shape)
    walk = shape == 'walk'
    cs_in, cs_out = (c + 4, c + 4) if walk else (c + 8, c + 12)
    wp = _packed(t['w'], c + 4)
    pre = R.dwlk_fwd_ref(d['x'], d['w'], d['bias'])
    forms = [dict(bias=1, act='gelu', post=1, res=1)] if walk else \
        [dict(), dict(bias=1), dict(act='gelu'), dict(post=1), dict(res=1), dict(bias=1, act='gelu', post=1, res=1)]
    for f in forms:
        want = R.dwlk_fwd_ref(d['x'], d['w'], d['bias'] if f.get('bias') else None, f.get('act', 'none'))
        if f.get('post'):
            want = want * d['ps'] + d['pt']
        if f.get('res'):
            want = want + d['res']

        def run(b, f=f):
            ops.dwlk(b['x'], b['w'], b['bias'] if f.get('bias') else None, c=c, k=k, x_coff=4, act=f.get('act', 'none'),
                     post_scale=b['ps'] if f.get('post') else None, post_shift=b['pt'] if f.get('post') else None, out=b['y'], o_coff=4,
                     residual=b['res'] if f.get('res') else None, res_coff=0)
        check_slice_op(run, dict(x=In(t['x'], cs_in, 4), w=wp, bias=t['bias'], ps=t['ps'], pt=t['pt'], res=In(t['res'], c + 4, 0)),
                       dict(y=Out((B, H, W), cs_out, 4, c)), dict(y=want), rel=POINT, what=f'dwlk k{k} c{c} {B}x{H}x{W} {sorted(f)}')
    g = R.gelu64(pre) - d['pivot']
    sums = dict(sum=g.sum((0, 1, 2)), sumsq=(g * g).sum((0, 1, 2)))
    for act, piv in (('gelu', True),) if walk else (('gelu', True), ('none', False)):
        if act == 'none':
            sums = dict(sum=pre.sum((0, 1, 2)), sumsq=(pre * pre).sum((0, 1, 2)))

        def run(b, act=act, piv=piv):
            st = {'pivot': b['pivot'] if piv else None}
            ops.dwlk(b['x'], b['w'], b['bias'], c=c, k=k, x_coff=4, act=act, out=b['y'], o_coff=4, bn_stats=st)
            assert st['rows'] == st['part'].shape[1] > 0
            return dict(sum=st['part'][0].double().sum(0), sumsq=st['part'][1].double().sum(0))
        check_slice_op(run, dict(x=In(t['x'], cs_in, 4), w=wp, bias=t['bias'], pivot=t['pivot']), dict(y=Out((B, H, W), cs_out, 4, c)),
                       dict(y=pre, **sums), rel=POINT, bars=dict(sum=REDUCED, sumsq=REDUCED), what=f'dwlk k{k} c{c} {B}x{H}x{W} statistics, {act}')


@pytest.mark.parametrize('c', R.WIDTHS)
@pytest.mark.parametrize('shape', [s for s in CASES if s != 'walk_wgrad'], ids=IDS)
@pytest.mark.parametrize('k', R.KS)
def test_data_gradient(k, shape, c):
    """dx = conv^T(dy): written; with acc1 and acc2 from other tensors; and added onto what dx holds (acc1 = dx)."""
    from somi_amd import ops
    (B, H, W), t, d = _case(c, k, shape)
    walk = shape == 'walk'
    cs_in, cs_out = (c + 4, c + 4) if walk else (c + 12, c + 8)
    wp = _packed(t['w'], c + 8)
    dx = R.dwlk_grads_ref(d['x'], d['w'], d['dy'])[0]
    what = f'dwlk dgrad k{k} c{c} {B}x{H}x{W}'
    if not walk:
        check_slice_op(lambda b: ops.dwlk_dgrad(b['dy'], b['w'], c=c, k=k, dy_coff=8, out=b['dx'], dx_coff=4),
                       dict(dy=In(t['dy'], cs_in, 8), w=wp), dict(dx=Out((B, H, W), cs_out, 4, c)), dict(dx=dx), rel=POINT, what=what)
        check_slice_op(lambda b: ops.dwlk_dgrad(b['dy'], b['w'], c=c, k=k, dy_coff=8, out=b['dx'], dx_coff=4, accumulate=b['a1'], acc_coff=4,
                                                accumulate2=b['a2'], acc2_coff=0),
                       dict(dy=In(t['dy'], cs_in, 8), w=wp, a1=In(t['acc'], c + 4, 4), a2=In(t['res'], c + 4, 0)),
                       dict(dx=Out((B, H, W), cs_out, 4, c)), dict(dx=dx + d['acc'] + d['res']), rel=POINT, what=what + ' + acc1 + acc2')
    check_slice_op(lambda b: ops.dwlk_dgrad(b['dy'], b['w'], c=c, k=k, dy_coff=4, out=b['dx'], dx_coff=4, accumulate=b['dx'], acc_coff=4),
                   dict(dy=In(t['dy'], cs_in, 4), w=wp), dict(dx=Out((B, H, W), cs_out, 4, c, prev=t['acc'], accumulate=True)), dict(dx=dx),
                   rel=POINT, what=what + ' onto dx')


@pytest.mark.parametrize('c', R.WIDTHS)
@pytest.mark.parametrize('shape', [s for s in CASES if s != 'walk'], ids=IDS)
@pytest.mark.parametrize('k', R.KS)
def test_weight_gradient(k, shape, c):
    """dw in the nn.Conv2d layout (c, 1, k, k) and db = the per-channel sum of dy from one pass: written over stale content, and added onto
    what they hold (accumulate); without a bias gradient dw is the same bits."""
    from somi_amd import ops
    (B, H, W), t, d = _case(c, k, shape)
    _, dw, db = R.dwlk_grads_ref(d['x'], d['w'], d['dy'])
    g = torch.Generator().manual_seed(c + k)
    dw0, db0 = torch.randn(c, 1, k, k, generator=g), torch.randn(c, generator=g)
    what = f'dwlk wgrad k{k} c{c} {B}x{H}x{W}'
    bars = dict(dw=REDUCED, db=REDUCED)

    def run(b, accumulate=False):
        gw, gb = ops.dwlk_wgrad(b['x'], b['dy'], c=c, k=k, x_coff=4, dy_coff=0, dw=b['dw0'], db=b['db0'], accumulate=accumulate)
        assert gw.data_ptr() == b['dw0'].data_ptr() and gb.data_ptr() == b['db0'].data_ptr()
        return dict(dw=gw, db=gb)
    ins = dict(x=In(t['x'], c + 8, 4), dy=In(t['dy'], c + 4, 0), dw0=dw0, db0=db0)
    first = check_slice_op(run, ins, {}, dict(dw=dw, db=db), bars=bars, what=what)
    if shape != 'walk_wgrad':
        check_slice_op(lambda b: run(b, True), ins, {}, dict(dw=dw + dw0.double(), db=db + db0.double()), bars=bars, what=what + ' accumulated')
        gw, gb = ops.dwlk_wgrad(t['x'].cuda(), t['dy'].cuda(), c=c, k=k, bias=False)
        assert gb is None and torch.equal(gw.cpu(), first['dw']), f'{what}: dw without db differs from dw with it'


def test_refusals_are_return_codes():
    """What the family cannot do comes back as an exception from the return code, before any launch: another k, channels that are no
    multiple of 4, an activation other than none / gelu, statistics together with a post-affine."""
    from somi_amd import ops
    x = torch.zeros(1, 4, 4, 8).cuda()
    w5, w9 = torch.zeros(25, 1, 8).cuda(), torch.zeros(81, 1, 8).cuda()
    with pytest.raises(RuntimeError, match='kernel size 5'):
        ops.dwlk(x, w5, c=8, k=5)
    with pytest.raises(RuntimeError, match='6 channels'):
        ops.dwlk(x, w9, c=6, k=9)
    with pytest.raises(RuntimeError, match='activation 1'):
        ops.dwlk(x, w9, c=8, k=9, act='silu')
    with pytest.raises(RuntimeError, match='with statistics the pre-activation is written'):
        ops.dwlk(x, w9, c=8, k=9, post_scale=torch.ones(8).cuda(), post_shift=torch.zeros(8).cuda(), bn_stats={})
    with pytest.raises(RuntimeError, match='kernel size 11'):
        ops.dwlk_wgrad(x, x, c=8, k=11)


# ---------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_blocks_eval_train_backward(tag):
    """Every fixture case: eval forward, training forward, dx, every parameter gradient (gamma's too: no_grad is empty), every running
    statistic.  The input seeds are convnext_ref.BLOCK_SEEDS, chosen from the restatement alone."""
    check_block(R.BLOCKS[tag], R, R.block_shape(tag), tag, seed=R.BLOCK_SEEDS[tag], no_grad=())


def test_layernorm_s_and_a_block_without_gamma():
    """LayerNorm_s on its own (forward, dx, both parameter gradients) and ConvNextBlock(layer_scale_init_value=0): gamma is None on both sides."""
    check_block(lambda ns: ns.LayerNorm_s(20), _NHWCNorm, (2, 20, 5, 7), 'layernorm_s', seed=0)
    check_block(lambda ns: ns.ConvNextBlock(16, 0., 0.), R, (2, 16, 5, 7), 'cnxblock_nogamma', seed=0)


class _NHWCNorm:
    """The namespace of the LayerNorm_s case: the restatement on an NCHW map (check_block feeds NCHW; the module itself is channels-last)."""

    class LayerNorm_s(R.LayerNorm_s):
        def forward(self, x):
            return super().forward(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


@pytest.mark.parametrize('tag', ['cnxblock', 'convmix_k7', 'cneb'])
def test_blocks_write_a_given_slice_and_add_into_a_given_gradient(tag):
    """forward(x, out=<slice>) in both modes leaves the channels around the slice alone (the leaf blocks; CNeB drives it inside);
    backward(dout, dx_out=have, accumulate=True) leaves R + dx in `have`; need_dx=False returns None and still takes the parameter gradients."""
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    ref, x, gen = R.block_case(tag)
    mine = R.BLOCKS[tag](MB)
    mine.load_state_dict(ref.state_dict())
    mine = bn_hyper(mine).cuda()
    c = x.shape[1]
    xd = nhwc(x).cuda()
    if tag != 'cneb':
        for mode in ('eval', 'train'):
            ref.train(mode == 'train'), mine.train(mode == 'train')
            with torch.no_grad():
                want = nhwc(ref(x))
            out = torch.full((*xd.shape[:3], c + 12), -77.0).cuda()
            got = mine(Act(xd.clone()), out=Act(out, 4, c))
            assert got.t.data_ptr() == out.data_ptr() and (got.coff, got.c) == (4, c)
            assert bool((out[..., :4] == -77.0).all()) and bool((out[..., 4 + c:] == -77.0).all()), f'{tag} {mode}: channels around the slice were written'
            rel_close(out[..., 4:4 + c], want, what=f'{tag} {mode} into a slice')
    mine.train()
    y = mine(Act(xd.clone()))
    dy = torch.randn(y.t.shape, generator=gen).cuda()
    dx = mine.backward(Act(dy.clone()))
    dx = dx.t[..., dx.coff:dx.coff + c].clone()
    mine(Act(xd.clone()))
    have = torch.randn(xd.shape, generator=gen).cuda()
    before = have.clone()
    got = mine.backward(Act(dy.clone()), dx_out=Act(have), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have, before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')
    mine(Act(xd.clone()))
    first = next(p for n, p in mine.named_parameters() if n.endswith(('dwconv.weight', 'Resnet.0.weight')))
    g = first.grad.clone()
    assert mine.backward(Act(dy.clone()), need_dx=False) is None and not torch.equal(first.grad, g), f'{tag}: need_dx=False'


@pytest.mark.parametrize('where', sorted(R.GRAPH_SEEDS))
def test_convnext_graph_training_step_eval_and_checkpoint(where, monkeypatch):
    """configs.yolov5_convnext_cfg at width 0.25 / depth 0.33, nc 4, batch 2, 64x64 against the oracle Model: one training forward, ComputeLoss
    and backward, the eval forward; two fresh TrainStep.step runs bit-identical; a pickled oracle model loads.  After one optimizer step every
    gamma is bit-identical to its loaded value while its gradient is non-zero (it is in none of the optimizer's groups, train.py:125-133), and
    the depthwise weights have moved.  Seeds: convnext_ref.GRAPH_SEEDS."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd import blocks as MB
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    R.register(monkeypatch)
    cfg, ref, imgs, targets = R.graph_case(where)
    state = copy.deepcopy(ref.state_dict())
    mine = Model(cfg)
    mine.load_state_dict(state)
    mine.hyp = dict(HYP_VISDRONE)
    kinds = {type(sub) for i in (2, 4, 6, 8) for sub in ([mine.model[i]] if not isinstance(mine.model[i], MB.Repeat) else list(mine.model[i]))}
    assert kinds == {MB.CNeB if where == 'cneb' else MB.CSPCM}
    check_train_step(ref, mine, imgs, targets, f'yolov5s-{where}')
    check_eval(ref, mine, imgs, f'yolov5s-{where}')
    assert mine.fuse() is mine
    check_two_steps_bit_identical(cfg, state, imgs, targets, 2)
    check_checkpoint_roundtrip(ref, imgs, ('oracle', 'convnext_ref'), f'yolov5s-{where}')
    m = Model(cfg)
    m.load_state_dict(state)
    tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), 2)
    gammas = {n: p for n, p in m.named_parameters() if n.endswith('.gamma')}
    assert len(gammas) == (7 if where == 'cneb' else 0)
    seen, real = {}, tr.optimizer.step

    def spy():                                                   # the gradients as the optimizer meets them (zero_grad drops them afterwards)
        seen.update({n: None if p.grad is None else p.grad.clone() for n, p in gammas.items()})
        real()
    tr.optimizer.step = spy
    loss, _ = tr.step(imgs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all(), f'the loss of a step is not finite: {loss.tolist()}'
    after = m.state_dict()
    moved = [k for k in state if k.endswith(('dwconv.weight', 'Resnet.0.weight'))]
    assert len(moved) == 7, len(moved)                             # n = 1, 2, 3, 1 blocks in the four swapped rows, inside or as repeats
    for k in moved:
        assert not torch.equal(after[k].cpu(), state[k]), f'a step left {k} where it was'
    assert set(seen) == set(gammas)
    ema = tr.optimizer.ema_state_dict()
    for n in gammas:
        assert torch.equal(after[n].cpu(), state[n]), f'a step moved {n}, which is in no optimizer group'
        assert seen[n] is not None and bool(seen[n].any()), f'{n} took no gradient'
        assert torch.equal(ema[n].cpu(), state[n]), f'the EMA state does not carry {n} as loaded'


@pytest.mark.parametrize('sgd', [False, True], ids=['adam', 'sgd'])
def test_gamma_stays_outside_the_flat_buffers_of_both_optimizer_forms(sgd):
    """FusedAdamEMA in its Adam and its SGD form on a CNeB: gamma's storage and gradient lie in none of the flat buffers, a step with a
    non-zero gradient everywhere leaves it bit for bit and moves the depthwise weight, the EMA state dict and the model's own state dict (what a
    checkpoint saves) carry its value, and zero_grad drops its gradient."""
    from somi_amd import blocks as MB
    from somi_amd.optim import FusedAdamEMA
    ref, _, _ = R.block_case('cneb')
    blk = R.BLOCKS['cneb'](MB)
    blk.load_state_dict(ref.state_dict())
    blk = blk.cuda()
    opt = FusedAdamEMA(blk, lr=1e-2, weight_decay=1e-2, sgd=sgd)
    names = {id(p): n for n, p in blk.named_parameters()}
    assert sorted(names[id(p)] for p in opt._ungrouped) == ['m.0.gamma', 'm.1.gamma']
    spans = [(b.data_ptr(), b.data_ptr() + 4 * b.numel()) for b in opt.flat_params + opt.flat_grads]
    before = {n: p.detach().clone() for n, p in blk.named_parameters()}
    for n, p in blk.named_parameters():
        inside = any(lo <= p.data_ptr() < hi for lo, hi in spans)
        assert inside == (not n.endswith('gamma')), f'{n}: storage inside a flat buffer: {inside}'
        if p.grad is None:
            p.grad = torch.ones_like(p)
        else:
            p.grad.fill_(1.0)
    opt.step()
    torch.cuda.synchronize()
    ema, sd = opt.ema_state_dict(), blk.state_dict()
    for n, p in blk.named_parameters():
        if n.endswith('gamma'):
            assert torch.equal(p.detach(), before[n]) and torch.equal(ema[n], before[n]) and torch.equal(sd[n], before[n]), f'{n} moved or is not carried'
        else:
            assert not torch.equal(p.detach(), before[n]), f'the step left {n} where it was'
    opt.zero_grad()
    assert all(p.grad is None for n, p in blk.named_parameters() if n.endswith('gamma'))
