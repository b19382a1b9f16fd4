"""The parity procedures of the GPU tests, once: the comparison bar (rel_close), the layout helpers, the block procedure (check_block) and the
graph procedure (check_train_step, check_eval, check_two_steps_bit_identical, check_checkpoint_roundtrip).  A plain module, imported like
ghost_ref / hub_ref / yolov10_ref; pytest does not rewrite its asserts, so every assert carries its own message."""
import copy
import io

import torch
import torch.nn as nn


def rel_close(got, want, rel=1e-3, what='', atol=0.0, floor=1e-12):
    """max |got - want| <= rel * (max |want| + floor) + atol, on equal shapes and a finite `got`; prints the error and the scale."""
    got, want = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(want).detach().cpu().double()
    assert got.shape == want.shape, f'{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}'
    assert torch.isfinite(got).all(), f'{what}: not finite'
    err = (got - want).abs().max().item()
    scale = want.abs().max().item() + floor
    print(f'{what}: max err {err:.3e}, scale {scale:.3e}')
    assert err <= rel * scale + atol, f'{what}: max err {err:.3e} vs scale {scale:.3e} (bar {rel * scale + atol:.3e})'


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def bn_hyper(mod):
    """The reference's BatchNorm hyperparameters (initialize_weights sets them on the oracle; a state dict does not carry them)."""
    for m in mod.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.03
    return mod


def _channels(a):
    return a.t[..., a.coff:a.coff + a.c]


def grads_close(mine, ref, what, no_grad=()):
    """Every parameter gradient against the oracle's.  Every oracle parameter has one, except the names in `no_grad`: there ours has none
    either, or a zero one.  atol: gradients that are analytically zero (e.g. a bias in front of a batch-norm) are rounding noise on both sides."""
    ours, theirs = list(mine.named_parameters()), list(ref.named_parameters())
    assert [n for n, _ in ours] == [n for n, _ in theirs], f'{what}: parameter names differ: {[n for n, _ in ours]} vs {[n for n, _ in theirs]}'
    for (n, p), (_, q) in zip(ours, theirs):
        if n in no_grad:
            assert q.grad is None, f'{what}: {n} is listed as without a gradient, but the oracle has one'
            assert p.grad is None or not p.grad.any(), f'{what}: {n} has a gradient (max {p.grad.abs().max().item():.3e}) where the oracle has none'
            continue
        assert q.grad is not None, f'{what}: the oracle left {n} without a gradient'
        assert p.grad is not None, f'{what}: {n} has no gradient'
        rel_close(p.grad, q.grad, what=f'{what}: d{n}', atol=2e-5)


def buffers_close(mine, ref, what, rel=1e-3):
    """Every running_* buffer at the bar, every num_batches_tracked equal."""
    ours, theirs = list(mine.named_buffers()), list(ref.named_buffers())
    assert [n for n, _ in ours] == [n for n, _ in theirs], f'{what}: buffer names differ: {[n for n, _ in ours]} vs {[n for n, _ in theirs]}'
    for (n, p), (_, q) in zip(ours, theirs):
        if 'running' in n:
            rel_close(p, q, rel=rel, what=f'{what}: {n}')
        elif 'num_batches_tracked' in n:
            assert int(p) == int(q), f'{what}: {n} is {int(p)}, the oracle\'s {int(q)}'


def check_built_block(ref, mine, x, gen, tag, *, eval_too=True, no_grad=(), device='cuda'):
    """The block procedure on a built pair that holds the same state: `ref` a CPU module under torch autograd, `mine` the hand-written block
    (forward and backward on an Act).  x: the NCHW input, gen: the generator the output gradient is drawn from.  Eval forward (when
    `eval_too`), training forward, dx over dx.coff : dx.coff + cin, every parameter gradient (grads_close), every running statistic and
    every num_batches_tracked."""
    from somi_amd.blocks import Act
    mine = bn_hyper(mine).to(device)
    x = x.detach().clone().requires_grad_(True)

    def act(t):
        return Act(nhwc(t.detach()).to(device))
    if eval_too:
        ref.eval(), mine.eval()
        with torch.no_grad():
            rel_close(_channels(mine(act(x))), nhwc(ref(x)), what=f'{tag} eval')
    ref.train(), mine.train()
    y = ref(x)
    dy = torch.randn(y.shape, generator=gen)
    y.backward(dy)
    rel_close(_channels(mine(act(x))), nhwc(y), what=f'{tag} train forward')
    dx = mine.backward(act(dy))
    rel_close(dx.t[..., dx.coff:dx.coff + x.shape[1]], nhwc(x.grad), what=f'{tag} dx')
    grads_close(mine, ref, tag, no_grad)
    buffers_close(mine, ref, tag)


def check_block(make, ref_ns, shape, tag, *, seed=None, shift=0.0, eval_too=True, no_grad=(), device='cuda'):
    """check_built_block on make(ref_ns) against make(somi_amd.blocks): the oracle filled by fill_state(ref, 5) + initialize_weights, input and
    output gradient from one generator seeded with `seed` (len(tag) when None), the input shifted by `shift`."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    ref, mine = make(ref_ns), make(MB)
    fill_state(ref, 5)
    OB.initialize_weights(ref)
    mine.load_state_dict(ref.state_dict())
    gen = torch.Generator().manual_seed(len(tag) if seed is None else seed)
    x = torch.randn(*shape, generator=gen) + shift
    check_built_block(ref, mine, x, gen, tag, eval_too=eval_too, no_grad=no_grad, device=device)


def check_train_step(ref, mine, imgs, targets, what):
    """One training forward, ComputeLoss and backward of the oracle Model on the CPU against ours: outputs, loss and loss items (1e-4), every
    parameter gradient against 2e-3 * scale + 2e-6, the running statistics.  -> the oracle's training outputs."""
    from oracle.somi_ref.loss import ComputeLoss as OLoss
    from somi_amd.loss import ComputeLoss
    ref.train()
    pr = ref(imgs.float() / 255)
    lr, ir = OLoss(ref)(pr, targets)
    lr.backward()
    mine.cuda().train()
    pm = mine(imgs.cuda())
    assert len(pm) == len(pr), f'{what}: {len(pm)} training outputs, the oracle has {len(pr)}'
    for a, b in zip(pm, pr):
        rel_close(a, b, what=f'{what} train outputs')
    lm, im = ComputeLoss(mine)(pm, targets.cuda())
    rel_close(lm, lr, rel=1e-4, what=f'{what} loss')
    rel_close(im, ir, rel=1e-4, what=f'{what} loss items')
    lm.backward()
    ours, theirs = list(mine.named_parameters()), list(ref.named_parameters())
    assert [n for n, _ in ours] == [n for n, _ in theirs], f'{what}: parameter names differ from the oracle\'s'
    bad, worst = [], 0.0
    for (n, p), (_, q) in zip(ours, theirs):
        assert q.grad is not None and p.grad is not None, f'{what}: {n} has no gradient (oracle: {q.grad is not None}, ours: {p.grad is not None})'
        err = (p.grad.cpu().double() - q.grad.double()).abs().max().item()
        scale = q.grad.double().abs().max().item() + 1e-9
        worst = max(worst, err / (2e-3 * scale + 2e-6))
        if not err <= 2e-3 * scale + 2e-6:
            bad.append((n, err, scale))
    print(f'{what}: worst parameter gradient at {worst:.3f} x the bar')
    assert not bad, f'{what}: {len(bad)} parameter gradients beyond 2e-3 * scale + 2e-6 (name, err, scale): {bad[:8]}'
    buffers_close(mine, ref, what)
    return pr


def check_eval(ref, mine, imgs, what):
    """The eval forward against the oracle's.  -> our predictions."""
    mine.cuda()
    ref.eval(), mine.eval()
    with torch.no_grad():
        zr, _ = ref(imgs.float() / 255)
        z, _ = mine(imgs.cuda())
    rel_close(z, zr, what=f'{what} z')
    return z


def check_two_steps_bit_identical(cfg, state, imgs, targets, batch):
    """Two fresh TrainStep.step runs from `state`: a finite loss; loss, gradients (taken right before optimizer.step) and the state after the
    step equal bit for bit; the step changed at least one conv weight."""
    from oracle.somi_ref.testing import HYP_VISDRONE
    from somi_amd.model import Model
    from somi_amd.train import TrainStep
    runs = []
    for _ in range(2):
        m = Model(cfg)
        m.load_state_dict(state)
        tr = TrainStep(m.cuda(), dict(HYP_VISDRONE), batch)
        grads, real = [], tr.optimizer.step

        def spy(real=real, grads=grads, tr=tr):
            grads.extend(g.clone() for g in tr.optimizer.flat_grads)
            real()
        tr.optimizer.step = spy
        loss, _ = tr.step(imgs.cuda(), targets.cuda())
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), grads, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    (l0, g0, s0), (l1, g1, s1) = runs
    assert torch.isfinite(l0).all(), f'the loss of a training step is not finite: {l0.tolist()}'
    assert torch.equal(l0, l1), f'the loss differs between two identical steps: {l0.tolist()} vs {l1.tolist()}'
    assert len(g0) == len(g1) and len(g0) > 0, f'optimizer.step saw {len(g0)} and {len(g1)} gradient buffers'
    differ = [i for i, (a, b) in enumerate(zip(g0, g1)) if not torch.equal(a, b)]
    assert not differ, f'gradients differ between two identical steps: flat buffers {differ}'
    differ = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not differ, f'state differs between two identical steps: {differ[:5]}'
    convs = [k for k in state if k.endswith('cv2.weight') or k.endswith('conv.weight')]
    assert any(not torch.equal(s0[k].cpu(), state[k]) for k in convs), f'the step changed none of {len(convs)} conv weights'


def check_checkpoint_roundtrip(ref, imgs, foreign_prefixes, what):
    """attempt_load of a pickled half-precision oracle model reproduces the eval forward of that half-precision model."""
    from somi_amd.checkpoint import attempt_load
    buf = io.BytesIO()
    torch.save({'epoch': 1, 'model': copy.deepcopy(ref).half(), 'ema': None}, buf)
    loaded, info = attempt_load(buf.getvalue(), foreign_prefixes=foreign_prefixes)
    assert info['used'] == 'model' and not loaded.training, f'{what}: attempt_load used {info["used"]!r}, training={loaded.training}'
    want_model = copy.deepcopy(ref).half().float().eval()
    with torch.no_grad():
        rel_close(loaded(imgs.cuda())[0], want_model(imgs.float() / 255)[0], what=f'{what} z from the loaded checkpoint')


def check_accumulate_contract(block, x, c, gen, tag, device='cuda'):
    """The accumulate contract of a block that declares it (`accumulates`), on a deep copy of the built `block`: a training forward and
    backward(dy) give dx; the same forward again and backward(dy, dx_out=have, accumulate=True) must leave R + dx in have[..., :c], where `have`
    is a whole padded contiguous tensor drawn from `gen` (pad channels zero) and R what it held before the call.
    x: the NHWC input (pad4(c) wide, pad channels zero), c its logical channels."""
    from somi_amd.blocks import Act, pad4
    blk = bn_hyper(copy.deepcopy(block)).to(device).train()
    assert type(blk).accumulates, f'{tag}: {type(blk).__name__} does not declare the accumulate contract'
    x = x.to(device)
    y = blk(Act(x.clone(), 0, c))
    dy = torch.randn(y.t.shape, generator=gen)
    dy[..., y.coff + y.c:] = 0
    dy = dy.to(device)
    dx = blk.backward(Act(dy.clone(), y.coff, y.c))
    dx = dx.t[..., dx.coff:dx.coff + c].clone()
    blk(Act(x.clone(), 0, c))
    have = torch.randn(*x.shape[:3], pad4(c), generator=gen)
    have[..., c:] = 0
    have = have.to(device)
    before = have[..., :c].clone()
    got = blk.backward(Act(dy.clone(), y.coff, y.c), dx_out=Act(have, 0, c), accumulate=True)
    assert got.t.data_ptr() == have.data_ptr() and got.coff == 0, f'{tag}: backward(dx_out=) returned another tensor'
    rel_close(have[..., :c], before + dx, what=f'{tag}: dx_out after backward(accumulate=True) against R + dx')
