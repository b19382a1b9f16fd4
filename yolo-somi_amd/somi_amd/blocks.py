"""SOMI building blocks executing on libsomi_hip.so (NHWC fp32, MI355X).

Each class keeps the reference's constructor signature and parameter names (so reference-format yaml and
state_dicts load unchanged) but its forward launches HIP kernels through the C ABI:
Conv+BN+SiLU is ONE implicit-GEMM launch with the BN folded into the packed weights (eval), `torch.cat` never
happens (producers write channel slices of the consumer's buffer), nearest upsampling is folded into the BiFPN
read and the CBAM scaling into the following conv's operand load.

Activations travel as `Act` = (NHWC tensor, channel offset, logical channels).  Channel strides are multiples of 4;
padded channels hold zeros (zero weight rows in the producer), so consumers may read them.
Reference citations are relative to /root/reference.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .pack import pack_conv_weight, pack_dgrad_weight, pack_gconv_weight, pad4, bn_fold


class Act:
    """A channel slice [coff, coff+c) of an NHWC tensor."""
    __slots__ = ('t', 'coff', 'c', 'up', 'pooled', 'pool')

    def __init__(self, t, coff=0, c=None, up=0):
        self.t, self.coff, self.c, self.up = t, coff, (t.shape[3] - coff if c is None else c), up
        # a GRADIENT may carry a part that is constant over an image's pixels and not yet added to the tensor: (davg, dmax, amaxp) with the meaning of
        # ops.bn_act_backward's `pooled` (value = t + davg / HW ...).  Whoever consumes it folds it in (Conv.backward) or adds it (settle_pooled)
        self.pooled = None
        self.pool = None          # an ACTIVATION may carry its global (average, max) per (image, channel) when the pass that wrote it took them (Conv(pool=))

    @property
    def shape(self):
        return self.t.shape

    def slice(self, coff, c):
        return Act(self.t, self.coff + coff, c)


def settle_pooled(a):
    """Adds a gradient's pending pooled part (Act.pooled) to its tensor."""
    if a is not None and a.pooled is not None:
        ops.pool_backward_add_(a.t, a.coff, a.c, *a.pooled)
        a.pooled = None
    return a


def new_act(like, H, W, c):
    return Act(torch.empty(like.shape[0], H, W, pad4(c), device=like.device, dtype=torch.float32), 0, c)


def concat_act(like, H, W, c):
    """The buffer several producers write channel slices of (the reference's torch.cat, never materialised).  Stored at pad4(c) channels like every
    activation: a total that is >= 64 and not a multiple of 32 (5 x 16 = 80 in a C2fCBAM of hidden width 16, n = 3) gets zero pad channels the
    consumer conv may read (its weight columns there are zero).  Round 4: the buffers were allocated at exactly c and such a width failed the
    consumer's channel-range check (found by the n = 3 case of test_c2fcbam_train_forward_backward; no shipped graph has such a width)."""
    cp = pad4(c)
    alloc = torch.empty if cp == c else torch.zeros
    return Act(alloc(like.shape[0], H, W, cp, device=like.device, dtype=torch.float32), 0, c)


def autopad(k, p=None, d=1):
    """models/common.py:43-51."""
    if p is not None:
        return p
    return (d * (k - 1) + 1) // 2 if d > 1 else k // 2


class _Packed(nn.Module):
    """Mixin: device-side packed parameters are rebuilt lazily after any parameter change."""

    def _pack_params(self):
        """The parameters _pack reads (they key the cache); a block whose children pack themselves names its own."""
        return self.parameters()

    def _packed(self, dev):
        # in-place edits through torch (load_state_dict, copy_) bump the version counters; the fused optimizer writes through
        # raw pointers and calls Model.invalidate() itself
        key = (dev, self.training, tuple(p._version for p in self._pack_params()))
        cache = self.__dict__.get('_pk')
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, self._pack(dev))
            self.__dict__['_pk'] = cache
        return cache[1]

    def invalidate(self):
        self.__dict__.pop('_pk', None)


def _acc_grad(param, g):
    """param.grad += g (reference layout, like autograd's accumulation)."""
    g = g.detach().to(param.dtype)
    if param.grad is None:
        param.grad = g.clone().contiguous()
    else:
        param.grad.add_(g)


def _grad_targets(*params):
    """Buffers a backward kernel may accumulate into directly: each parameter's gradient when it is a contiguous fp32 tensor (the optimizer's
    flat views are), else a zero scratch.  -> (buffers, finish): finish() adds the scratch ones (if any) to .grad with _acc_grad."""
    direct = [p_.grad is not None and p_.grad.is_contiguous() and p_.grad.dtype == torch.float32 for p_ in params]
    bufs = [p_.grad if d else torch.zeros_like(p_, dtype=torch.float32) for p_, d in zip(params, direct)]

    def finish():
        for p_, buf, d in zip(params, bufs, direct):
            if not d:
                _acc_grad(p_, buf)
    return bufs, finish


def _plain_conv_backward(conv, src, dy, wt=None, *, dy_coff=0, dx_out=None, accumulate=False, need_dx=True, direct=()):
    """Backward of a plain nn.Conv2d (stride 1, pad k // 2 - or, dilated, the conv's own padding; no norm, no activation) that read the Act `src`: weight and bias gradients into .grad,
    -> the data gradient as an Act (written into dx_out if given, added to it if accumulate; None without need_dx).
    dy: gradient tensor w.r.t. the output, pad4(out_channels) wide from channel dy_coff (pad channels zero).  wt: the weight packed for the
    data-gradient kernel (packed here when None).  direct: which of 'weight' / 'bias' the kernels accumulate straight into .grad when it is
    a contiguous fp32 tensor and nothing is padded (the weight of a 1x1 conv only); the others go through a scratch tensor and _acc_grad."""
    k, dil = conv.kernel_size[0], conv.dilation[0]
    p = conv.padding[0] if dil > 1 else k // 2
    c1, c2 = conv.in_channels, conv.out_channels
    c1p, cp = pad4(c1), pad4(c2)
    g = conv.weight.grad
    if ('weight' in direct and k == 1 and c1p == c1 and cp == c2 and g is not None and g.is_contiguous() and g.dtype == torch.float32 and
            g.device == dy.device):
        gv = g.view(c2, c1)                                       # the optimizer's flat view: the kernel adds to it in place
        ops.conv2d_wgrad_nhwc(src.t, dy, kh=1, kw=1, cin=c1p, x_coff=src.coff, cout=cp, dy_coff=dy_coff, out=gv, accumulate=gv)
    else:
        dw = ops.conv2d_wgrad_nhwc(src.t, dy, kh=k, kw=k, stride=1, pad=p, dil=dil, cin=c1p, x_coff=src.coff, cout=cp, dy_coff=dy_coff)
        _acc_grad(conv.weight, dw.view(cp, k, k, c1p)[:c2, :, :, :c1].permute(0, 3, 1, 2))
    if conv.bias is not None:
        if 'bias' in direct and cp == c2:
            (db,), fin = _grad_targets(conv.bias)
        else:
            db = torch.zeros(cp, device=dy.device)
            fin = lambda: _acc_grad(conv.bias, db[:c2])          # noqa: E731
        ops.chan_sum_(dy, cp, dy_coff, db)
        fin()
    if not need_dx:
        return None
    if wt is None:
        wt = pack_dgrad_weight(conv.weight.detach().float()).to(dy.device)
    B, H, W, _ = src.shape
    if dx_out is None:
        dx_out = Act(torch.empty(B, H, W, c1p, device=dy.device, dtype=torch.float32), 0, c1)
    ops.conv2d_dgrad_nhwc(dy, wt, B=B, H=H, W=W, cin=c1p, kh=k, kw=k, stride=1, pad=p, dil=dil, cout=cp, dy_coff=dy_coff, out=dx_out.t,
                          dx_coff=dx_out.coff, accumulate=dx_out.t if accumulate else None, acc_coff=dx_out.coff)
    return dx_out


_NBT_PENDING = None      # Model.forward collects the BatchNorm step counters here and bumps them with one multi-tensor add


def _bump_batches_tracked(bn):
    if _NBT_PENDING is not None:
        _NBT_PENDING.append(bn.num_batches_tracked)
    else:
        bn.num_batches_tracked += 1


class collect_batches_tracked:
    """Context manager: BatchNorm step counters touched inside are incremented together on exit."""

    def __enter__(self):
        global _NBT_PENDING
        self.outer, _NBT_PENDING = _NBT_PENDING, []
        return self

    def __exit__(self, *exc):
        global _NBT_PENDING
        pending, _NBT_PENDING = _NBT_PENDING, self.outer
        if pending and exc[0] is None:
            torch._foreach_add_(pending, 1)
        return False


# ------------------------------------------------------------------------------------------------ BatchNorm in training mode
def _bn_vectors(bn, dev, cp):
    """The BatchNorm vectors as the kernels read them, cp >= num_features wide: the module's own tensors when nothing is padded (the running
    statistics then update in place), else padded device copies (gamma / beta / mean 0 and variance 1 in the pad channels)."""
    c2 = bn.num_features
    if cp == c2 and bn.weight.device == dev:
        return dict(gamma=bn.weight.detach(), beta=bn.bias.detach(), rm=bn.running_mean, rv=bn.running_var, inplace=True)
    padv = lambda t, fill: torch.cat([t.detach().float().to(dev), torch.full((cp - c2,), fill, device=dev)])   # noqa: E731
    return dict(gamma=padv(bn.weight, 0.), beta=padv(bn.bias, 0.), rm=padv(bn.running_mean, 0.), rv=padv(bn.running_var, 1.), inplace=False)


def _bn_clones(bn):
    """_bn_vectors of a layer that packs nothing: the module's parameters and clones of its running statistics for the kernel to update."""
    return dict(gamma=bn.weight.detach().float().contiguous(), beta=bn.bias.detach().float().contiguous(),
                rm=bn.running_mean.detach().clone(), rv=bn.running_var.detach().clone(), inplace=False)


def _bn_train(bn, c, x=None, *, coff=0, act='none', partials=None, npix=None, vec=None):
    """Forward half of a training BatchNorm over c channels: batch statistics of x's channel slice at coff (of act(x) when given, never stored)
    or from the partial sums a conv epilogue left (partials = the dict that launch filled, over npix pixels; its pivot is vec['rm']), the
    running statistics updated in `vec` (_bn_vectors / slices of it; _bn_clones(bn) when None).
    -> ((mean, rstd, scale, shift), commit): commit() writes the running statistics back to the module where `vec` holds copies and bumps
    num_batches_tracked - call it once per forward of `bn`, after the launches that today precede the write-back."""
    vec = _bn_clones(bn) if vec is None else vec
    if partials is not None:
        st = ops.bn_stats_from_partials(partials['part'], partials['rows'], npix, c, vec['gamma'], vec['beta'], bn.eps, bn.momentum,
                                        vec['rm'], vec['rv'])
    else:
        st = ops.bn_stats(x, c, coff, vec['gamma'], vec['beta'], bn.eps, bn.momentum, vec['rm'], vec['rv'], act=act)

    def commit():
        with torch.no_grad():
            if not vec['inplace']:
                bn.running_mean.copy_(vec['rm'][:bn.num_features])
                bn.running_var.copy_(vec['rv'][:bn.num_features])
            _bump_batches_tracked(bn)
    return st, commit


def _bn_grad_targets(bn, cp, dev):
    """_grad_targets of a BatchNorm's (weight, bias) for kernels that write cp >= num_features channels: padded scratch vectors when cp is wider."""
    if cp == bn.num_features:
        return _grad_targets(bn.weight, bn.bias)
    bufs = [torch.zeros(cp, device=dev), torch.zeros(cp, device=dev)]

    def finish():
        _acc_grad(bn.weight, bufs[0][:bn.num_features])
        _acc_grad(bn.bias, bufs[1][:bn.num_features])
    return bufs, finish


def _bn_backward(bn, dz, dz_coff, x, st, act, dx, c, *, coff=0, order=0, batch_stats=True, pooled=None, cp=None, targets=None):
    """Backward half: gradient of act(BN(x)) (order 0) or BN(act(x)) (order 1) over the channel slice [coff, coff + c) of x and dx, from dz's
    slice at dz_coff and the forward's st = (mean, rstd, scale, shift); gamma / beta gradients accumulated into .grad.  -> dx.
    batch_stats=False: the forward normalised with fixed statistics (ODConv's squeeze at batch 1) - nothing for the parameters.
    pooled: ops.bn_act_backward.  cp: the width the kernel writes the parameter gradients at (c when None).  targets: the (dgamma, dbeta)
    slices of a caller that resolved the buffers itself and finishes them after several calls (BottleneckCSP's two halves)."""
    if targets is not None:
        (dg, db), fin = targets, None
    elif batch_stats:
        (dg, db), fin = _bn_grad_targets(bn, c if cp is None else cp, x.device)
    else:
        dg, db, fin = torch.zeros(c, device=x.device), torch.zeros(c, device=x.device), None
    ops.bn_act_backward(dz, dz_coff, x, coff, c, *st, act, order, batch_stats, dx, coff, dg, db, pooled=pooled)
    if fin:
        fin()
    return dx


def _act_name(m):
    if isinstance(m, nn.SiLU):
        return 'silu'
    if isinstance(m, nn.Identity):
        return 'none'
    if isinstance(m, nn.ReLU):
        return 'relu'
    if isinstance(m, nn.GELU):
        return 'gelu'
    if isinstance(m, nn.LeakyReLU):
        if m.negative_slope != 0.1:
            raise NotImplementedError(f'LeakyReLU({m.negative_slope}) is not on the SOMI path (negative slope 0.1 only, SOMI_ACT_LEAKY)')
        return 'leaky'
    raise NotImplementedError(f'activation {type(m).__name__} is not on the SOMI path')


def _fold_conv_bn(conv, bn):
    """W' = diag(gamma/sqrt(var+eps)) W, b' = beta - gamma*mean/sqrt(var+eps) (+ scaled conv bias)
    (utils/torch_utils.py:202-222)."""
    w = conv.weight.detach().float()
    b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    if bn is not None:
        s, t = bn_fold(bn)
        w = w * s.view(-1, 1, 1, 1)
        b = b * s + t
    return w, b


def _pack_wb(w, b, dev):
    """-> packed weight [pad4(Cout)][k*k*pad4(Cin)], bias [pad4(Cout)] on dev (pads zero)."""
    cout = w.shape[0]
    wp = pack_conv_weight(w, cout_pad=pad4(cout)).to(dev)
    bp = torch.zeros(pad4(cout), device=dev)
    bp[:cout] = b.to(dev)
    return wp, bp


class Conv(_Packed):
    """conv2d(bias=False) -> BatchNorm2d -> SiLU as one fused launch (models/common.py:53-70).  d > 1 (dense, stride 1) walks dilated taps
    in the same kernels, forward and both gradients.  g > 1 runs on the grouped / depthwise
    kernels (gconv.hip): k 1, 3 or 5, stride 1 or 2, pad k // 2, at most 16 input channels per group."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        if isinstance(k, (tuple, list)):                         # C3 hands its bottlenecks (1, 1) / (3, 3) (models/common.py:1558)
            if len(k) != 2 or k[0] != k[1]:
                raise NotImplementedError('square kernels only')
            k = int(k[0])
        if d != 1 and g != 1:
            raise NotImplementedError('grouped / depthwise dilated Conv is not on the SOMI path (dense convs only)')
        if d != 1 and s != 1:
            raise NotImplementedError(f'dilated Conv with stride {s} is not on the SOMI path (its data gradient runs at stride 1 only)')
        if g != 1:
            if k not in (1, 3, 5) or s not in (1, 2) or autopad(k, p, d) != k // 2:
                raise NotImplementedError(f'grouped Conv with k={k}, s={s}, p={p} is not on the SOMI path (k 1/3/5, stride 1/2, pad k // 2)')
            if c1 % g == 0 and c1 // g > 16:
                raise NotImplementedError(f'grouped Conv with {c1 // g} input channels per group is not on the SOMI path (at most 16)')
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p, d), groups=g, dilation=d, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())

    # What Model's graph walk reads of every block.  accumulates: backward(dout, dx_out=<whole padded contiguous tensor>,
    # accumulate=True) adds the input gradient into dx_out in place.  folds_pooled: the closing Conv's BatchNorm + SiLU passes take a reader's global
    # pools in forward(pool=) and fold a pending Act.pooled in backward(pooled=).  reduction: input map size / output map size.
    accumulates = folds_pooled = True
    reduction = property(lambda self: self.conv.stride[0])

    def _pack(self, dev):
        if self.conv.groups > 1:
            return self._pack_grouped(dev)
        if self.training:                                        # raw weights, batch-norm applied from batch statistics
            w = self.conv.weight
            c2, c1, k = w.shape[0], w.shape[1], w.shape[2]
            cp, c1p = pad4(c2), pad4(c1)
            master = self.__dict__.get('_master')               # (weights, gradients) [cp][k*k*c1p] inside the optimizer's flat buffers
            if master is not None and master[0].device == dev:
                wp, gp = master
                wt = ops.pack_dgrad_weights(wp, cp, k * k, c1p)
            else:
                wf = w.detach().float()
                wp, gp, wt = pack_conv_weight(wf, cout_pad=cp).to(dev), None, pack_dgrad_weight(wf).to(dev)
            return dict(wp=wp, gp=gp, wt=wt, **_bn_vectors(self.bn, dev, cp))
        return _pack_wb(*_fold_conv_bn(self.conv, getattr(self, 'bn', None)), dev)

    def _pack_grouped(self, dev):
        """training: raw weights [k*k][cin_g][pad4(c2)] and the padded BatchNorm vectors; eval: BatchNorm folded into weights and bias."""
        c2, cp = self.conv.out_channels, pad4(self.conv.out_channels)
        if not self.training:
            w, b = _fold_conv_bn(self.conv, getattr(self, 'bn', None))
            bp = torch.zeros(cp, device=dev)
            bp[:c2] = b.to(dev)
            return pack_gconv_weight(w, cp).to(dev), bp
        return dict(gw=pack_gconv_weight(self.conv.weight.detach(), cp).to(dev), **_bn_vectors(self.bn, dev, cp))

    # ------------------------------------------------------------------------------------------ training mode
    def _forward_train(self, x, out, residual, pool=None):
        """y = conv(x) (raw) -> batch statistics -> z = act(y*scale+shift) [+ residual]; keeps what backward needs.
        pool: a dict - when the shape allows, the pass that writes z also takes its global average / max pools per (image, channel) and leaves
        them as pool['avg'], pool['max'] (a channel attention behind this block then needs no pass of its own over z)."""
        pk = self._packed(x.t.device)                            # rebuilt after every optimizer step (Model.invalidate)
        k, s, p, dil = self.conv.kernel_size[0], self.conv.stride[0], self.conv.padding[0], self.conv.dilation[0]
        c2, cp = self.conv.out_channels, pad4(self.conv.out_channels)
        B, H, W, _ = x.shape
        Ho, Wo = ops.conv_out_size(H, k, s, p, dil), ops.conv_out_size(W, k, s, p, dil)
        y = torch.empty(B, Ho, Wo, cp, device=x.t.device, dtype=torch.float32)
        st = {'pivot': pk['rm']} if self.conv.groups > 1 or y.numel() * 4 <= 0xE0000000 else None     # the epilogue leaves y's per-channel partial sums
        if self.conv.groups > 1:                                 # grouped / depthwise: the same partial sums, from the stencil kernel
            ops.gconv2d_nhwc(x.t, pk['gw'], c1=self.conv.in_channels, c2=c2, groups=self.conv.groups, k=k, stride=s, x_coff=x.coff, out=y, cw=cp,
                             bn_stats=st)
        else:
            ops.conv2d_nhwc(x.t, pk['wp'], None, kh=k, kw=k, stride=s, pad=p, dil=dil, act='none', cin=pad4(x.c), x_coff=x.coff, out=y, cout=cp,
                            alg_cin=x.c, alg_cout=c2, bn_stats=st)
        (mean, rstd, scale, shift), commit = _bn_train(self.bn, cp, y, partials=st, npix=B * Ho * Wo, vec=pk)
        commit()                                                 # running statistics back into the module buffers
        if out is None:
            out = new_act(x.t, Ho, Wo, c2)
        elif c2 % 4:
            raise NotImplementedError('writing into a channel slice needs c2 % 4 == 0')
        cw = cp if out.coff == 0 and out.t.shape[3] == cp else c2
        pooled = None
        if pool is not None and residual is None and cw == c2 and isinstance(self.act, nn.SiLU):
            pooled = ops.affine_silu_pool(y, c2, 0, scale, shift, out.t, out.coff)
        if pooled is not None:
            pool['avg'], pool['max'] = pooled
        elif residual is not None and cw != c2:
            ops.chan_affine_act(y, cw, 0, scale, shift, _act_name(self.act), 0, out.t, out.coff)
            ops.add_(out.t, out.coff, residual.t, residual.coff, c2)
        else:
            ops.chan_affine_act(y, cw, 0, scale, shift, _act_name(self.act), 0, out.t, out.coff,
                                residual=None if residual is None else residual.t, res_coff=0 if residual is None else residual.coff)
        self.__dict__['_ctx'] = (x, y, mean, rstd, scale, shift, pk)
        return Act(out.t, out.coff, c2)

    def backward(self, dz, dx_out=None, accumulate=False, need_dx=True, also_add=None, pooled=None, cbam=None):
        """dz: gradient w.r.t. this block's output (Act).  Returns the gradient w.r.t. the input as an Act (written into
        dx_out if given, added to it if accumulate; `also_add` is a further Act added in the same pass - a shortcut's
        gradient).  Parameter gradients are accumulated into .grad (reference layout).
        pooled: (davg, dmax, amaxp) of a channel attention that pooled this block's output (ops.bn_act_backward): its gradient joins dz inside
        the BatchNorm backward kernels.
        cbam: state of ops.cbam_backward(bn=...) - dz is then the gradient w.r.t. t*ca*sa of the CBAM bottleneck this conv opens, and the attention's
        step C runs inside the BatchNorm backward kernels too (pooled = the MLP backward's (davg, dmax, amaxp) on that call's dca)."""
        x, y, mean, rstd, scale, shift, pk = self.__dict__.pop('_ctx')
        k, s, p, dil = self.conv.kernel_size[0], self.conv.stride[0], self.conv.padding[0], self.conv.dilation[0]
        c1, c2, cp = self.conv.in_channels, self.conv.out_channels, pad4(self.conv.out_channels)
        dev = y.device
        dy = torch.zeros_like(y) if cp != c2 else torch.empty_like(y)
        cw = cp if (dz.coff == 0 and dz.t.shape[3] == cp) else c2     # whole padded tensor, or an aligned slice
        if cw % 4:
            raise NotImplementedError('training backward on a channel slice needs out_channels % 4 == 0')
        if cbam is not None:                                      # CBAM's step C + pooled gradients + BatchNorm backward in two passes over (dz, y)
            if cw != cp or cp != c2:
                raise NotImplementedError('fused CBAM backward works on whole, unpadded tensors')
            (dgam, dbet), fin = _bn_grad_targets(self.bn, cp, dev)
            ops.cbam_bn_backward_apply(cbam, rstd, pooled[0], pooled[1], dy, dgam, dbet)
            fin()
        else:
            _bn_backward(self.bn, dz.t, dz.coff, y, (mean, rstd, scale, shift), _act_name(self.act), dy, cw, pooled=pooled, cp=cp)
        B, H, W, _ = x.shape
        if self.conv.groups > 1:
            return self._backward_grouped(x, dy, pk, dx_out, accumulate, need_dx, also_add)
        if pk['gp'] is not None:                                  # accumulate into the packed gradient master
            ops.conv2d_wgrad_nhwc(x.t, dy, kh=k, kw=k, stride=s, pad=p, dil=dil, cin=pad4(c1), x_coff=x.coff, cout=cp, out=pk['gp'],
                                  accumulate=pk['gp'])
        else:
            dw = ops.conv2d_wgrad_nhwc(x.t, dy, kh=k, kw=k, stride=s, pad=p, dil=dil, cin=pad4(c1), x_coff=x.coff, cout=cp)
            _acc_grad(self.conv.weight, dw.view(cp, k, k, pad4(c1))[:c2, :, :, :c1].permute(0, 3, 1, 2))
        if not need_dx:
            return None
        if dx_out is None:
            dx_out = Act(torch.empty(B, H, W, pad4(c1), device=dev, dtype=torch.float32), 0, c1)
        ops.conv2d_dgrad_nhwc(dy, pk['wt'], B=B, H=H, W=W, cin=pad4(c1), kh=k, kw=k, stride=s, pad=p, dil=dil, cout=cp, out=dx_out.t,
                              dx_coff=dx_out.coff, accumulate=dx_out.t if accumulate else None, acc_coff=dx_out.coff,
                              accumulate2=None if also_add is None else also_add.t,
                              acc2_coff=0 if also_add is None else also_add.coff)
        return dx_out

    def _backward_grouped(self, x, dy, pk, dx_out, accumulate, need_dx, also_add):
        """Weight gradient straight into .grad ((c2, c1/g, k, k), no packed master for grouped weights), then the data gradient: written into
        dx_out (added to it if accumulate, + also_add's slice)."""
        k, s = self.conv.kernel_size[0], self.conv.stride[0]
        c1, c2, g = self.conv.in_channels, self.conv.out_channels, self.conv.groups
        B, H, W, _ = x.shape
        (gw,), fin = _grad_targets(self.conv.weight)
        ops.gconv2d_wgrad_nhwc(x.t, dy, c1=c1, c2=c2, groups=g, k=k, stride=s, x_coff=x.coff, out=gw, accumulate=True)
        fin()
        if not need_dx:
            return None
        whole = also_add is None and (dx_out is None or (dx_out.coff == 0 and dx_out.t.shape[3] == pad4(c1)))
        cx = pad4(c1) if whole else c1                            # a whole tensor gets its pad channels written (zero, + what accumulates there)
        if cx % 4:
            raise NotImplementedError('grouped Conv backward into a channel slice needs in_channels % 4 == 0')
        if dx_out is None:
            dx_out = Act((torch.empty if cx == pad4(c1) else torch.zeros)(B, H, W, pad4(c1), device=dy.device, dtype=torch.float32), 0, c1)
        ops.gconv2d_dgrad_nhwc(dy, pk['gw'], H=H, W=W, c1=c1, c2=c2, groups=g, k=k, stride=s, out=dx_out.t, dx_coff=dx_out.coff, cx=cx,
                               accumulate=dx_out.t if accumulate else None, acc_coff=dx_out.coff,
                               accumulate2=None if also_add is None else also_add.t, acc2_coff=0 if also_add is None else also_add.coff)
        return dx_out

    def forward(self, x, out=None, residual=None, a_chan=None, a_pix=None, pool=None):
        if self.training:
            return self._forward_train(x, out, residual, pool)
        if self.conv.groups > 1:
            return self._forward_grouped(x, out, residual, a_chan, a_pix)
        wp, bp = self._packed(x.t.device)
        k, s, p, dil = self.conv.kernel_size[0], self.conv.stride[0], self.conv.padding[0], self.conv.dilation[0]
        c2 = self.conv.out_channels
        B, H, W, _ = x.shape
        Ho, Wo = ops.conv_out_size(H, k, s, p, dil), ops.conv_out_size(W, k, s, p, dil)
        if out is None:
            out = new_act(x.t, Ho, Wo, c2)
            cout = pad4(c2)
        else:
            if c2 % 4:
                raise NotImplementedError('writing into a channel slice needs c2 % 4 == 0')
            cout = c2
        ops.conv2d_nhwc(x.t, wp[:cout], bp, kh=k, kw=k, stride=s, pad=p, dil=dil, act=_act_name(self.act), cin=pad4(x.c),
                        x_coff=x.coff, out=out.t, cout=cout, y_coff=out.coff,
                        residual=None if residual is None else residual.t,
                        res_coff=0 if residual is None else residual.coff, a_chan_scale=a_chan, a_pix_scale=a_pix,
                        alg_cin=x.c, alg_cout=c2)
        return Act(out.t, out.coff, c2)

    def _forward_grouped(self, x, out, residual, a_chan, a_pix):
        """Eval: BatchNorm folded, act, optional residual slice - one launch of the grouped kernel."""
        if a_chan is not None or a_pix is not None:
            raise NotImplementedError('attention scales are not folded into the grouped conv')
        wp, bp = self._packed(x.t.device)
        k, s = self.conv.kernel_size[0], self.conv.stride[0]
        c1, c2 = self.conv.in_channels, self.conv.out_channels
        B, H, W, _ = x.shape
        Ho, Wo = ops.conv_out_size(H, k, s, k // 2), ops.conv_out_size(W, k, s, k // 2)
        if out is None:
            out, cw = new_act(x.t, Ho, Wo, c2), pad4(c2)
        else:
            if c2 % 4:
                raise NotImplementedError('writing into a channel slice needs c2 % 4 == 0')
            cw = c2
        ops.gconv2d_nhwc(x.t, wp, bp, c1=c1, c2=c2, groups=self.conv.groups, k=k, stride=s, x_coff=x.coff, out=out.t, y_coff=out.coff, cw=cw,
                         act=_act_name(self.act), residual=None if residual is None else residual.t,
                         res_coff=0 if residual is None else residual.coff)
        return Act(out.t, out.coff, c2)


class PlainConv(_Packed):
    """nn.Conv2d with bias, no norm / activation (Decouple.b3 / c3, models/yolo.py:1057,1063)."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv

    def _pack(self, dev):
        return _pack_wb(*_fold_conv_bn(self.conv, None), dev)

    def forward(self, x):
        if self.training:
            self.invalidate()
        wp, bp = self._packed(x.t.device)
        k = self.conv.kernel_size[0]
        B, H, W, _ = x.shape
        out = new_act(x.t, H, W, self.conv.out_channels)
        ops.conv2d_nhwc(x.t, wp, bp, kh=k, kw=k, stride=1, pad=k // 2, act='none', cin=pad4(x.c), x_coff=x.coff,
                        out=out.t, cout=pad4(self.conv.out_channels), alg_cin=x.c, alg_cout=self.conv.out_channels)
        if self.training:
            self.__dict__['_ctx'] = x
        return out

    def backward(self, dy, dx_out=None, accumulate=False, need_dx=True):
        """dy: whole padded gradient tensor (pad channels zero).  Returns dx (Act): written into dx_out if given, added to it if accumulate."""
        return _plain_conv_backward(self.conv, self.__dict__.pop('_ctx'), dy, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class ChannelAttentionModule(_Packed):
    """sigmoid(MLP(GAP) + MLP(GMP)) (models/common.py:339-358) -> (B,C) scale vector."""

    def __init__(self, c1, reduction=16):
        super().__init__()
        mid = c1 // reduction
        self.shared_MLP = nn.Sequential(nn.Linear(c1, mid), nn.ReLU(), nn.Linear(mid, c1))

    def _pack(self, dev):
        l1, l2 = self.shared_MLP[0], self.shared_MLP[2]
        return tuple(t.detach().float().contiguous().to(dev) for t in (l1.weight, l1.bias, l2.weight, l2.bias))

    def forward(self, x, pooled=None):
        """pooled: (avg, max) of x per (image, channel) when the producer of x already took them (Conv(..., pool=))."""
        if self.training:
            self.invalidate()
        W1, b1, W2, b2 = self._packed(x.t.device)
        avg, mx = pooled if pooled is not None else ops.global_pool(x.t, c=x.c, x_coff=x.coff)
        ca = ops.attn_mlp(0, avg, mx, W1, b1, W2, b2)
        if self.training:
            self.__dict__['_ctx'] = (x, avg, mx, ca, (W1, b1, W2, b2))
        return ca

    def backward(self, dca, dt, amaxp, defer=False):
        """dca (B,C): gradient w.r.t. the attention vector; adds the pooled-input gradient into dt (Act) in place - or, defer=True, returns
        (davg, dmax, amaxp) for the producer's BatchNorm backward to fold in (Conv.backward(pooled=...)) and leaves dt alone.
        amaxp (B,C) int32: first pixel of every channel's spatial maximum (the CBAM backward finds it in its own pass over x)."""
        x, avg, mx, ca, (W1, b1, W2, b2) = self.__dict__.pop('_ctx')
        l1, l2 = self.shared_MLP[0], self.shared_MLP[2]
        g, fin = _grad_targets(l1.weight, l1.bias, l2.weight, l2.bias)      # the kernel accumulates; same layout as the parameters
        davg, dmax = ops.attn_mlp_backward(0, dca, ca, avg, mx, W1, b1, W2, *g)
        fin()
        if defer:
            return davg, dmax, amaxp
        ops.pool_backward_add_(dt.t, dt.coff, x.c, davg, dmax, amaxp)


class SpatialAttentionModule(_Packed):
    """sigmoid(conv_kxk([mean_c, max_c])) (models/common.py:392-405) -> (B,H,W) scale map of ca*x."""

    def __init__(self, kernel_size=7):
        super().__init__()
        assert kernel_size in (3, 5, 7)
        self.cv1 = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2)

    def _pack(self, dev):
        w = self.cv1.weight.detach().float()[0].permute(1, 2, 0).contiguous().to(dev)     # [k][k][2]
        return w, self.cv1.bias.detach().float().contiguous().to(dev)     # stays on the device: no host sync per repack

    def forward(self, x, ca):
        """Applies both attentions: x <- x * ca * sa.  Eval: in place (one stats pass + one apply pass).  Train: x is kept
        (backward needs it) and the product goes to a new tensor."""
        if self.training:
            self.invalidate()
        w, b = self._packed(x.t.device)
        stats = ops.chan_stats(x.t, ca, c=x.c, x_coff=x.coff)
        k = self.cv1.kernel_size[0]
        if not self.training:
            ops.cbam_apply_(x.t, ca, stats, w, b, k, c=x.c, x_coff=x.coff)
            return x
        if x.coff != 0 or x.t.shape[3] != x.c:
            raise NotImplementedError('CBAM training path works on whole tensors')
        sa = ops.spatial_attn(stats, w, b, k)
        out = ops.scale_channels(x.t, ca, sa)
        self.__dict__['_ctx'] = (x, ca, stats, sa, w)
        return Act(out, 0, x.c)

    def backward(self, dt2, t_max, bn=None):
        """dt2: gradient tensor w.r.t. x*ca*sa (whole tensor, modified in place into the x-gradient through both products and
        the spatial branch).  Returns dca (B,C) and amaxp (B,C): the first pixel holding each channel's maximum (for the max-pool's gradient),
        found from t_max (B,C), the spatial maximum of x the channel attention pooled.
        bn = (y, scale, shift, mean) of the Conv that produced x: dt2 is left as it is and a third value - the state for that Conv's
        backward(cbam=...) - is returned (ops.cbam_backward)."""
        x, ca, stats, sa, w = self.__dict__.pop('_ctx')
        k = self.cv1.kernel_size[0]
        (dw, db), fin = _grad_targets(self.cv1.weight, self.cv1.bias)    # the kernel accumulates in nn.Conv2d's (1,2,k,k) layout
        res = ops.cbam_backward(dt2, x.t, x.coff, x.c, ca, sa, stats, w, k, dw, db, t_max=t_max, dw_chw=True, bn=bn)
        fin()
        return res


class CBAMBottleneck(nn.Module):
    """cv1 3x3 -> channel attn -> spatial attn -> cv2 3x3 (+x) (models/common.py:671-691).
    The two attention scalings are applied to cv1's output in place by one streaming kernel (the in-operand form of
    the conv kernel measured 26 % slower than the plain one; the extra pass costs ~2 %)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=1.0, k=(3, 3), ratio=8, kernel_size=3):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=1)
        self.add = shortcut and c1 == c2
        self.channel_attention = ChannelAttentionModule(c_, ratio)
        self.spatial_attention = SpatialAttentionModule(kernel_size)

    def forward(self, x, out=None):
        pool = {} if self.training else None
        t = self.cv1(x, pool=pool)                                # training: the BatchNorm + SiLU pass also takes the attention's global pools
        ca = self.channel_attention(t, pooled=(pool['avg'], pool['max']) if pool else None)
        t2 = self.spatial_attention(t, ca)
        if self.training:
            self.__dict__['_ctx'] = (x, t)
        return self.cv2(t2, out=out, residual=x if self.add else None)

    def _step_c_in_bn(self, d, t):
        """Step C inside cv1's BatchNorm + SiLU backward (else a pass of its own): local batch statistics, a SiLU, whole unpadded d and t."""
        c_ = self.cv1.conv.out_channels
        return ops.SYNC_BN is None and isinstance(self.cv1.act, nn.SiLU) and pad4(c_) == c_ and d.coff == t.coff == 0 and d.t.shape[3] == c_

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """dout: gradient w.r.t. the block output (Act); the input gradient is ADDED into dx_out (Act, e.g. a slice of the
        C2f gradient buffer that already holds the gradient of the input's other consumers); or, with none of the three given, it is RETURNED
        as a tensor of its own (the form C3.backward takes: C3_CBAM, C3_CBAMS) - the same launches, cv1's data gradient written, not added."""
        returning = dx_out is None and not accumulate and need_dx
        if not returning and (dx_out is None or not accumulate or not need_dx):
            raise NotImplementedError('CBAMBottleneck adds its input gradient into dx_out, or returns it (dx_out=None, accumulate=False)')
        x, t = self.__dict__.pop('_ctx')
        d = self.cv2.backward(dout)                               # d(t*ca*sa)
        bn = None
        if self._step_c_in_bn(d, t):
            _, y1, mean1, _, scale1, shift1, _ = self.cv1.__dict__['_ctx']      # step C + the pooled terms + BatchNorm backward: two passes over (d, y1)
            bn = (y1, scale1, shift1, mean1)
        # d.t then holds the direct part of dt; the channel attention's pooled maximum lets the same pass find its arg-max pixels
        dca, amaxp, *state = self.spatial_attention.backward(d.t, t_max=self.channel_attention.__dict__['_ctx'][2], bn=bn)
        pooled = self.channel_attention.backward(dca, d, amaxp, defer=True)   # the pooled paths join d inside cv1's BatchNorm backward
        c1 = self.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0  # the shortcut's gradient rides the dgrad epilogue
        dx_out = self.cv1.backward(d, dx_out=dx_out, accumulate=not returning, also_add=dout if fuse else None, pooled=pooled,
                                   cbam=state[0] if state else None)
        if self.add and not fuse:
            ops.add_(dx_out.t, dx_out.coff, dout.t, dout.coff, x.c)
        return dx_out


class C2fCBAM(nn.Module):
    """models/common.py:2671-2695; all (2+n) pieces live in one buffer, nothing is concatenated."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, kernel_size=7):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(
            CBAMBottleneck(self.c, self.c, shortcut, g, k=(3, 3), e=1.0, ratio=16, kernel_size=kernel_size)
            for _ in range(n))

    accumulates, folds_pooled, reduction = True, True, 1

    def forward(self, x, pool=None):
        """pool: a dict the closing conv's BatchNorm + SiLU pass fills with the output's global average / max (Conv._forward_train)."""
        c, n = self.c, len(self.m)
        if c % 4:
            raise NotImplementedError('C2fCBAM hidden width must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, (2 + n) * c)
        self.cv1(x, out=cat.slice(0, 2 * c))
        for i, blk in enumerate(self.m):
            blk(cat.slice((1 + i) * c, c), out=cat.slice((2 + i) * c, c))
        return self.cv2(cat, pool=pool)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True, pooled=None):
        """pooled: a pending part of dout that is constant over each image's pixels (Act.pooled): the closing conv's BatchNorm backward folds it in."""
        c, n = self.c, len(self.m)
        dcat = self.cv2.backward(dout, pooled=pooled)             # gradient of every piece through the 1x1 mix
        for i in reversed(range(n)):
            self.m[i].backward(dcat.slice((2 + i) * c, c), dx_out=dcat.slice((1 + i) * c, c), accumulate=True)
        return self.cv1.backward(dcat.slice(0, 2 * c), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class SPPF(nn.Module):
    """models/common.py:1846-1861: the three chained max-pools are one kernel writing the concat slices."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        if k != 5:
            raise NotImplementedError('SPPF kernel size 5 only')
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)

    accumulates, folds_pooled, reduction = True, False, 1

    def forward(self, x):
        c_ = self.cv1.conv.out_channels
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 4 * c_)
        self.cv1(x, out=cat.slice(0, c_))
        if self.training:                                         # level by level, leaving each window's arg-max for the backward pass
            self.__dict__['_ctx'] = (cat, ops.sppf_pool_(cat.t, c_, 0, codes=True)[1])
        else:
            ops.sppf_pool_(cat.t, c_, 0)
        return self.cv2(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        cat, codes = self.__dict__.pop('_ctx')
        c_ = self.cv1.conv.out_channels
        dcat = self.cv2.backward(dout)
        ops.sppf_pool_backward_(cat.t, dcat.t, c_, 0, codes=codes)
        return self.cv1.backward(dcat.slice(0, c_), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class Swish(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


class BiFPN(_Packed):
    """w_i / (sum_j swish(w_j) + 1e-4) weighted sum (models/common.py:3688-3704); inputs may be virtual 2x-upsampled.
    The weights are normalised inside the kernels from the raw parameter on the device."""

    def __init__(self, length):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(length, dtype=torch.float32), requires_grad=True)
        self.swish = Swish()
        self.epsilon = 0.0001

    accumulates, folds_pooled, reduction = False, False, 1       # several inputs: backward(dout) returns the list of their gradients

    def forward(self, xs):
        for a in xs:
            if a.coff != 0 or a.t.shape[3] != xs[0].t.shape[3]:
                raise NotImplementedError('BiFPN inputs must be whole tensors of equal width')
        w = self.weight.detach()
        if not w.is_cuda:
            raise RuntimeError('somi_amd BiFPN runs on the MI355X only (no CPU fallback)')
        out = ops.bifpn([a.t for a in xs], [a.up for a in xs], w, self.epsilon)      # normalised inside the kernel
        if self.training:
            self.__dict__['_ctx'] = xs
        return Act(out, 0, xs[0].c)

    def backward(self, dout):
        """Returns the list of input gradients (low-resolution for the virtually upsampled inputs)."""
        xs = self.__dict__.pop('_ctx')
        (dw,), fin = _grad_targets(self.weight)
        ds = ops.bifpn_backward([a.t for a in xs], [a.up for a in xs], self.weight.detach(), dout.t, dw, self.epsilon)
        fin()
        return [Act(d, 0, a.c) for d, a in zip(ds, xs)]


class Upsample(nn.Module):
    """nn.Upsample(None, 2, 'nearest') (YOLO-SOMI.yaml:37,42,47): a view flag; the consumer (BiFPN) reads at (h>>1, w>>1)."""

    def __init__(self, size=None, scale_factor=None, mode='nearest'):
        super().__init__()
        if size is not None or scale_factor != 2 or mode != 'nearest':
            raise NotImplementedError('only 2x nearest upsampling is on the SOMI path')

    accumulates, folds_pooled, reduction = False, False, 0.5

    def forward(self, x):
        return Act(x.t, x.coff, x.c, up=x.up + 1)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('Upsample hands its gradient through')
        return dout if need_dx else None                         # the consumer (BiFPN) already produced the low-resolution gradient


def _up_backward_target(dout, x, dx_out, accumulate):
    """Where a learned upsampler's backward kernel WRITES its input gradient: the caller's slice when it is only to be written, else a tensor of its own."""
    B, H, W, _ = x.shape
    if dout.up or tuple(dout.shape[:3]) != (B, 2 * H, 2 * W):
        raise RuntimeError(f'gradient of a 2x upsampler must be ({B}, {2 * H}, {2 * W}, .), got {tuple(dout.shape)}')
    if dx_out is not None and not accumulate:
        return dx_out
    return Act(torch.empty(B, H, W, x.c, device=dout.t.device, dtype=torch.float32), 0, x.c)


def _up_backward_result(dx, dx_out, accumulate, need_dx):
    if not need_dx:
        return None
    if dx_out is not None and accumulate:
        ops.add_(dx_out.t, dx_out.coff, dx.t, dx.coff, dx.c)
        return dx_out
    return dx


class CARAFE(nn.Module):
    """Content-aware reassembly, 2x (models/common.py:4450-4490): comp (1x1 Conv) -> enc (Conv, no activation) gives (2 * k_up)^2 logits per source
    pixel; every output pixel is the softmax-weighted sum of the k_up x k_up source window around its source pixel.  The reference unfolds the
    upsampled map to (B, C, k_up^2, 2H, 2W); here one kernel does softmax + reassembly from x and the logits (ops.carafe), and training keeps only the
    softmax weights.  A real 2H x 2W tensor comes out (up = 0): BiFPN and Concat take it as it is."""

    def __init__(self, c, k_enc=3, k_up=5, c_mid=64, scale=2):
        super().__init__()
        if scale != 2:
            raise NotImplementedError(f'CARAFE with scale={scale} is not on the SOMI path (scale 2 only)')
        if k_up not in (3, 5):
            raise NotImplementedError(f'CARAFE with k_up={k_up} is not on the SOMI path (k_up 3 or 5)')
        if k_enc not in (1, 3):
            raise NotImplementedError(f'CARAFE with k_enc={k_enc} is not on the SOMI path (k_enc 1 or 3)')
        if c % 4:
            raise NotImplementedError(f'CARAFE needs a channel count that is a multiple of 4 (c % 4 == 0), got {c}')
        self.scale, self.k_up = scale, k_up
        self.comp = Conv(c, c_mid)
        self.enc = Conv(c_mid, (scale * k_up) ** 2, k=k_enc, act=False)

    accumulates, folds_pooled, reduction = False, False, 0.5

    def forward(self, x):
        if x.up:
            raise NotImplementedError('CARAFE reads a real tensor, not an nn.Upsample view')
        B, H, W, _ = x.shape
        logits = self.enc(self.comp(x))
        out = new_act(x.t, 2 * H, 2 * W, x.c)
        r = ops.carafe(x.t, logits.t, x.c, self.k_up, x.coff, logits.coff, out=out.t, weights=self.training)
        if self.training:
            self.__dict__['_ctx'] = (x, r[1])
        return out

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """The kernel writes dx's reassembly part and the logits' gradient; enc and comp then run their own backward, comp adding into that dx."""
        x, wts = self.__dict__.pop('_ctx')
        dx = _up_backward_target(dout, x, dx_out, accumulate)
        _, dl = ops.carafe_backward(dout.t, x.t, wts, x.c, self.k_up, dout.coff, x.coff, out=dx.t, dx_coff=dx.coff)
        dmid = self.enc.backward(Act(dl, 0, dl.shape[3]))
        self.comp.backward(dmid, dx_out=dx, accumulate=True, need_dx=need_dx)
        return _up_backward_result(dx, dx_out, accumulate, need_dx)


class DySample(nn.Module):
    """Dynamic point-sampling upsampler, 2x, style 'lp' without dyscope (models/common.py:4246-4309): a 1x1 conv with bias gives 2 * 4 offsets per
    group and source pixel; every output pixel is the bilinear sample of its group's channels at source pixel + 0.25 * offset + init_pos, clamped to
    the map.  The reference goes through pixel_shuffle, permute and grid_sample; here one kernel reads x and the raw conv output (ops.dysample).
    init_pos stays the reference's registered buffer.  A real 2H x 2W tensor comes out (up = 0)."""

    def __init__(self, in_channels, scale=2, style='lp', groups=4, dyscope=False):
        super().__init__()
        if scale != 2:
            raise NotImplementedError(f'DySample with scale={scale} is not on the SOMI path (scale 2 only)')
        if style != 'lp':
            raise NotImplementedError(f"DySample with style={style!r} is not on the SOMI path (style 'lp' only)")
        if dyscope:
            raise NotImplementedError('DySample with dyscope=True is not on the SOMI path')
        if in_channels % 4:
            raise NotImplementedError(f'DySample needs a channel count that is a multiple of 4 (c % 4 == 0), got {in_channels}')
        if groups < 1 or in_channels % groups or (in_channels // groups) % 4:
            raise NotImplementedError(f'DySample needs channels per group that are a multiple of 4 ((c / groups) % 4 == 0), got c={in_channels}, '
                                      f'groups={groups}')
        self.scale, self.style, self.groups = scale, style, groups
        self.offset = nn.Conv2d(in_channels, 2 * groups * scale ** 2, 1)
        nn.init.normal_(self.offset.weight, 0, 0.001)            # normal_init(self.offset, std=0.001), models/common.py:4265
        nn.init.constant_(self.offset.bias, 0)
        h = torch.arange((-scale + 1) / 2, (scale - 1) / 2 + 1) / scale
        self.register_buffer('init_pos', torch.stack(torch.meshgrid(h, h, indexing='ij')).transpose(1, 2).repeat(1, groups, 1).reshape(1, -1, 1, 1))
        self.__dict__['_offset'] = PlainConv(self.offset)       # the runner shares the parameters, stays out of state_dict

    accumulates, folds_pooled, reduction = False, False, 0.5

    def invalidate(self):
        self._offset.invalidate()

    def _init_pos(self, dev):
        ip = self.init_pos.detach().reshape(-1)
        if ip.device != dev:
            raise RuntimeError('somi_amd DySample runs on the MI355X only (no CPU fallback): move the module to the GPU')
        return ip if ip.dtype == torch.float32 else ip.float()

    def forward(self, x):
        if x.up:
            raise NotImplementedError('DySample reads a real tensor, not an nn.Upsample view')
        self._offset.train(self.training)
        B, H, W, _ = x.shape
        o = self._offset(x)
        out = new_act(x.t, 2 * H, 2 * W, x.c)
        ops.dysample(x.t, o.t, self._init_pos(x.t.device), x.c, self.groups, x.coff, o.coff, out=out.t)
        if self.training:
            self.__dict__['_ctx'] = (x, o)
        return out

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """The kernels write dx's sampling part and the raw offsets' gradient; the offset conv's backward then adds into that dx."""
        x, o = self.__dict__.pop('_ctx')
        dx = _up_backward_target(dout, x, dx_out, accumulate)
        _, do = ops.dysample_backward(dout.t, x.t, o.t, self._init_pos(x.t.device), x.c, self.groups, dout.coff, x.coff, o.coff, out=dx.t,
                                      dx_coff=dx.coff)
        self._offset.backward(do, dx_out=dx, accumulate=True)
        return _up_backward_result(dx, dx_out, accumulate, need_dx)


class ODConv2d_3rd(_Packed):
    """Parameter layout of models/common.py:4495-4536; executed by ODConv_3rd below."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 K=4, r=1 / 16):
        super().__init__()
        if groups != 1 or dilation != 1:
            raise NotImplementedError('grouped / dilated ODConv is not on the SOMI path')
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.kernel_size, self.stride, self.padding = (kernel_size, kernel_size), stride, padding
        self.weight = nn.Parameter(torch.empty(K, out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.zeros(K, out_channels)) if bias else None
        hidden = max(int(in_channels * r), 16)
        self.reduction = nn.Linear(in_channels, hidden)          # unused in the reference too (:4521)
        self.fc = nn.Conv2d(in_channels, hidden, 1, bias=False)
        self.bn = nn.BatchNorm2d(hidden)
        self.fc_f = nn.Linear(hidden, out_channels)
        self.fc_s = nn.Linear(hidden, kernel_size * kernel_size)
        self.fc_c = nn.Linear(hidden, in_channels)
        self.fc_w = nn.Linear(hidden, K)
        fan_out = kernel_size * kernel_size * out_channels
        with torch.no_grad():
            for i in range(K):
                self.weight[i].normal_(0, math.sqrt(2.0 / fan_out))


class ODConv_3rd(_Packed):
    """ODConv2d_3rd -> BN -> SiLU (models/common.py:4638-4653): GAP kernel -> attention + per-sample weight synthesis
    (with the outer BN folded in) -> per-sample implicit-GEMM conv with SiLU epilogue."""

    def __init__(self, c1, c2, k=1, s=1, kerNums=4, g=1, p=None, act=True):
        super().__init__()
        self.conv = ODConv2d_3rd(c1, c2, k, s, autopad(k, p), groups=g, K=kerNums)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())

    accumulates, folds_pooled = True, False
    # the graph walk's hand-off with a producer that folds_pooled: the forward reads the global average that producer left in its input's Act.pool,
    # backward(defer_pool=True) returns the squeeze gradient as the result's Act.pooled; dx_out has to be a whole UNPADDED tensor
    squeezes_input = True
    reduction = property(lambda self: self.conv.stride)

    # ------------------------------------------------------------------------------------------ training mode
    def _forward_train(self, x):
        cv = self.conv
        dev = x.t.device
        f = lambda t: t.detach().float().contiguous()            # noqa: E731
        B, H, W, _ = x.shape
        k, s, p = cv.kernel_size[0], cv.stride, cv.padding
        cin, cout, kk, K = cv.in_channels, cv.out_channels, k * k, cv.K
        if cin % 4 or cout % 4 or x.coff != 0 or x.t.shape[3] != cin:
            raise NotImplementedError('ODConv training path needs whole tensors with channels % 4 == 0')
        hid = cv.fc.weight.shape[0]
        fcw = f(cv.fc.weight).flatten(1)
        gap = x.pool[0] if x.pool is not None else ops.global_pool(x.t, want_max=False)[0]    # the producer's BatchNorm + SiLU pass may have taken it
        zpre = ops.linear(gap, fcw, None, 'none')
        one, zero = torch.ones(hid, device=dev), torch.zeros(hid, device=dev)
        if B > 1:                                                 # BatchNorm over the B samples (models/common.py:4562-4563)
            st, commit = _bn_train(cv.bn, hid, zpre.view(B, 1, 1, hid))
            commit()
        else:
            st = (zero, one, one, zero)
        z = ops.chan_affine_act(zpre.view(B, 1, 1, hid), hid, 0, st[2], st[3], 'relu', 0, torch.empty(B, 1, 1, hid, device=dev)).view(B, hid)
        na = cout + kk + cin + K
        attn = torch.empty(B, na, device=dev)
        heads = ((cv.fc_f, 0, 'sigmoid'), (cv.fc_s, cout, 'sigmoid'), (cv.fc_c, cout + kk, 'sigmoid'), (cv.fc_w, cout + kk + cin, 'softmax'))
        for lin, off, act in heads:
            ops.linear(z, f(lin.weight), f(lin.bias), act, attn, off)
        Wk = pack_conv_weight(cv.weight.detach().float()).to(dev)            # [K][Cout][kk*Cin]
        biask = f(cv.bias) if cv.bias is not None else None
        wout, bout = ops.odconv_synth(attn, Wk, biask, cin, cin, cout, kk, K)
        Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
        y = torch.empty(B, Ho, Wo, cout, device=dev)
        ops.conv2d_nhwc(x.t, wout, bout, kh=k, kw=k, stride=s, pad=p, act='none', out=y, cout=cout, per_sample_w=True)
        so, commit = _bn_train(self.bn, cout, y)
        commit()
        out = torch.empty_like(y)
        ops.chan_affine_act(y, cout, 0, so[2], so[3], _act_name(self.act), 0, out)
        self.__dict__['_ctx'] = (x, gap, fcw, zpre, st, z, attn, heads, Wk, biask, wout, y, so)
        return Act(out, 0, cout)

    def backward(self, dz, dx_out=None, accumulate=False, need_dx=True, defer_pool=False):
        """dx_out / accumulate: the data gradient is written (added) into that Act (a whole tensor) by the dgrad epilogue.  defer_pool: the squeeze's
        gradient - constant over an image's pixels - is not added here by a pass of its own but handed on as the result's `pooled` part, for the
        producing Conv's BatchNorm backward to fold in."""
        x, gap, fcw, zpre, st, z, attn, heads, Wk, biask, wout, y, so = self.__dict__.pop('_ctx')
        cv = self.conv
        dev = y.device
        B, H, W, _ = x.shape
        k, s, p = cv.kernel_size[0], cv.stride, cv.padding
        cin, cout, kk, K = cv.in_channels, cv.out_channels, k * k, cv.K
        hid = fcw.shape[0]
        f = lambda t: t.detach().float().contiguous()            # noqa: E731
        dy = _bn_backward(self.bn, dz.t, dz.coff, y, so, _act_name(self.act), torch.empty_like(y), cout)
        # per-sample conv: bias, weight and data gradients
        dbias_b, _ = ops.global_pool(dy, want_max=False)
        dbias_b = dbias_b * float(dy.shape[1] * dy.shape[2])                  # sum over pixels = mean * HoWo
        dWb = ops.conv2d_wgrad_nhwc(x.t, dy, kh=k, kw=k, stride=s, pad=p, per_sample_w=True)
        dx = None
        if need_dx:
            wt = wout.view(B, cout, kk, cin).permute(0, 3, 2, 1).contiguous().view(B, cin, kk * cout)
            if dx_out is not None and (dx_out.coff != 0 or dx_out.t.shape[3] != cin):
                raise NotImplementedError('ODConv backward writes whole input-gradient tensors')
            dx = ops.conv2d_dgrad_nhwc(dy, wt, B=B, H=H, W=W, cin=cin, kh=k, kw=k, stride=s, pad=p, per_sample_w=True,
                                       out=None if dx_out is None else dx_out.t, accumulate=dx_out.t if (dx_out is not None and accumulate) else None)
        # synthesis backward
        dWk = torch.zeros_like(Wk)
        dbk = torch.zeros_like(biask) if biask is not None else None
        dattn = ops.odconv_synth_backward(dWb, attn, Wk, biask, dbias_b if biask is not None else None, dWk, dbk, cin, cin, cout, kk, K)
        _acc_grad(cv.weight, dWk.view(K, cout, k, k, cin).permute(0, 1, 4, 2, 3))
        if biask is not None:
            _acc_grad(cv.bias, dbk)
        # attention heads -> dz
        dzv = torch.empty(B, hid, device=dev)
        for i, (lin, off, act) in enumerate(heads):
            gW, gb = torch.zeros_like(lin.weight.data), torch.zeros_like(lin.bias.data)
            ops.linear_backward(z, f(lin.weight), dattn, attn, off, act, gW, gb, dzv, accumulate=i > 0)
            _acc_grad(lin.weight, gW)
            _acc_grad(lin.bias, gb)
        # relu + BatchNorm over the batch (or plain relu for one sample)
        # (one sample: no BatchNorm in the forward (models/common.py:4562), nothing for its parameters)
        dzpre = _bn_backward(cv.bn, dzv.view(B, 1, 1, hid), 0, zpre.view(B, 1, 1, hid), st, 'relu', torch.empty(B, 1, 1, hid, device=dev), hid,
                             batch_stats=B > 1).view(B, hid)
        gfc = torch.zeros_like(fcw)
        dgap = torch.empty_like(gap) if need_dx else None
        ops.linear_backward(gap, fcw, dzpre, dzpre, 0, 'none', gfc, None, dgap)
        _acc_grad(cv.fc.weight, gfc.view_as(cv.fc.weight))
        if not need_dx:
            return None
        res = Act(dx, 0, cin)
        res.pooled = (dgap, None, None)
        return res if defer_pool else settle_pooled(res)

    def _pack(self, dev):
        cv = self.conv
        f = lambda t: t.detach().float().contiguous().to(dev)   # noqa: E731
        s_in, t_in = bn_fold(cv.bn)
        fcw = cv.fc.weight.detach().float().flatten(1)
        pk = dict(fc_w=f(fcw), fc_w_bn=f(fcw * s_in[:, None]), fc_b_bn=f(t_in),
                  Wf=f(cv.fc_f.weight), bf=f(cv.fc_f.bias), Ws=f(cv.fc_s.weight), bs=f(cv.fc_s.bias),
                  Wc=f(cv.fc_c.weight), bc=f(cv.fc_c.bias), Ww=f(cv.fc_w.weight), bw=f(cv.fc_w.bias),
                  Wk=pack_conv_weight(cv.weight.detach().float()).to(dev),           # [K][Cout][kk*Cin_pad]
                  biask=None if cv.bias is None else f(cv.bias))
        s_out, t_out = bn_fold(self.bn)
        pk['bn_s'], pk['bn_t'] = f(s_out), f(t_out)
        return pk

    def forward(self, x):
        if self.training:
            return self._forward_train(x)
        pk = self._packed(x.t.device)
        cv = self.conv
        B, H, W, _ = x.shape
        k, s, p = cv.kernel_size[0], cv.stride, cv.padding
        cin, cin_pad, cout = cv.in_channels, pad4(cv.in_channels), cv.out_channels
        if x.c != cin:
            raise ValueError(f'Expected input{[B, x.c, H, W]} to have {cin} channels, but got {x.c} channels instead')
        if cout % 4 or cin % 4:
            raise NotImplementedError('ODConv channels must be multiples of 4 on the MI355X path')
        gap, _ = ops.global_pool(x.t, c=cin, x_coff=x.coff, want_max=False)
        bn_attn = B > 1                                        # the reference skips the squeeze BN for one sample (:4562)
        wout = torch.empty(B, cout, k * k * cin_pad, device=x.t.device, dtype=torch.float32)
        bout = torch.empty(B, cout, device=x.t.device, dtype=torch.float32)
        ops.odconv_weights(gap, pk['fc_w_bn'] if bn_attn else pk['fc_w'], pk['fc_b_bn'] if bn_attn else None, pk, wout,
                           bout, cin, cin_pad, cout, k * k, cv.K)
        Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
        out = new_act(x.t, Ho, Wo, cout)
        ops.conv2d_nhwc(x.t, wout, bout, kh=k, kw=k, stride=s, pad=p, act=_act_name(self.act), cin=cin_pad,
                        x_coff=x.coff, out=out.t, cout=cout, per_sample_w=True)
        return out


class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


def _seam_stage(c2, act):
    """One stage of SEAM's / MultiSEAM's DCovN (models/common.py:8458-8467, 8513-8522)."""
    return nn.Sequential(Residual(nn.Sequential(nn.Conv2d(c2, c2, 3, 1, 1, groups=c2), act(), nn.BatchNorm2d(c2))),
                         nn.Conv2d(c2, c2, 1, 1, 0, groups=1), act(), nn.BatchNorm2d(c2))


def _seam_width_ok(c):
    """What somi_dwconv3x3_bwd_workspace_floats accepts: C / 4 divides 256."""
    return c % 4 == 0 and 256 % (c // 4) == 0


class _SeamStages(_Packed):
    """What SEAM and MultiSEAM share: the stages {Residual(dw3x3 -> act -> BN) -> 1x1 -> act -> BN} behind a stem -> act -> BN, the last of them
    read by the global average pool only.  `_act` is the activation's name (in front of every BatchNorm: order 1)."""
    accumulates, folds_pooled, reduction = False, False, 1

    def _pack_stage(self, st, dev):
        f = lambda t: t.detach().float().contiguous().to(dev)   # noqa: E731
        pk = dict(dw=f(st[0].fn[0].weight[:, 0].permute(1, 2, 0).reshape(9, -1)), b=f(st[0].fn[0].bias), pw=f(st[1].weight.flatten(1)),
                  pb=f(st[1].bias))
        if self.training:
            pk['pwt'] = pack_dgrad_weight(st[1].weight.detach().float()).to(dev)
        else:
            pk['bn1'], pk['bn2'] = tuple(map(f, bn_fold(st[0].fn[2]))), tuple(map(f, bn_fold(st[3])))
        return pk

    def _bn_train(self, u, bn, residual=None):
        """z = BN_batch(act(u)) [+ residual] (act before the norm, models/common.py:8455-8457; the Residual wrapper's add :7183 rides the same
        pass); returns z and the saved statistics."""
        dev, c, act = u.device, u.shape[3], self._act
        if ops.SYNC_BN is None:
            # two passes over u: the statistics of act(u) taken on the fly, then z = act(u) * scale + shift (order 1) - act(u) is never stored
            # (the backward reads u too); three passes and a tensor less than act -> statistics -> affine
            st, commit = _bn_train(bn, c, u, act=act)
            z = ops.chan_affine_act(u, c, 0, st[2], st[3], act, 1, torch.empty_like(u), residual=residual)
        else:
            vec = _bn_clones(bn)
            g = ops.chan_affine_act(u, c, 0, torch.ones(c, device=dev), torch.zeros(c, device=dev), act, 0, torch.empty_like(u))
            st, commit = _bn_train(bn, c, g, vec=vec)
            z = ops.chan_affine_act(g, c, 0, st[2], st[3], 'none', 0, g, residual=residual)
        commit()
        return z, st

    def _stages_train(self, stages, pks, y0):
        """y0: the stem's output.  -> (the (B, C) global average of the last stage's output, the context _stages_backward reads)."""
        ctx = []
        for i, (st, pk) in enumerate(zip(stages, pks)):
            u1 = ops.dwconv3x3(y0, pk['dw'], pk['b'])
            y1, s1 = self._bn_train(u1, st[0].fn[2], residual=y0)    # Residual: fn(y0) + y0
            u2 = ops.conv2d_nhwc(y1, pk['pw'], pk['pb'], kh=1, kw=1)
            if i + 1 < len(stages):
                y2, s2 = self._bn_train(u2, st[3])
            elif ops.SYNC_BN is None:
                # BN(act(u2)) is read by the global average pool only, and the mean of an affine map is the affine map of the mean: the statistics
                # pass, then ONE pass that averages act(u2) per image and applies scale / shift to the (B,C) result - the normalised tensor is
                # never written
                s2, commit = _bn_train(st[3], c := u2.shape[3], u2, act=self._act)
                commit()
                y2 = ops.global_pool_act(u2, self._act, s2[2], s2[3], c=c)
            else:
                y2, s2 = self._bn_train(u2, st[3])
                y2, _ = ops.global_pool(y2, want_max=False)
            ctx.append((y0, u1, s1, y1, u2, s2))
            y0 = y2
        return y0, ctx

    def _stages_backward(self, stages, pks, ctx, davg):
        """davg (B, C): the gradient of the average _stages_train returned.  Parameter gradients into .grad; -> the gradient of the stem's output."""
        dy2 = None
        for st, pk, (y0, u1, s1, y1, u2, s2) in reversed(list(zip(stages, pks, ctx))):
            c, dev, act = u2.shape[3], u2.device, self._act
            # the last y2 is read by the global average pool only: its gradient is davg / HW at every pixel - handed to the BatchNorm backward
            # as such (no zero tensor filled, added to and read twice)
            du2 = _bn_backward(st[3], dy2, 0, u2, s2, act, torch.empty_like(u2), c, order=1, pooled=(davg, None, None) if dy2 is None else None)
            dy1 = _plain_conv_backward(st[1], Act(y1), du2, pk['pwt'], direct=('bias',)).t
            du1 = _bn_backward(st[0].fn[2], dy1, 0, u1, s1, act, torch.empty_like(u1), c, order=1)
            gw, gb = torch.zeros_like(pk['dw']), torch.zeros(c, device=dev)
            dy2 = ops.dwconv3x3_backward(du1, y0, pk['dw'], gw, gb, dx_accumulate=dy1)       # + the residual branch
            _acc_grad(st[0].fn[0].weight, gw.view(3, 3, c).permute(2, 0, 1).unsqueeze(1))
            _acc_grad(st[0].fn[0].bias, gb)
        return dy2

    def _stages_eval(self, stages, pks, y0):
        act = self._act
        for st, pk in zip(stages, pks):
            y1 = ops.dwconv3x3(y0, pk['dw'], pk['b'], *pk['bn1'], residual=y0, act=act)
            y0 = ops.conv2d_nhwc(y1, pk['pw'], pk['pb'], kh=1, kw=1, act=act, post_scale=pk['bn2'][0], post_shift=pk['bn2'][1])
        return ops.global_pool(y0, want_max=False)[0]


class SEAM(_SeamStages):
    """models/common.py:8448-8505: dw3x3+GELU+BN -> n x [Residual(dw3x3+GELU+BN) -> 1x1+GELU+BN] -> GAP -> MLP -> x*exp(.); the stages are
    DCovN[3] ... DCovN[2 + n], as the reference spreads them."""
    _act = 'gelu'
    accumulates, folds_pooled, reduction = False, False, 1

    def __init__(self, c1, c2, n, reduction=16):
        super().__init__()
        if c1 != c2:
            c2 = c1
        if not isinstance(n, int) or n < 1:
            raise NotImplementedError(f'SEAM with n = {n!r} stages is not on the SOMI path (an int >= 1)')
        self.DCovN = nn.Sequential(nn.Conv2d(c1, c2, 3, 1, 1, groups=c1), nn.GELU(), nn.BatchNorm2d(c2), *(_seam_stage(c2, nn.GELU) for _ in range(n)))
        self.fc = nn.Sequential(nn.Linear(c2, c2 // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(c2 // reduction, c2, bias=False), nn.Sigmoid())
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _stages(self):
        return list(self.DCovN)[3:]

    def _pack(self, dev):
        f = lambda t: t.detach().float().contiguous().to(dev)   # noqa: E731
        d = self.DCovN
        pk = dict(dw0=f(d[0].weight[:, 0].permute(1, 2, 0).reshape(9, -1)), b0=f(d[0].bias), stages=[self._pack_stage(st, dev) for st in self._stages()],
                  W1=f(self.fc[0].weight), W2=f(self.fc[2].weight))
        if not self.training:
            pk['bn0'] = tuple(map(f, bn_fold(d[2])))
        return pk

    # ------------------------------------------------------------------------------------------ training mode
    def _forward_train(self, x):
        self.invalidate()
        pk = self._packed(x.t.device)
        u0 = ops.dwconv3x3(x.t, pk['dw0'], pk['b0'])
        y0, s0 = self._bn_train(u0, self.DCovN[2])
        avg, ctx = self._stages_train(self._stages(), pk['stages'], y0)
        sc = ops.attn_mlp(1, avg, None, pk['W1'], None, pk['W2'], None)
        self.__dict__['_ctx'] = (x, u0, s0, ctx, avg, sc, pk)
        return Act(ops.scale_channels(x.t, sc), 0, x.c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('SEAM writes its own input gradient')
        x, u0, s0, ctx, avg, sc, pk = self.__dict__.pop('_ctx')
        d = self.DCovN
        c = x.c
        dev = x.t.device
        dx, dsc = ops.scale_channels_backward(dout.t, x.t, sc)
        (gW1, gW2), fin = _grad_targets(self.fc[0].weight, self.fc[2].weight)
        davg, _ = ops.attn_mlp_backward(1, dsc, sc, avg, None, pk['W1'], None, pk['W2'], gW1, None, gW2, None)
        fin()
        dy0 = self._stages_backward(self._stages(), pk['stages'], ctx, davg)
        du0 = _bn_backward(d[2], dy0, 0, u0, s0, 'gelu', torch.empty_like(u0), c, order=1)
        gw0, gb0 = torch.zeros_like(pk['dw0']), torch.zeros(c, device=dev)
        dx = ops.dwconv3x3_backward(du0, x.t, pk['dw0'], gw0, gb0, dx_accumulate=dx)
        _acc_grad(d[0].weight, gw0.view(3, 3, c).permute(2, 0, 1).unsqueeze(1))
        _acc_grad(d[0].bias, gb0)
        return Act(dx, 0, c) if need_dx else None

    def forward(self, x):
        if x.coff != 0 or x.t.shape[3] != x.c or x.c % 4:
            raise NotImplementedError('SEAM input must be a whole tensor with channels a multiple of 4')
        if self.training:
            return self._forward_train(x)
        pk = self._packed(x.t.device)
        y0 = ops.dwconv3x3(x.t, pk['dw0'], pk['b0'], *pk['bn0'], act='gelu')
        avg = self._stages_eval(self._stages(), pk['stages'], y0)
        s = ops.attn_mlp(1, avg, None, pk['W1'], None, pk['W2'], None)
        return Act(ops.scale_channels(x.t, s), 0, x.c)


class MultiSEAM(_SeamStages):
    """models/common.py:8508-8555: three DcovN branches - a patch-embedding conv (k = s = p, with bias) + SiLU + BN, then `depth` stages
    {Residual(dw3x3+SiLU+BN) -> 1x1+SiLU+BN} - whose global averages and that of x itself are averaged, -> MLP -> x*exp(.).  Torch's default
    initialisation (the reference's MultiSEAM does not call SEAM's xavier initialiser).  Everything behind the patch convs works on maps p^2
    times smaller; no full-resolution tensor exists besides the output and dx."""
    _act = 'silu'
    accumulates, folds_pooled, reduction = False, False, 1

    def __init__(self, c1, c2, depth, kernel_size=3, patch_size=[3, 5, 7], reduction=16):    # noqa: B006  (the reference's signature)
        super().__init__()
        if c1 != c2:
            c2 = c1
        if kernel_size != 3:
            raise NotImplementedError(f'MultiSEAM with kernel_size {kernel_size!r}: the reference fixes padding=1, so only kernel_size 3 keeps the map size')
        if (not isinstance(patch_size, (list, tuple)) or len(patch_size) != 3 or
                not all(isinstance(p, int) and not isinstance(p, bool) and p > 0 for p in patch_size)):
            raise NotImplementedError(f'MultiSEAM with patch_size {patch_size!r}: three positive ints (one per DCovN branch)')
        if not isinstance(depth, int) or depth < 1:
            raise NotImplementedError(f'MultiSEAM with depth = {depth!r} is not on the SOMI path (an int >= 1)')
        if not _seam_width_ok(c2):
            raise NotImplementedError(f'MultiSEAM at {c2} channels: the depthwise 3x3 backward takes widths whose quarter divides 256 (4 ... 1024)')
        self.patch_size = tuple(patch_size)
        for j, p in enumerate(self.patch_size):
            setattr(self, f'DCovN{j}', nn.Sequential(nn.Conv2d(c1, c2, kernel_size=p, stride=p), nn.SiLU(), nn.BatchNorm2d(c2),
                                                     *(_seam_stage(c2, nn.SiLU) for _ in range(depth))))
        self.fc = nn.Sequential(nn.Linear(c2, c2 // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(c2 // reduction, c2, bias=False), nn.Sigmoid())

    def _branches(self):
        return [getattr(self, f'DCovN{j}') for j in range(3)]

    def _pack(self, dev):
        f = lambda t: t.detach().float().contiguous().to(dev)   # noqa: E731
        pk = dict(W1=f(self.fc[0].weight), W2=f(self.fc[2].weight), br=[])
        for d in self._branches():
            w = d[0].weight.detach().float()
            b = dict(w=pack_conv_weight(w).to(dev), b=f(d[0].bias), stages=[self._pack_stage(st, dev) for st in list(d)[3:]])
            if self.training:
                b['wt'] = pack_dgrad_weight(w).to(dev)
            else:
                b['bn0'] = tuple(map(f, bn_fold(d[2])))
            pk['br'].append(b)
        return pk

    def _check(self, x):
        if x.coff != 0 or x.t.shape[3] != x.c or x.c % 4:
            raise NotImplementedError('MultiSEAM input must be a whole tensor with channels a multiple of 4')
        H, W, p = x.t.shape[1], x.t.shape[2], max(self.patch_size)
        if H < p or W < p:
            raise RuntimeError(f'MultiSEAM: a {H} x {W} map is smaller than its largest patch, {p} x {p}')

    # ------------------------------------------------------------------------------------------ training mode
    def _forward_train(self, x):
        self.invalidate()
        pk = self._packed(x.t.device)
        avgs, ctx = [], []
        for d, b, p in zip(self._branches(), pk['br'], self.patch_size):
            u0 = ops.conv2d_nhwc(x.t, b['w'], b['b'], kh=p, kw=p, stride=p, pad=0)       # bias, no activation: the backward reads u0
            y0, s0 = self._bn_train(u0, d[2])
            a, c = self._stages_train(list(d)[3:], b['stages'], y0)
            avgs.append(a)
            ctx.append((u0, s0, c))
        ax, _ = ops.global_pool(x.t, want_max=False)
        avg = (avgs[0] + avgs[1] + avgs[2] + ax) / 4                    # four (B, C) vectors
        sc = ops.attn_mlp(1, avg, None, pk['W1'], None, pk['W2'], None)
        self.__dict__['_ctx'] = (x, ctx, avg, sc, pk)
        return Act(ops.scale_channels(x.t, sc), 0, x.c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('MultiSEAM writes its own input gradient')
        x, ctx, avg, sc, pk = self.__dict__.pop('_ctx')
        B, H, W, c = x.t.shape
        dev = x.t.device
        dx, dsc = ops.scale_channels_backward(dout.t, x.t, sc)
        (gW1, gW2), fin = _grad_targets(self.fc[0].weight, self.fc[2].weight)
        davg, _ = ops.attn_mlp_backward(1, dsc, sc, avg, None, pk['W1'], None, pk['W2'], gW1, None, gW2, None)
        fin()
        dq = davg / 4                                                   # a quarter to each of the four pools
        if need_dx:
            ops.pool_backward_add_(dx, 0, c, dq)                         # x's own pool: davg / (4 HW) at every pixel
        for d, b, p, (u0, s0, sctx) in zip(self._branches(), pk['br'], self.patch_size, ctx):
            dy0 = self._stages_backward(list(d)[3:], b['stages'], sctx, dq)
            du0 = _bn_backward(d[2], dy0, 0, u0, s0, 'silu', torch.empty_like(u0), c, order=1)
            dw = ops.conv2d_wgrad_nhwc(x.t, du0, kh=p, kw=p, stride=p, pad=0, cin=c, cout=c)
            _acc_grad(d[0].weight, dw.view(c, p, p, c).permute(0, 3, 1, 2))
            (db,), fin = _grad_targets(d[0].bias)
            ops.chan_sum_(du0, c, 0, db)
            fin()
            if need_dx:                                                 # the pixels beyond Ho * p, which no tap reaches, keep what dx holds
                ops.conv2d_dgrad_nhwc(du0, b['wt'], B=B, H=H, W=W, cin=c, kh=p, kw=p, stride=p, pad=0, cout=c, out=dx, accumulate=dx)
        return Act(dx, 0, c) if need_dx else None

    def forward(self, x):
        self._check(x)
        if self.training:
            return self._forward_train(x)
        pk = self._packed(x.t.device)
        avgs = []
        for d, b, p in zip(self._branches(), pk['br'], self.patch_size):
            y0 = ops.conv2d_nhwc(x.t, b['w'], b['b'], kh=p, kw=p, stride=p, pad=0, act='silu', post_scale=b['bn0'][0], post_shift=b['bn0'][1])
            avgs.append(self._stages_eval(list(d)[3:], b['stages'], y0))
        ax, _ = ops.global_pool(x.t, want_max=False)
        s = ops.attn_mlp(1, (avgs[0] + avgs[1] + avgs[2] + ax) / 4, None, pk['W1'], None, pk['W2'], None)
        return Act(ops.scale_channels(x.t, s), 0, x.c)


class Decouple(nn.Module):
    """Decoupled head for one level (models/yolo.py:1042-1073); the [5|nc] interleave happens in the decode kernel."""

    def __init__(self, c1, nc=80, na=3):
        super().__init__()
        c_ = min(c1, 256)
        self.na, self.nc = na, nc
        self.a = Conv(c1, c_, 1)
        c = [int(v + na * 5) for v in (c_ - na * 5) * torch.linspace(1, 0, 4)]
        self.b1, self.b2, self.b3 = Conv(c_, c[1], 3), Conv(c[1], c[2], 3), nn.Conv2d(c[2], na * 5, 1)
        self.c1, self.c2, self.c3 = Conv(c_, c_, 1), Conv(c_, c_, 1), nn.Conv2d(c_, na * nc, 1)
        self.__dict__['_b3'] = PlainConv(self.b3)              # runners share the parameters, stay out of state_dict
        self.__dict__['_c3'] = PlainConv(self.c3)

    def invalidate(self):
        self._b3.invalidate()
        self._c3.invalidate()

    def forward(self, x):
        self._b3.train(self.training), self._c3.train(self.training)
        x = self.a(x)
        b = self._b3(self.b2(self.b1(x)))
        c = self._c3(self.c2(self.c1(x)))
        return b, c

    def backward(self, dbox, dcls):
        d = self.c1.backward(self.c2.backward(self._c3.backward(dcls)))
        d = self.b1.backward(self.b2.backward(self._b3.backward(dbox)), dx_out=d, accumulate=True)
        return self.a.backward(d)


class DecoupledDetect(nn.Module):
    """models/yolo.py:925-980.  forward returns (z, [raw_i]) in eval like the reference; raw_i is (B,na,ny,nx,no)."""
    stride = None
    accumulates, folds_pooled, reduction = False, False, 1       # the head: backward(draws) returns the list of its inputs' gradients

    def __init__(self, nc=10, anchors=(), ch=(), inplace=False):
        super().__init__()
        self.nc, self.no = nc, nc + 5
        self.nl, self.na = len(anchors), len(anchors[0]) // 2
        self.register_buffer('anchors', torch.tensor(anchors).float().view(self.nl, -1, 2))
        self.m = nn.ModuleList(Decouple(c, self.nc, self.na) for c in ch)
        self.inplace = False

    def invalidate(self):
        self.__dict__.pop('_anchors_host', None)

    def forward(self, xs):
        B = xs[0].shape[0]
        dev = xs[0].t.device
        total = sum(self.na * a.shape[1] * a.shape[2] for a in xs)
        z = None if self.training else torch.empty(B, total, self.no, device=dev, dtype=torch.float32)
        raws, row = [], 0
        anchors = self.__dict__.get('_anchors_host')
        if anchors is None:                                   # cached host copy: no device sync per forward
            anchors = self.__dict__['_anchors_host'] = self.anchors.detach().float().cpu()
        for i in range(self.nl):
            b, c = self.m[i](xs[i])
            _, ny, nx, _ = b.shape
            raw = torch.empty(B, self.na, ny, nx, self.no, device=dev, dtype=torch.float32)
            stride = float(self.stride[i])
            ops.detect_decode(b.t, c.t, (anchors[i] * stride).flatten().tolist(), stride, self.na, self.nc, raw=raw,
                              z=z, total=total, row_off=row)
            raws.append(raw)
            row += self.na * ny * nx
            if self.training:
                self.__dict__.setdefault('_ctx', []).append((b.t.shape[3], c.t.shape[3]))
        return raws if self.training else (z, raws)

    def backward(self, draws):
        """draws: gradients w.r.t. the nl training outputs (B,na,ny,nx,no).  Returns the per-level input gradients."""
        widths = self.__dict__.pop('_ctx')
        outs = []
        for i in range(self.nl):
            dbox, dcls = ops.detect_raw_backward(draws[i].contiguous(), widths[i][0], widths[i][1], self.na, self.nc)
            outs.append(self.m[i].backward(dbox, dcls))
        return outs


# ================================================================================================ stock YOLOv5 module set
# north_star: "CSP/Darknet conv backbone, PANet/FPN neck, anchor-based detection head"; BASELINE configs[0] (yolov5s).
class Bottleneck(nn.Module):
    """cv1 -> cv2 (+x) (models/common.py:1494-1509); the shortcut rides cv2's epilogue (forward) and cv1's dgrad epilogue (backward)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2

    accumulates, folds_pooled, reduction = False, False, 1       # takes dx_out / accumulate, but not yet walked that way: it would reorder a sum

    def forward(self, x, out=None):
        return self.cv2(self.cv1(x), out=out, residual=x if self.add else None)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.cv2.backward(dout)
        c1 = self.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0
        dx = self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if self.add and not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class C3(nn.Module):
    """cv3(cat(m(cv1(x)), cv2(x))) (models/common.py:1541-1565).  The concatenation never materialises: the last bottleneck and cv2
    write the two halves of cv3's input buffer; in backward the halves of cv3's data gradient are read in place."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) for _ in range(n)))

    accumulates, folds_pooled, reduction = True, False, 1

    def forward(self, x):
        c_ = self.cv1.conv.out_channels
        if c_ % 4:
            raise NotImplementedError('C3 hidden width must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 2 * c_)
        n = len(self.m)
        t = self.cv1(x, out=cat.slice(0, c_) if n == 0 else None)
        for i, blk in enumerate(self.m):
            t = blk(t, out=cat.slice(0, c_) if i == n - 1 else None)
        self.cv2(x, out=cat.slice(c_, c_))
        return self.cv3(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        c_ = self.cv1.conv.out_channels
        dcat = self.cv3.backward(dout)
        dx = self.cv2.backward(dcat.slice(c_, c_), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        d = dcat.slice(0, c_)
        for blk in reversed(self.m):
            d = blk.backward(d)
        self.cv1.backward(d, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


class SPP(nn.Module):
    """models/common.py:1806-1826: cv1 -> parallel stride-1 max-pools -> concat -> cv2, the pools writing the concat slices in place.

    Two kernel sets, which differ in how a pooled value's gradient is routed at exact ties:
    * the stock sizes (5, 9, 13) run on the kernel SPPF uses: a window of 9 (13) is exactly two (three) chained 5x5 pools, so the VALUES are those of
      the parallel pools, but the gradient walks back through the chain and lands on the first maximum of each 5x5 stage - the same pixel as autograd's
      for distinct values, not always the same one among equal values;
    * every other set (1 to 3 ascending odd sizes, each 3 <= k <= 13: yolov5-p6's (3, 5, 7), yolov5-p7's (3, 5)) runs on the parallel-window kernels of
      pool.hip, which route to the first row-major maximum of the FULL window, as torch's max_pool2d autograd does."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        k = tuple(int(v) for v in k)
        if k != (5, 9, 13) and not (1 <= len(k) <= 3 and all(v % 2 == 1 and 3 <= v <= 13 for v in k) and all(a < b for a, b in zip(k, k[1:]))):
            raise NotImplementedError(f'SPP kernel sizes {k} are not on the SOMI path: 1 to 3 ascending odd window sizes, each 3 <= k <= 13')
        self.k = k
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])    # parameter-free; kept for state_dict / repr parity

    accumulates, folds_pooled, reduction = True, False, 1

    def forward(self, x):
        if self.k == (5, 9, 13):
            return SPPF.forward(self, x)
        c_ = self.cv1.conv.out_channels
        if c_ % 4:
            raise NotImplementedError('SPP hidden width must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, (len(self.k) + 1) * c_)
        self.cv1(x, out=cat.slice(0, c_))
        if self.training:
            self.__dict__['_ctx'] = ops.spp_pool_(cat.t, c_, self.k, 0, codes=True)[1]
        else:
            ops.spp_pool_(cat.t, c_, self.k, 0)
        return self.cv2(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if self.k == (5, 9, 13):
            return SPPF.backward(self, dout, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        codes = self.__dict__.pop('_ctx')
        c_ = self.cv1.conv.out_channels
        dcat = self.cv2.backward(dout)
        ops.spp_pool_backward_(dcat.t, codes, c_, self.k, dcat.coff)
        return self.cv1.backward(dcat.slice(0, c_), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class MaxPool2d(nn.Module):
    """nn.MaxPool2d(2, s, 0), s 1 or 2 (models/hub/yolov3-tiny.yaml; the reference's generic branch, models/yolo.py:1647-1648: channels pass through).
    `pad` = (left, right, top, bottom) of a ZeroPad2d in front of it that parse_model folded in: the kernel reads the zero border, no padded copy."""

    def __init__(self, kernel_size, stride=None, padding=0):
        super().__init__()
        stride = kernel_size if stride is None else stride
        if kernel_size != 2 or stride not in (1, 2) or padding != 0:
            raise NotImplementedError(f'nn.MaxPool2d({kernel_size}, {stride}, {padding}) is not on the SOMI path (kernel 2, stride 1 or 2, padding 0)')
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.pad = (0, 0, 0, 0)

    accumulates, folds_pooled = False, False
    reduction = property(lambda self: self.stride)                # stride 2 halves the map; yolov3-tiny's padded stride-1 pool keeps it

    def extra_repr(self):
        return f'kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, zero_pad={self.pad}'

    def forward(self, x):
        if x.c % 4:
            raise NotImplementedError('MaxPool2d needs a channel count that is a multiple of 4')
        B, H, W, _ = x.shape
        pl, pr, pt, pb = self.pad
        Ho, Wo = ops.maxpool2_out_size(H, self.stride, pt, pb), ops.maxpool2_out_size(W, self.stride, pl, pr)
        out = concat_act(x.t, Ho, Wo, x.c)                        # pad channels (if any) zero, like every activation
        r = ops.maxpool2(x.t, x.c, x.coff, stride=self.stride, pad=self.pad, out=out.t, codes=self.training)
        if self.training:
            self.__dict__['_ctx'] = (r[1], H, W, x.c)
        return out

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        codes, H, W, c = self.__dict__.pop('_ctx')
        if not need_dx:
            return None
        if dx_out is not None or accumulate:
            raise NotImplementedError('MaxPool2d writes its own input gradient')
        dx = concat_act(dout.t, H, W, c)
        ops.maxpool2_backward(dout.t, codes, c, H, W, dout.coff, stride=self.stride, pad=self.pad, out=dx.t)
        return dx


class ZeroPad2d(nn.Module):
    """nn.ZeroPad2d([left, right, top, bottom]) (yolov3-tiny layer 11).  Runs only folded into the MaxPool2d that follows it (parse_model sets that
    pool's `pad` and marks this layer `folded`): then it hands its input through."""

    def __init__(self, padding):
        super().__init__()
        p = (padding,) * 4 if isinstance(padding, int) else tuple(int(v) for v in padding)
        if len(p) != 4 or any(v not in (0, 1) for v in p):
            raise NotImplementedError(f'nn.ZeroPad2d({padding}) is not on the SOMI path (four pads of 0 or 1)')
        self.padding = p
        self.folded = False

    accumulates, folds_pooled, reduction = False, False, 1

    def extra_repr(self):
        return f'padding={self.padding}'

    def forward(self, x):
        if not self.folded:
            raise NotImplementedError(ZeroPad2d.STRAY)
        return x

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('ZeroPad2d hands its gradient through')
        return dout if need_dx else None

    STRAY = 'nn.ZeroPad2d runs only directly in front of an nn.MaxPool2d that is its only reader (folded into the pool kernel)'


class Repeat(nn.Sequential):
    """n > 1 repeats of a module the yaml does not repeat inside itself (models/yolo.py:1650: an nn.Sequential, so the names stay model.<i>.<j>...):
    forward and backward walk the children."""

    accumulates, folds_pooled = False, False
    reduction = property(lambda self: math.prod(m.reduction for m in self))

    def forward(self, x):
        for m in self:
            x = m(x)
        return x

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        mods = list(self)
        for m in mods[:0:-1]:
            dout = m.backward(dout)
        return mods[0].backward(dout, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class BottleneckCSP(_Packed):
    """cv4(silu(bn(cat(cv3(m(cv1(x))), cv2(x))))) (models/common.py:1512-1538); cv2 / cv3 are plain bias-free 1x1 nn.Conv2d, m's bottlenecks 3x3 -> 3x3
    with e = 1.  No torch.cat: cv3 and cv2 write the two halves of one buffer, and since BatchNorm is per channel, `bn` over the concat is two
    slices of one BatchNorm.  Eval: each slice folds into its conv, SiLU in the epilogue - two launches for cv3 / cv2 / bn / act.  Training: each conv
    leaves its BatchNorm partial sums from the conv epilogue, bn_stats_from_partials + the affine/SiLU sweep run per half on slices of bn's
    parameters and running statistics (in place); backward mirrors it with the BatchNorm/SiLU backward per half and the dense wgrad / dgrad kernels."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = nn.Conv2d(c1, c_, 1, 1, bias=False)
        self.cv3 = nn.Conv2d(c_, c_, 1, 1, bias=False)
        self.cv4 = Conv(2 * c_, c2, 1, 1)
        self.bn = nn.BatchNorm2d(2 * c_)
        self.act = nn.SiLU()
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))

    accumulates, folds_pooled, reduction = True, False, 1

    def _pack_params(self):
        return self.cv2.weight, self.cv3.weight, self.bn.weight, self.bn.bias      # the children pack themselves

    def _pack(self, dev):
        c_ = self.cv3.out_channels
        if c_ % 4 or pad4(c_) != c_:
            raise NotImplementedError('BottleneckCSP hidden width must be a multiple of 4 (of 32 from 64 up) on the MI355X path')
        if not self.training:                                    # the two slices of bn fold into cv3 / cv2
            s, t = bn_fold(self.bn)
            return [_pack_wb(conv.weight.detach().float() * s[o:o + c_].view(-1, 1, 1, 1), t[o:o + c_], dev)
                    for conv, o in ((self.cv3, 0), (self.cv2, c_))]
        pk = {}
        for name, conv in (('3', self.cv3), ('2', self.cv2)):
            w = conv.weight
            c1p = pad4(conv.in_channels)
            if c1p == conv.in_channels and w.device == dev and w.dtype == torch.float32 and w.is_contiguous():
                wp = w.detach().view(c_, c1p)                    # a 1x1 weight without pads IS its forward packing [cout][cin]
            else:
                wp = pack_conv_weight(w.detach().float(), cout_pad=c_).to(dev)
            pk['w' + name], pk['t' + name] = wp, ops.pack_dgrad_weights(wp, c_, 1, c1p)
        bn = self.bn
        if bn.weight.device != dev:
            raise RuntimeError('BottleneckCSP: move the module to the device before a training forward')
        vec = _bn_vectors(bn, dev, 2 * c_)                       # bn's own tensors, updated in place: cv3's half, then cv2's
        pk['bn'] = [{k: v if k == 'inplace' else v[o:o + c_] for k, v in vec.items()} for o in (0, c_)]
        return pk

    def forward(self, x):
        pk = self._packed(x.t.device)
        c_ = self.cv3.out_channels
        B, H, W, _ = x.shape
        t = self.cv1(x)
        for blk in self.m:
            t = blk(t)
        z = concat_act(x.t, H, W, 2 * c_)
        if not self.training:
            for (wp, bp), src, o in ((pk[0], t, 0), (pk[1], x, c_)):
                ops.conv2d_nhwc(src.t, wp, bp, kh=1, kw=1, stride=1, pad=0, act='silu', cin=pad4(src.c), x_coff=src.coff, out=z.t, cout=c_, y_coff=o,
                                alg_cin=src.c, alg_cout=c_)
            return self.cv4(z)
        y = torch.empty(B, H, W, 2 * c_, device=x.t.device, dtype=torch.float32)     # raw cv3 | cv2 outputs: what bn normalises
        stats = []
        for name, src, o, vec in (('3', t, 0, pk['bn'][0]), ('2', x, c_, pk['bn'][1])):
            st = {'pivot': vec['rm']}
            ops.conv2d_nhwc(src.t, pk['w' + name], None, kh=1, kw=1, stride=1, pad=0, act='none', cin=pad4(src.c), x_coff=src.coff, out=y, cout=c_,
                            y_coff=o, alg_cin=src.c, alg_cout=c_, bn_stats=st)
            s4, commit = _bn_train(self.bn, c_, partials=st, npix=B * H * W, vec=vec)
            ops.chan_affine_act(y, c_, o, s4[2], s4[3], 'silu', 0, z.t, o)
            stats.append(s4)
        commit()                                                 # both halves ran in place on bn's own buffers: one step counted
        self.__dict__['_ctx'] = (x, t, y, stats, pk)
        return self.cv4(z)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        x, t, y, stats, pk = self.__dict__.pop('_ctx')
        c_ = self.cv3.out_channels
        dz = self.cv4.backward(dout)
        dy = torch.empty_like(y)
        (gw, gb), fin = _grad_targets(self.bn.weight, self.bn.bias)
        for st, o in zip(stats, (0, c_)):
            _bn_backward(self.bn, dz.t, dz.coff + o, y, st, 'silu', dy, c_, coff=o, targets=(gw[o:o + c_], gb[o:o + c_]))
        fin()
        dx = _plain_conv_backward(self.cv2, x, dy, pk['t2'], dy_coff=c_, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, direct=('weight',))
        d = _plain_conv_backward(self.cv3, t, dy, pk['t3'], direct=('weight',))
        for blk in reversed(self.m):
            d = blk.backward(d)
        self.cv1.backward(d, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


class Focus(nn.Module):
    """Space-to-depth + Conv (models/common.py:1973-1997)."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        if act is not True:
            raise NotImplementedError("the reference passes `act` into Conv's dilation slot (models/common.py:1993); only act=True runs there")
        self.conv = Conv(c1 * 4, c2, k, s, p, g)

    accumulates, folds_pooled = False, False
    reduction = property(lambda self: 2 * self.conv.reduction)

    def forward(self, x):
        if x.shape[1] % 2 or x.shape[2] % 2:
            raise RuntimeError('Focus needs even height and width')
        deep = ops.space_to_depth(x.t, x.coff, x.c)
        return self.conv(Act(deep, 0, 4 * x.c))

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.conv.backward(dout, need_dx=need_dx)
        if not need_dx:
            return None
        if dx_out is not None or accumulate:
            raise NotImplementedError('Focus writes its own input gradient')
        c = self.conv.conv.in_channels // 4
        return Act(ops.space_to_depth(d.t, d.coff, c, inverse=True), 0, c)


class DWConv(Conv):
    """Conv with g = gcd(c1, c2) (models/common.py:9580-9583): depthwise when c1 == c2, a channel multiplier or gcd grouping otherwise."""

    def __init__(self, c1, c2, k=1, s=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), act=act)

    folds_pooled = False      # the pools ride the dense Conv's passes only


class GhostConv(nn.Module):
    """cat(cv1(x), cv2(cv1(x))) with cv2 a 5x5 depthwise Conv (models/common.py:2001-2011).  cv1 writes channels [0, c_) of the output,
    cv2 reads them and writes [c_, 2c_): no torch.cat.  act=False is no activation on both convs (the reference's own class passes `act`
    into Conv's dilation slot and cannot run with act=False)."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act=act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act=act)

    accumulates, folds_pooled = True, False
    reduction = property(lambda self: self.cv1.reduction)

    def forward(self, x, out=None, residual=None):
        """residual: an Act of 2c_ channels added to the output (GhostBottleneck's shortcut): its halves ride the two convs' output passes -
        cv1's output then goes to a tensor of its own first (cv2 reads it without the residual)."""
        c_ = self.cv1.conv.out_channels
        if c_ % 4:
            raise NotImplementedError('GhostConv hidden width must be a multiple of 4 on the MI355X path')
        k, s = self.cv1.conv.kernel_size[0], self.cv1.conv.stride[0]
        H, W = x.shape[1], x.shape[2]
        Ho, Wo = ops.conv_out_size(H, k, s, k // 2), ops.conv_out_size(W, k, s, k // 2)
        if out is None:
            out = concat_act(x.t, Ho, Wo, 2 * c_)
        t = self.cv1(x, out=out.slice(0, c_) if residual is None else None)
        self.cv2(t, out=out.slice(c_, c_), residual=None if residual is None else residual.slice(c_, c_))
        if residual is not None:
            ops.add_(t.t, t.coff, residual.t, residual.coff, c_, out=out.t, out_coff=out.coff)
        return Act(out.t, out.coff, 2 * c_)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True, also_add=None):
        """The first half's gradient is dout[0, c_) plus what flows back through cv2: one dgrad pass writes their sum."""
        c_ = self.cv1.conv.out_channels
        dt = self.cv2.backward(dout.slice(c_, c_), also_add=dout.slice(0, c_))
        return self.cv1.backward(dt, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=also_add)


class GhostBottleneck(nn.Module):
    """conv(x) + shortcut(x) (models/common.py:2014-2029): GhostConv -> [depthwise k x k, stride 2] -> GhostConv(act=False); the shortcut is
    the identity (s = 1) or depthwise stride 2 -> 1x1 Conv (s = 2), both without activation.  The sum rides the last GhostConv's passes."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1),
                                  DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    @property
    def stride(self):
        return 2 if isinstance(self.conv[1], Conv) else 1

    accumulates, folds_pooled, reduction = True, False, stride

    def forward(self, x, out=None):
        g1, dw, g2 = self.conv
        if self.stride == 2:
            sc = self.shortcut[1](self.shortcut[0](x))
            t = dw(g1(x))
        else:
            if x.c != g2.cv1.conv.out_channels * 2:
                raise RuntimeError(f'GhostBottleneck(s=1) adds its input to its output: {x.c} and {2 * g2.cv1.conv.out_channels} channels')
            sc, t = x, g1(x)
        return g2(t, out=out, residual=sc)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        g1, dw, g2 = self.conv
        d = g2.backward(dout)
        if self.stride == 2:
            dx = g1.backward(dw.backward(d), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
            ds = self.shortcut[1].backward(dout)
            return self.shortcut[0].backward(ds, dx_out=dx, accumulate=True, need_dx=need_dx)
        c1 = g1.cv1.conv.in_channels
        fuse = pad4(c1) == c1 and dout.coff % 4 == 0             # the identity shortcut's gradient rides the dgrad epilogue
        dx = g1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class C3Ghost(C3):
    """C3 whose bottlenecks are GhostBottleneck(c_, c_) (models/common.py:1798-1803); `shortcut` is ignored there too."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(GhostBottleneck(c_, c_) for _ in range(n)))


class GSConv(nn.Module):
    """Slim-neck GSConv (models/common.py:9586-9610): x1 = cv1(x), x_2 = cv2_2(cv2_1(x1)) - two stacked depthwise 3x3 Convs, not the paper's
    one 5x5 - and the fixed de-interleave of cat(x1, x_2): output channel o reads source 2 o for o < c_, 2 (o - c_) + 1 otherwise.
    Eval: cv1's launch, then ONE launch for everything behind it (ops.gs_tail: both depthwise convs with their folded BatchNorms and
    activations, the shuffle, the residual).  Training: the three Convs' own passes, cv2_2's BatchNorm + activation pass being the one that also
    shuffles (ops.gs_shuffle_affine_act); backward is one un-shuffle pass in front of the three Convs' backward chain.
    act=False switches the activation off on all three convs."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, p, g, d, act)
        self.cv2_1 = Conv(c_, c_, 3, 1, p, c_, d, act)
        self.cv2_2 = Conv(c_, c_, 3, 1, p, c_, d, act)

    accumulates = folds_pooled = False                            # Conv's own are True: the shuffle stands between this block's output and a Conv
    reduction = property(lambda self: self.cv1.reduction)

    def forward(self, x, out=None, residual=None):
        """out: the 2 c_ wide slice to write (a tensor of its own when None); residual: an Act of 2 c_ channels added to the shuffled output."""
        c_ = self.cv1.conv.out_channels
        if c_ % 4:
            raise NotImplementedError(f'GSConv half width {c_} (c2 // 2) must be a multiple of 4 on the MI355X path')
        x1 = self.cv1(x)
        if out is None:
            out = new_act(x1.t, x1.shape[1], x1.shape[2], 2 * c_)
        res_t, res_coff = (None, 0) if residual is None else (residual.t, residual.coff)
        act = _act_name(self.cv2_2.act)
        if not self.training:
            (w1, b1), (w2, b2) = self.cv2_1._packed(x1.t.device), self.cv2_2._packed(x1.t.device)
            ops.gs_tail(x1.t, w1, b1, w2, b2, c_, act, x1.coff, out=out.t, o_coff=out.coff, residual=res_t, res_coff=res_coff)
            return Act(out.t, out.coff, 2 * c_)
        t = self.cv2_1(x1)
        m = self.cv2_2                                            # Conv._forward_train up to its BatchNorm + activation pass, which the shuffle is
        pk = m._packed(t.t.device)
        B, H, W, _ = t.shape
        y = torch.empty(B, H, W, c_, device=t.t.device, dtype=torch.float32)
        st = {'pivot': pk['rm']}
        ops.gconv2d_nhwc(t.t, pk['gw'], c1=c_, c2=c_, groups=c_, k=3, stride=1, x_coff=t.coff, out=y, cw=c_, bn_stats=st)
        (mean, rstd, scale, shift), commit = _bn_train(m.bn, c_, y, partials=st, npix=B * H * W, vec=pk)
        commit()
        m.__dict__['_ctx'] = (t, y, mean, rstd, scale, shift, pk)
        ops.gs_shuffle_affine_act(x1.t, y, c_, scale, shift, act, x1.coff, 0, out=out.t, o_coff=out.coff, residual=res_t, res_coff=res_coff)
        return Act(out.t, out.coff, 2 * c_)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True, also_add=None):
        """x1's gradient is its half of the un-shuffled dout plus what flows back through the two depthwise convs: cv2_1's dgrad pass writes the sum."""
        c_ = self.cv1.conv.out_channels
        d1, d2 = ops.gs_unshuffle(dout.t, c_, dout.coff)
        dt = self.cv2_2.backward(Act(d2, 0, c_))
        dx1 = self.cv2_1.backward(dt, also_add=Act(d1, 0, c_))
        return self.cv1.backward(dx1, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=also_add)


class GSBottleneck(nn.Module):
    """conv_lighting(x) + shortcut(x) (models/common.py:9628-9642): GSConv 1x1 -> GSConv 3x3 without activation, and a 1x1 Conv without
    activation as the shortcut, always added: it rides the second GSConv's output pass."""

    def __init__(self, c1, c2, k=3, s=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.conv_lighting = nn.Sequential(GSConv(c1, c_, 1, 1), GSConv(c_, c2, 3, 1, act=False))
        self.shortcut = Conv(c1, c2, 1, 1, act=False)

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x, out=None):
        g1, g2 = self.conv_lighting
        return g2(g1(x), out=out, residual=self.shortcut(x))

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        g1, g2 = self.conv_lighting
        dx = g1.backward(g2.backward(dout), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        self.shortcut.backward(dout, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


class VoVGSCSP(nn.Module):
    """cv3(cat(cv2(x), gsb(cv1(x)))) (models/common.py:9665-9681), cv2's branch first.  cv2 and the last bottleneck write the two halves of
    cv3's input buffer.  `res` is built, loaded and saved like the reference's and, like there, never runs: no gradient, its running statistics
    and step counter stay as loaded, and no optimizer step moves it (never_runs, read by optim.FusedAdamEMA)."""
    never_runs = ('res',)

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.gsb = nn.Sequential(*(GSBottleneck(c_, c_, e=1.0) for _ in range(n)))
        self.res = Conv(c_, c_, 3, 1, act=False)
        self.cv3 = Conv(2 * c_, c2, 1)

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x):
        c_ = self.cv1.conv.out_channels
        if c_ % 4:
            raise NotImplementedError(f'{type(self).__name__} hidden width {c_} must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 2 * c_)
        n = len(self.gsb)
        self.cv2(x, out=cat.slice(0, c_))
        t = self.cv1(x, out=cat.slice(c_, c_) if n == 0 else None)
        for i, blk in enumerate(self.gsb):
            t = blk(t, out=cat.slice(c_, c_) if i == n - 1 else None)
        return self.cv3(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        c_ = self.cv1.conv.out_channels
        dcat = self.cv3.backward(dout)
        dx = self.cv2.backward(dcat.slice(0, c_), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        d = dcat.slice(c_, c_)
        for blk in reversed(self.gsb):
            d = blk.backward(d)
        self.cv1.backward(d, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


class GSCBAMBottleneck(nn.Module):
    """GSConv -> channel attention -> spatial attention -> GSConv without activation (+ x) (models/common.py:737-757): CBAMBottleneck's layout
    without its step-C-in-BatchNorm fusion, which needs a Conv right in front of the attention.  The CBAM training path works on whole
    unpadded tensors, so the hidden width c_ must be a multiple of 4 (of 8 for the GSConv that writes it)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, k=(1, 3), ratio=8, kernel_size=3):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = GSConv(c1, c_, k[0], 1)
        self.cv2 = GSConv(c_, c2, k[1], 1, act=False)
        self.add = shortcut and c1 == c2
        self.channel_attention = ChannelAttentionModule(c_, ratio)
        self.spatial_attention = SpatialAttentionModule(kernel_size)

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x, out=None):
        t = self.cv1(x)
        ca = self.channel_attention(t)
        t2 = self.spatial_attention(t, ca)                        # eval: t scaled in place; training: a new tensor, t is kept
        return self.cv2(t2, out=out, residual=x if self.add else None)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.cv2.backward(dout)                               # d(t * ca * sa), a whole tensor of its own
        dca, amaxp = self.spatial_attention.backward(d.t, t_max=self.channel_attention.__dict__['_ctx'][2], bn=None)
        self.channel_attention.backward(dca, d, amaxp)            # adds the pooled paths into d in place
        c1 = self.cv1.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0  # the shortcut's gradient rides cv1's dgrad epilogue
        dx = self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if self.add and not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class VoVGSCSPCBAM(VoVGSCSP):
    """VoVGSCSP whose bottlenecks are GSCBAMBottleneck(c_, c_, e=1.0) (models/common.py:2697-2711); `shortcut` is ignored there too, and
    `res` is as unused."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.gsb = nn.Sequential(*(GSCBAMBottleneck(c_, c_, e=1.0) for _ in range(n)))


class C2f(nn.Module):
    """cv2(cat(cv1(x).chunk(2), m_1, ..., m_n)) (models/common.py:2638-2658), laid out like C2fCBAM: all (2+n) pieces live in one buffer,
    block i reads piece i+1 and writes piece i+2.  In backward a block's data gradient is added into the piece that already holds cv2's."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    accumulates, folds_pooled, reduction = True, False, 1

    def forward(self, x):
        c, n = self.c, len(self.m)
        if c % 4:
            raise NotImplementedError(f'{type(self).__name__} hidden width must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, (2 + n) * c)
        self.cv1(x, out=cat.slice(0, 2 * c))
        for i, blk in enumerate(self.m):
            blk(cat.slice((1 + i) * c, c), out=cat.slice((2 + i) * c, c))
        return self.cv2(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        c, n = self.c, len(self.m)
        dcat = self.cv2.backward(dout)
        for i in reversed(range(n)):
            self.m[i].backward(dcat.slice((2 + i) * c, c), dx_out=dcat.slice((1 + i) * c, c), accumulate=True)
        return self.cv1.backward(dcat.slice(0, 2 * c), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class SCDown(nn.Module):
    """1x1 Conv -> k x k depthwise Conv, stride s, BatchNorm, no activation (models/common.py:7192-7200)."""

    def __init__(self, c1, c2, k, s):
        super().__init__()
        self.cv1 = Conv(c1, c2, 1, 1)
        self.cv2 = Conv(c2, c2, k=k, s=s, g=c2, act=False)

    accumulates, folds_pooled = True, False
    reduction = property(lambda self: self.cv2.reduction)

    def forward(self, x, out=None):
        return self.cv2(self.cv1(x), out=out)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        return self.cv1.backward(self.cv2.backward(dout), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class CIB(nn.Module):
    """dw3x3 -> 1x1 -> dw3x3 -> 1x1 -> dw3x3, all Conv+BN+SiLU, (+x) (models/common.py:8981-9002).  The shortcut rides the last depthwise
    conv's output pass in forward and the first one's data-gradient pass in backward."""

    def __init__(self, c1, c2, shortcut=True, e=0.5, lk=False):
        super().__init__()
        if lk:
            raise NotImplementedError("CIB(lk=True): RepVGGDW's 7x7 depthwise conv is outside the grouped conv kernels (k 1/3/5)")
        c_ = int(c2 * e)
        self.cv1 = nn.Sequential(Conv(c1, c1, 3, g=c1), Conv(c1, 2 * c_, 1), Conv(2 * c_, 2 * c_, 3, g=2 * c_), Conv(2 * c_, c2, 1),
                                 Conv(c2, c2, 3, g=c2))
        self.add = shortcut and c1 == c2

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x, out=None):
        t = x
        for m in self.cv1[:-1]:
            t = m(t)
        return self.cv1[-1](t, out=out, residual=x if self.add else None)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = dout
        for m in reversed(self.cv1[1:]):
            d = m.backward(d)
        return self.cv1[0].backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if self.add else None)


class C2fCIB(C2f):
    """C2f whose blocks are CIB(c, c, shortcut, e=1.0, lk) (models/common.py:9005-9013)."""

    def __init__(self, c1, c2, n=1, shortcut=False, lk=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(CIB(self.c, self.c, shortcut, e=1.0, lk=lk) for _ in range(n))


class AttentionPSA(nn.Module):
    """proj(attention(q, k, v) + pe(v)) over the H*W tokens of each image (models/common.py:7203-7230).  The attention kernels
    (attention.hip) read q, k and v in place from qkv's output; the forward also leaves v as a contiguous tensor, which is pe's input, and pe
    takes the attention output as its residual, so o + pe(v) is one pass.  In backward, pe's data gradient is the attention's dv addend."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim ** -0.5
        if self.head_dim != 64 or self.key_dim != 32 or dim != 64 * num_heads:
            raise NotImplementedError(f'AttentionPSA({dim}, {num_heads}, {attn_ratio}): the attention kernels need head_dim 64 and key_dim 32 '
                                      f'(dim = 64 * num_heads, attn_ratio 0.5), got {self.head_dim} / {self.key_dim}')
        self.qkv = Conv(dim, dim + 2 * self.key_dim * num_heads, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x, out=None, residual=None):
        """residual: an Act added to the output in proj's pass (PSA's b + attn(b))."""
        dim, nh = self.proj.conv.out_channels, self.num_heads
        qkv = self.qkv(x)
        o, lse, v = ops.psa_attention(qkv.t, nh, qkv_coff=qkv.coff, lse=self.training, v_out=True)
        t = self.pe(Act(v, 0, dim), residual=Act(o, 0, dim))
        if self.training:
            self.__dict__['_ctx'] = (qkv, o, lse)
        return self.proj(t, out=out, residual=residual)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True, also_add=None):
        qkv, o, lse = self.__dict__.pop('_ctx')
        nh = self.num_heads
        dt = self.proj.backward(dout)                             # the gradient of o + pe(v): dO of the attention and pe's output gradient
        dv = self.pe.backward(dt)
        B, H, W, _ = dt.shape
        dqkv = torch.empty(B, H, W, 128 * nh, device=dt.t.device, dtype=torch.float32)
        ops.psa_attention_backward(qkv.t, o, dt.t, lse, nh, qkv_coff=qkv.coff, do_coff=dt.coff, out=dqkv, dv_add=dv.t)
        return self.qkv.backward(Act(dqkv, 0, 128 * nh), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=also_add)


class PSA(nn.Module):
    """cv2(cat(a, b2)) with a, b = cv1(x).split, b1 = b + attn(b), b2 = b1 + ffn(b1) (models/common.py:7233-7255).  cv1 writes [a | b] into
    cv2's input buffer; b is copied out once (attn.qkv's weight gradient still needs it after b2 has taken its place).  Both residual sums
    ride the output passes of attn.proj and ffn[1]; in backward they ride the data-gradient passes of ffn[0] and attn.qkv, and qkv's writes
    b's gradient next to a's, so cv1 reads one buffer."""

    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        if c1 != c2:
            raise ValueError(f'PSA needs c1 == c2, got {c1} and {c2}')
        self.c = int(c1 * e)
        if self.c % 64 or self.c == 0:
            raise NotImplementedError(f'PSA with {self.c} channels per branch: the attention kernels need head_dim 64 / key_dim 32, i.e. '
                                      f'channels per branch a multiple of 64')
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.attn = AttentionPSA(self.c, attn_ratio=0.5, num_heads=self.c // 64)
        self.ffn = nn.Sequential(Conv(self.c, self.c * 2, 1), Conv(self.c * 2, self.c, 1, act=False))

    accumulates, folds_pooled, reduction = True, False, 1

    def forward(self, x):
        c = self.c
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 2 * c)
        self.cv1(x, out=cat)
        b = new_act(x.t, H, W, c)
        ops.resample_slice(cat.t, c, b.t, 0, c)
        b1 = self.attn(b, residual=b)
        self.ffn[1](self.ffn[0](b1), out=cat.slice(c, c), residual=b1)
        return self.cv2(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        c = self.c
        dcat = self.cv2.backward(dout)
        db2 = dcat.slice(c, c)
        db1 = self.ffn[0].backward(self.ffn[1].backward(db2), also_add=db2)
        self.attn.backward(db1, dx_out=db2, also_add=db1)         # db2's slice is free again: it takes b's gradient
        return self.cv1.backward(dcat, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


# ------------------------------------------------------------------------------------------------ Swin (C3STR)
def swin_region_ids(hp, wp, window_size=8, shift_size=4):
    """The region ids a shifted layer masks by: create_mask's img_mask (models/common.py:1295-1306) on the padded map, (hp, wp) in the
    reference's frame - hp is ITS axis 1, which runs along the map's W (SwinTransformerLayer.forward names b, c, w, h = x.shape and permutes to
    (b, h, w, c), :1317-1318).  The first entry of the reference's h_slices is the tuple (0, -window_size), not a slice: an index list, so
    along that axis only rows 0 and hp - window_size take the first group's ids - the latter overwritten by the second group - and the rows
    between keep 0.  Reproduced as written.  -> int32 (hp, wp)."""
    m = torch.zeros(hp, wp, dtype=torch.int32)
    rows = ([0, hp - window_size], slice(hp - window_size, hp - shift_size), slice(hp - shift_size, hp))
    cols = (slice(0, wp - window_size), slice(wp - window_size, wp - shift_size), slice(wp - shift_size, wp))
    cnt = 0
    for r in rows:
        for c in cols:
            m[r, c] = cnt
            cnt += 1
    return m


def _whole(a, c, what):
    if a.coff != 0 or a.c != c or a.t.shape[3] != c:
        raise NotImplementedError(f'{what} takes a whole (B,H,W,{c}) tensor, got channels [{a.coff}, {a.coff + a.c}) of {a.t.shape[3]}')
    return a.t


def _linear_backward(lin, src, dy, wt):
    """Backward of an nn.Linear run as a 1x1 NHWC convolution over the whole tensor `src`: weight and bias gradients into .grad (the weight's
    straight into a contiguous fp32 .grad - the optimizer's flat view - by the wgrad kernel), -> the data gradient.  wt: weight.t(), contiguous."""
    c2, c1 = lin.weight.shape
    g = lin.weight.grad
    if g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.device == dy.device:
        ops.conv2d_wgrad_nhwc(src, dy, kh=1, kw=1, cin=c1, cout=c2, out=g, accumulate=g)
    else:
        _acc_grad(lin.weight, ops.conv2d_wgrad_nhwc(src, dy, kh=1, kw=1, cin=c1, cout=c2))
    if lin.bias is not None:
        (db,), fin = _grad_targets(lin.bias)
        ops.chan_sum_(dy, c2, 0, db)
        fin()
    B, H, W, _ = src.shape
    return ops.conv2d_dgrad_nhwc(dy, wt, B=B, H=H, W=W, cin=c1, kh=1, kw=1, cout=c2)


def _f32dev(t, dev):
    return t.detach().float().contiguous().to(dev)


class WindowAttention(_Packed):
    """proj(window attention(qkv(x))) (models/common.py:1184-1264) with the reference's constructor, parameter and buffer names.  It runs on the
    NHWC map, not on partitioned windows: forward(x, shift, region_ids) takes the normalised (B,H,W,C) tensor; the cyclic shift, the padding,
    the window partition and their inverses happen inside the attention kernels (swin.hip).  Window 8x8, head_dim 32, no qkv bias, no dropout."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, tuple(window_size), num_heads
        if self.window_size != (8, 8):
            raise NotImplementedError(f'WindowAttention: window {self.window_size}: the attention kernels have window 8x8')
        if num_heads < 1 or dim != 32 * num_heads:
            raise NotImplementedError(f'WindowAttention({dim}, heads {num_heads}): the attention kernels need head_dim 32 (dim = 32 * num_heads; '
                                      f'C3STR: hidden width c_ a multiple of 32)')
        if qkv_bias or attn_drop or proj_drop:
            raise NotImplementedError('WindowAttention: qkv_bias / dropout are not on the path (C3STR uses neither)')
        self.scale = (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros(15 * 15, num_heads))
        co = torch.stack(torch.meshgrid([torch.arange(8), torch.arange(8)], indexing='ij')).flatten(1)
        rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous() + 7
        self.register_buffer('relative_position_index', rel[:, :, 0] * 15 + rel[:, :, 1])   # kept for state dicts; the kernels compute it
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack(self, dev):
        pk = dict(wqkv=_f32dev(self.qkv.weight, dev), wproj=_f32dev(self.proj.weight, dev), bproj=_f32dev(self.proj.bias, dev),
                  table=_f32dev(self.relative_position_bias_table, dev))
        if self.training:
            pk.update(wqkv_t=_f32dev(self.qkv.weight.t(), dev), wproj_t=_f32dev(self.proj.weight.t(), dev))
        return pk

    def forward(self, x, shift=0, region_ids=None, residual=None):
        """x: the (B,H,W,C) tensor behind norm1; residual: a tensor added in proj's pass (the layer's shortcut)."""
        pk = self._packed(x.device)
        qkv = ops.conv2d_nhwc(x, pk['wqkv'], None, kh=1, kw=1)
        o, lse = ops.window_attention(qkv, pk['table'], self.num_heads, shift, region_ids, lse=self.training)
        if self.training:
            self.__dict__['_ctx'] = (x, qkv, o, lse, shift, region_ids, pk)
        return ops.conv2d_nhwc(o, pk['wproj'], pk['bproj'], kh=1, kw=1, residual=residual)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('WindowAttention writes its own input gradient')
        x, qkv, o, lse, shift, region_ids, pk = self.__dict__.pop('_ctx')
        do = _linear_backward(self.proj, o, dout, pk['wproj_t'])
        (gt,), fin = _grad_targets(self.relative_position_bias_table)
        dqkv = ops.window_attention_backward(qkv, pk['table'], do, lse, self.num_heads, shift, region_ids, dtable=gt)
        fin()
        return _linear_backward(self.qkv, x, dqkv, pk['wqkv_t'])


class Mlp(_Packed):
    """fc2(GELU(fc1(x))) (models/common.py:1147-1168), the Linear layers as 1x1 NHWC convolutions.  Eval: GELU rides fc1's epilogue; training
    keeps fc1's output (the GELU backward reads it) and applies the GELU in a pass of its own."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if act_layer is not nn.GELU or drop:
            raise NotImplementedError('Mlp: exact GELU and no dropout on the path')
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack(self, dev):
        pk = dict(w1=_f32dev(self.fc1.weight, dev), b1=_f32dev(self.fc1.bias, dev), w2=_f32dev(self.fc2.weight, dev), b2=_f32dev(self.fc2.bias, dev))
        if self.training:
            hid = self.fc1.out_features
            pk.update(w1_t=_f32dev(self.fc1.weight.t(), dev), w2_t=_f32dev(self.fc2.weight.t(), dev), one=torch.ones(hid, device=dev),
                      zero=torch.zeros(hid, device=dev))
        return pk

    def forward(self, x, residual=None, out=None):
        """x: a whole (B,H,W,C) tensor; residual: added in fc2's pass; out: the Act (channel slice) fc2 writes."""
        pk = self._packed(x.device)
        hid, c2 = self.fc1.out_features, self.fc2.out_features
        if self.training:
            u = ops.conv2d_nhwc(x, pk['w1'], pk['b1'], kh=1, kw=1)
            g = ops.chan_affine_act(u, hid, 0, pk['one'], pk['zero'], 'gelu', 0, torch.empty_like(u))
            self.__dict__['_ctx'] = (x, u, g, pk)
        else:
            g = ops.conv2d_nhwc(x, pk['w1'], pk['b1'], kh=1, kw=1, act='gelu')
        if out is None:
            return ops.conv2d_nhwc(g, pk['w2'], pk['b2'], kh=1, kw=1, residual=residual)
        ops.conv2d_nhwc(g, pk['w2'], pk['b2'], kh=1, kw=1, residual=residual, out=out.t, cout=c2, y_coff=out.coff)
        return out.t

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('Mlp writes its own input gradient')
        x, u, g, pk = self.__dict__.pop('_ctx')
        dg = _linear_backward(self.fc2, g, dout, pk['w2_t'])
        return _linear_backward(self.fc1, x, ops.gelu_backward_(u, dg), pk['w1_t'])


class SwinTransformerLayer(_Packed):
    """x + attn(norm1(x)), then + mlp(norm2(.)) on 8x8 windows, shifted by shift_size (models/common.py:1267-1358), on the NHWC map.  Both
    residual sums ride the output passes of attn.proj and mlp.fc2; in backward they ride the two LayerNorm backward passes.  Stochastic depth
    (drop_path = 0.1 when num_heads > 10, :1273-1274) is the identity in eval and not implemented for training."""

    def __init__(self, c, num_heads, window_size=7, shift_size=0, mlp_ratio=4, qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        if num_heads > 10:
            drop_path = 0.1
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError('SwinTransformerLayer: nn.LayerNorm only')
        if shift_size not in (0, 4):
            raise NotImplementedError(f'SwinTransformerLayer: shift {shift_size} (0 or 4: window 8)')
        self.window_size, self.shift_size, self.mlp_ratio, self.drop_path_rate = window_size, shift_size, mlp_ratio, float(drop_path)
        self.norm1 = norm_layer(c)
        self.attn = WindowAttention(c, window_size=(window_size, window_size), num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop,
                                    proj_drop=drop)
        self.norm2 = norm_layer(c)
        self.mlp = Mlp(in_features=c, hidden_features=int(c * mlp_ratio), act_layer=act_layer, drop=drop)

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack_params(self):
        return [self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias]

    def _pack(self, dev):
        return tuple(_f32dev(p, dev) for p in self._pack_params())

    def _region_ids(self, H, W, dev):
        """The shift mask's region ids for an (H, W) map: (Wp, Hp), the reference's transposed frame (swin_region_ids)."""
        if not self.shift_size:
            return None
        key = (H, W, dev)
        cache = self.__dict__.setdefault('_ids', {})
        if key not in cache:
            cache[key] = swin_region_ids((W + 7) // 8 * 8, (H + 7) // 8 * 8, self.window_size, self.shift_size).to(dev)
        return cache[key]

    def forward(self, x, out=None):
        c = self.norm1.normalized_shape[0]
        if self.training and self.drop_path_rate > 0:
            raise NotImplementedError(f'SwinTransformerLayer with {self.attn.num_heads} heads trains with stochastic depth (drop_path = '
                                      f'{self.drop_path_rate}, num_heads > 10), which is not on the path; eval works')
        xt = _whole(x, c, 'SwinTransformerLayer')
        g1, b1, g2, b2 = self._packed(xt.device)
        B, H, W, _ = xt.shape
        n1 = ops.layernorm_act(xt, g1, b1, self.norm1.eps)
        x1 = self.attn(n1, self.shift_size, self._region_ids(H, W, xt.device), residual=xt)
        n2 = ops.layernorm_act(x1, g2, b2, self.norm2.eps)
        y = self.mlp(n2, residual=x1, out=out)
        if self.training:
            self.__dict__['_ctx'] = (xt, x1, g1, g2)
        return out if out is not None else Act(y, 0, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('SwinTransformerLayer writes its own input gradient')
        xt, x1, g1, g2 = self.__dict__.pop('_ctx')
        c = xt.shape[3]
        if dout.coff != 0 or dout.t.shape[3] != c:                # a channel slice (C3STR: half of cv3's data gradient): one copy
            d = torch.empty_like(xt)
            ops.resample_slice(dout.t, dout.coff, d, 0, c)
        else:
            d = dout.t
        dn2 = self.mlp.backward(d)
        (gw, gb), fin = _grad_targets(self.norm2.weight, self.norm2.bias)
        dx1 = ops.layernorm_backward(x1, g2, self.norm2.eps, dn2, gw, gb, add=d)
        fin()
        dn1 = self.attn.backward(dx1)
        (gw, gb), fin = _grad_targets(self.norm1.weight, self.norm1.bias)
        dx = ops.layernorm_backward(xt, g1, self.norm1.eps, dn1, gw, gb, add=dx1)
        fin()
        return Act(dx, 0, c)


class SwinTransformerBlock(nn.Module):
    """num_layers SwinTransformerLayers, shift 0 for even and window_size // 2 for odd ones (models/common.py:1361-1378)."""

    def __init__(self, c1, c2, num_heads, num_layers, window_size=8):
        super().__init__()
        self.conv = None
        if c1 != c2:
            self.conv = Conv(c1, c2)
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.tr = nn.Sequential(*(SwinTransformerLayer(c2, num_heads=num_heads, window_size=window_size,
                                                       shift_size=0 if (i % 2 == 0) else self.shift_size) for i in range(num_layers)))

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x, out=None):
        """out: the Act (channel slice) the last layer writes."""
        if self.conv is not None:
            x = self.conv(x)
        n = len(self.tr)
        for i, layer in enumerate(self.tr):
            x = layer(x, out=out if i == n - 1 else None)
        return x

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('SwinTransformerBlock writes its own input gradient')
        for layer in reversed(self.tr):
            dout = layer.backward(dout)
        return dout if self.conv is None else self.conv.backward(dout, need_dx=need_dx)


class C3STR(C3):
    """C3 whose bottlenecks are one SwinTransformerBlock(c_, c_, c_ // 32, n) (models/common.py:1632-1637).  The last Swin layer's fc2 and cv2
    write the two halves of cv3's input."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        if c_ % 32 or c_ == 0:
            raise NotImplementedError(f'C3STR with hidden width {c_}: the window attention kernels need head_dim 32, i.e. c_ a multiple of 32')
        self.m = SwinTransformerBlock(c_, c_, c_ // 32, n)

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x):
        c_ = self.cv1.conv.out_channels
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 2 * c_)
        self.m(self.cv1(x), out=cat.slice(0, c_))
        self.cv2(x, out=cat.slice(c_, c_))
        return self.cv3(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('C3STR writes its own input gradient')
        c_ = self.cv1.conv.out_channels
        dcat = self.cv3.backward(dout)
        dx = self.cv2.backward(dcat.slice(c_, c_), need_dx=need_dx)
        d = self.m.backward(dcat.slice(0, c_))
        self.cv1.backward(d, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


# ------------------------------------------------------------------------------------------------ ConvNeXt / ConvMixer blocks (dwlk.hip)
def _whole4(a, c, what):
    """The tensor of an Act that is a whole (B,H,W,c) tensor with c % 4 == 0 - what the large-kernel depthwise blocks read."""
    if a.coff != 0 or a.c != c or a.t.shape[3] != c or c % 4:
        raise NotImplementedError(f'{what} takes a whole (B,H,W,{c}) tensor with c % 4 == 0, got channels [{a.coff}, {a.coff + a.c}) of '
                                  f'{a.t.shape[3]}')
    return a.t


def _out_slice(out, like, c):
    """(tensor, channel offset) a block writes: the given Act, else a new (B,H,W,c) tensor."""
    return (torch.empty(*like.shape[:3], c, device=like.device, dtype=torch.float32), 0) if out is None else (out.t, out.coff)


class LayerNorm_s(nn.Module):
    """LayerNorm over the channels of an NHWC map with a free eps (models/common.py:6728-6748), channels_last form only - the form
    ConvNextBlock uses; channels_first is refused.  On a whole (B,H,W,C) tensor."""

    def __init__(self, normalized_shape, eps=1e-6, data_format='channels_last'):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        if data_format == 'channels_first':
            raise NotImplementedError('LayerNorm_s(data_format="channels_first") is not on the path (nothing here uses it): channels_last only')
        if data_format != 'channels_last':
            raise NotImplementedError
        self.normalized_shape = (normalized_shape,)

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x):
        c = self.normalized_shape[0]
        xt = _whole(x, c, 'LayerNorm_s')
        w, b = _f32dev(self.weight, xt.device), _f32dev(self.bias, xt.device)
        if self.training:
            self.__dict__['_ctx'] = (xt, w)
        return Act(ops.layernorm_act(xt, w, b, self.eps), 0, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('LayerNorm_s writes its own input gradient')
        xt, w = self.__dict__.pop('_ctx')
        c = xt.shape[3]
        (gw, gb), fin = _grad_targets(self.weight, self.bias)
        dx = ops.layernorm_backward(xt, w, self.eps, _whole(dout, c, 'LayerNorm_s.backward'), gw, gb)
        fin()
        return Act(dx, 0, c) if need_dx else None


class ConvNextBlock(_Packed):
    """x + gamma * pwconv2(GELU(pwconv1(LayerNorm(dwconv7x7(x))))) (models/common.py:6751-6777), on the NHWC map the reference permutes to.
    The 7x7 depthwise conv is ops.dwlk; the Linear layers are 1x1 convolutions as in Mlp.  Eval: four launches - GELU rides pwconv1's
    epilogue, gamma and the shortcut pwconv2's (post_scale / residual).  Training keeps pwconv1's output for the GELU backward and pwconv2's
    for dgamma, and scales + adds in a pass of its own; backward: one reduce + apply pair gives dgamma (a per-channel sum of dout * pwconv2's
    output) and gamma * dout, the shortcut's gradient rides the depthwise data-gradient pass.  gamma is a bare Parameter: like the reference's,
    it is in none of the optimizer's groups (train.py:125-133) - it takes a gradient and no step moves it."""

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6):
        super().__init__()
        if drop_path > 0.:
            raise NotImplementedError(f'ConvNextBlock(drop_path={drop_path}): stochastic depth is not on the path (drop_path = 0 only)')
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm_s(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones((dim)), requires_grad=True) if layer_scale_init_value > 0 else None
        self.drop_path = nn.Identity()

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack(self, dev):
        c = self.dwconv.in_channels
        pk = dict(dw=pack_gconv_weight(self.dwconv.weight.detach().float()).to(dev), db=_f32dev(self.dwconv.bias, dev),
                  lw=_f32dev(self.norm.weight, dev), lb=_f32dev(self.norm.bias, dev), w1=_f32dev(self.pwconv1.weight, dev),
                  b1=_f32dev(self.pwconv1.bias, dev), w2=_f32dev(self.pwconv2.weight, dev), b2=_f32dev(self.pwconv2.bias, dev),
                  gamma=None if self.gamma is None else _f32dev(self.gamma, dev), zero_c=torch.zeros(c, device=dev))
        if self.training:
            pk.update(w1_t=_f32dev(self.pwconv1.weight.t(), dev), w2_t=_f32dev(self.pwconv2.weight.t(), dev), one=torch.ones(4 * c, device=dev),
                      zero=torch.zeros(4 * c, device=dev), one_c=torch.ones(c, device=dev))
        return pk

    def forward(self, x, out=None):
        """out: the Act (channel slice) the block writes (CNeB: the first half of cv3's input)."""
        c = self.dwconv.in_channels
        xt = _whole4(x, c, 'ConvNextBlock')
        pk = self._packed(xt.device)
        yt, y_coff = _out_slice(out, xt, c)
        u = ops.dwlk(xt, pk['dw'], pk['db'], c=c, k=7)
        n = ops.layernorm_act(u, pk['lw'], pk['lb'], self.norm.eps)
        if not self.training:
            g = ops.conv2d_nhwc(n, pk['w1'], pk['b1'], kh=1, kw=1, act='gelu')
            ops.conv2d_nhwc(g, pk['w2'], pk['b2'], kh=1, kw=1, post_scale=pk['gamma'], post_shift=None if pk['gamma'] is None else pk['zero_c'],
                            residual=xt, out=yt, cout=c, y_coff=y_coff)
            return Act(yt, y_coff, c)
        h = ops.conv2d_nhwc(n, pk['w1'], pk['b1'], kh=1, kw=1)
        g = ops.chan_affine_act(h, 4 * c, 0, pk['one'], pk['zero'], 'gelu', 0, torch.empty_like(h))
        if pk['gamma'] is None:
            v = None
            ops.conv2d_nhwc(g, pk['w2'], pk['b2'], kh=1, kw=1, residual=xt, out=yt, cout=c, y_coff=y_coff)
        else:
            v = ops.conv2d_nhwc(g, pk['w2'], pk['b2'], kh=1, kw=1)
            ops.chan_affine_act(v, c, 0, pk['gamma'], pk['zero_c'], 'none', 0, yt, y_coff, residual=xt)
        self.__dict__['_ctx'] = (xt, u, n, h, g, v, pk)
        return Act(yt, y_coff, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        xt, u, n, h, g, v, pk = self.__dict__.pop('_ctx')
        c = xt.shape[3]
        if v is not None:
            # the layer scale as a frozen per-channel affine map of v (mean 0, rstd 1, scale gamma): its backward's reduce half is
            # dgamma = sum dout * v, its apply half dv = gamma * dout - which also makes a whole tensor of a channel slice
            (gg,), fin = _grad_targets(self.gamma)
            dv = ops.bn_act_backward(dout.t, dout.coff, v, 0, c, pk['zero_c'], pk['one_c'], pk['gamma'], pk['zero_c'], 'none', 0, False,
                                     torch.empty_like(v), 0, gg, torch.zeros(c, device=v.device))
            fin()
        elif dout.coff != 0 or dout.t.shape[3] != c:
            dv = torch.empty_like(xt)
            ops.resample_slice(dout.t, dout.coff, dv, 0, c)
        else:
            dv = dout.t
        dg = _linear_backward(self.pwconv2, g, dv, pk['w2_t'])
        dn = _linear_backward(self.pwconv1, n, ops.gelu_backward_(h, dg), pk['w1_t'])
        (gw, gb), fin = _grad_targets(self.norm.weight, self.norm.bias)
        du = ops.layernorm_backward(u, pk['lw'], self.norm.eps, dn, gw, gb)
        fin()
        (gw, gb), fin = _grad_targets(self.dwconv.weight, self.dwconv.bias)
        ops.dwlk_wgrad(xt, du, c=c, k=7, dw=gw, db=gb, accumulate=True)
        fin()
        if not need_dx:
            return None
        dxt, dx_coff = _out_slice(dx_out, xt, c)
        ops.dwlk_dgrad(du, pk['dw'], c=c, k=7, out=dxt, dx_coff=dx_coff, accumulate=dout.t, acc_coff=dout.coff,      # + the shortcut's gradient
                       accumulate2=dxt if accumulate else None, acc2_coff=dx_coff)
        return Act(dxt, dx_coff, c)


class _CSPLargeKernel(nn.Module):
    """What CNeB and CSPCM share: cv3(cat(m(cv1(x)), cv2(x))), the block branch FIRST (models/common.py:6790-6791, 7179-7180), C3's layout:
    the last block of m and cv2 write the two halves of cv3's input buffer."""
    accumulates, folds_pooled, reduction = False, False, 1

    def _build(self, c1, c2, e, blocks):
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*blocks(c_))

    def forward(self, x):
        c_ = self.cv1.conv.out_channels
        if c_ % 4:
            raise NotImplementedError(f'{type(self).__name__} hidden width {c_} must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 2 * c_)
        n = len(self.m)
        t = self.cv1(x)
        for i, blk in enumerate(self.m):
            t = blk(t, out=cat.slice(0, c_) if i == n - 1 else None)
        self.cv2(x, out=cat.slice(c_, c_))
        return self.cv3(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        c_ = self.cv1.conv.out_channels
        dcat = self.cv3.backward(dout)
        dx = self.cv2.backward(dcat.slice(c_, c_), dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)
        d = dcat.slice(0, c_)
        for blk in reversed(self.m):
            d = blk.backward(d)
        self.cv1.backward(d, dx_out=dx, accumulate=True, need_dx=need_dx)
        return dx


class CNeB(_CSPLargeKernel):
    """The ConvNeXt C3 (models/common.py:6780-6791): C3 whose bottlenecks are n ConvNextBlock(c_).  shortcut and g are ignored there too."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        self._build(c1, c2, e, lambda c_: (ConvNextBlock(c_) for _ in range(n)))


def _act_bn_train(u, bn, act, yt, y_coff, residual=None, partials=None, vec=None):
    """yt's slice at y_coff = BN_batch(act(u)) [+ residual], the activation IN FRONT of the norm; u a whole tensor.  partials: the sums of
    act(u) the producing launch left (around vec['rm']); else the statistics pass reads u.  Under sync-BN, whose statistics entries take no
    activation, act(u) is materialised first.  -> the saved statistics."""
    c = u.shape[3]
    if ops.SYNC_BN is None:
        st, commit = _bn_train(bn, c, None if partials is not None else u, act=act, partials=partials, npix=ops._npix(u), vec=vec)
        ops.chan_affine_act(u, c, 0, st[2], st[3], act, 1, yt, y_coff, residual=residual)
    else:
        g = ops.chan_affine_act(u, c, 0, torch.ones(c, device=u.device), torch.zeros(c, device=u.device), act, 0, torch.empty_like(u))
        st, commit = _bn_train(bn, c, g, vec=vec)
        ops.chan_affine_act(g, c, 0, st[2], st[3], 'none', 0, yt, y_coff, residual=residual)
    commit()
    return st


class ConvMix(_Packed):
    """ConvMixer layer (models/common.py:7149-7166): x = x + BN(GELU(dwconv_k(x))), then BN(GELU(conv1x1(x))) - both BatchNorms BEHIND their
    activation.  dim1 is ignored, as in the reference: the module returns dim channels.  k = 9 (the default) or 7, ops.dwlk.
    Eval: two launches - the stencil with bias, GELU, the folded BatchNorm as post-affine and the residual; the 1x1 with bias, GELU and
    post-affine.  Training: the stencil's epilogue leaves the BatchNorm's partial sums (of GELU(conv + bias)) and writes the pre-activation,
    which the GELU backward needs; under sync-BN the activated tensor is materialised instead."""

    def __init__(self, dim, dim1, kernel_size=9):
        super().__init__()
        if kernel_size not in (7, 9):
            raise NotImplementedError(f'ConvMix(kernel_size={kernel_size}): the large-kernel depthwise kernels have k = 7 and k = 9 only')
        self.Resnet = nn.Sequential(nn.Conv2d(dim, dim, kernel_size=kernel_size, groups=dim, padding='same'), nn.GELU(), nn.BatchNorm2d(dim))
        self.Conv_1x1 = nn.Sequential(nn.Conv2d(dim, dim, kernel_size=1), nn.GELU(), nn.BatchNorm2d(dim))

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack(self, dev):
        dwc, pwc = self.Resnet[0], self.Conv_1x1[0]
        pk = dict(dw=pack_gconv_weight(dwc.weight.detach().float()).to(dev), db=_f32dev(dwc.bias, dev), pw=_f32dev(pwc.weight.flatten(1), dev),
                  pb=_f32dev(pwc.bias, dev))
        if self.training:
            pk['pwt'] = pack_dgrad_weight(pwc.weight.detach().float()).to(dev)
        else:
            pk['bn1'] = tuple(_f32dev(t, dev) for t in bn_fold(self.Resnet[2]))
            pk['bn2'] = tuple(_f32dev(t, dev) for t in bn_fold(self.Conv_1x1[2]))
        return pk

    def forward(self, x, out=None):
        """out: the Act (channel slice) the block writes (CSPCM: the first half of cv3's input)."""
        c, k = self.Resnet[0].in_channels, self.Resnet[0].kernel_size[0]
        xt = _whole4(x, c, 'ConvMix')
        pk = self._packed(xt.device)
        yt, y_coff = _out_slice(out, xt, c)
        if not self.training:
            y1 = ops.dwlk(xt, pk['dw'], pk['db'], c=c, k=k, act='gelu', post_scale=pk['bn1'][0], post_shift=pk['bn1'][1], residual=xt)
            ops.conv2d_nhwc(y1, pk['pw'], pk['pb'], kh=1, kw=1, act='gelu', post_scale=pk['bn2'][0], post_shift=pk['bn2'][1], out=yt, cout=c,
                            y_coff=y_coff)
            return Act(yt, y_coff, c)
        bn1, bn2 = self.Resnet[2], self.Conv_1x1[2]
        y1 = torch.empty_like(xt)
        if ops.SYNC_BN is None:
            vec = _bn_vectors(bn1, xt.device, c)
            part = {'pivot': vec['rm']}
            u1 = ops.dwlk(xt, pk['dw'], pk['db'], c=c, k=k, act='gelu', bn_stats=part)
            s1 = _act_bn_train(u1, bn1, 'gelu', y1, 0, residual=xt, partials=part, vec=vec)
        else:
            u1 = ops.dwlk(xt, pk['dw'], pk['db'], c=c, k=k)
            s1 = _act_bn_train(u1, bn1, 'gelu', y1, 0, residual=xt)
        u2 = ops.conv2d_nhwc(y1, pk['pw'], pk['pb'], kh=1, kw=1)
        s2 = _act_bn_train(u2, bn2, 'gelu', yt, y_coff)
        self.__dict__['_ctx'] = (xt, u1, s1, y1, u2, s2, pk)
        return Act(yt, y_coff, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        xt, u1, s1, y1, u2, s2, pk = self.__dict__.pop('_ctx')
        c, k = xt.shape[3], self.Resnet[0].kernel_size[0]
        du2 = _bn_backward(self.Conv_1x1[2], dout.t, dout.coff, u2, s2, 'gelu', torch.empty_like(u2), c, order=1)
        dy1 = _plain_conv_backward(self.Conv_1x1[0], Act(y1), du2, pk['pwt'], direct=('bias',)).t
        du1 = _bn_backward(self.Resnet[2], dy1, 0, u1, s1, 'gelu', torch.empty_like(u1), c, order=1)
        (gw, gb), fin = _grad_targets(self.Resnet[0].weight, self.Resnet[0].bias)
        ops.dwlk_wgrad(xt, du1, c=c, k=k, dw=gw, db=gb, accumulate=True)
        fin()
        if not need_dx:
            return None
        dxt, dx_coff = _out_slice(dx_out, xt, c)
        ops.dwlk_dgrad(du1, pk['dw'], c=c, k=k, out=dxt, dx_coff=dx_coff, accumulate=dy1,                           # + the residual branch
                       accumulate2=dxt if accumulate else None, acc2_coff=dx_coff)
        return Act(dxt, dx_coff, c)


class CSPCM(_CSPLargeKernel):
    """The ConvMixer C3 (models/common.py:7169-7180): n ConvMix(c_, c_) (k = 9) between cv1 and the concatenation, the block branch first."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        self._build(c1, c2, e, lambda c_: (ConvMix(c_, c_) for _ in range(n)))


class _CoordGates(_Packed):
    """The coordinate attention both CoorAttention and CABottleneck carry (models/common.py:1425-1450, 4902-4922), on the children `conv1`, `bn1`,
    `conv_h`, `conv_w` of the class that mixes this in:  out = [res +] x1 * a_h[b,h,c] * a_w[b,w,c]  with
    a_h, a_w = sigmoid(conv_h / conv_w (h_swish(bn1(conv1(cat(mean over W, mean over H)))))).
    Two passes over x1 forward (ops.coordatt_means, ops.coordatt_apply) and two over (dout, x1) backward (ops.coordatt_backward_gates,
    ops.coordatt_backward_input).  The small tensors in between have B * (H + W) rows: conv1 runs on the means as a (B, H + W, 1, C) map, bn1
    through the one BatchNorm train path with h-swish as its activation (eval: folded into conv1, h-swish in the conv epilogue), and conv_h and
    conv_w as ONE 1x1 conv with their weights stacked, (B, H + W, 1, 2C): a_h is rows [0, H) of channels [0, C), a_w rows [H, H + W) of
    channels [C, 2C).  The other two quadrants are computed and never read; their gradient is zero."""

    def _init_gates(self, c1, c2, mip):
        self.conv1 = nn.Conv2d(c1, mip, kernel_size=1, stride=1, padding=0)
        self.bn1 = nn.BatchNorm2d(mip)
        self.conv_h = nn.Conv2d(mip, c2, kernel_size=1, stride=1, padding=0)
        self.conv_w = nn.Conv2d(mip, c2, kernel_size=1, stride=1, padding=0)

    def _pack_params(self):
        return [*self.conv1.parameters(), *self.bn1.parameters(), *self.conv_h.parameters(), *self.conv_w.parameters()]

    def _pack(self, dev):
        c, mip = self.conv_h.out_channels, self.conv1.out_channels
        mp = pad4(mip)
        wg = torch.cat([self.conv_h.weight, self.conv_w.weight]).detach().float()
        bg = torch.cat([self.conv_h.bias, self.conv_w.bias]).detach().float().to(dev)
        pk = dict(wg=pack_conv_weight(wg, cin_pad=mp).to(dev), bg=bg)
        if not self.training:                                    # bn1 folded into conv1 (utils/torch_utils.py:202-222)
            w1, b1 = _fold_conv_bn(self.conv1, self.bn1)
            pk['w1'], pk['b1'] = pack_conv_weight(w1, cin_pad=c, cout_pad=mp).to(dev), torch.zeros(mp, device=dev)
            pk['b1'][:mip] = b1.to(dev)
            return pk
        w1 = self.conv1.weight.detach().float()
        pk['w1'], pk['b1'] = pack_conv_weight(w1, cin_pad=c, cout_pad=mp).to(dev), torch.zeros(mp, device=dev)
        pk['b1'][:mip] = self.conv1.bias.detach().float().to(dev)
        pk['wt1'] = pack_dgrad_weight(w1, cin_pad=c, cout_pad=mp).to(dev)
        pk['wtg'] = pack_dgrad_weight(wg, cin_pad=mp, cout_pad=2 * c).to(dev)
        pk['one'], pk['zero'] = torch.ones(2 * c, device=dev), torch.zeros(2 * c, device=dev)
        pk.update(_bn_vectors(self.bn1, dev, mp))
        return pk

    def _gates_forward(self, x1, res, out):
        """x1: the attended map (Act, c % 4 == 0); res: the shortcut (Act) or None; out: the Act to write (a new one when None)."""
        c, mip = self.conv_h.out_channels, self.conv1.out_channels
        if x1.c != c or self.conv1.in_channels != c:
            raise RuntimeError(f'coordinate attention over {c} channels got a map of {x1.c} (conv1 reads {self.conv1.in_channels})')
        if c % 4 or x1.up:
            raise NotImplementedError('coordinate attention needs a real tensor with a channel count that is a multiple of 4')
        if not x1.t.is_cuda:
            raise RuntimeError('somi_amd coordinate attention runs on the MI355X only (no CPU fallback)')
        pk = self._packed(x1.t.device)
        B, H, W, _ = x1.shape
        mp = pad4(mip)
        pool = ops.coordatt_means(x1.t, c, x1.coff)
        if out is None:
            out = new_act(x1.t, H, W, c)
            if out.t.shape[3] != c:
                out.t.zero_()                                     # pad channels of a tensor of its own
        conv = dict(kh=1, kw=1, stride=1, pad=0)
        if not self.training:
            t = ops.conv2d_nhwc(pool, pk['w1'], pk['b1'], act='hswish', cin=c, cout=mp, alg_cout=mip, **conv)
            g = ops.conv2d_nhwc(t, pk['wg'], pk['bg'], act='sigmoid', cin=mp, cout=2 * c, alg_cin=mip, **conv)
        else:
            y1 = ops.conv2d_nhwc(pool, pk['w1'], pk['b1'], act='none', cin=c, cout=mp, alg_cout=mip, **conv)
            st, commit = _bn_train(self.bn1, mp, y1, vec=pk)
            commit()
            t = ops.chan_affine_act(y1, mp, 0, st[2], st[3], 'hswish', 0, torch.empty_like(y1))
            pre = ops.conv2d_nhwc(t, pk['wg'], pk['bg'], act='none', cin=mp, cout=2 * c, alg_cin=mip, **conv)
            g = ops.chan_affine_act(pre, 2 * c, 0, pk['one'], pk['zero'], 'sigmoid', 0, torch.empty_like(pre))
            self.__dict__['_gctx'] = (x1, pool, y1, st, t, pre, g, pk)
        ops.coordatt_apply(x1.t, (g, 0, 0), (g, c, H), c, x1.coff, res=None if res is None else res.t, res_coff=0 if res is None else res.coff,
                           out=out.t, o_coff=out.coff)
        return Act(out.t, out.coff, c)

    def _gates_backward(self, dout, dx_out=None, accumulate=False):
        """dout: the gradient of the product x1 * a_h * a_w (the shortcut's share is the caller's).  -> the gradient of x1 as an Act: a whole padded
        tensor of its own (pad channels zero) when dx_out is None, else written into dx_out, added to it with `accumulate`.  The parameter
        gradients of conv1, bn1, conv_h and conv_w are accumulated into .grad."""
        x1, pool, y1, st, t, pre, g, pk = self.__dict__.pop('_gctx')
        c, mip = self.conv_h.out_channels, self.conv1.out_channels
        mp = pad4(mip)
        B, H, W, _ = x1.shape
        dev = x1.t.device
        conv = dict(kh=1, kw=1, stride=1, pad=0)
        a_h, a_w = (g, 0, 0), (g, c, H)
        dg = torch.zeros_like(g)                                  # the two quadrants nobody reads keep a zero gradient
        ops.coordatt_backward_gates(dout.t, x1.t, a_h, a_w, c, dout.coff, x1.coff, da_h=(dg, 0, 0), da_w=(dg, c, H))
        # through the sigmoid: a BatchNorm-activation backward with frozen unit statistics; its dbeta is the stacked bias gradient
        dbg = torch.zeros(2 * c, device=dev)
        ops.bn_act_backward(dg, 0, pre, 0, 2 * c, pk['zero'], pk['one'], pk['one'], pk['zero'], 'sigmoid', 0, False, dg, 0, None, dbg)
        _acc_grad(self.conv_h.bias, dbg[:c])
        _acc_grad(self.conv_w.bias, dbg[c:])
        dwg = ops.conv2d_wgrad_nhwc(t, dg, cin=mp, cout=2 * c, **conv).view(2 * c, mp)[:, :mip]
        _acc_grad(self.conv_h.weight, dwg[:c].reshape(c, mip, 1, 1))
        _acc_grad(self.conv_w.weight, dwg[c:].reshape(c, mip, 1, 1))
        dt = ops.conv2d_dgrad_nhwc(dg, pk['wtg'], B=B, H=H + W, W=1, cin=mp, cout=2 * c, **conv)
        dy1 = _bn_backward(self.bn1, dt, 0, y1, st, 'hswish', torch.empty_like(y1), mp)
        db1 = torch.zeros(mp, device=dev)
        ops.chan_sum_(dy1, mp, 0, db1)
        _acc_grad(self.conv1.bias, db1[:mip])
        dw1 = ops.conv2d_wgrad_nhwc(pool, dy1, cin=c, cout=mp, **conv).view(mp, c)[:mip]
        _acc_grad(self.conv1.weight, dw1.reshape(mip, c, 1, 1))
        dpool = ops.conv2d_dgrad_nhwc(dy1, pk['wt1'], B=B, H=H + W, W=1, cin=c, cout=mp, **conv)
        if dx_out is None:
            dx_out = new_act(x1.t, H, W, c)
            if dx_out.t.shape[3] != c:
                dx_out.t.zero_()
            accumulate = False
        ops.coordatt_backward_input(dout.t, a_h, a_w, (dpool, 0, 0), (dpool, 0, H), c, dout.coff, out=dx_out.t, dx_coff=dx_out.coff,
                                    accumulate=accumulate)
        return dx_out


class CoorAttention(_CoordGates):
    """Coordinate attention as a layer of its own (models/common.py:1399-1450): out = x * a_w * a_h, every pixel gated by its row and by its column."""

    def __init__(self, inp, oup, reduction=32):
        super().__init__()
        if inp != oup:
            raise NotImplementedError(f'CoorAttention({inp}, {oup}): the gates have oup channels and multiply the inp-channel input; the '
                                      f'reference\'s product does not broadcast either unless inp == oup')
        self._init_gates(inp, oup, max(8, inp // reduction))

    accumulates, folds_pooled, reduction = False, False, 1       # like Bottleneck: takes dx_out / accumulate, not walked that way

    def forward(self, x, out=None):
        return self._gates_forward(x, None, out)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        return self._gates_backward(dout, dx_out, accumulate)


class CABottleneck(_CoordGates):
    """cv1 (1x1) -> cv2 (3x3) -> coordinate attention (+x) (models/common.py:4884-4922); the shortcut rides the attention's apply pass (forward)
    and cv1's dgrad epilogue (backward).  mip comes from c1, as in the reference."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, ratio=32):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2
        self._init_gates(c1, c2, max(8, c1 // ratio))             # conv1 reads cv2's c2-channel output with c1 inputs: c1 == c2, or forward raises

    accumulates, folds_pooled, reduction = False, False, 1       # like Bottleneck: takes dx_out / accumulate, not walked that way

    def forward(self, x, out=None):
        return self._gates_forward(self.cv2(self.cv1(x)), x if self.add else None, out)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.cv2.backward(self._gates_backward(dout))
        c1 = self.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0
        dx = self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if self.add and not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class C3_CA(C3):
    """C3 whose bottlenecks are CABottleneck(c_, c_, shortcut, g, e=1.0) (models/common.py:4925-4931).  The reference's parser does not repeat
    it inside (models/yolo.py:1487-1490): a yaml row with n > 1 is a Repeat of n C3_CA blocks with one bottleneck each."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(CABottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))

    accumulates, folds_pooled, reduction = False, False, 1       # C3's backward, dx_out / accumulate included; the walk adds its gradient itself


class EMA(_Packed):
    """Efficient multi-scale attention (models/common.py:5263-5292) on the children `gn`, `conv1x1`, `conv3x3`: the map, seen as `factor`
    groups of cg = channels / factor channels that share every weight, is gated per (image, group, pixel) by
    sigmoid(softmax(mean x1) . x2 + softmax(mean x2) . x1), x1 = gn(x * sigmoid(hw_h) * sigmoid(hw_w)), hw = conv1x1(cat(mean over W, mean
    over H)), x2 = conv3x3(x).  nn.GroupNorm(cg, cg) on the (B * factor, cg, H, W) view is a norm per (image, channel).
    Forward: ops.coordatt_means, conv1x1 with its sigmoid as ONE 1x1 conv over the (B, H + W, factor, cg) view of the means, conv3x3, then
    ops.ema_stats and ops.ema_gate; x1, the expanded gates and the weight map never reach memory.  Backward: ops.ema_backward_gate and
    ops.ema_backward_norm, the conv backward of conv3x3 (its data gradient added into dx) and conv1x1, and ops.coordatt_backward_input, which
    adds dt * gates and the means' broadcast.  conv3x3 runs on the dense implicit-GEMM kernels, one launch per group slice with the one shared
    weight set, the weight gradient chained through `accumulate` (the grouped kernels with replicated weights measured 2.5 to 6.5 times slower
    per block)."""

    def __init__(self, channels, factor=8):
        super().__init__()
        self.groups = factor
        assert channels // self.groups > 0
        cg = channels // self.groups
        self.gn = nn.GroupNorm(cg, cg)
        self.conv1x1 = nn.Conv2d(cg, cg, kernel_size=1, stride=1, padding=0)
        self.conv3x3 = nn.Conv2d(cg, cg, kernel_size=3, stride=1, padding=1)

    accumulates, folds_pooled, reduction = False, False, 1       # takes dx_out / accumulate, not walked that way

    def _pack(self, dev):
        w1, w3 = self.conv1x1.weight.detach().float(), self.conv3x3.weight.detach().float()
        pk = dict(w1=pack_conv_weight(w1).to(dev), b1=_f32dev(self.conv1x1.bias, dev), w3=pack_conv_weight(w3).to(dev),
                  b3=_f32dev(self.conv3x3.bias, dev), gamma=_f32dev(self.gn.weight, dev), beta=_f32dev(self.gn.bias, dev))
        if self.training:
            pk['wt1'], pk['wt3'] = pack_dgrad_weight(w1).to(dev), pack_dgrad_weight(w3).to(dev)
        return pk

    def _check(self, x):
        c, g = self.groups * self.conv3x3.in_channels, self.groups
        cg = self.conv3x3.in_channels
        if x.c != c or x.c % g:
            raise NotImplementedError(f'EMA over {g} groups of {cg} channels got a map of {x.c}: the reference\'s reshape to (B * {g}, {cg}, H, W) '
                                      f'needs channels % factor == 0 and the width it was built for (models/common.py:5280)')
        if cg % 4 or cg > 64 or x.up:
            raise NotImplementedError(f'EMA with {cg} channels per group is not on the SOMI path (a multiple of 4, at most 64, a real tensor)')
        if not x.t.is_cuda:
            raise RuntimeError('somi_amd EMA runs on the MI355X only (no CPU fallback)')
        return c, g, cg

    def forward(self, x, out=None, residual=None):
        """x: the attended map (Act); out: the Act to write (a new one when None); residual: an Act added to the result in the gate pass."""
        c, g, cg = self._check(x)
        pk = self._packed(x.t.device)
        B, H, W, _ = x.shape
        pool = ops.coordatt_means(x.t, c, x.coff)
        sg = ops.conv2d_nhwc(pool.view(B, H + W, g, cg), pk['w1'], pk['b1'], kh=1, kw=1, act='sigmoid', cin=cg, cout=cg).view(B, H + W, c)
        x2 = torch.empty(B, H, W, c, device=x.t.device, dtype=torch.float32)
        for gi in range(g):
            ops.conv2d_nhwc(x.t, pk['w3'], pk['b3'], kh=3, kw=3, pad=1, cin=cg, x_coff=x.coff + gi * cg, out=x2, cout=cg, y_coff=gi * cg)
        _, vec = ops.ema_stats(x.t, sg, c, g, pk['gamma'], pk['beta'], self.gn.eps, x.coff, x2=x2)
        if out is None:
            out = new_act(x.t, H, W, c)
            if out.t.shape[3] != c:
                out.t.zero_()                                     # pad channels of a tensor of its own
        ops.ema_gate(x.t, x2, sg, vec, c, g, pk['gamma'], pk['beta'], x.coff, res=None if residual is None else residual.t,
                     res_coff=0 if residual is None else residual.coff, out=out.t, o_coff=out.coff)
        if self.training:
            self.__dict__['_ctx'] = (x, pool, sg, x2, vec, pk)
        return Act(out.t, out.coff, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """dout: the gradient of x * sigmoid(wgt) (a residual's share is the caller's).  -> the gradient of x as an Act: a whole padded tensor of
        its own (pad channels zero) when dx_out is None, else written into dx_out, added to it with `accumulate`.  Parameter gradients into .grad."""
        x, pool, sg, x2, vec, pk = self.__dict__.pop('_ctx')
        g, cg = self.groups, self.conv3x3.in_channels
        c = g * cg
        B, H, W, _ = x.shape
        dev = x.t.device
        if dx_out is None:
            dx_out = new_act(x.t, H, W, c)
            if dx_out.t.shape[3] != c:
                dx_out.t.zero_()
            accumulate = False
        (dgam, dbet), fin = _grad_targets(self.gn.weight, self.gn.bias)
        _, dw, _, bvec = ops.ema_backward_gate(dout.t, x.t, x2, sg, vec, c, g, pk['gamma'], pk['beta'], dgam, dbet, dout.coff, x.coff,
                                               dx=dx_out.t, dx_coff=dx_out.coff, accumulate=accumulate)
        fin()
        dt, dx2, dsg = ops.ema_backward_norm(x.t, sg, dw, vec, bvec, c, g, pk['gamma'], pk['beta'], x.coff)
        # conv3x3: bias, weight (summed over the groups that share it), data gradient added into dx
        db3 = torch.zeros(c, device=dev)
        ops.chan_sum_(dx2, c, 0, db3)
        _acc_grad(self.conv3x3.bias, db3.view(g, cg).sum(0))
        dw3 = torch.empty(cg, 9 * cg, device=dev, dtype=torch.float32)
        for gi in range(g):
            ops.conv2d_wgrad_nhwc(x.t, dx2, kh=3, kw=3, pad=1, cin=cg, x_coff=x.coff + gi * cg, cout=cg, dy_coff=gi * cg, out=dw3,
                                  accumulate=dw3 if gi else None)
            ops.conv2d_dgrad_nhwc(dx2, pk['wt3'], B=B, H=H, W=W, cin=cg, kh=3, kw=3, pad=1, cout=cg, dy_coff=gi * cg, out=dx_out.t,
                                  dx_coff=dx_out.coff + gi * cg, accumulate=dx_out.t, acc_coff=dx_out.coff + gi * cg)
        _acc_grad(self.conv3x3.weight, dw3.view(cg, 3, 3, cg).permute(0, 3, 1, 2))
        # conv1x1 on the (B, H + W, g, cg) view; dsg is the gradient in front of its sigmoid
        dsv, plv = dsg.view(B, H + W, g, cg), pool.view(B, H + W, g, cg)
        db1 = torch.zeros(cg, device=dev)
        ops.chan_sum_(dsv, cg, 0, db1)
        _acc_grad(self.conv1x1.bias, db1)
        dw1 = ops.conv2d_wgrad_nhwc(plv, dsv, kh=1, kw=1, cin=cg, cout=cg)
        _acc_grad(self.conv1x1.weight, dw1.view(cg, cg, 1, 1))
        dpool = ops.conv2d_dgrad_nhwc(dsv, pk['wt1'], B=B, H=H + W, W=g, cin=cg, kh=1, kw=1, cout=cg).view(B, H + W, c)
        ops.coordatt_backward_input(dt, (sg, 0, 0), (sg, 0, H), (dpool, 0, 0), (dpool, 0, H), c, 0, out=dx_out.t, dx_coff=dx_out.coff,
                                    accumulate=True)
        return Act(dx_out.t, dx_out.coff, c)


class ACmix(_Packed):
    """Self-attention and convolution mixed (models/common.py:7281-7365) with the reference's constructor, parameter names and initial values:
    out = rate1 * att + rate2 * conv over q, k, v = conv1(x), conv2(x), conv3(x).  att: per head (4) and pixel a softmax attention over the 7x7
    window around it, reflection padding 3, scores s * q . (k_j + pe_p - pe_j) with pe = conv_p(position map), s = head_dim ** -0.5; conv:
    dep_conv(fc(.)), fc a 1x1 conv over the 12 (q, k, v) x head maps of every head dim, dep_conv a grouped 3x3 conv.
    Forward: the three projections as ONE 1x1 conv c1 -> 3 c2 on the dense kernels, ops.acmix_conv (fc and dep_conv folded into one grouped conv,
    the 9 x head_dim-channel fc output never exists) and ops.acmix_attn with the mix in its epilogue; the unfolded windows, the position map and
    the scores never reach memory.  Only differences of pe enter, so conv_p.bias cancels: its gradient is exactly zero.  Backward:
    ops.acmix_conv_backward_data writes the gradient of the stacked q, k, v, ops.acmix_attn_backward_q and _kv add theirs, then the plain conv
    backward of the stacked projection.  The reference's reset_parameters leaves dep_conv WITHOUT a bias (`self.dep_conv.bias =
    init_rate_0(...)` assigns the helper's None, models/common.py:7321), and so does this class; a bias given to dep_conv later is honoured.
    rate1 / rate2 are plain parameters: they take a gradient and the reference puts them in no optimizer group (train.py:125-133)."""

    def __init__(self, in_planes, out_planes, kernel_att=7, head=4, kernel_conv=3, stride=1, dilation=1):
        super().__init__()
        for name, got, want in (('kernel_att', kernel_att, 7), ('head', head, 4), ('kernel_conv', kernel_conv, 3), ('stride', stride, 1),
                                ('dilation', dilation, 1)):
            if got != want:
                raise NotImplementedError(f'ACmix({in_planes}, {out_planes}, {name}={got}): only {name}={want}, the reference\'s default, is on '
                                          f'the SOMI path')
        self.in_planes, self.out_planes, self.head, self.kernel_att, self.kernel_conv = in_planes, out_planes, head, kernel_att, kernel_conv
        self.stride, self.dilation = stride, dilation
        self.rate1 = nn.Parameter(torch.Tensor(1))
        self.rate2 = nn.Parameter(torch.Tensor(1))
        self.head_dim = out_planes // head
        self.conv1 = nn.Conv2d(in_planes, out_planes, kernel_size=1)
        self.conv2 = nn.Conv2d(in_planes, out_planes, kernel_size=1)
        self.conv3 = nn.Conv2d(in_planes, out_planes, kernel_size=1)
        self.conv_p = nn.Conv2d(2, self.head_dim, kernel_size=1)
        self.padding_att = (dilation * (kernel_att - 1) + 1) // 2
        self.fc = nn.Conv2d(3 * head, kernel_conv * kernel_conv, kernel_size=1, bias=False)
        self.dep_conv = nn.Conv2d(kernel_conv * kernel_conv * self.head_dim, out_planes, kernel_size=kernel_conv, bias=True,
                                  groups=self.head_dim, padding=1, stride=stride)
        self.reset_parameters()

    accumulates, folds_pooled, reduction = False, False, 1       # takes dx_out / accumulate, not walked that way

    def reset_parameters(self):
        """models/common.py:7313-7321: rates 0.5, dep_conv.weight the shift kernel (tap i of input i), dep_conv.bias removed."""
        self.rate1.data.fill_(0.5)
        self.rate2.data.fill_(0.5)
        k = self.kernel_conv
        kernel = torch.zeros(k * k, k, k)
        for i in range(k * k):
            kernel[i, i // k, i % k] = 1.
        self.dep_conv.weight = nn.Parameter(kernel.repeat(self.out_planes, 1, 1, 1), requires_grad=True)
        self.dep_conv.bias = None

    def _pack(self, dev):
        c1, c2 = self.in_planes, self.out_planes
        w = torch.cat([m.weight.detach().float() for m in (self.conv1, self.conv2, self.conv3)], 0)
        bdep = self.dep_conv.bias
        pk = dict(w=pack_conv_weight(w).to(dev), b=torch.cat([_f32dev(m.bias, dev) for m in (self.conv1, self.conv2, self.conv3)]),
                  wp=_f32dev(self.conv_p.weight, dev).view(self.head_dim, 2), rate1=_f32dev(self.rate1, dev), rate2=_f32dev(self.rate2, dev),
                  fc=_f32dev(self.fc.weight, dev).view(9, 12), dep=_f32dev(self.dep_conv.weight, dev),
                  bdep=torch.zeros(c2, device=dev) if bdep is None else _f32dev(bdep, dev))
        pk['weff'] = ops.acmix_fold_weff(pk['fc'], pk['dep'], c2)
        if self.training:
            pk['wt'] = pack_dgrad_weight(w).to(dev)
        return pk

    def _check(self, x):
        c1, c2 = self.in_planes, self.out_planes
        if x.c != c1 or x.up:
            raise NotImplementedError(f'ACmix({c1}, {c2}) takes a real map of {c1} channels, got {x.c}')
        if c2 % 16 or c2 > 1024:
            raise NotImplementedError(f'ACmix with {c2} output channels is not on the SOMI path: 4 heads of a multiple of 4 channels '
                                      f'(out_planes % 16 == 0), at most 1024')
        B, H, W, _ = x.shape
        if H <= self.padding_att or W <= self.padding_att:        # nn.ReflectionPad2d(3), models/common.py:7302, 7343
            raise RuntimeError(f'Padding size should be less than the corresponding input dimension, but got: padding ({self.padding_att}, '
                               f'{self.padding_att}) at dimension {3 if W <= self.padding_att else 2} of input {[B * 4, c2 // 4, H, W]} '
                               f'(ACmix\'s ReflectionPad2d({self.padding_att}), models/common.py:7302)')
        if not x.t.is_cuda:
            raise RuntimeError('somi_amd ACmix runs on the MI355X only (no CPU fallback)')
        return c1, c2

    def forward(self, x, out=None):
        """x: the input map (Act); out: the Act to write (a new one when None)."""
        c1, c2 = self._check(x)
        pk = self._packed(x.t.device)
        B, H, W, _ = x.shape
        qkv = ops.conv2d_nhwc(x.t, pk['w'], pk['b'], kh=1, kw=1, cin=pad4(c1), x_coff=x.coff, cout=3 * c2)
        mix = ops.acmix_conv(qkv, c2, pk['weff'], pk['bdep'])
        if out is None:
            out = new_act(x.t, H, W, c2)
            if out.t.shape[3] != c2:
                out.t.zero_()                                     # pad channels of a tensor of its own
        _, lse = ops.acmix_attn(qkv, c2, pk['wp'], pk['rate1'], pk['rate2'], mix=mix, out=out.t, o_coff=out.coff, want_lse=self.training)
        if self.training:
            self.__dict__['_ctx'] = (x, qkv, mix, lse, pk)
        return Act(out.t, out.coff, c2)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """dout: the gradient of the output.  -> the gradient of x as an Act (None without need_dx): a padded tensor of its own when dx_out is
        None, else written into dx_out, added to it with `accumulate`.  Parameter gradients into .grad."""
        x, qkv, mix, lse, pk = self.__dict__.pop('_ctx')
        c1, c2, D = self.in_planes, self.out_planes, self.head_dim
        c1p = pad4(c1)
        B, H, W, _ = x.shape
        dev = x.t.device
        dqkv = torch.empty_like(qkv)
        ops.acmix_conv_backward_data(dout.t, c2, pk['weff'], pk['rate2'], dqkv, do_coff=dout.coff)
        _, aux, dwp, drates = ops.acmix_attn_backward_q(dout.t, qkv, c2, pk['wp'], pk['rate1'], pk['rate2'], lse, do_coff=dout.coff, mix=mix,
                                                        dq=dqkv, dq_coff=0, accumulate=True)
        ops.acmix_attn_backward_kv(dout.t, qkv, c2, pk['wp'], pk['rate1'], pk['rate2'], lse, aux, do_coff=dout.coff, dk=dqkv, dk_coff=c2,
                                   dv=dqkv, dv_coff=2 * c2, accumulate=True)
        dweff, dbdep = ops.acmix_conv_backward_weight(dout.t, qkv, c2, pk['rate2'], do_coff=dout.coff)
        dfc, ddep = ops.acmix_split_dweff(dweff, pk['fc'], pk['dep'], c2)
        _acc_grad(self.rate1, drates[0:1])
        _acc_grad(self.rate2, drates[1:2])
        _acc_grad(self.conv_p.weight, dwp.view(D, 2, 1, 1))
        _acc_grad(self.conv_p.bias, torch.zeros(D, device=dev))   # only differences of pe enter the scores
        _acc_grad(self.fc.weight, dfc.view(9, 12, 1, 1))
        _acc_grad(self.dep_conv.weight, ddep)
        if self.dep_conv.bias is not None:
            _acc_grad(self.dep_conv.bias, dbdep)
        # the stacked projection: a plain 1x1 conv c1 -> 3 c2 with bias
        dw = ops.conv2d_wgrad_nhwc(x.t, dqkv, kh=1, kw=1, cin=c1p, x_coff=x.coff, cout=3 * c2)
        db = torch.zeros(3 * c2, device=dev)
        ops.chan_sum_(dqkv, 3 * c2, 0, db)
        for i, m in enumerate((self.conv1, self.conv2, self.conv3)):
            _acc_grad(m.weight, dw[i * c2:(i + 1) * c2, :c1].reshape(c2, c1, 1, 1))
            _acc_grad(m.bias, db[i * c2:(i + 1) * c2])
        if not need_dx:
            return None
        if dx_out is None:
            dx_out = Act(torch.empty(B, H, W, c1p, device=dev, dtype=torch.float32), 0, c1)
            accumulate = False
        ops.conv2d_dgrad_nhwc(dqkv, pk['wt'], B=B, H=H, W=W, cin=c1p, kh=1, kw=1, cout=3 * c2, out=dx_out.t, dx_coff=dx_out.coff,
                              accumulate=dx_out.t if accumulate else None, acc_coff=dx_out.coff)
        return Act(dx_out.t, dx_out.coff, c1)


class _ConvNormAct(Conv):
    """The reference's ConvNormAct (models/common.py:5387-5406) at what iRMB_EMA builds of it: conv (no bias) -> BatchNorm -> activation, the
    children named `conv` and `norm`.  Runs as Conv does; `bn` is `norm` under Conv's name."""

    def __init__(self, dim, k, g, act):
        super().__init__(dim, dim, k, 1, g=g, act=act)
        self.norm = self._modules.pop('bn')
        self.norm.eps = 1e-6                                      # get_norm's eps, until initialize_weights sets 1e-3 / 0.03

    bn = property(lambda self: self.norm)
    accumulates, folds_pooled, reduction = False, False, 1


class _Proj(nn.Module):
    """ConvNormAct(dim, dim, 1, norm_layer='none', act_layer='none'): a 1x1 conv without bias, the child `conv`."""

    def __init__(self, dim):
        super().__init__()
        self.conv = nn.Conv2d(dim, dim, 1, 1, 0, bias=False)


class iRMB_EMA(_Packed):
    """Inverted residual mobile block with EMA as its attention (models/common.py:5409-5451), at the reference's defaults:
    out = x + proj(e + SiLU(BN(dw3x3(e)))), e = EMA(norm(x)), norm a BatchNorm without activation, proj a 1x1 conv without bias; the shortcut is
    the input BEFORE norm.  norm and conv_local.norm go through the one BatchNorm train path (eval: norm is a per-channel affine, conv_local's
    folds at pack time); the first residual rides the depthwise conv's output pass, the second proj's epilogue; in backward the first rides the
    depthwise data gradient, the second is one add behind the norm's backward."""

    def __init__(self, dim_in, norm_in=True, has_skip=True, exp_ratio=1.0, norm_layer='bn_2d', act_layer='relu', v_proj=True, dw_ks=3, stride=1,
                 dilation=1, se_ratio=0.0, attn_s=True, qkv_bias=False, drop=0., drop_path=0.):
        super().__init__()
        given = dict(norm_in=norm_in, has_skip=has_skip, exp_ratio=exp_ratio, norm_layer=norm_layer, dw_ks=dw_ks, stride=stride, dilation=dilation,
                     se_ratio=se_ratio, attn_s=attn_s, drop=drop, drop_path=drop_path)
        want = dict(norm_in=True, has_skip=True, exp_ratio=1.0, norm_layer='bn_2d', dw_ks=3, stride=1, dilation=1, se_ratio=0.0, attn_s=True,
                    drop=0., drop_path=0.)
        off = {k: v for k, v in given.items() if v != want[k]}
        if off:
            raise NotImplementedError(f'iRMB_EMA({dim_in}, {off}): only the reference\'s defaults are on the SOMI path '
                                      f'(models/common.py:5411-5413: {want})')
        self.norm = nn.BatchNorm2d(dim_in, eps=1e-6)             # get_norm's eps; initialize_weights sets 1e-3 / 0.03 on every BatchNorm2d
        self.ema = EMA(dim_in)
        self.conv_local = _ConvNormAct(dim_in, dw_ks, dim_in, nn.SiLU())
        self.proj = _Proj(dim_in)

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack_params(self):
        return [*self.norm.parameters(), *self.proj.parameters()]

    def _pack(self, dev):
        w = self.proj.conv.weight.detach().float()
        pk = dict(wp=pack_conv_weight(w).to(dev))
        if self.training:
            pk['wtp'] = pack_dgrad_weight(w).to(dev)
        else:
            pk['norm'] = tuple(_f32dev(t, dev) for t in bn_fold(self.norm))
        return pk

    def forward(self, x, out=None, residual=None):
        """residual: a further Act added to the result (the bottleneck's shortcut), by one add behind proj."""
        c = self.norm.num_features
        if x.c != c or c % 4 or pad4(c) != c or x.up:
            raise NotImplementedError(f'iRMB_EMA({c}) takes a real map of {c} channels (a multiple of 32), got {x.c}')
        if not x.t.is_cuda:
            raise RuntimeError('somi_amd iRMB_EMA runs on the MI355X only (no CPU fallback)')
        pk = self._packed(x.t.device)
        B, H, W, _ = x.shape
        xn = torch.empty(B, H, W, c, device=x.t.device, dtype=torch.float32)
        if self.training:
            st, commit = _bn_train(self.norm, c, x.t, coff=x.coff)
            commit()
            ops.chan_affine_act(x.t, c, x.coff, st[2], st[3], 'none', 0, xn)
        else:
            st = None
            ops.chan_affine_act(x.t, c, x.coff, pk['norm'][0], pk['norm'][1], 'none', 0, xn)
        e = self.ema(Act(xn, 0, c))
        t2 = self.conv_local(e, residual=e)
        if out is None:
            out = new_act(x.t, H, W, c)
        ops.conv2d_nhwc(t2.t, pk['wp'], None, kh=1, kw=1, cin=c, x_coff=t2.coff, out=out.t, cout=c, y_coff=out.coff, residual=x.t, res_coff=x.coff)
        if residual is not None:
            ops.add_(out.t, out.coff, residual.t, residual.coff, c)
        if self.training:
            self.__dict__['_ctx'] = (x, st, t2, pk)
        return Act(out.t, out.coff, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        x, st, t2, pk = self.__dict__.pop('_ctx')
        c = self.norm.num_features
        dt2 = _plain_conv_backward(self.proj.conv, t2, dout.t, pk['wtp'], dy_coff=dout.coff, direct=('weight',))
        de = self.conv_local.backward(dt2, also_add=dt2)         # e + conv_local(e): the residual's share rides the depthwise data gradient
        dxn = self.ema.backward(de)
        dxb = torch.empty_like(x.t)
        _bn_backward(self.norm, dxn.t, dxn.coff, x.t, st, 'none', dxb, c, coff=x.coff)
        if dx_out is None:
            ops.add_(dxb, x.coff, dout.t, dout.coff, c)
            return Act(dxb, x.coff, c)
        if accumulate:
            ops.add_(dx_out.t, dx_out.coff, dxb, x.coff, c)
            ops.add_(dx_out.t, dx_out.coff, dout.t, dout.coff, c)
        else:
            ops.add_(dxb, x.coff, dout.t, dout.coff, c, out=dx_out.t, out_coff=dx_out.coff)
        return Act(dx_out.t, dx_out.coff, c)


class iRMB_EMABottleneck(nn.Module):
    """cv1 -> cv2 -> iRMB_EMA (+x) (models/common.py:5454-5470); the shortcut is one add behind the block's proj (forward) and rides cv1's dgrad
    epilogue (backward)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2
        self.iRMB = iRMB_EMA(c2)

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x, out=None):
        return self.iRMB(self.cv2(self.cv1(x)), out=out, residual=x if self.add else None)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.cv2.backward(self.iRMB.backward(dout))
        c1 = self.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0
        dx = self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if self.add and not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class C2f_iRMB_EMA(C2f):
    """C2f whose blocks are iRMB_EMABottleneck(c, c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) (models/common.py:5473-5497); the branches are
    written into the concat buffer in place, as C2f's.  The reference's parser builds it from the yaml arguments as written
    (models/yolo.py:1648-1650)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(iRMB_EMABottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    accumulates, folds_pooled, reduction = False, False, 1       # C2f's backward, dx_out / accumulate included; the walk adds its gradient itself


class CPCA_ChannelAttention(_Packed):
    """t * (sigmoid(MLP(avgpool t)) + sigmoid(MLP(maxpool t))) (models/common.py:5753-5779): the shared MLP - two 1x1 convs with bias on a 1x1
    map, i.e. two small dense layers - runs once on the 2B rows (averages, then maxima) one pooling pass leaves; each half gets its own sigmoid
    before the sum (CBAM sums first)."""

    def __init__(self, input_channels, internal_neurons):
        super().__init__()
        self.fc1 = nn.Conv2d(in_channels=input_channels, out_channels=internal_neurons, kernel_size=1, stride=1, bias=True)
        self.fc2 = nn.Conv2d(in_channels=internal_neurons, out_channels=input_channels, kernel_size=1, stride=1, bias=True)
        self.input_channels = input_channels

    accumulates = folds_pooled = False
    reduction = 1

    def _pack(self, dev):
        return tuple(t.detach().float().contiguous().to(dev) for t in (self.fc1.weight.flatten(1), self.fc1.bias, self.fc2.weight.flatten(1),
                                                                       self.fc2.bias))

    def forward(self, x):
        """x: a whole unpadded tensor as an Act.  -> x * g as an Act of its own."""
        c = self.input_channels
        if x.coff != 0 or x.t.shape[3] != c or x.c != c:
            raise NotImplementedError(f'CPCA_ChannelAttention({c}) works on whole tensors of {c} channels')
        if self.fc1.out_channels < 1:
            raise NotImplementedError(f'CPCA_ChannelAttention({c}, {self.fc1.out_channels}): the MLP needs at least one hidden neuron')
        if c > 1024:
            raise NotImplementedError(f'CPCA_ChannelAttention({c}): the shared MLP runs on the small dense layer, at most 1024 channels')
        if not x.t.is_cuda:
            raise RuntimeError('somi_amd CPCA runs on the MI355X only (no CPU fallback)')
        W1, b1, W2, b2 = self._packed(x.t.device)
        B = x.shape[0]
        pooled = torch.empty(2 * B, c, device=x.t.device, dtype=torch.float32)
        ops.global_pool(x.t, c=c, out=pooled)
        h = ops.linear(pooled, W1, b1, 'relu')
        z = ops.linear(h, W2, b2, 'none')
        g = ops.cpca_sigmoid2(z)
        if self.training:
            self.__dict__['_ctx'] = (x, pooled, h, z, g, (W1, W2))
        return Act(ops.scale_channels(x.t, g), 0, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """dout: the gradient of x * g, a whole tensor (Act or tensor).  -> the gradient of x as an Act: a tensor of its own, or copied into
        dx_out's slice (added to it with `accumulate`) by one more pass; None without need_dx (the MLP's gradients are still taken)."""
        x, pooled, h, z, g, (W1, W2) = self.__dict__.pop('_ctx')
        d = dout.t if isinstance(dout, Act) else dout
        B, c = g.shape
        dt, dg = ops.scale_channels_backward(d, x.t, g)
        dz = ops.cpca_sigmoid2_backward(z, dg)
        (gW1, gb1, gW2, gb2), fin = _grad_targets(self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        dh = torch.empty_like(h)
        ops.linear_backward(h, W2, dz, z, 0, 'none', gW2, gb2, dx=dh)
        dpooled = torch.empty_like(pooled)
        ops.linear_backward(pooled, W1, dh, h, 0, 'relu', gW1, gb1, dx=dpooled)
        fin()
        if not need_dx:
            return None
        amaxp = ops.argmax_pixel(x.t, pooled[B:], c)
        ops.pool_backward_add_(dt, 0, c, dpooled[:B], dpooled[B:], amaxp)
        if dx_out is None:
            return Act(dt, 0, c)
        if accumulate:
            ops.add_(dx_out.t, dx_out.coff, dt, 0, c)
        else:
            ops.resample_slice(dt, 0, dx_out.t, dx_out.coff, c)
        return Act(dx_out.t, dx_out.coff, c)


_CPCA_STRIPS = (('dconv1_7', 'dconv7_1', 7), ('dconv1_11', 'dconv11_1', 11), ('dconv1_21', 'dconv21_1', 21))


class _CPCACore(_Packed):
    """The arithmetic CPCA and CPCABottleneck share (models/common.py:5797-5815, 5842-5857), on the children `ca`, `dconv5_5`, the six strip
    convs, `conv` and `act` of the class that mixes this in:
        a = ca(gelu(conv(x)));  u = dconv5_5(a);  s = u + V7(H7(u)) + V11(H11(u)) + V21(H21(u));  out = [s +] conv(conv(s) * a)
    `conv` is ONE 1x1 conv with bias used three times: its weight and bias gradients are the sum over the three uses, accumulated into one
    buffer by the existing wgrad and channel-sum kernels.  The strips are two launches forward (ops.cpca_fanout along W, ops.cpca_fanin along H),
    two for the data gradient (the same kernels with the axes swapped and the taps flipped) and one call for all twelve strip parameter
    gradients (ops.cpca_wgrad).  GELU rides the conv epilogue in eval; in training the pre-activation is kept.  The bottleneck's shortcut
    adds s, the strip sum - the reference's forward rebinds the name `x` to it before `return x + out` (models/common.py:5854, 5859), so that
    is what a trained checkpoint expects -; it rides the last conv's epilogue forward and the second conv's dgrad epilogue backward.  All inner tensors are whole tensors of exactly C channels: C must be a width pad4 leaves alone."""

    def _init_cpca(self, c, r):
        self.ca = CPCA_ChannelAttention(input_channels=c, internal_neurons=c // r)
        self.dconv5_5 = nn.Conv2d(c, c, kernel_size=5, padding=2, groups=c)
        self.dconv1_7 = nn.Conv2d(c, c, kernel_size=(1, 7), padding=(0, 3), groups=c)
        self.dconv7_1 = nn.Conv2d(c, c, kernel_size=(7, 1), padding=(3, 0), groups=c)
        self.dconv1_11 = nn.Conv2d(c, c, kernel_size=(1, 11), padding=(0, 5), groups=c)
        self.dconv11_1 = nn.Conv2d(c, c, kernel_size=(11, 1), padding=(5, 0), groups=c)
        self.dconv1_21 = nn.Conv2d(c, c, kernel_size=(1, 21), padding=(0, 10), groups=c)
        self.dconv21_1 = nn.Conv2d(c, c, kernel_size=(21, 1), padding=(10, 0), groups=c)
        self.conv = nn.Conv2d(c, c, kernel_size=(1, 1), padding=0)
        self.act = nn.GELU()

    def _strip_params(self):
        hs = [getattr(self, h) for h, _, _ in _CPCA_STRIPS]
        vs = [getattr(self, v) for _, v, _ in _CPCA_STRIPS]
        return hs, vs

    def _pack_params(self):
        hs, vs = self._strip_params()
        return [*self.conv.parameters(), *self.dconv5_5.parameters(), *(p for m in hs + vs for p in m.parameters())]

    def _pack(self, dev):
        c = self.conv.in_channels
        f = lambda t: t.detach().float().contiguous().to(dev)       # noqa: E731
        hs, vs = self._strip_params()
        w = self.conv.weight.detach().float()
        pk = dict(wh=[f(m.weight) for m in hs], bh=[f(m.bias) for m in hs], wv=[f(m.weight) for m in vs], bv=[f(m.bias) for m in vs],
                  g5=pack_gconv_weight(self.dconv5_5.weight.detach(), c).to(dev), b5=f(self.dconv5_5.bias))
        pk['wp'], pk['bp'] = pack_conv_weight(w, cin_pad=c, cout_pad=c).to(dev), f(self.conv.bias)
        if self.training:
            pk['wt'] = pack_dgrad_weight(w, cin_pad=c, cout_pad=c).to(dev)
            pk['one'], pk['zero'] = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        return pk

    def _cpca_forward(self, x, add_s, out):
        """x: the attended map (Act of C channels); add_s: the bottleneck's shortcut, + s; out: the Act to write (a new one when None)."""
        c = self.conv.in_channels
        if x.c != c:
            raise RuntimeError(f'CPCA over {c} channels got a map of {x.c}')
        if c % 4 or pad4(c) != c or x.up:
            raise NotImplementedError(f'CPCA over {c} channels: the strip kernels need a real tensor whose channel count is a multiple of 4 and '
                                      f'stored unpadded (a multiple of 32 from 64 up)')
        if not x.t.is_cuda:
            raise RuntimeError('somi_amd CPCA runs on the MI355X only (no CPU fallback)')
        pk = self._packed(x.t.device)
        B, H, W, _ = x.shape
        conv = dict(kh=1, kw=1, stride=1, pad=0, cin=c, cout=c)
        y0 = None
        if self.training:
            y0 = ops.conv2d_nhwc(x.t, pk['wp'], pk['bp'], act='none', x_coff=x.coff, **conv)
            t = ops.chan_affine_act(y0, c, 0, pk['one'], pk['zero'], 'gelu', 0, torch.empty_like(y0))
        else:
            t = ops.conv2d_nhwc(x.t, pk['wp'], pk['bp'], act='gelu', x_coff=x.coff, **conv)
        a = self.ca(Act(t, 0, c))
        u = ops.gconv2d_nhwc(a.t, pk['g5'], pk['b5'], c1=c, c2=c, groups=c, k=5)
        ts = ops.cpca_fanout(u, pk['wh'], pk['bh'], c, axis='w')
        s = ops.cpca_fanin(ts, u, pk['wv'], pk['bv'], c, axis='h')
        sa = ops.conv2d_nhwc(s, pk['wp'], pk['bp'], act='none', **conv)
        p = ops.cpca_gate(sa, a.t, c)
        if out is None:
            out = new_act(x.t, H, W, c)
        ops.conv2d_nhwc(p, pk['wp'], pk['bp'], act='none', out=out.t, y_coff=out.coff, residual=s if add_s else None, **conv)
        if self.training:
            self.__dict__['_cctx'] = (x, y0, a, u, ts, s, sa, p, pk, add_s)
        return Act(out.t, out.coff, c)

    def _cpca_backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """dout: the gradient of the output (Act).  -> the gradient of the attended map as an Act (written into dx_out if given, added to it with
        `accumulate`).  Every parameter gradient is accumulated into .grad."""
        x, y0, a, u, ts, s, sa, p, pk, add_s = self.__dict__.pop('_cctx')
        c = self.conv.in_channels
        B, H, W, _ = x.shape
        direct = ('weight', 'bias')
        dp = _plain_conv_backward(self.conv, Act(p, 0, c), dout.t, pk['wt'], dy_coff=dout.coff, direct=direct)
        dsa, da = ops.cpca_gate_backward(dp.t, sa, a.t, c)
        _plain_conv_backward(self.conv, Act(s, 0, c), dsa, pk['wt'], need_dx=False, direct=direct)
        ds = torch.empty_like(s)                                  # + dout where the shortcut added s
        ops.conv2d_dgrad_nhwc(dsa, pk['wt'], B=B, H=H, W=W, cin=c, kh=1, kw=1, cout=c, out=ds, accumulate=dout.t if add_s else None,
                              acc_coff=dout.coff)
        dts = ops.cpca_fanout(ds, pk['wv'], None, c, axis='h', flip=True)
        du = ops.cpca_fanin(dts, ds, pk['wh'], None, c, axis='w', flip=True)
        hs, vs = self._strip_params()
        tg, fin = _grad_targets(*(m.weight for m in hs), *(m.weight for m in vs), *(m.bias for m in hs), *(m.bias for m in vs))
        ops.cpca_wgrad(u, ts, ds, dts, c, tg[0:3], tg[3:6], tg[6:9], tg[9:12], accumulate=True)
        fin()
        (gw5, gb5), fin = _grad_targets(self.dconv5_5.weight, self.dconv5_5.bias)
        ops.gconv2d_wgrad_nhwc(a.t, du, c1=c, c2=c, groups=c, k=5, out=gw5, accumulate=True)
        ops.chan_sum_(du, c, 0, gb5)
        fin()
        ops.gconv2d_dgrad_nhwc(du, pk['g5'], H=H, W=W, c1=c, c2=c, groups=c, k=5, out=da, cx=c, accumulate=da)
        dt = self.ca.backward(da).t
        ops.gelu_backward_(y0, dt)
        return _plain_conv_backward(self.conv, x, dt, pk['wt'], dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, direct=direct)


class CPCA(_CPCACore):
    """Channel prior convolutional attention as a layer of its own (models/common.py:5782-5815)."""

    def __init__(self, channels, channelAttention_reduce=4):
        super().__init__()
        self._init_cpca(channels, channelAttention_reduce)

    accumulates = folds_pooled = False                           # takes dx_out / accumulate, not walked that way
    reduction = 1

    def forward(self, x, out=None):
        return self._cpca_forward(x, False, out)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        return self._cpca_backward(dout, dx_out, accumulate, need_dx)


class CPCABottleneck(_CPCACore):
    """cv1 -> cv2 -> CPCA arithmetic (+ the strip sum s when shortcut, see _CPCACore) (models/common.py:5818-5859).  The attention's modules are
    sized by c1 and read cv2's c2-channel output: c1 == c2 is required."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5, channelAttention_reduce=4):
        super().__init__()
        if c1 != c2:
            raise NotImplementedError(f'CPCABottleneck({c1}, {c2}): the attention is sized by c1 and reads cv2\'s c2 channels; the reference\'s '
                                      f'forward fails too unless c1 == c2')
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2
        self._init_cpca(c1, channelAttention_reduce)

    accumulates = folds_pooled = False                           # like Bottleneck: takes dx_out / accumulate, not walked that way
    reduction = 1

    def forward(self, x, out=None):
        return self._cpca_forward(self.cv2(self.cv1(x)), self.add, out)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.cv2.backward(self._cpca_backward(dout))
        return self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class C3CPCA(C3):
    """C3 whose bottlenecks are CPCABottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) (models/common.py:1684-1689); repeated inside,
    like C3 (models/yolo.py:1477, 1490)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(CPCABottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) for _ in range(n)))

    accumulates = folds_pooled = False                           # C3's backward, dx_out / accumulate included; the walk adds its gradient itself
    reduction = 1


# ------------------------------------------------------------------------------------------------ the CBAM C3 family
def _cbam_limits(who, c, ratio, train_whole=False, unpadded=False):
    """The widths the CBAM kernels take, checked before any launch: channel quads, a shared MLP of 1..64 hidden neurons over at most 1024
    channels (somi_attn_mlp_f32), and - train_whole: the block's training path scales a whole tensor; unpadded: the block hands tensors of
    exactly c channels on - a width stored unpadded."""
    if c % 4:
        raise NotImplementedError(f'{who}: hidden width {c} is not a multiple of 4 (a lane owns a channel quad)')
    if c // ratio == 0:
        raise NotImplementedError(f'{who}: {c} channels at ratio {ratio} leave the channel attention\'s MLP no hidden neuron '
                                  f'(at least {ratio} channels)')
    if c > 1024 or c // ratio > 64:
        raise NotImplementedError(f'{who}: the channel attention\'s MLP runs on at most 1024 channels and 64 hidden neurons, got {c} and {c // ratio}')
    if unpadded and pad4(c) != c:
        raise NotImplementedError(f'{who}: the gated tensors are exactly {c} channels wide, and {c} channels are stored as a slice of {pad4(c)} '
                                  f'(a multiple of 32 from 64 up)')
    if train_whole and pad4(c) != c:
        raise NotImplementedError(f'{who}: the CBAM training path works on whole tensors, and {c} channels are stored as a slice of {pad4(c)}')


def _gate_kernel_size(who, kernel_size):
    if kernel_size not in (3, 5, 7):
        raise NotImplementedError(f'{who}: kernel_size {kernel_size} of the spatial gate is not built, only 3, 5 and 7')
    return kernel_size


class DepthWiseConv(nn.Module):
    """depthwise k x k conv -> BatchNorm -> ReLU -> 1x1 conv -> BatchNorm -> ReLU (models/common.py:361-389): the parameter holder of the
    depthwise-separable spatial gate; SpatialAttentionModuleDWC runs it."""

    def __init__(self, in_channel, out_channel, kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.depth_conv = nn.Conv2d(in_channel, in_channel, kernel_size, stride, padding, groups=in_channel)
        self.bn = nn.BatchNorm2d(in_channel)
        self.point_conv = nn.Conv2d(in_channel, out_channel, 1, 1, 0)
        self.relu = nn.ReLU(inplace=True)
        self.bn1 = nn.BatchNorm2d(out_channel)

    accumulates = folds_pooled = False
    reduction = 1

    def ordered(self):
        """The parameters in the order of the kernels' flat vector (ops.dwc_gate_*)."""
        return (self.depth_conv.weight, self.depth_conv.bias, self.bn.weight, self.bn.bias, self.point_conv.weight, self.point_conv.bias,
                self.bn1.weight, self.bn1.bias)


class SpatialAttentionModuleDWC(nn.Module):
    """sigmoid(relu(BN1(conv1x1(relu(BN(dwconv_kxk([mean_c, max_c]))))))) (models/common.py:425-438): the ReLU comes before the sigmoid, so the
    gate lies in [0.5, 1).  k is 3 or 7.  Inference: one launch on the running statistics.  Training: three launches (the two BatchNorms take
    batch statistics over (B, H, W), two grid-wide reductions that follow one another), the running statistics and num_batches_tracked move
    as in nn.BatchNorm2d; backward starts at the raw gradient of the gate: six launches for dstats and the eight parameter gradients."""

    def __init__(self, kernel_size=7):
        super().__init__()
        if kernel_size not in (3, 7):
            raise NotImplementedError(f'SpatialAttentionModuleDWC: kernel_size {kernel_size} is not built, only 3 and 7 (the reference asserts the same)')
        self.cv1 = DepthWiseConv(2, 1, kernel_size, padding=3 if kernel_size == 7 else 1)
        self.sigmoid = nn.Sigmoid()

    accumulates = folds_pooled = False
    reduction = 1

    def _vectors(self, dev):
        g = self.cv1
        params = torch.cat([p_.detach().float().reshape(-1) for p_ in g.ordered()]).to(dev)
        run = torch.cat([g.bn.running_mean, g.bn.running_var, g.bn1.running_mean, g.bn1.running_var]).detach().float().to(dev)
        return params, run

    def gate(self, stats):
        """stats (B,H,W,2) -> sa (B,H,W)."""
        g = self.cv1
        k = g.depth_conv.kernel_size[0]
        if g.bn.eps != g.bn1.eps or g.bn.momentum != g.bn1.momentum:
            raise NotImplementedError('SpatialAttentionModuleDWC: the two BatchNorms share eps and momentum on the SOMI path')
        params, run = self._vectors(stats.device)
        if not self.training:
            return ops.dwc_gate_eval(stats, params, run, k, g.bn.eps)
        if ops.SYNC_BN is not None:
            raise NotImplementedError('SpatialAttentionModuleDWC: the gate\'s two BatchNorms take local batch statistics; not under ops.SYNC_BN')
        sa, u, p, st = ops.dwc_gate_train(stats, params, run, k, g.bn.eps, g.bn.momentum)
        with torch.no_grad():
            g.bn.running_mean.copy_(run[0:2]), g.bn.running_var.copy_(run[2:4])
            g.bn1.running_mean.copy_(run[4:5]), g.bn1.running_var.copy_(run[5:6])
        _bump_batches_tracked(g.bn)
        _bump_batches_tracked(g.bn1)
        self.__dict__['_ctx'] = (stats, u, p, st, params)
        return sa

    def gate_backward(self, dsa):
        """dsa: the raw gradient of the gate -> dstats; the eight parameter gradients into .grad."""
        stats, u, p, st, params = self.__dict__.pop('_ctx')
        k = self.cv1.depth_conv.kernel_size[0]
        dparams = torch.zeros_like(params)
        dstats = ops.dwc_gate_backward(dsa, stats, u, p, st, params, k, dparams)
        off = 0
        for p_ in self.cv1.ordered():
            _acc_grad(p_, dparams[off:off + p_.numel()].view_as(p_))
            off += p_.numel()
        return dstats


class _TailGate(nn.Module):
    """What SCBAMBottleneck and C3CBAM share: on the children `channel_attention` (ChannelAttentionModule) and `spatial_attention`
    (SpatialAttentionModule), ca = channel_attention(t), sa = the k x k gate of [mean_c, max_c] of t * ca, and ONE pass that combines t, ca and sa
    into the output's channel slice (+ a shortcut): ops.gate_combine, as a product (CBAM) or as sigmoid(t * (ca + sa)) (SCBAM).  Forward:
    global_pool (none when the producing Conv took the pools), attn_mlp, chan_stats, spatial_attn, gate_combine.  Backward: the per-pixel pass
    (d logit, both arg-maxima), step B of train_blocks.hip (three launches), the per-element pass (dt + dca, two launches), the MLP backward (two)."""

    def _gate_forward(self, t, mode, residual=None, out=None, pooled=None):
        c = t.c
        if t.up:
            raise NotImplementedError(f'{type(self).__name__}: an upsampled view is not a map the gates can pool')
        if not t.t.is_cuda:
            raise RuntimeError(f'somi_amd {type(self).__name__} runs on the MI355X only (no CPU fallback)')
        ca = self.channel_attention(t, pooled=pooled)
        sam = self.spatial_attention
        stats = ops.chan_stats(t.t, ca, c=c, x_coff=t.coff)
        w = None
        if isinstance(sam, SpatialAttentionModuleDWC):
            sa = sam.gate(stats)
        else:
            if self.training:
                sam.invalidate()
            w, b = sam._packed(t.t.device)
            sa = ops.spatial_attn(stats, w, b, sam.cv1.kernel_size[0])
        B, H, W, _ = t.shape
        if out is None:
            out = concat_act(t.t, H, W, c)                        # pad channels (if any) zero
        ops.gate_combine(t.t, ca, sa, c, mode, t.coff, residual=None if residual is None else residual.t,
                         res_coff=0 if residual is None else residual.coff, out=out.t, o_coff=out.coff)
        if self.training:
            self.__dict__['_gctx'] = (t, ca, stats, sa, w, mode)
        return Act(out.t, out.coff, c)

    def _gate_backward(self, dout, dt=None, accumulate=False, defer=False):
        """dout: the gradient of the combined output (Act).  -> (the gradient of t as an Act: a tensor of its own, or dt's slice, added to it
        with `accumulate`; the channel attention's pooled part (davg, dmax, amaxp) with `defer`, else None: it is added to that Act in place)."""
        t, ca, stats, sa, w, mode = self.__dict__.pop('_gctx')
        sam, c = self.spatial_attention, t.c
        dwc = isinstance(sam, SpatialAttentionModuleDWC)          # its backward starts at the sigmoid: the raw gradient of the gate
        t_max = self.channel_attention.__dict__['_ctx'][2]        # the pooled maxima: the per-pixel pass finds their first pixels by value
        dlogit, amaxc, amaxp = ops.gate_combine_backward_pixel(dout.t, t.t, ca, sa, c, mode, dout.coff, t.coff, t_max=t_max, logit=not dwc)
        if dwc:
            dstats = sam.gate_backward(dlogit)
        else:
            (dw, db), fin = _grad_targets(sam.cv1.weight, sam.cv1.bias)     # accumulated in nn.Conv2d's (1,2,k,k) layout
            dstats = ops.spatial_attn_backward(dlogit, stats, w, sam.cv1.kernel_size[0], dw, db)
            fin()
        d, dca = ops.gate_combine_backward_chan(dout.t, t.t, ca, sa, dstats, amaxc, c, mode, dout.coff, t.coff, dt=None if dt is None else dt.t,
                                                dt_coff=0 if dt is None else dt.coff, accumulate=accumulate)
        d = Act(d, 0 if dt is None else dt.coff, c)
        return d, self.channel_attention.backward(dca, d, amaxp, defer=defer)


class SCBAMBottleneck(_TailGate):
    """x2 = cv2(cv1(x)) (1x1, 3x3);  yc = ca(x2) * x2;  ys = sa(yc) * x2 - the gate is computed from yc but multiplies x2 -;
    out = sigmoid(yc + ys) (+ x) (models/common.py:975-995).  Ratio 16, plain 7x7 gate.  The gated tensor is the block's output: the combine
    pass writes `out`'s channel slice, shortcut included; backward hands the pooled part of the channel attention's gradient to cv2's BatchNorm
    backward and the shortcut's gradient to cv1's data-gradient epilogue."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, ratio=16, kernel_size=7):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2
        self.channel_attention = ChannelAttentionModule(c2, ratio)
        self.spatial_attention = SpatialAttentionModule(_gate_kernel_size(f'SCBAMBottleneck({c1}, {c2})', kernel_size))
        self.sigmoid = nn.Sigmoid()
        self.ratio = ratio

    accumulates = folds_pooled = False                           # like Bottleneck: takes dx_out / accumulate, not walked that way
    reduction = 1

    def forward(self, x, out=None):
        c1, c2 = self.cv1.conv.in_channels, self.cv2.conv.out_channels
        _cbam_limits(f'SCBAMBottleneck({c1}, {c2})', c2, self.ratio, unpadded=True)
        pool = {} if self.training else None
        x2 = self.cv2(self.cv1(x), pool=pool)                     # training: the BatchNorm + SiLU pass also takes the attention's global pools
        return self._gate_forward(x2, 'sigmoid_sum', x if self.add else None, out, (pool['avg'], pool['max']) if pool else None)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d, pooled = self._gate_backward(dout, defer=True)
        d = self.cv2.backward(d, pooled=pooled)
        c1 = self.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0
        dx = self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if self.add and not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class CBAMBottleneckDWC(_TailGate):
    """x2 = cv2(cv1(x));  t1 = ca(x2) * x2 (ratio 16);  out = sa(t1) * t1 (+ x), sa the depthwise-separable gate (models/common.py:953-972).
    The signature is the reference's: e comes BEFORE k.  The gated tensor is the block's output: the combine pass writes `out`'s slice."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, k=(3, 3), ratio=16, kernel_size=7):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2
        self.channel_attention = ChannelAttentionModule(c2, ratio)
        self.spatial_attention = SpatialAttentionModuleDWC(kernel_size)
        self.ratio = ratio

    accumulates = folds_pooled = False                           # like Bottleneck: takes dx_out / accumulate, not walked that way
    reduction = 1

    def forward(self, x, out=None):
        c1, c2 = self.cv1.conv.in_channels, self.cv2.conv.out_channels
        _cbam_limits(f'CBAMBottleneckDWC({c1}, {c2})', c2, self.ratio, unpadded=True)
        if self.training and ops.SYNC_BN is not None:
            raise NotImplementedError(f'CBAMBottleneckDWC({c1}, {c2}): the gate\'s two BatchNorms take local batch statistics; not under ops.SYNC_BN')
        pool = {} if self.training else None
        x2 = self.cv2(self.cv1(x), pool=pool)
        return self._gate_forward(x2, 'product', x if self.add else None, out, (pool['avg'], pool['max']) if pool else None)

    backward = SCBAMBottleneck.backward


class C3CBAM(_TailGate):
    """A bare CBAM on its input as a row of its own: out = sa(ca(x) * x) * (ca(x) * x) (models/common.py:494-504).  Ratio 16, 7x7 gate; c2 is
    ignored, the channels pass through.  Never in place: other rows may read its input."""

    def __init__(self, c1, c2):
        super().__init__()
        self.kernel_size = 7
        self.channel_attention = ChannelAttentionModule(c1)
        self.spatial_attention = SpatialAttentionModule(self.kernel_size)

    accumulates = folds_pooled = False                           # takes dx_out / accumulate, not walked that way
    reduction = 1

    def forward(self, x, out=None):
        c = self.channel_attention.shared_MLP[0].in_features
        if x.c != c:
            raise RuntimeError(f'C3CBAM over {c} channels got a map of {x.c}')
        _cbam_limits(f'C3CBAM({c})', c, 16, unpadded=True)
        return self._gate_forward(x, 'product', None, out)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        """-> the gradient of the input as an Act (a tensor of its own, or dx_out's slice, added to it with `accumulate`); None without need_dx
        (the gates' parameter gradients are still taken)."""
        if not need_dx:
            self._gate_backward(dout, defer=True)
            return None
        return self._gate_backward(dout, dx_out, accumulate and dx_out is not None)[0]


class _C3Gated(C3):
    """A C3 whose bottlenecks carry CBAM-style attention; `_limits` refuses the widths the attention kernels do not take before any launch."""

    accumulates = folds_pooled = False
    reduction = 1

    def forward(self, x):
        self._limits()
        return super().forward(x)


class C3_CBAM(_C3Gated):
    """C3 whose bottlenecks are CBAMBottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0, kernel_size=7) (models/common.py:1640-1648):
    ratio 8, attention between cv1 (1x1) and cv2; repeated inside (models/yolo.py:1473, 1487).  C3.backward takes each bottleneck's input
    gradient as a returned tensor (CBAMBottleneck.backward's returning form)."""
    KERNEL = 7

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, kernel_size=None):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        k = _gate_kernel_size(f'{type(self).__name__}({c1}, {c2})', self.KERNEL if kernel_size is None else kernel_size)
        self.m = nn.Sequential(*(CBAMBottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0, kernel_size=k) for _ in range(n)))

    accumulates = folds_pooled = False                           # C3's backward, dx_out / accumulate included; the walk adds its gradient itself
    reduction = 1

    def _limits(self):
        c1, c_, c2 = self.cv1.conv.in_channels, self.cv1.conv.out_channels, self.cv3.conv.out_channels
        _cbam_limits(f'{type(self).__name__}({c1}, {c2})', c_, 8, train_whole=self.training)


class C3_CBAMS(C3_CBAM):
    """C3_CBAM with a 3x3 spatial gate (models/common.py:1662-1670)."""
    KERNEL = 3

    accumulates = folds_pooled = False
    reduction = 1


class C3_SCBAM(_C3Gated):
    """C3 whose bottlenecks are SCBAMBottleneck(c_, c_, shortcut, g, e=1.0) (models/common.py:1700-1705); repeated inside
    (models/yolo.py:1477, 1490).  The last bottleneck's combine pass writes C3's concat slice."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(SCBAMBottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))

    accumulates = folds_pooled = False
    reduction = 1

    def _limits(self):
        c1, c_, c2 = self.cv1.conv.in_channels, self.cv1.conv.out_channels, self.cv3.conv.out_channels
        _cbam_limits(f'C3_SCBAM({c1}, {c2})', c_, 16, unpadded=True)


class _C3DWC(_C3Gated):
    KERNEL = 7

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, kernel_size=None):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        k = self.KERNEL if kernel_size is None else kernel_size
        if k not in (3, 7):
            raise NotImplementedError(f'{type(self).__name__}({c1}, {c2}): kernel_size {k} of the depthwise-separable gate is not built, only 3 and 7')
        self.m = nn.Sequential(*(CBAMBottleneckDWC(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0, kernel_size=k) for _ in range(n)))

    accumulates = folds_pooled = False
    reduction = 1

    def _limits(self):
        c1, c_, c2 = self.cv1.conv.in_channels, self.cv1.conv.out_channels, self.cv3.conv.out_channels
        _cbam_limits(f'{type(self).__name__}({c1}, {c2})', c_, 16, unpadded=True)
        if self.training and ops.SYNC_BN is not None:
            raise NotImplementedError(f'{type(self).__name__}({c1}, {c2}): the gate\'s two BatchNorms take local batch statistics; not under ops.SYNC_BN')


class C3_CBAM_DWC(_C3DWC):
    """C3 whose bottlenecks are CBAMBottleneckDWC(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0, kernel_size=7) (models/common.py:1651-1659);
    repeated inside (models/yolo.py:1474, 1488)."""
    KERNEL = 7

    accumulates = folds_pooled = False
    reduction = 1


class C3_CBAMS_DWC(_C3DWC):
    """C3_CBAM_DWC with a 3x3 depthwise gate (models/common.py:1673-1681)."""
    KERNEL = 3

    accumulates = folds_pooled = False
    reduction = 1


# ------------------------------------------------------------------------------------------------ SimAM
class _SimAMGate(nn.Module):
    """The parameter-free SimAM gate over a grid of regions (simam.hip), shared by SimAM (one region), SimAMWithSlicing (four quadrants) and
    SimAMWithFlexibleSlicing (windows): per (image, region, channel) mu = the mean over the region's own pixels, d = x - mu, S = sum d^2,
    D = 4 (S / n + e_lambda), out = sum over the regions covering a pixel of w x sigmoid(d^2 / D + 0.5).  Forward: ops.simam_stats, then
    ops.simam_apply; backward: ops.simam_backward_sums, then ops.simam_backward_input, the gate recomputed from x and the kept statistics.
    Subclasses give _grid(H, W) -> ops.simam_grid(...), which raises the limits by name before anything is launched."""

    def _gate_width(self, a, what):
        """How many channels the kernels walk of Act `a`: its whole padded width (pad channels hold zeros and come out zero), or an aligned slice."""
        if a.up:
            raise NotImplementedError(f'{type(self).__name__} needs a real tensor, not an upsampled view')
        if a.coff == 0 and a.t.shape[3] == pad4(a.c):
            return pad4(a.c)
        if a.c % 4 or a.coff % 4:
            raise NotImplementedError(f'{type(self).__name__}: {what} as a channel slice needs a channel count and offset that are multiples of 4')
        return a.c

    def forward(self, x, out=None, add_input=False):
        """out = [x +] gate(x); add_input: PSSimAM's b + attn(b) in the same pass."""
        B, H, W, _ = x.shape
        grid = self._grid(H, W)
        cw = self._gate_width(x, 'the input')
        if not x.t.is_cuda:
            raise RuntimeError('somi_amd SimAM runs on the MI355X only (no CPU fallback)')
        if out is None:
            out = new_act(x.t, H, W, x.c)
        elif self._gate_width(Act(out.t, out.coff, x.c), 'the output') != cw:
            raise NotImplementedError(f'{type(self).__name__}: input and output must both be whole padded tensors or both aligned slices')
        stats = ops.simam_stats(x.t, cw, grid, x.coff)
        ops.simam_apply(x.t, stats, cw, grid, x.coff, out=out.t, o_coff=out.coff, add_input=add_input)
        if self.training:
            self.__dict__['_ctx'] = (x, stats, grid, cw)
        return Act(out.t, out.coff, x.c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True, add_input=False):
        """-> the gradient of x as an Act: written into dx_out if given, added to it with `accumulate`.  add_input: the forward's `x +`."""
        x, stats, grid, cw = self.__dict__.pop('_ctx')
        if not need_dx:
            return None
        if self._gate_width(Act(dout.t, dout.coff, x.c), 'the output gradient') != cw:
            raise NotImplementedError(f'{type(self).__name__}: the output gradient must be laid out like the input')
        B, H, W, _ = x.shape
        if dx_out is None:
            dx_out, accumulate = new_act(x.t, H, W, x.c), False
        elif self._gate_width(Act(dx_out.t, dx_out.coff, x.c), 'the input gradient') != cw:
            raise NotImplementedError(f'{type(self).__name__}: the input gradient must be laid out like the input')
        sums = ops.simam_backward_sums(dout.t, x.t, stats, cw, grid, dout.coff, x.coff)
        ops.simam_backward_input(dout.t, x.t, stats, sums, cw, grid, dout.coff, x.coff, out=dx_out.t, dx_coff=dx_out.coff,
                                 accumulate=accumulate, add_input=add_input)
        return Act(dx_out.t, dx_out.coff, x.c)


class SimAM(_SimAMGate):
    """SimAM over the whole map (models/common.py:2915-2939): one region, n = H W - 1.  c1 is ignored, as in the reference."""

    def __init__(self, c1, e_lambda=1e-4):
        super().__init__()
        self.activaton = nn.Sigmoid()                            # the reference's spelling; parameter-free
        self.e_lambda = e_lambda

    accumulates, folds_pooled, reduction = False, False, 1       # takes dx_out / accumulate, not walked that way

    def _grid(self, H, W):
        return ops.simam_grid('map', H, W, self.e_lambda)


class SimAMWithSlicing(_SimAMGate):
    """SimAM per quadrant (models/common.py:9374-9408): rows split at H // 2, columns at W // 2 - on odd sizes the second region is the larger
    one -, each region's mean and S over its own pixels, and n = (H // 2)(W // 2) - 1 for all four, the larger ones included."""

    def __init__(self, c1, e_lambda=1e-4):
        super().__init__()
        self.activation = nn.Sigmoid()
        self.e_lambda = e_lambda

    accumulates, folds_pooled, reduction = False, False, 1

    def _grid(self, H, W):
        return ops.simam_grid('quadrants', H, W, self.e_lambda)


class SimAMWithFlexibleSlicing(_SimAMGate):
    """SimAM per target_size x target_size window (models/common.py:9411-9480): windows start at range(0, H - t + 1, st) x range(0, W - t + 1, st),
    st = t without overlap, else int(t (1 - overlap_ratio)); n = t t - 1.  Pixels no window covers are ZERO in the output.  With overlap the
    reference divides a window's contribution by the coverage count at the time it is added, so the k-th window over a pixel (row-major) counts
    1 / k - not 1 / (the final count); the kernels do the same."""

    def __init__(self, c1, target_size, overlap_ratio=0.0, e_lambda=1e-4):
        super().__init__()
        self.target_size = target_size
        self.overlap_ratio = overlap_ratio
        if target_size < 2:
            raise ValueError(f'SimAMWithFlexibleSlicing: target_size {target_size}: a window of one pixel has no variance (the reference divides 0 by 0)')
        st = target_size if overlap_ratio == 0.0 else int(target_size * (1 - overlap_ratio))
        if st < 1:
            raise ValueError(f'SimAMWithFlexibleSlicing: overlap_ratio {overlap_ratio} at target_size {target_size} gives a stride of {st} '
                             f'(the reference\'s range() raises)')
        if -(-target_size // st) > ops.SIMAM_MAX_COVER:
            raise NotImplementedError(f'SimAMWithFlexibleSlicing: overlap_ratio {overlap_ratio} at target_size {target_size} (stride {st}) puts '
                                      f'{-(-target_size // st)} windows over a pixel along one axis; the kernels take at most {ops.SIMAM_MAX_COVER}')
        self.stride = (st, st)
        self.activation = nn.Sigmoid()
        self.e_lambda = e_lambda

    accumulates, folds_pooled, reduction = False, False, 1

    def _grid(self, H, W):
        return ops.simam_grid('windows', H, W, self.e_lambda, self.target_size, self.stride[0])


class Conv_SWS(Conv):
    """act(bn(conv(att(x)))), att = SimAMWithFlexibleSlicing(c1, target_size, overlap_ratio, e_lambda) (models/common.py:9483-9495): a Conv with
    sliding-window SimAM in front of it.  Children conv, bn, act, att as in the reference; att has no parameters.  The reference's fuseforward
    (another order) is dead code there - Model.fuse only touches Conv / DWConv instances - and is not mirrored."""

    def __init__(self, c1, c2, target_size, overlap_ratio=0.0, e_lambda=1e-4, k=1, s=1, p=None, g=1, act=True):
        super().__init__(c1, c2, k, s, p, g, 1, act)
        self.att = SimAMWithFlexibleSlicing(c1, target_size, overlap_ratio, e_lambda)

    accumulates = folds_pooled = False                           # the gate's backward stands between the conv's data gradient and the input
    reduction = property(lambda self: self.conv.stride[0])

    def forward(self, x, out=None):
        return Conv.forward(self, self.att(x), out=out)

    def backward(self, dz, dx_out=None, accumulate=False, need_dx=True):
        if not need_dx:
            self.att.__dict__.pop('_ctx', None)
            return Conv.backward(self, dz, need_dx=False)
        return self.att.backward(Conv.backward(self, dz), dx_out=dx_out, accumulate=accumulate)


class PSSimAM(nn.Module):
    """cv2(cat(a, b2)) with a, b = cv1(x).split, b1 = b + SimAM(b), b2 = b1 + ffn(b1) (models/common.py:2942-2961): PSA's shape around SimAM.
    cv1 writes [a | b] into cv2's input buffer and ffn[1] writes b2 over b.  Eval: the gate reads b in place, a channel slice at offset c.
    Training: b is copied out once first - the gate's backward recomputes it from the b it read -; `b +` rides the gate's apply pass and its
    gradient the gate's input-gradient pass, which writes b's gradient next to a's, so cv1 reads one buffer."""

    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        if c1 != c2:
            raise ValueError(f'PSSimAM needs c1 == c2, got {c1} and {c2}')
        self.c = int(c1 * e)
        if self.c % 4 or self.c == 0:
            raise NotImplementedError(f'PSSimAM with {self.c} channels per branch: the branches are channel slices, a multiple of 4 channels each')
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.attn = SimAM(self.c)
        self.ffn = nn.Sequential(Conv(self.c, self.c * 2, 1), Conv(self.c * 2, self.c, 1, act=False))

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x):
        c = self.c
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, 2 * c)
        self.cv1(x, out=cat)
        b = cat.slice(c, c)
        if self.training:                                         # ffn[1] overwrites cat's b; the gate's backward needs it
            b = new_act(x.t, H, W, c)
            ops.resample_slice(cat.t, c, b.t, 0, c)
        b1 = self.attn(b, add_input=True)
        self.ffn[1](self.ffn[0](b1), out=cat.slice(c, c), residual=b1)
        return self.cv2(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        c = self.c
        dcat = self.cv2.backward(dout)
        db2 = dcat.slice(c, c)
        db1 = self.ffn[0].backward(self.ffn[1].backward(db2), also_add=db2)
        self.attn.backward(db1, dx_out=db2, add_input=True)       # db2's slice is free again: it takes b's gradient
        return self.cv1.backward(dcat, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


# ================================================================================================ ASF-YOLO neck
def _asf_real(a, what):
    """An input of the ASF blocks: a real tensor (no nn.Upsample view), channel slice offset and width multiples of 4."""
    if a.up:
        raise NotImplementedError(f'{what}: an nn.Upsample view as input is not on the SOMI path (the kernels read real maps)')
    if a.c % 4 or a.coff % 4:
        raise NotImplementedError(f'{what}: channel counts and slice offsets must be multiples of 4 (C % 4 == 0), got {a.c} at {a.coff}')


def _asf_on_gpu(a, what):
    if not a.t.is_cuda:
        raise RuntimeError(f'somi_amd {what} runs on the MI355X only (no CPU fallback)')


class Zoom_cat(nn.Module):
    """cat(adaptive_max_pool2d(l) + adaptive_avg_pool2d(l), m, nearest(s)) at m's size (models/common.py:4312-4327) for l exactly 2x and s
    exactly 1/2 of m per axis: one launch writes the three channel slices of the output (the reference makes two pooled maps, a sum, an
    upsampled map and a concat); training keeps a two-bit arg-max code per pooled element.  Backward, one owner-computes launch: dl and ds in
    tensors of their own, dm a slice of the incoming gradient (no copy), as Concat hands its gradients out."""

    def __init__(self, in_dim):
        super().__init__()

    accumulates, folds_pooled, reduction = False, False, 2       # several inputs: backward(dout) returns the list of their gradients; l is 2x the output

    def forward(self, xs):
        if len(xs) != 3:
            raise RuntimeError(f'Zoom_cat takes three inputs (l, m, s), got {len(xs)}')
        l, m, s = xs
        for a in xs:
            _asf_real(a, 'Zoom_cat')
        B, H, W = m.shape[:3]
        if tuple(l.shape[:3]) != (B, 2 * H, 2 * W):
            raise NotImplementedError(f'Zoom_cat: l must be exactly 2x m per axis ({2 * H}x{2 * W}), got {l.shape[1]}x{l.shape[2]} '
                                      f'(non-integer zoom ratios are not on the SOMI path)')
        if H % 2 or W % 2 or tuple(s.shape[:3]) != (B, H // 2, W // 2):
            raise NotImplementedError(f'Zoom_cat: s must be exactly m / 2 per axis, got {s.shape[1]}x{s.shape[2]} under m {H}x{W} '
                                      f'(non-integer zoom ratios are not on the SOMI path)')
        _asf_on_gpu(m, 'Zoom_cat')
        out = concat_act(m.t, H, W, l.c + m.c + s.c)
        r = ops.zoomcat(l.t, m.t, s.t, l.c, m.c, s.c, l.coff, m.coff, s.coff, out=out.t, codes=self.training)
        if self.training:
            self.__dict__['_ctx'] = (r[1], l.c, m.c, s.c)
        return out

    def backward(self, dout):
        codes, cl, cm, cs = self.__dict__.pop('_ctx')
        dl, _, ds = ops.zoomcat_backward(dout.t, codes, cl, cm, cs, dout.coff)
        return [Act(dl, 0, cl), dout.slice(cl, cm), Act(ds, 0, cs)]


class ScalSeq(_Packed):
    """Scale sequence fusion (models/common.py:4330-4355): P4 and P5 through a 1x1 Conv each, nearest-upsampled to P3's size, the three stacked
    along a depth axis, Conv3d(1x1x1) -> BatchNorm3d -> LeakyReLU(0.1) -> max over the depth.  The Conv3d acts per pixel and the upsampling is
    nearest at exactly 2x and 4x, so conv and affine commute with it: u_i = conv3d(.) is ONE 1x1 conv per level at the level's own resolution,
    the batch statistics over the virtual (B,C,3,H,W) stack are the three maps' sums weighted 1, 4, 16 (ops.scalseq_stats), and one launch
    takes max_i leaky(scale u_i + shift) per P3 pixel (ops.scalseq_fuse).  No stacked and no upsampled tensor exists.  Eval folds the BatchNorm
    into the shared 1x1 weights.  Backward: two launches (route, apply) give du_i at the maps' own resolutions, then the existing wgrad
    (three calls into one buffer) and dgrad; conv1 and conv2 are plain Conv backwards."""

    def __init__(self, channel):
        super().__init__()
        self.conv1 = Conv(512, channel, 1)
        self.conv2 = Conv(1024, channel, 1)
        self.conv3d = nn.Conv3d(channel, channel, kernel_size=(1, 1, 1))
        self.bn = nn.BatchNorm3d(channel)
        self.act = nn.LeakyReLU(0.1)
        self.pool_3d = nn.MaxPool3d(kernel_size=(3, 1, 1))

    accumulates, folds_pooled, reduction = False, False, 1       # several inputs: backward(dout) returns the list of their gradients

    def _pack_params(self):
        return [*self.conv3d.parameters(), *self.bn.parameters()]

    def _pack(self, dev):
        c = self.conv3d.out_channels
        w = self.conv3d.weight.detach().float().view(c, c, 1, 1)
        b = self.conv3d.bias.detach().float()
        if not self.training:                                    # BatchNorm3d folded into the shared 1x1 conv
            s, t = bn_fold(self.bn)
            w, b = w * s.detach().float().view(-1, 1, 1, 1), b * s.detach().float() + t.detach().float()
        pk = dict(w=pack_conv_weight(w, cin_pad=pad4(c), cout_pad=c).to(dev), b=b.to(dev).contiguous())
        if self.training:
            pk['wt'] = pack_dgrad_weight(w, cin_pad=pad4(c), cout_pad=c).to(dev)
            pk['gamma'], pk['beta'] = self.bn.weight.detach().float().to(dev).contiguous(), self.bn.bias.detach().float().to(dev).contiguous()
        return pk

    def forward(self, xs):
        if len(xs) != 3:
            raise RuntimeError(f'ScalSeq takes three inputs (p3, p4, p5), got {len(xs)}')
        p3, p4, p5 = xs
        c = self.conv3d.out_channels
        for a in xs:
            _asf_real(a, 'ScalSeq')
        if c % 4:
            raise NotImplementedError(f'ScalSeq({c}): the channel count must be a multiple of 4 (C % 4 == 0)')
        if p3.c != c:
            raise NotImplementedError(f'ScalSeq({c}): the p3 input must have {c} channels (the reference stacks it unchanged), got {p3.c}')
        B, H, W = p3.shape[:3]
        if H % 4 or W % 4 or tuple(p4.shape[:3]) != (B, H // 2, W // 2) or tuple(p5.shape[:3]) != (B, H // 4, W // 4):
            raise NotImplementedError(f'ScalSeq: the maps must be exactly 1 : 1/2 : 1/4 per axis, got {tuple(p3.shape[1:3])}, '
                                      f'{tuple(p4.shape[1:3])}, {tuple(p5.shape[1:3])} (non-integer zoom ratios are not on the SOMI path)')
        if self.training and ops.SYNC_BN is not None:
            raise NotImplementedError("ScalSeq's BatchNorm3d has no sync-BN form (--sync-bn)")
        _asf_on_gpu(p3, 'ScalSeq')
        pk = self._packed(p3.t.device)
        srcs = (p3, self.conv1(p4), self.conv2(p5))
        us = tuple(ops.conv2d_nhwc(a.t, pk['w'], pk['b'], kh=1, kw=1, stride=1, pad=0, act='none', cin=pad4(c), x_coff=a.coff, cout=c,
                                   out=torch.empty(*a.shape[:3], c, device=a.t.device, dtype=torch.float32), alg_cin=c) for a in srcs)
        out = new_act(p3.t, H, W, c)
        if out.t.shape[3] != c:
            out.t.zero_()                                         # pad channels of a tensor of its own
        if not self.training:
            ops.scalseq_fuse(us, c, out=out.t)
            return out
        bn = self.bn
        dev = p3.t.device
        inplace = bn.running_mean.device == dev and bn.running_mean.dtype == torch.float32
        rm = bn.running_mean if inplace else bn.running_mean.detach().float().to(dev).clone()
        rv = bn.running_var if inplace else bn.running_var.detach().float().to(dev).clone()
        momentum = bn.momentum if bn.momentum is not None else 1.0 / (int(bn.num_batches_tracked) + 1)
        st = ops.scalseq_stats(us, c, pk['gamma'], pk['beta'], bn.eps, momentum, rm, rv)
        with torch.no_grad():
            if not inplace:
                bn.running_mean.copy_(rm)
                bn.running_var.copy_(rv)
            _bump_batches_tracked(bn)
        _, codes = ops.scalseq_fuse(us, c, st[2], st[3], out=out.t, codes=True)
        self.__dict__['_ctx'] = (srcs, us, st, codes, pk)
        return out

    def backward(self, dout):
        srcs, us, st, codes, pk = self.__dict__.pop('_ctx')
        c = self.conv3d.out_channels
        dev = dout.t.device
        (dgam, dbet), fin = _grad_targets(self.bn.weight, self.bn.bias)
        gs, sums = ops.scalseq_route_backward(dout.t, codes, us, c, st, do_coff=dout.coff, dgamma=dgam, dbeta=dbet)
        fin()
        ops.scalseq_apply_backward(gs, us, c, st, sums)           # gs now hold du_i
        conv = dict(kh=1, kw=1, stride=1, pad=0)
        dw, db = None, torch.zeros(c, device=dev)
        for a, du in zip(srcs, gs):                               # the shared weight: three wgrad calls into one buffer
            dw = ops.conv2d_wgrad_nhwc(a.t, du, cin=pad4(c), x_coff=a.coff, cout=c, out=dw, accumulate=dw, **conv)
            ops.chan_sum_(du, c, 0, db)
        _acc_grad(self.conv3d.weight, dw.view(c, pad4(c))[:, :c].reshape(c, c, 1, 1, 1))
        _acc_grad(self.conv3d.bias, db)
        ds = []
        for a, du in zip(srcs, gs):
            B, H, W, _ = a.shape
            dx = torch.empty(B, H, W, pad4(c), device=dev, dtype=torch.float32)
            ops.conv2d_dgrad_nhwc(du, pk['wt'], B=B, H=H, W=W, cin=pad4(c), cout=c, out=dx, **conv)
            ds.append(Act(dx, 0, c))
        return [ds[0], self.conv1.backward(ds[1]), self.conv2.backward(ds[2])]


class channel_att(nn.Module):
    """ECA: x * sigmoid(conv1d_k(global average of x)) along the channels (models/common.py:4358-4374); k from the reference's formula.  Holds the
    nn.Conv1d; attention_model runs it (ops.global_pool, ops.eca_gate) with the product folded into the mix in front of local_att."""

    def __init__(self, channel, b=1, gamma=2):
        super().__init__()
        kernel_size = ops.eca_kernel_size(channel, b, gamma)
        if kernel_size > ops.ECA_KMAX:
            raise NotImplementedError(f'channel_att({channel}): kernel size {kernel_size} is beyond {ops.ECA_KMAX}')
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv = nn.Conv1d(1, 1, kernel_size=kernel_size, padding=(kernel_size - 1) // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        raise RuntimeError('channel_att runs inside attention_model on the SOMI path (its product is folded into the mix kernel)')


class local_att(nn.Module):
    """x * s_h * s_w, s_h / s_w = sigmoid(F_h / F_w(relu(bn(conv_1x1(cat(row means, column means)))))) (models/common.py:4377-4409): coordinate
    attention with ReLU for h-swish and no conv biases.  Holds the parameters; attention_model runs it on the coordinate-attention kernels."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.conv_1x1 = nn.Conv2d(in_channels=channel, out_channels=channel // reduction, kernel_size=1, stride=1, bias=False)
        self.relu = nn.ReLU()
        self.bn = nn.BatchNorm2d(channel // reduction)
        self.F_h = nn.Conv2d(in_channels=channel // reduction, out_channels=channel, kernel_size=1, stride=1, bias=False)
        self.F_w = nn.Conv2d(in_channels=channel // reduction, out_channels=channel, kernel_size=1, stride=1, bias=False)
        self.sigmoid_h = nn.Sigmoid()
        self.sigmoid_w = nn.Sigmoid()

    def forward(self, x):
        raise RuntimeError('local_att runs inside attention_model on the SOMI path (its means come from the mix kernel)')


class attention_model(_Packed):
    """local_att(channel_att(x1) + x2) (models/common.py:4412-4424).  Forward: the global average of x1 (ops.global_pool), the ECA gate on
    (B, C) (ops.eca_gate), ONE pass that writes t = x1 gate + x2 and takes t's row and column means (ops.asf_mix_means), the small convs and
    the BatchNorm on B (H + W) rows as coordinate attention runs them (ReLU, no biases; F_h and F_w stacked as one 1x1 conv), and
    ops.coordatt_apply.  Backward: coordinate attention's two passes give dt, which IS dx2; ds = sum dt x1 (one pass), the ECA backward on
    (B, C), dx1 = dt gate + davg / HW (one pass)."""

    def __init__(self, ch=256):
        super().__init__()
        self.channel_att = channel_att(ch)
        self.local_att = local_att(ch)

    accumulates, folds_pooled, reduction = False, False, 1       # several inputs: backward(dout) returns the list of their gradients

    def _pack(self, dev):
        la = self.local_att
        c, mip = la.F_h.out_channels, la.conv_1x1.out_channels
        mp = pad4(mip)
        wg = torch.cat([la.F_h.weight, la.F_w.weight]).detach().float()
        pk = dict(wg=pack_conv_weight(wg, cin_pad=mp).to(dev), we=self.channel_att.conv.weight.detach().float().reshape(-1).to(dev).contiguous())
        if not self.training:                                    # bn folded into conv_1x1
            w1, b1 = _fold_conv_bn(la.conv_1x1, la.bn)
            pk['w1'], pk['b1'] = pack_conv_weight(w1, cin_pad=c, cout_pad=mp).to(dev), torch.zeros(mp, device=dev)
            pk['b1'][:mip] = b1.to(dev)
            return pk
        w1 = la.conv_1x1.weight.detach().float()
        pk['w1'] = pack_conv_weight(w1, cin_pad=c, cout_pad=mp).to(dev)
        pk['wt1'] = pack_dgrad_weight(w1, cin_pad=c, cout_pad=mp).to(dev)
        pk['wtg'] = pack_dgrad_weight(wg, cin_pad=mp, cout_pad=2 * c).to(dev)
        pk['one'], pk['zero'] = torch.ones(2 * c, device=dev), torch.zeros(2 * c, device=dev)
        pk.update(_bn_vectors(la.bn, dev, mp))
        return pk

    def forward(self, xs):
        if len(xs) != 2:
            raise RuntimeError(f'attention_model takes two inputs, got {len(xs)}')
        x1, x2 = xs
        la = self.local_att
        c, mip = la.F_h.out_channels, la.conv_1x1.out_channels
        for a in xs:
            _asf_real(a, 'attention_model')
        if tuple(x1.shape[:3]) != tuple(x2.shape[:3]) or x1.c != x2.c:
            raise NotImplementedError(f'attention_model: inputs of unequal shape, {tuple(x1.shape[:3])} x {x1.c} and {tuple(x2.shape[:3])} x '
                                      f'{x2.c} (the reference adds them)')
        if x1.c != c:
            raise RuntimeError(f'attention_model({c}) got maps of {x1.c} channels')
        _asf_on_gpu(x1, 'attention_model')
        pk = self._packed(x1.t.device)
        B, H, W, _ = x1.shape
        mp = pad4(mip)
        avg, _ = ops.global_pool(x1.t, c, x1.coff, want_max=False)
        gate = ops.eca_gate(avg, pk['we'])
        t, pool = ops.asf_mix_means(x1.t, x2.t, gate, c, x1.coff, x2.coff)
        out = new_act(x1.t, H, W, c)
        if out.t.shape[3] != c:
            out.t.zero_()                                         # pad channels of a tensor of its own
        conv = dict(kh=1, kw=1, stride=1, pad=0)
        if not self.training:
            t1 = ops.conv2d_nhwc(pool, pk['w1'], pk['b1'], act='relu', cin=c, cout=mp, alg_cout=mip, **conv)
            g = ops.conv2d_nhwc(t1, pk['wg'], None, act='sigmoid', cin=mp, cout=2 * c, alg_cin=mip, **conv)
        else:
            y1 = ops.conv2d_nhwc(pool, pk['w1'], None, act='none', cin=c, cout=mp, alg_cout=mip, **conv)
            st, commit = _bn_train(la.bn, mp, y1, vec=pk)
            commit()
            t1 = ops.chan_affine_act(y1, mp, 0, st[2], st[3], 'relu', 0, torch.empty_like(y1))
            pre = ops.conv2d_nhwc(t1, pk['wg'], None, act='none', cin=mp, cout=2 * c, alg_cin=mip, **conv)
            g = ops.chan_affine_act(pre, 2 * c, 0, pk['one'], pk['zero'], 'sigmoid', 0, torch.empty_like(pre))
            self.__dict__['_ctx'] = (x1, avg, gate, t, pool, y1, st, t1, pre, g, pk)
        ops.coordatt_apply(t, (g, 0, 0), (g, c, H), c, out=out.t, o_coff=out.coff)
        return Act(out.t, out.coff, c)

    def backward(self, dout):
        x1, avg, gate, t, pool, y1, st, t1, pre, g, pk = self.__dict__.pop('_ctx')
        la = self.local_att
        c, mip = la.F_h.out_channels, la.conv_1x1.out_channels
        mp = pad4(mip)
        B, H, W, _ = x1.shape
        dev = x1.t.device
        conv = dict(kh=1, kw=1, stride=1, pad=0)
        a_h, a_w = (g, 0, 0), (g, c, H)
        dg = torch.zeros_like(g)                                  # the two quadrants nobody reads keep a zero gradient
        ops.coordatt_backward_gates(dout.t, t, a_h, a_w, c, dout.coff, 0, da_h=(dg, 0, 0), da_w=(dg, c, H))
        # through the sigmoid: a BatchNorm-activation backward with frozen unit statistics (F_h and F_w have no bias: its dbeta is dropped)
        ops.bn_act_backward(dg, 0, pre, 0, 2 * c, pk['zero'], pk['one'], pk['one'], pk['zero'], 'sigmoid', 0, False, dg, 0, None,
                            torch.zeros(2 * c, device=dev))
        dwg = ops.conv2d_wgrad_nhwc(t1, dg, cin=mp, cout=2 * c, **conv).view(2 * c, mp)[:, :mip]
        _acc_grad(la.F_h.weight, dwg[:c].reshape(c, mip, 1, 1))
        _acc_grad(la.F_w.weight, dwg[c:].reshape(c, mip, 1, 1))
        dt1 = ops.conv2d_dgrad_nhwc(dg, pk['wtg'], B=B, H=H + W, W=1, cin=mp, cout=2 * c, **conv)
        dy1 = _bn_backward(la.bn, dt1, 0, y1, st, 'relu', torch.empty_like(y1), mp)
        dw1 = ops.conv2d_wgrad_nhwc(pool, dy1, cin=c, cout=mp, **conv).view(mp, c)[:mip]
        _acc_grad(la.conv_1x1.weight, dw1.reshape(mip, c, 1, 1))
        dpool = ops.conv2d_dgrad_nhwc(dy1, pk['wt1'], B=B, H=H + W, W=1, cin=c, cout=mp, **conv)
        dt = torch.empty(B, H, W, pad4(c), device=dev, dtype=torch.float32)
        if pad4(c) != c:
            dt.zero_()
        ops.coordatt_backward_input(dout.t, a_h, a_w, (dpool, 0, 0), (dpool, 0, H), c, dout.coff, out=dt)
        ds = ops.asf_mix_backward_sums(dt, x1.t, c, 0, x1.coff)
        davg, dwe = ops.eca_gate_backward(avg, pk['we'], gate, ds)
        _acc_grad(self.channel_att.conv.weight, dwe.view(1, 1, -1))
        dx1 = torch.empty_like(dt)
        if pad4(c) != c:
            dx1.zero_()
        ops.asf_mix_backward_input(dt, gate, davg, c, out=dx1)
        return [Act(dx1, 0, c), Act(dt, 0, c)]                    # dx2 is dt itself


class ASPP(nn.Module):
    """cv2(cat(t, maxpool3(t), m_0(t), ..)), t = cv1(x) (models/common.py:1829-1843): atrous spatial pyramid pooling.  The m_i are bare 3x3
    nn.Conv2d(bias=False) of dilation = padding = (k_i - 1) // 2 (2, 4, 6 for the default k), no norm and no activation.  Nothing is
    concatenated: cv1 writes slice 0 of cv2's input buffer, the parallel-window pool kernel writes slice 1 (window 3, with codes in training)
    and each dilated conv its own slice.  Backward: cv2's data gradient, the pool's share and every dilated conv's data gradient added into
    slice 0 in place, then cv1."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        k = tuple(int(v) for v in k)
        if not k or any(v < 3 or v % 2 == 0 for v in k):
            raise NotImplementedError(f'ASPP rates from k={k}: odd k >= 3 only (dilation = padding = (k - 1) // 2 >= 1 keeps the map size)')
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=1, padding=1)      # parameter-free; kept for repr parity
        self.m = nn.ModuleList([nn.Conv2d(c_, c_, kernel_size=3, stride=1, padding=(x - 1) // 2, dilation=(x - 1) // 2, bias=False) for x in k])
        self.cv2 = Conv(c_ * (len(k) + 2), c2, 1, 1)

    accumulates, folds_pooled, reduction = False, False, 1

    def _packed_m(self, dev):
        """Per dilated conv (forward packing, data-gradient packing), rebuilt when a weight changed (in training: every forward)."""
        key = (dev, tuple(m.weight._version for m in self.m))
        cache = self.__dict__.get('_pk')
        if self.training or cache is None or cache[0] != key:
            with torch.no_grad():
                ws = [m.weight.detach().float() for m in self.m]
                cache = (key, [(pack_conv_weight(w).to(dev), pack_dgrad_weight(w).to(dev) if self.training else None) for w in ws])
            self.__dict__['_pk'] = cache
        return cache[1]

    def invalidate(self):
        self.__dict__.pop('_pk', None)

    def forward(self, x):
        c_, n = self.cv1.conv.out_channels, len(self.m)
        if c_ % 4:
            raise NotImplementedError('ASPP hidden width must be a multiple of 4 on the MI355X path')
        B, H, W, _ = x.shape
        cat = concat_act(x.t, H, W, (n + 2) * c_)
        self.cv1(x, out=cat.slice(0, c_))
        codes = ops.spp_pool_(cat.t, c_, (3,), 0, codes=self.training)
        pk = self._packed_m(x.t.device)
        for i, (m, (wp, _)) in enumerate(zip(self.m, pk)):
            ops.conv2d_nhwc(cat.t, wp, None, kh=3, kw=3, stride=1, pad=m.padding[0], dil=m.dilation[0], act='none', cin=c_, x_coff=0,
                            out=cat.t, cout=c_, y_coff=(2 + i) * c_)
        if self.training:
            self.__dict__['_ctx'] = (cat, codes[1], pk)
        return self.cv2(cat)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        cat, codes, pk = self.__dict__.pop('_ctx')
        c_ = self.cv1.conv.out_channels
        dcat = self.cv2.backward(dout)
        ops.spp_pool_backward_(dcat.t, codes, c_, (3,), dcat.coff)
        d0 = dcat.slice(0, c_)
        for i, (m, (_, wt)) in enumerate(zip(self.m, pk)):
            _plain_conv_backward(m, cat.slice(0, c_), dcat.t, wt, dy_coff=dcat.coff + (2 + i) * c_, dx_out=d0, accumulate=True)
        return self.cv1.backward(d0, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class DWR(nn.Module):
    """Dilation-wise residual (models/common.py:7431-7447): conv_1x1(cat(d1(t), d3(t), d5(t))) + x with t = conv_3x3(x); the branches are 3x3
    Convs of dilation 1, 3 and 5 and dim, dim / 2, dim / 2 channels.  The branches write the three slices of one 2 * dim buffer, the
    residual rides conv_1x1's output pass.  Backward: the branches' data gradients are summed into one tensor by `accumulate`, and x's own
    share (the residual) joins conv_3x3's data-gradient epilogue."""

    def __init__(self, dim):
        super().__init__()
        self.conv_3x3 = Conv(dim, dim // 2, 3)
        self.conv_3x3_d1 = Conv(dim // 2, dim, 3, d=1)
        self.conv_3x3_d3 = Conv(dim // 2, dim // 2, 3, d=3)
        self.conv_3x3_d5 = Conv(dim // 2, dim // 2, 3, d=5)
        self.conv_1x1 = Conv(dim * 2, dim, k=1)

    accumulates, folds_pooled, reduction = False, False, 1

    def _branches(self):
        dim = self.conv_1x1.conv.out_channels
        return ((self.conv_3x3_d1, 0, dim), (self.conv_3x3_d3, dim, dim // 2), (self.conv_3x3_d5, dim + dim // 2, dim // 2))

    def forward(self, x, out=None):
        dim = self.conv_1x1.conv.out_channels
        if dim % 8:
            raise NotImplementedError('DWR width must be a multiple of 8 on the MI355X path (its branches write slices of dim / 2 channels)')
        B, H, W, _ = x.shape
        t = self.conv_3x3(x)
        cat = concat_act(x.t, H, W, 2 * dim)
        for blk, off, c in self._branches():
            blk(t, out=cat.slice(off, c))
        return self.conv_1x1(cat, out=out, residual=x)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        dim = self.conv_1x1.conv.out_channels
        dcat = self.conv_1x1.backward(dout)
        dt = None
        for blk, off, c in self._branches():
            dt = blk.backward(dcat.slice(off, c), dx_out=dt, accumulate=dt is not None)
        fuse = dout.coff % 4 == 0                                 # dim % 8 == 0: the residual's gradient rides the dgrad epilogue
        dx = self.conv_3x3.backward(dt, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, dim)
        return dx


class DWRSeg_Conv(_Packed):
    """gelu(bn(DWR(conv(x)))) with a 1x1 Conv (models/common.py:7450-7466; kernel_size, stride, groups and dilation are accepted and unused, as in
    the reference, whose DWR child is called `dcnv3`).  Eval: the BatchNorm's running statistics and the GELU are one pass over DWR's output;
    training: the one BatchNorm train path, GELU after the normalisation (order 0)."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, groups=1, dilation=1):
        super().__init__()
        self.conv = Conv(in_channels, out_channels, k=1)
        self.dcnv3 = DWR(out_channels)
        self.bn = nn.BatchNorm2d(out_channels)
        self.gelu = nn.GELU()

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack_params(self):
        return self.bn.parameters()                               # the children pack themselves

    def _pack(self, dev):
        return tuple(v.detach().float().contiguous().to(dev) for v in bn_fold(self.bn))

    def forward(self, x, out=None, residual=None):
        c = self.bn.num_features
        u = self.dcnv3(self.conv(x))                              # a whole tensor of its own, c % 8 == 0
        if out is None:
            out = new_act(x.t, u.shape[1], u.shape[2], c)
        res = dict(residual=None if residual is None else residual.t, res_coff=0 if residual is None else residual.coff)
        if not self.training:
            s, t = self._packed(u.t.device)
            ops.chan_affine_act(u.t, c, u.coff, s, t, 'gelu', 0, out.t, out.coff, **res)
            return Act(out.t, out.coff, c)
        st, commit = _bn_train(self.bn, c, u.t, coff=u.coff)
        commit()
        ops.chan_affine_act(u.t, c, u.coff, st[2], st[3], 'gelu', 0, out.t, out.coff, **res)
        self.__dict__['_ctx'] = (u, st)
        return Act(out.t, out.coff, c)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        u, st = self.__dict__.pop('_ctx')
        c = self.bn.num_features
        du = _bn_backward(self.bn, dout.t, dout.coff, u.t, st, 'gelu', torch.empty_like(u.t), c, coff=u.coff, order=0)
        d = self.dcnv3.backward(Act(du, u.coff, c))
        return self.conv.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx)


class Bottleneck_DWRSeg(nn.Module):
    """cv1 (k[0] Conv) -> DWRSeg_Conv (+x) (models/common.py:7469-7484); the shortcut rides the GELU pass (forward) and cv1's dgrad epilogue
    (backward)."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = DWRSeg_Conv(c_, c2, k[1], 1, groups=g)
        self.add = shortcut and c1 == c2

    accumulates, folds_pooled, reduction = False, False, 1

    def forward(self, x, out=None):
        return self.cv2(self.cv1(x), out=out, residual=x if self.add else None)

    def backward(self, dout, dx_out=None, accumulate=False, need_dx=True):
        d = self.cv2.backward(dout)
        c1 = self.cv1.conv.in_channels
        fuse = self.add and pad4(c1) == c1 and dout.coff % 4 == 0
        dx = self.cv1.backward(d, dx_out=dx_out, accumulate=accumulate, need_dx=need_dx, also_add=dout if fuse else None)
        if self.add and not fuse and dx is not None:
            ops.add_(dx.t, dx.coff, dout.t, dout.coff, c1)
        return dx


class C2f_DWR(C2f):
    """C2f whose blocks are Bottleneck_DWRSeg(c, c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) (models/common.py:7487-7511): C2f's slice scheme."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(Bottleneck_DWRSeg(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    accumulates, folds_pooled, reduction = False, False, 1       # C2f's backward, dx_out / accumulate included; the walk adds its gradient itself


class Concat(nn.Module):
    """torch.cat(x, 1) (models/common.py:2085-2097) of NHWC channel slices; an input that is a 2x nearest-upsampled view
    (`Upsample` only sets a flag) is expanded by the same copy.  Backward hands out slices of the incoming gradient (no copy) and
    block-sums the slice of an upsampled input."""

    def __init__(self, dimension=1):
        super().__init__()
        if dimension != 1:
            raise NotImplementedError('channel concatenation only')
        self.d = dimension

    accumulates, folds_pooled, reduction = False, False, 1       # several inputs: backward(dout) returns the list of their gradients

    def forward(self, xs):
        B, H, W = xs[0].shape[0], xs[0].shape[1] << xs[0].up, xs[0].shape[2] << xs[0].up
        for a in xs:
            if a.c % 4 or a.coff % 4:
                raise NotImplementedError('Concat inputs must be channel slices with offsets and widths that are multiples of 4')
            if (a.shape[0], a.shape[1] << a.up, a.shape[2] << a.up) != (B, H, W):
                raise RuntimeError(f'Sizes of tensors must match except in dimension 1. Got {[tuple(v.shape) for v in xs]}')
        out = concat_act(xs[0].t, H, W, sum(a.c for a in xs))
        off = 0
        for a in xs:
            ops.resample_slice(a.t, a.coff, out.t, off, a.c, up=a.up)
            off += a.c
        if self.training:
            self.__dict__['_ctx'] = [(a.c, a.up, a.shape) for a in xs]
        return out

    def backward(self, dout):
        ctx = self.__dict__.pop('_ctx')
        outs, off = [], 0
        for c, up, shp in ctx:
            if up == 0:
                outs.append(dout.slice(off, c))
            else:
                lo = torch.empty(shp[0], shp[1], shp[2], c, device=dout.t.device, dtype=torch.float32)
                ops.resample_slice(dout.t, dout.coff + off, lo, 0, c, up=up, reduce=True)
                outs.append(Act(lo, 0, c))
            off += c
        return outs


class Detect(nn.Module):
    """The stock anchor head (models/yolo.py:46-109): one 1x1 conv (+bias) per level, the view/permute and the eval decode in one
    kernel.  forward returns (z, [raw_i]) in eval and [raw_i] in training like the reference; raw_i is (B,na,ny,nx,no)."""
    stride = None
    accumulates, folds_pooled, reduction = False, False, 1       # the head: backward(draws) returns the list of its inputs' gradients

    def __init__(self, nc=80, anchors=(), ch=(), inplace=True):
        super().__init__()
        self.nc, self.no = nc, nc + 5
        self.nl, self.na = len(anchors), len(anchors[0]) // 2
        self.register_buffer('anchors', torch.tensor(anchors).float().view(self.nl, -1, 2))
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)
        self.inplace = inplace
        self.__dict__['_runners'] = [PlainConv(m) for m in self.m]      # share the parameters, stay out of state_dict

    def invalidate(self):
        self.__dict__.pop('_anchors_host', None)
        for r in self._runners:
            r.invalidate()

    def forward(self, xs):
        B, dev = xs[0].shape[0], xs[0].t.device
        total = sum(self.na * a.shape[1] * a.shape[2] for a in xs)
        z = None if self.training else torch.empty(B, total, self.no, device=dev, dtype=torch.float32)
        anchors = self.__dict__.get('_anchors_host')
        if anchors is None:                                   # cached host copy: no device sync per forward
            anchors = self.__dict__['_anchors_host'] = self.anchors.detach().float().cpu()
        raws, row, widths = [], 0, []
        for i, run in enumerate(self._runners):
            run.conv = self.m[i]                                 # _initialize_biases replaces the bias Parameter, the module stays
            run.train(self.training)
            t = run(xs[i])
            _, ny, nx, cs = t.shape
            raw = torch.empty(B, self.na, ny, nx, self.no, device=dev, dtype=torch.float32)
            stride = float(self.stride[i])
            ops.detect_plain_decode(t.t, (anchors[i] * stride).flatten().tolist(), stride, self.na, self.nc, raw=raw, z=z, total=total,
                                    row_off=row)
            raws.append(raw)
            widths.append(cs)
            row += self.na * ny * nx
        if self.training:
            self.__dict__['_ctx'] = widths
        return raws if self.training else (z, raws)

    def backward(self, draws):
        widths = self.__dict__.pop('_ctx')
        return [run.backward(ops.detect_plain_raw_backward(draws[i].contiguous(), widths[i], self.na, self.nc))
                for i, run in enumerate(self._runners)]


# ================================================================================================ ASFF head
class ConvBNLeaky(Conv):
    """add_conv (models/common.py:5322-5343): Conv2d(bias=False, pad (k - 1) // 2) -> BatchNorm2d -> LeakyReLU(0.1), with the reference's child names
    (`conv`, `batch_norm`, `leaky`) so its state dicts load.  Everything else is Conv: eval with the BatchNorm folded and the activation in the
    conv epilogue, training through Conv's one BatchNorm path, the packed weight master of the optimizer."""

    def __init__(self, in_ch, out_ch, ksize, stride, leaky=True):
        nn.Module.__init__(self)
        if not leaky:
            raise NotImplementedError('add_conv(leaky=False) (ReLU6) is not on the SOMI path (LeakyReLU(0.1) only)')
        if ksize not in (1, 3) or stride not in (1, 2):
            raise NotImplementedError(f'add_conv with ksize={ksize}, stride={stride} is not on the SOMI path (ksize 1 or 3, stride 1 or 2)')
        self.conv = nn.Conv2d(in_ch, out_ch, ksize, stride, (ksize - 1) // 2, bias=False)
        self.batch_norm = nn.BatchNorm2d(out_ch)
        self.leaky = nn.LeakyReLU(0.1)

    bn = property(lambda self: self.batch_norm)                   # the names Conv's code reads
    act = property(lambda self: self.leaky)
    # never a layer of the parsed graph (it lives inside ASFF, which calls backward(dx_out=, accumulate=) itself): what the graph walk reads is off
    accumulates = folds_pooled = False


def add_conv(in_ch, out_ch, ksize, stride, leaky=True):
    return ConvBNLeaky(in_ch, out_ch, ksize, stride, leaky)


class MaxPool3s2(nn.Module):
    """F.max_pool2d(x, 3, stride=2, padding=1) (models/common.py:5536), the pad an implicit -inf.  No parameters; ASFF keeps it out of its state dict."""

    def forward(self, x):
        if x.c % 4 or x.up:
            raise NotImplementedError('max_pool2d(3, 2, 1) needs a real tensor with a channel count that is a multiple of 4')
        B, H, W, _ = x.shape
        out = new_act(x.t, ops.maxpool3s2_out_size(H), ops.maxpool3s2_out_size(W), x.c)
        r = ops.maxpool3s2(x.t, x.c, x.coff, out=out.t, codes=self.training)
        if self.training:
            self.__dict__['_ctx'] = (r[1], H, W, x.c)
        return out

    def backward(self, dout, dx_out=None, accumulate=False):
        codes, H, W, c = self.__dict__.pop('_ctx')
        if dx_out is not None and not accumulate:
            ops.maxpool3s2_backward(dout.t, codes, c, H, W, dout.coff, out=dx_out.t, dx_coff=dx_out.coff)
            return dx_out
        dx = Act(ops.maxpool3s2_backward(dout.t, codes, c, H, W, dout.coff), 0, c)
        if dx_out is None:
            return dx
        ops.add_(dx_out.t, dx_out.coff, dx.t, 0, c)
        return dx_out


class ASFF(nn.Module):
    """Adaptive spatial feature fusion at one level (models/common.py:5500-5567): the three pyramid maps are brought to this level's width and size
    (x0 = P5, x1 = P4, x2 = P3: a 3x3 stride-2 conv down, max_pool2d(3, 2, 1) + conv two levels down, a 1x1 conv + nearest upsampling up), three
    1x1 convs make 16-channel weight maps of them, a 48 -> 3 1x1 conv and a softmax turn those into per-pixel weights, and the weighted sum goes
    through a 3x3 `expand` conv.  Here a 1x1-compressed map stays at its LOW resolution: the fusion kernels (ops.asff_fuse) read it, and its
    weight map, at (h >> up, w >> up), so neither the upsampled maps, nor the concat, nor the softmax's logits, nor the products reach memory.
    `weight_level_i` of an upsampled map runs at the low resolution too - a 1x1 conv commutes with nearest upsampling, the batch mean and the
    biased variance are the same over the replicated pixels, the gradient of a low-resolution element is the sum over its children (formed in
    the fusion backward) - and only the running variance's unbiased correction n / (n - 1) has to use the high-resolution pixel count."""
    DIM = (512, 256, 128)

    def __init__(self, level, rfb=False, vis=False):
        super().__init__()
        if rfb:
            raise NotImplementedError('ASFF(rfb=True) (8-channel weight maps) is not on the SOMI path: the fusion kernels take 16-channel weight maps')
        if vis:
            raise NotImplementedError('ASFF(vis=True) (returning the weights and the channel sum) is not on the SOMI path: the weights stay in the kernel')
        if level not in (0, 1, 2):
            raise NotImplementedError(f'ASFF level {level}: three levels only')
        self.level = level
        self.dim = list(self.DIM)
        self.inter_dim = self.dim[level]
        if level == 0:
            self.stride_level_1 = add_conv(256, self.inter_dim, 3, 2)
            self.stride_level_2 = add_conv(128, self.inter_dim, 3, 2)
            self.expand = add_conv(self.inter_dim, 512, 3, 1)
        elif level == 1:
            self.compress_level_0 = add_conv(512, self.inter_dim, 1, 1)
            self.stride_level_2 = add_conv(128, self.inter_dim, 3, 2)
            self.expand = add_conv(self.inter_dim, 256, 3, 1)
        else:
            self.compress_level_0 = add_conv(512, self.inter_dim, 1, 1)
            self.compress_level_1 = add_conv(256, self.inter_dim, 1, 1)
            self.expand = add_conv(self.inter_dim, 128, 3, 1)
        compress_c = 16
        self.weight_level_0 = add_conv(self.inter_dim, compress_c, 1, 1)
        self.weight_level_1 = add_conv(self.inter_dim, compress_c, 1, 1)
        self.weight_level_2 = add_conv(self.inter_dim, compress_c, 1, 1)
        self.weight_levels = nn.Conv2d(compress_c * 3, 3, kernel_size=1, stride=1, padding=0)
        self.vis = vis
        self.__dict__['_pool'] = MaxPool3s2()                     # parameter-free, outside the state dict

    accumulates, folds_pooled, reduction = False, False, 1       # three inputs: backward(dout) returns the list of their gradients

    def invalidate(self):
        for m in self.children():
            if hasattr(m, 'invalidate'):
                m.invalidate()

    def _resizers(self):
        """Per input: (the modules that bring it to this level - None: the input itself -, the factor log2 it is read at)."""
        if self.level == 0:
            return [(None, 0), ((self.stride_level_1,), 0), ((self._pool, self.stride_level_2), 0)]
        if self.level == 1:
            return [((self.compress_level_0,), 1), (None, 0), ((self.stride_level_2,), 0)]
        return [((self.compress_level_0,), 2), ((self.compress_level_1,), 1), (None, 0)]

    def _weight_map(self, conv, r, up):
        """weight_level_i at the resolution `r` is stored at; in training the running variance gets the unbiased correction of the replicated map."""
        v = conv(r)
        if self.training and up:
            bn, rstd = conv.bn, conv.__dict__['_ctx'][3]
            world = ops.SYNC_BN.get_world_size(ops.SYNC_BN_GROUP) if ops.SYNC_BN is not None else 1
            nl = v.shape[0] * v.shape[1] * v.shape[2] * world
            nh = nl << (2 * up)
            with torch.no_grad():                                 # the kernel used nl / (nl - 1); var_biased = 1 / rstd^2 - eps
                bn.running_var.add_((1.0 / (rstd[:bn.num_features] * rstd[:bn.num_features]) - bn.eps) *
                                    (bn.momentum * (nh / (nh - 1) - (nl / (nl - 1) if nl > 1 else 1.0))))
        return v

    def forward(self, x_level_0, x_level_1, x_level_2):
        xs = (x_level_0, x_level_1, x_level_2)
        w, b = self.weight_levels.weight.detach(), self.weight_levels.bias.detach()
        if not w.is_cuda:
            raise RuntimeError('somi_amd ASFF runs on the MI355X only (no CPU fallback)')
        self._pool.train(self.training)
        rs, ups = [], []
        for x, c, (mods, up) in zip(xs, self.dim, self._resizers()):
            if x.up or x.c != c:
                raise RuntimeError(f'ASFF level {self.level}: the inputs are real maps of {self.dim} channels (P5, P4, P3), got {x.c} (up={x.up})')
            for m in mods or ():
                x = m(x)
            rs.append(x)
            ups.append(up)
        vs = [self._weight_map(conv, r, up) for conv, r, up in zip((self.weight_level_0, self.weight_level_1, self.weight_level_2), rs, ups)]
        B, H, W = rs[0].shape[0], rs[0].shape[1] << ups[0], rs[0].shape[2] << ups[0]
        fused = new_act(rs[0].t, H, W, self.inter_dim)
        r = ops.asff_fuse([(a.t, a.coff) for a in rs], [(a.t, a.coff) for a in vs], ups, ups, w.view(3, 48), b, self.inter_dim, out=fused.t,
                          weights=self.training)
        if self.training:
            self.__dict__['_ctx'] = (rs, vs, ups, r[1])
        return self.expand(fused)

    def backward(self, dout, dx_out=None, accumulate=False):
        """-> the gradients of (x_level_0, x_level_1, x_level_2).  dx_out: three entries, each None (a tensor of its own) or a whole padded contiguous
        Act the gradient is written into, or added to with `accumulate`."""
        rs, vs, ups, p = self.__dict__.pop('_ctx')
        dx_out = (None, None, None) if dx_out is None else dx_out
        dfused = self.expand.backward(dout)
        res = self._resizers()
        direct = [mods is None for mods, _ in res]
        # the source that IS an input takes its gradient straight in the caller's tensor; the others get low-resolution tensors of their own
        drs = [(dx_out[i].t, dx_out[i].coff) if direct[i] and dx_out[i] is not None else None for i in range(3)]
        (dw, db), fin = _grad_targets(self.weight_levels.weight, self.weight_levels.bias)
        drt, dvt = ops.asff_fuse_backward(dfused.t, [(a.t, a.coff) for a in rs], [(a.t, a.coff) for a in vs], ups, ups,
                                          self.weight_levels.weight.detach().view(3, 48), self.weight_levels.bias.detach(), p, self.inter_dim,
                                          dw.view(3, 48), db, do_coff=dfused.coff, drs=drs,
                                          accumulate=[accumulate and d is not None for d in drs])
        fin()
        outs = []
        for i, conv in enumerate((self.weight_level_0, self.weight_level_1, self.weight_level_2)):
            dr = Act(drt[i], drs[i][1] if drs[i] is not None else 0, self.inter_dim)
            conv.backward(Act(dvt[i], 0, 16), dx_out=dr, accumulate=True)       # the weight map's share joins the source's gradient
            mods = res[i][0]
            if mods is None:
                outs.append(dr)
                continue
            for m in reversed(mods[1:]):
                dr = m.backward(dr)
            outs.append(mods[0].backward(dr, dx_out=dx_out[i], accumulate=accumulate and dx_out[i] is not None))
        return outs


class ASFF_Detect(Detect):
    """The stock anchor head behind three ASFF blocks (models/yolo.py:172-184).  The reference rewrites its input list in place while it walks it, so
    with x = [P5, P4, P3]:  f0 = asff0(P5, P4, P3),  f1 = asff1(f0, P4, P3),  f2 = asff2(f0, f1, P3)  - later levels fuse the already fused coarser
    maps - and Detect runs on [f2, f1, f0].  Reproduced as it is.  backward runs the chain in reverse: every ASFF adds its input gradients into the
    tensors the later consumers already wrote."""

    def __init__(self, nc=80, anchors=(), ch=(), inplace=False):
        if len(ch) != 3 or tuple(ch) != (128, 256, 512):
            raise NotImplementedError(f'ASFF_Detect is built for three levels of (128, 256, 512) channels - the reference hard-codes ASFF.dim = '
                                      f'[512, 256, 128] (yolov5s width) - got {len(ch)} levels of {tuple(ch)} channels')
        super().__init__(nc, anchors, ch, inplace)
        if self.nl != 3:
            raise NotImplementedError(f'ASFF_Detect is built for three levels of (128, 256, 512) channels, got {self.nl} anchor rows')
        self.asffs = nn.ModuleList(ASFF(i) for i in range(self.nl))

    def invalidate(self):
        super().invalidate()
        for m in self.asffs.modules():
            if m is not self.asffs and hasattr(m, 'invalidate'):
                m.invalidate()

    def forward(self, xs):
        x = list(xs)[::-1]
        for i in range(self.nl):
            x[i] = self.asffs[i](*x)
        return super().forward(x[::-1])

    def backward(self, draws):
        d2, d1, d0 = super().backward(draws)                      # the gradients of f2, f1, f0: whole tensors of their own
        _, _, dp3 = self.asffs[2].backward(d2, dx_out=(d0, d1, None), accumulate=True)
        _, dp4, _ = self.asffs[1].backward(d1, dx_out=(d0, None, dp3), accumulate=True)
        dp5, _, _ = self.asffs[0].backward(d0, dx_out=(None, dp4, dp3), accumulate=True)
        return [dp3, dp4, dp5]


# ================================================================================================ DCNv3 wired into a graph
class DCNv3_YOLO(_Packed):
    """NHWC DCNv3 layer (models/ops_dcnv3/modules/dcnv3.py:222-379) -> BatchNorm2d -> SiLU, channel-preserving: the build's wiring
    of the reference's deformable-conv layer into the YOLO graph (the reference wires it into no model).  The
    activations are already NHWC on this path, so the NCHW<->NHWC permutes of an NCHW graph do not exist.  Eval: BN is folded into
    the layer's output projection (+SiLU in that conv's epilogue): no pass of its own.  Train: the DCNv3 module's hand-written
    backward (somi_amd.dcnv3.DCNv3._backward_impl) is chained with the BN / SiLU backward kernel."""

    def __init__(self, c, k=3, s=1, g=4, offset_scale=1.0, center_feature_scale=False):
        super().__init__()
        from .dcnv3 import DCNv3
        if s != 1:
            raise NotImplementedError('DCNv3_YOLO is wired with stride 1')
        self.dcnv3 = DCNv3(c, kernel_size=k, stride=s, pad=k // 2, group=g, offset_scale=offset_scale,
                           center_feature_scale=center_feature_scale)
        self.bn = nn.BatchNorm2d(c)
        self.act = nn.SiLU()

    accumulates, folds_pooled, reduction = False, False, 1

    def _pack(self, dev):
        """eval: output projection with the BatchNorm folded in (W' = diag(s) W, b' = s b + t)."""
        s_, t_ = bn_fold(self.bn)
        w = (self.dcnv3.output_proj.weight.detach().float() * s_[:, None]).contiguous().to(dev)
        b = (self.dcnv3.output_proj.bias.detach().float() * s_ + t_).contiguous().to(dev)
        return w, b

    def forward(self, x):
        c = self.bn.num_features
        if x.coff != 0 or x.t.shape[3] != c or x.c != c or c % 4:
            raise NotImplementedError('DCNv3_YOLO input must be a whole tensor with channels a multiple of 4')
        if not self.training:
            w, b = self._packed(x.t.device)
            return Act(self.dcnv3._forward_impl(x.t, out_proj=(w, b, _act_name(self.act))), 0, c)
        self.invalidate()
        vec = _bn_clones(self.bn)
        sd = {'pivot': vec['rm']} if x.t.numel() * 4 <= 0xE0000000 else None
        u, saved = self.dcnv3._forward_impl(x.t, keep=True, bn_stats=sd)
        # when the output projection's epilogue left the partial sums: no extra read of u
        st, commit = _bn_train(self.bn, c, u, partials=sd if sd is not None and 'part' in sd else None, npix=u.numel() // c, vec=vec)
        commit()
        out = ops.chan_affine_act(u, c, 0, st[2], st[3], _act_name(self.act), 0, torch.empty_like(u))
        self.__dict__['_ctx'] = (u, st, saved)
        return Act(out, 0, c)

    def backward(self, dz, dx_out=None, accumulate=False, need_dx=True):
        if dx_out is not None or accumulate:
            raise NotImplementedError('DCNv3_YOLO writes its own input gradient')
        u, st, saved = self.__dict__.pop('_ctx')
        c = self.bn.num_features
        du = _bn_backward(self.bn, dz.t, dz.coff, u, st, _act_name(self.act), torch.empty_like(u), c)
        dinput, grads = self.dcnv3._backward_impl(saved, du)
        for p_, g_ in zip(self.dcnv3._params(), grads):
            _acc_grad(p_, g_.view_as(p_) if g_.numel() == p_.numel() else g_[:p_.shape[0]])
        return Act(dinput, 0, c) if need_dx else None
