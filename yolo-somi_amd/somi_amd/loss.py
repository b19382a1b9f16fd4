"""`ComputeLoss` with the reference's interface (utils/loss.py:112-208) on top of somi_yolo_loss_f32.

`ComputeLoss(model)(p, targets) -> (loss[1], loss_items[3] detached)`; p is the list of (B,na,ny,nx,no) training
outputs, targets (nt,6) = [image, class, x, y, w, h] normalised.  The loss value and d loss / d p come out of the same
fused launches; autograd sees one node.  hyp keys read: cls_pw, obj_pw, fl_gamma, slide_ratio, nwdloss, shapeloss, box, obj, cls,
anchor_t (+label_smoothing) - the ones the reference's __init__ / __call__ read.  FocalLoss (fl_gamma > 0), SlideLoss (slide_ratio > 0)
and the NWD box term (nwdloss > 0; constant 12.8, or 2.5 under shapeloss > 0) run inside the same kernels; autobalance is host state
(the balance list, updated from the per-level objectness means the launch reports) as in the reference.

The box rule: the reference scores a matched box with `bbox_iou(pbox.T, tbox[i], x1y1x2y2=False, CIoU=True)` (utils/loss.py:161) and ships a
family of other terms for that line (utils/metrics.py:397-702).  `ComputeLoss(model, iou=...)` selects which of those calls stands there
(`box_rule` below has the table and what is refused); the default is the reference's line and runs the kernels it always ran.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import LossBoxRule, LossDesc, LossLevel, check
from .ops import _ptr, _stream


def smooth_BCE(eps=0.1):
    """utils/loss.py:14-15."""
    return 1.0 - 0.5 * eps, 0.5 * eps


IOU_KINDS = {'IoU': 0, 'GIoU': 1, 'DIoU': 2, 'CIoU': 3, 'EIoU': 4, 'SIoU': 5, 'EfficiCIoU': 6, 'WIoU': 7, 'shape': 8}   # enum somi_loss_iou_kind
_FOCAL_OK = ('IoU', 'GIoU', 'DIoU', 'CIoU', 'EIoU')
_INNER_OK = _FOCAL_OK + ('SIoU',)
WIOU_MOMENTUM = 1 - 0.5 ** (1 / 7000)                             # WIoU_Scale._momentum (utils/metrics.py:452)


# Every rule setting the fixture of tests/golden/iou_loss.npz pins and tools/loss_bench.py times: tag -> ComputeLoss keywords
RULE_SETTINGS = {
    'IoU': dict(iou='IoU'), 'GIoU': dict(iou='GIoU'), 'DIoU': dict(iou='DIoU'), 'CIoU': dict(iou='CIoU'), 'EIoU': dict(iou='EIoU'),
    'SIoU': dict(iou='SIoU'), 'EfficiCIoU': dict(iou='EfficiCIoU'), 'WIoU': dict(iou='WIoU'), 'WIoU_scaled': dict(iou='WIoU', wiou_scale=True),
    'shape': dict(iou='shape'), 'shape_s0': dict(iou='shape', shape_scale=0.0),
    'CIoU_focal': dict(iou='CIoU', focal=True), 'EIoU_focal': dict(iou='EIoU', focal=True),
    'CIoU_a3': dict(iou='CIoU', alpha=3.0), 'GIoU_a3': dict(iou='GIoU', alpha=3.0), 'SIoU_a3': dict(iou='SIoU', alpha=3.0),
    'CIoU_in0.7': dict(iou='CIoU', inner_ratio=0.7), 'SIoU_in0.7': dict(iou='SIoU', inner_ratio=0.7), 'IoU_in1.25': dict(iou='IoU', inner_ratio=1.25),
}


def box_rule(iou='CIoU', focal=False, alpha=1.0, gamma=0.5, inner_ratio=None, shape_scale=0.5, wiou_scale=False):
    """The reference call that scores a matched box, as a LossBoxRule (without the WIoU state), or ValueError.

      iou                                       call (utils/metrics.py)                                             keywords it takes
      'IoU' 'GIoU' 'DIoU' 'CIoU' 'EIoU'         bbox_iou(pbox.T, tbox, x1y1x2y2=False, <flag>, Focal, alpha, gamma)   focal, alpha >= 1, gamma | inner_ratio
      'SIoU'                                    the same with SIoU=True                                             alpha | inner_ratio
      'EfficiCIoU'                              the same with EfficiCIoU=True (:519-527)                            -
      'WIoU'                                    bbox_iou(..., WIoU=True, scale=wiou_scale) (:560-569)               wiou_scale
      'shape'                                   shape_iou(pbox.T, tbox, scale1=shape_scale) (:397-439)              shape_scale
    inner_ratio=r: bbox_inner_iou(pbox, tbox, xywh=True, <flag>, ratio=r) (:604-702) instead.
    A tensor result r gives the box term mean(1 - r) and the similarity s = r; a pair (r0, r1) gives mean(r1.detach() * (1 - r0)), s = r0;
    scaled WIoU's triple gives mean(r0 * r1), s = r2.  s.detach() is what utils/loss.py:169,172 call `iou`."""
    if iou not in IOU_KINDS:
        raise ValueError(f'unknown box rule iou={iou!r}: one of {sorted(IOU_KINDS)}')
    if not float(alpha) >= 1.0:
        raise ValueError(f'alpha={alpha!r}: alpha < 1 is not built (the power of a vanishing IoU has no bounded gradient)')
    if focal and iou == 'SIoU':
        raise ValueError("focal with iou='SIoU': the reference's Focal exponent there is its own angle-cost tensor by a name clash "
                         "(utils/metrics.py:550,556), which is not reproduced")
    if focal and iou not in _FOCAL_OK:
        raise ValueError(f'focal with iou={iou!r}: the reference has no Focal form of this rule')
    if float(alpha) != 1.0 and iou not in _INNER_OK:
        raise ValueError(f'alpha={alpha!r} with iou={iou!r}: this rule takes no alpha')
    if inner_ratio is not None:
        if iou not in _INNER_OK:
            raise ValueError(f'inner_ratio with iou={iou!r}: bbox_inner_iou has no such form')
        if focal or float(alpha) != 1.0:
            raise ValueError('inner_ratio together with focal or alpha != 1: bbox_inner_iou takes neither')
        if not float(inner_ratio) > 0.0:
            raise ValueError(f'inner_ratio={inner_ratio!r} has to be positive')
    if wiou_scale and iou != 'WIoU':
        raise ValueError(f'wiou_scale with iou={iou!r}: only WIoU has the scaled form')
    if focal and not float(gamma) >= 0.0:
        raise ValueError(f'gamma={gamma!r} < 0')
    r = LossBoxRule()
    r.kind, r.focal, r.inner, r.wiou_scaled = IOU_KINDS[iou], int(bool(focal)), int(inner_ratio is not None), int(bool(wiou_scale))
    r.alpha, r.gamma, r.inner_ratio, r.shape_scale = float(alpha), float(gamma), float(inner_ratio or 0.0), float(shape_scale)
    return r


class _AttachGrad(torch.autograd.Function):
    """Makes the pre-computed d loss / d p an autograd edge from the loss to the prediction tensors."""

    @staticmethod
    def forward(ctx, loss, grads, *p):
        ctx.grads = grads
        return loss.clone()

    @staticmethod
    def backward(ctx, go):
        return (None, None) + tuple(g * go for g in ctx.grads)


class ComputeLoss:
    def __init__(self, model, autobalance=False, iou='CIoU', focal=False, alpha=1.0, gamma=0.5, inner_ratio=None, shape_scale=0.5,
                 wiou_scale=False):
        self.rule = box_rule(iou, focal, alpha, gamma, inner_ratio, shape_scale, wiou_scale)      # ValueError before anything is launched
        self._default_rule = iou == 'CIoU' and not focal and inner_ratio is None and float(alpha) == 1.0
        # WIoU_Scale's class state (utils/metrics.py:450-453) as state of this criterion, on the device: only scaled WIoU reads or writes it
        self.wiou_mean = torch.ones(1, dtype=torch.float64, device=model.model[-1].anchors.device)
        self.wiou_train = True
        self.sort_obj_iou = False
        h = model.hyp
        det = model.model[-1]
        self.cp, self.cn = smooth_BCE(eps=h.get('label_smoothing', 0.0))
        self.balance = {3: [4.0, 1.0, 0.4]}.get(det.nl, [4.0, 1.0, 0.25, 0.06, 0.02])       # utils/loss.py:135
        self.gr, self.hyp, self.autobalance = 1.0, h, autobalance
        self.ssi = list(det.stride).index(16) if autobalance else 0                           # stride 16 index (:137)
        self.na, self.nc, self.nl, self.anchors = det.na, det.nc, det.nl, det.anchors
        if self.nl > 5:
            raise NotImplementedError(f'at most 5 detection levels, got {self.nl}')
        self._anc = None

    def _anchors(self, dev):
        if self._anc is None or self._anc.device != dev:
            self._anc = self.anchors.detach().float().contiguous().to(dev)
        return self._anc

    def _launch(self, p, targets, need_grad):
        d, l5 = LossDesc(), LossLevel()                           # the descriptor holds four levels; a fifth (yolov5-p7) travels beside it
        grads = []
        for i, t in enumerate(p):
            if t.dtype != torch.float32 or not t.is_cuda:
                raise RuntimeError('prediction tensors have to be float32 on the GPU (no CPU fallback)')
            g = torch.empty_like(t) if need_grad else None
            grads.append(g)
            if i == 4:
                l5.p, l5.grad, l5.ny, l5.nx, l5.balance = _ptr(t), _ptr(g), t.shape[2], t.shape[3], self.balance[4]
                continue
            d.p[i] = _ptr(t)
            d.grad[i] = _ptr(g)
            d.ny[i], d.nx[i] = t.shape[2], t.shape[3]
        dev = p[0].device
        tg = targets.detach().to(dev).float().contiguous()
        d.nl, d.na, d.nc, d.B, d.nt = len(p), self.na, self.nc, p[0].shape[0], tg.shape[0]
        d.targets, d.anchors = (_ptr(tg) if tg.numel() else None), _ptr(self._anchors(dev))
        for i in range(min(len(p), 4)):
            d.balance[i] = self.balance[i]
        h = self.hyp
        d.box_gain, d.obj_gain, d.cls_gain = float(h['box']), float(h['obj']), float(h['cls'])
        d.cls_pw, d.obj_pw, d.anchor_t = float(h['cls_pw']), float(h['obj_pw']), float(h['anchor_t'])
        d.cp, d.cn, d.gr = float(self.cp), float(self.cn), float(self.gr)
        d.fl_gamma, d.slide = float(h['fl_gamma']), int(h['slide_ratio'] > 0)
        d.nwd_ratio = 0.5 if h['nwdloss'] > 0 else 0.0           # iou_ratio, utils/loss.py:148
        d.nwd_constant = 2.5 if h.get('shapeloss', 0) > 0 else 12.8   # wasserstein (utils/metrics.py:373) / wasserstein_loss (:341), :163-166
        L = _lib.lib()
        five = len(p) == 5
        r, l5p = self.rule, (C.byref(l5) if five else None)
        if self._default_rule:                                    # the reference's own line: the entry points, and the host path, it always had
            nbytes = L.somi_loss5_workspace_bytes(C.byref(d), C.byref(l5)) if five else L.somi_loss_workspace_bytes(C.byref(d))
        else:
            if r.wiou_scaled:
                if self.wiou_mean.device != dev:
                    self.wiou_mean = self.wiou_mean.to(dev)
                r.wiou_mean, r.wiou_train = _ptr(self.wiou_mean), int(bool(self.wiou_train))
            nbytes = L.somi_loss_rule_workspace_bytes(C.byref(d), l5p, C.byref(r))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        out = torch.empty(9 if five else 8, dtype=torch.float32, device=dev)
        if not self._default_rule:
            check(L.somi_yolo_loss_rule_f32(C.byref(d), l5p, C.byref(r), _ptr(out), _ptr(ws), nbytes, _stream()), 'ComputeLoss')
        elif five:
            check(L.somi_yolo_loss5_f32(C.byref(d), C.byref(l5), _ptr(out), _ptr(ws), nbytes, _stream()), 'ComputeLoss')
        else:
            check(L.somi_yolo_loss_f32(C.byref(d), _ptr(out), _ptr(ws), nbytes, _stream()), 'ComputeLoss')
        if self.autobalance:                                      # utils/loss.py:197-201 (a host sync per call, like the reference's .item())
            obji = out[4:4 + len(p)].tolist()
            bal = [self.balance[i] * 0.9999 + 0.0001 / obji[i] for i in range(len(p))] + list(self.balance[len(p):])
            self.balance = [x / bal[self.ssi] for x in bal]
        return out[:4], grads

    def __call__(self, p, targets):
        if len(p) != self.nl:
            raise RuntimeError(f'expected {self.nl} prediction levels, got {len(p)}')
        need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in p)
        pc = [t.detach().contiguous() for t in p]
        out, grads = self._launch(pc, targets, need_grad)
        loss = out[0:1]
        if need_grad:
            loss = _AttachGrad.apply(loss, grads, *p)
        return loss, out[1:4].detach()


def repulsion_loss(pbox, gtbox, fg_mask, sigma_repgt=0.9, sigma_repbox=0, pnms=0, gtnms=0):
    """RepGT + RepBox with the signature of utils/RepulsionLoss.py:47 -> (rep_gt, rep_box) 0-d GPU tensors.  The reference
    imports this term but never adds it to the loss (utils/loss.py:8); it is provided the same way: optional, value only."""
    if not (pbox.is_cuda and gtbox.is_cuda and fg_mask.is_cuda):
        raise RuntimeError('repulsion_loss runs on GPU tensors only (no CPU fallback)')
    if pbox.dim() != 3 or pbox.shape[-1] != 4 or gtbox.shape != pbox.shape or fg_mask.shape != pbox.shape[:2]:
        raise RuntimeError('repulsion_loss expects pbox, gtbox (B,A,4) and fg_mask (B,A)')
    Bn, A = fg_mask.shape
    pb, gb = pbox.detach().float().contiguous(), gtbox.detach().float().contiguous()
    fg = fg_mask.to(torch.uint8).contiguous()
    out = torch.empty(2, device=pbox.device, dtype=torch.float32)
    L = _lib.lib()
    nbytes = L.somi_repulsion_workspace_bytes(Bn, A)
    ws = torch.empty(nbytes, device=pbox.device, dtype=torch.uint8)
    check(L.somi_repulsion_loss_f32(pb.data_ptr(), gb.data_ptr(), fg.data_ptr(), Bn, A, float(sigma_repgt), float(sigma_repbox),
                                    float(pnms), float(gtnms), out.data_ptr(), ws.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream), 'repulsion_loss')
    return out[0], out[1]
