"""Plain-torch restatement of the box-regression rules the fused loss can score a matched box with (test infrastructure).

Follows utils/metrics.py: bbox_iou with its GIoU / DIoU / CIoU / EIoU / SIoU / EfficiCIoU / WIoU switches, Focal, alpha and scale (:476-583),
WIoU_Scale (:442-473, the non-monotonic v3 form), shape_iou (:397-439) and bbox_inner_iou / get_inner_iou in their xywh branch (:604-702),
eps for eps.  `RuleLoss` is ComputeLoss.__call__ (utils/loss.py:142-208, through oracle.somi_ref.loss) with the call of :161 replaced by a
box function and its return value composed into the loss the way somi_amd.loss.box_rule documents.  tools/gen_iou_loss_golden.py plugs the
reference's own functions into the same composition and writes tests/golden/iou_loss.npz; tests/test_iou_loss_host.py pins this file to it.

Also here: the rule table and the cases the fixture holds, the inputs' recipe, and `decision_margins`, the distance of every branch a rule
takes from flipping.
"""
import math

import numpy as np
import torch

from oracle.somi_ref.loss import ComputeLoss as _OracleLoss
from somi_amd.loss import RULE_SETTINGS

EPS = 1e-7
DEFAULTS = dict(iou='CIoU', focal=False, alpha=1.0, gamma=0.5, inner_ratio=None, shape_scale=0.5, wiou_scale=False)
RULES = RULE_SETTINGS                                            # tag -> ComputeLoss keywords (somi_amd.loss: the bench tool times the same table)
FOUR = ['GIoU', 'EIoU_focal', 'SIoU', 'WIoU_scaled']
# case -> (where its inputs are stored, extra hyper-parameters, rule tags)
CASES = {
    'a': ('a', {}, list(RULES)),
    'b': ('b', {}, FOUR),                                       # one level without entries
    'c': ('c', {}, FOUR),                                       # no targets
    'd': ('d', {}, FOUR),                                       # five levels
    'e': ('e', {}, FOUR),                                       # near-duplicated targets: cells hit more than once
    'f': ('a', {'nwdloss': 1.0}, ['EIoU_focal', 'WIoU_scaled']),
    'g': ('b', {'slide_ratio': 1.0}, FOUR),                     # SlideLoss over a level without entries: its 0.5 default under a rule
}
SHAPES = {'a': ((8, 4, 2), 40, False), 'b': ((8, 4, 2), 40, False), 'c': ((8, 4, 2), 0, False), 'd': ((16, 8, 4, 2, 1), 30, False),
          'e': ((8, 4, 2), 40, True)}
B, NC, NA = 2, 3, 3
WIOU_MOMENTUM = 1 - 0.5 ** (1 / 7000)


class Model:
    """What ComputeLoss reads of a model."""

    def __init__(self, anchors, hyp, nc=NC):
        class Det:
            pass
        d = Det()
        d.anchors, d.nl, d.na, d.nc = anchors, anchors.shape[0], anchors.shape[1], nc
        self.model, self.hyp = [d], hyp


def make_inputs(grids, nt, seed, near_duplicates=False, batch=B, nc=NC, na=NA):
    """anchors (nl,na,2) in grid units, predictions [(B,na,g,g,5+nc)], targets (nt,6): the recipe of the loss's random differential test."""
    g = torch.Generator().manual_seed(seed)
    anchors = torch.rand(len(grids), na, 2, generator=g) * 3 + 0.5
    p = [torch.randn(batch, na, s, s, nc + 5, generator=g) for s in grids]
    tg = torch.zeros(nt, 6)
    if nt:
        tg[:, 0] = torch.randint(0, batch, (nt,), generator=g).float()
        tg[:, 1] = torch.randint(0, nc, (nt,), generator=g).float()
        tg[:, 2:4] = torch.rand(nt, 2, generator=g) * 0.98 + 0.01
        tg[:, 4:6] = torch.exp(torch.randn(nt, 2, generator=g) * 0.7 - 2.5).clamp(0.01, 0.6)
        if near_duplicates:
            k = nt // 3
            tg[:k, 2:6] = tg[k:2 * k, 2:6] + torch.randn(k, 4, generator=g) * 1e-3
        tg[:, 2:6] = tg[:, 2:6].clamp(0.005, 0.995)
    return anchors, p, tg


# ------------------------------------------------------------------------------------------------ the rules
def _edges(box):
    x, y, w, h = box.unbind(-1)
    return x - w / 2, x + w / 2, y - h / 2, y + h / 2


def _overlap(a, b):
    ax1, ax2, ay1, ay2 = a
    bx1, bx2, by1, by2 = b
    return (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(0) * (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(0)


def _hull(a, b):
    return torch.maximum(a[1], b[1]) - torch.minimum(a[0], b[0]), torch.maximum(a[3], b[3]) - torch.minimum(a[2], b[2])


def _centre_gap(a, b):
    return b[0] + b[1] - a[0] - a[1], b[2] + b[3] - a[2] - a[3]


def _aspect(w1, h1, w2, h2):
    return (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2


def _shape_cost(ow, oh):
    return (1 - torch.exp(-ow)) ** 4 + (1 - torch.exp(-oh)) ** 4


def _siou_cost(dx, dy, cw, ch, w1, h1, w2, h2):
    """distance_cost + shape_cost of SIoU (:540-554)."""
    scw, sch = dx * 0.5 + EPS, dy * 0.5 + EPS
    sigma = (scw ** 2 + sch ** 2) ** 0.5
    sin1, sin2 = scw.abs() / sigma, sch.abs() / sigma
    angle = torch.cos(torch.arcsin(torch.where(sin1 > 2 ** 0.5 / 2, sin2, sin1)) * 2 - math.pi / 2)
    dist = 2 - torch.exp((angle - 2) * (scw / cw) ** 2) - torch.exp((angle - 2) * (sch / ch) ** 2)
    return dist + _shape_cost((w1 - w2).abs() / torch.maximum(w1, w2), (h1 - h2).abs() / torch.maximum(h1, h2))


class WIoUState:
    """WIoU_Scale's class state (:450-453) as an object; monotonous = False."""

    def __init__(self):
        self.mean, self.train = 1.0, True

    def factor(self, u):
        if self.train:
            self.mean = (1 - WIOU_MOMENTUM) * self.mean + WIOU_MOMENTUM * u.detach().mean().item()
        beta = u.detach() / self.mean
        return beta / (3 * torch.pow(1.9, beta - 3))


def rule_result(pbox, tbox, state=None, iou='CIoU', focal=False, alpha=1.0, gamma=0.5, inner_ratio=None, shape_scale=0.5, wiou_scale=False):
    """What the reference call of the rule returns for pbox, tbox (n,4) xywh: a tensor, a pair or (scaled WIoU) a triple."""
    a, b = _edges(pbox), _edges(tbox)
    inter = _overlap(a, b)
    cw, ch = _hull(a, b)
    dx, dy = _centre_gap(a, b)
    if inner_ratio is not None:                                  # bbox_inner_iou, xywh branch: widths and heights as given, no eps
        w1, h1, w2, h2 = pbox[:, 2], pbox[:, 3], tbox[:, 2], tbox[:, 3]
        q = inner_ratio
        ia = (pbox[:, 0] - w1 * q / 2, pbox[:, 0] + w1 * q / 2, pbox[:, 1] - h1 * q / 2, pbox[:, 1] + h1 * q / 2)
        ib = (tbox[:, 0] - w2 * q / 2, tbox[:, 0] + w2 * q / 2, tbox[:, 1] - h2 * q / 2, tbox[:, 1] + h2 * q / 2)
        iin = _overlap(ia, ib)
        inner = iin / (w1 * h1 * q * q + w2 * h2 * q * q - iin + EPS)
        union = w1 * h1 + w2 * h2 - inter + EPS
        if iou == 'IoU':
            return inner
        if iou == 'GIoU':
            c_area = cw * ch + EPS
            return inner - (c_area - union) / c_area
        pen = ((dx ** 2 + dy ** 2) / 4) / (cw ** 2 + ch ** 2 + EPS)
        if iou == 'DIoU':
            return inner - pen
        if iou == 'CIoU':
            v = _aspect(w1, h1, w2, h2)
            with torch.no_grad():
                av = v / (v - inter / union + (1 + EPS))
            return inner - (pen + v * av)
        if iou == 'EIoU':
            return inner - (pen + ((b[1] - b[0]) - (a[1] - a[0])) ** 2 / (cw ** 2 + EPS) + ((b[3] - b[2]) - (a[3] - a[2])) ** 2 / (ch ** 2 + EPS))
        assert iou == 'SIoU'
        return inner - 0.5 * _siou_cost(dx, dy, cw, ch, w1, h1, w2, h2) + EPS
    w1, h1 = a[1] - a[0], a[3] - a[2] + EPS
    w2, h2 = b[1] - b[0], b[3] - b[2] + EPS
    union = w1 * h1 + w2 * h2 - inter + EPS
    if iou == 'shape':
        sw, sh = torch.pow(w2, shape_scale), torch.pow(h2, shape_scale)
        ww, hh = 2 * sw / (sw + sh), 2 * sh / (sw + sh)
        dist = (hh * dx ** 2 / 4 + ww * dy ** 2 / 4) / (cw ** 2 + ch ** 2 + EPS + EPS)
        return inter / union - dist - 0.5 * _shape_cost(hh * (w1 - w2).abs() / torch.maximum(w1, w2), ww * (h1 - h2).abs() / torch.maximum(h1, h2))
    raw = inter / (union + EPS)
    r = torch.pow(raw, alpha)
    weight = torch.pow(raw, gamma)
    if iou == 'IoU':
        out = r
    elif iou == 'GIoU':
        c_area = cw * ch + EPS
        out = r - torch.pow((c_area - union) / c_area + EPS, alpha)
    else:
        pen = ((dx ** 2 + dy ** 2) / 4) ** alpha / ((cw ** 2 + ch ** 2) ** alpha + EPS)
        if iou == 'WIoU':
            if wiou_scale:
                return state.factor(1 - inter / union), (1 - r) * torch.exp(pen), r
            return r, torch.exp(pen)
        if iou == 'DIoU':
            out = r - pen
        elif iou in ('CIoU', 'EfficiCIoU'):
            v = _aspect(w1, h1, w2, h2)
            with torch.no_grad():
                av = v / (v - r + (1 + EPS))
            if iou == 'CIoU':
                out = r - (pen + torch.pow(v * av + EPS, alpha))
            else:
                wd, hd = a[1] - a[0] - b[1] + b[0], a[3] - a[2] - b[3] + b[2]
                out = r - (pen + wd ** 2 / (cw ** 2 + EPS) + hd ** 2 / (ch ** 2 + EPS) + v * av)
        elif iou == 'EIoU':
            rw, rh = (b[1] - b[0]) - (a[1] - a[0]), (b[3] - b[2]) - (a[3] - a[2])
            out = r - (pen + rw ** 2 / torch.pow(cw ** 2 + EPS, alpha) + rh ** 2 / torch.pow(ch ** 2 + EPS, alpha))
        else:
            assert iou == 'SIoU'
            out = r - torch.pow(0.5 * _siou_cost(dx, dy, cw, ch, w1, h1, w2, h2) + EPS, alpha)
    return (out, weight) if focal else out


def compose(ret):
    """A rule's return value -> (per-entry box term, similarity s): see somi_amd.loss.box_rule."""
    if not isinstance(ret, tuple):
        return 1.0 - ret, ret
    if len(ret) == 2:
        return ret[1].detach() * (1.0 - ret[0]), ret[0]
    return ret[0] * ret[1], ret[2]


class RuleLoss(_OracleLoss):
    """ComputeLoss.__call__ with `box_fn(pbox, tbox)` at utils/loss.py:161.  The anchor matching runs in fp32 whatever the predictions' type
    (an fp64 evaluation then takes the same decisions as the kernel); everything after it runs in the predictions' type."""

    def __init__(self, model, box_fn):
        super().__init__(model)
        self.box_fn = box_fn

    def __call__(self, p, targets):
        dt = p[0].dtype
        lcls, lbox, lobj = (torch.zeros(1, dtype=dt) for _ in range(3))
        tcls, tbox, indices, anchors = self.build_targets([t.detach().float() for t in p], targets.float())
        self.entries, self.boxes, self.sims = [], [], []                # per level: entry count, (pbox, tbox), the similarity before its clamp
        for i, pi in enumerate(p):
            b, a, gj, gi = indices[i]
            tobj = torch.zeros_like(pi[..., 0])
            n = b.shape[0]
            self.entries.append(n)
            auto_iou = None
            if n:
                ps = pi[b, a, gj, gi]
                pxy = ps[:, :2].sigmoid() * 2 - 0.5
                pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * anchors[i].to(dt)
                pbox, tb = torch.cat((pxy, pwh), 1), tbox[i].to(dt)
                self.boxes.append((pbox.detach(), tb))
                term, s = compose(self.box_fn(pbox, tb))
                if self.nwd:
                    nwd = self._wasserstein(pbox, tb, constant=self.nwd_constant).squeeze(-1)
                    lbox = lbox + 0.5 * term.mean() + 0.5 * (1.0 - nwd).mean()
                    s = s.detach() * 0.5 + nwd.detach() * 0.5
                else:
                    lbox = lbox + term.mean()
                    s = s.detach()
                self.sims.append(s)
                s = s.clamp(0, 1)
                order = torch.argsort(s)
                b, a, gj, gi, s = b[order], a[order], gj[order], gi[order], s[order]
                tobj[b, a, gj, gi] = (1.0 - self.gr) + self.gr * s
                auto_iou = s.mean()
                if self.nc > 1:
                    t = torch.full_like(ps[:, 5:], self.cn)
                    t[range(n), tcls[i]] = self.cp
                    lcls = lcls + self._bce(ps[:, 5:], t, self.cls_pw, auto_iou)
            else:
                self.boxes.append(None)
                self.sims.append(None)
            lobj = lobj + self._bce(pi[..., 4], tobj, self.obj_pw, auto_iou) * self.balance[i]
        lbox, lobj, lcls = lbox * self.hyp['box'], lobj * self.hyp['obj'], lcls * self.hyp['cls']
        return (lbox + lobj + lcls) * p[0].shape[0], torch.cat((lbox, lobj, lcls)).detach()


def restated_loss(anchors, hyp, rule, state=None):
    """RuleLoss around this file's restatement of `rule` (ComputeLoss keywords); `state`: a WIoUState for scaled WIoU."""
    kw = dict(DEFAULTS, **rule)
    return RuleLoss(Model(anchors, hyp, NC), lambda pb, tb: rule_result(pb, tb, state, **kw))


# ------------------------------------------------------------------------------------------------ decision margins
def _spacings(x, y):
    """|x - y| in fp32 spacings of the larger operand."""
    x, y = np.asarray(x, np.float32), np.broadcast_to(np.asarray(y, np.float32), np.shape(x))
    big = np.maximum(np.abs(x), np.abs(y))
    return np.abs(x.astype(np.float64) - y.astype(np.float64)) / np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64)


def decision_margins(pbox, tbox, s, rule):
    """The smallest distance from flipping, in fp32 spacings of the larger operand, of the branches `rule` takes on fp32 boxes (n,4):
    min / max operand choices, the sign under clamp(0), the sign under each abs, max(w1, w2) / max(h1, h2), SIoU's sin_alpha_1 > sqrt(2)/2
    and the clamp(0, 1) of the similarity `s` against either bound (an s that sits on a bound exactly - an IoU of boxes that do not overlap -
    is no decision: the clamp returns the bound from either side)."""
    kw = dict(DEFAULTS, **rule)
    pbox, tbox = pbox.float(), tbox.float()
    m = []
    pairs = [(_edges(pbox), _edges(tbox))]
    if kw['inner_ratio'] is not None:
        q = kw['inner_ratio']
        sc = torch.tensor([1, 1, q, q])
        pairs.append((_edges(pbox * sc), _edges(tbox * sc)))
    for a, b in pairs:
        for k in range(4):
            m.append(_spacings(a[k], b[k]))                                                       # min / max operand choice
        m.append(_spacings(torch.minimum(a[1], b[1]), torch.maximum(a[0], b[0])))                 # sign under clamp(0)
        m.append(_spacings(torch.minimum(a[3], b[3]), torch.maximum(a[2], b[2])))
    a, b = pairs[0]
    if kw['iou'] in ('SIoU', 'shape'):
        eps = 0.0 if kw['inner_ratio'] is not None else EPS
        m.append(_spacings(a[1] - a[0], b[1] - b[0]))                                             # |w1 - w2|, max(w1, w2)
        m.append(_spacings(a[3] - a[2] + eps, b[3] - b[2] + eps))
    if kw['iou'] == 'SIoU':
        m.append(_spacings((b[0] + b[1]) * 0.5 + EPS, (a[0] + a[1]) * 0.5))                       # sign of s_cw, s_ch under abs
        m.append(_spacings((b[2] + b[3]) * 0.5 + EPS, (a[2] + a[3]) * 0.5))
        scw, sch = (b[0] + b[1] - a[0] - a[1]) * 0.5 + EPS, (b[2] + b[3] - a[2] - a[3]) * 0.5 + EPS
        m.append(_spacings(scw.abs() / (scw ** 2 + sch ** 2) ** 0.5, np.float32(2 ** 0.5 / 2)))
    s = np.asarray(s, np.float32)
    live = s[(s != 0) & (s != 1)]                                # at a bound itself the clamp changes nothing on either side
    if live.size:
        m.append(_spacings(live, np.float32(0.0)))
        m.append(_spacings(live, np.float32(1.0)))
    return float(min(x.min() for x in m)) if len(pbox) else float('inf')
