"""CPU restatement of utils/autoanchor.py (`check_anchors`, `kmean_anchors`) and of the part of scipy.cluster.vq it calls (`kmeans`, `_kmeans`,
`_kpoints`, `vq` for two features, `update_cluster_means`), numpy and torch only.  The yardstick of tests/test_autoanchor_*.py next to the recorded
results under tests/golden/autoanchor_{a,b}.npz.

One deliberate difference from the reference, shared with the product: the fitness of a set of anchors is the EXACT sum of `best * (best > thr)` over
the labels (every term is 0 or an fp32 value in (thr, 1], a multiple of 2^-26 for thr >= 1/8, so an fp64 sum over < 2^27 labels is exact in any order),
where the reference takes an fp32 `.mean()` whose value depends on torch's summation order.  `fg > f` compares two such sums over the same labels.

The random draws are made on the two global generators (numpy's and `random`'s) in the reference's order.
"""
import random
from types import SimpleNamespace

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------- labels
def label_wh(dataset, img_size, scale=None):
    """autoanchor.py:29-31 / :103-104: label sizes in pixels of the letterboxed image, fp64 (fp32 labels times fp64 shapes)."""
    shapes = img_size * dataset.shapes / dataset.shapes.max(1, keepdims=True)
    if scale is not None:
        shapes = shapes * scale
    return np.concatenate([l[:, 3:5] * s for s, l in zip(shapes, dataset.labels)])


# ---------------------------------------------------------------------------------------------------------------- metric
def metric_terms(wh, k):
    """autoanchor.py:78-81.  wh (n,2), k (na,2) torch tensors -> x (n,na), best (n)."""
    r = wh[:, None] / k[None]
    x = torch.min(r, 1 / r).min(2)[0]
    return x, x.max(1)[0]


def anchor_metric(wh, k, thr):
    """thr: the reference's `anchor_t` (4.0).  -> labels with best > 1/thr, (label, anchor) pairs with x > 1/thr, exact fitness sum, best."""
    wh = torch.as_tensor(wh, dtype=torch.float32)
    k = torch.as_tensor(np.asarray(k), dtype=torch.float32).view(-1, 2)
    x, best = metric_terms(wh, k)
    t = 1 / thr
    keep = best > t
    return int(keep.sum()), int((x > t).sum()), float(best[keep].double().sum()), best


def fitness_sum(k, wh, thr):
    """autoanchor.py:83-85 with the exact sum; k fp64 (na,2) rounded to fp32 like torch.tensor(k, dtype=torch.float32)."""
    _, best = metric_terms(wh, torch.tensor(np.asarray(k), dtype=torch.float32))
    return float((best * (best > 1 / thr).float()).double().sum())


# ---------------------------------------------------------------------------------------------------------------- scipy.cluster.vq
def vq(obs, book):
    """_vq.vq for fewer than 5 features (`_vq_small_nf`): squared distance summed feature by feature, first minimum wins, sqrt of the minimum."""
    d = None
    for f in range(obs.shape[1]):
        diff = book[None, :, f] - obs[:, None, f]
        d = diff * diff if d is None else d + diff * diff
    code = d.argmin(1)
    return code, np.sqrt(d[np.arange(len(obs)), code])


def update_cluster_means(obs, code, nc):
    """_vq.update_cluster_means: members added in observation order (np.bincount adds sequentially), divided by the member count."""
    count = np.bincount(code, minlength=nc)
    cb = np.stack([np.bincount(code, weights=obs[:, f], minlength=nc) for f in range(obs.shape[1])], 1)
    has = count > 0
    cb[has] /= count[has][:, None]
    return cb, has


def lloyd(obs, guess, thresh=1e-5):
    """scipy.cluster.vq._kmeans -> (book, mean distance of the last assignment, iterations)."""
    book, prev, cur, diff, it = np.array(guess, dtype=np.float64), np.inf, np.inf, np.inf, 0
    while diff > thresh:
        code, distort = vq(obs, book)
        prev, cur = cur, distort.mean(axis=-1)
        book, has = update_cluster_means(obs, code, book.shape[0])
        book = book[has]
        diff = np.abs(prev - cur)
        it += 1
    return book, cur, it


def kmeans(obs, k, iter=30, thresh=1e-5):
    """scipy.cluster.vq.kmeans(obs, k, iter) with rng=None: `_kpoints` draws on numpy's global generator."""
    best_book, best_dist = None, np.inf
    for _ in range(iter):
        idx = np.random.choice(obs.shape[0], size=int(k), replace=False)
        book, dist, _ = lloyd(obs, obs[idx], thresh)
        if dist < best_dist:
            best_book, best_dist = book, dist
    return best_book, best_dist


# ---------------------------------------------------------------------------------------------------------------- evolution
def draw_mutations(gen, sh, mp=0.9, s=0.1):
    """autoanchor.py:120-123: the draws of every generation, up front (they do not depend on what was accepted)."""
    npr = np.random
    out = np.empty((gen,) + tuple(sh))
    for g in range(gen):
        v = np.ones(sh)
        while (v == 1).all():
            v = ((npr.random(sh) < mp) * random.random() * npr.randn(*sh) * s + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(k, wh, thr, v):
    """autoanchor.py:118-128 on given mutation factors -> (k, exact fitness sum, accepted generations)."""
    k = np.array(k, dtype=np.float64)
    f, accepted = fitness_sum(k, wh, thr), []
    for g in range(len(v)):
        kg = (k.copy() * v[g]).clip(min=2.0)
        fg = fitness_sum(kg, wh, thr)
        if fg > f:
            f, k = fg, kg.copy()
            accepted.append(g)
    return k, f, accepted


def kmean_anchors(dataset, n=9, img_size=640, thr=4.0, gen=1000, return_info=False):
    """autoanchor.py:73-131."""
    wh0 = label_wh(dataset, img_size)
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    k, dist = kmeans(wh / s, n, iter=30)
    assert len(k) == n, f'kmeans requested {n} points but returned only {len(k)}'
    k_white = k.copy()
    k = k * s
    wh = torch.tensor(wh, dtype=torch.float32)
    k = k[np.argsort(k.prod(1))]
    k_start = k.copy()
    v = draw_mutations(gen, k.shape)
    k, f, accepted = evolve(k, wh, thr, v)
    k = k[np.argsort(k.prod(1))]
    if return_info:
        return k, SimpleNamespace(k_white=k_white, dist=dist, std=s, k_start=k_start, accepted=accepted, fitness_sum=f, n_fit=len(wh), v=v)
    return k


# ---------------------------------------------------------------------------------------------------------------- check_anchors
def check_anchor_order(m):
    a = m.anchors.prod(-1).view(-1)
    if (a[-1] - a[0]).sign() != (m.stride[-1] - m.stride[0]).sign():
        m.anchors[:] = m.anchors.flip(0)


def check_anchors(dataset, m, thr=4.0, imgsz=640, gen=1000):
    """autoanchor.py:25-70 on the head `m` (anchors (nl,na,2) in grid units, stride (nl)).  -> dict(bpr, aat, new_bpr, replaced)."""
    scale = np.random.uniform(0.9, 1.1, size=(len(dataset.shapes), 1))
    wh = torch.tensor(label_wh(dataset, imgsz, scale)).float()

    def metric(k):
        r = wh[:, None] / k[None]
        x = torch.min(r, 1 / r).min(2)[0]
        best = x.max(1)[0]
        return (best > 1 / thr).float().mean(), (x > 1 / thr).float().sum(1).mean()

    anchors = m.anchors.clone() * m.stride.to(m.anchors.device).view(-1, 1, 1)
    bpr, aat = metric(anchors.cpu().view(-1, 2))
    out = dict(bpr=float(bpr), aat=float(aat), new_bpr=None, replaced=False)
    if bpr < 0.98:
        na = m.anchors.numel() // 2
        anchors = kmean_anchors(dataset, n=na, img_size=imgsz, thr=thr, gen=gen)
        new_bpr = metric(torch.as_tensor(anchors))[0]         # fp64 anchors against fp32 labels: this one BPR is computed in fp64, as in the reference
        out['new_bpr'] = float(new_bpr)
        if new_bpr > bpr:
            anchors = torch.tensor(anchors, device=m.anchors.device).type_as(m.anchors)
            m.anchors[:] = anchors.clone().view_as(m.anchors) / m.stride.to(m.anchors.device).view(-1, 1, 1)
            check_anchor_order(m)
            out['replaced'] = True
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
class LabelSet:
    """The data-set stand-in both `check_anchors` and `kmean_anchors` accept: `.shapes` (n_img, 2) and `.labels` (list of (n_i, 5))."""

    def __init__(self, wh_norm, counts, shapes):
        self.shapes = np.asarray(shapes, dtype=np.float64)
        self.labels, o = [], 0
        for c in counts:
            lab = np.zeros((int(c), 5), dtype=np.float32)
            lab[:, 3:5] = wh_norm[o:o + int(c)]
            self.labels.append(lab)
            o += int(c)


def synth_label_set(n_img, seed=0):
    """The recipe of the fixtures -> (wh_norm fp32 (N,2), counts, shapes int (n_img,2)).  Classes and centres are drawn (the order matters) and dropped."""
    r = np.random.RandomState(seed)
    w = r.randint(480, 1920, n_img)
    h = r.randint(360, 1080, n_img)
    whs, counts = [], []
    for _ in range(n_img):
        n = int(np.clip(r.poisson(54), 1, 300))
        wh = np.clip(np.exp(r.normal(np.log(0.03), 0.7, (n, 2))), 0.004, 0.5)
        r.randint(0, 10, n)
        r.uniform(0.02, 0.98, (n, 2))
        whs.append(wh.astype(np.float32)), counts.append(n)
    return np.concatenate(whs), np.array(counts, dtype=np.int32), np.stack([w, h], 1).astype(np.int32)
