"""AutoAnchor (utils/autoanchor.py) on the MI355X: `check_anchors`, `kmean_anchors` and their building block `anchor_metric`.

The host layer keeps the reference's call signatures, decisions and - draw for draw, on the two global generators (numpy's and `random`'s) -
its random numbers, so that after `np.random.seed(s); random.seed(s)` a run follows the reference's.  The arithmetic over the labels runs in
csrc/autoanchor.hip: the fp32 metric, the genetic evolution with `k`, its fitness and all mutation factors resident on the device (one read-back at the
end), and scipy's `kmeans` as batched fp64 Lloyd steps (one small read-back per step: the stop flags).

One deliberate difference from the reference: fitness is the EXACT sum of `best * (best > thr)` (fp64 over fp32 terms, exact in any order for
thr <= 8 and fewer than 2^27 labels), where the reference takes an fp32 mean whose value depends on torch's CPU summation order.  Accepting a generation
compares two exact sums over the same labels; see DESIGN.md section 4e.
"""
import logging
import os
import random
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import _ptr, _stream

LOGGER = logging.getLogger(__name__)
MAX_ANCHORS = 64                 # kAnchorMax of csrc/autoanchor.hip
MAX_KMEANS_K = 32                # kKmeansMaxK
KMEANS_MAX_STEPS = 10000         # a restart that has not met scipy's stop test by then is an error, not a hang

AnchorMetric = namedtuple('AnchorMetric', 'n n_best n_above fitness_sum bpr aat fitness best')
AnchorCheck = namedtuple('AnchorCheck', 'bpr aat new_bpr new_aat replaced anchors')


def _device(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError('somi_amd autoanchor runs on the MI355X only (no CPU fallback)')
    return torch.device('cuda' if device is None else device)


def label_wh(dataset, img_size, scale=None):
    """autoanchor.py:29-31 / :103-104: label sizes in pixels of the image scaled to `img_size`, fp64 (n, 2)."""
    shapes = np.asarray(dataset.shapes, dtype=np.float64)
    if shapes.ndim != 2 or shapes.shape[1] != 2 or len(shapes) != len(dataset.labels):
        raise ValueError('dataset.shapes has to be (n_img, 2) width / height, one row per entry of dataset.labels')
    shapes = img_size * shapes / shapes.max(1, keepdims=True)
    if scale is not None:
        shapes = shapes * scale
    return np.concatenate([np.asarray(l)[:, 3:5] * s for s, l in zip(shapes, dataset.labels)])


def _thr32(thr):
    """The reference compares fp32 tensors with the Python float 1 / thr: torch rounds that scalar to fp32."""
    return float(np.float32(1.0 / thr))


# ---------------------------------------------------------------------------------------------------------------- metric
def _metric_launch(wh, anchors, thr, best=None):
    L = _lib.lib()
    n, na = wh.shape[0], anchors.shape[0]
    nbytes = L.somi_anchor_metric_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=wh.device)
    out = torch.empty(3, dtype=torch.float64, device=wh.device)
    check(L.somi_anchor_metric_f32(_ptr(wh), n, _ptr(anchors), na, _thr32(thr), _ptr(best), _ptr(out), _ptr(ws), nbytes, _stream()), 'anchor_metric')
    return out


def anchor_metric(wh, anchors, thr=4.0, return_best=False, device=None):
    """The metric both `check_anchors` (:33-39) and `kmean_anchors` (:78-85) use.  wh (n, 2) label sizes and anchors (na, 2), both in pixels (rounded
    to fp32 as the reference does before it divides), thr = `anchor_t`.  -> AnchorMetric: n labels, n_best labels with best > 1 / thr, n_above (label,
    anchor) pairs with x > 1 / thr, fitness_sum = exact sum of best over the n_best labels; and from them bpr = n_best / n, aat = n_above / n,
    fitness = fitness_sum / n.  best: the per-label fp32 values (device tensor) when `return_best`."""
    dev = _device(device)
    wh = torch.as_tensor(wh).to(dev).to(torch.float32).reshape(-1, 2).contiguous()
    anchors = torch.as_tensor(anchors).to(dev).to(torch.float32).reshape(-1, 2).contiguous()
    n, na = wh.shape[0], anchors.shape[0]
    if n < 1 or not 1 <= na <= MAX_ANCHORS:
        raise ValueError(f'anchor_metric needs at least one label and 1 to {MAX_ANCHORS} anchors')
    best = torch.empty(n, dtype=torch.float32, device=dev) if return_best else None
    nb, nx, fs = _metric_launch(wh, anchors, thr, best).tolist()
    return AnchorMetric(n, int(nb), int(nx), fs, nb / n, nx / n, fs / n, best)


# ---------------------------------------------------------------------------------------------------------------- k-means
def lloyd(obs, guess, thresh=1e-5, device=None):
    """scipy.cluster.vq._kmeans for a batch of start books.  obs (n, 2) fp64, guess (R, k, 2): R independent restarts run side by side, one pair of
    launches per Lloyd step for all that are still moving.  -> list of R (book, dist, steps): codes that lost all members are dropped like scipy does,
    dist = mean Euclidean distance of the last assignment."""
    dev = _device(device)
    L = _lib.lib()
    obs_d = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float64)).to(dev)
    book = torch.as_tensor(np.ascontiguousarray(guess, dtype=np.float64)).to(dev).contiguous()
    if obs_d.ndim != 2 or obs_d.shape[1] != 2 or book.ndim != 3 or book.shape[2] != 2:
        raise ValueError('lloyd: obs (n, 2) and guess (restarts, k, 2)')
    n, (R, K) = obs_d.shape[0], book.shape[:2]
    if not 1 <= K <= MAX_KMEANS_K:
        raise NotImplementedError(f'the k-means kernel holds 1 to {MAX_KMEANS_K} codes, {K} asked for')
    alive = torch.ones(R, K, dtype=torch.int32, device=dev)
    dist = torch.full((R,), float('inf'), dtype=torch.float64, device=dev)
    done = torch.zeros(R, dtype=torch.int32, device=dev)
    iters = torch.zeros(R, dtype=torch.int32, device=dev)
    nbytes = L.somi_kmeans_workspace_bytes(n, K, R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for _ in range(KMEANS_MAX_STEPS):
        check(L.somi_kmeans_lloyd_step_f64(_ptr(obs_d), n, _ptr(book), _ptr(alive), K, R, float(thresh), _ptr(dist), _ptr(done), _ptr(iters),
                                           _ptr(ws), nbytes, _stream()), 'kmeans lloyd step')
        if bool(done.cpu().all()):                     # the one read-back of the step: R stop flags
            break
    else:
        raise RuntimeError(f'k-means did not meet its stop test within {KMEANS_MAX_STEPS} steps')
    book, alive, dist, iters = book.cpu().numpy(), alive.cpu().numpy().astype(bool), dist.cpu().numpy(), iters.cpu().numpy()
    return [(book[r][alive[r]], float(dist[r]), int(iters[r])) for r in range(R)]


def kmeans(obs, k, iter=30, thresh=1e-5, device=None):
    """scipy.cluster.vq.kmeans(obs, k, iter) with rng=None: `iter` restarts from k observations drawn by `np.random.choice(n, k, replace=False)` on
    numpy's global generator (the restarts draw nothing else, so all starts are drawn first and the restarts run as one batch).
    -> (book, dist) of the first restart with the lowest mean distance."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    starts = np.stack([obs[np.random.choice(obs.shape[0], size=int(k), replace=False)] for _ in range(iter)])
    best_book, best_dist = None, np.inf
    for book, dist, _ in lloyd(obs, starts, thresh, device):
        if dist < best_dist:
            best_book, best_dist = book, dist
    return best_book, best_dist


# ---------------------------------------------------------------------------------------------------------------- evolution
def draw_mutations(gen, shape, mp=0.9, s=0.1):
    """autoanchor.py:120-123 for all generations up front: the draws do not depend on which candidates were accepted.  Per generation, repeated
    while the factors are all 1: `np.random.random(shape)`, `random.random()`, `np.random.randn(*shape)` - the reference's calls in its order."""
    npr = np.random
    out = np.empty((gen,) + tuple(shape), dtype=np.float64)
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((npr.random(shape) < mp) * random.random() * npr.randn(*shape) * s + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(wh, k, v, thr=4.0, device=None):
    """autoanchor.py:118-128 on the device.  wh (n, 2) fp32 labels (device tensor or array), k (na, 2) fp64 start anchors, v (gen, na, 2) fp64
    mutation factors.  -> (k fp64 (na, 2), exact fitness sum, accepted generations); the only device-to-host copies are these three at the end."""
    dev = _device(device)
    L = _lib.lib()
    wh = torch.as_tensor(wh).to(dev).to(torch.float32).reshape(-1, 2).contiguous()
    k_d = torch.as_tensor(np.ascontiguousarray(k, dtype=np.float64)).to(dev).reshape(-1, 2).contiguous()
    n, na = wh.shape[0], k_d.shape[0]
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, na, 2)
    gen = v.shape[0]
    if n < 1 or not 1 <= na <= MAX_ANCHORS:
        raise ValueError(f'evolve needs at least one label and 1 to {MAX_ANCHORS} anchors')
    v_d = torch.as_tensor(v).to(dev)                                    # every generation's factors, uploaded once
    f = _metric_launch(wh, k_d.to(torch.float32), thr)[2:3].clone()     # fitness sum of the start anchors, stays on the device
    accepted = torch.zeros(gen + 1, dtype=torch.int32, device=dev)
    nbytes = L.somi_anchor_metric_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.somi_anchor_evolve_f32(_ptr(wh), n, _ptr(k_d), na, _ptr(v_d) if gen else None, gen, _thr32(thr), _ptr(f), _ptr(accepted), _ptr(ws),
                                   nbytes, _stream()), 'anchor evolve')
    accepted = accepted.cpu().tolist()
    return k_d.cpu().numpy(), float(f.item()), accepted[1:1 + accepted[0]]


def _report(prefix, k, wh0, thr, n, img_size):
    m = anchor_metric(wh0, k, thr)
    LOGGER.info('%sthr=%.2f: %.4f best possible recall, %.2f anchors past thr; n=%d, img_size=%s: %s', prefix, 1 / thr, m.bpr, m.aat, n, img_size,
                ',  '.join('%i,%i' % (round(x[0]), round(x[1])) for x in k))


def kmean_anchors(dataset, n=9, img_size=640, thr=4.0, gen=1000, verbose=True, device=None):
    """autoanchor.py:73-131: k-means anchors from the labels of `dataset`, then `gen` generations of mutation.  dataset: any object with `.shapes`
    ((n_img, 2) original width / height) and `.labels` (list of (n_i, 5) [cls, x, y, w, h] normalised), e.g. a DeviceImageCache; a yaml path is not
    accepted (that branch builds the reference's CPU loader).  -> (n, 2) fp64 anchors in pixels, sorted by area."""
    if isinstance(dataset, (str, os.PathLike)):
        raise NotImplementedError('kmean_anchors takes a data set object with .shapes and .labels, not a yaml path')
    if not 1 <= n <= MAX_KMEANS_K:
        raise NotImplementedError(f'kmean_anchors holds 1 to {MAX_KMEANS_K} anchors, {n} asked for')
    dev = _device(device)
    prefix = 'autoanchor: '
    wh0 = label_wh(dataset, img_size)
    i = int((wh0 < 3.0).any(1).sum())
    if i:
        LOGGER.warning('%sextremely small objects found: %d of %d labels are < 3 pixels in size', prefix, i, len(wh0))
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    k, _ = kmeans(wh / s, n, iter=30, device=dev)
    assert len(k) == n, f'{prefix}ERROR: k-means requested {n} points but returned only {len(k)}'
    k = k * s
    wh = torch.tensor(wh, dtype=torch.float32).to(dev)
    k = k[np.argsort(k.prod(1))]
    if verbose:
        _report(prefix + 'k-means: ', k, wh0, thr, n, img_size)
    v = draw_mutations(gen, k.shape)
    k, f, accepted = evolve(wh, k, v, thr, dev)
    k = k[np.argsort(k.prod(1))]
    if verbose:
        _report(prefix + f'{len(accepted)} of {gen} generations accepted, fitness {f / len(wh):.4f}: ', k, wh0, thr, n, img_size)
    return k


# ---------------------------------------------------------------------------------------------------------------- check_anchors
def check_anchors(dataset, model, thr=4.0, imgsz=640, save_dir=None, kmean=1):
    """autoanchor.py:25-70: measure the model's anchors against the labels and replace them by `kmean_anchors` when their best possible recall is
    below 0.98 and the new ones recall more.  Writes the head's `anchors` buffer (ordered with the strides by Model._check_anchor_order, divided by stride),
    drops the head's cached host copy and, with `save_dir`, writes new_anchors.txt.  -> AnchorCheck(bpr, aat, new_bpr, new_aat, replaced, anchors):
    the figures of the old anchors, of the new ones (None when no search ran) and the (n, 2) pixel anchors written (None when kept).
    Both BPR figures are computed by the fp32 device metric on the anchors rounded to fp32 - the values the head then holds (the reference scores the
    new ones through an fp64 array).  Build ComputeLoss after this call: it reads the head's anchors at construction."""
    if kmean != 1:
        raise NotImplementedError('kmean=2 (kmeanPlus_anchors: scikit-learn\'s k-means++) is not built; only kmean=1 (scipy-style k-means) is')
    from .model import Model
    m = model.module.model[-1] if hasattr(model, 'module') else model.model[-1]
    dev = _device(m.anchors.device if m.anchors.is_cuda else None)
    prefix = 'autoanchor: '
    scale = np.random.uniform(0.9, 1.1, size=(len(dataset.shapes), 1))
    wh = torch.tensor(label_wh(dataset, imgsz, scale)).float().to(dev)
    stride = m.stride.to(m.anchors.device).view(-1, 1, 1)
    old = anchor_metric(wh, (m.anchors.clone() * stride).view(-1, 2), thr)
    LOGGER.info('%sanchors/target = %.2f, Best Possible Recall (BPR) = %.4f', prefix, old.aat, old.bpr)
    if not np.float32(old.n_best) / np.float32(old.n) < np.float32(0.98):        # the reference's test is on an fp32 mean against fp32(0.98)
        return AnchorCheck(old.bpr, old.aat, None, None, False, None)
    na = m.anchors.numel() // 2
    anchors = kmean_anchors(dataset, n=na, img_size=imgsz, thr=thr, gen=1000, verbose=False, device=dev)
    anchors = torch.tensor(anchors, device=m.anchors.device).type_as(m.anchors)
    new = anchor_metric(wh, anchors, thr)
    if not new.n_best > old.n_best:                       # same labels: comparing the counts is comparing the recalls
        LOGGER.info('%soriginal anchors better than new anchors, proceeding with original anchors', prefix)
        return AnchorCheck(old.bpr, old.aat, new.bpr, new.aat, False, None)
    # Order against the strides in PIXELS, then scale - the sequence Model uses when it builds a DecoupledDetect head.  The reference scales first
    # and compares areas in grid units, where dividing by stride^2 turns an ascending set around whenever the largest anchor has less than
    # (s_last / s_first)^2 times the area of the smallest (16 SOMI anchors on strides 4..32 over small objects: it reverses them and the stride-4
    # level ends up with the largest anchors).  The sorted k-means result on ascending strides stays as it is; descending strides reverse it.
    m.anchors[:] = anchors.clone().view_as(m.anchors)
    Model._check_anchor_order(m)
    anchors = m.anchors.clone()
    m.anchors /= stride
    m.invalidate()                                        # the head decodes from a cached host copy of its anchors
    if save_dir is not None:
        with open(os.path.join(save_dir, 'new_anchors.txt'), 'w') as fh:
            for a in anchors.view(-1, 2).cpu().numpy():
                fh.write(f'{a[0]} {a[1]}\n')
    LOGGER.info('%snew anchors saved to model (BPR %.4f); update the model yaml to use them in the future', prefix, new.bpr)
    return AnchorCheck(old.bpr, old.aat, new.bpr, new.aat, True, anchors.view(-1, 2).cpu().numpy())
