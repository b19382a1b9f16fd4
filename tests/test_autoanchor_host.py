"""AutoAnchor without a GPU: the CPU restatement (tests/autoanchor_ref.py) against what the reference and scipy recorded in
tests/golden/autoanchor_{a,b}.npz (tools/gen_autoanchor_golden.py), and the host layer of somi_amd.autoanchor that needs no device - the random draws,
`DeviceImageCache.shapes`, the `kmean=2` limit."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autoanchor_ref as R  # noqa: E402

SETS = ['a', 'b']


def np_state():
    s = np.random.get_state()
    return np.concatenate([s[1].astype(np.uint32), np.array([s[2]], dtype=np.uint32)])


def py_state():
    return np.array(random.getstate()[1], dtype=np.uint64)


def seed(s=0):
    np.random.seed(s), random.seed(s)


def label_set(g):
    return R.LabelSet(g['wh_norm'], g['counts'], g['shapes'])


def head(anchors, strides):
    from types import SimpleNamespace
    m = SimpleNamespace(anchors=torch.tensor(anchors).float().view(len(anchors), -1, 2), stride=torch.tensor(strides).float())
    m.anchors /= m.stride.view(-1, 1, 1)
    return m


def fit_labels(ds):
    wh0 = R.label_wh(ds, 640)
    return wh0, wh0[(wh0 >= 2.0).any(1)]


@pytest.mark.parametrize('name', SETS)
def test_fixture_is_the_recipe(golden, name):
    g = golden('autoanchor_' + name)
    n_img = {'a': 200, 'b': 600}[name]
    wh, counts, shapes = R.synth_label_set(n_img, 0)
    assert len(wh) == {'a': 10745, 'b': 32365}[name]
    assert np.array_equal(wh, g['wh_norm']) and np.array_equal(counts, g['counts']) and np.array_equal(shapes, g['shapes'])
    assert int(g['n']) == {'a': 9, 'b': 12}[name]


@pytest.mark.parametrize('name', SETS)
def test_restated_metric_counts_equal_the_recorded_ones(golden, name):
    g = golden('autoanchor_' + name)
    ds = label_set(g)
    seed(0)
    scale = np.random.uniform(0.9, 1.1, size=(len(ds.shapes), 1))
    assert np.array_equal(np_state(), g['check_np_state'])
    wh = torch.tensor(R.label_wh(ds, 640, scale)).float()
    n = int(g['n'])
    coco = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
    for tag, anchors in (('placeholder', [list(range(2 * (n // 3)))] * 3), ('coco', coco)):
        m = head(anchors, g['strides'])
        nb, nx, fs, best = R.anchor_metric(wh, (m.anchors * m.stride.view(-1, 1, 1)).view(-1, 2), 4.0)
        assert [nb, nx] == g[tag + '_counts'].tolist()
        assert np.float32(nb) / np.float32(len(wh)) == np.float32(g[tag + '_bpr_aat'][0])
        assert fs == float(best[best > 0.25].double().sum()) and 0.25 * nb < fs <= nb
    if name == 'a':
        assert f"{g['placeholder_bpr_aat'][0]:.4f} {g['placeholder_bpr_aat'][1]:.2f}" == '0.3098 1.11'
        assert f"{g['coco_bpr_aat'][0]:.4f} {g['coco_bpr_aat'][1]:.2f}" == '0.9076 2.85'


@pytest.mark.parametrize('name', SETS)
def test_restated_kmeans_follows_scipy(golden, name):
    """1e-9 absolute in whitened units: the only freedom is the order of fp64 sums over n <= 1e5 values of order 1, at most n * 2^-53 ~ 1e-11."""
    g = golden('autoanchor_' + name)
    _, wh = fit_labels(label_set(g))
    obs = wh / wh.std(0)
    book, dist, _ = R.lloyd(obs, obs[g['lloyd_start']])
    assert book.shape == g['lloyd_book'].shape
    assert np.abs(book - g['lloyd_book']).max() <= 1e-9 and abs(dist - float(g['lloyd_dist'])) <= 1e-9
    seed(0)
    k, dist = R.kmeans(obs, int(g['n']), iter=30)
    assert k.shape == g['kmeans_white'].shape
    assert np.abs(k - g['kmeans_white']).max() <= 1e-9 and abs(dist - float(g['kmeans_dist'])) <= 1e-9
    assert np.array_equal(np_state(), g['kmeans_np_state'])


@pytest.mark.parametrize('name', SETS)
def test_restated_evolution_is_bit_identical_to_the_reference(golden, name):
    """The condition on the fixtures: from the reference's own k-means result, exact-sum fitness (restatement) and fp32-mean fitness (reference) accept
    the same generations and end on the same anchors, bit for bit; and the draws leave both global generators where the reference left them."""
    g = golden('autoanchor_' + name)
    _, wh = fit_labels(label_set(g))
    k0 = g['kmeans_white'] * wh.std(0)
    k0 = k0[np.argsort(k0.prod(1))]
    whf = torch.tensor(wh, dtype=torch.float32)
    assert len(whf) == int(g['n_fit'])
    assert R.fitness_sum(k0, whf, 4.0) / len(whf) == float(g['kmeans_fitness'])
    np.random.set_state(('MT19937', g['kmeans_np_state'][:624], int(g['kmeans_np_state'][624]), 0, 0.0))
    random.seed(0)
    v = R.draw_mutations(1000, k0.shape)
    assert np.array_equal(np_state(), g['final_np_state']) and np.array_equal(py_state(), g['final_py_state'])
    assert np.array_equal(v[:len(g['mutations'])], g['mutations'])
    k, f, accepted = R.evolve(k0, whf, 4.0, v)
    k = k[np.argsort(k.prod(1))]
    assert accepted == g['accepted'].tolist() and len(accepted) == {'a': 121, 'b': 124}[name]
    assert np.array_equal(k, g['final_anchors'])
    assert f / len(whf) == float(g['seed_fitness_exact'][0])
    assert abs(f / len(whf) - float(g['seed_fitness'][0])) < 1e-6           # the reference's fp32 mean of the same anchors


def test_restated_kmean_anchors_and_check_anchors_end_to_end(golden):
    """Set a, seed 0, the whole calls: restated k-means (not scipy's recorded book) feeding the evolution.  `check_anchors` runs its search from
    another position of the generators, where nothing says that exact-sum and fp32-mean fitness take the same branches (the fixtures' condition was
    checked for `kmean_anchors` at seed 0 only): there the draws and the decisions are pinned, and the result has to recall as much as the
    reference's worst of six seeds."""
    g = golden('autoanchor_a')
    ds = label_set(g)
    seed(0)
    k = R.kmean_anchors(ds, n=9, img_size=640, thr=4.0, gen=1000)
    assert np.array_equal(np_state(), g['final_np_state']) and np.array_equal(py_state(), g['final_py_state'])
    assert np.abs(k - g['final_anchors']).max() <= 1e-6                    # equal books up to 1e-9 whitened; the same generations accepted
    seed(0)
    m = head([list(range(6))] * 3, g['strides'])
    out = R.check_anchors(ds, m, thr=4.0, imgsz=640)
    assert out['replaced'] and f"{out['bpr']:.4f}" == '0.3098' and out['new_bpr'] > 0.99
    assert np.array_equal(np_state(), g['check_final_np_state']) and np.array_equal(py_state(), g['check_final_py_state'])
    wh0, _ = fit_labels(ds)                                                 # BPR as recorded per seed: all labels, unscaled
    nb = R.anchor_metric(wh0, (m.anchors * m.stride.view(-1, 1, 1)).view(-1, 2), 4.0)[0]
    assert float(np.float32(nb) / np.float32(len(wh0))) >= g['seed_bpr'].min()
    a = (m.anchors * m.stride.view(-1, 1, 1)).prod(-1).view(-1)
    assert a[-1] > a[0]


# ---------------------------------------------------------------------------------------------------------------- the product's host layer
def test_host_draws_are_the_references(golden):
    from somi_amd import autoanchor as A
    g = golden('autoanchor_a')
    np.random.set_state(('MT19937', g['kmeans_np_state'][:624], int(g['kmeans_np_state'][624]), 0, 0.0))
    random.seed(0)
    v = A.draw_mutations(1000, (9, 2))
    assert v.dtype == np.float64 and v.shape == (1000, 9, 2)
    assert np.array_equal(v[:len(g['mutations'])], g['mutations'])
    assert np.array_equal(np_state(), g['final_np_state']) and np.array_equal(py_state(), g['final_py_state'])
    assert not (v == 1).all(axis=(1, 2)).any() and v.min() >= 0.3 and v.max() <= 3.0


def test_host_label_sizes_and_threshold(golden):
    from somi_amd import autoanchor as A
    g = golden('autoanchor_a')
    ds = label_set(g)
    scale = np.random.RandomState(3).uniform(0.9, 1.1, size=(len(ds.shapes), 1))
    assert np.array_equal(A.label_wh(ds, 640), R.label_wh(ds, 640))
    assert np.array_equal(A.label_wh(ds, 512, scale), R.label_wh(ds, 512, scale))
    for thr in (4.0, 2.91, 3.44, 8.0):
        assert A._thr32(thr) == float(torch.tensor(1 / thr, dtype=torch.float32))
    with pytest.raises(ValueError):
        ds.shapes = ds.shapes[:-1]
        A.label_wh(ds, 640)


def test_limits_are_named():
    from somi_amd import autoanchor as A
    with pytest.raises(NotImplementedError, match='kmean=2'):
        A.check_anchors(None, None, kmean=2)
    with pytest.raises(NotImplementedError, match='yaml'):
        A.kmean_anchors('data/coco128.yaml')
    with pytest.raises(NotImplementedError, match='32'):
        A.kmean_anchors(object(), n=33)


def test_device_image_cache_has_shapes():
    """`.shapes` = the shapes= argument, else the cached sizes, (width, height) rows in the order of `.labels` (re-ordered under rect=True)."""
    from somi_amd import augment
    imgs = [np.zeros((h, w, 3), np.uint8) for h, w in ((32, 64), (64, 48), (40, 64), (64, 64))]
    labels = [np.full((i + 1, 5), 0.1 * (i + 1), np.float32) for i in range(4)]
    ds = augment.DeviceImageCache(imgs, labels, img_size=64, augment=False, device='cpu')
    assert ds.shapes.dtype == np.float64 and ds.shapes.tolist() == [[64, 32], [48, 64], [64, 40], [64, 64]]
    orig = [(1280, 640), (720, 960), (1920, 1200), (800, 800)]
    ds = augment.DeviceImageCache(imgs, labels, img_size=64, augment=False, shapes=orig, device='cpu')
    assert ds.shapes.tolist() == [list(map(float, s)) for s in orig]
    ds = augment.DeviceImageCache(imgs, labels, img_size=64, augment=False, rect=True, batch_size=2, shapes=orig, device='cpu')
    assert sorted(ds.order.tolist()) == [0, 1, 2, 3] and ds.order.tolist() != [0, 1, 2, 3]
    assert ds.shapes.tolist() == [list(map(float, orig[i])) for i in ds.order]
    assert [len(l) for l in ds.labels] == [i + 1 for i in ds.order]
    wh = R.label_wh(ds, 640)                                                     # a cache is a data set for autoanchor
    assert wh.shape == (10, 2)
