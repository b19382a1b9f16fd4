"""AutoAnchor on the MI355X (somi_amd.autoanchor over csrc/autoanchor.hip) against the fixtures tests/golden/autoanchor_{a,b}.npz - recorded from the
reference and scipy by tools/gen_autoanchor_golden.py - and against the CPU restatement tests/autoanchor_ref.py; never against the product itself.
Neither the reference nor scipy is read here."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autoanchor_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SETS = ['a', 'b']


def seed(s=0):
    np.random.seed(s), random.seed(s)


def label_set(g):
    return R.LabelSet(g['wh_norm'], g['counts'], g['shapes'])


def fit_labels(ds):
    wh0 = R.label_wh(ds, 640)
    return wh0, wh0[(wh0 >= 2.0).any(1)]


def set_np_state(state):
    np.random.set_state(('MT19937', state[:624], int(state[624]), 0, 0.0))


# ---------------------------------------------------------------------------------------------------------------- 1. metric
@pytest.mark.parametrize('na', [1, 9, 16])
@pytest.mark.parametrize('n', [1, 255, 256, 4096, 10745, 300001])
def test_metric_is_torchs_fp32_result_and_the_sums_are_exact(golden, n, na):
    """Per-label best bit-equal to torch's CPU fp32 arithmetic, both counts equal, the fitness sum equal to the restatement's exact sum - at label counts
    that are and are not multiples of the 256-thread block, below and above one full grid (1024 blocks)."""
    from somi_amd import autoanchor as A
    g = golden('autoanchor_b')
    rng = np.random.RandomState(100 * na + n % 97)
    wh0, _ = fit_labels(label_set(g))
    wh = torch.tensor(wh0[rng.randint(0, len(wh0), n)] * rng.uniform(0.5, 2.0, (n, 1))).float()
    k = torch.tensor(np.exp(rng.uniform(np.log(2.0), np.log(300.0), (na, 2)))).float()
    for thr in (4.0, 2.91):
        nb, nx, fs, best = R.anchor_metric(wh, k, thr)
        m = A.anchor_metric(wh, k, thr, return_best=True)
        assert torch.equal(m.best.cpu(), best)
        assert (m.n, m.n_best, m.n_above) == (n, nb, nx)
        assert m.fitness_sum == fs
        assert m.bpr == nb / n and m.aat == nx / n and m.fitness == fs / n


def test_metric_of_placeholder_and_coco_anchors_equals_the_recorded_counts(golden):
    from somi_amd import autoanchor as A
    for name in SETS:
        g = golden('autoanchor_' + name)
        ds = label_set(g)
        seed(0)
        scale = np.random.uniform(0.9, 1.1, size=(len(ds.shapes), 1))
        wh = torch.tensor(R.label_wh(ds, 640, scale)).float()
        n = int(g['n'])
        coco = [[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]]
        for tag, anchors in (('placeholder', [[2 * i, 2 * i + 1] for i in range(n // 3)] * 3), ('coco', coco)):
            m = A.anchor_metric(wh, torch.tensor(anchors).float(), 4.0)           # the placeholder has a zero width: x = 0 for it, as on the CPU
            assert [m.n_best, m.n_above] == g[tag + '_counts'].tolist()
            assert np.float32(m.n_best) / np.float32(m.n) == np.float32(g[tag + '_bpr_aat'][0])


# ---------------------------------------------------------------------------------------------------------------- 2. k-means
@pytest.mark.parametrize('name', SETS)
def test_lloyd_from_a_given_start_follows_scipy(golden, name):
    """1e-9 absolute in whitened units: the only freedom is the order of fp64 sums over n <= 1e5 values of order 1, at most n * 2^-53 ~ 1e-11."""
    from somi_amd import autoanchor as A
    g = golden('autoanchor_' + name)
    _, wh = fit_labels(label_set(g))
    obs = wh / wh.std(0)
    (book, dist, steps), = A.lloyd(obs, obs[g['lloyd_start']][None])
    ref_book, ref_dist, ref_steps = R.lloyd(obs, obs[g['lloyd_start']])
    print(f'{name}: {steps} steps, max |book - scipy| {np.abs(book - g["lloyd_book"]).max():.3g}, |dist - scipy| {abs(dist - float(g["lloyd_dist"])):.3g}')
    assert book.shape == g['lloyd_book'].shape and steps == ref_steps
    assert np.abs(book - g['lloyd_book']).max() <= 1e-9 and abs(dist - float(g['lloyd_dist'])) <= 1e-9


@pytest.mark.parametrize('name', SETS)
def test_kmeans_of_30_restarts_follows_scipy(golden, name):
    from somi_amd import autoanchor as A
    g = golden('autoanchor_' + name)
    _, wh = fit_labels(label_set(g))
    obs = wh / wh.std(0)
    seed(0)
    k, dist = A.kmeans(obs, int(g['n']), iter=30)
    state = np.random.get_state()
    print(f'{name}: max |book - scipy| {np.abs(k - g["kmeans_white"]).max():.3g}, |dist - scipy| {abs(dist - float(g["kmeans_dist"])):.3g}')
    assert k.shape == g['kmeans_white'].shape
    assert np.abs(k - g['kmeans_white']).max() <= 1e-9 and abs(dist - float(g['kmeans_dist'])) <= 1e-9
    assert np.array_equal(state[1], g['kmeans_np_state'][:624]) and state[2] == int(g['kmeans_np_state'][624])
    seed(0)
    k2, dist2 = A.kmeans(obs, int(g['n']), iter=30)
    assert np.array_equal(k, k2) and dist == dist2


def test_lloyd_drops_a_code_without_members():
    """Two equal start codes: the second never wins an assignment (first minimum), leaves the book like in scipy's _kmeans, and the rest goes on."""
    from somi_amd import autoanchor as A
    rng = np.random.RandomState(5)
    obs = np.concatenate([rng.normal(c, 0.2, (700, 2)) for c in ((0, 0), (3, 0), (0, 3))])
    start = np.stack([obs[0], obs[0], obs[800], obs[1500]])
    (book, dist, steps), = A.lloyd(obs, start[None])
    ref_book, ref_dist, ref_steps = R.lloyd(obs, start)
    assert book.shape == ref_book.shape == (3, 2) and steps == ref_steps
    assert np.abs(book - ref_book).max() <= 1e-9 and abs(dist - ref_dist) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- 3. evolution
@pytest.mark.parametrize('name', SETS)
def test_evolution_from_the_recorded_kmeans_result_is_bit_identical(golden, name):
    """Accepted generations and final k: equal to the restatement and to what the reference recorded, bit for bit."""
    from somi_amd import autoanchor as A
    g = golden('autoanchor_' + name)
    _, wh = fit_labels(label_set(g))
    k0 = g['kmeans_white'] * wh.std(0)
    k0 = k0[np.argsort(k0.prod(1))]
    whf = torch.tensor(wh, dtype=torch.float32)
    set_np_state(g['kmeans_np_state'])
    random.seed(0)
    v = A.draw_mutations(1000, k0.shape)
    k, f, accepted = A.evolve(whf, k0, v, 4.0)
    k_ref, f_ref, accepted_ref = R.evolve(k0, whf, 4.0, v)
    assert accepted == accepted_ref and np.array_equal(k, k_ref) and f == f_ref
    assert accepted == g['accepted'].tolist()
    assert np.array_equal(k[np.argsort(k.prod(1))], g['final_anchors'])
    k2, f2, accepted2 = A.evolve(whf, k0, v, 4.0)
    assert np.array_equal(k, k2) and f == f2 and accepted == accepted2


def test_evolution_of_16_anchors_equals_the_restatement(golden):
    """n = 16 (the SOMI head) on set a - the combination where exact-sum and fp32-mean fitness part ways, so only the restatement is the yardstick."""
    from somi_amd import autoanchor as A
    g = golden('autoanchor_a')
    _, wh = fit_labels(label_set(g))
    whf = torch.tensor(wh, dtype=torch.float32)
    rng = np.random.RandomState(2)
    k0 = wh[rng.choice(len(wh), 16, replace=False)]
    seed(3)
    v = A.draw_mutations(300, k0.shape)
    k, f, accepted = A.evolve(whf, k0, v, 4.0)
    k_ref, f_ref, accepted_ref = R.evolve(k0, whf, 4.0, v)
    assert len(accepted) > 10 and accepted == accepted_ref and np.array_equal(k, k_ref) and f == f_ref


# ---------------------------------------------------------------------------------------------------------------- 4. kmean_anchors
@pytest.mark.parametrize('name', SETS)
def test_kmean_anchors_end_to_end_lands_inside_the_references_spread(golden, name):
    from somi_amd import autoanchor as A
    g = golden('autoanchor_' + name)
    ds = label_set(g)
    seed(0)
    k = A.kmean_anchors(ds, n=int(g['n']), img_size=640, thr=4.0, gen=1000, verbose=False)
    state, pstate = np.random.get_state(), random.getstate()
    assert k.shape == (int(g['n']), 2) and k.dtype == np.float64 and (np.diff(k.prod(1)) >= 0).all()
    wh0, wh = fit_labels(ds)
    whf = torch.tensor(wh, dtype=torch.float32)
    fitness = R.fitness_sum(k, whf, 4.0) / len(whf)
    nb = R.anchor_metric(wh0, k, 4.0)[0]
    bpr = float(np.float32(nb) / np.float32(len(wh0)))
    print(f'{name}: fitness {fitness:.5f} (reference seeds {g["seed_fitness"].min():.5f} .. {g["seed_fitness"].max():.5f}), BPR {bpr:.4f} '
          f'(reference {g["seed_bpr"].min():.4f} .. {g["seed_bpr"].max():.4f}), max |k - reference| {np.abs(k - g["final_anchors"]).max():.3g} px')
    assert fitness >= g['seed_fitness'].min() and bpr >= g['seed_bpr'].min()
    assert np.array_equal(state[1], g['final_np_state'][:624]) and state[2] == int(g['final_np_state'][624])
    assert np.array_equal(np.array(pstate[1], dtype=np.uint64), g['final_py_state'])
    seed(0)
    assert np.array_equal(A.kmean_anchors(ds, n=int(g['n']), img_size=640, thr=4.0, gen=1000, verbose=False), k)


# ---------------------------------------------------------------------------------------------------------------- 5. check_anchors
def _models():
    from somi_amd.configs import somi_cfg, yolov10_cfg
    return {'somi': (lambda anchors: somi_cfg(0.25, 0.33, anchors=anchors), 4, 4), 'yolov10': (lambda anchors: yolov10_cfg(0.25, 0.33, anchors=anchors), 3, 3)}


@pytest.mark.parametrize('which', ['somi', 'yolov10'])
def test_check_anchors_replaces_the_placeholder_of_a_real_model(golden, which, tmp_path, monkeypatch):
    from somi_amd import autoanchor as A
    from somi_amd.configs import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.loss import ComputeLoss
    from somi_amd.model import Model
    cfg, na, nl = _models()[which]
    g = golden('autoanchor_a')
    ds = label_set(g)
    model = fill_state(Model(cfg(na)), 1).cuda().eval()
    det = model.model[-1]
    assert det.anchors.shape == (nl, na, 2) and (det.anchors[:, 0, 0] == 0).all()                 # the placeholder: list(range(2 * na)) per level
    imgs, _ = synthetic_batch(2, 64, seed=0)
    with torch.no_grad():
        z_old, _ = model(imgs.cuda())                    # leaves the head's cached host copy of the anchors behind
    old_anchors = det.anchors.clone()
    seed(0)
    out = A.check_anchors(ds, model, thr=4.0, imgsz=640, save_dir=str(tmp_path))
    assert out.replaced and out.new_bpr > out.bpr and out.new_bpr >= 0.98
    if which == 'yolov10':                               # list(range(6)) on three levels: the placeholder the fixture recorded
        assert f'{out.bpr:.4f} {out.aat:.2f}' == '0.3098 1.11'
    assert not torch.equal(det.anchors, old_anchors) and det.anchors.is_cuda
    px = (det.anchors * det.stride.to(det.anchors.device).view(-1, 1, 1)).cpu()
    assert np.array_equal(px.view(-1, 2).numpy(), out.anchors)                                   # the strides are powers of two: exact both ways
    area = px.prod(-1).view(-1)
    assert (area[1:] >= area[:-1]).all() and (det.stride[1:] > det.stride[:-1]).all()            # small to large, with the stride
    lines = open(tmp_path / 'new_anchors.txt').read().split('\n')
    assert len(lines) == nl * na + 1 and [float(v) for v in lines[0].split()] == out.anchors[0].tolist()
    # the eval forward decodes with the new anchors: equal to a model that was built with them
    twin = fill_state(Model(cfg(px.view(nl, -1).tolist())), 1).cuda().eval()
    assert torch.equal(twin.model[-1].anchors, det.anchors)
    with torch.no_grad():
        z_new, _ = model(imgs.cuda())
        z_twin, _ = twin(imgs.cuda())
    assert torch.equal(z_new, z_twin) and not torch.equal(z_new, z_old)
    # a loss built afterwards reads the new anchors
    model.hyp = dict(HYP_VISDRONE)
    assert torch.equal(ComputeLoss(model)._anchors(det.anchors.device), det.anchors)
    # second call: the anchors recall enough, nothing changes and no search is launched
    monkeypatch.setattr(A, 'kmean_anchors', lambda *a, **k: (_ for _ in ()).throw(AssertionError('kmean_anchors launched')))
    monkeypatch.setattr(A, 'kmeans', lambda *a, **k: (_ for _ in ()).throw(AssertionError('k-means launched')))
    kept = det.anchors.clone()
    again = A.check_anchors(ds, model, thr=4.0, imgsz=640, save_dir=str(tmp_path / 'nowhere'))
    assert not again.replaced and again.bpr >= 0.98 and again.new_bpr is None and torch.equal(det.anchors, kept)
    assert not (tmp_path / 'nowhere').exists()


def test_device_image_cache_goes_into_check_anchors(golden):
    """A DeviceImageCache carries `.shapes` and `.labels`: it is a data set for kmean_anchors as it stands."""
    from somi_amd import autoanchor as A
    from somi_amd.augment import DeviceImageCache
    g = golden('autoanchor_a')
    ds = label_set(g)
    n_img = 40
    imgs = [np.zeros((8, 8, 3), np.uint8)] * n_img
    cache = DeviceImageCache(imgs, ds.labels[:n_img], img_size=8, augment=False, shapes=g['shapes'][:n_img])
    sub = R.LabelSet(g['wh_norm'][:int(g['counts'][:n_img].sum())], g['counts'][:n_img], g['shapes'][:n_img])
    seed(1)
    k = A.kmean_anchors(cache, n=6, img_size=640, thr=4.0, gen=50, verbose=False)
    seed(1)
    assert np.array_equal(k, A.kmean_anchors(sub, n=6, img_size=640, thr=4.0, gen=50, verbose=False))
