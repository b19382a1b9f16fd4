"""Writes tests/golden/autoanchor_{a,b}.npz: synthetic label sets and what the reference's utils/autoanchor.py (with the installed scipy) makes of them.

    python tools/gen_autoanchor_golden.py --reference /path/to/the/reference/checkout

The reference module is imported with `utils.general` stubbed in sys.modules (only `colorstr` is used; the real module pulls in cv2).  Nothing of the
reference is copied: the fixtures hold the inputs (normalised label sizes as fp32, boxes per image, image shapes) and recorded results.  Recorded at
`np.random.seed(0); random.seed(0)`:
  * BPR / anchors-above-threshold of the placeholder anchors and of the COCO anchors after check_anchors' `uniform(0.9, 1.1)` draw (computed here with
    the reference's formula and checked against the rounded figures the reference prints);
  * scipy's `kmeans` return value inside `kmean_anchors` (captured by wrapping scipy.cluster.vq.kmeans), and a single Lloyd run from a given start;
  * the mutation draws (captured by wrapping the three generator calls), the accepted generations (the reference sets `pbar.desc` exactly when it
    accepts: a stand-in for tqdm records them) and the final anchors;
  * the positions of both global generators after each stage;
  * final fitness and BPR for seeds 0..5.
It then checks the condition the tests rely on - from the reference's own k-means result, tests/autoanchor_ref.py (exact-sum fitness) and the reference
(fp32 mean) accept the same generations and end on bit-identical anchors - and refuses to write a fixture that fails it: change the set's seed or
size then, not the test.
"""
import argparse
import contextlib
import io
import os
import random
import re
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import autoanchor_ref as R  # noqa: E402

SETS = {'a': dict(n_img=200, seed=0, n=9), 'b': dict(n_img=600, seed=0, n=12)}
COCO = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
STRIDES = [8., 16., 32.]
N_V = 200            # mutation matrices kept in the fixture (the generator positions pin the rest)


def import_reference(path):
    general = types.ModuleType('utils.general')
    general.colorstr = lambda *a: a[-1]
    sys.path.insert(0, path)
    import utils  # noqa: F401  (the reference's package)
    sys.modules['utils.general'] = general
    import utils.autoanchor as AA
    return AA


class Recorder:
    """Stand-in for tqdm: iterates, and notes the generation whenever the loop body assigns `desc`."""
    accepted = None

    def __init__(self, it, desc=''):
        self.__dict__['it'], self.__dict__['g'] = it, -1
        Recorder.accepted = []

    def __iter__(self):
        for g in self.it:
            self.__dict__['g'] = g
            yield g

    def __setattr__(self, name, value):
        if name == 'desc':
            Recorder.accepted.append(self.g)
        self.__dict__[name] = value


def np_state():
    s = np.random.get_state()
    return np.concatenate([s[1].astype(np.uint32), np.array([s[2]], dtype=np.uint32)])


def py_state():
    return np.array(random.getstate()[1], dtype=np.uint64)


def head(anchors):
    m = types.SimpleNamespace(anchors=torch.tensor(anchors).float().view(len(anchors), -1, 2), stride=torch.tensor(STRIDES))
    m.anchors /= m.stride.view(-1, 1, 1)
    return m


def quiet(fn, *a, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **kw)
    return out, buf.getvalue()


def record(AA, name, n_img, seed, n):
    import scipy.cluster.vq as VQ
    wh_norm, counts, shapes = R.synth_label_set(n_img, seed)
    ds = R.LabelSet(wh_norm, counts, shapes)
    rec = dict(wh_norm=wh_norm, counts=counts, shapes=shapes, n=np.int64(n), strides=np.array(STRIDES))
    AA.tqdm = Recorder
    real_kmeans = VQ.kmeans
    captured = {}

    def kmeans_spy(obs, k, **kw):
        captured['obs'] = np.array(obs)
        out = real_kmeans(obs, k, **kw)
        captured['k'], captured['dist'] = np.array(out[0]), float(out[1])
        captured['np_state'] = np_state()
        return out

    VQ.kmeans = kmeans_spy
    draws = []
    real = (np.random.random, np.random.randn, random.random)
    np.random.random = lambda sh: draws.append(('u', real[0](sh))) or draws[-1][1]
    np.random.randn = lambda *sh: draws.append(('n', real[1](*sh))) or draws[-1][1]
    random.random = lambda: draws.append(('r', real[2]())) or draws[-1][1]
    try:
        # ---- kmean_anchors, seeds 0..5
        fits, fits_exact, bprs = [], [], []
        for s in range(6):
            np.random.seed(s), random.seed(s)
            del draws[:]
            k, _ = quiet(AA.kmean_anchors, ds, n=n, img_size=640, thr=4.0, gen=1000, verbose=False)
            wh0 = R.label_wh(ds, 640)
            whf = torch.tensor(wh0[(wh0 >= 2.0).any(1)], dtype=torch.float32)
            _, best = R.metric_terms(whf, torch.tensor(k, dtype=torch.float32))
            fits.append(float((best * (best > 0.25).float()).mean()))
            fits_exact.append(R.fitness_sum(k, whf, 4.0) / len(whf))
            _, best0 = R.metric_terms(torch.tensor(wh0, dtype=torch.float32), torch.tensor(k, dtype=torch.float32))
            bprs.append(float((best0 > 0.25).float().mean()))
            if s == 0:
                rec.update(kmeans_white=captured['k'], kmeans_dist=np.float64(captured['dist']), kmeans_np_state=captured['np_state'],
                           final_anchors=np.array(k), accepted=np.array(Recorder.accepted, dtype=np.int32),
                           final_np_state=np_state(), final_py_state=py_state(), n_fit=np.int64(len(whf)))
                std = wh0[(wh0 >= 2.0).any(1)].std(0)
                k0 = captured['k'] * std
                k0 = k0[np.argsort(k0.prod(1))]
                rec['kmeans_fitness'] = np.float64(R.fitness_sum(k0, whf, 4.0) / len(whf))
                # the reference's mutation factors from its own draws (the last (u, r, n) triple of a generation is the one that was used)
                vs, i = [], 0
                while i < len(draws):
                    (tu, u), (tr, r), (tn, z) = draws[i:i + 3]
                    assert (tu, tr, tn) == ('u', 'r', 'n')
                    v = ((u < 0.9) * r * z * 0.1 + 1).clip(0.3, 3.0)
                    i += 3
                    if not (v == 1).all():
                        vs.append(v)
                assert len(vs) == 1000
                rec['mutations'] = np.stack(vs[:N_V])
                # the condition: restatement from the reference's k-means result
                k1, f1, acc1 = R.evolve(k0, whf, 4.0, np.stack(vs))
                k1 = k1[np.argsort(k1.prod(1))]
                same = acc1 == Recorder.accepted and np.array_equal(k1, k)
                print(f'{name}: {len(whf)} boxes, {len(Recorder.accepted)} accepted generations, restatement follows the reference: {same}, '
                      f'max |dk| = {np.abs(k1 - k).max():.3g}')
                if not same:
                    raise SystemExit(f'set {name} fails the condition (exact-sum and fp32-mean fitness take different branches): change its seed or size')
        rec.update(seed_fitness=np.array(fits), seed_fitness_exact=np.array(fits_exact), seed_bpr=np.array(bprs))
        print(f'{name}: final fitness seeds 0..5 {min(fits):.5f} .. {max(fits):.5f}, k-means alone {float(rec["kmeans_fitness"]):.5f}')

        # ---- one Lloyd run from a given start (scipy's kmeans with an initial book = _kmeans)
        obs = captured['obs']
        idx = np.random.RandomState(7).choice(len(obs), n, replace=False)
        book, dist = real_kmeans(obs, obs[idx])
        rec.update(lloyd_start=idx.astype(np.int64), lloyd_book=np.array(book), lloyd_dist=np.float64(dist))

        # ---- check_anchors: metric of the placeholder and the COCO anchors after the scale draw, and the whole call on the placeholder
        np.random.seed(0), random.seed(0)
        scale = np.random.uniform(0.9, 1.1, size=(n_img, 1))
        rec['check_np_state'] = np_state()
        wh = torch.tensor(R.label_wh(ds, 640, scale)).float()
        nl = 3
        placeholder = [list(range(2 * (n // nl)))] * nl
        for tag, anchors in (('placeholder', placeholder), ('coco', COCO)):
            m = head(anchors)
            x, best = R.metric_terms(wh, (m.anchors * m.stride.view(-1, 1, 1)).view(-1, 2))
            rec[f'{tag}_counts'] = np.array([int((best > 0.25).sum()), int((x > 0.25).sum())], dtype=np.int64)
            bpr, aat = float((best > 0.25).float().mean()), float((x > 0.25).float().sum(1).mean())
            np.random.seed(0), random.seed(0)
            import tempfile
            with tempfile.TemporaryDirectory() as d:
                _, text = quiet(AA.check_anchors, ds, types.SimpleNamespace(model=[m]), thr=4.0, imgsz=640, save_dir=d)
            if tag == 'placeholder':
                rec.update(check_final_np_state=np_state(), check_final_py_state=py_state())     # the anchors themselves are not pinned: see the tests
            got = re.search(r'anchors/target = (\d+\.\d+), Best Possible Recall \(BPR\) = (\d+\.\d+)', text)
            assert got and f'{aat:.2f}' == got.group(1) and f'{bpr:.4f}' == got.group(2), (text[:200], aat, bpr)
            rec[f'{tag}_bpr_aat'] = np.array([bpr, aat])
            print(f'{name}: {tag} anchors BPR {bpr:.4f} / AAT {aat:.2f}')
    finally:
        VQ.kmeans = real_kmeans
        np.random.random, np.random.randn, random.random = real
    out = os.path.join(ROOT, 'tests', 'golden', f'autoanchor_{name}.npz')
    np.savez_compressed(out, **rec)
    print(f'{name}: wrote {out} ({os.path.getsize(out) / 1024:.0f} KB)')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SOMI_REFERENCE'), required=not os.environ.get('SOMI_REFERENCE'))
    ap.add_argument('--sets', default='a,b')
    args = ap.parse_args()
    AA = import_reference(args.reference)
    for name in args.sets.split(','):
        record(AA, name, **SETS[name])
