"""CPU-side checks of the NMS variants: the plain-torch restatements (tests/nms_variants_ref.py) retrace the reference's own `NMS`,
`soft_nms` and merge-NMS on the fixture tools/gen_nms_variants_golden.py wrote, the fixture meets the margin condition, the new C entries
are declared, exported and bound, and the argument errors are raised before any device is needed."""
import ctypes
import os
import re

import pytest
import torch

import nms_variants_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
NEW_SYMBOLS = ('somi_nms_ex_workspace_bytes', 'somi_nms_ex_f32', 'somi_nms_boxes_workspace_bytes', 'somi_nms_boxes_f32')


@pytest.mark.parametrize('mode', R.PENALISED)
def test_penalised_restatement_retraces_the_reference(golden, mode):
    g = golden('nms_variants')
    boxes, scores, thr = T(g['nms_boxes']), T(g['nms_scores']), float(g['nms_thr'])
    assert scores.unique().numel() == scores.numel()            # the reference's argsort is not stable: no exact ties in its fixture
    m = {}
    keep = R.penalised_nms(boxes, scores, thr, mode, margins=m)
    assert torch.equal(keep, T(g[f'nms_keep_{mode}']))
    assert 0 < keep.numel() < scores.numel()
    assert m['thr'] == float(g[f'nms_margin_{mode}']) >= R.MIN_MARGIN


@pytest.mark.parametrize('tag', ['soft_a', 'soft_b'])
def test_soft_restatement_retraces_the_reference(golden, tag):
    g = golden('nms_variants')
    boxes, scores = T(g[f'{tag}_boxes']), T(g[f'{tag}_scores'])
    thr, sigma, sthr = (float(v) for v in g[f'{tag}_params'])
    want_keep, want_scores = T(g[f'{tag}_keep']), T(g[f'{tag}_decayed'])
    m, s = {}, scores.clone()
    keep = R.soft_nms(boxes, s, thr, sigma, sthr, drop_last=True, margins=m)
    assert torch.equal(keep, want_keep) and torch.equal(s, want_scores)
    assert want_keep.numel() > 10 and not torch.equal(want_scores, scores)
    assert [m['thr'], m['score'], m['gap']] == [float(v) for v in g[f'{tag}_margins']]
    assert min(m.values()) >= R.MIN_MARGIN
    # the kept form: the same picks plus at most the one candidate the reference leaves its loop with
    s2 = scores.clone()
    kept = R.soft_nms(boxes, s2, thr, sigma, sthr)
    assert kept.numel() - want_keep.numel() in (0, 1) and torch.equal(kept[:want_keep.numel()], want_keep)
    assert torch.equal(s2[want_keep], want_scores[want_keep])


def test_soft_restatement_on_one_and_two_boxes():
    """The reference returns [] for a single box; the kept form returns it.  With two boxes the reference keeps the first only."""
    b = torch.tensor([[10., 10., 50., 60.], [25., 10., 65., 60.]])
    assert R.soft_nms(b[:1], torch.tensor([0.9]), drop_last=True).tolist() == []
    assert R.soft_nms(b[:1], torch.tensor([0.9])).tolist() == [0]
    assert R.soft_nms(b, torch.tensor([0.9, 0.8]), drop_last=True).tolist() == [0]
    s = torch.tensor([0.9, 0.8])
    assert R.soft_nms(b, s).tolist() == [0, 1] and 0.25 < float(s[1]) < 0.8


def test_merge_restatement_retraces_the_reference(golden):
    g = golden('nms_variants')
    pred = T(g['merge_pred'])
    kw = dict(conf_thres=0.02, iou_thres=0.5, multi_label=True)
    info, m = [], {}
    got = R.non_max_suppression(pred.clone(), merge=True, info=info, margins=m, **kw)
    got64 = R.non_max_suppression(pred.clone(), merge=True, dtype=torch.float64, **kw)
    plain = R.non_max_suppression(pred.clone(), **kw)
    assert [r['n'] for r in info] == g['merge_n'].tolist() and 1 < info[0]['n'] < 3000 <= info[1]['n']
    assert m['merge'] == float(g['merge_margin']) >= R.MIN_MARGIN
    for b in range(2):
        want = T(g[f'merge_out{b}'])
        assert got[b].shape == want.shape and torch.equal(got[b][:, 4:], want[:, 4:])          # membership, conf, class
    assert torch.equal(got[1], T(g['merge_out1'])) and torch.equal(got[1], plain[1])           # outside the window: unmerged
    assert got[0].shape[0] < plain[0].shape[0]                                                 # `redundant` dropped the singletons
    # each merged coordinate of the reference within the worst case of a k-term non-negative weighted mean in fp32
    size = info[0]['size'].double()
    bound = (size + 8)[:, None] * 2.0 ** -24 * info[0]['xmax']
    assert ((T(g['merge_out0'])[:, :4].double() - got64[0][:, :4]).abs() <= bound).all()
    assert size.max() >= 4


def test_new_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    from somi_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert 'SOMI_ABI_VERSION 15' in re.sub(r'\s+', ' ', hdr) and _lib.ABI_VERSION == 15
    lib = _lib.lib()
    base = lib.somi_nms_workspace_bytes(2, 1000, 10, 1)
    assert lib.somi_nms_ex_workspace_bytes(2, 1000, 10, 1, 0, 0) == base
    assert lib.somi_nms_ex_workspace_bytes(2, 1000, 10, 1, 6, 0) > base < lib.somi_nms_ex_workspace_bytes(2, 1000, 10, 1, 2, 1)
    assert lib.somi_nms_boxes_workspace_bytes(0) == 0 < lib.somi_nms_boxes_workspace_bytes(100)


def test_mode_table_matches_the_header():
    from somi_amd import nms
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    for name, code in nms.MODES.items():
        assert re.search(rf'SOMI_NMS_{name.upper()} = {code}\b', hdr), name
    assert tuple(nms.MODES) == R.MODES


def test_argument_errors():
    from somi_amd.nms import NMS, non_max_suppression, non_max_suppression_raw, soft_nms
    p = torch.zeros(1, 10, 15)
    for f in (non_max_suppression, non_max_suppression_raw):
        with pytest.raises(ValueError, match='unknown NMS mode'):
            f(p, nms='WIoU')
        with pytest.raises(NotImplementedError, match="nms='soft'"):
            f(p, nms='soft', merge=True)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            f(p, nms='DIoU')
        with pytest.raises(TypeError):
            f(p, 0.25, 0.45, None, False, False, (), 300, 'DIoU')                              # keyword-only
    boxes, scores = torch.zeros(4, 4), torch.zeros(4)
    with pytest.raises(ValueError, match='unknown NMS mode'):
        NMS(boxes, scores, 0.5, class_nms='nope')                                              # the reference would run SIoU
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        NMS(boxes, scores, 0.5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        soft_nms(boxes, scores)


def test_val_run_passes_the_selection_rule_through():
    import inspect
    from somi_amd import val
    sig = inspect.signature(val.run)
    assert sig.parameters['nms'].default == 'iou' and sig.parameters['merge'].default is False
    assert re.search(r'non_max_suppression\(.*nms=nms, merge=merge\)', inspect.getsource(val.run))
