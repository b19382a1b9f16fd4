"""CPU checks of the slim-neck blocks (GSConv, GSBottleneck, VoVGSCSP: models/common.py:9586-9681; GSCBAMBottleneck, :737-757; VoVGSCSPCBAM,
:2697-2711): the test restatement (tests/slimneck_ref.py) reproduces the reference's own classes through the tests/golden/block_gs*.npz
fixtures, and four plausible wrong restatements do not; the shuffle's index rule is the reference's reshape / permute expression; state-dict
keys and shapes are the restatement's, `res.*` included; the parser gives the oracle Model's layer table for configs.yolov5_slimneck_cfg; the
seeded cases of the GPU tests are the ones the selection rule gives; limits raise by name; the new entry points are declared, bound, exported
and refuse bad arguments without a launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import slimneck_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_gs_tail_nhwc_f32', 'somi_gs_shuffle_affine_act_nhwc_f32', 'somi_gs_unshuffle_nhwc_f32', 'somi_gs_tiles_per_workgroup')

FIXTURES = {'block_gsconv': 'gsconv', 'block_gsconv_s2': 'gsconv_s2', 'block_gsconv_noact': 'gsconv_noact', 'block_gsbottleneck': 'gsbottleneck',
            'block_gsvovgscsp': 'vovgscsp', 'block_gscbam': 'gscbam', 'block_gsvovgscspcbam': 'vovgscspcbam'}
WITH_RES = ('vovgscsp', 'vovgscspcbam')


def _fixture_errors(name, make):
    """-> {mode: max error / max value} of make(R) under fill_state weights against the fixture."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    mod = fill_state(make(R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == R.block_shape(FIXTURES[name])
    assert bool((x * 2 == (x * 2).round()).all()), 'the fixture input lies on a grid of 1/2'
    out = {}
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        assert y.shape == want.shape
        out[mode] = (y - want).abs().max().item() / want.abs().max().item()
    return out


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_restatement_reproduces_the_reference(name):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    for mode, err in _fixture_errors(name, R.BLOCKS[FIXTURES[name]]).items():
        assert err <= 1e-5, f'{name} {mode}: {err:.3e}'
    d = np.load(os.path.join(GOLDEN, 'block_gsconv_s2.npz'))
    assert d['x'].shape[2:] == (9, 6) and d['out_eval'].shape == (2, 48, 5, 3)       # stride 2 over an odd and an even size


def test_wrong_restatements_are_ruled_out():
    """The interleaving channel_shuffle, cat(x1, y) order in VoVGSCSP and a VoVGSCSP that runs `res` each miss a fixture by more than 1e-3 in
    both modes; one depthwise 5x5 in place of the two 3x3s has another parameter count and another state dict."""
    errs = _fixture_errors('block_gsconv', lambda ns: ns.InterleavingGSConv(32, 32, 1, 1))
    assert min(errs.values()) > 1e-3, f'the interleaving shuffle fits the fixture: {errs}'
    errs = _fixture_errors('block_gsconv_noact', lambda ns: ns.InterleavingGSConv(16, 24, 3, 1, act=False))
    assert min(errs.values()) > 1e-3, f'the interleaving shuffle fits the c_ = 12 fixture: {errs}'
    errs = _fixture_errors('block_gsvovgscsp', lambda ns: ns.SwappedVoVGSCSP(32, 32, 1))
    assert min(errs.values()) > 1e-3, f'the swapped concatenation fits the fixture: {errs}'
    errs = _fixture_errors('block_gsvovgscsp', lambda ns: ns.ResVoVGSCSP(32, 32, 1))
    assert min(errs.values()) > 1e-3, f'a VoVGSCSP that runs res fits the fixture: {errs}'
    count = lambda m: sum(p.numel() for p in m.parameters())      # noqa: E731
    two, one = R.GSConv(32, 32, 1, 1), R.OneFiveGSConv(32, 32, 1, 1)
    assert count(two) == 32 * 16 + 2 * 16 + 2 * (16 * 9 + 2 * 16) and count(one) == 32 * 16 + 2 * 16 + 16 * 25 + 2 * 16
    assert 'cv2_1.conv.weight' in two.state_dict() and 'cv2_1.conv.weight' not in one.state_dict()


@pytest.mark.parametrize('b,c_', [(3, 4), (2, 6), (2, 5), (1, 12)])
def test_the_index_rule_is_the_reference_expression(b, c_):
    """models/common.py:9604-9610 on cat(x1, x_2): output channel o reads source 2 o for o < c_, 2 (o - c_) + 1 otherwise; nothing crosses
    images; and it is not the interleave."""
    h, w = 3, 2
    x2 = torch.arange(b * 2 * c_ * h * w, dtype=torch.float32).view(b, 2 * c_, h, w)
    n = 2 * c_
    y = x2.reshape(b * n // 2, 2, h * w).permute(1, 0, 2).reshape(2, -1, n // 2, h, w)
    want = torch.cat((y[0], y[1]), 1)
    src = [2 * o if o < c_ else 2 * (o - c_) + 1 for o in range(n)]
    assert torch.equal(want, x2[:, src]) and torch.equal(want, R.deinterleave(x2))
    assert not torch.equal(want, R.InterleavingGSConv.shuffle(None, x2))


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    makes = list(R.BLOCKS.values()) + [lambda M: M.GSConv(64, 128, 3, 2), lambda M: M.VoVGSCSPCBAM(128, 128, 3, False), lambda M: M.VoVGSCSP(64, 32, 2),
                                       lambda M: M.GSCBAMBottleneck(64, 32), lambda M: M.GSBottleneck(32, 64, e=1.0)]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # a checkpoint of the restatement loads ...
        a.load_state_dict(b.state_dict())                         # ... and ours loads there
    sd = MB.GSConv(32, 48, 3, 2).state_dict()
    assert [k for k in sd if k.endswith('conv.weight')] == ['cv1.conv.weight', 'cv2_1.conv.weight', 'cv2_2.conv.weight']
    assert tuple(sd['cv1.conv.weight'].shape) == (24, 32, 3, 3) and tuple(sd['cv2_1.conv.weight'].shape) == tuple(sd['cv2_2.conv.weight'].shape) == (24, 1, 3, 3)
    blk = MB.VoVGSCSPCBAM(32, 64, 2, False)
    assert [n for n, _ in blk.named_children()] == ['cv1', 'cv2', 'gsb', 'res', 'cv3']
    assert len(blk.gsb) == 2 and all(type(m) is MB.GSCBAMBottleneck and m.add for m in blk.gsb)
    assert [n for n, _ in blk.gsb[0].named_children()] == ['cv1', 'cv2', 'channel_attention', 'spatial_attention']
    assert blk.gsb[0].cv1.cv1.conv.kernel_size == (1, 1) and blk.gsb[0].cv2.cv1.conv.kernel_size == (3, 3)
    assert blk.gsb[0].channel_attention.shared_MLP[0].out_features == 32 // 8 and blk.gsb[0].spatial_attention.cv1.kernel_size == (3, 3)
    assert isinstance(blk.gsb[0].cv1.cv2_2.act, torch.nn.SiLU) and all(isinstance(c.act, torch.nn.Identity) for c in blk.gsb[0].cv2.children())
    assert {'res.conv.weight', 'res.bn.weight', 'res.bn.bias', 'res.bn.running_mean', 'res.bn.running_var', 'res.bn.num_batches_tracked'} <= set(blk.state_dict())
    assert tuple(blk.res.conv.weight.shape) == (32, 32, 3, 3) and isinstance(blk.res.act, torch.nn.Identity)
    gsb = MB.VoVGSCSP(32, 32, 1).gsb[0]
    assert type(gsb) is MB.GSBottleneck and [n for n, _ in gsb.named_children()] == ['conv_lighting', 'shortcut']
    assert isinstance(gsb.shortcut.act, torch.nn.Identity) and gsb.conv_lighting[1].cv1.conv.kernel_size == (3, 3)


def test_contract_and_limits_are_explicit():
    from somi_amd import blocks as MB
    for cls in (MB.GSConv, MB.GSBottleneck, MB.VoVGSCSP, MB.GSCBAMBottleneck, MB.VoVGSCSPCBAM):
        assert cls.accumulates is False and cls.folds_pooled is False, cls.__name__
        assert list(inspect.signature(cls.backward).parameters)[2:5] == ['dx_out', 'accumulate', 'need_dx'], cls.__name__
    for cls in (MB.GSBottleneck, MB.VoVGSCSP, MB.GSCBAMBottleneck, MB.VoVGSCSPCBAM):
        assert cls.reduction == 1, cls.__name__
    assert not issubclass(MB.GSConv, MB.Conv) and MB.Conv.accumulates is True
    assert MB.GSConv.__dict__['accumulates'] is False and MB.GSConv.__dict__['folds_pooled'] is False
    assert MB.GSConv(32, 48, 3, 2).reduction == 2 and MB.GSConv(32, 32).reduction == 1
    assert list(inspect.signature(MB.GSConv.forward).parameters) == ['self', 'x', 'out', 'residual']
    assert list(inspect.signature(MB.GSConv.__init__).parameters) == ['self', 'c1', 'c2', 'k', 's', 'p', 'g', 'd', 'act']
    assert MB.VoVGSCSP.never_runs == MB.VoVGSCSPCBAM.never_runs == ('res',)
    for mode in (True, False):
        with pytest.raises(NotImplementedError, match=r'GSConv half width 6 \(c2 // 2\) must be a multiple of 4'):
            MB.GSConv(8, 12).train(mode)(MB.Act(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(NotImplementedError, match='VoVGSCSP hidden width 6 must be a multiple of 4'):
        MB.VoVGSCSP(8, 12, 1).eval()(MB.Act(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(NotImplementedError, match='VoVGSCSPCBAM hidden width 10 must be a multiple of 4'):
        MB.VoVGSCSPCBAM(16, 20, 1).eval()(MB.Act(torch.zeros(1, 4, 4, 16)))
    with pytest.raises(NotImplementedError, match='GSConv half width 2'):      # the CBAM bottleneck's hidden width 4 halves to 2
        MB.GSCBAMBottleneck(8, 8, ratio=2).eval()(MB.Act(torch.zeros(1, 4, 4, 8)))
    with pytest.raises(NotImplementedError, match='grouped Conv with k=3, s=1, p=0'):
        MB.GSConv(8, 16, 3, 1, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        MB.GSConv(8, 16).eval()(MB.Act(torch.zeros(1, 4, 4, 8)))


def test_parser_placement_and_optimizer_groups():
    """GSConv in the (c1, c2, ...) branch, VoVGSCSPCBAM there and repeated inside (models/yolo.py:1473-1474, 1489); VoVGSCSP, GSBottleneck and
    GSCBAMBottleneck are in none of the reference's lists and stay outside.  train.py:125-133 puts `res` in the groups like every parameter;
    what keeps a step from moving it is that it never has a gradient, which the block declares (never_runs)."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_slimneck_cfg
    from somi_amd.model import Model, _CH, _REPEAT_INSIDE
    from somi_amd.optim import reference_param_groups
    assert _CH['GSConv'] is MB.GSConv and _CH['VoVGSCSPCBAM'] is MB.VoVGSCSPCBAM
    assert 'VoVGSCSPCBAM' in _REPEAT_INSIDE and 'GSConv' not in _REPEAT_INSIDE
    for name in ('VoVGSCSP', 'GSBottleneck', 'GSCBAMBottleneck'):
        assert name not in _CH
        cfg = yolov5_slimneck_cfg(0.25, 0.33, nc=4)
        cfg['head'][3][2] = name
        with pytest.raises(NotImplementedError, match=f"module '{name}' is outside the SOMI hot path"):
            Model(cfg)
    for tag, mk in R.BLOCKS.items():
        m, r = mk(MB), mk(R)
        names = {id(p): n for n, p in m.named_parameters()}
        g0, g1, g2 = ([names[id(p)] for p in g] for g in reference_param_groups(m))
        assert sorted(g0 + g1 + g2) == sorted(names.values()), 'a parameter is in no group'
        assert all(n.endswith('.bias') for n in g2) and all(n.endswith('bn.weight') for n in g0)
        assert any(n.endswith('cv2_1.conv.weight') for n in g1) and any(n.endswith('cv2_2.conv.weight') for n in g1)
        rnames = {id(p): n for n, p in r.named_parameters()}
        assert [[rnames[id(p)] for p in g] for g in reference_param_groups(r)] == [g0, g1, g2]
        if tag in WITH_RES:
            assert 'res.conv.weight' in g1 and 'res.bn.weight' in g0 and 'res.bn.bias' in g2
            assert [n for n, _ in getattr(m, m.never_runs[0]).named_parameters()] == ['conv.weight', 'bn.weight', 'bn.bias']
            assert 'channel_attention.shared_MLP.0.weight' in ' '.join(g1) or tag == 'vovgscsp'


def test_slimneck_graph_matches_the_oracle(monkeypatch):
    """The same layer table, state dict and parameter count as the oracle Model, n > 1 inside VoVGSCSPCBAM included."""
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cfg, yolov5_slimneck_cfg
    from somi_amd.model import Model
    from oracle.somi_ref import Model as OModel
    R.register(monkeypatch)
    for width, depth in ((0.25, 0.33), (0.25, 0.67)):
        cfg = yolov5_slimneck_cfg(width, depth, nc=4)
        ref, mine = OModel(cfg), Model(cfg)
        want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
        got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
        assert list(got) == list(want)
        assert got == want
        assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
        assert [m.np for m in mine.model] == [m.np for m in ref.model]
        assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
        assert mine.save == ref.save and [(m.i, m.f, m.type) for m in mine.model] == [(m.i, m.f, m.type) for m in ref.model]
        mine.load_state_dict(ref.state_dict())
        ref.load_state_dict(mine.state_dict())
        assert mine.fuse() is mine
        n = 1 if depth == 0.33 else 2
        assert [type(mine.model[i]) for i in (10, 14, 18, 21)] == [MB.GSConv] * 4
        assert [type(mine.model[i]) for i in (13, 17, 20, 23)] == [MB.VoVGSCSPCBAM] * 4 and [len(mine.model[i].gsb) for i in (13, 17, 20, 23)] == [n] * 4
        assert [mine.model[i].reduction for i in (10, 14, 18, 21)] == [1, 1, 2, 2]
        assert f'model.17.gsb.{n - 1}.cv2.cv2_2.bn.running_var' in got and 'model.23.res.bn.num_batches_tracked' in got
    base, cfg = yolov5_cfg(0.25, 0.33, nc=4), yolov5_slimneck_cfg(0.25, 0.33, nc=4)
    assert cfg['backbone'] == base['backbone'] and cfg['head'][-1] == base['head'][-1]
    assert [r[:2] + r[3:] for r in cfg['head']] == [r[:2] + r[3:] for r in base['head']]
    swapped = [(a[2], b[2]) for a, b in zip(base['head'], cfg['head']) if a[2] != b[2]]
    assert swapped == [('Conv', 'GSConv'), ('C3', 'VoVGSCSPCBAM')] * 4


def test_cfg_defaults_and_the_other_cfgs_are_unchanged():
    from somi_amd import configs
    from somi_amd.model import Model
    cfg = configs.yolov5_slimneck_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, configs.COCO_ANCHORS)
    assert list(inspect.signature(configs.yolov5_slimneck_cfg).parameters) == ['width', 'depth', 'nc', 'anchors']
    assert [r[2] for r in cfg['head']] == ['GSConv', 'nn.Upsample', 'Concat', 'VoVGSCSPCBAM', 'GSConv', 'nn.Upsample', 'Concat', 'VoVGSCSPCBAM',
                                           'GSConv', 'Concat', 'VoVGSCSPCBAM', 'GSConv', 'Concat', 'VoVGSCSPCBAM', 'Detect']
    others = [configs.yolov5_cfg(), configs.yolov5_cfg(version='5.0'), configs.yolov5_ghost_cfg(), configs.yolov5_cpca_cfg(), configs.yolov5_asf_cfg(),
              configs.yolov5_swin_cfg(), configs.yolov10_cfg(), configs.somi_cfg()]
    assert all('GS' not in r[2] for c in others for r in c['backbone'] + c['head'])
    cfg = configs.yolov5_slimneck_cfg(0.25, 0.33, nc=4)
    cfg['backbone'][8][2] = 'C3TR'                                # stays outside
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


def test_block_seeds_are_the_ones_the_rule_gives():
    """slimneck_ref.BLOCK_SEEDS: per block the first of the seeds 0..7 whose fp32-against-fp64 figure is below half the bar and whose smallest
    attention-maximum gap is at least MIN_GAP - computed from the restatement alone."""
    for tag in R.BLOCKS:
        for seed in range(8):
            gap, bars = R.block_figures(tag, seed)
            print(f'{tag} seed {seed}: max gap {gap:.3e}, fp32 against fp64 {bars:.3f} x the bar')
            if bars < 0.5 and gap >= R.MIN_GAP:
                break
        assert R.BLOCK_SEEDS[tag] == seed, f'{tag}: the rule gives seed {seed}'
    assert R.block_figures('gsconv')[0] == float('inf') and R.block_figures('gscbam')[0] < 1.0       # only the attention blocks take a maximum


def test_the_graph_case_is_one_the_fp32_oracle_can_be_judged_on(monkeypatch):
    """slimneck_ref.GRAPH_SEEDS is the FIRST of the candidates (fill 1..4) x (batch 0..3) at which the fp32 CPU oracle's parameter gradients are
    below half check_train_step's bar (2e-3 * scale + 2e-6) against its own fp64 twin's and no maximum an attention of the fp64 oracle takes is
    closer than MIN_GAP to the runner-up: every candidate before it misses one of the two."""
    R.register(monkeypatch)
    for cand in ((fill, batch) for fill in range(1, 5) for batch in range(4)):
        gap, bars = R.graph_figures('slimneck', cand)
        print(f'slimneck {cand}: max gap {gap:.3e}, fp32 oracle against fp64 at {bars:.3f} x the bar')
        if gap >= R.MIN_GAP and bars < 0.5:
            break
    assert R.GRAPH_SEEDS['slimneck'] == cand, f'the rule gives {cand}'


def test_new_symbols_are_declared_bound_and_exported():
    from somi_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/somi_hip.h'
        assert name in _lib.SIGNATURES, f'{name} is not bound in _lib.SIGNATURES'
        assert hasattr(L, name), f'{name} is not exported'
        proto = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert not re.search(r'_coff\b', proto), f'{name} takes a slice as loose *_coff parameters'
    assert '#define SOMI_ABI_VERSION 15' in hdr and _lib.lib().somi_abi_version() == _lib.ABI_VERSION == 15
    for fn in ('gs_tail', 'gs_shuffle_affine_act', 'gs_unshuffle', 'gs_tiles_per_workgroup'):
        assert callable(getattr(ops, fn))
    mk = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()
    assert 'gsconv.hip' in mk
    src = open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'gsconv.hip')).read()
    assert 'SOMI_REQUIRE_SLICES' in src and not re.search(r'\batomic[A-Z]\w*\b', src)


BREAKS = [('pointer + 4 bytes', lambda s: setattr(s, 'p', s.p + 4)), ('pointer NULL', lambda s: setattr(s, 'p', None)),
          ('coff = -4', lambda s: setattr(s, 'coff', -4)), ('past the stride', lambda s: setattr(s, 'coff', s.cs - 4)),
          ('coff + 2', lambda s: setattr(s, 'coff', s.coff + 2)), ('cs + 2', lambda s: setattr(s, 'cs', s.cs + 2))]


def _calls(_lib, L):
    """name -> (call(slices, **scalars), the slice names in argument order, which of them are optional): made-up addresses, Ch = 8."""
    S = _lib.Slice
    w = dict(w1=0xA0000, b1=0xB0000, w2=0xC0000, b2=0xD0000, w_cs=8, act=1, B=1, H=4, W=6, Ch=8, npix=24, scale=0xE0000, shift=0xF0000)

    def tail(s, **k):
        a = dict(w, **k)
        return L.somi_gs_tail_nhwc_f32(s['x1'], a['w1'], a['b1'], a['w2'], a['b2'], a['w_cs'], a['act'], s['out'], s['residual'], a['B'], a['H'], a['W'],
                                       a['Ch'], None)

    def shuffle(s, **k):
        a = dict(w, **k)
        return L.somi_gs_shuffle_affine_act_nhwc_f32(s['z1'], s['y2'], a['scale'], a['shift'], a['act'], s['out'], s['residual'], a['npix'], a['Ch'], None)

    def unshuffle(s, **k):
        a = dict(w, **k)
        return L.somi_gs_unshuffle_nhwc_f32(s['dout'], s['d1'], s['d2'], a['npix'], a['Ch'], None)
    make = lambda names: {n: S(0x10000 * (i + 1), 24, 4) for i, n in enumerate(names)}     # noqa: E731  width 8 or 16 from offset 4 of 24
    return {'gs tail': (tail, lambda: make(('x1', 'out', 'residual')), ('residual',)),
            'gs shuffle': (shuffle, lambda: make(('z1', 'y2', 'out', 'residual')), ('residual',)),
            'gs unshuffle': (unshuffle, lambda: make(('dout', 'd1', 'd2')), ())}


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    """Every slice an entry point reads or writes, broken in six ways, is SOMI_EINVAL with a message that names it (an optional slice without a
    pointer is no slice); a half width that is no multiple of 4, empty sizes, an unknown activation, misaligned or missing weights and a scale
    without a shift are refused by name.  A rejected call launches nothing, so the made-up addresses are never touched."""
    from somi_amd import _lib
    L = _lib.lib()
    for who, (call, slices, optional) in _calls(_lib, L).items():
        for field in slices():
            for what, brk in BREAKS:
                s = slices()
                brk(s[field])
                if field in optional and what == 'pointer NULL':
                    continue
                assert call(s) == -1, f'{who}: {field}: {what} is let through'
                assert f'{who}: {field} = ['.encode() in L.somi_last_error(), f'{who}: {field}: {what}: {L.somi_last_error()}'
        for ch in (6, 0, -4, 2):
            assert call(slices(), Ch=ch) == -1 and f'half width {ch}'.encode() in L.somi_last_error(), f'{who}: Ch = {ch}: {L.somi_last_error()}'
        s = slices()
        wide = 'out' if 'out' in s else 'dout'
        s[wide].coff = 12                                         # 8 channels fit from offset 12 of 24, the 16 of the shuffled side do not
        assert call(s) == -1 and f'{wide} = [12, 28) of 24 channels: runs past the channel stride'.encode() in L.somi_last_error()
    tail, slices, _ = _calls(_lib, L)['gs tail']
    for kw, word in ((dict(H=0), b'bad sizes'), (dict(B=-1), b'bad sizes'), (dict(act=7), b'bad activation'), (dict(act=-1), b'bad activation'),
                     (dict(w1=None), b'w1, b1, w2, b2'), (dict(b2=0xD0004), b'w1, b1, w2, b2'), (dict(w_cs=6), b'row stride w_cs (6)'),
                     (dict(w_cs=4), b'row stride w_cs (4)')):
        assert tail(slices(), **kw) == -1 and word in L.somi_last_error(), f'gs tail {kw}: {L.somi_last_error()}'
    shuffle, slices, _ = _calls(_lib, L)['gs shuffle']
    for kw, word in ((dict(npix=0), b'0 pixels'), (dict(act=9), b'bad activation'), (dict(shift=None), b'scale and shift come together'),
                     (dict(scale=0xE0008), b'scale and shift come together')):
        assert shuffle(slices(), **kw) == -1 and word in L.somi_last_error(), f'gs shuffle {kw}: {L.somi_last_error()}'
    unshuffle, slices, _ = _calls(_lib, L)['gs unshuffle']
    assert unshuffle(slices(), npix=-3) == -1 and b'-3 pixels' in L.somi_last_error()


def test_the_plan_export_is_host_arithmetic():
    """A workgroup of the two streaming kernels is nq source quads wide (the power of two that covers Ch / 2, 64 at most, further quads in a
    second grid dimension) and 256 / nq pixels tall; it walks as many such tiles as leave about 2048 workgroups, 64 at most."""
    from somi_amd import ops
    tiles = ops.gs_tiles_per_workgroup
    assert [tiles(3 * 5 * 7, ch) for ch in (4, 8, 12, 20, 68)] == [1] * 5 and tiles(1, 4) == 1
    assert tiles(128 * 128, 68) == 2                              # 34 quads -> 64 lanes, 4 pixels a tile: 4096 tiles
    assert tiles(128 * 128 - 4, 68) == 1 and tiles(2 * 128 * 128, 68) == 4
    assert tiles(1 << 19, 4) == 2                                 # 2 quads, 128 pixels a tile
    assert tiles(32 * 80 * 80, 64) == 12 and tiles(32 * 40 * 40, 64) == 3 and tiles(128 * 80 * 80, 64) == 50
    assert tiles(32 * 80 * 80, 256) == 50                         # 128 quads: two chunks of 64
    assert tiles(1 << 30, 64) == 64                               # capped
    assert tiles(0, 8) == 0 and tiles(10, 6) == 0 and tiles(10, 0) == 0 and tiles(-1, 8) == 0
