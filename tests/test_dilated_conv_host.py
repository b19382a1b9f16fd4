"""CPU checks of dilated convolution and the context blocks built on it (ASPP, models/common.py:1829-1843; DWR, DWRSeg_Conv, Bottleneck_DWRSeg and
C2f_DWR, :7431-7511): blocks.Conv accepts a dense dilated conv at stride 1 and refuses the rest by name; the C ABI's two gradient entries
accept a dilated forward geometry, check Ho / Wo against the DILATED extent and refuse the dilated data gradient at stride > 1; the test
restatement (tests/context_ref.py) reproduces the reference's own classes through the five tests/golden/block_*.npz fixtures; state-dict
layouts, parser, strides and parameter counts are the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':                                       # the child (below) runs this file as a script: the oracle lives at the root
    sys.path.insert(0, ROOT)

import context_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EINVAL, ENOTIMPL = -1, -2


# ---------------------------------------------------------------------------------------------------------------- blocks.Conv
def test_dense_dilated_conv_builds_with_the_reference_padding():
    from somi_amd import blocks as MB
    c = MB.Conv(8, 8, 3, 1, None, 1, 2)
    assert c.conv.dilation == (2, 2) and c.conv.padding == (2, 2) and c.conv.stride == (1, 1) and c.conv.groups == 1
    assert MB.Conv(8, 8, 3, d=5).conv.padding == (5, 5) and MB.Conv(8, 8, 3, d=1).conv.padding == (1, 1)
    assert MB.Conv(8, 8, (3, 3), 1, None, 1, 3).conv.dilation == (3, 3)          # the tuple form C2f_DWR hands its bottlenecks


def test_dilated_conv_limits_are_explicit():
    from somi_amd import blocks as MB
    with pytest.raises(NotImplementedError, match='dilated'):
        MB.Conv(8, 8, 3, 1, None, 8, 2)                            # depthwise
    with pytest.raises(NotImplementedError, match='dilated'):
        MB.Conv(8, 8, 3, 1, None, 2, 2)                            # grouped
    with pytest.raises(NotImplementedError, match='stride 2'):
        MB.Conv(8, 8, 3, 2, None, 1, 2)
    with pytest.raises(NotImplementedError, match='dilated ODConv'):
        MB.ODConv2d_3rd(8, 8, 3, dilation=2)


def test_ops_gradients_take_dil():
    import inspect
    from somi_amd import ops
    for fn in (ops.conv2d_dgrad_nhwc, ops.conv2d_wgrad_nhwc, ops.conv2d_nhwc):
        assert inspect.signature(fn).parameters['dil'].default == 1
    assert ops.conv_out_size(9, 3, 1, 0, 2) == 5 and ops.conv_out_size(10, 3, 2, 2, 2) == 5


# ---------------------------------------------------------------------------------------------------------------- the C ABI, in a child without a device
GEO = {'d.w': 0, 'd.B': 1, 'd.H': 9, 'd.W': 7, 'd.Cin': 32, 'd.Cout': 32, 'd.kh': 3, 'd.kw': 3, 'd.pad': 2, 'd.x': 0, 'd.y': 0,
       'd.x_cs': 32, 'd.y_cs': 32, 'dy_cs': 32, 'dx_cs': 32, 'x_cs': 32, 'accumulate': None, 'workspace_bytes': 1 << 40}
CASES = {        # name -> (entry point, geometry on top of GEO)
    'fwd dil 2': ('somi_conv2d_nhwc_f32', {'d.dil': 2, 'd.stride': 1, 'd.Ho': 9, 'd.Wo': 7}),
    'dgrad dil 2': ('somi_conv2d_dgrad_nhwc_f32', {'d.dil': 2, 'd.stride': 1, 'd.Ho': 9, 'd.Wo': 7}),
    'wgrad dil 2': ('somi_conv2d_wgrad_nhwc_f32', {'d.dil': 2, 'd.stride': 1, 'd.Ho': 9, 'd.Wo': 7}),
    'wgrad dil 2 stride 2': ('somi_conv2d_wgrad_nhwc_f32', {'d.dil': 2, 'd.stride': 2, 'd.Ho': 5, 'd.Wo': 4}),
    'dgrad dil 2 stride 2': ('somi_conv2d_dgrad_nhwc_f32', {'d.dil': 2, 'd.stride': 2, 'd.Ho': 5, 'd.Wo': 4}),
    'dgrad dil 1 stride 2': ('somi_conv2d_dgrad_nhwc_f32', {'d.dil': 1, 'd.stride': 2, 'd.pad': 1, 'd.Ho': 5, 'd.Wo': 4}),
    # Ho / Wo of the undilated conv (pad 2, k 3: 11 x 9) with dil = 2 set
    'fwd stale size': ('somi_conv2d_nhwc_f32', {'d.dil': 2, 'd.stride': 1, 'd.Ho': 11, 'd.Wo': 9}),
    'dgrad stale size': ('somi_conv2d_dgrad_nhwc_f32', {'d.dil': 2, 'd.stride': 1, 'd.Ho': 11, 'd.Wo': 9}),
    'wgrad stale size': ('somi_conv2d_wgrad_nhwc_f32', {'d.dil': 2, 'd.stride': 1, 'd.Ho': 11, 'd.Wo': 9}),
    'dgrad dil 0': ('somi_conv2d_dgrad_nhwc_f32', {'d.dil': 0, 'd.stride': 1, 'd.Ho': 11, 'd.Wo': 9}),
    'wgrad dil 0': ('somi_conv2d_wgrad_nhwc_f32', {'d.dil': 0, 'd.stride': 1, 'd.Ho': 11, 'd.Wo': 9}),
}


def _child():
    import torch
    n = torch.cuda.device_count()
    if n != 0:                                               # the guard: with a device visible nothing is called
        print(json.dumps({'devices': n}))
        return
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_slice_args_host as S                         # its caller of an entry point from made-up addresses, and the header's prototypes
    from somi_amd import _lib
    L = _lib.lib()
    protos = S.prototypes()
    out = {}
    for name, (fn, geo) in CASES.items():
        rc, err = S._call(L, _lib, protos[fn], dict(GEO, fn=fn, **geo))
        out[name] = {'rc': rc, 'error': err}
    import ctypes
    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.pad, d.dil, d.Ho, d.Wo = 1, 9, 7, 32, 32, 3, 3, 1, 2, 2, 9, 7
    out['workspace dil 2'] = L.somi_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    d.Ho, d.Wo = 11, 9
    out['workspace stale size'] = L.somi_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    print(json.dumps({'devices': 0, 'results': out}))


_cache = {}


def child_results():
    if 'run' not in _cache:
        env = dict(os.environ, HIP_VISIBLE_DEVICES='-1')
        _cache['run'] = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    r = _cache['run']
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out['devices'] != 0:
        pytest.skip(f"{out['devices']} GPU(s) visible to the child despite HIP_VISIBLE_DEVICES=-1: made-up addresses are never handed to a process "
                    "that could launch on them")
    return out['results']


@pytest.mark.parametrize('name', ['fwd dil 2', 'dgrad dil 2', 'wgrad dil 2', 'wgrad dil 2 stride 2', 'dgrad dil 1 stride 2'])
def test_abi_accepts_the_dilated_geometry(name):
    c = child_results()[name]
    assert c['rc'] > 0, f'{name}: returned {c["rc"]}, "{c["error"]}" - without a device an accepted call ends in the launch failure'


def test_abi_refuses_the_dilated_data_gradient_at_stride_2():
    c = child_results()['dgrad dil 2 stride 2']
    assert c['rc'] == ENOTIMPL and 'stride 1 only' in c['error'], c


@pytest.mark.parametrize('name', ['fwd stale size', 'dgrad stale size', 'wgrad stale size', 'dgrad dil 0', 'wgrad dil 0'])
def test_abi_checks_the_output_size_against_the_dilated_extent(name):
    c = child_results()[name]
    assert c['rc'] == EINVAL, f'{name}: returned {c["rc"]}, "{c["error"]}"'


def test_wgrad_workspace_follows_the_dilated_extent():
    r = child_results()
    assert r['workspace dil 2'] >= 32 * 9 * 32 * 4 and r['workspace stale size'] == 0


# ---------------------------------------------------------------------------------------------------------------- the restatement and the blocks
@pytest.mark.parametrize('tag', sorted(R.BLOCKS))
def test_restatement_reproduces_the_reference(tag):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    mod = fill_state(R.BLOCKS[tag](R), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['x'])
    assert tuple(x.shape) == R.BLOCK_SHAPE and x.shape[2] != x.shape[3]
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        err = (y - want).abs().max().item()
        assert y.shape == want.shape and err <= 1e-5 * want.abs().max().item(), f'{tag} {mode}: {err:.3e}'


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    makes = list(R.BLOCKS.values()) + [lambda M: M.DWRSeg_Conv(32, 64), lambda M: M.Bottleneck_DWRSeg(32, 64, True), lambda M: M.C2f_DWR(32, 64, 1),
                                       lambda M: M.ASPP(512, 256, (5,))]
    for mk in makes:
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())
    aspp = MB.ASPP(64, 64)
    assert [(m.dilation, m.padding, m.bias) for m in aspp.m] == [((2, 2), (2, 2), None), ((4, 4), (4, 4), None), ((6, 6), (6, 6), None)]
    assert aspp.cv2.conv.in_channels == 5 * 32 and [m.dilation[0] for m in MB.ASPP(64, 32, (3, 7)).m] == [1, 3]
    dwr = MB.DWR(64)
    assert [(c.conv.dilation[0], c.conv.padding[0], c.conv.out_channels) for c in (dwr.conv_3x3_d1, dwr.conv_3x3_d3, dwr.conv_3x3_d5)] == \
        [(1, 1, 64), (3, 3, 32), (5, 5, 32)]
    assert [n for n, _ in MB.DWRSeg_Conv(64, 64).named_children()] == ['conv', 'dcnv3', 'bn', 'gelu']
    blk = MB.C2f_DWR(64, 128, 2, True)
    assert len(blk.m) == 2 and all(type(m) is MB.Bottleneck_DWRSeg and m.add and m.cv1.conv.kernel_size == (3, 3) for m in blk.m)
    with pytest.raises(NotImplementedError, match='odd k >= 3'):
        MB.ASPP(64, 64, (4,))


def test_new_blocks_declare_the_walk_contract_themselves():
    from somi_amd import blocks as MB
    for cls in (MB.ASPP, MB.DWR, MB.DWRSeg_Conv, MB.Bottleneck_DWRSeg, MB.C2f_DWR):
        assert cls.__dict__['accumulates'] is False and cls.__dict__['folds_pooled'] is False and cls.__dict__['reduction'] == 1, cls.__name__


# ---------------------------------------------------------------------------------------------------------------- configs and the parser
@pytest.mark.parametrize('where', ['aspp', 'dwr', 'both'])
def test_context_graph_matches_the_oracle(where, monkeypatch):
    from somi_amd import blocks as MB
    from somi_amd.configs import yolov5_cfg, yolov5_context_cfg
    from somi_amd.model import Model, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert 'C2f_DWR' in _REPEAT_INSIDE and 'ASPP' not in _REPEAT_INSIDE
    cfg = yolov5_context_cfg(0.25, 0.33, nc=10, where=where)
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    bns = [m for m in mine.modules() if isinstance(m, nn.BatchNorm2d)]
    assert all(m.eps == 1e-3 and m.momentum == 0.03 for m in bns)
    mine.load_state_dict(ref.state_dict())
    assert mine.fuse() is mine
    for m in mine.model:                                          # what the graph walk reads of every layer
        assert isinstance(m.accumulates, bool) and isinstance(m.folds_pooled, bool) and m.reduction in (0.5, 1, 2), m.type
    base = yolov5_cfg(0.25, 0.33, nc=10)
    assert cfg['head'] == base['head'] and [r[:2] for r in cfg['backbone']] == [r[:2] for r in base['backbone']]
    changed = [i for i, (a, b) in enumerate(zip(cfg['backbone'], base['backbone'])) if a != b]
    assert changed == {'aspp': [9], 'dwr': [6, 8], 'both': [6, 8, 9]}[where]
    if where != 'dwr':
        assert cfg['backbone'][9] == [-1, 1, 'ASPP', [1024]] and type(mine.model[9]) is MB.ASPP and mine.model[9].cv1.conv.out_channels == 128
    if where != 'aspp':
        assert cfg['backbone'][6] == [-1, 9, 'C2f_DWR', [512, True]] and cfg['backbone'][8] == [-1, 3, 'C2f_DWR', [1024, True]]
        assert type(mine.model[6]) is MB.C2f_DWR and len(mine.model[6].m) == 3 and len(mine.model[8].m) == 1 and mine.model[8].m[0].add
        assert mine.model[8].m[0].cv2.dcnv3.conv_3x3_d5.conv.dilation == (5, 5)


def test_cfg_defaults_and_the_other_cfgs_are_unchanged():
    from somi_amd.configs import COCO_ANCHORS, yolov5_ca_cfg, yolov5_cfg, yolov5_context_cfg, yolov5_swin_cfg
    cfg = yolov5_context_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert [r[2] for r in cfg['backbone']] == ['Conv', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'C3', 'ASPP']
    assert [r[2] for r in yolov5_context_cfg(where='both')['backbone']] == ['Conv', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'C2f_DWR', 'Conv', 'C2f_DWR', 'ASPP']
    for other in (yolov5_cfg(), yolov5_cfg(version='5.0'), yolov5_ca_cfg(), yolov5_swin_cfg()):
        assert all(r[2] not in ('ASPP', 'C2f_DWR') for r in other['backbone'] + other['head'])
    assert yolov5_cfg()['backbone'][9] == [-1, 1, 'SPPF', [1024, 5]] and yolov5_cfg()['backbone'][6] == [-1, 9, 'C3', [512]]
    with pytest.raises(ValueError, match="'aspp', 'dwr' or 'both'"):
        yolov5_context_cfg(where='neck')


def test_c3tr_stays_outside():
    from somi_amd.configs import yolov5_context_cfg
    from somi_amd.model import Model
    cfg = yolov5_context_cfg(0.25, 0.33, nc=10, where='both')
    cfg['backbone'][4][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)


if __name__ == '__main__':
    _child()
