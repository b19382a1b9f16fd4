"""CPU checks of the ASF-YOLO neck (Zoom_cat, models/common.py:4312-4327; ScalSeq, :4330-4355; attention_model, :4358-4424): the test
restatement (tests/asf_ref.py) reproduces the reference's own classes through the tests/golden/block_asf_*.npz fixtures; the low-resolution
form of ScalSeq the kernels compute equals the literal one in fp64 - outputs, every gradient, the running buffers - and two plausible but
wrong forms do not; both tie rules; the ECA kernel size; the parser's c2 rules, the cfg and every limit's message; state-dict keys; and the
new entry points are declared, bound, exported and refuse bad descriptors without a launch."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import asf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

NEW_SYMBOLS = ('somi_zoomcat_nhwc_f32', 'somi_zoomcat_bwd_nhwc_f32', 'somi_zoomcat_desc_bytes',
               'somi_scalseq_stats_f32', 'somi_scalseq_fuse_nhwc_f32', 'somi_scalseq_route_bwd_nhwc_f32', 'somi_scalseq_apply_bwd_f32',
               'somi_scalseq_workspace_floats', 'somi_scalseq_desc_bytes',
               'somi_eca_gate_f32', 'somi_eca_gate_bwd_f32', 'somi_asf_mix_means_nhwc_f32', 'somi_asf_mix_bwd_sums_nhwc_f32',
               'somi_asf_mix_bwd_input_nhwc_f32', 'somi_asfatt_workspace_floats', 'somi_asfatt_desc_bytes')
FAMILY = ('Zoom_cat', 'ScalSeq', 'attention_model')


def _fixture(tag):
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    xs = [torch.from_numpy(d[f'x{i}']) for i in range(len([k for k in d.files if re.fullmatch(r'x\d', k)]))]
    return xs, {m: torch.from_numpy(d[f'out_{m}']) for m in ('eval', 'train')}


def _filled(tag, seed=0):
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    mod = fill_state(R.BLOCKS[tag][0](R), seed)
    OB.initialize_weights(mod)
    return mod


@pytest.mark.parametrize('tag', R.FIXTURES)
def test_restatement_reproduces_the_reference(tag):
    """Eval and train outputs of the reference's own class under fill_state weights, fp32, 1e-5 relative; the fixtures hold data only."""
    xs, want = _fixture(tag)
    assert [tuple(x.shape) for x in xs] == R.BLOCKS[tag][1]
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    assert sorted(d.files) == sorted([f'x{i}' for i in range(len(xs))] + ['out_eval', 'out_train'])
    assert os.path.getsize(os.path.join(GOLDEN, f'block_{tag}.npz')) < os.path.getsize(os.path.join(GOLDEN, 'block_carafe.npz'))
    mod = _filled(tag)
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod([x.clone() for x in xs])
        err = (y - want[mode]).abs().max().item()
        assert y.shape == want[mode].shape and err <= 1e-5 * want[mode].abs().max().item(), f'{tag} {mode}: {err:.3e}'


def test_scalseq_lowres_form_reproduces_the_fixture_and_wrong_forms_do_not():
    """The low-resolution form against the reference's own training output; weights 1, 1, 1 (the upsampled pixels counted once) and
    N = B H W (one level's count) are off by far more than the bar."""
    xs, want = _fixture('asf_scalseq')
    scale = want['train'].abs().max().item()
    errs = {}
    for name, kw in (('right', {}), ('weights 1,1,1', dict(weights=(1, 1, 1))), ('N = BHW', dict(count='BHW'))):
        mod = _filled('asf_scalseq').train()
        with torch.no_grad():
            errs[name] = (R.scalseq_lowres(mod, xs, **kw) - want['train']).abs().max().item() / scale
    print(errs)
    assert errs['right'] <= 1e-5, errs
    assert errs['weights 1,1,1'] > 1e-2 and errs['N = BHW'] > 1e-2, f'the fixture does not tell the wrong forms apart: {errs}'
    mod = _filled('asf_scalseq').eval()
    with torch.no_grad():
        assert (R.scalseq_lowres(mod, xs) - want['eval']).abs().max().item() <= 1e-5 * want['eval'].abs().max().item()


@pytest.mark.parametrize('shape', [(2, 4, 8), (1, 8, 4), (3, 12, 20)], ids=str)
def test_scalseq_lowres_equals_the_literal_form_in_fp64(shape):
    """Output, the gradient of p3, p4, p5 and of every parameter, and the running buffers: the low-resolution form against the literal stack
    (Conv3d, BatchNorm3d, MaxPool3d of torch) in fp64, 1e-12 relative; the WRONG variants miss the running variance and the output."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(B * H + W)
    xs = [torch.randn(B, 8, H, W, generator=gen, dtype=torch.float64), torch.randn(B, 512, H // 2, W // 2, generator=gen, dtype=torch.float64),
          torch.randn(B, 1024, H // 4, W // 4, generator=gen, dtype=torch.float64)]
    dy = torch.randn(B, 8, H, W, generator=gen, dtype=torch.float64)
    runs = {}
    for form in ('literal', 'lowres', 'w111', 'bhw'):
        mod = _filled('asf_scalseq', 3).double().train()
        ins = [x.clone().requires_grad_(True) for x in xs]
        y = {'literal': lambda: mod(ins), 'lowres': lambda: R.scalseq_lowres(mod, ins),
             'w111': lambda: R.scalseq_lowres(mod, ins, weights=(1, 1, 1)), 'bhw': lambda: R.scalseq_lowres(mod, ins, count='BHW')}[form]()
        y.backward(dy)
        runs[form] = dict(out=y.detach(), **{f'dx{i}': t.grad for i, t in enumerate(ins)},
                          **{'d' + n: p.grad for n, p in mod.named_parameters()}, **{n: b.clone().double() for n, b in mod.named_buffers()})
    rel = lambda a, b: (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)     # noqa: E731
    lit = runs['literal']
    assert set(lit) == set(runs['lowres'])
    for k, v in lit.items():
        if k == 'dconv3d.bias':                                   # analytically zero in front of a batch norm: rounding noise on both sides
            assert runs['lowres'][k].abs().max().item() < 1e-10 and v.abs().max().item() < 1e-10
            continue
        assert rel(runs['lowres'][k], v) <= 1e-12, f'{k}: {rel(runs["lowres"][k], v):.3e}'
    for wrong in ('w111', 'bhw'):
        assert rel(runs[wrong]['out'], lit['out']) > 1e-3 and rel(runs[wrong]['bn.running_var'], lit['bn.running_var']) > 1e-3, wrong


def test_tie_rules_on_constant_maps():
    """MaxPool3d((3,1,1)) sends a tie to the first depth index and adaptive_max_pool2d to the first pixel of the window in row-major order -
    in torch itself (the literal forms) and in the restatement's first_max."""
    l = torch.full((1, 2, 4, 6), 1.5, requires_grad=True)
    out = R.Zoom_cat(2)([l, torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 1, 2)])
    out[:, :2].sum().backward()
    want = torch.full((4, 6), 0.25)
    want[0::2, 0::2] += 1
    assert torch.equal(l.grad[0, 0], want) and torch.equal(l.grad[0, 1], want)
    _, codes = R.zoomcat_ref(torch.full((1, 4, 6, 4), 1.5), torch.zeros(1, 2, 3, 4), torch.zeros(1, 1, 2, 4))
    assert int(codes.abs().max()) == 0
    stack = torch.full((1, 2, 3, 4, 4), -0.5, requires_grad=True)
    torch.nn.MaxPool3d((3, 1, 1))(stack).sum().backward()
    assert bool((stack.grad[:, :, 0] == 1).all()) and bool((stack.grad[:, :, 1:] == 0).all())
    v = torch.full((1, 4, 4, 4), 2.0)
    assert int(R.first_max([v, v.clone(), v.clone()])[1].max()) == 0
    assert int(R.first_max([v - 1, v, v.clone()])[1].min()) == 1


def test_eca_kernel_size_for_32_to_1024_channels():
    from somi_amd import blocks as MB
    from somi_amd import ops
    want = {32: 3, 64: 3, 128: 5, 256: 5, 512: 5, 1024: 5}
    for c, k in want.items():
        assert ops.eca_kernel_size(c) == R.eca_kernel_size(c) == k, c
        assert MB.channel_att(c).conv.kernel_size == (k,) and MB.channel_att(c).conv.padding == (k // 2,)
        assert R.channel_att(c).conv.kernel_size == (k,)
    assert ops.eca_kernel_size(8) == 3 and ops.eca_kernel_size(2 ** 15) == 9 == ops.ECA_KMAX


def test_blocks_keep_the_reference_parameter_layout():
    from oracle.somi_ref.testing import fill_state
    from somi_amd import blocks as MB
    for tag, (make, _) in R.BLOCKS.items():
        a, b = make(R), make(MB)
        assert list(a.state_dict()) == list(b.state_dict()), tag
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # checkpoints load both ways
        a.load_state_dict(b.state_dict())
    ss = MB.ScalSeq(8)
    assert type(ss.conv3d) is torch.nn.Conv3d and type(ss.bn) is torch.nn.BatchNorm3d and ss.conv3d.weight.shape == (8, 8, 1, 1, 1)
    assert [n for n, _ in ss.named_children()] == ['conv1', 'conv2', 'conv3d', 'bn', 'act', 'pool_3d']
    am = MB.attention_model(64)
    assert type(am.channel_att.conv) is torch.nn.Conv1d and am.channel_att.conv.weight.shape == (1, 1, 3)
    assert list(am.state_dict()) == ['channel_att.conv.weight', 'local_att.conv_1x1.weight', 'local_att.bn.weight', 'local_att.bn.bias',
                                     'local_att.bn.running_mean', 'local_att.bn.running_var', 'local_att.bn.num_batches_tracked',
                                     'local_att.F_h.weight', 'local_att.F_w.weight']
    assert list(MB.Zoom_cat(8).state_dict()) == []
    for name in FAMILY:
        cls = getattr(MB, name)
        assert cls.__dict__['accumulates'] is False and cls.__dict__['folds_pooled'] is False, name
    assert MB.Zoom_cat.reduction == 2 and MB.ScalSeq.reduction == 1 and MB.attention_model.reduction == 1


def test_every_limit_raises_by_name():
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    z = lambda h, w, c=8, **k: Act(torch.zeros(1, h, w, c), **k)  # noqa: E731  (CPU tensors: every limit is raised before a launch)
    zc = MB.Zoom_cat(8).eval()
    with pytest.raises(NotImplementedError, match='l must be exactly 2x m'):
        zc([z(9, 8), z(4, 4), z(2, 2)])
    with pytest.raises(NotImplementedError, match='s must be exactly m / 2'):
        zc([z(8, 8), z(4, 4), z(3, 2)])
    with pytest.raises(NotImplementedError, match='s must be exactly m / 2'):
        zc([z(6, 6), z(3, 3), z(2, 2)])
    with pytest.raises(NotImplementedError, match=r'C % 4 == 0'):
        zc([Act(torch.zeros(1, 8, 8, 8), 0, 6), z(4, 4), z(2, 2)])
    with pytest.raises(NotImplementedError, match='nn.Upsample view'):
        zc([z(8, 8), z(4, 4), z(2, 2, up=1)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        zc([z(8, 8), z(4, 4), z(2, 2)])
    ss = MB.ScalSeq(8).eval()
    with pytest.raises(NotImplementedError, match='exactly 1 : 1/2 : 1/4'):
        ss([z(8, 8), z(4, 4, 512), z(2, 3, 1024)])
    with pytest.raises(NotImplementedError, match='exactly 1 : 1/2 : 1/4'):
        ss([z(6, 6), z(3, 3, 512), z(1, 1, 1024)])
    with pytest.raises(NotImplementedError, match='p3 input must have 8 channels'):
        ss([z(8, 8, 16), z(4, 4, 512), z(2, 2, 1024)])
    with pytest.raises(NotImplementedError, match=r'C % 4 == 0'):
        MB.ScalSeq(6).eval()([Act(torch.zeros(1, 8, 8, 8), 0, 6), z(4, 4, 512), z(2, 2, 1024)])
    with pytest.raises(NotImplementedError, match='nn.Upsample view'):
        ss([z(8, 8), z(4, 4, 512, up=1), z(2, 2, 1024)])
    am = MB.attention_model(64).eval()
    with pytest.raises(NotImplementedError, match='inputs of unequal shape'):
        am([z(5, 7, 64), z(5, 6, 64)])
    with pytest.raises(NotImplementedError, match='inputs of unequal shape'):
        am([z(5, 7, 64), z(5, 7, 32)])
    with pytest.raises(NotImplementedError, match='nn.Upsample view'):
        am([z(5, 7, 64, up=1), z(5, 7, 64)])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        am([z(5, 7, 64), z(5, 7, 64)])
    with pytest.raises(RuntimeError, match='inside attention_model'):
        MB.channel_att(64)(z(4, 4, 64))


def test_parser_c2_rules_cfg_and_the_oracle_layer_table(monkeypatch):
    from somi_amd import blocks as MB
    from somi_amd.configs import COCO_ANCHORS, yolov5_asf_cfg, yolov5_cfg
    from somi_amd.model import Model, _REPEAT_INSIDE
    R.register(monkeypatch)
    assert not set(FAMILY) & set(_REPEAT_INSIDE)
    cfg = yolov5_asf_cfg(depth=0.33, nc=4)
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple']) == (4, 0.33, 1.0) and yolov5_asf_cfg()['anchors'] == COCO_ANCHORS
    assert cfg['backbone'] == yolov5_cfg(1.0, 0.33, nc=4)['backbone']
    rows = {10 + i: r for i, r in enumerate(cfg['head'])}
    assert rows[12] == [[-1, 6, -2], 1, 'Zoom_cat', [512]] and rows[16] == [[-1, 4, -2], 1, 'Zoom_cat', [256]]
    assert rows[24] == [[4, 6, 8], 1, 'ScalSeq', [256]] and rows[25] == [[17, -1], 1, 'attention_model', [256]]
    assert rows[26] == [[25, 20, 23], 1, 'Detect', ['nc', 'anchors']]
    assert all(r[2] not in FAMILY for r in yolov5_cfg()['backbone'] + yolov5_cfg()['head'])
    ref, mine = R.oracle_model(cfg), Model(cfg)
    want = {k: (tuple(v.shape), v.dtype) for k, v in ref.state_dict().items()}
    got = {k: (tuple(v.shape), v.dtype) for k, v in mine.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert [n for n, _ in mine.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save and [m.type for m in mine.model] == [m.type for m in ref.model]
    mine.load_state_dict(ref.state_dict())
    assert type(mine.model[12]) is MB.Zoom_cat and mine.model[13].cv1.conv.in_channels == 1536       # c2 = 3 * 512, unscaled
    assert type(mine.model[16]) is MB.Zoom_cat and mine.model[17].cv1.conv.in_channels == 768
    assert type(mine.model[24]) is MB.ScalSeq and mine.model[24].conv3d.out_channels == 256
    assert type(mine.model[25]) is MB.attention_model and mine.model[26].m[0].in_channels == 256
    bad = copy.deepcopy(cfg)
    bad['head'][2][3] = [256]                                     # names 256 where the three inputs carry 512 each
    with pytest.raises(ValueError, match=r"'Zoom_cat' row that names 256 channels records 3 \* 256 = 768 .* \[512, 512, 512\]"):
        Model(bad)
    half = copy.deepcopy(cfg)
    half['width_multiple'] = 0.5                                  # nothing scales the three rows: the widths no longer add up
    with pytest.raises(ValueError, match="'Zoom_cat' row"):
        Model(half)


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
    lib = _lib.lib()
    assert lib.somi_zoomcat_desc_bytes() == ctypes.sizeof(_lib.ZoomcatDesc)
    assert lib.somi_scalseq_desc_bytes() == ctypes.sizeof(_lib.ScalseqDesc)
    assert lib.somi_asfatt_desc_bytes() == ctypes.sizeof(_lib.AsfAttDesc)
    assert lib.somi_abi_version() == 15
    for fn in ('zoomcat', 'zoomcat_backward', 'scalseq_stats', 'scalseq_fuse', 'scalseq_route_backward', 'scalseq_apply_backward', 'eca_gate',
               'eca_gate_backward', 'asf_mix_means', 'asf_mix_backward_sums', 'asf_mix_backward_input'):
        assert callable(getattr(ops, fn))
    assert 'asf.hip' in open(os.path.join(ROOT, 'yolo-somi_amd', 'csrc', 'Makefile')).read()


def test_bad_descriptors_are_refused_without_a_launch():
    """Fake aligned addresses: every refusal comes back before anything is launched (SOMI_EINVAL -1, SOMI_ENOTIMPL -2, SOMI_EWORKSPACE -3)."""
    from somi_amd import _lib
    L = _lib.lib()
    S = _lib.Slice

    def zc():
        d = _lib.ZoomcatDesc()
        d.l, d.m, d.s, d.out = S(0x10000, 8, 0), S(0x20000, 8, 0), S(0x30000, 8, 0), S(0x40000, 24, 0)
        d.codes, d.B, d.H, d.W, d.Cl, d.Cm, d.Cs = 0x50000, 1, 2, 2, 8, 8, 8
        return d
    for fn in (L.somi_zoomcat_nhwc_f32, L.somi_zoomcat_bwd_nhwc_f32):
        for attr, value in (('Cl', 6), ('H', 0), ('B', 1 << 30)):
            d = zc()
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and b'bad sizes' in L.somi_last_error(), attr
        d = zc()
        d.out = S(0x40000, 20, 0)                                 # 24 channels do not fit 20
        assert fn(ctypes.byref(d), None) == -1 and b'runs past' in L.somi_last_error()
        d = zc()
        d.l = S(0x10004, 8, 0)
        assert fn(ctypes.byref(d), None) == -1 and b'16-byte' in L.somi_last_error()
    d = zc()
    d.codes = None
    assert L.somi_zoomcat_bwd_nhwc_f32(ctypes.byref(d), None) == -1 and b'codes' in L.somi_last_error()

    def ss():
        d = _lib.ScalseqDesc()
        d.u3, d.u4, d.u5, d.out = S(0x10000, 8, 0), S(0x20000, 8, 0), S(0x30000, 8, 0), S(0x40000, 8, 0)
        d.g3, d.g4, d.g5 = S(0x50000, 8, 0), S(0x60000, 8, 0), S(0x70000, 8, 0)
        d.codes, d.gamma, d.beta, d.mean, d.rstd, d.scale, d.shift, d.sums = (0x80000 + 0x100 * i for i in range(8))
        d.B, d.H, d.W, d.C, d.eps, d.momentum = 1, 4, 4, 8, 1e-5, 0.1
        d.workspace, d.workspace_floats = 0x90000, L.somi_scalseq_workspace_floats(1, 4, 4, 8)
        return d
    entries = (L.somi_scalseq_stats_f32, L.somi_scalseq_fuse_nhwc_f32, L.somi_scalseq_route_bwd_nhwc_f32, L.somi_scalseq_apply_bwd_f32)
    for fn in entries:
        for attr, value in (('C', 6), ('H', 6), ('W', 2), ('B', 0)):
            d = ss()
            setattr(d, attr, value)
            assert fn(ctypes.byref(d), None) == -1 and b'bad sizes' in L.somi_last_error(), attr
        d = ss()
        d.u4 = S(0x20000, 8, 4)
        assert fn(ctypes.byref(d), None) == -1 and b'u4' in L.somi_last_error()
    for fn in (entries[0], entries[2]):
        d = ss()
        d.workspace_floats -= 1
        assert fn(ctypes.byref(d), None) == -3
        d.workspace = None
        assert fn(ctypes.byref(d), None) == -1
    d = ss()
    d.codes = None
    assert entries[2](ctypes.byref(d), None) == -1 and b'codes' in L.somi_last_error()
    d = ss()
    d.shift = None
    assert entries[1](ctypes.byref(d), None) == -1 and b'come together' in L.somi_last_error()
    d.scale = None
    assert entries[3](ctypes.byref(d), None) == -1
    assert L.somi_scalseq_workspace_floats(1, 6, 4, 8) == 0 and L.somi_scalseq_workspace_floats(1, 4, 4, 6) == 0

    def am():
        d = _lib.AsfAttDesc()
        d.x1, d.x2, d.t, d.pool, d.dx1 = S(0x10000, 8, 0), S(0x20000, 8, 0), S(0x30000, 8, 0), S(0x40000, 8, 0), S(0x50000, 8, 0)
        d.gate, d.ds, d.davg, d.B, d.H, d.W, d.C = 0x60000, 0x70000, 0x80000, 1, 3, 5, 8
        d.workspace, d.workspace_floats = 0x90000, L.somi_asfatt_workspace_floats(1, 3, 5, 8)
        return d
    entries = (L.somi_asf_mix_means_nhwc_f32, L.somi_asf_mix_bwd_sums_nhwc_f32, L.somi_asf_mix_bwd_input_nhwc_f32)
    for fn in entries:
        d = am()
        d.C = 6
        assert fn(ctypes.byref(d), None) == -1 and b'bad sizes' in L.somi_last_error()
        d = am()
        d.t = S(0x30000, 8, 4)
        assert fn(ctypes.byref(d), None) == -1 and b'runs past' in L.somi_last_error()
    for fn in entries[:2]:
        d = am()
        d.workspace_floats -= 1
        assert fn(ctypes.byref(d), None) == -3
    d = am()
    d.gate = None
    assert entries[0](ctypes.byref(d), None) == -1 and entries[2](ctypes.byref(d), None) == -1
    assert L.somi_eca_gate_f32(0x1000, 0x2000, 4, 0x3000, 1, 8, None) == -2 and b'odd' in L.somi_last_error()
    assert L.somi_eca_gate_f32(0x1000, 0x2000, 11, 0x3000, 1, 8, None) == -2
    assert L.somi_eca_gate_f32(None, 0x2000, 3, 0x3000, 1, 8, None) == -1
    assert L.somi_eca_gate_bwd_f32(0x1000, 0x2000, 3, 0x3000, None, 0x4000, 0x5000, 1, 8, None) == -1
