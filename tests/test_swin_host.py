"""CPU checks of the Swin module set (C3STR, models/common.py:1632-1637): the test restatement (tests/swin_ref.py) reproduces the reference's
own classes through the tests/golden/block_*.npz fixtures, the shift mask's region ids are the reference's - its quirk included -, the product
blocks and graph are built like the reference's (parameter and buffer names and shapes, strides, save list, parameter count), the limits of
the MI355X path are explicit and the relative-position bias table stays outside every optimizer group, as in the reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import swin_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

FIXTURES = {'c3str': lambda: R.C3STR(64, 64, 2), 'c3str_h2': lambda: R.C3STR(128, 128, 2, False),
            'swinblock_small': lambda: R.SwinTransformerBlock(32, 32, 1, 2)}

NEW_SYMBOLS = ('somi_swin_attention_f32', 'somi_swin_attention_lse_floats', 'somi_swin_attention_backward_f32',
               'somi_swin_attention_bwd_workspace_floats', 'somi_layernorm_bwd_nhwc_f32', 'somi_layernorm_bwd_workspace_floats', 'somi_gelu_bwd_f32')


@pytest.mark.parametrize('tag', list(FIXTURES))
def test_restatement_reproduces_the_reference_blocks(tag):
    """Eval and train outputs of the reference's classes under fill_state weights (oracle.gen_golden.run_block), fp32, 1e-5 relative."""
    from oracle.somi_ref import blocks as OB
    from oracle.somi_ref.testing import fill_state
    d = np.load(os.path.join(GOLDEN, f'block_{tag}.npz'))
    mod = fill_state(FIXTURES[tag](), 0)
    OB.initialize_weights(mod)
    x = torch.from_numpy(d['in0'])
    for mode in ('eval', 'train'):
        mod.train(mode == 'train')
        with torch.no_grad():
            y = mod(x.clone())
        want = torch.from_numpy(d[f'out_{mode}'])
        err = (y - want).abs().max().item()
        assert err <= 1e-5 * want.abs().max().item(), f'{tag} {mode}: {err:.3e}'


PROBED_16x24 = [[0] * 16 + [1] * 4 + [2] * 4] + [[0] * 24] * 7 + [[3] * 16 + [4] * 4 + [5] * 4] * 4 + [[6] * 16 + [7] * 4 + [8] * 4] * 4


def _differs(ids):
    """(windows, 64, 64) uint8: 1 where two tokens of a window carry different region ids (where create_mask puts -100)."""
    hp, wp = ids.shape
    w = ids.view(hp // 8, 8, wp // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
    return (w[:, None, :] != w[:, :, None]).to(torch.uint8)


def test_region_ids_are_the_reference_ones_quirk_included():
    """The id map probed on the reference for a padded (16, 24) map - row 0 and rows 8.. only carry the first row group's ids, rows 1-7 are all
    0 - and, for two more sizes, the token pairs the reference's create_mask separates (tests/golden/swin_shift_masks.npz)."""
    from somi_amd.blocks import swin_region_ids
    for fn in (swin_region_ids, R.region_ids):
        got = fn(16, 24)
        assert got.tolist() == PROBED_16x24, fn.__module__
        d = np.load(os.path.join(GOLDEN, 'swin_shift_masks.npz'))
        for (H, W), (hp, wp) in (((5, 3), (8, 8)), ((20, 12), (24, 16))):
            want = torch.from_numpy(d[f'differs_{H}x{W}'])
            assert want.any() and torch.equal(_differs(fn(hp, wp)), want), f'{fn.__module__} ({hp}, {wp})'
    assert swin_region_ids(16, 24).dtype == torch.int32


def test_swin_blocks_keep_reference_parameter_layout():
    from somi_amd import blocks as MB
    from oracle.somi_ref.testing import fill_state
    for mk in (lambda M: M.WindowAttention(64, (8, 8), 2, qkv_bias=False), lambda M: M.Mlp(32, 128),
               lambda M: M.SwinTransformerLayer(32, 1, window_size=8, shift_size=4), lambda M: M.SwinTransformerBlock(32, 32, 1, 2),
               lambda M: M.SwinTransformerBlock(16, 32, 1, 1), lambda M: M.C3STR(64, 64, 2), lambda M: M.C3STR(128, 128, 2, False)):
        a, b = mk(R), mk(MB)
        assert list(a.state_dict()) == list(b.state_dict())
        assert {k: (v.shape, v.dtype) for k, v in a.state_dict().items()} == {k: (v.shape, v.dtype) for k, v in b.state_dict().items()}
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        b.load_state_dict(fill_state(a, 2).state_dict())          # a restatement (reference-format) state dict loads
    wa = MB.WindowAttention(64, (8, 8), 2, qkv_bias=False)
    assert wa.relative_position_index.dtype == torch.long
    assert torch.equal(wa.relative_position_index, R.WindowAttention(64, (8, 8), 2).relative_position_index)
    blk = MB.C3STR(256, 256, 3).m
    assert blk.tr[0].attn.num_heads == 4 and [layer.shift_size for layer in blk.tr] == [0, 4, 0] and blk.conv is None


def test_swin_graph_matches_the_oracle(monkeypatch):
    from oracle.somi_ref import Model as OModel
    from somi_amd.configs import yolov5_swin_cfg
    from somi_amd.model import Model
    R.register(monkeypatch)
    cfg = yolov5_swin_cfg(0.25, 0.67)
    ref, mine = OModel(cfg), Model(cfg)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert sum(p.numel() for p in mine.parameters()) == sum(p.numel() for p in ref.parameters())
    assert mine.stride.tolist() == ref.stride.tolist() == [8.0, 16.0, 32.0]
    assert mine.save == ref.save
    assert [m.type for m in mine.model] == [m.type for m in ref.model]
    assert mine.model[9].type == 'C3STR' and len(mine.model[9].m.tr) == 2 and mine.model[9].m.tr[0].attn.num_heads == 4
    mine.load_state_dict(ref.state_dict())


def test_swin_cfg_is_the_transformer_yaml_with_c3str():
    from somi_amd.configs import COCO_ANCHORS, yolov5_swin_cfg
    cfg = yolov5_swin_cfg()
    assert (cfg['nc'], cfg['depth_multiple'], cfg['width_multiple'], cfg['anchors']) == (80, 0.33, 0.50, COCO_ANCHORS)
    assert [row[2] for row in cfg['backbone']] == ['Focus', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'C3', 'Conv', 'SPP', 'C3STR']
    assert cfg['backbone'][9] == [-1, 3, 'C3STR', [1024, False]]
    assert cfg['head'][-1] == [[17, 20, 23], 1, 'Detect', ['nc', 'anchors']]


def test_swin_limits_are_explicit():
    from somi_amd import blocks as MB
    from somi_amd.blocks import Act
    from somi_amd.configs import yolov5_swin_cfg
    from somi_amd.model import Model
    for c in (48, 80, 16):                                        # hidden width 24, 40, 8: not a multiple of 32
        with pytest.raises(NotImplementedError, match='multiple of 32'):
            MB.C3STR(c, c, 1)
    with pytest.raises(NotImplementedError, match='head_dim 32'):
        MB.WindowAttention(96, (8, 8), 2, qkv_bias=False)
    with pytest.raises(NotImplementedError, match='window'):
        MB.WindowAttention(32, (7, 7), 1, qkv_bias=False)
    with pytest.raises(NotImplementedError, match='multiple of 32'):
        Model(yolov5_swin_cfg(0.33, 0.33))                        # 344 channels: hidden width 172
    cfg = yolov5_swin_cfg(0.25, 0.33)
    cfg['backbone'][9][2] = 'C3TR'
    with pytest.raises(NotImplementedError, match='outside the SOMI hot path'):
        Model(cfg)
    big = MB.C3STR(704, 704, 1)                                   # hidden width 352: 11 heads, the reference switches stochastic depth on
    assert big.m.tr[0].attn.num_heads == 11 and big.m.tr[0].drop_path_rate == 0.1
    big.eval()                                                    # eval construction is fine; only a training forward is refused
    with pytest.raises(NotImplementedError, match='drop_path'):
        big.train().m.tr[0](Act(torch.zeros(1, 8, 8, 352)))
    assert MB.C3STR(640, 640, 1).m.tr[0].drop_path_rate == 0.0    # 10 heads: no stochastic depth
    for name in ('WindowAttention', 'Mlp', 'SwinTransformerLayer', 'SwinTransformerBlock', 'C3STR'):
        cls = getattr(MB, name)
        assert cls.__dict__['accumulates'] is False and cls.__dict__['folds_pooled'] is False, name
    with pytest.raises(NotImplementedError, match='its own input gradient'):
        MB.C3STR(64, 64, 1).backward(None, dx_out=Act(torch.zeros(1, 8, 8, 64)), accumulate=True)


def test_bias_table_is_in_no_optimizer_group():
    """train.py:125-133 groups `.weight` and `.bias` Parameters only: the table is in none, LayerNorm weights fall into the decayed group."""
    from somi_amd import blocks as MB
    from somi_amd.optim import reference_param_groups
    m = MB.C3STR(64, 64, 2)
    g0, g1, g2 = reference_param_groups(m)
    grouped = {id(p) for p in g0 + g1 + g2}
    names = {id(p): n for n, p in m.named_parameters()}
    outside = sorted(names[i] for i in names if i not in grouped)
    assert outside == ['m.tr.0.attn.relative_position_bias_table', 'm.tr.1.attn.relative_position_bias_table']
    assert any(p is m.m.tr[0].norm1.weight for p in g1) and any(p is m.m.tr[0].norm1.bias for p in g2)
    og0, og1, og2 = reference_param_groups(R.C3STR(64, 64, 2))
    assert (len(g0), len(g1), len(g2)) == (len(og0), len(og1), len(og2))


def test_new_symbols_are_declared_bound_and_exported_at_abi_15():
    from somi_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'somi_hip.h')).read()
    declared = set(re.findall(r'\b(somi_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f'{name} is not declared in include/somi_hip.h'
        assert name in _lib.SIGNATURES, f'{name} is not bound in _lib.SIGNATURES'
        assert hasattr(L, name), f'{name} is not exported'
    assert '#define SOMI_ABI_VERSION 15' in hdr
    assert _lib.lib().somi_abi_version() == _lib.ABI_VERSION == 15
    # no slice parameters: whole contiguous tensors (tests/test_slice_args_host.py keeps a row per entry point that has one)
    for name in NEW_SYMBOLS:
        proto = re.search(name + r'\s*\(([^;]*)\)\s*;', hdr).group(1)
        assert not re.search(r'_coff\b', proto), f'{name} takes a channel slice'


def test_workspace_sizes_and_argument_checks_need_no_device():
    """Sizes are host arithmetic; a rejected argument launches nothing and leaves its reason in somi_last_error()."""
    from somi_amd import _lib
    L = _lib.lib()
    assert L.somi_swin_attention_lse_floats(2, 12, 20, 2) == 2 * 6 * 2 * 64           # padded to 16 x 24: 6 windows
    assert L.somi_swin_attention_bwd_workspace_floats(2, 12, 20, 2) == 2 * 6 * 2 * 225
    assert L.somi_layernorm_bwd_workspace_floats(1000, 32) == 250 * 2 * 32
    fake = 4096                                                   # a plausible aligned address: the checks run before any launch
    assert L.somi_swin_attention_f32(fake, fake, None, 1, 8, 8, 48, 1, 0, fake, None, None) == -2     # SOMI_ENOTIMPL: head_dim 48
    assert b'head_dim 32' in L.somi_last_error()
    assert L.somi_swin_attention_f32(fake, fake, None, 1, 8, 8, 32, 1, 4, fake, None, None) == -1     # a shifted layer without its id map
    assert b'region-id' in L.somi_last_error()
    assert L.somi_swin_attention_f32(fake + 4, fake, None, 1, 8, 8, 32, 1, 0, fake, None, None) == -1
    assert L.somi_swin_attention_f32(fake, fake, None, 1, 8, 8, 32, 1, 3, fake, None, None) == -1
    assert L.somi_swin_attention_backward_f32(fake, fake, None, None, fake, 1, 8, 8, 32, 1, 0, fake, fake, fake, None) == -1
    assert L.somi_layernorm_bwd_nhwc_f32(fake, fake, 1e-5, fake, None, fake, fake, fake, fake, 10, 30, None) == -1
    assert L.somi_gelu_bwd_f32(fake, fake, fake, 6, None) == -1
