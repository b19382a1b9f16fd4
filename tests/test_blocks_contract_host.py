"""What the blocks declare for Model's graph walk (somi_amd.blocks: `accumulates`, `folds_pooled`, `reduction`): the declared sets are the
ones the walk used to spell out by class, every declaring class has the keywords the walk passes, and the strides the declared reduction
factors give are the ones each shipped graph had before the blocks declared them."""
import inspect

import pytest
import torch.nn as nn

ACCUMULATES = {'Conv', 'DWConv', 'C2fCBAM', 'C3', 'C3Ghost', 'SPPF', 'SPP', 'ODConv_3rd', 'GhostConv', 'GhostBottleneck', 'C2f', 'C2fCIB', 'SCDown',
               'PSA', 'BottleneckCSP'}
FOLDS_POOLED = {'Conv', 'C2fCBAM'}


def _block_classes():
    from somi_amd import blocks as B
    return {n: c for n, c in vars(B).items() if inspect.isclass(c) and issubclass(c, nn.Module) and c.__module__ == B.__name__}


def test_declared_sets_are_the_ones_the_walk_named():
    cls = _block_classes()
    assert {n for n, c in cls.items() if getattr(c, 'accumulates', False)} == ACCUMULATES
    assert {n for n, c in cls.items() if getattr(c, 'folds_pooled', False)} == FOLDS_POOLED
    assert cls['DWConv'].__dict__['folds_pooled'] is False, 'DWConv inherits from Conv and must switch the pooled folding off itself'
    for n in ('CARAFE', 'DySample', 'Bottleneck', 'CIB', 'Focus', 'MaxPool2d', 'Repeat'):
        assert cls[n].accumulates is False, n
    assert {n for n, c in cls.items() if getattr(c, 'squeezes_input', False)} == {'ODConv_3rd'}


def test_declaring_classes_take_the_keywords_the_walk_passes():
    cls = _block_classes()
    for n in sorted(ACCUMULATES):
        names = list(inspect.signature(cls[n].backward).parameters)
        assert names[:5] == ['self', names[1], 'dx_out', 'accumulate', 'need_dx'], f'{n}.backward{tuple(names)}'
    for n in sorted(FOLDS_POOLED):
        assert 'pooled' in inspect.signature(cls[n].backward).parameters and 'pool' in inspect.signature(cls[n].forward).parameters, n
    assert 'defer_pool' in inspect.signature(cls['ODConv_3rd'].backward).parameters
    # every single-input block the parser can place takes the same four first
    for n in ('Upsample', 'CARAFE', 'DySample', 'SEAM', 'Bottleneck', 'MaxPool2d', 'ZeroPad2d', 'Repeat', 'Focus', 'CIB', 'DCNv3_YOLO', 'CBAMBottleneck',
              'AttentionPSA'):
        names = list(inspect.signature(cls[n].backward).parameters)
        assert names[2:5] == ['dx_out', 'accumulate', 'need_dx'], f'{n}.backward{tuple(names)}'


def test_every_accumulating_class_has_a_gpu_case():
    from test_accumulate_gpu import CASES
    assert {c[0] for c in CASES} == ACCUMULATES


def _graphs():
    from somi_amd import configs as C
    for up in ('nearest', 'carafe', 'dysample'):
        for dcn in (False, True):
            yield f'somi dcn={dcn} {up}', C.somi_cfg(0.25, 0.33, dcn=dcn, upsample=up), [4.0, 8.0, 16.0, 32.0]
        for ver in ('6.0', '5.0'):
            yield f'yolov5 {ver} {up}', C.yolov5_cfg(version=ver, upsample=up), [8.0, 16.0, 32.0]
        yield f'yolov10 {up}', C.yolov10_cfg(0.25, 0.33, upsample=up), [8.0, 16.0, 32.0]
    yield 'yolov5-ghost', C.yolov5_ghost_cfg(), [8.0, 16.0, 32.0]
    yield 'yolov3', C.yolov3_cfg('', 0.25, 0.33), [8.0, 16.0, 32.0]
    yield 'yolov3-spp', C.yolov3_cfg('spp', 0.25, 0.33), [8.0, 16.0, 32.0]
    yield 'yolov3-tiny', C.yolov3_cfg('tiny', 0.25, 0.33), [16.0, 32.0]
    yield 'yolov5-fpn', C.yolov5_hub_cfg('fpn', 0.25, 0.33), [8.0, 16.0, 32.0]
    yield 'yolov5-panet', C.yolov5_hub_cfg('panet', 0.25, 0.33), [8.0, 16.0, 32.0]
    yield 'yolov5-p6', C.yolov5_hub_cfg('p6', 0.25, 0.33), [8.0, 16.0, 32.0, 64.0]
    yield 'yolov5-p7', C.yolov5_hub_cfg('p7', 0.25, 0.33), [8.0, 16.0, 32.0, 64.0, 128.0]


def test_shipped_graphs_keep_their_strides_and_every_layer_declares():
    """Model built on the CPU (construction needs no device) for every shipped config and variant; the strides are the literals above."""
    from somi_amd import blocks as B
    from somi_amd.model import Model
    seen = set()
    for name, cfg, want in _graphs():
        m = Model(cfg)
        assert m.stride.tolist() == want, f'{name}: strides {m.stride.tolist()}, were {want}'
        layers = [sub for layer in m.model for sub in ([layer, *layer] if isinstance(layer, B.Repeat) else [layer])]
        for layer in layers:
            for attr in ('accumulates', 'folds_pooled', 'reduction'):
                assert hasattr(type(layer), attr), f'{name}: layer {layer.i if hasattr(layer, "i") else "?"} ({type(layer).__name__}) declares no {attr}'
        seen |= {type(layer).__name__ for layer in layers}
    assert {'Conv', 'ODConv_3rd', 'C2fCBAM', 'SEAM', 'SPPF', 'BiFPN', 'Upsample', 'CARAFE', 'DySample', 'DCNv3_YOLO', 'Focus', 'C3', 'C3Ghost', 'GhostConv',
            'SPP', 'Concat', 'C2f', 'C2fCIB', 'SCDown', 'PSA', 'Bottleneck', 'BottleneckCSP', 'MaxPool2d', 'ZeroPad2d', 'Repeat', 'Detect',
            'DecoupledDetect'} <= seen, sorted(seen)


def test_the_launch_timer_is_inert_while_nothing_profiles():
    """ops._timed around a launch: without a PROFILE list it creates no events and never asks for the entry's name / work / key."""
    from somi_amd import ops
    assert ops.PROFILE is None
    t = ops._timed(lambda: 1 / 0)
    with t:
        pass
    assert t.ev is None
