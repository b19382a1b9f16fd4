"""CPU restatement of what the remaining stock hub graphs need beyond the oracle's own module set (models/hub/yolov3*.yaml, yolov5-fpn / -panet /
-p6 / -p7.yaml): BottleneckCSP (models/common.py:1512-1538) on the oracle's Conv / Bottleneck, written from its semantics so that torch autograd
runs through it, and a parse_model that also takes the two parameter-free nn.* names of yolov3-tiny.  tests/test_hub_host.py pins the
restatement to the reference's own classes through the tests/golden/hub_*.npz fixtures."""
import torch
import torch.nn as nn

from oracle.somi_ref import blocks as OB


class BottleneckCSP(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = OB.Conv(c1, c_, 1, 1)
        self.cv2 = nn.Conv2d(c1, c_, 1, 1, bias=False)
        self.cv3 = nn.Conv2d(c_, c_, 1, 1, bias=False)
        self.cv4 = OB.Conv(2 * c_, c2, 1, 1)
        self.bn = nn.BatchNorm2d(2 * c_)
        self.act = nn.SiLU()
        self.m = nn.Sequential(*(OB.Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))

    def forward(self, x):
        y1 = self.cv3(self.m(self.cv1(x)))
        y2 = self.cv2(x)
        return self.cv4(self.act(self.bn(torch.cat((y1, y2), 1))))


class PadPool(nn.Module):
    """nn.ZeroPad2d(pad) + nn.MaxPool2d(k, s, 0) as one module (the pair of yolov3-tiny's layers 11 / 12), for block-level comparisons."""

    def __init__(self, pad=(0, 1, 0, 1), k=2, s=1):
        super().__init__()
        self.pad, self.pool = nn.ZeroPad2d(list(pad)), nn.MaxPool2d(k, s, 0)

    def forward(self, x):
        return self.pool(self.pad(x))


_PASS_THROUGH = {'nn.MaxPool2d': nn.MaxPool2d, 'nn.ZeroPad2d': nn.ZeroPad2d}


def register(monkeypatch):
    """BottleneckCSP in the oracle's parse_model tables, and the two nn.* names through a parse_model of this file's own that hands every other row
    to the oracle's (test-time only: nothing under oracle/ changes)."""
    from oracle.somi_ref import model as OM
    monkeypatch.setattr(OM, '_CH_MODULES', dict(OM._CH_MODULES, BottleneckCSP=BottleneckCSP))
    monkeypatch.setattr(OM, '_REPEAT_INSIDE', set(OM._REPEAT_INSIDE) | {'BottleneckCSP'})
    inner = OM.parse_model

    def parse_model(d, ch):
        """The oracle's parser row by row; a row with a parameter-free nn.* module (channels pass through, models/yolo.py:1647-1648) is built here
        and stands in the oracle's pass as an nn.Upsample row, which takes the same branch (c2 = ch[f])."""
        rows = d['backbone'] + d['head']
        swapped = dict(d, backbone=[], head=[[f, n, 'nn.Upsample', [None, 1, 'nearest']] if name in _PASS_THROUGH else [f, n, name, args]
                                             for f, n, name, args in rows])
        seq, save = inner(swapped, ch)
        layers = list(seq)
        for i, (f, n, name, args) in enumerate(rows):
            if name in _PASS_THROUGH:
                m_ = _PASS_THROUGH[name](*args)
                m_.i, m_.f, m_.type, m_.np = i, f, name, 0
                layers[i] = m_
        return nn.Sequential(*layers), save
    monkeypatch.setattr(OM, 'parse_model', parse_model)


P6_ANCHORS = [[19, 27, 44, 40, 38, 94], [96, 68, 86, 152, 180, 137], [140, 301, 303, 264, 238, 542], [436, 615, 739, 380, 925, 792]]
"""The P3..P6 anchors of models/hub/yolov5s6.yaml."""
P7_ANCHORS_256 = [[5, 6, 8, 14, 15, 11], [15, 30, 31, 22, 29, 59], [58, 45, 78, 99, 90, 60], [100, 120, 130, 90, 90, 150], [150, 180, 200, 140, 170, 230]]
"""Five ascending anchor sets for a 256 px image (strides 8..128): the yamls ship none for P7 (`anchors: 3`)."""

HUB = {'yolov3': ('yolov3_cfg', ''), 'yolov3-spp': ('yolov3_cfg', 'spp'), 'yolov3-tiny': ('yolov3_cfg', 'tiny'), 'yolov5-fpn': ('yolov5_hub_cfg', 'fpn'),
       'yolov5-panet': ('yolov5_hub_cfg', 'panet'), 'yolov5-p6': ('yolov5_hub_cfg', 'p6'), 'yolov5-p7': ('yolov5_hub_cfg', 'p7')}


def hub_cfg(name, **kw):
    from somi_amd import configs
    fn, arg = HUB[name]
    return getattr(configs, fn)(arg, **kw)
