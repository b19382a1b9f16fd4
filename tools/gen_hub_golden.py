#!/usr/bin/env python3
"""Writes tests/golden/block_hub_*.npz and tests/golden/hub_graphs.json: what the remaining stock hub graphs add (models/hub/yolov3*.yaml,
yolov5-fpn / -panet / -p6 / -p7.yaml), run through the reference's own classes by oracle.gen_golden.run_block - importing it installs the stub
harness that makes the reference importable.  Blocks: BottleneckCSP (models/common.py:1512-1538) with and without shortcut and with n = 2,
SPP (:1806-1826) with (3, 5, 7) and (3, 5), an nn.Sequential of two Bottlenecks (models/yolo.py:1650), and nn.ZeroPad2d([0, 1, 0, 1]) +
nn.MaxPool2d(2, 1, 0) on an odd-sized map with negative values.  The fixtures hold data only: inputs and eval / train outputs; weights are
regenerated from parameter names by fill_state.  hub_graphs.json records, for the seven yamls built by the reference's own Model, the
parameter count, the strides and the number of state_dict entries.  tests/test_hub_host.py reads both.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_hub_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from oracle import gen_golden as G  # noqa: E402

YAMLS = ('yolov3', 'yolov3-spp', 'yolov3-tiny', 'yolov5-fpn', 'yolov5-panet', 'yolov5-p6', 'yolov5-p7')


def main():
    RC = G.RC
    g = torch.Generator().manual_seed(120)
    r = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    G.run_block('hub_csp_sc', RC.BottleneckCSP(32, 32, 1, True), r(2, 32, 9, 11))
    G.run_block('hub_csp_nosc', RC.BottleneckCSP(24, 32, 1, False), r(2, 24, 7, 9))
    G.run_block('hub_csp_n2', RC.BottleneckCSP(32, 64, 2, True), r(2, 32, 8, 6))
    G.run_block('hub_spp357', RC.SPP(32, 32, (3, 5, 7)), r(2, 32, 9, 6))
    G.run_block('hub_spp35', RC.SPP(32, 24, (3, 5)), r(2, 32, 2, 3))
    G.run_block('hub_seq2', nn.Sequential(RC.Bottleneck(32, 32), RC.Bottleneck(32, 32)), r(2, 32, 7, 9))
    G.run_block('hub_padpool', nn.Sequential(nn.ZeroPad2d([0, 1, 0, 1]), nn.MaxPool2d(2, 1, 0)), r(2, 8, 5, 7) - 0.5, train_too=False)
    # Focus hands `act=True` into Conv's dilation slot (models/common.py:1993); torch releases before 2.x took dilation=True as 1, this one's conv2d
    # refuses the bool, so nn.Conv2d gets it as the integer it stands for while the reference's Model builds the Focus graphs
    conv_init = nn.Conv2d.__init__

    def init(self, *a, **k):
        a = list(a)
        if len(a) > 5 and a[5] is True:
            a[5] = 1
        if k.get('dilation') is True:
            k['dilation'] = 1
        conv_init(self, *a, **k)
    nn.Conv2d.__init__ = init
    rec = {}
    for name in YAMLS:
        m = G.RY.Model(os.path.join(G.REF, 'models', 'hub', name + '.yaml'))
        rec[name] = dict(params=sum(p.numel() for p in m.parameters()), strides=[float(s) for s in m.stride],
                         entries=len(m.state_dict()), layers=len(m.model))
    with open(os.path.join(ROOT, 'tests', 'golden', 'hub_graphs.json'), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
