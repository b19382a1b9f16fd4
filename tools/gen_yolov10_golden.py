#!/usr/bin/env python3
"""Writes tests/golden/block_{c2f_sc,c2f_nosc,scdown,cib,c2fcib,attnpsa,psa}.npz: the YOLOv10 module set (models/hub/yolov10.yaml) run
through the reference's own classes (models/common.py:2638-2658 C2f, 7192-7255 SCDown / AttentionPSA / PSA, 8981-9013 CIB / C2fCIB) by
oracle.gen_golden.run_block - importing it installs the stub harness that makes the reference importable.  The fixtures hold data only:
inputs and eval / train outputs; weights are regenerated from parameter names by fill_state.  tests/test_yolov10_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_yolov10_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402


def main():
    RC = G.RC
    g = torch.Generator().manual_seed(110)
    r = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    G.run_block('c2f_sc', RC.C2f(32, 32, 2, True), r(2, 32, 9, 11))
    G.run_block('c2f_nosc', RC.C2f(24, 32, 1, False), r(2, 24, 7, 9))
    G.run_block('scdown', RC.SCDown(16, 32, 3, 2), r(2, 16, 13, 17))
    G.run_block('cib', RC.CIB(32, 32, True, e=1.0), r(2, 32, 9, 7))
    G.run_block('c2fcib', RC.C2fCIB(32, 32, 1, True), r(2, 32, 9, 11))
    G.run_block('attnpsa', RC.AttentionPSA(128, 2), r(2, 128, 5, 7))
    G.run_block('psa', RC.PSA(256, 256), r(1, 256, 5, 7))


if __name__ == '__main__':
    main()
