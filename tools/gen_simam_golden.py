#!/usr/bin/env python3
"""Writes tests/golden/block_simam.npz, block_simam_slicing.npz, block_simam_windows.npz, block_simam_windows_overlap.npz,
block_simam_conv_sws.npz and block_simam_pssimam.npz: the reference's own SimAM(16) at 2x16x5x7 (models/common.py:2915-2939),
SimAMWithSlicing(16) at 2x16x7x5, odd both ways (:9374-9408), SimAMWithFlexibleSlicing(16, 4, 0.0) and (16, 4, 0.5) at 2x16x11x13 (:9411-9480:
23 pixels no window covers, and pixels under four windows), Conv_SWS(16, 32, 4, 0.5, 1e-4, 3, 2) at 2x16x11x13 (:9483-9495) and
PSSimAM(32, 32) at 2x32x5x7 (:2942-2961), in eval and train mode on one input each.  Importing oracle.gen_golden installs the stub harness
that makes the reference importable.  The fixtures hold data only: the input and the two outputs (weights are regenerated from parameter
names by fill_state).  tests/test_simam_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_simam_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(211)

    def grid(*shape):
        return (torch.randn(*shape, generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses to a fraction of its size
    xw = grid(2, 16, 11, 13)
    cases = {'block_simam': (lambda: RC.SimAM(16), grid(2, 16, 5, 7)),
             'block_simam_slicing': (lambda: RC.SimAMWithSlicing(16), grid(2, 16, 7, 5)),
             'block_simam_windows': (lambda: RC.SimAMWithFlexibleSlicing(16, 4, 0.0), xw),
             'block_simam_windows_overlap': (lambda: RC.SimAMWithFlexibleSlicing(16, 4, 0.5), xw),
             'block_simam_conv_sws': (lambda: RC.Conv_SWS(16, 32, 4, 0.5, 1e-4, 3, 2), xw),
             'block_simam_pssimam': (lambda: RC.PSSimAM(32, 32), grid(2, 32, 5, 7))}
    for name, (make, inp) in cases.items():
        mod = G.fill_state(make(), 0)
        RY.initialize_weights(mod)
        rec = dict(x=inp)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(inp.clone())
        G.save(name, **rec)


if __name__ == '__main__':
    write_fixtures()
