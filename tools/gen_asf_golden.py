#!/usr/bin/env python3
"""Writes tests/golden/block_asf_zoom_cat.npz, block_asf_scalseq.npz, block_asf_attention_64.npz and block_asf_attention_128.npz: the
reference's own Zoom_cat at l 2x4x4x8, m 2x8x2x4, s 2x12x1x2 - unequal widths - (models/common.py:4312-4327), ScalSeq(8) at p3 2x8x4x8,
p4 2x512x2x4, p5 2x1024x1x2 (:4330-4355), attention_model(64) at 2x64x5x7 (ECA kernel size 3) and attention_model(128) at 1x128x3x2 (kernel
size 5) (:4358-4424), in eval and train mode on one set of inputs each.  Importing oracle.gen_golden installs the stub harness that makes
the reference importable.  The fixtures hold data only: the inputs (x0, x1, ..) and the two outputs (weights are regenerated from parameter
names by fill_state).  tests/test_asf_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_asf_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def write_fixtures():
    from oracle import gen_golden as G
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(307)

    def grid(*shape):
        return (torch.randn(*shape, generator=g) * 2).round() / 2     # a grid of 1/2: the file compresses to a fraction of its size
    cases = {'block_asf_zoom_cat': (lambda: RC.Zoom_cat(8), [grid(2, 4, 4, 8), grid(2, 8, 2, 4), grid(2, 12, 1, 2)]),
             'block_asf_scalseq': (lambda: RC.ScalSeq(8), [grid(2, 8, 4, 8), grid(2, 512, 2, 4), grid(2, 1024, 1, 2)]),
             'block_asf_attention_64': (lambda: RC.attention_model(64), [grid(2, 64, 5, 7), grid(2, 64, 5, 7)]),
             'block_asf_attention_128': (lambda: RC.attention_model(128), [grid(1, 128, 3, 2), grid(1, 128, 3, 2)])}
    for name, (make, inputs) in cases.items():
        mod = G.fill_state(make(), 0)
        RY.initialize_weights(mod)
        rec = {f'x{i}': t for i, t in enumerate(inputs)}
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod([t.clone() for t in inputs])
        G.save(name, **rec)


if __name__ == '__main__':
    write_fixtures()
