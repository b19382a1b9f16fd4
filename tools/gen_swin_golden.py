#!/usr/bin/env python3
"""Writes tests/golden/block_{c3str,c3str_h2,swinblock_small}.npz and tests/golden/swin_shift_masks.npz: the Swin module set run through
the reference's own classes (models/common.py:1267-1378 SwinTransformerLayer / SwinTransformerBlock, 1632-1637 C3STR) by
oracle.gen_golden.run_block - importing it installs the stub harness that makes the reference importable.  The fixtures hold data only:
inputs and eval / train outputs (weights are regenerated from parameter names by fill_state), and for two map sizes which token pairs
create_mask separates.  tests/test_swin_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_swin_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402


def main():
    RC = G.RC
    g = torch.Generator().manual_seed(120)
    # inputs on a grid of 1/2: they compress to a fraction of their size, which keeps every file below the largest block fixture there was
    r = lambda *s: (torch.randn(*s, generator=g) * 2).round() / 2    # noqa: E731
    G.run_block('c3str', RC.C3STR(64, 64, 2), r(1, 64, 12, 20))                   # both axes padded, non-square, a plain and a shifted layer
    G.run_block('c3str_h2', RC.C3STR(128, 128, 2, False), r(1, 128, 16, 8))       # two heads, exact multiples of the window
    G.run_block('swinblock_small', RC.SwinTransformerBlock(32, 32, 1, 2), r(2, 32, 5, 3))   # smaller than one window
    # create_mask(x, H, W) on two more sizes, in the layer's own frame: 1 where the mask is -100
    layer = RC.SwinTransformerLayer(32, 1, window_size=8, shift_size=4)
    rec = {}
    for H, W in ((5, 3), (20, 12)):
        rec[f'differs_{H}x{W}'] = (layer.create_mask(torch.zeros(1), H, W) != 0).to(torch.uint8)
    G.save('swin_shift_masks', **rec)


if __name__ == '__main__':
    main()
