#!/usr/bin/env python3
"""Writes tests/golden/block_{carafe,carafe_k3,dysample,dysample_g2}.npz: the two learned 2x upsamplers of the neck run through the reference's
own classes (models/common.py:4450-4490 CARAFE, 4246-4309 DySample) by oracle.gen_golden.run_block - importing it installs the stub harness
that makes the reference importable.  The fixtures hold data only: inputs and eval / train outputs; weights (and DySample's init_pos buffer,
which fill_state fills like every floating-point entry of the state dict) are regenerated from parameter names by fill_state.
tests/test_upsample_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_upsample_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402


def main():
    RC = G.RC
    g = torch.Generator().manual_seed(120)
    r = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    G.run_block('carafe', RC.CARAFE(32, 3, 5), r(2, 32, 7, 9))
    G.run_block('carafe_k3', RC.CARAFE(16, 1, 3, 16), r(2, 16, 6, 5))
    G.run_block('dysample', RC.DySample(32), r(2, 32, 7, 9))
    G.run_block('dysample_g2', RC.DySample(24, 2, 'lp', 2), r(2, 24, 6, 5))


if __name__ == '__main__':
    main()
