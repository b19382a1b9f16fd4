#!/usr/bin/env python3
"""Writes tests/golden/block_asff{0,1,2}.npz and tests/golden/block_asff_detect.npz: the reference's own ASFF(0), ASFF(1), ASFF(2)
(models/common.py:5500-5567) and ASFF_Detect(3, anchors, (128, 256, 512)) (models/yolo.py:172-184) in eval and train mode, on one pyramid
(P5 2x3, P4 4x6, P3 8x12, batch 1) - importing oracle.gen_golden installs the stub harness that makes the reference importable.  The fixtures hold
data only: the three inputs and the outputs (weights are regenerated from parameter names by fill_state).  The head's fixture pins the chain the
reference forms by rewriting its input list in place.  tests/test_asff_host.py reads them.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tools/gen_asff_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as G  # noqa: E402

ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
STRIDES = (8.0, 16.0, 32.0)


def main():
    RC, RY = G.RC, G.RY
    g = torch.Generator().manual_seed(130)
    # inputs on a grid of 1/2: they compress to a fraction of their size
    r = lambda *s: (torch.randn(*s, generator=g) * 2).round() / 2    # noqa: E731
    p5, p4, p3 = r(1, 512, 2, 3), r(1, 256, 4, 6), r(1, 128, 8, 12)
    for level in range(3):
        mod = G.fill_state(RC.ASFF(level), 0)
        RY.initialize_weights(mod)
        rec = dict(in0=p5, in1=p4, in2=p3)
        for mode in ('eval', 'train'):
            mod.train(mode == 'train')
            with torch.no_grad():
                rec[f'out_{mode}'] = mod(p5.clone(), p4.clone(), p3.clone())
        G.save(f'block_asff{level}', **rec)
    anchors = torch.tensor(ANCHORS).float().view(3, -1, 2) / torch.tensor(STRIDES).view(-1, 1, 1)     # grid units, as Model leaves them
    head = G.fill_state(RY.ASFF_Detect(3, anchors.view(3, -1).tolist(), (128, 256, 512)), 0)
    RY.initialize_weights(head)
    head.stride = torch.tensor(STRIDES)
    rec = dict(in0=p3, in1=p4, in2=p5, anchors=anchors)          # the head's own order: [P3, P4, P5]
    head.eval()
    with torch.no_grad():
        z, raws = head([p3.clone(), p4.clone(), p5.clone()])
    rec['z_eval'] = z
    rec.update({f'raw{i}_eval': t for i, t in enumerate(raws)})
    head.train()
    with torch.no_grad():
        rec.update({f'raw{i}_train': t for i, t in enumerate(head([p3.clone(), p4.clone(), p5.clone()]))})
    G.save('block_asff_detect', **rec)


if __name__ == '__main__':
    main()
