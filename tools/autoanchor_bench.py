"""Times AutoAnchor on the device: a synthetic label set of VisDrone's size (6471 images, seed 1 of the fixture recipe in tests/autoanchor_ref.py,
about 349 000 boxes), n = 16 anchors, 1000 generations.

    python tools/autoanchor_bench.py [--runs 5] [--cpu] [--out profiles/autoanchor_bench_line.json]

Device events bracket the k-means stage (30 restarts, batched Lloyd steps) and the evolution stage of `kmean_anchors`; one warm-up run, then the median
of --runs.  Beside them: the time of a plain device copy of the label table (the floor of one pass over the labels), the launch counts, and with --cpu
the CPU restatement of the same call on this machine's host threads.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --memory-copy-trace
--stats` (no counters) use --runs 1: the trace then shows one small copy per Lloyd step and none per generation."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'yolo-somi_amd')):
    sys.path.insert(0, p)
import autoanchor_ref as R  # noqa: E402
from somi_amd import autoanchor as A  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def one_run(ds, n, gen, seed):
    """kmean_anchors stage by stage -> (anchors, stats)."""
    np.random.seed(seed), random.seed(seed)
    t0 = time.perf_counter()
    wh0 = A.label_wh(ds, 640)
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    obs = wh / s
    starts = np.stack([obs[np.random.choice(len(obs), size=n, replace=False)] for _ in range(30)])
    res, ms_kmeans = timed(lambda: A.lloyd(obs, starts))
    k = min(res, key=lambda r: r[1])[0] * s                      # min keeps the first of equal distances, like scipy's strict <
    k = k[np.argsort(k.prod(1))]
    v = A.draw_mutations(gen, k.shape)
    whd = torch.tensor(wh, dtype=torch.float32).cuda()
    (k, f, accepted), ms_evolve = timed(lambda: A.evolve(whd, k, v, 4.0))
    wall = time.perf_counter() - t0
    steps = [r[2] for r in res]
    return k[np.argsort(k.prod(1))], dict(ms_kmeans=ms_kmeans, ms_evolve=ms_evolve, wall_s=wall, lloyd_steps_batched=max(steps),
                                         lloyd_steps_total=sum(steps), accepted=len(accepted), fitness=f / len(wh), n_fit=len(wh))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=6471)
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--gen', type=int, default=1000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--cpu', action='store_true', help='also time the CPU restatement (minutes)')
    ap.add_argument('--out')
    args = ap.parse_args()
    wh_norm, counts, shapes = R.synth_label_set(args.images, 1)
    ds = R.LabelSet(wh_norm, counts, shapes)
    if args.runs > 1:
        one_run(ds, args.n, args.gen, 0)                          # warm-up: library load, allocator, first launches
    runs = [one_run(ds, args.n, args.gen, 0) for _ in range(args.runs)]
    assert all(np.array_equal(runs[0][0], r[0]) for r in runs), 'runs differ'
    st = [r[1] for r in runs]
    med = lambda key: statistics.median(s[key] for s in st)       # noqa: E731
    n_fit, steps = st[0]['n_fit'], st[0]['lloyd_steps_batched']
    whd = torch.empty(n_fit, 2, dtype=torch.float32, device='cuda')
    dst = torch.empty_like(whd)
    copies = sorted(timed(lambda: dst.copy_(whd))[1] for _ in range(20))
    line = dict(tool='autoanchor_bench', images=args.images, boxes=int(len(wh_norm)), boxes_fit=n_fit, n=args.n, gen=args.gen, runs=args.runs,
                kmeans_ms=round(med('ms_kmeans'), 3), evolve_ms=round(med('ms_evolve'), 3), wall_s=round(med('wall_s'), 3),
                lloyd_steps_batched=steps, lloyd_steps_total=st[0]['lloyd_steps_total'], kmeans_launches=2 * steps,
                kmeans_readbacks=steps, ms_per_lloyd_step=round(med('ms_kmeans') / steps, 4),
                evolve_launches=2 * args.gen + 2, evolve_readbacks_per_generation=0, us_per_generation=round(1e3 * med('ms_evolve') / max(args.gen, 1), 3),
                label_bytes_per_pass=n_fit * 8, obs_bytes_per_lloyd_step=n_fit * 16 * 30, copy_of_labels_us=round(1e3 * copies[len(copies) // 2], 3),
                accepted=st[0]['accepted'], fitness=round(st[0]['fitness'], 6), device=torch.cuda.get_device_name(0))
    if args.cpu:
        np.random.seed(0), random.seed(0)
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        t0 = time.perf_counter()
        k_cpu, info = R.kmean_anchors(ds, n=args.n, img_size=640, thr=4.0, gen=args.gen, return_info=True)
        line.update(cpu_restatement_s=round(time.perf_counter() - t0, 2), cpu_threads=torch.get_num_threads(),
                    cpu_fitness=round(info.fitness_sum / info.n_fit, 6), cpu_accepted=len(info.accepted),
                    max_abs_diff_vs_cpu_px=float(np.abs(k_cpu - runs[0][0]).max()))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
