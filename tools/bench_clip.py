"""What gradient clipping costs per train step: a same-session A/B on bench.py's own workload.

    python tools/bench_clip.py [--workload audio_gru] [--steps 100] [--warmup 20] [--rounds 6] [--out FILE]

ONE workload (bench.build_workload: model, optimizer, synthetic batch, the step closure bench.py times) is stepped with the
optimizer's clipping off and on in alternation, `rounds` runs a side of `steps` steps each, wall time between two device
synchronisations.  Off is the launch sequence of the plain optimizer; on adds dep_grad_sqnorm and swaps dep_adam_step for
dep_adam_step_clipped (max_grad_norm 1.0, skip_nonfinite off).  Prints one JSON line: per-side ms per step of every run, the medians,
their difference and the spread (max - min) of each side.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='audio_gru')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--max-grad-norm', type=float, default=1.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    spec = importlib.util.spec_from_file_location('dep_bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = torch.device('cuda:0')
    wl = bench.build_workload(a.workload, dev, 0, 1)
    opt, step = wl['optimizer'], wl['step']

    def run(on, n):
        opt.max_grad_norm = a.max_grad_norm if on else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for on in (False, True):
        run(on, a.warmup)
    ms = {False: [], True: []}
    for r in range(a.rounds):
        for on in ((False, True) if r % 2 == 0 else (True, False)):         # neither side always runs first
            ms[on].append(run(on, a.steps))
    wl['model'].check_health()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {'workload': a.workload, 'steps': a.steps, 'rounds': a.rounds, 'ms_per_step_off': [round(v, 4) for v in ms[False]],
           'ms_per_step_on': [round(v, 4) for v in ms[True]], 'median_off': round(med[False], 4), 'median_on': round(med[True], 4),
           'delta_ms': round(med[True] - med[False], 4), 'spread_off': round(max(ms[False]) - min(ms[False]), 4),
           'spread_on': round(max(ms[True]) - min(ms[True]), 4), 'grad_stats': opt.grad_stats()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
