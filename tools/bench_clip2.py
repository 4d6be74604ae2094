"""What the value clamp, the per-group norms and the landed step count cost per train step: a same-session A/B on bench.py's own
workload, by the method of tools/bench_clip.py.

    python tools/bench_clip2.py [--workload audio_gru] [--steps 100] [--warmup 20] [--rounds 6] [--sides clipped,value,...] [--lib SO] [--out FILE]

ONE workload (bench.build_workload) is stepped with the optimizer's options switched between the `sides`, alternated round by round
(the order reverses every round, so that no side always runs first), `rounds` runs a side of `steps` steps each, wall time between
two device synchronisations.  Sides: `default` (the plain optimizer), `clipped` (max_grad_norm 1.0: dep_grad_sqnorm +
dep_adam_step_clipped, the parent's clipped step -- tools/isa_diff.py shows its kernels unchanged), and on top of `clipped`: `value`
(max_grad_value), `per_group` (clip_per_group), `landed` (skip_nonfinite, count_skipped=False), `all`; `skip` is `clipped` with
skip_nonfinite, the fair baseline of `landed`.  --lib: another build of the library (the parent's, for the `default` and `clipped`
sides across builds; it may lack the new symbols).  Prints one JSON line: per side the ms per step of every run, the median and the range."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFF = dict(max_grad_norm=None, max_grad_value=None, clip_per_group=False, skip_nonfinite=False, count_skipped=True)
SIDES = {
    'default': {},
    'clipped': dict(max_grad_norm=1.0),
    'skip': dict(max_grad_norm=1.0, skip_nonfinite=True),
    'value': dict(max_grad_norm=1.0, max_grad_value=1e-3),
    'per_group': dict(max_grad_norm=1.0, clip_per_group=True),
    'landed': dict(max_grad_norm=1.0, skip_nonfinite=True, count_skipped=False),
    'all': dict(max_grad_norm=1.0, max_grad_value=1e-3, clip_per_group=True, skip_nonfinite=True, count_skipped=False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='audio_gru')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--sides', default='clipped,value,per_group,skip,landed,all')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--tag', default=None, help="what the result line calls the library (default: 'in-tree', or --lib's file name)")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sides = a.sides.split(',')
    if a.lib:
        os.environ['DEP_LIB_PATH'] = os.path.abspath(a.lib)
    import torch
    from icassp2022_depression_amd import _lib as L
    L.load(optional=('dep_adam_step_opt', 'dep_grad_clip_value') if a.lib else ())
    spec = importlib.util.spec_from_file_location('dep_bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    wl = bench.build_workload(a.workload, torch.device('cuda:0'), 0, 1)
    opt, step = wl['optimizer'], wl['step']

    def run(side, n):
        for k, v in dict(OFF, **SIDES[side]).items():
            setattr(opt, k, v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for s in sides:
        run(s, a.warmup)
    ms = {s: [] for s in sides}
    for r in range(a.rounds):
        for s in (sides if r % 2 == 0 else sides[::-1]):
            ms[s].append(run(s, a.steps))
    wl['model'].check_health()
    res = {'workload': a.workload, 'steps': a.steps, 'rounds': a.rounds, 'lib': a.tag or (os.path.basename(a.lib) if a.lib else 'in-tree'),
           'sides': {s: {'ms_per_step': [round(v, 4) for v in ms[s]], 'median': round(statistics.median(ms[s]), 4),
                         'min': round(min(ms[s]), 4), 'max': round(max(ms[s]), 4)} for s in sides}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
