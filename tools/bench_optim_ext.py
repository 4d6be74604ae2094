"""What AMSGrad and the fused average of the weights cost per optimizer step, on the parameter ranges of bench.py's model.

    python tools/bench_optim_ext.py [--workload audio_gru] [--steps 2000] [--warmup 200] [--rounds 5] [--out FILE]

bench.build_workload makes the model; one train step leaves gradients in place, and from then on ONLY optimizer.step() is timed
(wall time between two device synchronisations, `steps` updates a run), for five optimizers over the same parameters:
    plain     nn.AdamW as bench.py builds it            (dep_adam_step per range)
    amsgrad   amsgrad=True                               (dep_adam_step_ext per range, + vmax read and written)
    ema       ema_decay=0.999                            (dep_adam_step_ext per range, + the average read and written)
    both      amsgrad=True, ema_decay=0.999
    separate  plain, then avg.lerp_(parameters, 1 - d)   what a user does without the fusion: one more launch and pass per owner
The cases alternate inside every round, the order reversed every other round.  Prints one JSON line: ms per step of every run, the
medians and the spread (max - min) of each case.
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
DECAY = 0.999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='audio_gru')
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    spec = importlib.util.spec_from_file_location('dep_bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from icassp2022_depression_amd import nn
    wl = bench.build_workload(a.workload, torch.device('cuda:0'), 0, 1)
    model, mod, lr = wl['model'], wl['mod'], wl['cfg']['learning_rate']
    wl['step']()                                              # gradients of one real step; nothing clears them below
    torch.cuda.synchronize()
    model.check_health()

    def make(**kw):
        return nn.AdamW(mod.get_param_group(model), lr=lr, **kw)
    opts = {'plain': make(), 'amsgrad': make(amsgrad=True), 'ema': make(ema_decay=DECAY), 'both': make(amsgrad=True, ema_decay=DECAY),
            'separate': make()}
    avg = model._flat.clone()

    def one(name):
        opts[name].step()
        if name == 'separate':
            avg.lerp_(model._flat, 1.0 - DECAY)

    def run(name, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for name in opts:
        run(name, a.warmup)
    ms = {name: [] for name in opts}
    for r in range(a.rounds):
        for name in (list(opts) if r % 2 == 0 else list(opts)[::-1]):
            ms[name].append(run(name, a.steps))
    n_par = int(model._flat.numel())
    ranges = [(int(e - s)) for _, rs in opts['plain']._plan() for _, s, e in rs]
    res = {'workload': a.workload, 'parameters': n_par, 'ranges': ranges, 'steps': a.steps, 'rounds': a.rounds, 'ema_decay': DECAY,
           'ms_per_step': {k: [round(v, 5) for v in vs] for k, vs in ms.items()},
           'median_ms': {k: round(statistics.median(vs), 5) for k, vs in ms.items()},
           'spread_ms': {k: round(max(vs) - min(vs), 5) for k, vs in ms.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
