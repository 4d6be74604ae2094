"""What a ragged train step costs, next to the dense one (not bench.py, whose headline stays the dense step).

    python tools/bench_ragged.py --workload audio_gru --legs dense,ragged_full,ragged_half --steps 100 --warmup 10 --windows 5
    python tools/bench_ragged.py --workload audio_gru --legs dense --lib /path/to/another/libdep_rnn.so     # e.g. the parent commit's build

The model, optimizer and synthetic HBM-resident batch are bench.build_workload()'s (BASELINE cfg2 = audio_gru, cfg3 = text_bilstm:
B = 512, T = 300, dropout 0.5).  Legs:
    dense        model(x)                              -- the fused two-layer GRU launches at cfg2
    ragged_full  model(x, lengths = T everywhere)      -- the per-layer cluster sweeps + the predicate, same work
    ragged_half  model(x, lengths uniform in [T/2, T]) -- what skipping padded work could buy is the distance to ragged_full
Every window is `--steps` train steps between two device events; the legs of one process alternate window by window, so that they see the
same clocks and neighbours.  `--lib` loads another build of the library for the dense leg (one process per library: compare the
processes' dense windows for the run-to-run spread).  One JSON line per process.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='audio_gru', choices=['audio_gru', 'text_bilstm'])
    ap.add_argument('--legs', default='dense,ragged_full,ragged_half')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--lib', default=None, help='another build of libdep_rnn.so (dense leg only: it may predate the ragged entry points)')
    ap.add_argument('--tag', default='')
    a = ap.parse_args()
    legs = a.legs.split(',')
    if a.lib:
        if legs != ['dense']:
            ap.error('--lib times the dense leg only')
        os.environ['DEP_LIB_PATH'] = os.path.abspath(a.lib)
    import torch
    from icassp2022_depression_amd import _lib as L
    # --lib: an older build of the same ABI may lack the ragged entry points (the dense step needs none of them)
    L.load(optional=[n for n in L.EXPORTS if n.endswith('_varlen')] if a.lib else ())
    spec = importlib.util.spec_from_file_location('dep_bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    from icassp2022_depression_amd import parallel
    dev = torch.device('cuda:0')
    wl = bench.build_workload(a.workload, dev, 0, 1)
    model, optimizer, criterion, x, y, B, T = wl['model'], wl['optimizer'], wl['criterion'], wl['x'], wl['y'], wl['B'], wl['T']
    g = torch.Generator(device='cpu'); g.manual_seed(7)
    lengths = {'dense': None,
               'ragged_full': torch.full((B,), T, dtype=torch.int32, device=dev),
               'ragged_half': torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int32).to(dev)}

    def step(leg):
        parallel.set_global_count(B)
        optimizer.zero_grad()
        o = model(x) if lengths[leg] is None else model(x, lengths=lengths[leg])
        loss = criterion(o, y)
        loss.backward()
        optimizer.step()
        return loss

    for leg in legs:
        for _ in range(a.warmup):
            step(leg)
    torch.cuda.synchronize()
    model.check_health()
    ms = {leg: [] for leg in legs}
    for _ in range(a.windows):
        for leg in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                loss = step(leg)
            e1.record(); torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / a.steps)
    model.check_health()
    out = {'workload': a.workload, 'tag': a.tag, 'lib': os.environ.get('DEP_LIB_PATH') or 'in-tree', 'B': B, 'T': T, 'steps': a.steps,
           'windows': a.windows, 'final_loss': float(loss.item()),
           'mean_live_fraction': {k: (1.0 if v is None else float(v.float().mean().item()) / T) for k, v in lengths.items() if k in legs},
           'ms_per_step': {leg: {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4),
                                 'windows': [round(t, 4) for t in v]} for leg, v in ms.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
