"""What gradient accumulation costs per optimizer update, and what it saves in memory: a same-session comparison on bench.py's workload.

    python tools/bench_accum.py [--workload audio_gru] [--configs 512x1,256x2,128x4] [--updates 30] [--warmup 6] [--rounds 6] [--out FILE]

Every configuration `b x K` is the SAME effective batch (b * K rows of one synthetic batch, bench.WORKLOADS' shape) stepped as K
micro-batches of b rows through a model and an nn.AdamW(accumulate_steps=K) of its own: per micro-batch zero_grad, forward, criterion
(dividing by the declared b * K rows), backward, optimizer.step(); the K-th step updates.  b x 1 is the plain train step bench.py times.
The configurations run in alternation in one process, `rounds` runs each of `updates` updates, the order rotated from round to round so
that none always runs first; wall time between two device synchronisations.  Prints one JSON line: per configuration the ms per UPDATE
of every run, the median and the range (max - min), the reserve + workspace bytes of its recurrent stack (one micro-batch's: all that
is alive at a time) and the accumulator's bytes.
"""
import argparse
import importlib
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
    ap.add_argument('--configs', default='512x1,256x2,128x4', help='comma-separated micro-batch x accumulate_steps')
    ap.add_argument('--updates', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--max-grad-norm', type=float, default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    spec = importlib.util.spec_from_file_location('dep_bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from icassp2022_depression_amd import nn, parallel
    modname, cls, _, T, F, H = bench.WORKLOADS[a.workload]
    if a.workload == 'fusion':
        raise SystemExit('bench_accum: the encoder workloads only (the fusion step trains 768 floats)')
    mod = importlib.import_module('icassp2022_depression_amd.' + modname)
    dev = torch.device('cuda:0')
    configs = [tuple(int(v) for v in c.split('x')) for c in a.configs.split(',')]
    rows = max(b * k for b, k in configs)
    g = torch.Generator(device='cpu'); g.manual_seed(1234)
    y = torch.randint(0, 2, (rows,), generator=g).to(dev)
    x = torch.randn(rows, T, F, generator=g).to(dev)                         # synthetic features, resident in HBM
    crit = nn.CrossEntropyLoss()

    def build(b, k):
        cfg = dict(mod.config); cfg.update(embedding_size=F, hidden_dims=H)
        torch.manual_seed(0)
        model = getattr(mod, cls)(cfg, seed=0)
        model.train()
        kw = {} if k == 1 else {'accumulate_steps': k}                       # b x 1 builds the optimizer exactly as bench.py does
        opt = nn.AdamW(mod.get_param_group(model), lr=cfg['learning_rate'], max_grad_norm=a.max_grad_norm, **kw)

        def update():
            parallel.set_accumulated_count(b * k if k > 1 else None)
            for i in range(k):
                opt.zero_grad()
                loss = crit(model(x[i * b:(i + 1) * b]), y[i * b:(i + 1) * b])
                loss.backward()
                opt.step()
            return loss
        return model, opt, update

    sides = {c: build(*c) for c in configs}

    def run(c, n):
        update = sides[c][2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            update()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for c in configs:
        run(c, a.warmup)
    ms = {c: [] for c in configs}
    for r in range(a.rounds):
        order = configs[r % len(configs):] + configs[:r % len(configs)]      # no configuration always runs first
        for c in order:
            ms[c].append(run(c, a.updates))
    parallel.set_accumulated_count(None)
    res = {'workload': a.workload, 'shape': [T, F, H], 'updates': a.updates, 'rounds': a.rounds, 'max_grad_norm': a.max_grad_norm, 'configs': []}
    for c in configs:
        model, opt, _ = sides[c]
        model.check_health()
        rnns = [r for r in model._rnns.cache.values() if r.desc.training]
        res['configs'].append({
            'micro_batch': c[0], 'accumulate_steps': c[1], 'ms_per_update': [round(v, 4) for v in ms[c]],
            'median_ms': round(statistics.median(ms[c]), 4), 'range_ms': round(max(ms[c]) - min(ms[c]), 4),
            'reserve_bytes': sum(r.reserve.numel() * 4 for r in rnns), 'workspace_bytes': sum(r.workspace.numel() * 4 for r in rnns),
            'accumulator_bytes': sum(t.numel() * 4 for t in opt._accum.values()), 'optimizer_updates': opt._step})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
