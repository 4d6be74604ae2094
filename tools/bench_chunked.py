#!/usr/bin/env python3
"""The chunked exact training step against the whole-call step: AudioGRU 'clf' in train mode, forward + loss + backward,
timed three ways in one process, alternated:

    whole      model(x) on the (B, T, F) batch: one reserve for all T steps
    chunked5   model.forward_chunked(x, chunk, impl=5): the per-layer cluster sweeps, state through training (where that impl exists)
    chunked2   model.forward_chunked(x, chunk, impl=2): the same step on the per-layer tile-MFMA sweeps

    python tools/bench_chunked.py [B T F H chunk]        (default 64 3000 256 256 300; RUNS=9 rounds, each one timing of every side)

One line per round, then per side the median, min and max over the rounds, the device memory a step of each side adds, and the
criterion of DESIGN 4.14 for forward_chunked's default: chunked5's median is below chunked2's by more than chunked2's own max - min.
The distance to the whole-call step (the recompute, the launch chains of the chunks, the fp32-row contractions) is reported, not judged.
Host wall time around a device synchronisation (a chunked step is many small launches: their enqueue cost is part of what a caller pays)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402
from icassp2022_depression_amd import audio_gru_whole, nn  # noqa: E402


def main():
    B, T, F, H, chunk = map(int, sys.argv[1:6]) if len(sys.argv) > 5 else (64, 3000, 256, 256, 300)
    runs = int(os.environ.get('RUNS', 9))
    cfg = dict(audio_gru_whole.config); cfg.update(embedding_size=F, hidden_dims=H)
    model = audio_gru_whole.AudioBiLSTM(cfg, seed=0)
    model.train()
    crit = nn.CrossEntropyLoss()
    dev = model.device
    torch.manual_seed(0)
    x = torch.randn(B, T, F, device=dev)
    y = torch.randint(0, 2, (B,)).numpy()

    def step(impl):
        out = model(x) if impl is None else model.forward_chunked(x, chunk, impl=impl)
        crit(out, y).backward()

    sides = [('whole', None)]
    probe = L.RnnDesc(L.CELL_GRU, 1, 1, F, H, cfg['rnn_layers'], 1, L.RUN_TRAIN, 0.0, 0, L.POOL_SUM, L.IMPL_CLUSTER_PER_LAYER_STATE)
    if L.load().dep_rnn_workspace_bytes(probe) != 0:
        sides.append(('chunked5', L.IMPL_CLUSTER_PER_LAYER_STATE))
    sides.append(('chunked2', L.IMPL_TILE))
    times = {n: [] for n, _ in sides}
    peak = {}
    for n, impl in sides:                                # warm-up: descriptors, buffers, code objects; the side's own peak memory
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()             # (the other sides' cached descriptors stay allocated: not this side's)
        torch.cuda.reset_peak_memory_stats()
        step(impl); step(impl)
        torch.cuda.synchronize()
        peak[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for r in range(runs):
        for n, impl in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(impl)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3)
        model.check_health()
        print(f'round {r}: ' + '  '.join(f'{n} {times[n][-1]:.3f} ms' for n, _ in sides), flush=True)
    print(f"AudioGRU 'clf' train step (dropout {cfg['dropout']}), B={B} T={T} F={F} H={H}, {(T + chunk - 1) // chunk} chunks of {chunk}; "
          f'{runs} alternated rounds')
    for n, _ in sides:
        t = times[n]
        print(f'{n:9s} median {statistics.median(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  (max - min {max(t) - min(t):.3f});  '
              f'device memory of the step above the batch and the weights {peak[n]:.0f} MiB')
    mw = statistics.median(times['whole'])
    for n in ('chunked5', 'chunked2'):
        if n in times:
            print(f'{n} / whole = {statistics.median(times[n]) / mw:.2f}x (reported, not judged)')
    if 'chunked5' in times:
        m2, m5 = statistics.median(times['chunked2']), statistics.median(times['chunked5'])
        bar = max(times['chunked2']) - min(times['chunked2'])
        print(f'criterion: chunked2 median - chunked5 median = {m2 - m5:.3f} ms against a bar of {bar:.3f} ms (chunked2 max - min): '
              f'{"MET" if m2 - m5 > bar else "NOT MET"};  chunked2 / chunked5 = {m2 / m5:.2f}x')


if __name__ == '__main__':
    main()
