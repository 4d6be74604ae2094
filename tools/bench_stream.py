#!/usr/bin/env python3
"""Chunked scoring against the whole call: AudioGRU 'clf' in eval mode, timed three ways in one session, alternated:

    whole     model(x) on the (B, T, F) batch
    stream2   model.stream(impl=2): T / chunk pushes on the per-layer tile-MFMA sweeps, then output()
    stream4   model.stream(impl=4): the same pushes on the per-layer cluster sweeps (descriptors where that impl exists)

    python tools/bench_stream.py [B T F H chunk]        (default 64 3000 256 256 300; RUNS=7 rounds, each one timing of every side)

One line per round, then per side the median, min and max over the rounds, and the criterion of DESIGN 4.14: stream4's median is below
stream2's by more than stream2's own max - min.  Host wall time around a device synchronisation (a stream is many small launches: their
enqueue cost is part of what a caller pays)."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402
from icassp2022_depression_amd import audio_gru_whole  # noqa: E402


def main():
    B, T, F, H, chunk = map(int, sys.argv[1:6]) if len(sys.argv) > 5 else (64, 3000, 256, 256, 300)
    runs = int(os.environ.get('RUNS', 7))
    cfg = dict(audio_gru_whole.config); cfg.update(embedding_size=F, hidden_dims=H, dropout=0.0)
    model = audio_gru_whole.AudioBiLSTM(cfg, seed=0)
    model.eval()
    dev = model.device
    torch.manual_seed(0)
    x = torch.randn(B, T, F, device=dev)
    chunks = [x[:, t0:t0 + chunk].contiguous() for t0 in range(0, T, chunk)]
    outs = {}

    def whole():
        outs['whole'] = model(x)

    def stream(impl):
        s = model.stream(impl=impl)
        for c in chunks:
            s.push(c)
        outs[f'stream{impl}'] = s.output()
        return s

    sides = [('whole', whole), ('stream2', lambda: stream(L.IMPL_TILE))]
    probe = L.RnnDesc(L.CELL_GRU, 1, 1, F, H, cfg['rnn_layers'], 1, L.RUN_EVAL, 0.0, 0, L.POOL_SUM, L.IMPL_CLUSTER_PER_LAYER)
    if L.load().dep_rnn_workspace_bytes(probe) != 0:
        sides.append(('stream4', lambda: stream(L.IMPL_CLUSTER_PER_LAYER)))
    times = {n: [] for n, _ in sides}
    for n, f in sides:                                   # warm-up: descriptors, buffers, code objects
        f(); f()
    torch.cuda.synchronize()
    for r in range(runs):
        for n, f in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = f()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3)
            if s is not None:
                s.check_health()
        print(f'round {r}: ' + '  '.join(f'{n} {times[n][-1]:.3f} ms' for n, _ in sides), flush=True)
    model.check_health()
    ref = outs['whole'].data
    print(f"AudioGRU 'clf' eval, B={B} T={T} F={F} H={H}, {len(chunks)} chunks of {chunk}; {runs} alternated rounds")
    for n, _ in sides:
        t = times[n]
        dz = float((outs[n].data - ref).abs().max())
        print(f'{n:8s} median {statistics.median(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  (max - min {max(t) - min(t):.3f});  |out - whole| {dz:.2e}')
    if 'stream4' in times:
        m2, m4 = statistics.median(times['stream2']), statistics.median(times['stream4'])
        bar = max(times['stream2']) - min(times['stream2'])
        print(f'criterion: stream2 median - stream4 median = {m2 - m4:.3f} ms against a bar of {bar:.3f} ms (stream2 max - min): '
              f'{"MET" if m2 - m4 > bar else "NOT MET"};  stream2 / stream4 = {m2 / m4:.2f}x')


if __name__ == '__main__':
    main()
