#!/usr/bin/env python3
"""The exchange-free LSTM forward (impl = 8, lstm_fwd_local) against the cluster BiLSTM forward (impl = 3, lstm_fwd_cluster) on the same
inputs at the text workload's shape, (B, T, F, H, L, dirs) = (512, 300, 1024, 128, 2, 2), sides alternated in one process:

    sweeps   dep_rnn_forward in DEP_RUN_EVAL and DEP_RUN_DROPOUT_ONLY (p = 0.3): the two sweep launches of a call, timed with HIP
             events around the launches (the library's profile hooks), and the whole call as host wall time around a synchronisation
    fusion   one late-fusion training step of fuse_net_whole.fusion_net (tools/bench_fusion_bi.py's step) with text_impl = 8
             against the default
    train    forward plus backward of the stack in DEP_RUN_TRAIN (p = 0.3, dy and dh_n given, no dX of layer 0: the text model's
             call) on impl = 3 (lstm_fwd_cluster / lstm_bwd_cluster) against impl = 9 (lstm_fwd_save_local / lstm_bwd_local),
             GEMM mode 1: the sweep launches of each pass and the whole pair of calls

    python tools/bench_lstm_local.py [sweeps] [fusion] [train]     (no argument: all three; RUNS=9 alternated rounds after two warm-up
                                                                    calls per side)"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402
from icassp2022_depression_amd import fuse_net_whole as m, nn  # noqa: E402

B, T, Fa, Ft, Ha, Ht, Lyr = 512, 300, 256, 1024, 256, 128, 2
DEV = torch.device('cuda:0')


class Sweep:
    def __init__(self, name, impl, run, p, x, W):
        self.name, self.x, self.W = name, x, W
        self.rnn = L.Rnn(L.CELL_LSTM, B, T, Ft, Ht, Lyr, 2, run, p, L.POOL_NONE, DEV, impl=impl)
        self.h_n = torch.empty(2 * Lyr, B, Ht, device=DEV)
        self.call_ms, self.sweep_ms = [], []

    def call(self):
        self.rnn.forward(self.x, self.W, seed=7, h_n=self.h_n)

    def timed(self):
        torch.cuda.synchronize()
        L.profile_read()
        t0 = time.perf_counter()
        self.call()
        torch.cuda.synchronize()
        self.call_ms.append((time.perf_counter() - t0) * 1e3)
        ms, n = L.profile_read()['lstm_fwd_sweep']
        assert n == Lyr, n
        self.sweep_ms.append(ms)


class Train:
    """One training side: dep_rnn_forward in DEP_RUN_TRAIN and the dep_rnn_backward behind it, on buffers of its own."""

    def __init__(self, name, impl, p, x, W, dy, dh_n):
        self.name, self.x, self.W, self.dy, self.dh_n = name, x, W, dy, dh_n
        self.rnn = L.Rnn(L.CELL_LSTM, B, T, Ft, Ht, Lyr, 2, L.RUN_TRAIN, p, L.POOL_NONE, DEV, impl=impl)
        self.h_n = torch.empty(2 * Lyr, B, Ht, device=DEV)
        self.G = [torch.empty_like(w) for w in W]
        self.call_ms, self.fwd_ms, self.bwd_ms = [], [], []

    def call(self):
        self.rnn.forward(self.x, self.W, seed=7, h_n=self.h_n)
        self.rnn.backward(self.x, self.W, self.G, dy=self.dy, dh_n=self.dh_n, dx=None)

    def timed(self):
        torch.cuda.synchronize()
        L.profile_read()
        t0 = time.perf_counter()
        self.call()
        torch.cuda.synchronize()
        self.call_ms.append((time.perf_counter() - t0) * 1e3)
        prof = L.profile_read()
        (fms, fn), (bms, bn) = prof['lstm_fwd_sweep'], prof['lstm_bwd_sweep']
        assert fn == Lyr and bn == Lyr, (fn, bn)
        self.fwd_ms.append(fms); self.bwd_ms.append(bms)


class Fusion:
    def __init__(self, name, text_impl):
        self.name = name
        c = m.config
        self.model = m.fusion_net(Ft, Ht, c['rnn_layers'], c['dropout'], c['num_classes'], Ha, Fa, seed=0, text_impl=text_impl)
        self.model.train()
        self.opt = nn.Adam(self.model.parameters(), lr=c['learning_rate'])
        self.crit = m.MyLoss()
        g = torch.Generator(device='cpu').manual_seed(1)
        dev = self.model.device
        self.x = (torch.randn(B, T, Fa, generator=g).to(dev), (torch.randn(B, T, Ft, generator=g) * 0.5).to(dev))
        self.y = torch.randint(0, 2, (B,), generator=g).numpy()
        self.times = []

    def step(self):
        self.opt.zero_grad()
        tf, af = self.model.pretrained_feature(self.x)
        self.model(torch.cat((tf, af), dim=1))
        self.crit(tf, af, self.y, self.model).backward()
        self.opt.step()


def line(name, t):
    return f'{name:22s} median {statistics.median(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  (max - min {max(t) - min(t):.3f})'


def train_section(runs, x, W):
    g = torch.Generator(device='cpu').manual_seed(3)
    dy = (torch.randn(B, T, 2 * Ht, generator=g) * 0.1).to(DEV)
    dh_n = (torch.randn(2 * Lyr, B, Ht, generator=g) * 0.1).to(DEV)
    mode = L.get_gemm_mode()
    L.set_gemm_mode(1, 1 << 28)
    L.profile_enable(True)
    sides = [Train('impl 3 (cluster)', L.IMPL_CLUSTER, 0.3, x, W, dy, dh_n), Train('impl 9 (local)', L.IMPL_LOCAL_LSTM_TRAIN, 0.3, x, W, dy, dh_n)]
    for s in sides:
        s.call(); s.call()
        s.rnn.check()
    rel = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(sides[1].G, sides[0].G))
    for r in range(runs):
        for s in sides:
            s.timed()
    print(f'LSTM training forward + backward at (B, T, F, H, L, dirs) = {(B, T, Ft, Ht, Lyr, 2)}, p = 0.3, {runs} alternated rounds, GEMM mode 1')
    for s in sides:
        s.rnn.check()
        print('train        ' + line(s.name + ' fwd sweeps', s.fwd_ms))
        print('train        ' + line(s.name + ' bwd sweeps', s.bwd_ms))
        print('train        ' + line(s.name + ' fwd + bwd', s.call_ms))
    print(f'train        weight gradients, impl 9 against impl 3: worst max |diff| / max |.| {rel:.3g}')
    L.profile_enable(False)
    L.profile_read()
    L.set_gemm_mode(mode, 1 << 28)


def sweeps_section(runs, x, W):
    print(f'LSTM forward at (B, T, F, H, L, dirs) = {(B, T, Ft, Ht, Lyr, 2)}, {runs} alternated rounds, GEMM mode {L.get_gemm_mode()}')
    L.profile_enable(True)
    for mode, run, p in (('eval', L.RUN_EVAL, 0.0), ('dropout-only', L.RUN_DROPOUT_ONLY, 0.3)):
        sides = [Sweep('impl 3 (cluster)', L.IMPL_CLUSTER, run, p, x, W), Sweep('impl 8 (local)', L.IMPL_LOCAL_LSTM, run, p, x, W)]
        for s in sides:
            s.call(); s.call()
            s.rnn.check()
        d = (sides[0].rnn.layer_output() - sides[1].rnn.layer_output()).abs().max().item()
        for r in range(runs):
            for s in sides:
                s.timed()
        for s in sides:
            s.rnn.check()
            print(f'{mode:13s}' + line(s.name + ' sweeps', s.sweep_ms))
            print(f'{mode:13s}' + line(s.name + ' call', s.call_ms))
        print(f'{mode:13s}top layer output, impl 8 against impl 3: max |diff| {d:.3g}')
        del sides
    L.profile_enable(False)
    L.profile_read()


def fusion_section(runs):
    sides = [Fusion('default', None), Fusion('text_impl 8', 8)]
    for s in sides:
        s.step(); s.step()
        torch.cuda.synchronize()
        s.model.check_health()
    for r in range(runs):
        for s in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.step()
            torch.cuda.synchronize()
            s.times.append((time.perf_counter() - t0) * 1e3)
    print(f'late-fusion train step (dropout {m.config["dropout"]}, Adam, MyLoss) at (B, T, Fa, Ft, Ha, Ht) = {(B, T, Fa, Ft, Ha, Ht)}')
    for s in sides:
        s.model.check_health()
        print(line('fusion ' + s.name, s.times))


def main():
    runs = int(os.environ.get('RUNS', 9))
    want = [a for a in sys.argv[1:] if a in ('sweeps', 'fusion', 'train')] or ['sweeps', 'fusion', 'train']
    g = torch.Generator(device='cpu').manual_seed(2)
    x = (torch.randn(B, T, Ft, generator=g) * 0.5).to(DEV)
    k = 1.0 / Ht ** 0.5
    W = []
    for l in range(Lyr):
        for _ in range(2):
            for shp in ((4 * Ht, Ft if l == 0 else 2 * Ht), (4 * Ht, Ht), (4 * Ht,), (4 * Ht,)):
                W.append(((torch.rand(*shp, generator=g) * 2 - 1) * k).to(DEV))
    if 'sweeps' in want:
        sweeps_section(runs, x, W)
    if 'fusion' in want:
        fusion_section(runs)
    if 'train' in want:
        train_section(runs, x, W)


if __name__ == '__main__':
    main()
