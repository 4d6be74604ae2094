#!/usr/bin/env python3
"""One late-fusion training step with the unidirectional and with the bidirectional audio encoder on synthetic pairs:
pretrained_feature (frozen encoders, dropout active) -> cat -> head -> MyLoss -> backward -> Adam step of fuse_net_whole.fusion_net in train
mode, at the cfg4 shapes (B, T, Fa, Ft, Ha, Ht) = (512, 300, 256, 1024, 256, 128), two sides alternated in one process:

    uni      audio_bidirectional = False      the bench.py fusion step
    bi       audio_bidirectional = True       BiGRU on the impl = 7 sweeps + attention in place of GRU + SUM pool

    python tools/bench_fusion_bi.py          (RUNS=9 alternated rounds after two warm-up steps per side)

Step times are host wall time around a device synchronisation."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402
from icassp2022_depression_amd import fuse_net_whole as m, nn  # noqa: E402

B, T, Fa, Ft, Ha, Ht = 512, 300, 256, 1024, 256, 128


class Side:
    def __init__(self, name, bi):
        self.name = name
        c = m.config
        self.model = m.fusion_net(Ft, Ht, c['rnn_layers'], c['dropout'], c['num_classes'], Ha, Fa, seed=0, audio_bidirectional=bi)
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


def main():
    runs = int(os.environ.get('RUNS', 9))
    sides = [Side('uni', False), Side('bi', True)]
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
        print(f'round {r}: ' + '  '.join(f'{s.name} {s.times[-1]:.3f} ms' for s in sides), flush=True)
    print(f'late-fusion train step (dropout {m.config["dropout"]}, Adam, MyLoss) at (B, T, Fa, Ft, Ha, Ht) = {(B, T, Fa, Ft, Ha, Ht)}, {runs} alternated rounds; '
          f'GEMM mode {L.get_gemm_mode()}')
    for s in sides:
        t = s.times
        s.model.check_health()
        print(f'{s.name:4s} median {statistics.median(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  (max - min {max(t) - min(t):.3f})')


if __name__ == '__main__':
    main()
