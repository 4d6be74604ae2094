#!/usr/bin/env python3
"""Host time of a criterion call, alone: microseconds per call on the CPU with the binding's entry points replaced by functions that do
nothing (tests/criterion_rec.py's substitution without the recording), so what is timed is the Python between the target and the Loss.

    tools/criterion_host_time.py [TREE]        # TREE: a checkout of the project (default: this one); prints one JSON line

Compare two trees in alternated fresh processes and take the median of each side ('Host alone')."""
import json
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from icassp2022_depression_amd import models, nn  # noqa: E402

B, HT, HA, CALLS, ROUNDS = 32, 32, 16, 2000, 7


class Owner:
    training = True

    def __init__(self, Cc):
        self._params = {'fc_final.0.weight': type('P', (), {'data': torch.zeros(Cc, HT + HA), 'requires_grad': True, '_grad': None})()}

    def backward(self, dz):
        pass

    def check_health(self):
        pass


def main():
    torch.set_num_threads(1)
    nn._device = lambda: torch.device('cpu')
    for name in ('head_loss', 'head_loss_ce', 'head_loss_reg', 'reduce_loss', 'reduce_loss_by', 'ce_weight_sum', 'row_weight_sum', 'gemm'):
        setattr(nn.L, name, lambda *a, **k: None)
    rng = np.random.default_rng(0)
    y = torch.from_numpy(rng.integers(0, 2, B))
    v = torch.from_numpy(rng.uniform(0, 2, (B, 1)).astype(np.float32))
    w = rng.uniform(0.2, 3.0, B)
    z2, z1 = torch.zeros(B, 2), torch.zeros(B, 1)
    out2, out1 = nn.Output(z2, Owner(2), z2), nn.Output(z1, Owner(1), z1)
    tf, af, model = torch.zeros(B, HT), torch.zeros(B, HA), Owner(2)
    ce, ce_opt, sl1, mse, fusion = (nn.CrossEntropyLoss(), nn.CrossEntropyLoss(weight=[0.5, 2.0], label_smoothing=0.1), nn.SmoothL1Loss(),
                                    nn.MSELoss(), models.MyLoss())
    cases = {'CrossEntropyLoss()': lambda: ce(out2, y), 'CrossEntropyLoss(weight, label_smoothing=0.1)': lambda: ce_opt(out2, y),
             'SmoothL1Loss()': lambda: sl1(out1, v), 'MSELoss() with weight': lambda: mse(out1, v, weight=w),
             'MyLoss()': lambda: fusion(tf, af, y, model)}
    res = {}
    for name, call in cases.items():
        for _ in range(200):
            call()
        best = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            best.append((time.perf_counter() - t0) / CALLS * 1e6)
        res[name] = round(sorted(best)[ROUNDS // 2], 3)                     # median of the rounds of this process
    print(json.dumps({'tree': ROOT, 'us_per_call': res}))


if __name__ == '__main__':
    main()
