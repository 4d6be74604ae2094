"""How often the device's bias factors (count_skipped=False: beta^t by squaring) differ from the host's (pow).

    python tools/bias_steps.py [--out FILE]

One element, betas (0.9, 0.999), steps 1..4096 with no step skipped: dep_adam_step_opt with the landed count against
dep_adam_step_clipped with the host's step number, once with the state copied from the counted side before every step (`same_state`:
a difference is that step's factors alone) and once free-running.  Prints one JSON line: the number of steps at which p differs in
any bit, the largest difference in fp32 ulps, the first such step, and the two landed words at the end."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
from icassp2022_depression_amd import _lib as L
DEV = torch.device('cuda:0')
rng = np.random.default_rng(0)
N = 4096
G = (0.05 * rng.standard_normal(N)).astype(np.float32)
def fresh():
    return [torch.tensor([0.3], device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)]
part = torch.empty(L.grad_norm_slots(), dtype=torch.float64, device=DEV)
landed = torch.zeros(2, dtype=torch.int32, device=DEV)
res = {}
for mode in ('same_state', 'free_running'):
    a, b = fresh(), fresh()
    landed.zero_()
    pa, pb = [], []
    for k in range(1, N + 1):
        g = torch.tensor([G[k - 1]], device=DEV)
        L.grad_sqnorm([g], part)
        if mode == 'same_state':
            for x, y in zip(a, b):
                y.copy_(x)
        L.adam_step_clipped(a[0], g, a[1], a[2], 1e-3, 0.9, 0.999, 1e-8, 1e-2, True, k, part, 0.0, True)
        at = (k - 1) & 1
        L.adam_step_opt(b[0], g, b[1], b[2], 1e-3, 0.9, 0.999, 1e-8, 1e-2, True, k, partials=part, max_norm=0.0, skip_nonfinite=True,
                        landed_in=landed[at:at + 1], landed_out=landed[1 - at:2 - at])
        pa.append(a[0].clone()); pb.append(b[0].clone())
    torch.cuda.synchronize()
    ia = torch.cat(pa).view(torch.int32).cpu().numpy().astype(np.int64)
    ib = torch.cat(pb).view(torch.int32).cpu().numpy().astype(np.int64)
    d = np.abs(ia - ib)
    res[mode] = {'steps_differing': int((d > 0).sum()), 'max_ulps': int(d.max()), 'first': int(np.flatnonzero(d)[0] + 1) if d.any() else None,
                 'landed': landed.tolist()}
print(json.dumps(res))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, 'w').write(json.dumps(res) + '\n')
