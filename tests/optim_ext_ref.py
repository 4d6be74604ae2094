"""The float64 yardstick of the AMSGrad / averaged-weights tests (test_optim_ext_cpu.py pins it against torch.optim.Adam[W](amsgrad=True)
and torch.optim.swa_utils.AveragedModel; test_optim_ext_gpu.py holds dep_adam_step_ext to it), the gradient sequence both use, and the
tolerances of the device comparison with their derivation."""
import numpy as np

from clip_ref import clip_coef, sqnorm

F32 = np.float32
LR, B1, B2, EPS = (float(F32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))        # as the kernel receives them
STEPS = 20

# Device against float64 over STEPS steps, parameters inside (-0.5, 0.5) (the tests assert it), hyper-parameters rounded to float32 on
# both sides.  u = 2**-24 is the relative error of one float32 rounding; a value below 0.5 rounds within 2**-26 absolutely.
#   m: fmac(b1 * m + (1 - b1) * g) after one product, and the clipped form's g * coef: at most 3 roundings per step, relative to the
#      largest |m|, each damped by b1 per later step: 3 u (1 - b1^20) / (1 - b1) = 1.6e-6.
#   v, vmax: two products, one sum, and the clipped g entering squared: 5 u per step, damped by b2: 5 u (1 - b2^20) / (1 - b2) = 5.9e-6
#      relative to the largest v.  A maximum of values inside a bound is inside it.
#   p: |m_hat| / sqrt(v_hat) <= (1 - b1) / sqrt(1 - b2) = 3.2, and AMSGrad only enlarges the root, so p moves at most 3.2 lr per step
#      and stays below 0.4 + 20 * 3.2e-3 < 0.5.  Per step: two roundings of p (the decoupled decay, the update) of 2**-26 each, plus the
#      update term's own relative error (m's, half of v's, the root, the division: below 6e-6) times its size 3.2 lr: 2e-8.
#      20 * (3e-8 + 2e-8) = 1e-6, the bound adam_run of test_small_kernels_gpu.py holds the plain step to.
#   average: a convex combination of the parameters so far, so it inherits at most their error, plus per update the rounding of
#      p - ema (u times at most 0.07, the distance p can have moved) and of the fma's result (2**-26): 1e-6 + 20 * 1.9e-8 = 1.4e-6.
U = 2.0 ** -24
M_TOL = 3 * U * (1 - B1 ** STEPS) / (1 - B1)
V_TOL = 5 * U * (1 - B2 ** STEPS) / (1 - B2)
P_TOL = 1e-6
EMA_TOL = P_TOL + STEPS * (2.0 ** -26 + U * 0.07)


def r32(a):
    """float64 holding float32 values: what the kernel is given."""
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def shrinking_gradients(n, steps, seed):
    """Standard-normal gradients, a hundred times smaller after step 5: v decays from then on, so that the running maximum is
    above v somewhere (the case in which AMSGrad differs from Adam)."""
    rng = np.random.default_rng(seed)
    return [r32(rng.standard_normal(n) * (1.0 if k < 5 else 0.01)) for k in range(steps)]


def growing_gradients(n, steps, seed):
    """|g| grows by 1.5x per step: v never decreases, so AMSGrad is Adam."""
    rng = np.random.default_rng(seed)
    return [r32(rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 1.2, n) * 1.5 ** k) for k in range(steps)]


def new_state(p, amsgrad, ema):
    p = np.asarray(p, np.float64)
    return {'p': p.copy(), 'm': np.zeros_like(p), 'v': np.zeros_like(p), 'vmax': np.zeros_like(p) if amsgrad else None,
            'ema': np.full_like(p, np.nan) if ema else None}


def step(st, g, k, lr=LR, wd=0.0, decoupled=False, b1=B1, b2=B2, eps=EPS, ema_decay=None, ema_first=False, coef=None):
    """One update of step count k (1-based) in place on st = {p, m, v, vmax | None, ema | None} (new_state): torch's single-tensor
    Adam / AdamW, with vmax = max(vmax, v) under the root when st['vmax'] is there, then ema += (1 - d) * (p_new - ema) -- or
    ema = p_new on the first update -- when st['ema'] is.  coef: the clip coefficient, applied to g with one float32 rounding."""
    g = np.asarray(g, np.float64)
    if coef is not None:
        g = (g.astype(F32) * F32(coef)).astype(np.float64)
    p = st['p']
    if decoupled:
        p = p * (1.0 - lr * wd)
    elif wd != 0.0:
        g = g + wd * p
    st['m'] = b1 * st['m'] + (1 - b1) * g
    st['v'] = b2 * st['v'] + (1 - b2) * g * g
    root = st['v']
    if st['vmax'] is not None:
        st['vmax'] = root = np.maximum(st['vmax'], st['v'])
    denom = np.sqrt(root) / np.sqrt(1 - b2 ** k) + eps
    st['p'] = p - (lr / (1 - b1 ** k)) * st['m'] / denom
    if st['ema'] is not None:
        st['ema'] = st['p'].copy() if ema_first else st['ema'] + (1.0 - ema_decay) * (st['p'] - st['ema'])
    return st


def run(p, grads, amsgrad, ema_decay, wd=0.0, decoupled=False, max_norm=None, first_step=1):
    """The whole sequence; max_norm: every step clipped by the global norm of its own gradient.  Returns (state, [state after each step])."""
    st = new_state(p, amsgrad, ema_decay is not None)
    trail = []
    for i, g in enumerate(grads):
        coef = None if max_norm is None else clip_coef(sqnorm([g]), max_norm)
        step(st, g, first_step + i, wd=wd, decoupled=decoupled, ema_decay=ema_decay, ema_first=i == 0, coef=coef)
        trail.append({k: None if a is None else a.copy() for k, a in st.items()})
    return st, trail


def ema_recurrence(ps, d):
    """The average of the iterates ps[0], ps[1], ... (float64): ps[0], then avg += (1 - d) * (p - avg)."""
    avg = np.asarray(ps[0], np.float64).copy()
    for p in ps[1:]:
        avg = avg + (1.0 - d) * (np.asarray(p, np.float64) - avg)
    return avg
