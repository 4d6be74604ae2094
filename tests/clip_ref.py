"""The fp64 yardstick of the gradient-clipping tests (test_clip_cpu.py pins it against torch; test_clip_gpu.py holds the kernels to it):
S = sum of g^2 over ALL tensors, torch's clip coefficient with ONE rounding to fp32, then oracle.ref_numpy.adam_step on g * coef."""
import numpy as np

from oracle import ref_numpy as R


def sqnorm(gs):
    """Sum of squares of a list of arrays, in float64 (every product of two fp32 values is exact there)."""
    return float(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in gs))


def clip_coef(S, max_norm):
    """(float32) min(1, max_norm / (sqrt(S) + 1e-6)); a NaN quotient stays NaN as in torch.clamp; max_norm <= 0 or inf: 1 (measure only)."""
    if not (max_norm > 0.0) or np.isinf(max_norm):
        return np.float32(1.0)
    with np.errstate(all='ignore'):
        q = np.float64(max_norm) / (np.sqrt(np.float64(S)) + 1e-6)
    return np.float32(1.0 if q > 1.0 else q)


def clipped_adam_step(p, g, m, v, step, lr, coef, wd=0.0, decoupled=False):
    """One tensor: adam_step on g * coef, the product rounded to fp32 as the kernel (and torch's in-place mul_ on .grad) rounds it."""
    with np.errstate(all='ignore'):
        gc = (np.asarray(g, np.float32) * np.float32(coef)).astype(np.float64)
        return R.adam_step(np.asarray(p, np.float64), gc, m, v, step, lr, wd=wd, decoupled=decoupled)


def clipped_adam_steps(P, G, max_norm, lr, wd=0.0, decoupled=False):
    """P: list of parameter arrays; G: per step, the list of their gradients.  Returns (parameters after the steps, coefficients, norms)."""
    P = [np.asarray(p, np.float64) for p in P]
    M = [np.zeros_like(p) for p in P]
    V = [np.zeros_like(p) for p in P]
    coefs, norms = [], []
    for step, gs in enumerate(G, 1):
        S = sqnorm(gs)
        c = clip_coef(S, max_norm)
        coefs.append(float(c)); norms.append(float(np.sqrt(S)))
        for i, g in enumerate(gs):
            P[i], M[i], V[i] = clipped_adam_step(P[i], g, M[i], V[i], step, lr, c, wd=wd, decoupled=decoupled)
    return P, coefs, norms
