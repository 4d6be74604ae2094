"""The fp64 yardstick of the value clamp, the per-group norms and the landed step count (test_clip2_cpu.py pins it against torch;
test_clip2_gpu.py holds the kernels to it), beside clip_ref.py, plus the recording stand-in of the binding's new entry points.

Order, as torch's loop has it: clip_grad_norm_ (per group or over all tensors) -> clip_grad_value_ -> step().  The coefficient is
clip_ref.clip_coef (ONE rounding to fp32), the product g * coef is rounded to fp32, the clamp acts on that fp32 value, and
oracle.ref_numpy.adam_step takes it from there.  With count_skipped=False the step number of the bias correction is the number of
updates that landed, this one included; a skipped step changes nothing at all."""
import numpy as np

from clip_ref import clip_coef, sqnorm
from oracle import ref_numpy as R
import optim_rec

F32 = np.float32


def clamp(x, c):
    """Tensor.clamp_(-c, c) on float32 values, by comparisons: NaN stays NaN, +-inf becomes +-c, -0.0 stays -0.0."""
    x = np.asarray(x, F32).copy()
    c = F32(c)
    x[x > c] = c
    x[x < -c] = -c
    return x


def clamped_gradient(g, coef, max_value):
    """fp32(g * coef), clamped: what the update launch hands to the Adam expression, as float64."""
    with np.errstate(all='ignore'):
        gc = np.asarray(g, F32) * F32(coef)
    if max_value is not None:
        gc = clamp(gc, max_value)
    return gc.astype(np.float64)


def run(P, G, groups=None, bounds=(None,), max_value=None, skip_nonfinite=False, count_skipped=True, lr=1e-4, wds=None, decoupled=False,
        M=None, V=None, step0=0, landed0=0):
    """P: list of parameter arrays.  G: per step, the list of their gradients.  groups: lists of tensor indices (default: one group of
    all); bounds[k]: group k's max_norm or None (measured only); wds[k]: its weight decay.  Steps are numbered step0 + 1, ...
    Returns {'P', 'M', 'V', 'landed', 'skipped', 'steps': [{'norms', 'coefs', 'norm', 'coef', 'skipped', 't'}, ...]}."""
    groups = [list(range(len(P)))] if groups is None else groups
    wds = [0.0] * len(groups) if wds is None else wds
    P = [np.asarray(p, np.float64).copy() for p in P]
    M = [np.zeros_like(p) for p in P] if M is None else [np.asarray(a, np.float64).copy() for a in M]
    V = [np.zeros_like(p) for p in P] if V is None else [np.asarray(a, np.float64).copy() for a in V]
    landed, skipped_n, recs = landed0, 0, []
    for k, gs in enumerate(G, step0 + 1):
        S = [sqnorm([gs[i] for i in idx]) for idx in groups]
        coefs = [clip_coef(s, 0.0 if b is None else b) for s, b in zip(S, bounds)]
        skipped = skip_nonfinite and not all(np.isfinite(s) for s in S)
        t = k if count_skipped else landed + (0 if skipped else 1)
        with np.errstate(all='ignore'):
            recs.append({'norms': [float(np.sqrt(s)) for s in S], 'coefs': [float(c) for c in coefs], 'norm': float(np.sqrt(np.sum(S))),
                         'coef': float(np.min(coefs)) if not np.any(np.isnan(coefs)) else float('nan'), 'skipped': skipped, 't': t})
        if skipped:
            skipped_n += 1
            continue
        landed += 1
        for idx, c, wd in zip(groups, coefs, wds):
            for i in idx:
                with np.errstate(all='ignore'):
                    P[i], M[i], V[i] = R.adam_step(P[i], clamped_gradient(gs[i], c, max_value), M[i], V[i], t, lr, wd=wd, decoupled=decoupled)
    return {'P': P, 'M': M, 'V': V, 'landed': landed, 'skipped': skipped_n, 'steps': recs}


# ------------------------------------------------------------------------------------------------ recording stand-in
def record_binding2(monkeypatch, adam_logs_p=False):
    """optim_rec.record_binding plus the entry points it does not know: nn.L.adam_step_opt appends ('opt', span(p), span(g), kw) with
    kw = every other argument by name (positional hyper-parameters under 'lr', 'b1', ...), nn.L.adam_step_ext ('ext', span(p), span(g), kw)
    and nn.L.grad_clip_value ('value', [span...], clip_value)."""
    nn, log, names = optim_rec.record_binding(monkeypatch, adam_logs_p)
    sqnorm_rec = nn.L.grad_sqnorm                       # the stand-in just installed: a list comprehension over span()

    def span_of(t):
        """record_binding's span of a tensor (its class is local to that function): let its sqnorm stand-in make one and take it back."""
        sqnorm_rec([t], None)
        return log.pop()[1][0]

    def updater(kind):
        def f(p, g, m, v, lr, b1, b2, eps, wd, decoupled, step, **kw):
            kw.update(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, decoupled=decoupled, step=step)
            log.append((kind, span_of(p), span_of(g), kw))
        return f

    monkeypatch.setattr(nn.L, 'adam_step_opt', updater('opt'))
    monkeypatch.setattr(nn.L, 'adam_step_ext', updater('ext'))
    monkeypatch.setattr(nn.L, 'grad_clip_value', lambda ranges, c: log.append(('value', [span_of(t) for t in ranges], c)))
    return nn, log, names
