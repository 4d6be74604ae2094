"""Cases, seeded inputs and references of the switch-selected sweep instances (tests/test_switch_forms_gpu.py).

The rows of the cluster families' instance tables that only an environment switch selects can be launched by no in-process test: the
switches are read once per process.  tests/switch_probe.py runs the case lists below in one child process per environment; the parent
builds the SAME arrays from `inputs()` and compares with the float64 oracle (oracle/ref_numpy.py, tests/varlen_ref.py).  numpy only:
the CPU test of this module (tests/test_switch_cases_cpu.py) runs without a GPU.

A case is a dict: name, cell ('gru' | 'lstm'), B, T, F, H, impl, form, p (inter-layer dropout), ragged, dx, mode (dep_set_gemm_mode),
regime.
  GRU  'full' : dy + dpooled in, dx out (mean pool);  'model': dpooled only, no dx -- what the training step passes
  LSTM        : dy + dh_n in, dx as the case says

regime: where the gates sit (apply_regime below).  'init' is what every other parity test of the suite draws -- weights and biases uniform
in +-1/sqrt(H), x standard normal: every gate near 0.5.  The others move the SAME draw to where trained networks live and where the fast
gate functions (fast_sigmoid / fast_tanh, csrc/rnn_cluster_common.h) and the 16-bit saved gates behave differently:
  'memory'  +4 on the z block of bias_ih (GRU) | the f block (LSTM), every layer and direction: update / forget gates near 0.98
  'reset'   -4 on the r block of bias_ih (GRU only): a closed reset gate
  'sat'     every weight_* times 4: saturated candidates and cell values
  'drive'   x times 10
"""
import numpy as np

from oracle import ref_numpy as R
from varlen_ref import bilstm_ragged, gru_ragged, lengths_mix

LAYERS = 2
DROP_SEED = 1234            # desc.seed of every case; the inter-layer mask is dep_dropout_mask(.., DROP_SEED, site 16)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


REGIMES = ('init', 'memory', 'reset', 'sat', 'drive')
MEMORY_BIAS = 4.0           # sigmoid(4) = 0.982
RESET_BIAS = -4.0
SAT_SCALE = 4.0
DRIVE_SCALE = 10.0


def _case(cell, B, T, F, H, impl=3, form='full', p=0.0, ragged=False, dx=True, mode=1, regime='init'):
    assert regime in REGIMES and not (regime == 'reset' and cell != 'gru')
    c = dict(cell=cell, B=B, T=T, F=F, H=H, impl=impl, form=form, p=p, ragged=ragged, dx=dx and form == 'full', mode=mode, regime=regime)
    c['name'] = '%s-B%d-T%d-F%d-H%d-i%d-%s-p%g-%s-%s-m%d' % (cell, B, T, F, H, impl, form, p, 'ragged' if ragged else 'dense',
                                                             'dx' if c['dx'] else 'nodx', mode)
    if regime != 'init':                            # the names of the init cases stay: the cached results and TRACE_EXTRA go by them
        c['name'] += '-' + regime
    return c


# ---- DEP_SV16=0: the per-layer GRU sweeps.  B = 37: three tiles, the last ragged, padded to 8; T = 5: burst + 1; T = 6: whole step
# pairs (gate gradients as fp32 rows at either: the contractions of shapes this small run gemm_small, see GRU_FUSED_PK).  Dense and ragged.
GRU_LAYER = [_case('gru', 37, T, 8, H, ragged=r) for H in (64, 128, 512) for T in (5, 6) for r in (False, True)]
# ... H = 256 on the per-layer sweeps: a ragged call (the fused launches take no lengths) and impl = 4
GRU_LAYER_256 = [_case('gru', 33, 4, 16, 256, ragged=True), _case('gru', 20, 3, 8, 256, ragged=True), _case('gru', 33, 4, 16, 256, impl=4),
                 _case('gru', 20, 3, 8, 256, impl=4)]
# ---- the fused two-layer stack (H = 256): a ragged tile with step pairs | odd T (fp32 rows), dropout off / on, both call forms
FUSED_SHAPES = [(33, 4, 16), (20, 3, 8)]
GRU_FUSED = [_case('gru', B, T, F, 256, form=form, p=p) for (B, T, F) in FUSED_SHAPES for p in (0.0, 0.5) for form in ('full', 'model')]
# ... and the smallest shape at which the fused backward writes the PK image of its gate gradients: api.hip's pk_ok wants every
# contraction that reads them on the three-term kernel, and gemm_plan (gemm.hip) hands a problem of fewer than 32 output tiles to
# gemm_small up to 2^27 multiply-adds -- layer 1's dW_ih is 768 x 256 x (B T), so B T >= 683, T even: 37 x 20, and F = 256 for layer 0's
# dW_ih and dX alike.  Below that the stack above runs the fp32-row forms at even T too, and mode 3 (bf16 storage) refuses the call.
PK_MIN_MACS = 1 << 27
GRU_FUSED_PK = [_case('gru', 37, 20, 256, 256, form=form, p=p) for p in (0.0, 0.5) for form in ('full', 'model')]


def writes_pk_image(c):
    return c['cell'] == 'gru' and c['H'] == 256 and c['T'] % 2 == 0 and 768 * min(c['F'], 256) * c['B'] * c['T'] > PK_MIN_MACS


# ---- DEP_LSTM_SV16=1: BiLSTM, H = 128.  Even and odd T (whole step pairs | not); dropout off / on; with and without dx; dense and ragged
LSTM = [_case('lstm', 19, T, 8, 128, p=p, dx=dx, ragged=r) for T in (6, 7) for p in (0.0, 0.5) for dx in (True, False) for r in (False, True)]
# ---- DEP_TRACE=1: the fused cases, one per-layer GRU case and one BiLSTM case
TRACE_EXTRA = [GRU_LAYER[6], LSTM[4]]
assert TRACE_EXTRA[0]['name'] == 'gru-B37-T6-F8-H128-i3-full-p0-dense-dx-m1' and TRACE_EXTRA[1]['name'] == 'lstm-B19-T6-F8-H128-i3-full-p0.5-dense-dx-m1'
# ---- DEP_FUSED2_BWD=0 under the single-product modes: the per-layer backward behind the fused forward, fp32 storage (2) | bf16 storage (3),
# at the shape that writes the PK image (the bf16-storage backward has no other form)
BF16_LAYER = [dict(c, mode=m, name=c['name'][:-1] + str(m)) for c in GRU_FUSED_PK for m in (2, 3)]

# ---- the gate regimes (module docstring), at shapes inside the rule above.  The fused stack: every regime, the full form at the two small
# shapes and the training step's form at the PK shape (T = 20: the only chain here long enough for a remembered state to matter)
NON_INIT = REGIMES[1:]
# One case of that grid is left out: 'sat' at the PK shape with dropout.  Its FORWARD misses the suite's 1e-4 on y (device 1.086e-4;
# 9.46e-5 without dropout, which stays in) in both saved-gate formats, and the gate phase is not the cause: the split-precision products
# hold each operand to 16 mantissa bits, and with weights times 4 the recurrence amplifies that over 20 steps -- a float64 forward
# with only the products split shows the same 1.07e-4 (split_products_forward, pinned in tests/test_switch_cases_cpu.py).
LEFT_OUT = [_case('gru', 37, 20, 256, 256, form='model', p=0.5, regime='sat')]
GRU_FUSED_REGIMES = [_case('gru', B, T, F, 256, form='full', p=p, regime=g) for g in NON_INIT for (B, T, F) in FUSED_SHAPES for p in (0.0, 0.5)] + \
                    [c for c in (_case('gru', 37, 20, 256, 256, form='model', p=p, regime=g) for g in NON_INIT for p in (0.0, 0.5)) if c not in LEFT_OUT]
# ... the per-layer sweeps, whole step pairs, dense and ragged; H = 256 ragged and impl = 4; the BiLSTM with dropout and dx, odd T
GRU_LAYER_REGIMES = [_case('gru', 37, 6, 8, H, ragged=r, regime=g) for g in ('memory', 'sat') for H in (64, 128, 512) for r in (False, True)]
GRU_LAYER_256_REGIMES = [_case('gru', 33, 4, 16, 256, ragged=True, regime='memory'), _case('gru', 33, 4, 16, 256, impl=4, regime='memory')]
LSTM_REGIMES = [_case('lstm', 19, 7, 8, 128, p=0.5, dx=True, ragged=r, regime=g) for g in ('memory', 'sat') for r in (False, True)]
GRU_REGIMES = GRU_LAYER_REGIMES + GRU_LAYER_256_REGIMES + GRU_FUSED_REGIMES
REGIME_CASES = GRU_REGIMES + LSTM_REGIMES
TRACE_REGIME = [c for c in GRU_FUSED_REGIMES if c['regime'] == 'memory' and writes_pk_image(c) and c['p'] > 0][:1]       # stamped forward and backward

# environment tag -> (the variables, the cases).  'default' is the bit-identity baseline of every other one.
ENVIRONMENTS = {
    'default': ({}, GRU_LAYER + GRU_LAYER_256 + GRU_FUSED + GRU_FUSED_PK + LSTM + REGIME_CASES),
    'sv16_off': ({'DEP_SV16': '0'}, GRU_LAYER + GRU_LAYER_256 + GRU_FUSED + GRU_FUSED_PK + GRU_REGIMES),
    'lstm_sv16': ({'DEP_LSTM_SV16': '1'}, LSTM + LSTM_REGIMES),
    'trace': ({'DEP_TRACE': '1'}, GRU_FUSED + GRU_FUSED_PK + TRACE_EXTRA + TRACE_REGIME),
    # the stamped fused forward has a row per saved-gate format: the fp32-gates one needs both switches
    'trace_sv16_off': ({'DEP_TRACE': '1', 'DEP_SV16': '0'}, GRU_FUSED),
    'layer_bwd': ({'DEP_FUSED2_BWD': '0'}, BF16_LAYER),
}
SWITCHES = ('DEP_SV16', 'DEP_LSTM_SV16', 'DEP_TRACE', 'DEP_FUSED2_BWD')        # a child's environment sets its own and none of the others


def make_rnn_params(rng, cell, F, H, L, dirs):
    """The weights of tests/test_kernels_gpu.py's make_rnn_params: uniform in +-1/sqrt(H), float32-rounded."""
    G = 3 if cell == 'gru' else 4
    P = {}; names = []
    prefix = 'lstm_net_audio' if cell == 'gru' else 'lstm_net'
    k = 1.0 / np.sqrt(H)
    for l in range(L):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else H * dirs
            for nm, shp in (('weight_ih', (G * H, inp)), ('weight_hh', (G * H, H)), ('bias_ih', (G * H,)), ('bias_hh', (G * H,))):
                key = f'{prefix}.{nm}_{sfx}'
                P[key] = f32(rng.uniform(-k, k, shp))
                names.append(key)
    return P, names, prefix


def apply_regime(regime, cell, P, x):
    """(P, x) of gate regime `regime` (module docstring) from an init-scale draw: new arrays, float32-rounded again.  P: any dict of
    torch.nn.GRU / LSTM parameters by name ('...weight_ih_l0', '...bias_ih_l1_reverse', ...); gate blocks [r | z | n] and [i | f | g | o]."""
    assert regime in REGIMES and not (regime == 'reset' and cell != 'gru'), (regime, cell)
    P = {k: v.copy() for k, v in P.items()}
    x = x.copy()
    block, shift = {'memory': (1, MEMORY_BIAS), 'reset': (0, RESET_BIAS)}.get(regime, (None, 0.0))
    for k in P:
        base = k.rsplit('.', 1)[-1]
        if block is not None and base.startswith('bias_ih'):
            H = P[k].shape[0] // (3 if cell == 'gru' else 4)
            P[k][block * H:(block + 1) * H] += shift
        if regime == 'sat' and base.startswith('weight_'):
            P[k] *= SAT_SCALE
        P[k] = f32(P[k])
    if regime == 'drive':
        x *= DRIVE_SCALE
    return P, f32(x)


def inputs(c):
    """Everything a run of case c is fed, float32-rounded float64 arrays: the child and the parent call this with the same case.  The
    seed leaves out form, p, dx, mode, impl and the regime: cases that differ in those alone share one draw of weights and inputs."""
    B, T, F, H = c['B'], c['T'], c['F'], c['H']
    gru = c['cell'] == 'gru'
    dirs = 1 if gru else 2
    rng = np.random.default_rng(B * 1000 + T * 100 + F + H + (7 if c['ragged'] else 0))
    P, names, prefix = make_rnn_params(rng, c['cell'], F, H, LAYERS, dirs)
    lengths = lengths_mix(B, T, rng) if c['ragged'] else None
    x = f32(rng.standard_normal((B, T, F)))
    if lengths is not None:
        x[np.arange(T)[None, :] >= lengths[:, None]] = 0.0           # finite padding
    P, x = apply_regime(c.get('regime', 'init'), c['cell'], P, x)
    out = dict(P=P, names=names, prefix=prefix, x=x, lengths=lengths,
               dy=f32(rng.standard_normal((B, T, H * dirs)) * 0.3))
    if gru:
        out['dpooled'] = f32(rng.standard_normal((B, H)))
    else:
        out['dh_n'] = f32(rng.standard_normal((LAYERS * 2, B, H)) * 0.3)
    return out


# ---- the 16-bit saved gates (csrc/rnn_cluster_common.h; rnn_cluster_lstm.hip: "SV16"): sigmoid gates as unorm16, tanh gates as snorm16
def unorm16(a):
    return np.round(a * 65535.0) / 65535.0


def snorm16(a):
    return np.round(a * 32767.0) / 32767.0


def quantise_gru_caches(caches):
    """Copies of gru_stack_fwd's caches with r, z as unorm16 and n as snorm16 (gh_n, the outputs and the inputs stay as they are)."""
    return [(x, ys, unorm16(Rg), unorm16(Zg), snorm16(Ng), HN) for (x, ys, Rg, Zg, Ng, HN) in caches]


def quantise_lstm_caches(caches):
    """Copies of bilstm_stack_fwd's caches with the activated gates [i | f | g | o] as unorm16, g as snorm16 (c stays fp32 on the device)."""
    out = []
    for (x, ys, cs, gates, reverse) in caches:
        H = ys.shape[-1]
        q = unorm16(gates)
        q[..., 2 * H:3 * H] = snorm16(gates[..., 2 * H:3 * H])
        out.append((x, ys, cs, q, reverse))
    return out


GATE_DELTA_SIGMOID = 2e-7   # the documented error of fast_sigmoid / fast_tanh (csrc/rnn_cluster_common.h) on a gate's value
GATE_DELTA_TANH = 4e-7
PERTURB_SEED = 2024


def perturb_gates(cell, seed=PERTURB_SEED):
    """-> a function of the caches: the saved gates moved by uniform +-GATE_DELTA_SIGMOID (sigmoid gates) | +-GATE_DELTA_TANH (tanh
    gates), what float32 gate functions may do to them.  One generator per returned function: two functions of one seed called on the
    same caches in the same order make the same moves."""
    rng = np.random.default_rng(seed)
    u = lambda a, d: a + rng.uniform(-d, d, a.shape)
    if cell == 'gru':
        return lambda caches: [(x, ys, u(Rg, GATE_DELTA_SIGMOID), u(Zg, GATE_DELTA_SIGMOID), u(Ng, GATE_DELTA_TANH), HN)
                               for (x, ys, Rg, Zg, Ng, HN) in caches]

    def lstm(caches):
        out = []
        for (x, ys, cs, gates, reverse) in caches:
            H = ys.shape[-1]
            d = np.full(gates.shape[-1], GATE_DELTA_SIGMOID); d[2 * H:3 * H] = GATE_DELTA_TANH
            out.append((x, ys, cs, gates + rng.uniform(-1.0, 1.0, gates.shape) * d, reverse))
        return out
    return lstm


def references(c, inp, mask, transforms):
    """One forward of the oracle's row loop and one backward per entry of `transforms`, each a function of the saved-gate caches (None:
    the caches as they are) -> [dict(y, h_n, [pooled,] dx, G)] in that order; the outputs are the same arrays in every entry."""
    gru = c['cell'] == 'gru'
    P, prefix, x, lengths = inp['P'], inp['prefix'], inp['x'], inp['lengths']
    B, T, H = c['B'], c['T'], c['H']
    masks = None if mask is None else [mask]
    dy = inp['dy'] if (not gru or c['form'] == 'full') else None
    rows = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(lengths[b])) for b in range(B) if lengths[b] > 0]
    dirs = 1 if gru else 2
    y = np.zeros((B, T, H * dirs)); h_n = np.zeros((LAYERS * dirs, B, H))
    pooled = np.zeros((B, H))
    dxs = [np.zeros(x.shape) for _ in transforms]
    Gs = [{k: np.zeros_like(v) for k, v in P.items()} for _ in transforms]
    for sl, n in rows:
        mb = None if masks is None else [masks[0][sl, :n]]
        if gru:
            yb, caches = R.gru_stack_fwd(x[sl, :n], P, prefix, LAYERS, mb)
            pooled[sl] = yb.mean(1)
            for l in range(LAYERS):
                h_n[l, sl] = caches[l][1][:, -1]
            d = np.repeat(inp['dpooled'][sl][:, None, :] / n, n, axis=1)
            if dy is not None:
                d = d + dy[sl, :n]
        else:
            yb, hb, caches = R.bilstm_stack_fwd(x[sl, :n], P, prefix, LAYERS, mb)
            h_n[:, sl] = hb
        y[sl, :n] = yb
        for dx, G, tr in zip(dxs, Gs, transforms):
            fed = caches if tr is None else tr(caches)
            if gru:
                dxb, Gb = R.gru_stack_bwd(d, P, prefix, LAYERS, fed, mb)
            else:
                dxb, Gb = R.bilstm_stack_bwd(dy[sl, :n], inp['dh_n'][:, sl], P, prefix, LAYERS, fed, mb)
            dx[sl, :n] = dxb
            for k, v in Gb.items():
                G[k] += v
    outs = [dict(y=y, h_n=h_n, dx=dx, G=G) for dx, G in zip(dxs, Gs)]
    if gru:
        for o in outs:
            o['pooled'] = pooled
    return outs


def reference(c, inp, mask=None, quantised=False):
    """The oracle's outputs and gradients of case c: dict(y, h_n, [pooled,] dx, G).  mask: the inter-layer dropout mask the device drew
    ((B, T, H * dirs), scaled), when c['p'] > 0.  quantised: the backward is fed the 16-bit saved gates -- the oracle of the operation the
    16-bit forms compute.  A ragged case is the row loop of tests/varlen_ref.py (which it calls when nothing is quantised)."""
    gru = c['cell'] == 'gru'
    if inp['lengths'] is not None and not quantised:
        P, prefix, x, lengths = inp['P'], inp['prefix'], inp['x'], inp['lengths']
        masks = None if mask is None else [mask]
        if gru:
            return gru_ragged(x, lengths, P, prefix, LAYERS, 'mean', dy=inp['dy'] if c['form'] == 'full' else None, dpooled=inp['dpooled'], masks=masks)
        return bilstm_ragged(x, lengths, P, prefix, LAYERS, dy=inp['dy'], dhn=inp['dh_n'], masks=masks)
    # (looked up at the call: tests/test_switch_cases_cpu.py swaps the quantisers for the identity)
    requant = (lambda caches: (quantise_gru_caches if gru else quantise_lstm_caches)(caches)) if quantised else None
    return references(c, inp, mask, [requant])[0]


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


# ---- the split-precision products (csrc/rnn_cluster_common.h: split_word; gemm_bf16x3.hip): each operand as bf16(x) + bf16(x - bf16(x)),
# 16 mantissa bits, and hi hi + hi lo + lo hi of the four partial products
def bf16_round(a):
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def split_matmul(a, w):
    """a @ w.T as the split-precision kernels form it, accumulated in float64."""
    ah, wh = bf16_round(a), bf16_round(w)
    al, wl = bf16_round(a - ah), bf16_round(w - wh)
    return ah @ wh.T + ah @ wl.T + al @ wh.T


def split_products_forward(c, inp, mask=None):
    """The two-layer GRU forward of dense case c in float64 with split_matmul for every product and nothing else changed -> y (B, T, H).
    Its distance from the oracle's y is what the operand format alone costs the forward at this case."""
    assert c['cell'] == 'gru' and inp['lengths'] is None
    P, prefix, H = inp['P'], inp['prefix'], c['H']
    seq = inp['x']
    for l in range(LAYERS):
        w_ih, w_hh, b_ih, b_hh = (P[f'{prefix}.{n}_l{l}'] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
        B, T, _ = seq.shape
        gi = split_matmul(seq.reshape(B * T, -1), w_ih).reshape(B, T, -1) + b_ih
        h = np.zeros((B, H)); ys = np.zeros((B, T, H))
        for t in range(T):
            gh = split_matmul(h, w_hh) + b_hh
            r = R.sigmoid(gi[:, t, :H] + gh[:, :H])
            z = R.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
            h = (1.0 - z) * n + z * h
            ys[:, t] = h
        seq = ys if (mask is None or l == LAYERS - 1) else ys * mask
    return seq


def backward_tensors(c, inp):
    """The names of what a run of case c returns from its backward: every weight gradient, and dx where the case has one."""
    return list(inp['names']) + (['dx'] if c['dx'] else [])


def worst_relerr(c, inp, got, ref):
    """(worst relerr, tensor name) of reference dict `got` against `ref` over backward_tensors(c)."""
    pick = lambda r, n: r['dx'] if n == 'dx' else r['G'][n]
    return max((relerr(pick(got, n), pick(ref, n)), n) for n in backward_tensors(c, inp))


def storage_figures(c, inp, mask=None):
    """What the saved-gate storage alone does to case c's backward, oracle against oracle in float64 -> dict of (relerr, tensor):
      E_q    the backward fed the 16-bit gates against the exact one
      F_d    the backward fed gates moved by the float32 gate functions' error (perturb_gates) against the exact one
      sim    moved, then quantised: a simulated 16-bit device"""
    gru = c['cell'] == 'gru'
    quant = quantise_gru_caches if gru else quantise_lstm_caches
    move, move2 = perturb_gates(c['cell']), perturb_gates(c['cell'])
    exact, q, f, sim = references(c, inp, mask, [None, quant, move, lambda caches: quant(move2(caches))])
    return dict(E_q=worst_relerr(c, inp, q, exact), F_d=worst_relerr(c, inp, f, exact), sim=worst_relerr(c, inp, sim, exact))
