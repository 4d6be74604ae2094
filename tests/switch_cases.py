"""Cases, seeded inputs and references of the switch-selected sweep instances (tests/test_switch_forms_gpu.py).

The rows of the cluster families' instance tables that only an environment switch selects can be launched by no in-process test: the
switches are read once per process.  tests/switch_probe.py runs the case lists below in one child process per environment; the parent
builds the SAME arrays from `inputs()` and compares with the float64 oracle (oracle/ref_numpy.py, tests/varlen_ref.py).  numpy only:
the CPU test of this module (tests/test_switch_cases_cpu.py) runs without a GPU.

A case is a dict: name, cell ('gru' | 'lstm'), B, T, F, H, impl, form, p (inter-layer dropout), ragged, dx, mode (dep_set_gemm_mode).
  GRU  'full' : dy + dpooled in, dx out (mean pool);  'model': dpooled only, no dx -- what the training step passes
  LSTM        : dy + dh_n in, dx as the case says
"""
import numpy as np

from oracle import ref_numpy as R
from varlen_ref import bilstm_ragged, gru_ragged, lengths_mix

LAYERS = 2
DROP_SEED = 1234            # desc.seed of every case; the inter-layer mask is dep_dropout_mask(.., DROP_SEED, site 16)


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _case(cell, B, T, F, H, impl=3, form='full', p=0.0, ragged=False, dx=True, mode=1):
    c = dict(cell=cell, B=B, T=T, F=F, H=H, impl=impl, form=form, p=p, ragged=ragged, dx=dx and form == 'full', mode=mode)
    c['name'] = '%s-B%d-T%d-F%d-H%d-i%d-%s-p%g-%s-%s-m%d' % (cell, B, T, F, H, impl, form, p, 'ragged' if ragged else 'dense',
                                                             'dx' if c['dx'] else 'nodx', mode)
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

# environment tag -> (the variables, the cases).  'default' is the bit-identity baseline of every other one.
ENVIRONMENTS = {
    'default': ({}, GRU_LAYER + GRU_LAYER_256 + GRU_FUSED + GRU_FUSED_PK + LSTM),
    'sv16_off': ({'DEP_SV16': '0'}, GRU_LAYER + GRU_LAYER_256 + GRU_FUSED + GRU_FUSED_PK),
    'lstm_sv16': ({'DEP_LSTM_SV16': '1'}, LSTM),
    'trace': ({'DEP_TRACE': '1'}, GRU_FUSED + GRU_FUSED_PK + TRACE_EXTRA),
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


def inputs(c):
    """Everything a run of case c is fed, float32-rounded float64 arrays: the child and the parent call this with the same case.  The
    seed leaves out form, p, dx, mode and impl: cases that differ in those alone share weights and inputs."""
    B, T, F, H = c['B'], c['T'], c['F'], c['H']
    gru = c['cell'] == 'gru'
    dirs = 1 if gru else 2
    rng = np.random.default_rng(B * 1000 + T * 100 + F + H + (7 if c['ragged'] else 0))
    P, names, prefix = make_rnn_params(rng, c['cell'], F, H, LAYERS, dirs)
    lengths = lengths_mix(B, T, rng) if c['ragged'] else None
    x = f32(rng.standard_normal((B, T, F)))
    if lengths is not None:
        x[np.arange(T)[None, :] >= lengths[:, None]] = 0.0           # finite padding
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


def reference(c, inp, mask=None, quantised=False):
    """The oracle's outputs and gradients of case c: dict(y, h_n, [pooled,] dx, G).  mask: the inter-layer dropout mask the device drew
    ((B, T, H * dirs), scaled), when c['p'] > 0.  quantised: the backward is fed the 16-bit saved gates -- the oracle of the operation the
    16-bit forms compute.  A ragged case is the row loop of tests/varlen_ref.py (which it calls when nothing is quantised)."""
    gru = c['cell'] == 'gru'
    P, prefix, x, lengths = inp['P'], inp['prefix'], inp['x'], inp['lengths']
    B, T, H = c['B'], c['T'], c['H']
    masks = None if mask is None else [mask]
    dy = inp['dy'] if (not gru or c['form'] == 'full') else None
    if lengths is not None and not quantised:
        if gru:
            return gru_ragged(x, lengths, P, prefix, LAYERS, 'mean', dy=dy, dpooled=inp['dpooled'], masks=masks)
        return bilstm_ragged(x, lengths, P, prefix, LAYERS, dy=dy, dhn=inp['dh_n'], masks=masks)
    requant = (quantise_gru_caches if gru else quantise_lstm_caches) if quantised else (lambda caches: caches)
    rows = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), int(lengths[b])) for b in range(B) if lengths[b] > 0]
    dirs = 1 if gru else 2
    y = np.zeros((B, T, H * dirs)); h_n = np.zeros((LAYERS * dirs, B, H)); dx = np.zeros(x.shape)
    G = {k: np.zeros_like(v) for k, v in P.items()}
    pooled = np.zeros((B, H))
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
            dxb, Gb = R.gru_stack_bwd(d, P, prefix, LAYERS, requant(caches), mb)
        else:
            yb, hb, caches = R.bilstm_stack_fwd(x[sl, :n], P, prefix, LAYERS, mb)
            h_n[:, sl] = hb
            dxb, Gb = R.bilstm_stack_bwd(dy[sl, :n], inp['dh_n'][:, sl], P, prefix, LAYERS, requant(caches), mb)
        y[sl, :n] = yb; dx[sl, :n] = dxb
        for k, v in Gb.items():
            G[k] += v
    out = dict(y=y, h_n=h_n, dx=dx, G=G)
    if gru:
        out['pooled'] = pooled
    return out


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)
