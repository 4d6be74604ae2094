"""The cases of tests/test_local_lstm_train_gpu.py (impl = 9, the exchange-free LSTM training sweeps) and the guard that their state
matters, on the float64 reference alone: numpy only, no torch and no GPU, so tests/test_local_lstm_train_cpu.py runs the guard on the very
data the GPU test uses."""
import os
import re

import numpy as np

import hx_ref
import state_varlen_ref as svr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-4
RTOL = 1e-4
PREFIX = 'lstm'
H = 128
F = 8
STATE_SCALE = 1.5          # of hx / cx: large enough that the reference's dW_hh, dx and dhx move by > 100 bars in every case (state_guard;
                           # at 0.6 the dx of the three-layer unidirectional case moves by 61)


def prefetch_depth():
    """Steps lstm_bwd_local requests its inputs ahead (its register ring), read from the source."""
    src = open(os.path.join(ROOT, 'icassp2022-depression_amd', 'csrc', 'rnn_local_lstm.hip')).read()
    return int(re.search(r'constexpr int LBL_PF = (\d+);', src).group(1))


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def case_rng(*v):
    return np.random.default_rng(900 + sum(int(a * 2) * 7 ** i for i, a in enumerate(v)))


def make_params(rng, Lyr, dirs):
    """Weights in the order the header documents: l0 [, l0_reverse], l1, ...; layer l > 0 has weight_ih (4H, dirs*H)."""
    P = {}; names = []
    k = 1.0 / np.sqrt(H)
    for l in range(Lyr):
        for d in range(dirs):
            sfx = f'l{l}' + ('_reverse' if d else '')
            inp = F if l == 0 else dirs * H
            for nm, shp in (('weight_ih', (4 * H, inp)), ('weight_hh', (4 * H, H)), ('bias_ih', (4 * H,)), ('bias_hh', (4 * H,))):
                key = f'{PREFIX}.{nm}_{sfx}'
                P[key] = f32(rng.uniform(-k, k, shp))
                names.append(key)
    return P, names


class Data:
    """Host side of one case: weights, input, state and gradient inputs (numpy, no GPU).  lengths: a numpy int vector or None."""

    def __init__(self, B, T, Lyr, dirs, lengths=None, p=0.0, tag=0):
        rng = case_rng(B, T, Lyr, dirs, p, tag)
        self.B, self.T, self.Lyr, self.dirs, self.n, self.p = B, T, Lyr, dirs, None if lengths is None else np.asarray(lengths), p
        self.P, self.names = make_params(rng, Lyr, dirs)
        self.x = f32(rng.standard_normal((B, T, F)))
        K = Lyr * dirs
        self.hx = f32(rng.standard_normal((K, B, H)) * STATE_SCALE)
        self.cx = f32(rng.standard_normal((K, B, H)) * STATE_SCALE)
        self.dy = f32(rng.standard_normal((B, T, dirs * H)) * 0.3)
        self.dhn = f32(rng.standard_normal((K, B, H)) * 0.3)
        self.dcn = f32(rng.standard_normal((K, B, H)) * 0.3)
        if self.n is not None:
            self.pad = np.arange(T)[None, :] >= self.n[:, None]
            self.x[self.pad] = 0.0

    def ref(self, hx=True, cx=True, dy=True, dhn=True, dcn=True, masks=None):
        kw = dict(hx=self.hx if hx else None, cx=self.cx if cx else None, dy=self.dy if dy else None, dhn=self.dhn if dhn else None,
                  dcn=self.dcn if dcn else None, masks=masks)
        if self.n is not None:
            return svr.stack(self.x, self.n, self.P, PREFIX, 'lstm', self.dirs, self.Lyr, **kw)
        return hx_ref.stack(self.x, self.P, PREFIX, 'lstm', self.dirs, self.Lyr, **kw)

    def state_guard(self, hx=True, cx=True, masks=None):
        """On the reference alone: dW_hh of layer 0, dx and dhx with the state differ from those without it by more than 100 bars, so a
        kernel that dropped a state term cannot pass.  Returns the three figures."""
        a, b = self.ref(hx, cx, masks=masks), self.ref(False, False, masks=masks)
        live = slice(None) if self.n is None else self.n > 0
        k = f'{PREFIX}.weight_hh_l0'
        figs = (float(relerr(a['G'][k], b['G'][k])) / RTOL, float(np.abs(a['dx'] - b['dx']).max()) / ATOL,
                float(np.abs(a['dhx'][:, live] - b['dhx'][:, live]).max()) / ATOL)
        assert min(figs) > 100, f'the state does not matter enough (dW_hh, dx, dhx in bars): {figs}'
        return figs


# (B, T, layers, dirs, p).  B: a partial tile | a whole tile | two tiles | more tiles than one padded group of 8.  T: one step, no MFMA
# unless dhx is asked | both LDS parities | the ring wraps | prefetch depth + 1 | 7.  Depth 1 .. 3 with and without the inter-layer mask.
def dense_cases():
    return [(3, 1, 1, 2, 0.0), (16, 2, 1, 1, 0.0), (17, 3, 2, 2, 0.5), (129, prefetch_depth() + 1, 1, 2, 0.0), (5, 7, 3, 2, 0.5),
            (5, 7, 3, 1, 0.0), (17, 7, 2, 1, 0.5)]


def dense_data(case):
    B, T, Lyr, dirs, p = case
    return Data(B, T, Lyr, dirs, p=p)


def ragged_lengths(B, T, rng):
    """Rows 0 .. 7 and 8 .. 15 each hold every length 0 .. T once, shuffled; the second tile has a full row, a one-step row and an empty one."""
    assert T + 1 == 8 and B == 19
    first = np.concatenate([rng.permutation(T + 1), rng.permutation(T + 1)])
    return np.concatenate([first, [T, 1, 0]]).astype(np.int64)


def ragged_data(dirs):
    B, T = 19, 7
    return Data(B, T, 2, dirs, lengths=ragged_lengths(B, T, case_rng(B, T, dirs)), p=0.5, tag=1)


def trap_a_data():
    """Direction 1's first live step (t = len - 1) sits inside the padding of rows 0 and 2, with a non-zero cx."""
    return Data(3, 5, 1, 2, lengths=[2, 5, 3], tag=2)
