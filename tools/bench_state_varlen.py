#!/usr/bin/env python3
"""Forward / backward time of the dep_rnn operator on the per-layer tile sweeps in the four call forms around the recurrent state
(DESIGN 4.14): tools/bench_rnn.py's stack (2 layers, dropout 0.5, training, impl 2) called

    dense          dep_rnn_forward / dep_rnn_backward
    dense_state    dep_rnn_forward_state / dep_rnn_backward_state with hx (cx), dhx (dcx)
    ragged         dep_rnn_forward_varlen / dep_rnn_backward_varlen, lengths uniform in [T/2, T]
    ragged_state   dep_rnn_forward_state_varlen / dep_rnn_backward_state_varlen, the same lengths and state

    python tools/bench_state_varlen.py gru|lstm|bigru dense,dense_state,ragged [B T F H]        (STEPS=20 steps per form)

DEP_LIB_PATH=/path/to/another/libdep_rnn.so times another build of the same ABI (the parent commit's, for an alternated A/B); a build
that predates the *_state_varlen entry points runs the first three forms.  One line per form."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402

NEWER = ('dep_rnn_forward_state_varlen', 'dep_rnn_backward_state_varlen', 'dep_stream_accumulate', 'dep_stream_finish')


def main():
    cell = sys.argv[1] if len(sys.argv) > 1 else 'gru'
    forms = (sys.argv[2] if len(sys.argv) > 2 else 'dense,dense_state,ragged,ragged_state').split(',')
    B, T, F, H = map(int, sys.argv[3:7]) if len(sys.argv) > 6 else (512, 300, 256, 256)
    steps = int(os.environ.get('STEPS', 20))
    L.load(optional=NEWER if os.environ.get('DEP_LIB_PATH') else ())
    dev = torch.device('cuda:0')
    gru = cell in ('gru', 'bigru')
    dirs = 1 if cell == 'gru' else 2
    G = 3 if gru else 4
    torch.manual_seed(0)
    x = torch.randn(B, T, F, device=dev)
    W = []
    for l in range(2):
        for d in range(dirs):
            inp = F if l == 0 else H * dirs
            k = H ** -0.5
            W += [(torch.rand(G * H, inp, device=dev) * 2 - 1) * k, (torch.rand(G * H, H, device=dev) * 2 - 1) * k,
                  (torch.rand(G * H, device=dev) * 2 - 1) * k, (torch.rand(G * H, device=dev) * 2 - 1) * k]
    Gd = [torch.empty_like(w) for w in W]
    rnn = L.Rnn(L.CELL_GRU if gru else L.CELL_LSTM, B, T, F, H, 2, dirs, True, 0.5, L.POOL_MEAN if gru else L.POOL_NONE, dev, impl=2)
    pooled = torch.empty(B, dirs * H, device=dev) if gru else None
    hn = torch.empty(2 * dirs, B, H, device=dev)
    dpool = torch.randn(B, dirs * H, device=dev) if gru else None
    dy = None if gru else torch.randn(B, T, 2 * H, device=dev)
    dhn = None if gru else torch.randn(2 * dirs, B, H, device=dev)
    dx = torch.empty_like(x)
    hx = torch.randn(2 * dirs, B, H, device=dev) * 0.5
    cx = None if gru else torch.randn(2 * dirs, B, H, device=dev) * 0.5
    cn = None if gru else torch.empty_like(hx)
    dhx = torch.empty_like(hx)
    dcx = None if gru else torch.empty_like(hx)
    g = torch.Generator(device='cpu'); g.manual_seed(7)
    n = torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    calls = {
        'dense': (lambda i: rnn.forward(x, W, seed=i, pooled=pooled, h_n=hn),
                  lambda: rnn.backward(x, W, Gd, dy=dy, dpooled=dpool, dh_n=dhn, dx=dx)),
        'dense_state': (lambda i: rnn.forward(x, W, seed=i, pooled=pooled, h_n=hn, hx=hx, cx=cx, c_n=cn),
                        lambda: rnn.backward(x, W, Gd, dy=dy, dpooled=dpool, dh_n=dhn, dx=dx, hx=hx, cx=cx, dhx=dhx, dcx=dcx)),
        'ragged': (lambda i: rnn.forward(x, W, seed=i, pooled=pooled, h_n=hn, lengths=n),
                   lambda: rnn.backward(x, W, Gd, dy=dy, dpooled=dpool, dh_n=dhn, dx=dx, lengths=n)),
        'ragged_state': (lambda i: rnn.forward_state_varlen(x, W, n, seed=i, pooled=pooled, h_n=hn, hx=hx, cx=cx, c_n=cn),
                         lambda: rnn.backward_state_varlen(x, W, Gd, n, dy=dy, dpooled=dpool, dh_n=dhn, dx=dx, hx=hx, cx=cx, dhx=dhx, dcx=dcx)),
    }
    for form in forms:
        fwd, bwd = calls[form]
        fwd(0); bwd(); torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tf = tb = 0.0
        for i in range(steps):
            e[0].record(); fwd(i + 1); e[1].record(); bwd(); e[2].record()
            torch.cuda.synchronize()
            tf += e[0].elapsed_time(e[1]); tb += e[1].elapsed_time(e[2])
        rnn.check()
        print(f'{cell} {form} B={B} T={T} F={F} H={H}: fwd {tf / steps:.3f} ms  bwd {tb / steps:.3f} ms', flush=True)


if __name__ == '__main__':
    main()
