"""Helper of test_switch_forms_gpu.py: runs cases of tests/switch_cases.py through _lib.Rnn in THIS process' environment (the sweep
switches are read once per process) and saves, per case, every output, every gradient and the kernel template instances it launched.

    python tests/switch_probe.py --batch cases.json        cases.json: [[out.npz, case], ...], one process for the whole list

run_case() is also what the in-process bf16-storage test of that module calls."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402
import switch_cases as S  # noqa: E402


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to('cuda:0')


def run_case(c, own_log=True):
    """-> {name: numpy array}: y (fp32-storage modes), pooled (GRU), h_n, g0.. (the weight gradients in the order of inputs()['names']), dx
    where the case asks, mask (the inter-layer dropout mask drawn for the case's seed, p > 0) and `instances`.  The precision mode is
    the case's on every contraction size (threshold 0), as the suite's gemm_mode fixture sets it; the caller restores the default.
    own_log = False: the launch-instance log is the caller's (conftest.py keeps it on during an oracle test), no `instances`."""
    DEV = torch.device('cuda:0')
    inp = S.inputs(c)
    gru = c['cell'] == 'gru'
    B, T, F, H, p = c['B'], c['T'], c['F'], c['H'], c['p']
    dirs = 1 if gru else 2
    L.set_gemm_mode(c['mode'], 0)
    if own_log:
        L.instance_log_enable(True)
    Wd = [dev(inp['P'][n]) for n in inp['names']]
    Gd = [torch.full_like(w, float('nan')) for w in Wd]
    xd = dev(inp['x'])
    ld = None if inp['lengths'] is None else dev(inp['lengths'], np.int32)
    rnn = L.Rnn(L.CELL_GRU if gru else L.CELL_LSTM, B, T, F, H, S.LAYERS, dirs, True, p, L.POOL_MEAN if gru else L.POOL_NONE, DEV, impl=c['impl'])
    rnn.reserve.fill_(float('nan'))
    pooled = torch.full((B, H), float('nan'), device=DEV) if gru else None
    h_n = torch.full((S.LAYERS * dirs, B, H), float('nan'), device=DEV)
    dxd = torch.full((B, T, F), float('nan'), device=DEV) if c['dx'] else None
    rnn.forward(xd, Wd, seed=S.DROP_SEED, pooled=pooled, h_n=h_n, lengths=ld)
    dy = inp['dy'].copy()
    if ld is not None and c['form'] == 'full':
        dy[np.arange(T)[None, :] >= inp['lengths'][:, None]] = np.nan      # the padded positions of dy are ignored
    if gru:
        rnn.backward(xd, Wd, Gd, dy=dev(dy) if c['form'] == 'full' else None, dpooled=dev(inp['dpooled']), dx=dxd, lengths=ld)
    else:
        rnn.backward(xd, Wd, Gd, dy=dev(dy), dh_n=dev(inp['dh_n']), dx=dxd, lengths=ld)
    rnn.check()
    torch.cuda.synchronize()
    res = {'g%d' % i: g.cpu().numpy() for i, g in enumerate(Gd)}
    res['h_n'] = h_n.cpu().numpy()
    if c['mode'] != 3:                                  # (bf16 storage: the reserve's output sequence is not an fp32 array)
        res['y'] = rnn.layer_output().cpu().numpy()
    if gru:
        res['pooled'] = pooled.cpu().numpy()
    if dxd is not None:
        res['dx'] = dxd.cpu().numpy()
    if p > 0:
        res['mask'] = L.dropout_mask(B * T * H * dirs, p, S.DROP_SEED, 16, DEV).cpu().numpy().reshape(B, T, H * dirs)      # site = DEP_SITE_RNN0 + 0
    if own_log:
        res['instances'] = np.array(sorted(L.instance_log_read(reset=True)))
        L.instance_log_enable(False)
    return res


if __name__ == '__main__':
    import json
    assert sys.argv[1] == '--batch'
    for out_, case_ in json.load(open(sys.argv[2])):
        t0 = time.time()
        np.savez(out_, **run_case(case_))
        print('switch_probe %s: %.2f s' % (case_['name'], time.time() - t0), flush=True)
        torch.cuda.empty_cache()
