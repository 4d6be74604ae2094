#!/usr/bin/env python3
"""attention_net_with_w alone at (B, T, H) = (256, 300, 512), K = 4, dense: the first-generation kernels (DEP_ATTN_V1=1) against the default
(attention.hip's instances where it has one for the width), forward and backward separately.

    python tools/bench_attn.py            (ROUNDS=3 alternated rounds of one child process per side; REPS=50 timed calls per child and direction;
                                           SHAPE=256,300,512)

The switch is read once per process, so every measurement is a child process of its own; the parent never opens the GPU.  A child warms up, then
times REPS calls of L.attn_fwd and of L.attn_bwd with device events (the whole call: hsum, the projection GEMM, the attention kernel; the
backward with its broadcast and weight-gradient GEMMs) and prints the median, the min and the max, the instances the log saw, and a checksum of
ctx and dout, which the two sides must share to the last digits printed.  The parent prints per side and direction the median over the rounds'
medians and their spread (max - min)."""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    import torch
    sys.path.insert(0, ROOT)
    from icassp2022_depression_amd import _lib as L
    B, T, H = (int(v) for v in os.environ.get('SHAPE', '256,300,512').split(','))
    K, reps = 4, int(os.environ.get('REPS', 50))
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    out, h_n, Wa, ba, dctx = r(B, T, 2 * H), r(K, B, H), r(H, H) * (0.02 / H ** 0.5), r(H) * 0.02, r(B, H)
    dWa, dba = torch.empty_like(Wa), torch.empty_like(ba)
    L.instance_log_enable(True)
    ctx, att = L.attn_fwd(out, h_n, Wa, ba)
    dout, _ = L.attn_bwd(dctx, out, Wa, att, K, dWa, dba)
    torch.cuda.synchronize()
    inst = sorted({m.group(0).lstrip('( ') for m in (re.match(r'^\(?\s*\w+\s*(?:<[^>]*>)?', s) for s in L.instance_log_read(reset=True)) if 'attn_' in m.group(0)})
    L.instance_log_enable(False)
    res = dict(side=os.environ.get('DEP_ATTN_V1', '0'), instances=inst, ctx_sum=float(ctx.double().sum()), dout_abs_sum=float(dout.double().abs().sum()))
    for what, fn in (('fwd', lambda: L.attn_fwd(out, h_n, Wa, ba)), ('bwd', lambda: L.attn_bwd(dctx, out, Wa, att, K, dWa, dba))):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[what] = dict(median=statistics.median(ts), min=min(ts), max=max(ts))
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    rounds = int(os.environ.get('ROUNDS', 3))
    sides = (('first generation (DEP_ATTN_V1=1)', '1'), ('default', '0'))
    got = {name: [] for name, _ in sides}
    for r in range(rounds):
        for name, v1 in sides:
            env = dict(os.environ, DEP_ATTN_V1=v1)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, capture_output=True, text=True, timeout=600)
            line = next((l for l in p.stdout.split('\n') if l.startswith('RESULT ')), None)
            if p.returncode != 0 or line is None:
                sys.exit('child failed (%d):\n%s\n%s' % (p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            res = json.loads(line[7:])
            got[name].append(res)
            print('round %d  %-34s fwd %.3f ms (%.3f .. %.3f)  bwd %.3f ms (%.3f .. %.3f)  ctx sum %.6f  |dout| sum %.4f  %s' % (
                r, name, res['fwd']['median'], res['fwd']['min'], res['fwd']['max'], res['bwd']['median'], res['bwd']['min'], res['bwd']['max'],
                res['ctx_sum'], res['dout_abs_sum'], ' '.join(res['instances'])), flush=True)
    print('attention at (B, T, H) = (%s), K = 4, dense; %d alternated rounds, one process each' % (os.environ.get('SHAPE', '256,300,512'), rounds))
    for name, _ in sides:
        for d in ('fwd', 'bwd'):
            m = [x[d]['median'] for x in got[name]]
            print('%-34s %s  median %.3f ms  spread %.3f (min %.3f max %.3f)' % (name, d, statistics.median(m), max(m) - min(m), min(m), max(m)))


if __name__ == '__main__':
    child() if '--child' in sys.argv else main()
