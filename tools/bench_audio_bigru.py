#!/usr/bin/env python3
"""One training step of the audio classifier, unidirectional and bidirectional, on synthetic data: forward + CE loss +
backward + AdamW step of audio_gru_whole.AudioBiLSTM in train mode (dropout 0.5), three sides alternated in one process:

    uni      (B, T, F, H) = (512, 300, 256, 256), config['bidirectional'] = False    the cfg2 step (fused two-layer kernels)
    bi       (512, 300, 256, 256), bidirectional = True                              impl = 7 sweeps, attention, two-map LayerNorm fold
    bi512    (256, 300, 256, 512), bidirectional = True                              the width only impl = 7 trains

    python tools/bench_audio_bigru.py          (RUNS=9 alternated rounds after two warm-up steps per side; SIDES=uni,bi,bi512)

One line per round, then per side the median, min and max of the step, and the parts of one further step of each side: the sweeps and
the contractions from the library's own per-category event timing (dep_profile_*: that step is profiled, not timed), and the attention
forward and backward (bidirectional sides) timed alone with device events on the step's own tensors.  Step times are host wall time
around a device synchronisation."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icassp2022_depression_amd import _lib as L  # noqa: E402
from icassp2022_depression_amd import audio_gru_whole, nn  # noqa: E402

SIDES = {'uni': (512, 300, 256, 256, False), 'bi': (512, 300, 256, 256, True), 'bi512': (256, 300, 256, 512, True)}


class Side:
    def __init__(self, name):
        self.name = name
        B, T, F, H, bi = SIDES[name]
        self.shape = (B, T, F, H)
        cfg = dict(audio_gru_whole.config); cfg.update(embedding_size=F, hidden_dims=H, bidirectional=bi)
        self.model = audio_gru_whole.AudioBiLSTM(cfg, seed=0)
        self.model.train()
        self.opt = nn.AdamW(audio_gru_whole.get_param_group(self.model), lr=cfg['learning_rate'])
        self.crit = nn.CrossEntropyLoss()
        g = torch.Generator(device='cpu').manual_seed(1)
        self.x = torch.randn(B, T, F, generator=g).to(self.model.device)
        self.y = torch.randint(0, 2, (B,), generator=g).numpy()
        self.times = []

    def step(self):
        self.opt.zero_grad()
        self.crit(self.model(self.x), self.y).backward()
        self.opt.step()

    def parts(self):
        """{part: ms} of one step."""
        torch.cuda.synchronize()
        L.profile_enable(True); L.profile_read()
        self.step()
        torch.cuda.synchronize()
        prof = L.profile_read(); L.profile_enable(False)
        out = {'sweeps fwd': prof['gru_fwd_sweep'][0], 'sweeps bwd': prof['gru_bwd_sweep'][0],
               'contractions': sum(prof[k][0] for k in ('gemm_nt', 'gemm_nn', 'gemm_tn'))}
        m = self.model
        if m.bidirectional:
            _, _, _, lengths, seq, att = m._saved
            P = m._params
            Wa, ba = P['attention_layer.0.weight'], P['attention_layer.0.bias']
            K = 2 * m.rnn_layers
            h_n = torch.randn(K, seq.shape[0], m.hidden_dims, device=m.device)
            dctx = torch.randn(seq.shape[0], m.hidden_dims, device=m.device)
            dWa, dba = torch.empty_like(Wa.data), torch.empty_like(ba.data)
            for what, fn in (('attention fwd', lambda: L.attn_fwd(seq, h_n, Wa.data, ba.data)),
                             ('attention bwd', lambda: L.attn_bwd(dctx, seq, Wa.data, att, K, dWa, dba))):
                fn(); ts = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                out[what] = statistics.median(ts)          # (attn_bwd's call allocates dout: the allocator's cached block, no device call)
        return out


def main():
    runs = int(os.environ.get('RUNS', 9))
    sides = [Side(n) for n in os.environ.get('SIDES', 'uni,bi,bi512').split(',')]
    for s in sides:
        s.step(); s.step()
        torch.cuda.synchronize()
        s.model.check_health()
    for r in range(runs):
        for s in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.step()
            torch.cuda.synchronize()
            s.times.append((time.perf_counter() - t0) * 1e3)
        print(f'round {r}: ' + '  '.join(f'{s.name} {s.times[-1]:.3f} ms' for s in sides), flush=True)
    print(f'audio classifier train step (dropout 0.5, AdamW), {runs} alternated rounds; GEMM mode {L.get_gemm_mode()}')
    for s in sides:
        t = s.times
        s.model.check_health()
        print(f'{s.name:6s} (B, T, F, H) = {s.shape}: median {statistics.median(t):.3f} ms  min {min(t):.3f}  max {max(t):.3f}  '
              f'(max - min {max(t) - min(t):.3f})')
    for s in sides:
        print(f'{s.name:6s} parts of one step: ' + ', '.join(f'{k} {v:.3f} ms' for k, v in s.parts().items()))


if __name__ == '__main__':
    main()
