"""Device-bit anchors of the criteria (NOT reference-derived fixtures: a self-regression record).

Feeds seeded pre-activations through nn.Output with a stand-in owner into every default criterion, the fusion loss in both variants, and
one weighted case per family (labels / weights host-resident and device-resident), and writes the sha256 of the loss value and of dLoss/dz
(both halves for the fusion loss) to tests/golden/criterion_bits_parent.json.  No model is involved: the bits depend on the head-loss and
reduce kernels only (the fusion loss: also on its two small GEMMs).  Recorded ONCE on an MI355X, in a checkout of commit 1b3067d -- the
last one whose criteria each wrote their call sequence out for themselves -- with this script copied into it:

    python tests/golden/make_criterion_bits.py [destination [commit, where the checkout is an export without its .git]]

tests/test_criterion_bits_gpu.py holds the one call path the criteria share now to these bits; never regenerate the file from a later
tree.  The arithmetic is deterministic on gfx950: one thread per row, one block for the reduce, fixed summation order."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HT, HA = 32, 16                                   # the fusion loss's text / audio feature widths
SHAPES = {'labels': [(129, 2), (5, 2)],           # 129 rows: two 128-thread blocks, the second with one row
          'values': [(129, 2), (5, 1)]}


class _Weight:
    requires_grad = True

    def __init__(self, data):
        self.data = data
        self._grad = None


class Owner:
    """What a criterion (and models.MyLoss) needs of the module behind it; backward is never run."""
    training = True

    def __init__(self, W=None):
        self._params = {'fc_final.0.weight': _Weight(W)}

    def backward(self, dz):
        raise AssertionError('not part of the record')

    def check_health(self):
        pass


def _criteria(nn, models):
    """[(name, family, make, target placement or None, weighted)]"""
    return [('ce', 'labels', nn.CrossEntropyLoss, None, False),
            ('l1', 'values', nn.L1Loss, None, False),
            ('smoothl1', 'values', nn.SmoothL1Loss, None, False),
            ('huber', 'values', nn.HuberLoss, None, False),
            ('mse', 'values', nn.MSELoss, None, False),
            ('fusion_clf', 'labels', lambda: models.MyLoss('clf'), None, False),
            ('fusion_reg', 'values', lambda: models.MyLoss('reg'), None, False),
            ('ce_options_host', 'labels', lambda: nn.CrossEntropyLoss(weight=[0.5, 2.0], label_smoothing=0.1), 'host', True),
            ('ce_options_device', 'labels', lambda: nn.CrossEntropyLoss(weight=[0.5, 2.0], label_smoothing=0.1), 'device', True),
            ('huber_quarter_weight_host', 'values', lambda: nn.HuberLoss(delta=0.25), 'host', True),
            ('huber_quarter_weight_device', 'values', lambda: nn.HuberLoss(delta=0.25), 'device', True)]


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()[:24]


def all_digests():
    """{case name: {'loss': sha256, 'dz': sha256} or {'loss', 'dz_text', 'dz_audio'}} of every case, on cuda:0."""
    import torch
    from icassp2022_depression_amd import models, nn
    dev = torch.device('cuda', 0)
    rec = {}
    for name, family, make, where, weighted in _criteria(nn, models):
        for B, Cc in SHAPES[family]:
            rng = np.random.default_rng(1000 * B + Cc)
            crit = make()
            if family == 'labels':
                y = rng.integers(0, Cc, B)
                if weighted:
                    y[B // 2] = -100                                              # an ignored row
                target = torch.from_numpy(y)
            else:
                target = torch.from_numpy(rng.uniform(-0.5, 2.0, (B, Cc)).astype(np.float32))
            kw = {}
            if weighted and family == 'values':
                w = rng.uniform(0.2, 3.0, B).astype(np.float32); w[B // 2] = 0.0
                kw['weight'] = torch.from_numpy(w).to(dev) if where == 'device' else w
            elif where == 'device':
                target = target.to(dev)
            if name.startswith('fusion'):
                W = torch.from_numpy(rng.standard_normal((Cc, HT + HA)).astype(np.float32)).to(dev)
                tf = torch.from_numpy(rng.standard_normal((B, HT)).astype(np.float32)).to(dev)
                af = torch.from_numpy(rng.standard_normal((B, HA)).astype(np.float32)).to(dev)
                loss = crit(tf, af, target, Owner(W))
                got = {'loss': _sha(loss._v), 'dz_text': _sha(loss.dz_halves[0]), 'dz_audio': _sha(loss.dz_halves[1])}
            else:
                z = torch.from_numpy((rng.standard_normal((B, Cc)) * 1.5).astype(np.float32)).to(dev)
                loss = crit(nn.Output(z.clone(), Owner(), z), target, **kw)
                got = {'loss': _sha(loss._v), 'dz': _sha(loss.dz)}
            assert np.isfinite(float(loss._v.item())), name
            rec['%s_%dx%d' % (name, B, Cc)] = got
    return rec


if __name__ == '__main__':
    commit = sys.argv[2] if len(sys.argv) > 2 else \
        subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    rec = all_digests()
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'criterion_bits_parent.json')
    json.dump({'commit': commit, 'cases': rec}, open(dst, 'w'), indent=1, sort_keys=True)
    print('wrote', dst, len(rec), 'cases')
