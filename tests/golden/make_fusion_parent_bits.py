#!/usr/bin/env python3
"""Records what the default FusionNet (audio_bidirectional off, no lengths) is held to by tests/test_fusion_bi_cpu.py and
tests/test_fusion_bi_gpu.py.  Run ONCE in a checkout of the commit before the flag existed; needs no flag and no lengths, so it runs there as is:

    python tests/golden/make_fusion_parent_bits.py layout   -> fusion_layout_parent.json   names, shapes, flat offsets (no GPU: host buffers)
    python tests/golden/make_fusion_parent_bits.py bits     -> fusion_parent_bits.json     sha256 of text / audio features on an MI355X

The case is seeded end to end: model seed 11, inputs from numpy's default_rng(5), torch.manual_seed(0) and the dropout seed counter at 0
before the train-mode call (nn.next_dropout_seed is a function of those two)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SHAPE = dict(Ft=8, Ht=16, Lyr=2, p=0.5, Ha=16, Fa=8)            # the shape of the GPU file's cases
B, Ta, Tt = 3, 5, 4


def build(models, variant, seed=11, **kw):
    s = SHAPE
    return models.FusionNet(s['Ft'], s['Ht'], s['Lyr'], s['p'], 2 if variant == 'clf' else 1, s['Ha'], s['Fa'], variant=variant, seed=seed, **kw)


def layout(model):
    P = model._params
    return dict(names=list(P), shapes=[list(P[k].shape) for k in P], offsets=[int(P[k].offset) for k in P], live=[bool(P[k].live) for k in P],
                n_live=int(model._n_live), total=int(model._flat.numel()))


def feature_bits(models, nn, variant):
    """{mode: {text, audio: sha256}} of pretrained_feature on the seeded pair batch, eval and train."""
    rng = np.random.default_rng(5)
    xa = rng.standard_normal((B, Ta, SHAPE['Fa'])).astype(np.float32)
    xt = (rng.standard_normal((B, Tt, SHAPE['Ft'])) * 0.5).astype(np.float32)
    model = build(models, variant)
    out = {}
    for mode in ('eval', 'train'):
        model.train() if mode == 'train' else model.eval()
        torch.manual_seed(0); nn._seed_counter[0] = 0
        tf, af = model.pretrained_feature((torch.from_numpy(xa), torch.from_numpy(xt)))
        out[mode] = dict(text=hashlib.sha256(tf.cpu().numpy().tobytes()).hexdigest(), audio=hashlib.sha256(af.cpu().numpy().tobytes()).hexdigest())
    model.check_health()
    return out


def main():
    what = sys.argv[1]
    from icassp2022_depression_amd import models, nn
    if what == 'layout':
        nn._device = lambda: torch.device('cpu')
        rec = {v: layout(build(models, v)) for v in ('clf', 'reg')}
        dst = os.path.join(HERE, 'fusion_layout_parent.json')
    else:
        rec = {v: feature_bits(models, nn, v) for v in ('clf', 'reg')}
        dst = os.path.join(HERE, 'fusion_parent_bits.json')
    dst = sys.argv[2] if len(sys.argv) > 2 else dst
    json.dump(rec, open(dst, 'w'), indent=1)
    print('wrote', dst)


if __name__ == '__main__':
    main()
