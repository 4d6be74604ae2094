"""The criteria write the bits they wrote before they shared one call path: sha256 of the loss value and of dLoss/dz of every default
criterion, of the fusion loss in both variants and of one weighted case per family (labels / weights on the host and on the device), at
129 x 2 (two blocks, a one-row tail) and 5 x 1 / 5 x 2, against tests/golden/criterion_bits_parent.json -- recorded on an MI355X at commit
1b3067d by tests/golden/make_criterion_bits.py.  The 'old path' comparisons of tests/test_weighted_loss_gpu.py and
tests/test_reg_loss_gpu.py run the same code on both sides now; this record does not."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_criteria_reproduce_the_recorded_device_bits():
    spec = importlib.util.spec_from_file_location('make_criterion_bits', os.path.join(GOLDEN, 'make_criterion_bits.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    rec = json.load(open(os.path.join(GOLDEN, 'criterion_bits_parent.json')))
    assert rec['commit'] == '1b3067d' and len(rec['cases']) == 22
    got = make.all_digests()
    assert sorted(got) == sorted(rec['cases'])
    bad = {k: (got[k], rec['cases'][k]) for k in got if got[k] != rec['cases'][k]}
    assert not bad, bad
