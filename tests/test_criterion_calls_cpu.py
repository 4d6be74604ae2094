"""Every criterion call enqueues what it enqueued before the criteria shared one call path: the launches, their arguments, their buffers
and the denominator of tests/golden/criterion_calls_parent.json (recorded at commit 1b3067d by tests/golden/make_criterion_calls.py),
replayed on the CPU by tests/criterion_rec.py.  No GPU, nothing is launched."""
import json
import os

import pytest

import criterion_rec

torch = pytest.importorskip('torch')

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'criterion_calls_parent.json')))
CASES = criterion_rec.cases()


def test_the_record_is_the_parents_and_covers_the_cases():
    assert GOLDEN['commit'] == '1b3067d'
    assert sorted(GOLDEN['cases']) == sorted(c[0] for c in CASES)
    want = {name: GOLDEN['traces'][i] for name, i in GOLDEN['cases'].items()}
    # the record holds what the issue's rule says, not only something: spot checks by hand
    t = want['ce/i64_tensor/train/nothing']
    assert [c[0] for c in t['calls']] == ['head_loss', 'reduce_loss', 'owner.backward'] and t['calls'][0][1] == 0x100 and t['calls'][0][7] == (5.0).hex()
    assert want['ce/list/train/accumulated_count']['calls'][0][7] == (12.0).hex()
    assert want['ce_weight/list/train/two_ranks_nothing'] == {'raises': 'DepError', 'calls': [], 'tensors': {}}
    assert want['mse_weight/f32_tensor/train/two_ranks_nothing']['raises'] == 'DepError'
    quirk = want['mse/f32_tensor/train/two_ranks_nothing']                        # unweighted MSE on two ranks: not refused, the local count
    assert 'raises' not in quirk and quirk['calls'][0][0] == 'head_loss_reg' and quirk['calls'][0][9] == (5.0).hex() and quirk['loss']['reduce']
    assert want['mse/f32_tensor/train/accumulated_weight']['calls'][0][9] == (7.5).hex()   # ... and a declared weight comes first
    assert want['ce_all_ignored/list/eval/nothing']['calls'][0][7][0] == 'device'
    assert [c[0] for c in want['ce_all_ignored/list/eval/nothing']['calls']] == ['head_loss_ce', 'reduce_loss_by']
    assert [c[0] for c in want['fusion_reg_l1/f32_tensor/eval/nothing']['calls']] == ['gemm', 'gemm', 'head_loss_reg', 'reduce_loss'] + ['head_loss_reg', 'reduce_loss']


@pytest.mark.parametrize('criterion', sorted({c[1][0] for c in CASES}))
def test_criterion_calls_are_the_recorded_ones(criterion):
    for case in CASES:
        if case[1][0] != criterion:
            continue
        got = json.loads(json.dumps(criterion_rec.record(case)))                   # tuples and lists, as the file spells them
        want = GOLDEN['traces'][GOLDEN['cases'][case[0]]]
        assert got == want, '%s:\n got  %s\n want %s' % (case[0], json.dumps(got, sort_keys=True), json.dumps(want, sort_keys=True))


def test_reduce_loss_takes_a_number_or_a_device_scalar(monkeypatch):
    """L.reduce_loss hands a 1-element tensor on to dep_reduce_loss_by before anything touches the library."""
    from icassp2022_depression_amd import _lib as L
    seen = []
    monkeypatch.setattr(L, 'reduce_loss_by', lambda rows, norm, out, accumulate=False: seen.append((rows, norm, out, accumulate)))
    rows, norm, out = torch.zeros(5), torch.full((1,), 2.0), torch.zeros(1)
    L.reduce_loss(rows, norm, out)
    L.reduce_loss(rows, norm, out, True)
    assert [(a is rows, b is norm, c is out, d) for a, b, c, d in seen] == [(True, True, True, False), (True, True, True, True)]
