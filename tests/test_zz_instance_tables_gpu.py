"""The closing check of the sweep parity (the file name sorts it behind every other test file): every row of the cluster families'
instance tables -- dep_instance_table_read(), the rows an environment switch selects included -- was launched by an oracle-comparing
test of this session.

"Launched" = the row is in the session's record of what the `oracle`-marked tests launched (conftest.py, in-process) or what the child
processes of tests/test_switch_forms_gpu.py reported for the cases those tests compared (they add it under their own node id).  A new
table row without such a test fails here; a row no call can reach is to be deleted from its table, not exempted.
"""
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# rows that may stay unlaunched, each with its reason.  Empty: every row is reachable and tested.
EXEMPT = {}

# the test files that launch the tables' rows between them: the check means something only when all of them ran
SUITES = ('test_kernels_gpu', 'test_varlen_gpu', 'test_stack_depth_gpu', 'test_state_cluster_gpu', 'test_switch_forms_gpu')


def test_every_row_of_the_instance_tables_is_oracle_tested(request):
    from icassp2022_depression_amd import _lib as L
    rec = request.config._dep_instances
    absent = [s for s in SUITES if not any(s in k for k in rec)]
    if absent:
        pytest.skip('needs the whole GPU suite in one session; no oracle test of ' + ', '.join(absent) + ' ran')
    rows = L.instance_table_read()
    assert len(rows) == len(set(rows)) and len(rows) >= 80
    tested = set()
    for v in rec.values():
        tested |= v
    for r in rows:                                  # (shown with -s: a row and the first test that launched it, the parity suites' first)
        by = [k for k, v in rec.items() if r in v]
        print('instance-table %s: %s' % (r, next((k for k in by if any(s in k for s in SUITES)), by[0] if by else 'NOT LAUNCHED')))
    missing = sorted(set(rows) - tested - set(EXEMPT))
    assert not missing, 'rows of the instance tables that no oracle-comparing test of this session launched:\n  ' + '\n  '.join(missing)
    stale = sorted(set(EXEMPT) - set(rows))
    assert not stale, stale
