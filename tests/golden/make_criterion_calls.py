"""Call-trace anchor of the criteria (NOT a reference-derived fixture: a self-regression record).

Writes tests/golden/criterion_calls_parent.json: for every case of tests/criterion_rec.py the launches a criterion call enqueues, with their
arguments, buffers and denominator, and what the returned Loss carries.  Recorded ONCE, in a checkout of commit 1b3067d -- the last one
whose criteria each wrote their call sequence out for themselves -- with this script and tests/criterion_rec.py copied into it:

    python tests/golden/make_criterion_calls.py [destination]

The refactoring that gave the criteria one call path has to reproduce it (tests/test_criterion_calls_cpu.py); never regenerate it from a
later tree.  Many cases share a trace (evaluate() does not look at what is declared), so the file holds each distinct trace once."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]


def pack(records):
    """{'traces': [distinct traces], 'cases': {case name: index}} of {case name: trace}."""
    traces, index, of = [], {}, {}
    for name, rec in records.items():
        key = json.dumps(rec, sort_keys=True)
        if key not in index:
            index[key] = len(traces)
            traces.append(rec)
        of[name] = index[key]
    return {'traces': traces, 'cases': of}


if __name__ == '__main__':
    import criterion_rec
    commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(['git', '-C', ROOT, 'status', '--porcelain', '--untracked-files=no'], capture_output=True, text=True, check=True).stdout.strip()
    doc = {'commit': commit + ('+modified' if dirty else '')}
    doc.update(pack(criterion_rec.record_all()))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'criterion_calls_parent.json')
    with open(dst, 'w') as f:
        one = lambda v: json.dumps(v, sort_keys=True, separators=(',', ':'))      # one case / one trace per line: a diff stays readable
        f.write('{"commit":%s,\n"cases":{\n%s\n},\n"traces":[\n%s\n]}\n' % (
            one(doc['commit']), ',\n'.join('%s:%d' % (one(k), v) for k, v in doc['cases'].items()), ',\n'.join(one(t) for t in doc['traces'])))
    print('wrote', dst, len(doc['cases']), 'cases,', len(doc['traces']), 'distinct traces, at', doc['commit'])
