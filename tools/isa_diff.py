#!/usr/bin/env python3
"""Per-kernel gfx950 ISA of one csrc file, at a git revision against the work tree.

    tools/isa_diff.py rnn_cluster_lstm [REV] [--map 'old substring=new substring' ...] [--old-stem STEM [--only SUBSTRING]]

Both sides compile with build_ext.FLAGS + --cuda-device-only -S in a temporary directory, each with the headers of its own side.
Per kernel pair: `identical`, or the first differing lines; plus VGPRs, SGPRs, spills, LDS, scratch and kernarg size.  Own symbol,
.LBB<n>_ function index and __hip_cuid_* are normalised, comments dropped.  --map renames a (demangled) revision-side kernel before pairing.
--old-stem: the revision side is csrc/<STEM>.hip (a kernel that moved between files); --only keeps the kernels whose name has SUBSTRING.
"""
import argparse, difflib, os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'icassp2022-depression_amd'
sys.path.insert(0, os.path.join(ROOT, PKG))
from build_ext import FLAGS
CXXFILT = next(f for f in ('/opt/rocm/llvm/bin/llvm-cxxfilt', shutil.which('llvm-cxxfilt'), shutil.which('c++filt')) if f and os.path.exists(f))
RES = ['.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.group_segment_fixed_size', '.private_segment_fixed_size', '.kernarg_segment_size']


def kernels(tree, stem, tmp):
    """{demangled name: (normalised body lines, resource dict)} of csrc/<stem>.hip under tree"""
    out = os.path.join(tmp, 'k.s')
    subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + ['--cuda-device-only', '-S', '-I' + os.path.join(tree, 'include'),
                    os.path.join(tree, PKG, 'csrc', stem + '.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    syms = re.findall(r'^\s+\.amdhsa_kernel (\S+)$', text, re.M)
    names = dict(zip(syms, subprocess.run([CXXFILT] + syms, capture_output=True, text=True, check=True).stdout.split('\n')))
    meta = {m.group(2): m.group(1) for m in re.finditer(r'^  - \.agpr_count:.*?\n((?:    .*\n)*?    \.symbol:\s+(\S+)\.kd\n(?:    .*\n)*)', text, re.M)}
    res = {}
    for s in syms:
        body = re.search(r'^%s:.*?^\s+\.end_amdhsa_kernel$' % re.escape(s), text, re.M | re.S).group(0)
        body = re.sub(r'\.LBB\d+_', '.LBB_', body.replace(s, '<kernel>'))
        body = re.sub(r'[ \t]*;.*$', '', body, flags=re.M)      # comments: loop notes carry the un-normalised function index (BB<n>_<k>)
        body = [l for l in re.sub(r'__hip_cuid_\w+', '__hip_cuid', body).split('\n') if l.strip()]
        res[names[s]] = (body, {k: re.search(r'%s:\s+(\S+)' % re.escape(k), meta[s]).group(1) for k in RES})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('stem'); ap.add_argument('rev', nargs='?', default='HEAD'); ap.add_argument('--map', action='append', default=[])
    ap.add_argument('--old-stem'); ap.add_argument('--only', default='')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, 'old'); os.makedirs(old)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', a.rev, 'include', PKG + '/csrc'], capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', old], input=tar, check=True)
        ko, kn = kernels(old, a.old_stem or a.stem, tmp), kernels(ROOT, a.stem, tmp)
        ko, kn = ({k: v for k, v in d.items() if a.only in k} for d in (ko, kn))
    print(f'# {a.old_stem or a.stem}.hip at {a.rev} -> {a.stem}.hip in the work tree' if a.old_stem else f'# {a.stem}.hip: {a.rev} -> work tree    ({" ".join(FLAGS)} --cuda-device-only -S)' + ''.join(f'\n# --map {m!r}' for m in a.map))
    for name, (body, r) in ko.items():
        new = name
        for m in a.map:
            new = new.replace(*m.split('=', 1))
        if new not in kn:
            print(f'{name}\n  -> {new}: NOT IN THE WORK TREE'); continue
        nbody, nr = kn.pop(new)
        d = [l for l in difflib.unified_diff(body, nbody, lineterm='', n=0) if l[:3] not in ('---', '+++')]
        print(name + (f'\n  -> {new}' if new != name else ''))
        print('  ' + ('identical' if not d else f'DIFFERENT ({len(body)} -> {len(nbody)} lines); first differing lines:\n    ' + '\n    '.join(d[:12])))
        print('  ' + '  '.join(f'{k[1:]} {r[k]}' + ('' if nr[k] == r[k] else f' -> {nr[k]}') for k in RES))
    for name in kn:
        print(f'{name}\n  ONLY IN THE WORK TREE')


if __name__ == '__main__':
    main()
