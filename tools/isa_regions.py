#!/usr/bin/env python3
"""Static instruction counts of the marked regions of one csrc file's gfx950 kernels.

    tools/isa_regions.py rnn_fused2 [--tree DIR] [--only SUBSTRING]

The source marks a block with a pair of assembler comments that survive into the -S output,
    asm volatile("; DEP_REGION gate begin");  ...  asm volatile("; DEP_REGION gate end");
and this tool compiles csrc/<stem>.hip device-only (build_ext.FLAGS + --cuda-device-only -S, no GPU needed) and counts, per kernel and
region, the instructions between a `begin` and the next `end` of the same name in the order of the assembly text.  A region the compiler
emitted more than once (two instantiations of a loop body, a duplicated tail) is listed once per occurrence (#1, #2, ...).  The counts are
STATIC: both arms of a branch inside a region are counted, and a block the compiler moved out of line is not.

Instructions are classified by mnemonic prefix alone:
  mfma     v_mfma*                       qVALU  the quarter-rate ops: transcendentals (v_exp, v_log, v_rcp, v_rsq, v_sqrt, v_sin, v_cos) and
                                                the 32-bit integer multiplies (v_mul_lo_u32, v_mul_hi_u32 / _i32, v_mad_u64_u32, v_mad_i64_i32)
  rdlane   v_readlane*, v_readfirstlane* VALU   every other v_* (rdlane and qVALU are listed beside it, not inside it)
  LDS      ds_*                          VMEM   buffer_*, global_*, flat_*, scratch_*
  branch   s_branch, s_cbranch*          SMEM   s_load*, s_buffer_load*
  sync     s_waitcnt*, s_barrier, s_nop, s_sleep, s_setprio, s_endpgm       SALU   every other s_*
--tree: the repository tree to compile (default: this one), e.g. an unpacked `git archive` of another revision.
"""
import argparse, os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'icassp2022-depression_amd'
sys.path.insert(0, os.path.join(ROOT, PKG))
from build_ext import FLAGS
CXXFILT = next(f for f in ('/opt/rocm/llvm/bin/llvm-cxxfilt', shutil.which('llvm-cxxfilt'), shutil.which('c++filt')) if f and os.path.exists(f))
CLASSES = ['total', 'VALU', 'qVALU', 'rdlane', 'mfma', 'SALU', 'SMEM', 'LDS', 'VMEM', 'branch', 'sync']
QUARTER = ('v_exp', 'v_log', 'v_rcp', 'v_rsq', 'v_sqrt', 'v_sin', 'v_cos', 'v_mul_lo_u32', 'v_mul_hi_u32', 'v_mul_hi_i32', 'v_mad_u64_u32', 'v_mad_i64_i32')
SYNC = ('s_waitcnt', 's_barrier', 's_nop', 's_sleep', 's_setprio', 's_endpgm')
MARK = re.compile(r';\s*DEP_REGION\s+(\S+)\s+(begin|end)')


def classify(m):
    if m.startswith('v_mfma'): return 'mfma'
    if m.startswith(('v_readlane', 'v_readfirstlane')): return 'rdlane'
    if m.startswith(QUARTER): return 'qVALU'
    if m.startswith('v_'): return 'VALU'
    if m.startswith('ds_'): return 'LDS'
    if m.startswith(('buffer_', 'global_', 'flat_', 'scratch_')): return 'VMEM'
    if m.startswith(('s_branch', 's_cbranch')): return 'branch'
    if m.startswith(('s_load', 's_buffer_load')): return 'SMEM'
    if m.startswith(SYNC): return 'sync'
    if m.startswith('s_'): return 'SALU'
    return None


def assembly(tree, stem, tmp):
    out = os.path.join(tmp, 'k.s')
    subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + ['--cuda-device-only', '-S', '-I' + os.path.join(tree, 'include'),
                    os.path.join(tree, PKG, 'csrc', stem + '.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def regions(text, only=''):
    """[(kernel, region, occurrence, {class: count})] and per kernel the code size in bytes, in the order of the assembly"""
    syms = re.findall(r'^\s+\.amdhsa_kernel (\S+)$', text, re.M)
    names = dict(zip(syms, subprocess.run([CXXFILT] + syms, capture_output=True, text=True, check=True).stdout.split('\n')))
    rows = []
    for s in syms:
        if only not in names[s]:
            continue
        body = re.search(r'^%s:.*?^\s+\.end_amdhsa_kernel$' % re.escape(s), text, re.M | re.S).group(0)
        size = re.search(r'^; codeLenInByte = (\d+)', text[text.index(body) + len(body):], re.M)      # (the first one behind the kernel's descriptor)
        open_, seen = {}, {}
        whole = dict.fromkeys(CLASSES, 0)
        for line in body.split('\n'):
            m = MARK.search(line)
            if m:
                name, edge = m.groups()
                if edge == 'begin':
                    open_[name] = dict.fromkeys(CLASSES, 0)
                elif name in open_:
                    seen[name] = seen.get(name, 0) + 1
                    rows.append((names[s], name, seen[name], open_.pop(name)))
                continue
            code = line.split(';')[0].strip()
            if not code or code.startswith('.') or code.endswith(':'):
                continue
            k = classify(code.split()[0])
            if k is None:
                continue
            for c in list(open_.values()) + [whole]:
                c['total'] += 1; c[k] += 1
        whole['bytes'] = int(size.group(1)) if size else 0
        rows.append((names[s], '(whole kernel)', 1, whole))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('stem'); ap.add_argument('--tree', default=ROOT); ap.add_argument('--only', default='')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        rows = regions(assembly(a.tree, a.stem, tmp), a.only)
    print(f'# {a.stem}.hip    ({" ".join(FLAGS)} --cuda-device-only -S)')
    print('%-26s' % 'region' + ''.join('%7s' % c for c in CLASSES) + '   code bytes')
    last = None
    for kernel, name, occ, c in rows:
        if kernel != last:
            print(kernel); last = kernel
        print('  %-24s' % (name + (' #%d' % occ if name[0] != '(' else '')) + ''.join('%7d' % c[k] for k in CLASSES) + ('   %d' % c['bytes'] if 'bytes' in c else ''))


if __name__ == '__main__':
    main()
