"""Did the default K1 instantiation change between two commits?  (round-3 verdict W4: 0.832 -> 0.808 of peak with one more
kernel argument.)  CPU box only (needs .git and hipcc):  python tools/k1_isa_diff.py f302264 HEAD
Compiles nemoflux_amd/csrc/nf_flux.hip of both commits to gfx950 assembly with the product's flags, extracts
nf::k_flux<double, 2, 10, true, 256, 1, 0> and compares instruction stream, register counts and kernel descriptor.

Any other kernels:  python tools/k1_isa_diff.py A B nf_integral.hip _ZN2nf  compares every kernel of that file of csrc/
whose mangled name begins with the prefix (the K3 stage-A kernels, k_tracer_flux).  `.` as a commit is the working tree."""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

FLAGS = ['-O3', '--offload-arch=gfx950', '-fPIC', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only']
PREFIX = '_ZN2nf6k_fluxIdLi2ELi10ELb1ELi256ELi1ELi0E'     # nf::k_flux<double, 2, 10, true, 256, 1, 0>
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def asm_of(commit, tmp, src):
    d = os.path.join(tmp, 'worktree' if commit == '.' else commit.replace('/', '_'))
    csrc = 'nemoflux_amd/csrc/'
    # every header of csrc/ that exists at the commit being built
    names = os.listdir(os.path.join(ROOT, csrc)) if commit == '.' else subprocess.check_output(
        ['git', '-C', ROOT, 'ls-tree', '--name-only', f'{commit}:{csrc[:-1]}'], text=True).split()
    for rel in [csrc + src, 'include/nemoflux_amd.h'] + [csrc + h for h in sorted(names) if h.endswith('.h')]:
        os.makedirs(os.path.dirname(os.path.join(d, rel)), exist_ok=True)
        with open(os.path.join(d, rel), 'wb') as f:
            f.write(open(os.path.join(ROOT, rel), 'rb').read() if commit == '.' else
                    subprocess.check_output(['git', '-C', ROOT, 'show', f'{commit}:{rel}']))
    out = os.path.join(d, src + '.s')
    subprocess.check_call(['/opt/rocm/bin/hipcc'] + FLAGS + ['-o', out, src], cwd=os.path.join(d, 'nemoflux_amd/csrc'),
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_names(txt, prefix):
    return [n for n in re.findall(r'^\s*\.amdhsa_kernel (\S+)', txt, re.M) if n.startswith(prefix)]


def kernel(txt, name):
    body = re.search(r'^' + re.escape(name) + r':[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M).group(1)
    ins = [re.sub(r'\s*;.*$', '', l.strip()) for l in body.splitlines()
           if l.strip() and not l.strip().startswith((';', '.', '//'))]
    desc = dict(re.findall(r'\.amdhsa_(\w+) (\S+)', re.search(r'\.amdhsa_kernel ' + re.escape(name) + r'\n(.*?)\.end_amdhsa_kernel',
                                                                txt, re.S).group(1)))
    regs = {k: int(re.search(re.escape(name) + r'\.' + k + r', (\d+)', txt).group(1)) for k in ('num_vgpr', 'num_agpr', 'numbered_sgpr')}
    return name, ins, desc, regs


def opcode_counts(ins):
    c = Counter(i.split()[0] for i in ins)
    group = lambda *pre: sum(n for op, n in c.items() if op.startswith(pre))
    return (f'global_load {group("global_load")} (dwordx4 {c["global_load_dwordx4"]}), global_store {group("global_store")} '
            f'(dwordx4 {c["global_store_dwordx4"]}, dwordx2 {c["global_store_dwordx2"]}), ds_bpermute {group("ds_bpermute")}, '
            f'dpp moves {sum(1 for i in ins if "_dpp" in i.split()[0])}, v_add_f64 {group("v_add_f64")}, '
            f'v_fma_f64 {group("v_fma_f64")}, v_fmac_f64 {group("v_fmac_f64")}, v_mul_f64 {group("v_mul_f64")}, s_waitcnt {c["s_waitcnt"]}')


def compare(a, b, ka, kb):
    for tag, (name, ins, desc, regs) in ((a, ka), (b, kb)):
        print(f'{tag}: {name}')
        print(f'   {len(ins)} instructions, {regs}, kernarg {desc.get("kernarg_size")} B, scratch {desc.get("private_segment_fixed_size")}, '
              f'static LDS {desc.get("group_segment_fixed_size")}, {opcode_counts(ins)}')
    strip = lambda ins: [re.sub(r'\.LBB\d+_', '.LBB_', i) for i in ins]      # labels are numbered per function in the file
    sa, sb = strip(ka[1]), strip(kb[1])
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(sa, sb)) if x != y]
    print(f'instruction-by-instruction (registers included, labels renumbered): {len(diff)} of {len(sa)} differ' +
          (', lengths differ' if len(sa) != len(sb) else ''))
    for i, x, y in diff[:20]:
        print(f'   [{i}]  {a}: {x}    {b}: {y}')
    dd = {k: (ka[2].get(k), kb[2].get(k)) for k in sorted(set(ka[2]) | set(kb[2])) if ka[2].get(k) != kb[2].get(k)}
    print('kernel descriptor fields that differ:', dd or 'none')


def main(a, b, src='nf_flux.hip', prefix=PREFIX):
    with tempfile.TemporaryDirectory() as tmp:
        ta, tb = asm_of(a, tmp, src), asm_of(b, tmp, src)
    names = kernel_names(ta, prefix)
    for name in names:
        if name not in kernel_names(tb, prefix):
            print(f'{name}: not in {b} (signature changed?)')
            continue
        compare(a, b, kernel(ta, name), kernel(tb, name))
    for name in kernel_names(tb, prefix):
        if name not in names:
            print(f'{name}: not in {a}')


if __name__ == '__main__':
    main(*(sys.argv[1:5] if len(sys.argv) >= 3 else ('f302264', 'HEAD')))
