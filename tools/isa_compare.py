"""Compare the gfx950 code of two builds of one library, kernel by kernel.

    python tools/isa_compare.py BEFORE.so AFTER.so [...more pairs] > profiles/common/isa_identical.txt

For each pair: the code object is taken out of both files (llvm-objdump
--offloading), disassembled (llvm-objdump -d) and split at the function
symbols; instruction addresses are dropped, encodings kept.  The resource
figures come from the code object's metadata note (llvm-readelf --notes).
Prints one line per kernel -- identical or DIFFERENT, then VGPR / AGPR / SGPR
counts, LDS and scratch bytes before -> after -- and one line for the device
functions that are no kernels.  Exit status 1 if anything differs.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
FIGURES = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
           '.kernarg_segment_size', '.max_flat_workgroup_size')


def code_object(lib, tmp):
    d = tempfile.mkdtemp(dir=tmp)
    local = os.path.join(d, 'lib.so')
    os.symlink(os.path.abspath(lib), local)
    subprocess.check_call([os.path.join(LLVM, 'llvm-objdump'), '--offloading', local], cwd=d, stdout=subprocess.DEVNULL)
    got = [f for f in os.listdir(d) if 'gfx950' in f]
    assert len(got) == 1, (lib, os.listdir(d))
    return os.path.join(d, got[0])


def functions(co):
    """{symbol: [instruction text + encoding, ...]}"""
    out = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', co], text=True)
    fns, cur = {}, None
    for line in out.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif cur is not None and '//' in line:
            text, _, tail = line.partition('//')
            cur.append(text.strip() + ' | ' + tail.split(':', 1)[1].strip())
    return fns


def figures(co):
    """{kernel: {figure: value}} from the NT_AMDGPU_METADATA note"""
    out = subprocess.check_output([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], text=True)
    res, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r'^  (- |  )(\.[a-z_]+):\s*(.*)$', line)   # a kernel's own keys; '- ' opens the next kernel
        if not m:
            continue
        if m.group(1) == '- ':
            cur = {}
        if m.group(2) == '.symbol':
            res[m.group(3).strip("'").removesuffix('.kd')] = cur
        elif m.group(2) in FIGURES:
            cur[m.group(2)] = m.group(3)
    return res


def demangle(name):
    return subprocess.check_output(['c++filt', name], text=True).strip().replace('(anonymous namespace)::', '')


def main(argv):
    assert len(argv) >= 2 and len(argv) % 2 == 0, __doc__
    bad = 0
    print('# per kernel: instructions and encodings compared; VGPR / AGPR / SGPR counts, group (LDS) and private\n'
          '# (scratch) bytes before->after.  A wave\'s occupancy follows from these figures.')
    with tempfile.TemporaryDirectory() as tmp:
        for before, after in zip(argv[::2], argv[1::2]):
            ca, cb = code_object(before, tmp), code_object(after, tmp)
            fa, fb, ga, gb = functions(ca), functions(cb), figures(ca), figures(cb)
            print('== %s -> %s: %d -> %d kernels' % (os.path.basename(before), os.path.basename(after), len(ga),
                                                     len(gb)))
            for k in sorted(set(ga) | set(gb)):
                same = k in fa and k in fb and fa[k] == fb[k] and ga.get(k) == gb.get(k)
                bad += not same
                fig = ' '.join('%s %s->%s' % (f[1:].replace('_count', '').replace('_segment_fixed_size', ''),
                                              ga.get(k, {}).get(f, '-'), gb.get(k, {}).get(f, '-'))
                               for f in FIGURES[:5])
                print('%-9s %5d insts  %s  %s' % ('identical' if same else 'DIFFERENT', len(fb.get(k, ())), fig,
                                                  demangle(k)))
            others = sorted((set(fa) | set(fb)) - set(ga) - set(gb))
            diff = [k for k in others if fa.get(k) != fb.get(k)]
            bad += len(diff)
            print('%-9s %d device functions that are no kernels%s' % ('DIFFERENT' if diff else 'identical', len(others),
                                                                      ': ' + ', '.join(diff) if diff else ''))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
