"""Compare the device code of two builds of one HIP object file, kernel by kernel, on a machine without a GPU.

    python tools/codeobj_diff.py PARENT.o NEW.o [--arch gfx950] [--llvm /opt/rocm/llvm/bin] [--list]

For each object: section .hip_fatbin is dumped (llvm-objcopy), the code object of ``hipv4-amdgcn-amd-amdhsa--ARCH`` is unbundled
(clang-offload-bundler) and its symbols, sections and notes are read (llvm-readelf).  A kernel is a function symbol with a ``.kd``
descriptor beside it.  Per kernel: its size, the sha256 of its bytes in .text, and its entry in the AMDGPU metadata note (register
counts, LDS = group_segment_fixed_size, scratch = private_segment_fixed_size, spill counts, arguments).  The tool hashes and
compares; it does not disassemble.  Kernel order and addresses may differ between the two objects.  A kernel that addresses a device
global (the time stamps of the diagnostic build) holds the distance to it in its code, which changes with the kernel order: such a
kernel counts as equal when size and metadata are equal and every differing 32-bit word changed by exactly the change of that
distance; the summary says how many there are.

Prints a summary line, the kernels only one object has, the kernels that differ (each with its old and new metadata figures), and with
``--list`` one line per common kernel that does not differ.
Exit status 0 when the two sets are equal and no kernel differs, else 1.  This is how a refactor of host code shows that it did
not reach device code (profiles/conv_plan_refactor.txt, profiles/conv_launch_refactor.txt)."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import textwrap

NOTE_KEYS = (('.vgpr_count', 'vgpr'), ('.agpr_count', 'agpr'), ('.sgpr_count', 'sgpr'), ('.group_segment_fixed_size', 'LDS'),
             ('.private_segment_fixed_size', 'scratch'), ('.vgpr_spill_count', 'vspill'), ('.sgpr_spill_count', 'sspill'))


def _run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def _kernel_notes(text):
    """{symbol without .kd: the text of its entry in amdhsa.kernels}."""
    out = {}
    m = re.search(r'^amdhsa\.kernels:\s*$', text, re.M)
    if not m:
        return out
    body = text[m.end():]
    end = re.search(r'^\S', body, re.M)                 # the next top-level key ends the list
    body = body[:end.start()] if end else body
    for block in re.split(r'^  - ', body, flags=re.M)[1:]:
        sym = re.search(r'^\s*\.symbol:\s*(\S+)\.kd\s*$', block, re.M)
        if sym:
            out[sym.group(1).strip("'\"")] = block
    return out


def kernels(obj, arch, llvm, tmp, tag):
    """{mangled kernel name: (size, sha256 of its bytes, metadata entry, demangled name)} of the ARCH code object inside ``obj``."""
    fatbin, co = os.path.join(tmp, tag + '.fatbin'), os.path.join(tmp, tag + '.co')
    _run(os.path.join(llvm, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fatbin, obj, os.path.join(tmp, tag + '.copy.o'))
    _run(os.path.join(llvm, 'clang-offload-bundler'), '--type=o', '--input=' + fatbin, '--targets=hipv4-amdgcn-amd-amdhsa--' + arch,
         '--output=' + co, '--unbundle')
    readelf = os.path.join(llvm, 'llvm-readelf')
    text_addr = text_off = None
    for line in _run(readelf, '-S', '-W', co).splitlines():
        m = re.match(r'\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
        if m:
            text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
    if text_addr is None:
        raise SystemExit(f'{obj}: no .text section in the {arch} code object')
    syms, pretty = {}, {}
    for line, demangled in zip(_run(readelf, '-s', '-W', co).splitlines(), _run(readelf, '-s', '-W', '-C', co).splitlines()):
        f = line.split()
        if len(f) == 8 and f[0].endswith(':') and f[3] in ('FUNC', 'OBJECT'):
            syms[f[7]] = (int(f[1], 16), int(f[2]), f[3])
            pretty[f[7]] = demangled.split(None, 7)[7].replace('(anonymous namespace)::', '').split('(')[0]     # without the parameter list
    notes = _kernel_notes(_run(readelf, '--notes', co))
    with open(co, 'rb') as fh:
        blob = fh.read()
    out, where = {}, {}
    for name, (value, size, kind) in syms.items():
        if kind != 'FUNC' or name + '.kd' not in syms:
            continue
        start = value - text_addr + text_off
        out[name] = (size, hashlib.sha256(blob[start:start + size]).hexdigest(), notes.get(name), pretty[name])
        where[name] = (value, blob[start:start + size])
    device_globals = {n: v[0] for n, v in syms.items() if v[2] == 'OBJECT' and not n.endswith('.kd')}
    return out, where, device_globals


def only_displacements_moved(name, old, new):
    """True when the two images of a kernel have one size and differ only in 32-bit words whose change is the change of the distance
    between the kernel and a device global both objects have: position-relative addresses of that global, which move when the
    kernels are laid out in another order.  (No decoding: words are compared as numbers.)"""
    (kaddr_old, code_old), globals_old = old[1][name], old[2]
    (kaddr_new, code_new), globals_new = new[1][name], new[2]
    if len(code_old) != len(code_new):
        return False
    moved = {((globals_new[g] - kaddr_new) - (globals_old[g] - kaddr_old)) & 0xffffffff for g in globals_old if g in globals_new}
    for i in range(0, len(code_old), 4):
        a, b = int.from_bytes(code_old[i:i + 4], 'little'), int.from_bytes(code_new[i:i + 4], 'little')
        if a != b and ((b - a) & 0xffffffff) not in moved:
            return False
    return True


def _note_fields(note):
    vals = []
    for key, _ in NOTE_KEYS:
        m = re.search(r'^\s*' + re.escape(key) + r':\s*(\S+)\s*$', note or '', re.M)
        vals.append(m.group(1) if m else '?')
    return vals


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent')
    ap.add_argument('new')
    ap.add_argument('--arch', default='gfx950')
    ap.add_argument('--llvm', default='/opt/rocm/llvm/bin')
    ap.add_argument('--list', action='store_true', help='one line per kernel that both objects have')
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old_all, new_all = kernels(a.parent, a.arch, a.llvm, tmp, 'parent'), kernels(a.new, a.arch, a.llvm, tmp, 'new')
    old, new = old_all[0], new_all[0]
    names = sorted(set(old) | set(new))
    pretty = {n: (old.get(n) or new.get(n))[3] for n in names}
    both = [n for n in names if n in old and n in new]
    missing_note = [n for n in names if (old.get(n) or new.get(n))[2] is None]
    differ = [n for n in both if old[n] != new[n]]
    # same size, same metadata, and every differing word is the displacement to a device global (diagnostic builds address some)
    moved = [n for n in differ if old[n][0] == new[n][0] and old[n][2] == new[n][2] and only_displacements_moved(n, old_all, new_all)]
    differ = [n for n in differ if n not in moved]
    print(f'kernel symbols: parent {len(old)}, new {len(new)}, in both {len(both)}; differing in size / code hash / metadata: {len(differ)}')
    if moved:
        print(textwrap.fill(f'of the kernels in both, {len(moved)} address a device global ({", ".join(sorted(set(old_all[2]) & set(new_all[2])))}) '
                            'and differ only in the words that hold its position-relative displacement (another kernel order moves it); all '
                            'other bytes, size and metadata equal', 128))
    for title, tree, other in (('symbols only in the parent:', old, new), ('symbols only in the new object:', new, old)):
        print(title)
        for n in names:
            if n in tree and n not in other:
                print(f'  {pretty[n]}   size {tree[n][0]}')
    if missing_note:
        print('kernels without a metadata entry:', ', '.join(pretty[n] for n in missing_note))
    for n in differ:
        what = [w for w, i in (('size', 0), ('code', 1), ('metadata', 2)) if old[n][i] != new[n][i]]
        print(f'DIFFERS ({", ".join(what)}): {pretty[n]}   size {old[n][0]} -> {new[n][0]}')
        print('    ' + '  '.join(f'{short} {o}' + ('' if o == v else f' -> {v}')
                                 for (_, short), o, v in zip(NOTE_KEYS, _note_fields(old[n][2]), _note_fields(new[n][2]))))
    if a.list:
        width = max([len(pretty[n]) for n in both] + [10])
        print()
        print(f'{"kernel (in both; size, sha256[:16] of its bytes, metadata equal)":<{width}} {"bytes":>6} {"sha256":<16} ' +
              ' '.join(f'{short:>5}' for _, short in NOTE_KEYS))
        for n in sorted(both, key=lambda n: pretty[n]):
            if n not in differ:
                print(f'{pretty[n]:<{width}} {new[n][0]:>6} {"(displacements)" if n in moved else new[n][1][:16]:<16} ' +
                      ' '.join(f'{v:>5}' for v in _note_fields(new[n][2])))
    return 0 if not differ and not missing_note and set(old) == set(new) else 1


if __name__ == '__main__':
    sys.exit(main())
