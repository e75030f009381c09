#!/usr/bin/env python
"""Per-kernel register / spill / LDS figures of the BUILT engine library, read from the AMDGPU code-object metadata inside it
(no recompilation): the gfx950 ELF images are cut out of the .hip_fatbin section and their NT_AMDGPU_METADATA note is printed by
llvm-readelf.   python tools/isa_report.py [path/to/libefe_mi355x.so]
                python tools/isa_report.py --diff OLD.so NEW.so      (per kernel: identical listing, the same instruction sequence, or what differs)"""
import collections, os, re, struct, subprocess, sys, tempfile

LLVM = '/opt/rocm/lib/llvm/bin'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, 'deep-active-inference-mc_amd', 'libefe_mi355x.so')
FIELDS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size',
          '.group_segment_fixed_size', '.max_flat_workgroup_size')


def code_objects(lib):
    """the EM_AMDGPU ELF images embedded in the library"""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fat.bin')
        subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', f'.hip_fatbin={fat}', lib, os.path.join(tmp, 'discard')])
        data = open(fat, 'rb').read()
    out = []
    for m in re.finditer(b'\x7fELF', data):
        o = m.start()
        hdr = data[o:o + 64]
        if len(hdr) < 64 or hdr[4] != 2 or struct.unpack_from('<H', hdr, 0x12)[0] != 224:       # ELF64, EM_AMDGPU
            continue
        e_shoff = struct.unpack_from('<Q', hdr, 0x28)[0]
        e_shentsize, e_shnum = struct.unpack_from('<HH', hdr, 0x3A)
        out.append(data[o:o + e_shoff + e_shentsize * e_shnum])
    return out


def demangle(names):
    try:
        p = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
        return p.stdout.splitlines() if p.returncode == 0 and p.stdout else names
    except OSError:
        return names


def kernels(lib=DEFAULT_LIB):
    """{demangled kernel name (arguments stripped): {field: int}}"""
    res = {}
    for img in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix='.elf') as f:
            f.write(img); f.flush()
            txt = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', f.name], capture_output=True, text=True).stdout
        for blk in re.split(r'\n  - \.agpr_count:', txt)[1:]:
            blk = '.agpr_count:' + blk
            name = re.search(r'\n\s+\.name:\s+(\S+)', blk)
            if not name:
                continue
            vals = {}
            for k in FIELDS:
                mm = re.search(r'(?:^|\n)\s*' + re.escape(k) + r':\s+(\d+)', blk)
                if mm:
                    vals[k] = int(mm.group(1))
            res[name.group(1)] = vals
    names = list(res)
    pretty = [re.sub(r'\(.*$', '', d).replace('efe::', '').replace('void ', '') for d in demangle(names)]
    return {p: res[n] for p, n in zip(pretty, names)}


def disassembly(lib=DEFAULT_LIB):
    """{demangled kernel name (arguments stripped): the instructions of its llvm-objdump listing, one per line}"""
    res = {}
    for img in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix='.elf') as f:
            f.write(img); f.flush()
            txt = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', f.name], capture_output=True, text=True).stdout
        for m in re.finditer(r'^[0-9a-f]+ <([^>\n]+)>:\n(.*?)(?=^[0-9a-f]+ <[^>\n]+>:\n|\Z)', txt, re.M | re.S):
            if not m.group(1).startswith('L'):            # (local labels of a kernel stay in its text)
                res[m.group(1)] = res.get(m.group(1), '') + m.group(2)
    names = list(res)
    pretty = [re.sub(r'\(.*$', '', d).replace('efe::', '').replace('void ', '') for d in demangle(names)]
    return {p: res[n] for p, n in zip(pretty, names)}


def listing(text):
    """the instructions of a kernel's listing with everything that depends on where the code sits taken out: addresses, encodings and
    the symbol + offset form of branch targets (all in the trailing comment; the operand itself is a relative distance), label lines"""
    out = []
    for line in text.splitlines():
        line = re.sub(r'\s+', ' ', line.split('//')[0]).strip()
        if line and not re.fullmatch(r'(?:[0-9a-f]+ )?<[^>]+>:', line):
            out.append(line)
    return out


def diff(old, new, out=sys.stdout):
    """per kernel of either library: 'identical' (same normalised listing and metadata); 'same instruction sequence' (equal metadata
    and the same mnemonic line for line: only operands differ); else the metadata fields (old -> new where they differ) and the
    per-mnemonic instruction counts that differ: a mnemonic that is not listed occurs equally often on both sides.
    -> number of kernels that are not identical"""
    ko, kn, do, dn = kernels(old), kernels(new), disassembly(old), disassembly(new)
    changed = 0
    for k in sorted(set(ko) | set(kn)):
        if k not in ko or k not in kn:
            out.write(f'{k}: only in {"NEW" if k in kn else "OLD"}\n')
            changed += 1
            continue
        lo, ln = listing(do.get(k, '')), listing(dn.get(k, ''))
        if lo == ln and ko[k] == kn[k]:
            out.write(f'{k}: identical ({len(lo)} instructions)\n')
            continue
        changed += 1
        if ko[k] == kn[k] and [i.split()[0] for i in lo] == [i.split()[0] for i in ln]:
            nd = sum(a != b for a, b in zip(lo, ln))
            out.write(f'{k}: same instruction sequence, {nd} of {len(lo)} lines differ in operands; metadata equal: '
                      + ', '.join(f'{f[1:]} {ko[k].get(f)}' for f in FIELDS) + '\n')
            continue
        meta = [f'{f[1:]} {ko[k].get(f)}' + ('' if ko[k].get(f) == kn[k].get(f) else f' -> {kn[k].get(f)}') for f in FIELDS]
        out.write(f'{k}: DIFFERS, {len(lo)} -> {len(ln)} instructions; metadata ' + ('equal' if ko[k] == kn[k] else 'DIFFERS') + ': ' + ', '.join(meta) + '\n')
        co, cn = (collections.Counter(i.split()[0] for i in l) for l in (lo, ln))
        for mn in sorted(set(co) | set(cn)):
            if co[mn] != cn[mn]:
                out.write(f'    {mn:40s} {co[mn]:6d} -> {cn[mn]:6d}\n')
        if co == cn:
            out.write('    (the same instructions in another order or with other operands)\n')
    out.write(f'{changed} of {len(set(ko) | set(kn))} kernels differ\n')
    return changed


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--diff':
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    ks = kernels(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB)
    print(f'{"kernel":44s} {"vgpr":>5s} {"agpr":>5s} {"sgpr":>5s} {"vspill":>6s} {"sspill":>6s} {"scratch":>7s} {"lds":>7s} {"wg":>5s}')
    for k in sorted(ks):
        v = ks[k]
        print(f'{k[:44]:44s} ' + ' '.join(f'{v.get(f, -1):>{w}d}' for f, w in zip(FIELDS, (5, 5, 5, 6, 6, 7, 7, 5))))
