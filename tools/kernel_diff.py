#!/usr/bin/env python3
"""Did a refactor move a kernel?  Compares the gfx950 instruction streams of two builds, kernel by kernel (no GPU):
    python tools/kernel_diff.py OLD NEW [--ignore ', false'] [--filter attention16]
OLD / NEW: two objects (csrc/*.o) or two assembly files (hipcc -S ... --cuda-device-only).  Per kernel of NEW: the instruction count and
SAME, DIFF(n) with the differing lines, or NEW; kernels only OLD has are listed as GONE.  A branch is compared by its kind, not its label.
--ignore S: S is dropped from the end of NEW's template-argument lists before pairing, so that a kernel that gained a defaulted template
parameter meets its predecessor (attention16_kernel<T, 64, 1, 64, true, false, false, false> against <.., true, false, false>)."""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusion_tts_amd import build

CXXFILT = shutil.which('llvm-cxxfilt', path=os.path.dirname(build.OBJDUMP)) or shutil.which('c++filt')     # none: mangled names


def kernels(path):
    """{demangled name without its argument list: [instruction, ...]}"""
    if path.endswith('.s'):
        text = open(path).read()
        head, end = re.compile(r'^(\w+):'), re.compile(r'^\.Lfunc_end')
    else:
        with tempfile.TemporaryDirectory() as tmp:
            text = subprocess.run([build.OBJDUMP, '-d', build._device_object(path, tmp)], capture_output=True, text=True, check=True).stdout
        head, end = re.compile(r'^[0-9a-f]+ <(\w+)>:'), re.compile(r'^$')
    out, cur = {}, None
    for ln in text.splitlines():
        m = head.match(ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif end.match(ln):
            cur = None
        elif cur is not None:
            code = re.split(r'//|;', ln)[0].strip()
            if code and not code.startswith('.') and not code.endswith(':'):
                cur.append(re.sub(r'^(s_c?branch\w*) \S+$', r'\1', code))                    # a branch keeps its kind, not its label / offset
    names = subprocess.run([CXXFILT], input='\n'.join(out), capture_output=True, text=True).stdout.split('\n') if CXXFILT else list(out)
    return {n.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0]: ins for n, ins in zip(names, out.values()) if 's_endpgm' in ins}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--ignore', default='', help="template-argument suffix of NEW's names to drop before pairing, e.g. ', false'")
    ap.add_argument('--filter', default='', help='only kernels whose name contains this')
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    seen = set()
    for name, ins in sorted(new.items()):
        key = name[:-len(a.ignore) - 1] + '>' if a.ignore and name.endswith(a.ignore + '>') and name not in old else name
        if a.filter not in name:
            continue
        seen.add(key)
        if key not in old:
            print(f'{len(ins):6d}  NEW      {name}')
            continue
        delta = [d for d in difflib.unified_diff(old[key], ins, lineterm='', n=0) if d[0] in '+-' and d[:3] not in ('+++', '---')]
        print(f'{len(ins):6d}  {"SAME    " if not delta else "DIFF(%d)" % max(sum(d[0] == "-" for d in delta), sum(d[0] == "+" for d in delta)):8s} {name}')
        for d in delta[:8]:
            print(' ' * 18 + d)
    for name in sorted(set(old) - seen):
        if a.filter in name:
            print(f'{len(old[name]):6d}  GONE     {name}')


if __name__ == '__main__':
    main()
