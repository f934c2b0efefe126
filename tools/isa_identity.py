#!/usr/bin/env python3
"""Per-symbol comparison of two device assembly files of one translation unit (a refactor's proof of "same device code").

  hipcc --offload-arch=gfx950 <the Makefile's flags for the unit> --cuda-device-only -S -o before.s unit.hip   (at the parent)
  hipcc ... -o after.s unit.hip                                                                              (at this commit)
  python tools/isa_identity.py before.s after.s

Each file is split at the function symbols ("name:  ; @name" .. ".Lfunc_endN:", which takes in the kernel's
.amdhsa_kernel descriptor: registers, spills, LDS).  Comments are stripped (they carry the function's index in the file)
and the function index in local labels is dropped (.LBB33_18 -> .LBB_18); everything else is compared as text, per
symbol.  Exit status 1 if the symbol sets differ or any symbol's text does.
"""
import re
import sys


def split(path):
    out = {}
    for m in re.finditer(r'^(_Z\w+):\s*;\s*@\1\n(.*?)^\.Lfunc_end\d+:', open(path).read(), re.S | re.M):
        lines = (re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r';.*', '', l).rstrip()) for l in m.group(2).splitlines())
        out[m.group(1)] = [l for l in lines if l]
    return out


def main():
    a, b = split(sys.argv[1]), split(sys.argv[2])
    diff = [k for k in a if k in b and a[k] != b[k]]
    print(f'symbols parent {len(a)} new {len(b)} same-set {set(a) == set(b)}; {sum(map(len, a.values()))} lines compared; '
          f'differing symbols {len(diff)}')
    for k in sorted(set(a) ^ set(b)):
        print('  only in', 'parent' if k in a else 'new', k)
    for k in diff:
        print(f'  differs ({len(a[k])} -> {len(b[k])} lines): {k}')
    return 1 if diff or set(a) != set(b) else 0


if __name__ == '__main__':
    sys.exit(main())
