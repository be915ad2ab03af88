"""Are the kernels of two builds the same machine code?  profiles/sharded_metric.md uses it for "the non-EV kernels are unchanged".

    hipcc -c -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden --offload-arch=gfx950 -x hip --save-temps \\
          -Rpass-analysis=kernel-resource-usage gbp_poplar_amd/csrc/gbp_kernels.hip -o k.o          (once per tree, in a directory of its own)
    python profiles/isa_same.py OLD/gbp_kernels-hip-amdgcn-amd-amdhsa-gfx950.s NEW/gbp_kernels-hip-amdgcn-amd-amdhsa-gfx950.s [substring ...]

Per kernel (those whose mangled name holds one of the substrings; all without any): `same`, `DIFF`, `NEW` or `GONE`.  Compared is the text of
the kernel from its label to its .end_amdhsa_kernel — instructions and the kernel descriptor (registers, scratch, LDS) — without comments
and debug directives, and with the function number taken out of local labels (it shifts when a kernel is added in front).  Exit status 1
if a kernel that exists in both differs."""
import re
import sys


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel', s, re.S | re.M):
        lines = [re.sub(r'\s*;.*$', '', l).rstrip() for l in m.group(2).split('\n')]
        lines = [re.sub(r'(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI|L__unnamed_)\d+', r'\1N', l) for l in lines]
        out[m.group(1)] = '\n'.join(l for l in lines if l.strip() and not l.strip().startswith(('.loc', '.file', '.cfi')))
    return out


def main(argv):
    a, b = kernels(argv[0]), kernels(argv[1])
    want = argv[2:]
    differ = 0
    for k in sorted(set(a) | set(b)):
        if want and not any(w in k for w in want):
            continue
        st = 'NEW' if k not in a else 'GONE' if k not in b else 'same' if a[k] == b[k] else 'DIFF'
        differ += st == 'DIFF'
        print('%-5s %s' % (st, k))
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
