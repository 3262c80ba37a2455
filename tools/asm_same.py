"""
Are the kernels of two builds the same instructions?  Compares two gfx950 assembly listings (hipcc -S --cuda-device-only of the same
source at two commits) kernel by kernel: comments, local label numbers, mangled names and the kernarg size are set aside, everything else --
every instruction, operand and register -- must match.  A kernel template that gained a trailing defaulted `bool` parameter is matched with
its instantiation `<..., false>` in the newer listing (--added-false NAME).

    hipcc --offload-arch=gfx950 $CXXFLAGS $FLAGS_kns_stft -S --cuda-device-only -x hip koala_amd/csrc/kns_stft.hip -o new.s
    (the same at the parent commit -> old.s)
    python tools/asm_same.py old.s new.s --added-false synthesis_kernel
"""
import argparse
import re
import sys


def bodies(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):\s*; @\S+\n(.*?)^\.Lfunc_end\d+:', text, re.M | re.S):
        body = re.sub(r';.*', '', m.group(2))
        body = re.sub(r'\.LBB\d+_', '.LBB_', body)
        body = re.sub(r'_Z\w+', 'KERNEL', body)
        body = re.sub(r'\.amdhsa_kernarg_size \d+', '', body)
        out[m.group(1)] = [line.rstrip() for line in body.splitlines() if line.strip()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--added-false', action='append', default=[], help='template that gained a trailing `bool = false` parameter')
    a = ap.parse_args()
    old, new = bodies(a.old), bodies(a.new)
    different = 0
    for name, body in old.items():
        other = name
        for t in a.added_false:
            other = re.sub(r'(%d%sI(?:Lb[01]E)+)E' % (len(t), t), r'\1Lb0EE', other)
        if other not in new:
            print('MISSING    %s' % name)
            different += 1
        elif new[other] == body:
            print('identical  %5d lines  %s' % (len(body), name))
        else:
            print('DIFFERENT  %s' % name)
            different += 1
    print('%d kernels of the old listing: %d identical, %d not; %d kernels only in the new listing' %
          (len(old), len(old) - different, different, len(new) - len(old)))
    sys.exit(1 if different else 0)


if __name__ == '__main__':
    main()
