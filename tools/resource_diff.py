#!/usr/bin/env python
"""Compare two `hipcc -Rpass-analysis=kernel-resource-usage` logs kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c csrc/conv_mfma.hip 2> new.txt   (same for the parent)
    python tools/resource_diff.py parent.txt new.txt [name filter]

Prints every kernel whose figures differ (VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy, LDS bytes), the count of
unchanged ones, and fails if any kernel gained scratch."""
import re
import subprocess
import sys

FIELDS = (('VGPRs', 'vgpr'), ('AGPRs', 'agpr'), ('TotalSGPRs', 'sgpr'), ('ScratchSize [bytes/lane]', 'scratch'),
          ('Occupancy [waves/SIMD]', 'occ'), ('LDS Size [bytes/block]', 'lds'))


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r'remark: .*Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r'remark: .*\s' + re.escape(label) + r': (\d+)', line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def demangle(names):
    try:
        res = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ''
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    same, bad = 0, 0
    for n in names:
        short = pretty[n].replace('(anonymous namespace)::', '').replace('void ', '', 1).split('(')[0]
        if flt and flt not in short:
            continue
        if a.get(n) == b.get(n):
            same += 1
            continue
        fa, fb = a.get(n, {}), b.get(n, {})
        print(short)
        print('    ' + '  '.join(f'{k} {fa.get(k, "-")} -> {fb.get(k, "-")}' for _, k in FIELDS))
        if fb.get('scratch', 0) > fa.get('scratch', 0):
            bad += 1
    print(f'{same} kernels unchanged in every figure; {bad} gained scratch')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
