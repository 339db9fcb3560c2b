#!/usr/bin/env python3
"""Per-kernel resource usage of the LDS apply engine (mt_apply.hip, and the wide editing form's
translation unit beside it, mt_apply_locw.hip) as the compiler reports it
(-Rpass-analysis=kernel-resource-usage, gfx950): VGPRs, SGPR spills, scratch bytes per lane, LDS bytes
per block, occupancy -- one row per instantiation, named by its template arguments.
    python tools/resource_usage_lds.py [path/to/mt_apply.hip] > profiles/rNN_resource_usage_lds.txt
Two trees (a parent checkout and this one) give two tables to diff."""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, 'fluidframework_amd', 'csrc', 'mt_apply.hip')


def form(kernel, args):
    """A readable name of an instantiation from its mangled template arguments."""
    b = [x == '1' for x in re.findall(r'Lb([01])E', args)]
    gw = re.findall(r'Li(\d+)E', args)[1:]
    if kernel == 'apply_kernel':      # <CAP, GEN, LOC>
        return 'generator' if b[0] else 'editing' if b[1] else 'narrow'
    if kernel == 'apply_kernel_wl':   # <CAP>
        return 'wide (LDS)'
    w, loc = b[0], b[1]               # apply_kernel_g<CAP, W, LOC, GW>
    return ('wide editing' if w and loc else 'wide' if w else 'editing' if loc else 'narrow') + ' (HBM)' + \
        (' GW=%s' % gw[0] if loc and gw else '')


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else SRC
    locw = os.path.join(os.path.dirname(src), 'mt_apply_locw.hip')  # (a tree from before it has none)
    srcs = [src] + ([locw] if os.path.exists(locw) else [])
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
                                   '-Wno-unused-value', '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage',
                                   '-c', f, '-o', os.path.join(d, 'o%d' % i)], stderr=subprocess.PIPE, text=True)
                 for i, f in enumerate(srcs)]
        remarks = ''
        for p in procs:
            remarks += p.communicate()[1]
            if p.returncode:
                sys.exit(remarks)
    table(remarks)


def table(remarks):
    """Print the table of the compiler's remarks (its stderr)."""
    print('# mt_apply.hip (LDS engine), hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage')
    print('# %-16s %5s  %-23s %5s %12s %15s %10s %11s' % ('kernel', 'CAP', 'form', 'VGPR', 'SGPR-spills', 'scratch B/lane',
                                                            'LDS B', 'waves/SIMD'))
    rows = []
    for b in re.split(r'remark: [^\n]*Function Name: ', remarks)[1:]:
        m = re.search(r'(apply_kernel(?:_g|_wl)?)ILi(\d+)E(\w*?)EEv', b.split('\n')[0])
        if not m:
            continue

        def g(k):
            x = re.search(k + r': (\S+)', b)
            return x.group(1) if x else '?'
        rows.append((m.group(1), int(m.group(2)), form(m.group(1), 'Li%sE%sE' % (m.group(2), m.group(3))), g('VGPRs'),
                     g('SGPRs Spill'), g(r'ScratchSize \[bytes/lane\]'), g(r'LDS Size \[bytes/block\]'),
                     g(r'Occupancy \[waves/SIMD\]')))
    for row in sorted(rows, key=lambda x: (x[2], x[0], x[1])):
        print('  %-16s %5d  %-23s %5s %12s %15s %10s %11s' % row)


if __name__ == '__main__':
    sys.exit(main())
