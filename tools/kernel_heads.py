#!/usr/bin/env python3
"""Order of the memory instructions at the head of a kernel, from the gfx950 assembly of one HIP source (no GPU needed):
runs of scalar loads, global loads / stores and LDS accesses with their counts, every s_waitcnt, branch and barrier, up to the
N-th s_barrier or the first global store.  `sc1` marks the loads of common.h's vload().

    hipcc --offload-arch=gfx950 <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/kernels_pcg.hip -o /tmp/k.s
    tools/kernel_heads.py /tmp/k.s 'k_pcg_sq_l<double, false, false, float>' [N=2]
"""
import re
import subprocess
import sys

path, pat = sys.argv[1], sys.argv[2]
nbar = int(sys.argv[3]) if len(sys.argv) > 3 else 2
txt = open(path).read()
for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end', txt, re.S | re.M):
    name = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip()
    name = re.sub(r'\(.*', '', name.replace('void ', '').replace('fl::', ''))
    if pat not in name:
        continue
    print('==', name)
    out, bars, run, cnt = [], 0, None, 0

    def flush():
        global run, cnt
        if run:
            out.append(f'{run} x{cnt}')
        run, cnt = None, 0

    for line in m.group(2).split('\n'):
        t = line.strip().split(';')[0].strip()
        if not t or t.startswith('.') and not t.startswith('.LBB'):
            continue
        if t.startswith('.LBB'):
            flush()
            out.append(t)
            continue
        op = t.split()[0]
        key = None
        if op.startswith(('s_load', 'global_load', 'global_store', 'ds_write', 'ds_read')):
            key = op + (' sc1' if ' sc1' in t else '')
        elif op.startswith(('s_waitcnt', 's_cbranch', 's_barrier')) or op in ('s_branch', 's_endpgm'):
            flush()
            out.append(t)
        if op.startswith('s_barrier'):
            bars += 1
        if key:
            if key == run:
                cnt += 1
            else:
                flush()
                run, cnt = key, 1
        if bars >= nbar or op.startswith('global_store'):   # (a kernel without a barrier: its head ends at its first store)
            break
    flush()
    print('  ' + '\n  '.join(out))
