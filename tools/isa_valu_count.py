"""Static instruction counts of kernels in a gfx950 assembly file (hipcc --cuda-device-only -S): per kernel whose mangled name
contains FILTER the vector ALU instructions (all / float64 / the slow ones: v_sqrt, v_rcp, v_div_*), LDS and global memory
instructions, registers and LDS bytes.  Static counts: every instruction once, whatever path a lane takes.

    python3 tools/isa_valu_count.py FILE.s [FILTER]
"""
import re
import sys


def main(path, flt):
    kernels, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r'^(_Z\w+):', line)
            if m:
                cur = m.group(1) if flt in m.group(1) else None
                if cur:
                    kernels[cur] = dict(valu=0, f64=0, slow=0, lds=0, vmem=0, vgpr=None, lds_bytes=None)
                continue
            if cur is None:
                continue
            if line.startswith('\t.end_amdhsa_kernel') or line.startswith('.Lfunc_end'):
                cur = None if line.startswith('\t.end_amdhsa_kernel') else cur
                continue
            k = kernels[cur]
            op = line.strip().split(' ')[0]
            if op.startswith('v_'):
                k['valu'] += 1
                k['f64'] += op.endswith('_f64')
                k['slow'] += op.startswith(('v_sqrt', 'v_rcp', 'v_rsq', 'v_div_'))
            elif op.startswith('ds_'):
                k['lds'] += 1
            elif op.startswith(('global_', 'flat_', 'buffer_')):
                k['vmem'] += 1
            m = re.match(r'\s*\.amdhsa_next_free_vgpr (\d+)', line)
            if m:
                k['vgpr'] = int(m.group(1))
            m = re.match(r'\s*\.amdhsa_group_segment_fixed_size (\d+)', line)
            if m:
                k['lds_bytes'] = int(m.group(1))
    print('%8s %8s %8s %6s %6s %8s %9s  kernel' % ('VALU', 'f64', 'slow', 'LDS', 'VMEM', 'nextVGPR', 'LDS bytes'))
    for name, k in kernels.items():
        print('%8d %8d %8d %6d %6d %8s %9s  %s' % (k['valu'], k['f64'], k['slow'], k['lds'], k['vmem'], k['vgpr'], k['lds_bytes'], name))


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else '')
