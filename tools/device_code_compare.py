"""Manual helper (not a test): is the device code of csrc/fft_kernels.hip the same in two source trees?  For a refactor that must
not change what the compiler emits.  Per FFT length, both trees' fft_kernels.hip are compiled device-only with the flags of
rescan_line_sted_amd/_build.py; the sets of kernel symbols must be equal and every kernel's instructions identical.  Kernels
are compared by name, not by their place in the file: the order in which templates are instantiated moves them around.

    python3 tools/device_code_compare.py TREE_A TREE_B [WORKDIR]        exit status 1 on any difference; no GPU needed
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rescan_line_sted_amd import _build  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(_build.HIPCC)), 'llvm', 'bin')


def kernels(tree, L, work):
    """{symbol: [instruction text]} of one length's device code"""
    elf = os.path.join(work, 'fft_%d.elf' % L)
    _build._run([_build.HIPCC, '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(tree, 'include')] + _build.DEVICE + _build.FFT_FLAGS +
                ['-DRL_CFG_L=%d' % L, '--cuda-device-only', '--no-gpu-bundle-output', '-c',
                 os.path.join(tree, 'rescan_line_sted_amd', 'csrc', 'fft_kernels.hip'), '-o', elf])
    text = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', elf], text=True)
    out, cur = {}, None
    for line in text.split('\n'):
        m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            ins = line.split('//')[0].strip()          # (the comment holds the address and the encoding)
            if ins and ins != '...':
                cur.append(ins)
    for body in out.values():                           # padding between functions
        while body and body[-1].startswith(('s_nop', 's_code_end')):
            body.pop()
    return out


def main():
    a, b = sys.argv[1:3]
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix='devcmp_')
    jobs = [(t, L, os.path.join(work, n)) for L in _build.FFT_LENGTHS for t, n in ((a, 'a'), (b, 'b'))]
    for _, _, d in jobs:
        os.makedirs(d, exist_ok=True)
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda j: kernels(*j), jobs))
    bad = 0
    for i, L in enumerate(_build.FFT_LENGTHS):
        ka, kb = res[2 * i], res[2 * i + 1]
        digest = [hashlib.sha256('\n'.join(k + '\n' + '\n'.join(d[k]) for k in sorted(d)).encode()).hexdigest()[:16] for d in (ka, kb)]
        differ = sorted(set(ka) ^ set(kb)) + [k for k in sorted(set(ka) & set(kb)) if ka[k] != kb[k]]
        bad += bool(differ)
        print('L = %-5d kernels %d / %d   sha256 of the sorted disassembly %s / %s   %s' % (L, len(ka), len(kb), digest[0], digest[1],
                                                                                        'identical' if not differ else 'DIFFERENT: %s' % differ[:4]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
