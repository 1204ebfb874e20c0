"""Manual helper (not a test): is the device code of csrc/fft_kernels.hip the same in two source trees?  For a refactor that must
not change what the compiler emits.  Per FFT length, both trees' fft_kernels.hip are compiled device-only with the flags of
rescan_line_sted_amd/_build.py; the sets of kernel symbols must be equal and every kernel's instructions identical.  Kernels
are compared by name, not by their place in the file: the order in which templates are instantiated moves them around.

    python3 tools/device_code_compare.py TREE_A TREE_B [WORKDIR]        exit status 1 on any difference; no GPU needed

With --all, every source of _build.jobs() that carries device code is compared instead (every .hip file, every FFT length, and the
.cpp files compiled as HIP), for a change that must leave every existing kernel alone.  A source that only one tree has is listed
and not counted as a difference.

    python3 tools/device_code_compare.py --all TREE_A TREE_B [WORKDIR]
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
    return disassembly(tree, 'fft_kernels.hip', _build.DEVICE + _build.FFT_FLAGS + ['-DRL_CFG_L=%d' % L], os.path.join(work, 'fft_%d.elf' % L))


def disassembly(tree, source, flags, elf):
    """{symbol: [instruction text]} of the device code of csrc/`source` of `tree`, compiled with `flags`"""
    _build._run([_build.HIPCC, '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(tree, 'include')] + flags +
                ['--cuda-device-only', '--no-gpu-bundle-output', '-c', os.path.join(tree, 'rescan_line_sted_amd', 'csrc', source), '-o', elf])
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


def report(name, ka, kb):
    digest = [hashlib.sha256('\n'.join(k + '\n' + '\n'.join(d[k]) for k in sorted(d)).encode()).hexdigest()[:16] for d in (ka, kb)]
    differ = sorted(set(ka) ^ set(kb)) + [k for k in sorted(set(ka) & set(kb)) if ka[k] != kb[k]]
    print('%-28s kernels %3d / %3d   sha256 of the sorted disassembly %s / %s   %s' % (name, len(ka), len(kb), digest[0], digest[1],
                                                                                 'identical' if not differ else 'DIFFERENT: %s' % differ[:4]))
    return bool(differ)


def main_all(a, b, work):
    """Every job of _build.jobs() with device flags, by its object's name; the symbols counted are the functions of the device ELF"""
    todo, only = [], []
    for obj, src, flags in _build.jobs():
        if not any(f.startswith('--offload-arch') for f in flags):
            continue
        name, source = os.path.splitext(os.path.basename(obj))[0], os.path.basename(src)
        have = [os.path.exists(os.path.join(t, 'rescan_line_sted_amd', 'csrc', source)) for t in (a, b)]
        if all(have):
            todo.append((name, source, flags))
        else:
            only.append((name, 'A' if have[0] else 'B'))
    for d in ('a', 'b'):
        os.makedirs(os.path.join(work, d), exist_ok=True)
    runs = [(t, source, flags, os.path.join(work, d, name + '.elf')) for name, source, flags in todo for t, d in ((a, 'a'), (b, 'b'))]
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda j: disassembly(*j), runs))
    bad = sum(report(name, res[2 * i], res[2 * i + 1]) for i, (name, _, _) in enumerate(todo))
    for name, which in only:
        print('%-28s only in tree %s: not compared' % (name, which))
    return 1 if bad else 0


def main():
    if sys.argv[1] == '--all':
        a, b = sys.argv[2:4]
        return main_all(a, b, sys.argv[4] if len(sys.argv) > 4 else tempfile.mkdtemp(prefix='devcmp_'))
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
