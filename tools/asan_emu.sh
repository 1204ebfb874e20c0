#!/bin/bash
# CPU sanitizer recipe ("-fsanitize=address host build").  Builds the host emulators of the kernel
# bodies (tests/emu/emu.cpp: the FFT passes; tests/emu/long_emu.cpp, long_outer_emu.cpp: the row kernels of the long
# lengths and the outer-decimation column kernels as the launcher instantiates them; tests/emu/sep_emu.cpp: the separable /
# direct stencils, their tap tables and the box normaliser; tests/emu/tv_emu.cpp: the RL-TV weight and apply kernels, the LDS
# tile allocated at exactly the kernel's element count; tests/emu/ring_emu.cpp: the ring-statistics products and reduction, image
# buffers of exactly the bytes the offsets reach -- the same templates the HIP kernels are made of, one OS thread
# per GPU thread) and the
# MINPACK restatement (csrc/gauss_fit.cpp) with AddressSanitizer + UndefinedBehaviorSanitizer and runs the tests that
# drive them -- every index computation of the convolution kernels, of the stencils' three LDS regions (allocated at
# exactly the launcher's byte count: the red zone begins where the launcher stopped paying), the Poisson sampler and the
# Gaussian fit -- under the sanitizer runtime.  CPU build only: GPU sanitizer builds are not part of this project.
#
#     tools/asan_emu.sh [extra pytest arguments]        (~8 min to compile at -O1)
#
# The long-row module is the slow part under the sanitizers (one OS thread per GPU thread, up to 576 per workgroup): about 2 / 4 /
# 7 min for its 1152 / 2304 / 4608 cases on 8 cores.  It shards by length -- the last step of this script with
#     tests/test_long_rows_cpu.py -k 1152   |   -k 2304   |   -k 4608   |   -k "not 1152 and not 2304 and not 4608"
# side by side covers every test of the module exactly once (RLSTED_ASAN_SKIP_BUILD=1 reuses the libraries of an earlier run).
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$ROOT/build/asan"
mkdir -p "$OUT"
FLAGS="-O1 -g -std=c++17 -fPIC -shared -ffp-contract=off -Wno-unknown-pragmas -pthread -fsanitize=address,undefined -fno-omit-frame-pointer"
if [ -z "${RLSTED_ASAN_SKIP_BUILD:-}" ]; then
echo "building $OUT/libemu.so (sanitized)"
g++ $FLAGS "$ROOT/tests/emu/emu.cpp" -o "$OUT/libemu.so"
for name in long_emu long_outer_emu; do
    echo "building $OUT/lib$name.so (sanitized)"
    g++ $FLAGS "$ROOT/tests/emu/$name.cpp" -o "$OUT/lib$name.so"
done
echo "building $OUT/libsep_emu.so (sanitized)"
g++ $FLAGS "$ROOT/tests/emu/sep_emu.cpp" -o "$OUT/libsep_emu.so"
echo "building $OUT/libtv_emu.so (sanitized)"
g++ $FLAGS "$ROOT/tests/emu/tv_emu.cpp" -o "$OUT/libtv_emu.so"
echo "building $OUT/libring_emu.so (sanitized)"
g++ $FLAGS "$ROOT/tests/emu/ring_emu.cpp" -o "$OUT/libring_emu.so"
echo "building $OUT/libgaussfit.so (sanitized)"
g++ $FLAGS -I"$ROOT/include" "$ROOT/rescan_line_sted_amd/csrc/gauss_fit.cpp" "$ROOT/tools/asan_gauss_fit_main.cpp" -o "$OUT/libgaussfit.so"
fi
ASAN_LIB="$(g++ -print-file-name=libasan.so)"
UBSAN_LIB="$(g++ -print-file-name=libubsan.so)"
export LD_PRELOAD="$ASAN_LIB:$UBSAN_LIB"
# python itself leaks by design; numpy allocates before the runtime is up: report real errors only
export ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1:allocator_may_return_null=1"
export UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"
export RLSTED_EMU_LIB="$OUT/libemu.so"
export RLSTED_LONG_EMU_LIB="$OUT/liblong_emu.so"
export RLSTED_LONG_OUTER_EMU_LIB="$OUT/liblong_outer_emu.so"
export RLSTED_SEP_EMU_LIB="$OUT/libsep_emu.so"
export RLSTED_TV_EMU_LIB="$OUT/libtv_emu.so"
export RLSTED_RING_EMU_LIB="$OUT/libring_emu.so"
export RLSTED_GAUSSFIT_LIB="$OUT/libgaussfit.so"
cd "$ROOT"
if [ -n "${RLSTED_ASAN_TESTS:-}" ]; then        # e.g. RLSTED_ASAN_TESTS=tests/test_long_rows_cpu.py tools/asan_emu.sh -k 4608
    python -m pytest $RLSTED_ASAN_TESTS -x -q -p no:cacheprovider "$@"
else
    python -m pytest tests/test_emulated_kernels.py tests/test_kernel_variants.py tests/test_long_rows_cpu.py tests/test_sep_cpu.py tests/test_tv_cpu.py tests/test_ring_cpu.py tests/test_poisson_spec.py tests/test_asan_gauss_fit.py -x -q -p no:cacheprovider "$@"
fi
echo "sanitizer run clean"
