#!/bin/bash
# The fused step's level form with every operand group in turn one float off a 16-byte boundary, under
# -fsanitize=alignment,address, on the CPU: tests/emu/step_operand_sweep.cpp (a stand-alone program) linked with the
# emulator build of the kernel sources. One process per (dimension class, group, zero-fill, readout): a misaligned 16-byte
# access ends its process, so every case names its own first site. Prints one line per case and a summary; exit 1 if any
# case reported.
#   tools/step_operand_sweep.sh [build-dir]
set -u
root=$(cd $(dirname $0)/.. && pwd)
CL=/opt/rocm/lib/llvm/bin/clang++
out=${1:-${TMPDIR:-/tmp}/mpqe_step_sweep}
mkdir -p $out
flags="-x c++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=alignment,address -I$root/tests/emu/include -I$root/include"
newest=$(ls -t $root/mpqe_amd/csrc/*.hip $root/mpqe_amd/csrc/*.h $root/tests/emu/*.cpp $root/tests/emu/include/hip/*.h $root/include/mpqe_amd.h | head -1)
if [ ! -f $out/step_operand_sweep ] || [ $newest -nt $out/step_operand_sweep ]; then
    ls $root/mpqe_amd/csrc/*.hip $root/tests/emu/emu_runtime.cpp $root/tests/emu/step_operand_sweep.cpp |
        xargs -P 8 -I{} sh -c "$CL $flags -c {} -o $out/\$(basename {}).o" || exit 2
    $CL -fsanitize=alignment,address $out/*.o -o $out/step_operand_sweep || exit 2
fi
export ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0
export UBSAN_OPTIONS=print_stacktrace=0
bad=0
run() {
    log=$out/case.log
    $out/step_operand_sweep "$@" > $log 2>&1
    st=$?
    site=$(grep -m1 -E "runtime error|^ +#1 " $log | sed "s|$root/||")
    if [ $st -ne 0 ] || [ -n "$site" ]; then
        bad=$((bad + 1))
        echo "FAIL D=$1 $2 zero=${3:-0} readout=${4:-0} (exit $st): ${site:-$(tail -1 $log)}"
    else
        echo "ok   D=$1 $2 zero=${3:-0} readout=${4:-0}"
    fi
}
plain="none tables mode_emb basis_root bias g_tables g_mode_emb g_basis g_root g_bias outputs all"
for D in 6 32 64 68 192; do
    for g in $plain; do
        run $D $g 0 0
    done
    run $D all 1 2
done
for D in 64 68; do
    for ro in 4 5; do
        for g in none readout g_readout all; do
            run $D $g 0 $ro
        done
        run $D all 1 $ro
    done
done
echo "$bad case(s) reported"
[ $bad -eq 0 ]
