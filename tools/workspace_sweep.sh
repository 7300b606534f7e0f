#!/bin/bash
# Entry points that take a library-sized workspace or plan, with that buffer exactly as large as its mpqe_*_bytes function
# says and every byte set, under -fsanitize=alignment,address, on the CPU: tests/emu/workspace_sweep.cpp,
# tests/emu/mixed_sweep.cpp, tests/emu/rgcn_mixed_sweep.cpp and tests/emu/rgcn_mixed_train_sweep.cpp (stand-alone programs)
# linked with the emulator build of the kernel sources. One process per (case, offset): the first access outside a buffer, or the first misaligned wide access, ends its process and names its
# site. Prints one line per case and a summary; exit 1 if any case reported.
#   tools/workspace_sweep.sh [build-dir]
set -u
root=$(cd $(dirname $0)/.. && pwd)
CL=/opt/rocm/lib/llvm/bin/clang++
out=${1:-${TMPDIR:-/tmp}/mpqe_workspace_sweep}
mkdir -p $out
flags="-x c++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=alignment,address -I$root/tests/emu/include -I$root/include"
newest=$(ls -t $root/mpqe_amd/csrc/*.hip $root/mpqe_amd/csrc/*.h $root/tests/emu/*.cpp $root/tests/emu/include/hip/*.h $root/include/mpqe_amd.h | head -1)
if [ ! -f $out/rgcn_mixed_train_sweep ] || [ $newest -nt $out/rgcn_mixed_train_sweep ]; then
    ls $root/mpqe_amd/csrc/*.hip $root/tests/emu/emu_runtime.cpp $root/tests/emu/workspace_sweep.cpp $root/tests/emu/mixed_sweep.cpp \
        $root/tests/emu/rgcn_mixed_sweep.cpp $root/tests/emu/rgcn_mixed_train_sweep.cpp |
        xargs -P 8 -I{} sh -c "$CL $flags -c {} -o $out/\$(basename {}).o" || exit 2
    kernels=$(ls $out/*.o | grep -v -e workspace_sweep.cpp.o -e mixed_sweep.cpp.o -e rgcn_mixed_sweep.cpp.o -e rgcn_mixed_train_sweep.cpp.o)
    $CL -fsanitize=alignment,address $kernels $out/workspace_sweep.cpp.o -o $out/workspace_sweep || exit 2
    $CL -fsanitize=alignment,address $kernels $out/mixed_sweep.cpp.o -o $out/mixed_sweep || exit 2
    $CL -fsanitize=alignment,address $kernels $out/rgcn_mixed_sweep.cpp.o -o $out/rgcn_mixed_sweep || exit 2
    $CL -fsanitize=alignment,address $kernels $out/rgcn_mixed_train_sweep.cpp.o -o $out/rgcn_mixed_train_sweep || exit 2
fi
export ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0
export UBSAN_OPTIONS=print_stacktrace=0
bad=0
for c in rank rank_strips general general64 linear template layernorm scatter rows auc_segments gqe_mixed rgcn_mixed rgcn_mixed_train; do
    prog=workspace_sweep
    case $c in auc_segments|gqe_mixed) prog=mixed_sweep ;; rgcn_mixed) prog=rgcn_mixed_sweep ;; rgcn_mixed_train) prog=rgcn_mixed_train_sweep ;; esac
    for off in 0 4; do
        log=$out/case.log
        $out/$prog $c $off > $log 2>&1
        st=$?
        site=$(grep -m1 -E "runtime error|^ +#1 " $log | sed "s|$root/||")
        if [ $st -ne 0 ] || [ -n "$site" ]; then
            bad=$((bad + 1))
            echo "FAIL $c off=$off (exit $st): ${site:-$(tail -1 $log)}"
        else
            echo "ok   $c off=$off: $(tail -1 $log)"
        fi
    done
done
echo "$bad case(s) reported"
[ $bad -eq 0 ]
