# Build the current csrc tree into build/variants/lib_<name>.so (dev tool, for tools/q2.sh VARIANTS=...)
# usage: tools/build_variant.sh <name> [extra hipcc flags...]
# The units and their flags are the Makefile's; the extra flags (-D switches) go to every unit.
set -e
name=$1; shift
out=$PWD/build/variants
mkdir -p $out/$name
make -s -j8 -C distributed_sudoku_solver_amd/csrc OUT=$out/lib_$name.so BUILD=$out/$name EXTRA="$*" $out/lib_$name.so
