#!/bin/bash
# development: build_variant.sh NAME 'sed-expr on kge_rank_screen.h' -> build_variants/NAME/libamdkge.so
# A copy of the sources (time stamps kept) and of the tree's own objects (build/obj; not their dependency files, which are valid
# in that directory only) is built by the library's Makefile without the object of the unit that includes the edited header: the
# screening unit, kge_rank_screen.o, is compiled again, every other object is up to date against its .hip.
# With EXTRA=-D... (SCRR_ABLATE, SCRR_DEPTH, SCRR_FIRST_SLOT, SCRR_SECOND_SLOT, KGE_MLD) every ranking unit is compiled again: make does
# not see a changed flag.
set -e
N=$1; R=$(cd "$(dirname "$0")/.." && pwd); V=/tmp/variant_$N
rm -rf $V; mkdir -p $V/ampligraph_amd $V/include $V/obj $R/build_variants/$N
cp -rp $R/ampligraph_amd/csrc $V/ampligraph_amd/; cp -p $R/include/amdkge.h $V/include/
cp -p $R/build/obj/*.o $V/obj/
[ -n "${2:-}" ] && sed -i "$2" $V/ampligraph_amd/csrc/kge_rank_screen.h
rm -f $V/obj/kge_rank_screen.o
[ -n "${EXTRA:-}" ] && rm -f $V/obj/kge_rank*.o
make -C $V/ampligraph_amd/csrc -j${MAX_JOBS:-4} OBJDIR=$V/obj OUT=$R/build_variants/$N/libamdkge.so EXTRA="${EXTRA:-}"
ls -la $R/build_variants/$N/libamdkge.so
