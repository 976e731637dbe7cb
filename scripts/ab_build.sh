#!/bin/bash
# A/B variant of the library: rebuild one kernel TU with extra -D flags and link it with the
# product's other objects into ablib/libpicocsum_<name>.so (scripts/gpu_ab.sh A=<name>).
#   [SRC=<other source of the TU>] scripts/ab_build.sh <name> <tu: raw|frag|fragtx|tcpseg|tcprx|sorted_m0..3|sorted_fused> -DFLAG=V ...
# The other objects are the ones the Makefile built (every pico_csum_k_*.o, k_sorted_m?.o, pico_csum.o).
# sorted_fused: the sorted TU's fused modes 1-3 (the stream paths) from SRC, mode 0 from the product.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; TU=$2; shift 2
make -s -j8 -C $R/picotcp_amd/csrc
B=$R/build/csrc; H=$R/picotcp_amd/csrc
BUILT=$(ls $B/pico_csum_k_*.o $B/k_sorted_m?.o $B/pico_csum.o)
mkdir -p $R/ablib $B/ab
HIPCC="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -I$R/include -I$R/picotcp_amd/csrc"
case $TU in
  sorted_fused)
    SRC=${SRC:-$H/pico_csum_k_sorted.hip}
    for m in 1 2 3; do $HIPCC -DSORTED_MODE=$m "$@" -c $SRC -o $B/ab/${NAME}_m$m.o & done; wait
    OBJS="$(echo "$BUILT" | grep -v "/k_sorted_m[123]\.o\$") $B/ab/${NAME}_m1.o $B/ab/${NAME}_m2.o $B/ab/${NAME}_m3.o" ;;
  sorted_m*) SRC=${SRC:-$H/pico_csum_k_sorted.hip}; EXTRA=-DSORTED_MODE=${TU#sorted_m}; OBJ=$B/k_$TU.o ;;
  raw|frag|fragtx|tcpseg|tcprx) SRC=${SRC:-$H/pico_csum_k_$TU.hip}; EXTRA=; OBJ=$B/pico_csum_k_$TU.o ;;
  *) echo "ab_build.sh: unknown TU $TU" >&2; exit 2 ;;
esac
if [ $TU != sorted_fused ]; then
  $HIPCC $EXTRA "$@" -c $SRC -o $B/ab/$NAME.o
  OBJS="$(echo "$BUILT" | grep -v "^$OBJ\$") $B/ab/$NAME.o"
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/ablib/libpicocsum_$NAME.so $OBJS \
    -Wl,--no-undefined -Wl,-soname,libpicocsum.so
echo "ablib/libpicocsum_$NAME.so"
