#!/bin/bash
# The kept part of streamed lists (include/espm_mu.h: ell_keep_h, ell_keep_w), measured against the parent commit on one GPU.
#   PARENT=<a checkout of the parent commit with its library built, tools/analysis/keep_iter.py copied into it>
#   PARENT_LIB=<the parent's kernels as a library that takes this tree's state struct: the parent's sources with this include/espm_mu.h
#               and the two new names in mu_api.hip's field list, so that variant_ab.py can hold both in one process>
#   PARTS="gonogo sweep ab sizes bench fetch c5" OUT=<directory> bash tools/analysis/keep_measure.sh
# gonogo: H walk plain / W walk non-temporal against all non-temporal - timing and a FETCH_SIZE pass of its own, nothing else traced
# sweep:  kept list groups {0, 2, 4, 6, 8 of 8} x kept channel groups {0, 8, 16, 24, 32 of 32} at the headline, one process
# ab:     parent | new (the engine's policy), headline, 7 interleaved repetitions        sizes: the same at ROWS / COUNTS
# bench:  bench.py, parent and new in turn, twice                                          fetch: FETCH_SIZE per fused launch, parent | new
# Every step that uses the GPU has a time limit of its own and the script stops at the first failure.
set -e -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-$R/build/keep_measure}
PARTS=${PARTS:-"gonogo"}
LIB=espm_amd/lib/libespm_mu.so
has() { case " $PARTS " in *" $1 "*) return 0;; *) return 1;; esac; }
mkdir -p $OUT
cd $R
pmc() {   # pmc <name> <tree> [VAR=value ...]: a counter pass of its own
  local name=$1 tree=$2; shift 2
  (cd /tmp && env TMPDIR=/tmp ITERS=60 "$@" timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_$name -- python3 $tree/tools/analysis/keep_iter.py > $OUT/pmc_$name.log 2>&1)
}
if has gonogo; then
  REPS=4 timeout -k 10 300 python tools/analysis/variant_ab.py parent=$PARENT_LIB nt=$LIB@ESPM_ELL_KEEP_GROUPS=0:0 h_plain=$LIB@ESPM_ELL_KEEP_GROUPS=8:0 \
      w_plain=$LIB@ESPM_ELL_KEEP_GROUPS=0:32 2>&1 | tee $OUT/gonogo_ab.log
  pmc nt $R ESPM_ELL_KEEP_GROUPS=0:0
  pmc h_plain $R ESPM_ELL_KEEP_GROUPS=8:0
  python3 tools/analysis/pmc_fetch.py nt=$OUT/pmc_nt h_plain=$OUT/pmc_h_plain | tee $OUT/gonogo_fetch.txt
fi
if has sweep; then
  SPECS=""
  for h in 0 2 4 6 8; do for w in 0 8 16 24 32; do SPECS="$SPECS h${h}w${w}=$LIB@ESPM_ELL_KEEP_GROUPS=$h:$w"; done; done
  REPS=4 timeout -k 10 900 python tools/analysis/variant_ab.py parent=$PARENT_LIB $SPECS 2>&1 | tee $OUT/keep_sweep.log
fi
if has ab; then
  REPS=7 timeout -k 10 300 python tools/analysis/variant_ab.py parent=$PARENT_LIB new=$LIB 2>&1 | tee $OUT/ab_keep_512.log
fi
if has sizes; then
  for RW in 64 128 256; do ROWS=$RW REPS=7 timeout -k 10 300 python tools/analysis/variant_ab.py parent=$PARENT_LIB new=$LIB 2>&1 | tee $OUT/ab_keep_rows$RW.log; done
  for CN in 100 250; do COUNTS=$CN REPS=7 timeout -k 10 300 python tools/analysis/variant_ab.py parent=$PARENT_LIB new=$LIB 2>&1 | tee $OUT/ab_keep_counts$CN.log; done
fi
if has bench; then
  : > $OUT/bench.txt
  for i in 1 2; do
    for side in parent new; do
      tree=$R; [ $side = parent ] && tree=$PARENT
      echo "== $side, run $i" >> $OUT/bench.txt
      (cd $tree && timeout -k 10 300 python bench.py --gpus 1 --steps 300 --warmup 30 2> $OUT/bench_${side}_$i.err | tail -1 | cut -c1-400 >> $OUT/bench.txt)
    done
  done
  cat $OUT/bench.txt
fi
if has fetch; then
  pmc parent $PARENT
  pmc new $R
  python3 tools/analysis/pmc_fetch.py parent=$OUT/pmc_parent new=$OUT/pmc_new | tee $OUT/pmc_fetch.txt
  for side in parent new; do grep '^rows ' $OUT/pmc_$side.log | sed "s/^/$side (under the profiler): /"; done | tee -a $OUT/pmc_fetch.txt
fi
if has c5; then
  CONFIG=c5 ROWS=1024 ITERS=100 REPS=3 timeout -k 10 600 python tools/analysis/variant_ab.py parent=$PARENT_LIB new=$LIB 2>&1 | tee $OUT/ab_keep_c5.log
fi
