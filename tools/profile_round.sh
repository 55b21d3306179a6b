#!/bin/bash
# GPU box: kernel-trace + PMC summaries of the headline bench for both solvers on two windows of the rollout -- the driver's
# (--warmup 5: steps 5-55, the humanoids still falling, nefc ~ 15) and the steady one (--warmup 300, nefc ~ 45) --, plus the bench lines.
# usage: tools/profile_round.sh <round tag, e.g. round4> [solvers, default "cg newton"]
set -u
R=${1:-round4}
export PROFILE_LAST=200
export PROFILE_OUT=${PROFILE_OUT:-profile_out}  # tools/profile.sh's summaries and this script's bench lines
for sv in ${2:-cg newton}; do
  for win in steady early; do
    W=300; LABEL="steps 300-350 of the rollout (steady state)"
    if [ $win = early ]; then W=5; LABEL="steps 5-55 of the rollout (the driver's --warmup 5 window)"; fi
    bash tools/profile.sh ${R}_${sv}_$win --solver $sv --warmup $W > /dev/null 2>&1
    python tools/make_pmc_summary.py $PROFILE_OUT/prof_${R}_${sv}_$win/summary.json $PROFILE_OUT/${R}_pmc_${sv}_$win.json $sv "$LABEL" > /dev/null
    cp $PROFILE_OUT/prof_${R}_${sv}_$win/summary.json $PROFILE_OUT/${R}_${sv}_${win}_summary.json
  done
  cp $PROFILE_OUT/${R}_pmc_${sv}_steady.json $PROFILE_OUT/${R}_pmc_$sv.json
  python bench.py --full --solver $sv --pmc-profile $PROFILE_OUT/${R}_pmc_$sv.json > $PROFILE_OUT/${R}_bench_$sv.json 2> $PROFILE_OUT/${R}_bench_$sv.err
  tail -c 1500 $PROFILE_OUT/${R}_bench_$sv.json
done
