#!/bin/bash
# Measurement set of a round (run on the MI355X box via gpurun): full GPU test suite, bench lines for BASELINE configs[1] / [2] / [4]
# (with cpu_baseline + parity), rocprofv3 kernel-trace stats of the serial driver per config, per-layer roofline table, and the
# PMC passes for configs[1] (SQ counters incl. SQ_VALU_MFMA_BUSY_CYCLES, FETCH_SIZE, WRITE_SIZE -- separate passes).
# usage: bash tools/run_profiles.sh <tag>      -> gpurun_out/<tag>/   (copy what should be judged into profiles/)
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${1:-r02}
O=gpurun_out/$TAG
mkdir -p $O
echo "== tests" ; date
timeout 1800 python -m pytest tests -m gpu -q --timeout 900 -p no:cacheprovider > $O/tests.log 2>&1; tail -4 $O/tests.log
echo "== bench" ; date
for c in c2 c3 c5; do
  timeout 600 python bench.py --config $c --full > $O/bench_$c.log 2>&1; grep '^{"metric' $O/bench_$c.log | tail -1 > $O/bench_$c.json; cut -c1-160 $O/bench_$c.json
done
echo "== rocprof" ; date
for cfg in c2 c3 c5; do
  (cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats -d /tmp/prof_$cfg -o r -- python $GRAFT_REPO_ROOT/tools/profile_serial.py --config $cfg --steps 8 --ops $GRAFT_REPO_ROOT/$O/ops_$cfg.json > /tmp/ps_$cfg.log 2>&1)
  db=$(find /tmp/prof_$cfg -name "*.db" | head -1)
  python tools/rocprof_summary.py $db > $O/rocprof_summary_$cfg.csv 2>> $O/err.log
  python tools/layer_table.py --ops $O/ops_$cfg.json --stats $db > $O/layer_table_$cfg.csv 2>> $O/err.log
done
i=0
for set in "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY" "GRBM_GUI_ACTIVE SQ_INSTS_MFMA SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS SQ_INST_LEVEL_VMEM SQ_INSTS_VMEM_RD" "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1))
  (cd /tmp && timeout 400 rocprofv3 --pmc $set -d /tmp/pmc_$i -o r -- python $GRAFT_REPO_ROOT/tools/profile_serial.py --config c2 --steps 8 > /tmp/pmc_$i.log 2>&1)
done
dbs=$(for i in 1 2 3 4; do find /tmp/pmc_$i -name "*.db" | head -1; done)
python tools/layer_table.py --ops $O/ops_c2.json --stats $(find /tmp/prof_c2 -name "*.db" | head -1) --pmc $dbs > $O/layer_table_c2_pmc.csv 2>> $O/err.log
tail -3 $O/layer_table_c2_pmc.csv; tail -5 $O/err.log
date
