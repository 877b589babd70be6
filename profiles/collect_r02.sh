#!/bin/bash
# Round-2 recipe behind profiles/r02_* (run on the GPU box from the repo root; ~12 GPU-minutes).
set -x
R=$(pwd)
O=$R/gpurun_out/r02
mkdir -p $O
timeout 300 python bench.py --full --steps 20 --warmup 5 > $O/bench_28m_final.log 2> $O/bench_28m_final.err
timeout 200 python bench.py --full --steps 20 --warmup 5 --camera-order path --no-cpu-baseline > $O/bench_28m_path.log 2>&1
timeout 200 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --opt overlap_cameras=false --no-host-leg > $O/bench_28m_no_overlap.log 2>&1
timeout 200 python bench.py --full --config rubble10m --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_rubble10m_clm.log 2>&1
timeout 200 python bench.py --full --config bicycle6m --strategy no_offload --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_bicycle6m_no_offload.log 2>&1
timeout 200 python bench.py --full --config bicycle6m --steps 10 --warmup 3 --no-cpu-baseline --no-host-leg > $O/bench_bicycle6m_clm.log 2>&1
timeout 300 python bench.py --full --config bigcity102m --steps 6 --warmup 2 --no-cpu-baseline > $O/bench_bigcity102m_1gpu.log 2>&1
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_s /tmp/pmcF /tmp/pmcW /tmp/pmcS /tmp/prof_h
# kernel trace of the timed steps only (--no-kernel-timing: no instrumented pass, no single-stream batch
# after them); the timelines take ONE pipelined batch, delimited by two visibility_bits launches
timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_s -o st -- python $R/bench.py --full --steps 8 --warmup 3 --no-cpu-baseline --no-host-leg --no-kernel-timing > $O/prof_s.log 2>&1
DB=$(find /tmp/prof_s -name "*.db" | head -1)
python $R/profiles/kernel_stats.py "$DB" 170 > $O/kernel_stats.csv
python $R/profiles/timeline.py $DB step3 > $O/timeline_step.txt 2>&1
python $R/profiles/timeline_streams.py $DB step3 > $O/timeline_streams.txt 2>&1
# the same step on ONE stream (solo kernel durations, launch gaps)
rm -rf /tmp/prof_1
timeout 300 rocprofv3 --kernel-trace -d /tmp/prof_1 -o st -- python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-host-leg --no-kernel-timing --opt overlap_cameras=false > $O/prof_1.log 2>&1
DB1=$(find /tmp/prof_1 -name "*.db" | head -1)
python $R/profiles/timeline.py $DB1 step2 > $O/timeline_step_single_stream.txt 2>&1
python $R/profiles/timeline_streams.py $DB1 step2 > $O/timeline_streams_single_stream.txt 2>&1
timeout 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d /tmp/pmcF -o f -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-host-leg > $O/pmcF.log 2>&1
python $R/profiles/pmc_summary.py $(find /tmp/pmcF -name "*counter_collection.csv" | head -1) > $O/pmc_fetch_size.txt 2>&1
timeout 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d /tmp/pmcW -o w -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-host-leg > $O/pmcW.log 2>&1
python $R/profiles/pmc_summary.py $(find /tmp/pmcW -name "*counter_collection.csv" | head -1) > $O/pmc_write_size.txt 2>&1
rm -f $O/pmc_sq_counters.txt
for SET in "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES" "SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE"; do
  rm -rf /tmp/pmcS
  timeout 300 rocprofv3 --kernel-trace --pmc $SET --output-format csv -d /tmp/pmcS -o s -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-host-leg --prime-seconds 0 --opt overlap_cameras=false > $O/pmcS.log 2>&1
  echo "== $SET" >> $O/pmc_sq_counters.txt
  python $R/profiles/pmc_summary.py $(find /tmp/pmcS -name "*counter_collection.csv" | head -1) >> $O/pmc_sq_counters.txt 2>&1
done
# host-resident mode: kernels + SDMA copies on one timeline
timeout 300 rocprofv3 --kernel-trace --memory-copy-trace -d /tmp/prof_h -o h -- python $R/bench.py --full --residency host --steps 4 --warmup 2 --no-cpu-baseline --no-kernel-timing --camera-order path > $O/prof_h.log 2>&1
DBH=$(find /tmp/prof_h -name "*.db" | head -1)
python $R/profiles/timeline_host.py $DBH batches2 > $O/timeline_host_resident.txt 2>&1
# do VALU-bound and HBM-bound kernels overlap, or share a budget?  (also the plain-FMA issue peak)
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 $R/profiles/corun_probe.hip -o /tmp/corun_probe && /tmp/corun_probe > $O/corun_probe.jsonl 2>&1
cd $R
ls -la $O
