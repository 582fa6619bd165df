#!/bin/bash
# The measurement run behind profiles/r02_m..s: benches, kernel statistics and the separate --pmc passes, one MI355X.
set -e
# rocprofv3 initialises HIP before python starts: the queue request bench.py makes for itself has to be exported here
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${1:?usage: final_measure.sh OUTPUT_DIR}
mkdir -p $O
python bench.py --full > $O/r02_final_bench_default.json 2> $O/r02_final_bench_default.err
python bench.py --functional b3lyp --no-secondary --no-cpu-baseline > $O/r02_final_bench_b3lyp.json 2> $O/r02_final_b3lyp.err
python bench.py --df --no-secondary --no-cpu-baseline > $O/r02_final_bench_df.json 2> $O/r02_final_df.err
rocprofv3 --kernel-trace --stats -d $O/fprof_rhf -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > $O/fprof_rhf.log 2>&1
rocprofv3 --kernel-trace --stats -d $O/fprof_b3lyp -- python3 bench.py --functional b3lyp --steps 2 --warmup 1 --no-cpu-baseline --no-secondary > $O/fprof_b3lyp.log 2>&1
python3 scripts/rocpd_stats.py $O/fprof_rhf $O/r02_final_kernel_stats_rhf.csv 12
python3 scripts/rocpd_stats.py $O/fprof_b3lyp $O/r02_final_kernel_stats_b3lyp.csv 6
SQ="SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES"
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/fpmc_fetch -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-secondary > $O/fpmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/fpmc_write -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-secondary > $O/fpmc_write.log 2>&1
rocprofv3 --pmc $SQ --kernel-trace --output-format csv -d $O/fpmc_sq -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-secondary > $O/fpmc_sq.log 2>&1
rocprofv3 --pmc $SQ --kernel-trace --output-format csv -d $O/fpmc_sq_b3lyp -- python3 bench.py --functional b3lyp --steps 1 --warmup 1 --no-cpu-baseline --no-secondary > $O/fpmc_sq_b3lyp.log 2>&1
rocprofv3 --pmc $SQ --kernel-trace --output-format csv -d $O/fpmc_sq_df -- python3 bench.py --df --steps 1 --warmup 1 --no-cpu-baseline --no-secondary > $O/fpmc_sq_df.log 2>&1
python3 scripts/pmc_summary.py fetch=$O/fpmc_fetch write=$O/fpmc_write sq=$O/fpmc_sq sq_b3lyp=$O/fpmc_sq_b3lyp sq_df=$O/fpmc_sq_df > $O/r02_final_pmc_summary.txt
cp profiles/r02_pmc_*.csv profiles/r02_pmc_summary.json $O/
echo done
