# the measurement set of the round: bash tools/prof/r02_final.sh <tag>   (one MI355X)
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out; mkdir -p $O; T=${1:-r02}
cd $R
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
python bench.py --full --image-size 512 --frames 64 --no-lbs --lasr-iters 0 > $O/${T}_bench_512.json 2>/dev/null
python tools/cosdist_bench.py > $O/${T}_cosdist.json 2>/dev/null
cd /tmp; export TMPDIR=/tmp
B="python $R/bench.py --full --no-cpu-baseline --no-lbs --lasr-iters 0"
rocprofv3 --kernel-trace -d $O/prof_k -o k -- $B --steps 30 --warmup 3 > /dev/null 2>&1
python $R/tools/rocpd_stats.py $(find $O/prof_k -name "*.db" | head -1) > $O/${T}_kernel_stats.txt; rm -rf $O/prof_k
rocprofv3 --kernel-trace -d $O/prof_o -o o -- python $R/bench.py --full --no-cpu-baseline --no-lbs --steps 1 --warmup 1 --frames 16 --lasr-iters 30 > /dev/null 2>&1
python $R/tools/rocpd_stats.py $(find $O/prof_o -name "*.db" | head -1) 90 > $O/${T}_optimize_step_kernel_stats.txt; rm -rf $O/prof_o
pmc() {  # $1 = output file, $2 = extra bench args, rest = counters
  out=$1; extra=$2; shift; shift
  rocprofv3 --pmc "$@" -d $O/pmc_x -o p -- $B $extra --steps 3 --warmup 1 > /dev/null 2>&1
  python $R/tools/pmc_summary.py $(find $O/pmc_x -name "*.db" | head -1) >> $out 2>/dev/null; rm -rf $O/pmc_x
}
rm -f $O/${T}_pmc.txt $O/${T}_pmc_sq.txt $O/${T}_pmc_512.txt $O/${T}_pmc_lbs.txt
pmc $O/${T}_pmc.txt "" FETCH_SIZE
pmc $O/${T}_pmc.txt "" WRITE_SIZE
pmc $O/${T}_pmc_512.txt "--image-size 512 --frames 64" FETCH_SIZE
pmc $O/${T}_pmc_512.txt "--image-size 512 --frames 64" WRITE_SIZE
pmc $O/${T}_pmc_sq.txt "" SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_THREAD_CYCLES_VALU SQ_INSTS_VMEM_RD
pmc $O/${T}_pmc_sq.txt "" SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_SCA SQ_LDS_BANK_CONFLICT SQ_BUSY_CU_CYCLES SQ_WAVES SQ_INSTS_BRANCH
pmc $O/${T}_pmc_sq.txt "" SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_CVT SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_ADD_F32
rocprofv3 --pmc SQ_INSTS_VALU_MFMA_F32 SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES -d $O/pmc_x -o p -- python $R/tools/lbs_bench.py > /dev/null 2>&1
python $R/tools/pmc_summary.py $(find $O/pmc_x -name "*.db" | head -1) > $O/${T}_pmc_lbs.txt 2>/dev/null; rm -rf $O/pmc_x
cd $R; python tools/op_census.py 2>&1 | grep -v -i warn > $O/${T}_op_census.txt
python tools/traffic_json.py $O/${T}_pmc.txt 256 "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes of bench.py --full --no-cpu-baseline --no-lbs --lasr-iters 0 --steps 3 --warmup 1 (256 frames per launch, mesh M2, 256x256); KiB per dispatch summed over all TCC instances; bytes = (FETCH_SIZE + WRITE_SIZE) * 1024 raw (the gfx950 x2 read correction of MI355X_MICROARCH.md is calibrated for 16 B/lane coalesced streams only; these kernels gather 4 B/lane and read records through the scalar cache)" > $O/${T}_traffic.json
python -c "
import json;d=json.load(open('$O/${T}_bench.json'))
print(d['value'], d['ms_per_step'], d['roofline']['all_kernels_avg_ms'], d['roofline']['frac'], d['roofline']['traffic']); print(d['cpu_baseline']['value'], d['cpu_baseline']['cores'], d['cpu_baseline']['one_thread_frames_per_s']); print(d.get('optimize_py',{}).get('iters_per_s'))
d=json.load(open('$O/${T}_bench_512.json')); print('512:', d['value'], d['roofline']['all_kernels_avg_ms'], d['roofline']['frac'])"
head -8 $O/${T}_kernel_stats.txt | cut -c1-140; cat $O/${T}_pmc.txt | cut -c1-120; cat $O/${T}_pmc_lbs.txt | grep -i lbs | cut -c1-130
