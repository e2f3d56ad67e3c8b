#!/bin/bash
# rocprofv3 passes behind profiles/: kernel stats, then HBM / VALU counters in separate --pmc runs (MI355X_MICROARCH.md, HBM section).
# usage (on an MI355X): bash tools/profile_round.sh <tag> [out_dir]     -> <out_dir>/<tag>_*.txt + bench lines (out_dir: profile_out/)
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}; TAG=${1:-r02}
O=${2:-$R/profile_out}; mkdir -p $O
cd /tmp; export TMPDIR=/tmp
B="python $R/bench.py --full --steps 8 --warmup 2 --no-cpu-baseline --no-pmc"
rocprofv3 --kernel-trace --stats -d $O/${TAG}_stats -o bench -- $B > $O/${TAG}_stats.log 2>&1
# counter passes: the child command of bench.py --full's own live counters (headline training steps + fused steps; no layered / trained-like extras, whose
# launches at other sizes would be averaged into the per-dispatch totals)
P="python $R/bench.py --steps 3 --warmup 1 --no-extras --blocks 1 --no-cpu-baseline --no-pmc --pmc-child"
rocprofv3 --kernel-trace --pmc FETCH_SIZE SQ_INSTS_VALU -d $O/${TAG}_fetch -o bench -- $P > $O/${TAG}_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE SQ_WAVES -d $O/${TAG}_write -o bench -- $P > $O/${TAG}_write.log 2>&1
S="python $R/bench.py --full --gpus 1 --steps 8 --warmup 2 --no-extras --no-cpu-baseline --no-pmc --dp-mode sharded --force-dp"
rocprofv3 --kernel-trace --stats -d $O/${TAG}_sharded_stats -o bench -- $S > $O/${TAG}_sharded_stats.log 2>&1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 -Wno-unused-value $R/tools/valu_rate.hip -o /tmp/valu_rate && /tmp/valu_rate > $O/${TAG}_valu_rate.txt 2>&1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 $R/tools/atomic_rate.hip -o /tmp/atomic_rate && /tmp/atomic_rate > $O/${TAG}_atomic_rate.txt 2>&1
cd $R
for k in stats sharded_stats; do db=$(find $O/${TAG}_$k -name '*.db' | head -1); python profiles/summarize_rocprof.py stats $db > $O/${TAG}_$k.txt; done
for k in fetch write; do db=$(find $O/${TAG}_$k -name '*.db' | head -1); python profiles/summarize_rocprof.py pmc $db > $O/${TAG}_$k.txt; done
find $O/${TAG}_stats $O/${TAG}_fetch $O/${TAG}_write $O/${TAG}_sharded_stats -name '*.db' -delete
python bench.py --full > $O/${TAG}_bench_s2.json 2> $O/${TAG}_bench_s2.err
python bench.py --full --scene S1 --no-cpu-baseline --no-pmc > $O/${TAG}_bench_s1.json 2>/dev/null
python bench.py --full --scene S3 --no-cpu-baseline --no-pmc > $O/${TAG}_bench_s3.json 2>/dev/null
python tools/ablate_k11.py 2>&1 | grep -v amdgpu > $O/${TAG}_k11_ablation.txt
python tools/time_densify.py 2>&1 | grep -v amdgpu > $O/${TAG}_time_densify.txt
head -14 $O/${TAG}_stats.txt
