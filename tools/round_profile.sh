# rocprofv3 kernel stats of the captured step and of the training step, and the bench line with its side measurements (--full).
#   usage: bash tools/round_profile.sh <tag, e.g. r03_v1> "<description>" <output folder>
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r03_v1}
DESC=${2:-"round 3"}
O=$(realpath -m "${3:?usage: bash tools/round_profile.sh <tag> <description> <output folder>}")
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_$TAG $O/proft_$TAG
timeout 400 rocprofv3 --kernel-trace --stats -d $O/prof_$TAG -o p -- python $R/bench.py --steps 5 --warmup 1 --step-only > $O/prof_$TAG.log 2>&1
timeout 400 rocprofv3 --kernel-trace --stats -d $O/proft_$TAG -o p -- python $R/bench.py --train --steps 5 --warmup 2 > $O/proft_$TAG.log 2>&1
cd $R
DB=$(find $O/prof_$TAG -name "*.db" | head -1)
python tools/prof_summary.py $DB 7 "rocprofv3 --kernel-trace --stats -- python bench.py --steps 5 --warmup 1 --step-only ($DESC; MI355X, batch 32, La=32)" > $O/${TAG}_bench_kernel_stats.txt
DB=$(find $O/proft_$TAG -name "*.db" | head -1)
python tools/prof_summary.py $DB 8 "rocprofv3 --kernel-trace --stats -- python bench.py --train --steps 5 --warmup 2 ($DESC; cfg 5: per-GPU batch 4, bf16, graph-replayed micro-step)" > $O/${TAG}_train_kernel_stats.txt
timeout 600 python bench.py --full > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
tail -c 1500 $O/${TAG}_bench.json; head -14 $O/${TAG}_bench_kernel_stats.txt | cut -c1-150; head -24 $O/${TAG}_train_kernel_stats.txt | cut -c1-150
rm -rf $O/prof_$TAG $O/proft_$TAG
