# the lines gnan_amd.replay touches, once more after its last change (copies of static outputs, copyable models, plans for 129+ nodes)
#   bash tools/profile_replay_lines.sh OUT_DIR
OUT=${1:?usage: bash tools/profile_replay_lines.sh OUT_DIR}
mkdir -p $OUT
python3 tools/reference_loop_bench.py --profile > $OUT/reference_loop.jsonl 2> $OUT/reference_loop_host_profile.txt
python3 bench.py --full --config c3 > $OUT/c3_bench.log 2>&1
python3 bench.py --config c3 --loop reference --no-cpu-baseline > $OUT/c3_loop_reference.log 2>&1
python3 bench.py --full --config c2 --steps 3 --warmup 1 > $OUT/c2_bench.log 2>&1
python3 bench.py --config c2 --loop reference --no-cpu-baseline --steps 3 --warmup 1 > $OUT/c2_loop_reference.log 2>&1
python3 tools/graphed_step.py arxiv cora muta arxiv40 > $OUT/graphed_steps.log 2>&1
python3 bench.py --full > $OUT/bench_full.log 2>&1
cat $OUT/reference_loop.jsonl | cut -c1-300
