# Bench A/B of the launch-bound loss-kernel events (RSLRL_BENCH_LAUNCH_EVENTS=0 vs default), alternating on one box.
set -e
o=${RSLRL_OUT_DIR:-out}/evab
mkdir -p $o
for r in 1 2; do
  for w in 0 1; do
    RSLRL_BENCH_LAUNCH_EVENTS=$w timeout -k 10 200 python bench.py --full --no-extra --no-cpu-baseline --steps 20 > $o/r${r}_$w.json 2> $o/r${r}_$w.err
  done
done
