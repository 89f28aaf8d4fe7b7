set -e
o=${RSLRL_OUT_DIR:-out}/r3f
mkdir -p $o
timeout -k 10 400 python bench.py --full > $o/bench_default.json 2> $o/bench_default.err
timeout -k 10 200 python bench.py --full --global-num-envs 16384 --no-extra --no-cpu-baseline > $o/b16k.json 2> $o/b16k.err
timeout -k 10 200 python bench.py --full --global-num-envs 32768 --no-extra --no-cpu-baseline --steps 10 > $o/b32k.json 2> $o/b32k.err
bash scripts/profile_round.sh
