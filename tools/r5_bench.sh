#!/bin/bash
# the full bench line, then the whole bench under a one-rank RCCL group (the data-parallel code paths)
set -o pipefail
OUT=${OUT:-bench_out}/r5bench
mkdir -p "$OUT"
timeout -k 10 900 python bench.py --full > "$OUT"/bench.json 2> "$OUT"/bench.err
echo "bench rc=$?"
tail -c 1500 "$OUT"/bench.json; echo
grep "bench " "$OUT"/bench.err | tail -30
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29611 bench.py --gpus 1 --steps 3 --warmup 2 --full --no-cpu-baseline > "$OUT"/bench_rank1.json 2> "$OUT"/bench_rank1.err
echo "torchrun rc=$?"
tail -c 1200 "$OUT"/bench_rank1.json; echo
