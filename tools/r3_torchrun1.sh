set -e
OUT=${OUT:-bench_out}
cd "$(dirname "$0")/.." && mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 1 --steps 3 --warmup 1 --full --no-cpu-baseline --no-kernel-timing > "$OUT"/torchrun1.json 2> "$OUT"/torchrun1.err || { tail -30 "$OUT"/torchrun1.err; exit 1; }
OUT="$OUT" python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ['OUT'], 'torchrun1.json')).read().strip().splitlines()[-1])
print(d['value'], d['n_gpus'], d['config'].get('collective_backend'))
e = d['extra']
for k in ('xe_train', 'xe_train_strong', 'grad_allreduce', 'rl_iteration'):
    print(k, e.get(k))
PY
