#!/bin/bash
# one rank through the launcher with the RCCL backend: the exact command shape the driver uses for N > 1
set -e
out=${1:?usage: rehearse1_nccl.sh OUTPUT_DIR}
mkdir -p "$out"
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29519 bench.py --gpus 1 --steps 50 --warmup 5 --full --no-mt6 --no-cpu-baseline > "$out/rehearse1.json" 2> "$out/rehearse1.err" || { tail -20 "$out/rehearse1.err"; exit 1; }
python - "$out" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1] + '/rehearse1.json').read().strip().splitlines()[-1])
print({k: d[k] for k in ('n_gpus', 'value', 'ms_per_step', 'rmse', 'nll', 'inclination_indicator', 'trajectories_aggregated')})
PY
