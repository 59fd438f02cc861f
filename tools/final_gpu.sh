# bash tools/final_gpu.sh OUT_DIR: whole GPU suite, smoke, torchrun world-1 bench line (--full), logs under OUT_DIR
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: bash tools/final_gpu.sh OUT_DIR}" && cd "$1" && pwd)
cd $R
( timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -6 ) | tee $O/pytest_gpu.log
( timeout 600 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -3 ) | tee $O/smoke.log
( timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 20 --warmup 3 --full 2> $O/torchrun.err | tail -1 ) > $O/bench_torchrun_world1.json
python - $O/bench_torchrun_world1.json <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['n_gpus'], json.dumps(d.get('multi_gpu',{}).get('replicas'))[:600])
P
