#!/usr/bin/env bash
# Multi-GPU evaluation launcher with the reference's argument order (tools/dist_test.sh there):
#     bash tools/dist_test.sh CONFIG CHECKPOINT GPUS [test.py args ...]
# env: PORT (default 29500), MASTER_ADDR (default 127.0.0.1), NNODES / NODE_RANK (default 1 / 0).
# One process per GPU; rank r scores the samples r, r + GPUS, ... and one all-reduce sums the confusion counts
# (vfmseg_amd/evaluation.py).  Rank 0 prints the result.  Single node goes through tools/dist_launch.py.
set -euo pipefail
CONFIG=$1
CHECKPOINT=$2
GPUS=$3
NNODES=${NNODES:-1}
NODE_RANK=${NODE_RANK:-0}
PORT=${PORT:-29500}
MASTER_ADDR=${MASTER_ADDR:-"127.0.0.1"}
HERE="$(cd "$(dirname "$0")" && pwd)"
export PYTHONPATH="$HERE/..":${PYTHONPATH:-}
export HSA_ENABLE_IPC_MODE_LEGACY=${HSA_ENABLE_IPC_MODE_LEGACY:-0}
if [ "$NNODES" = "1" ]; then
    MASTER_ADDR=$MASTER_ADDR python "$HERE/dist_launch.py" --nproc "$GPUS" --port "$PORT" \
        "$HERE/test.py" "$CONFIG" "$CHECKPOINT" --launcher pytorch "${@:4}"
else
    python -m torch.distributed.run --nnodes="$NNODES" --node_rank="$NODE_RANK" --master_addr="$MASTER_ADDR" \
        --nproc_per_node="$GPUS" --master_port="$PORT" "$HERE/test.py" "$CONFIG" "$CHECKPOINT" --launcher pytorch "${@:4}"
fi
