set -u
# One replayed training step of each bench config, kernel by kernel (rocprofv3 --kernel-trace of a short
# bench.py run; tools/step_breakdown.py picks the step between two adam_rec_k launches); the trace
# databases are deleted afterwards (gpurun copies back at most 64 MiB).
# usage: bash tools/cmd_step_breakdown.sh <tag>
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=gpurun_out/$1; mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace -d $O/tb -o kt -- python3 bench.py --full --steps 8 --warmup 3 --no-cpu-baseline \
  --no-parity --no-roofline --no-conformer > $O/base.log 2>&1 || { tail -20 $O/base.log; exit 1; }
python3 tools/step_breakdown.py $O/tb 8 40 > $O/base_replay_step.txt 2>&1; head -3 $O/base_replay_step.txt
timeout -k 10 300 rocprofv3 --kernel-trace -d $O/tc -o kt -- python3 bench.py --config conformer --steps 8 --warmup 3 \
  --no-cpu-baseline --no-parity --no-roofline > $O/conf.log 2>&1 || { tail -20 $O/conf.log; exit 1; }
python3 tools/step_breakdown.py $O/tc 8 40 > $O/conformer_replay_step.txt 2>&1; head -3 $O/conformer_replay_step.txt
find $O -name "*.db" -delete; find $O -name "*.csv" -delete
