#!/bin/bash
# samples rocm-smi (power, clocks, temperature; read-only) every 0.7 s while a workload runs: is the step power-capped?
# usage: scripts/power_probe.sh [-- COMMAND...]   -> the file `out` below; the exit status is the workload's
#   without a command: python bench.py --no-cpu-baseline --steps 150 --warmup 5
#   the wide step:     scripts/power_probe.sh -- python scripts/kbench.py 2048 512 8 12
# The workload runs under `timeout -k 10 600` with its stderr shown.
out=gpurun_out/power_probe.txt
mkdir -p gpurun_out
run=${out%.txt}_run.txt
if [ $# = 0 ]; then set -- python bench.py --no-cpu-baseline --steps 150 --warmup 5; bench=1
elif [ "$1" = "--" ] && [ $# -gt 1 ]; then shift; bench=0
else echo "usage: scripts/power_probe.sh [-- COMMAND...]" >&2; exit 2; fi
timeout -k 10 600 "$@" > $run &
bp=$!
sleep 4
while kill -0 $bp 2>/dev/null; do
  rocm-smi --showpower --showclocks --showtemp 2>/dev/null | grep -E "Power|sclk|mclk|Temperature \(Sensor (edge|junction|hotspot)" | tr -s ' ' | tr '\n' ';'
  echo
  sleep 0.7
done > $out
wait $bp
status=$?
echo "idle:" >> $out
sleep 2
rocm-smi --showpower --showclocks 2>/dev/null | grep -E "Power|sclk|mclk" | tr -s ' ' | tr '\n' ';' >> $out
echo >> $out
rocm-smi --showmaxpower 2>/dev/null | grep -i "power" >> $out
cat $out
if [ $bench = 1 ] && [ $status = 0 ]; then
  tail -n 1 $run | python -c "
import json, sys; d = json.loads(sys.stdin.read()); print('bench', d['value'], d['ms_per_step'])"
else tail -n 3 $run; fi
exit $status
