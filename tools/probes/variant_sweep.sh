# Diagnostic: the same step / kernels with libsdamd.so variants built under variants/ (compiler scheduling strategies).
# Usage: bash tools/probes/variant_sweep.sh default max-ilp ...        (every run under its own time limit; the first failure ends the script)
. "$(dirname "$0")/libswap.sh"
for V in "$@"; do
  use_lib "$V"
  echo "== $V"
  OUT=$(timeout -k 10 120 python tools/bench_conv.py 2>/dev/null)
  echo "$OUT" | grep -E " (full|flat|plain) |wgrad " | grep -v perm
  OUT=$(timeout -k 10 120 python tools/step_series.py 60 4 2>/dev/null)
  echo "$OUT" | tail -1
done
