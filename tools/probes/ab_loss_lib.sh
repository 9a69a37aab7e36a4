# Diagnostic: loss-stage micro-benchmarks (tools/bench_loss.py) for library variants under variants/: bash tools/probes/ab_loss_lib.sh a b
# (every run under its own time limit; the first failure ends the script)
. "$(dirname "$0")/libswap.sh"
for V in "$@" "$@"; do
  use_lib "$V"
  OUT=$(timeout -k 10 100 python tools/bench_loss.py 2>/dev/null)
  echo "== $V"; echo "$OUT" | grep -E "Bm=|sim gemm|dZ gemm"
done
