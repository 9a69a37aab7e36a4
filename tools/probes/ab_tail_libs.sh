# Diagnostic: the tail products alone (tools/probes/bench_tail.py) and the free-running step for library variants under variants/
# Usage: bash tools/probes/ab_tail_libs.sh a b c        (every run under its own time limit; the first failure ends the script)
. "$(dirname "$0")/libswap.sh"
for V in "$@"; do
  use_lib "$V"
  OUT=$(timeout -k 10 120 python tools/probes/bench_tail.py 2>/dev/null)
  echo "== $V"; echo "$OUT" | grep -v amdgpu
done
bash tools/probes/ab_step.sh 2 "${@/%/:}"
