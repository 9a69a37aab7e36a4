# Diagnostic: the emulated N-rank step (bench.py --emulate-world 8 --emulate-no-copy) for library variants under variants/, alternating
# Usage: bash tools/probes/ab_emul_libs.sh rounds v1 v2 ...        (every run under its own time limit; the first failure ends the script)
. "$(dirname "$0")/libswap.sh"
ROUNDS=$1; shift
for i in $(seq "$ROUNDS"); do
  for V in "$@"; do
    use_lib "$V"
    OUT=$(timeout -k 10 200 python bench.py --emulate-world 8 --emulate-no-copy --steps 20 --warmup 5 2>/dev/null)
    echo "== $V: $(echo "$OUT" | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['host_enqueue_ms_per_step'])")"
  done
done
