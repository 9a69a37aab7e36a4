# Diagnostic: per-kernel times of the bench step under rocprofv3 for library variants: bash tools/probes/prof_lib.sh old new
# -> $OUT_DIR/prof_<variant>.json and prof_<variant>_kernel_stats.csv
# (every run under its own time limit; the first failure ends the script)
. "$(dirname "$0")/libswap.sh"
R=$PWD
O=${OUT_DIR:-$R/build/profiling}        # (OUT_DIR: where the results go)
mkdir -p "$O"
export TMPDIR=/tmp
for V in "$@"; do
  use_lib "$V"
  rm -rf "$O/prof_$V"
  (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_$V" -o tr -- \
     python3 "$R/bench.py" --steps 10 --warmup 3 > "$O/prof_$V.json" 2> "$O/prof_$V.err")
  find "$O/prof_$V" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$O/prof_${V}_kernel_stats.csv"
  rm -rf "$O/prof_$V"
done
