# Diagnostic: free-running step period (tools/step_series.py) for (library variant, engine-switch setting) pairs, alternating.
# Usage: bash tools/probes/ab_step.sh rounds "variant:ENV=... ENV=..." ...
#   variant   a library under variants/; empty = the tree's own library
#   settings  SDA_ENGINE_<switch>=<literal> ...; empty = defaults          ("old:" "new:" / ":A=1 B=2" ":" / "v2:SDA_ENGINE_x=False")
# Every run has its own time limit; the first one that fails ends the script (libswap.sh).
. "$(dirname "$0")/libswap.sh"
ROUNDS=$1; shift
for i in $(seq "$ROUNDS"); do
  for P in "$@"; do
    case "$P" in *:*) V=${P%%:*}; S=${P#*:} ;; *) V=$P; S= ;; esac
    use_lib "$V"
    OUT=$(env $S timeout -k 10 120 python tools/step_series.py 60 4 2>/dev/null)
    echo "== ${V:-tree} [$S]: $(echo "$OUT" | tail -1)"
  done
done
