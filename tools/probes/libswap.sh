# Sourced by the library-variant probes.  Stops the script at the first command that fails (a fault, an abort, a time limit and a
# plain error alike: nothing more is started on the GPU), goes to the repository root, and gives use_lib <variant>: run on
# variants/libsdamd_<variant>.so, or on the tree's own library when <variant> is empty.  The tree's own library is put back on exit.
set -eu -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/../.."
LIB=speech_decoding_amd/libsdamd.so
KEEP=$(mktemp)
cp "$LIB" "$KEEP"
trap 'cp "$KEEP" "$LIB"; rm -f "$KEEP"' EXIT
use_lib() { if [ -n "$1" ]; then cp "variants/libsdamd_$1.so" "$LIB"; else cp "$KEEP" "$LIB"; fi; }
