#!/bin/bash
# SQ counter passes for one program and the kernels whose names match a filter (diagnostic):
#     bash tools/pmc_sq.sh <tag> <kernel-name regex> <program.py> [program args...]     ->  $OUT_DIR/sq_<tag>/  (OUT_DIR: build/profiling unless set)
#     bash tools/pmc_sq.sh w320 'conv_gemm|wgrad_gemm|conv3_flat' tools/conv_one.py wgrad 320 320 3 4
#     bash tools/pmc_sq.sh sim2048 sim_gemm tools/probes/sim_one.py 2048 256
# Three rocprofv3 --pmc passes (counters only, no other tracing beside the kernel names), each under its own time limit; a pass
# that fails ends the script.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
tag=$1; filter=$2; prog=$R/$3; shift 3
out=${OUT_DIR:-$R/build/profiling}/sq_$tag
cd /tmp && export TMPDIR=/tmp
pass() { p=$1; shift; timeout -k 10 300 rocprofv3 --kernel-trace --pmc "$@" -d "$out/$p" -o "$p" --output-format csv -- python3 "$prog" "${ARGS[@]}" > /dev/null 2>&1; }
ARGS=("$@")
pass p1 SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU &&
pass p2 SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_SCA SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INST_CYCLES_VMEM_RD SQ_VMEM_TA_ADDR_FIFO_FULL &&
pass p3 SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM SQ_INSTS_SALU SQ_VMEM_TA_CMD_FIFO_FULL SQ_LDS_CMD_FIFO_FULL SQ_LDS_DATA_FIFO_FULL ||
  exit $?
python3 - "$tag" "$filter" "$out" <<'PY'
import collections, csv, glob, re, sys
tag, flt, out = sys.argv[1], re.compile(sys.argv[2]), sys.argv[3]
for p in ("p1", "p2", "p3"):
    for f in glob.glob("%s/%s/**/*counter_collection.csv" % (out, p), recursive=True):
        acc = collections.defaultdict(lambda: [0.0, 0])
        for r in csv.DictReader(open(f)):
            if not flt.search(r["Kernel_Name"]): continue
            a = acc[r["Counter_Name"]]; a[0] += float(r["Counter_Value"]); a[1] += 1
        for c, (v, n) in sorted(acc.items()):
            print("%s %-32s %14.0f per launch (n=%d)" % (tag, c, v / n, n))
PY
