#!/bin/bash
# GPU box: address-unit (TA) and L1 (TCP) counters of the default bench line's kernels, in counter runs of their own (rocprofv3
# --pmc, four passes), summarised per kernel and launch -- for builds of the library side by side.
#   usage: bash profiles/tools/pmc_ta.sh [variant.so ...]   (paths under the repository, e.g. ab/base.so; none: the tree's build)
#   PMC_TA_OUT: where the passes and summaries go (default build/ta under the repository)
# ONE counter of a block a pass: four TA counters in one pass are more than the block has slots for ("Request exceeds the
# capabilities of the hardware to collect", and rocprofv3 aborts before the first kernel).
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
export TMPDIR=/tmp; cd /tmp
PASSES=${PMC_TA_PASSES:-"1 2 3 4"}
[ $# -eq 0 ] && set -- ""
for v in "$@"; do
    name=$(basename "${v:-tree}" .so)
    OUT=${PMC_TA_OUT:-$ROOT/build/ta}/$name
    mkdir -p $OUT
    BENCH="python3 $ROOT/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extra-legs ${v:+--library $ROOT/$v}"
    for p in $PASSES; do
        case $p in
            1) PMC="TA_TA_BUSY_sum TCP_TAGRAM0_REQ_sum GRBM_GUI_ACTIVE";;
            2) PMC="TA_FLAT_READ_WAVEFRONTS_sum TCP_TCC_READ_REQ_sum GRBM_GUI_ACTIVE";;
            3) PMC="TA_ADDR_STALLED_BY_TC_CYCLES_sum TCP_PENDING_STALL_CYCLES_sum GRBM_GUI_ACTIVE";;
            4) PMC="TA_DATA_STALLED_BY_TC_CYCLES_sum TCP_READ_TAGCONFLICT_STALL_CYCLES_sum GRBM_GUI_ACTIVE";;
        esac
        echo "$name pass $p: $PMC"
        timeout -k 10 240 rocprofv3 --pmc $PMC --kernel-trace --output-format csv -d $OUT/p$p -o run -- $BENCH > /dev/null 2> $OUT/p$p.err || { st=$?; grep -m 3 -i "error\|exceeds" $OUT/p$p.err; tail -2 $OUT/p$p.err; exit $st; }
    done
    find $OUT -name '*kernel_trace.csv' -delete
    # per kernel and launch, in millions (the _sum counters add up every CU's unit)
    python3 - "$OUT" "$name" <<'PY' | tee "$OUT/summary.txt"
import collections, csv, glob, sys
for f in sorted(glob.glob(sys.argv[1] + "/p*/**/*counter_collection.csv", recursive=True)):
    acc = collections.defaultdict(lambda: collections.defaultdict(float)); calls = collections.defaultdict(set)
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")[:44]
        acc[k][r["Counter_Name"]] += float(r["Counter_Value"]); calls[k].add(r["Dispatch_Id"])
    for k, v in acc.items():
        n = len(calls[k])
        if v.get("GRBM_GUI_ACTIVE", 0) / n > 2e5:
            print("%s %-44s launches %2d  " % (sys.argv[2], k, n) + "  ".join("%s %.3f" % (c.replace("_sum", ""), x / n / 1e6) for c, x in sorted(v.items())))
PY
done
