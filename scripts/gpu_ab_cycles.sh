# usage: bash scripts/gpu_ab_cycles.sh name=lib.so[,VAR=VALUE] ...   (on one MI355X) — A/B in kernel CYCLES (GRBM_GUI_ACTIVE per dispatch, a PMC pass of its own per
# library, never mixed with tracing), two rounds; the per-scene figure is the median over the steady dispatches (the first 4 of each scene dropped).
# The passes' output goes to $CTR_AB_OUT (default: ab_cycles_out in the repository root).  Every pass runs under a time limit of its own, and the first
# one that fails ends the script: nothing more is started on a GPU that a pass may have left in a bad state.
REPO=$(pwd)
OUT=${CTR_AB_OUT:-$REPO/ab_cycles_out}
mkdir -p $OUT
export CTR_AB_OUT=$OUT
cd /tmp && export TMPDIR=/tmp
for round in 1 2; do
  for spec in "$@"; do
    name=${spec%%=*}; lib=${spec#*=}
    # name=lib.so,VAR=VALUE: that library with VAR=VALUE in the environment of its pass alone (a switch read when a handle is created)
    setting=; case "$lib" in *,*) setting=${lib#*,}; lib=${lib%%,*};; esac
    if [ -n "$setting" ]; then export "$setting"; fi
    export CUTRACE_AMD_LIB=$REPO/$lib
    timeout -k 10 400 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d $OUT/${name}_$round -o pmc -- python3 $REPO/scripts/render_loop.py > $OUT/${name}_$round.log 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then tail -3 $OUT/${name}_$round.log; echo "gpu_ab_cycles: $name, round $round ended with status $rc: stopping"; exit $rc; fi
    if [ -n "$setting" ]; then unset "${setting%%=*}"; fi
  done
done
cd $REPO
python3 - "$@" <<'PY'
import csv, glob, os, statistics, sys, collections
names = [a.split("=")[0] for a in sys.argv[1:]]
# render_loop.py's order: bunny 34 dispatches, 64 000 triangles 20, C3-deep 20 (all 1920x1080), C4 12 (4096x4096); the first 4 of each are warm-up
PLAN = (("bunny", 34), ("dense64k", 20), ("c3deep", 20), ("c4", 12))
res = collections.defaultdict(dict)
for rnd in (1, 2):
    for n in names:
        rows = []
        for f in glob.glob(os.path.join(os.environ["CTR_AB_OUT"], f"{n}_{rnd}", "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "render_kernel" in row["Kernel_Name"] and row["Counter_Name"] == "GRBM_GUI_ACTIVE":
                    rows.append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
        v = [c for _, c in sorted(rows)]
        out, at = [], 0
        for scene, cnt in PLAN:
            part = v[at + 4:at + cnt]; at += cnt
            if part:
                m = statistics.median(part) / 1e6
                res[scene].setdefault(n, []).append(m)
                out.append(f"{scene} {m:.4f}")
        print(f"round {rnd} {n}: " + "  ".join(out) + "   (Mcycles, GRBM_GUI_ACTIVE summed over the XCDs, median of the steady dispatches)", flush=True)
print("---- relative to the first library (mean of the rounds) ----")
for scene, _ in PLAN:
    base = statistics.mean(res[scene][names[0]])
    print(scene, "  ".join(f"{n} {100 * (statistics.mean(res[scene][n]) / base - 1):+.2f}%" for n in names if n in res[scene]))
PY
