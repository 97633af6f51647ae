"""Static comparison of the launch shapes of the render kernel (kernel_choice.h KS_*), without a GPU: the registers, spills and
scratch of every build of CTR_SHAPE_KERNELS in both shapes, and the instructions a bunny frame issues in each, priced the way
scripts/dynamic_mix.py does — segment executions (a committed profile of the general shape: a shape only removes code, so a
segment that is left runs as often as before) x the segment's static instruction counts.

usage: shape_static.py <parent_marks.s> <new_marks.s> <new_plain.s> <counts.json> [build ...]
  *_marks.s : render_kernel.hip compiled with -DCTR_MARKS -S --cuda-device-only and the flags of cutrace_amd/build.py, of the parent
              commit and of this tree; new_plain.s: this tree without -DCTR_MARKS (the registers of the shipped code)
  build     : the KV whose mix is priced (default 107, the bunny frame's)"""
import json, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynamic_mix

BUILDS = (43, 107, 171, 235)   # CTR_SHAPE_KERNELS: default variant, | KV_OCC6 (64), | KV_HOSTOUT (128), | both
MARKS = (8, 13, 16)            # after the planes / before the top-level walk / the leaf's bookkeeping


def resources(path):
    """{(kv, shape): dict} from the code-object metadata of an assembly file; shape None = a one-parameter name"""
    text, out = open(path).read(), {}
    for m in re.finditer(r"\.name:\s+_ZN12_GLOBAL__N_113render_kernelILj(\d+)E(?:Lj(\d+)E)?EEv\S+\n(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        blk = m.group(3)
        get = lambda key: int(re.search(key + r":\s+(\d+)", blk).group(1))
        out[(int(m.group(1)), int(m.group(2) or 0))] = dict(NumVgprs=get(r"\.vgpr_count"), sgpr_spill_count=get(r"\.sgpr_spill_count"),
                                                            vgpr_spill_count=int(m.group(4)), ScratchSize=get(r"\.private_segment_fixed_size"))
    for m in re.finditer(r"^_ZN12_GLOBAL__N_113render_kernelILj(\d+)E(?:Lj(\d+)E)?EEv[^\n]*:.*?^; Occupancy: (\d+)", text, re.S | re.M):
        key = (int(m.group(1)), int(m.group(2) or 0))
        if key in out:
            out[key]["Occupancy"] = int(m.group(3))
    return out


def mix(path, kv, counts):
    seg = dynamic_mix.segments(dynamic_mix.kernel_body(path, kv))
    tot = dict(F=0.0, H=0.0, Q=0.0, salu=0.0, branch=0.0, smem=0.0, nop=0.0)
    marks = {}
    for i, d in seg.items():
        n = counts.get(i, 0.0)
        for k in tot:
            tot[k] += n * d[k] / d["copies"]
        marks[i] = n * sum(d[k] for k in ("F", "H", "Q", "salu", "branch", "smem", "vmem", "lds", "nop")) / d["copies"]
    valu = tot["F"] + tot["H"] + tot["Q"]
    cyc = dynamic_mix.F * tot["F"] + dynamic_mix.H * tot["H"] + dynamic_mix.Q * tot["Q"]
    return dict(scalar=tot["salu"] + tot["branch"] + tot["smem"] + tot["nop"], salu=tot["salu"], branch=tot["branch"], smem=tot["smem"],
                nop=tot["nop"], valu=valu, issue=cyc, marks=marks)


def main():
    parent_s, new_s, plain_s, counts_path = sys.argv[1:5]
    priced = [int(x) for x in sys.argv[5:]] or [107]
    counts = {int(k): float(v) for k, v in json.load(open(counts_path))["per_launch"].items()}
    M = 1e6
    for kv in priced:
        cols = (("parent", mix(parent_s, str(kv), counts)), ("shape 0", mix(new_s, str(kv), counts)), ("shape 1", mix(new_s, "%d,1" % kv, counts)))
        base = cols[0][1]
        print("render_kernel<%d>, per launch of %s, millions of instructions (segment executions: %s)" % (kv, "bunny.json 1920x1080 b5", os.path.basename(counts_path)))
        print("%-44s" % "" + "".join("%22s" % n for n, _ in cols))
        rows = (("scalar side (SALU + branch + SMEM + nop)", "scalar"), ("  SALU", "salu"), ("  branches", "branch"), ("  SMEM", "smem"), ("  s_nop", "nop"),
                ("VALU", "valu"), ("VALU issue cycles (F 2.2, H 4.1, Q 8.1)", "issue"))
        for label, key in rows:
            print("%-44s" % label + "".join("%13.1f (%+5.1f%%)" % (c[key] / M, 100 * (c[key] / base[key] - 1)) for _, c in cols))
        for mk in MARKS:
            print("%-44s" % ("mark %d, all instructions" % mk) + "".join("%13.1f         " % (c["marks"].get(mk, 0.0) / M) for _, c in cols))
        print()
    print("registers of the builds of CTR_SHAPE_KERNELS (shipped code, no marks): shape 0 -> shape 1")
    res = resources(plain_s)
    keys = ("NumVgprs", "sgpr_spill_count", "vgpr_spill_count", "ScratchSize", "Occupancy")
    print("%-8s" % "build" + "".join("%22s" % k for k in keys))
    ok = True
    for kv in BUILDS:
        a, b = res[(kv, 0)], res[(kv, 1)]
        print("%-8d" % kv + "".join("%22s" % ("%d -> %d" % (a[k], b[k])) for k in keys))
        ok = ok and b["sgpr_spill_count"] <= a["sgpr_spill_count"] and b["vgpr_spill_count"] <= a["vgpr_spill_count"] and b["ScratchSize"] <= a["ScratchSize"]
        if kv & 64:
            ok = ok and b["NumVgprs"] <= 80 and b["ScratchSize"] == 0
    print("rule (6-wave builds: <= 80 VGPRs, no scratch; no build spills more than its shape 0 twin):", "held" if ok else "BROKEN")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
