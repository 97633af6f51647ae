#!/usr/bin/env python3
"""Static figures of the phased render kernel builds against their opaque parents, and the proof that nothing else moved.

Two directories of gfx950 assembly, each made by `scripts/isa_diff.py asm <tree> <dir> render_kernel.hip`: the parent commit's
and this tree's.

  python scripts/phase_static.py <parent_dir> <tree_dir>

1. Per opaque one-mesh instantiation render_kernel<KV, 1, ROOM, 1, DARK> — the parent's, this tree's with PHASED false and this
   tree's phased twin — from the compiler's own summary behind each kernel: code bytes, VGPRs, SGPRs, scratch, waves per SIMD;
   and counted from the text: VALU, SALU (branches and waits left out), SALU that reads or writes `exec`, global loads,
   v_readlane / v_writelane.
2. scripts/isa_diff.py over the two directories, with the sixth template argument of this tree dropped from the mangled names
   where it is false, so that every kernel the parent has is matched with itself.
"""
import os
import re
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_diff

NAME = re.compile(r"render_kernelILj(\d+)ELj(\d+)ELb(\d)ELj(\d)ELb(\d)E(?:Lb(\d)E)?EEv")
SUMMARY = {"codeLenInByte": r"; codeLenInByte = (\d+)", "vgpr": r"; NumVgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)",
           "scratch": r"; ScratchSize: (\d+)", "occ": r"; Occupancy: (\d+)"}


def figures(directory):
    """(kv, shape, room, opq, dark, phased) -> figures of every render_kernel instantiation of the directory's render_kernel.s"""
    lines = open(os.path.join(directory, "render_kernel.s")).read().split("\n")
    out = {}
    for a, l in enumerate(lines):
        m = NAME.search(l)
        if not (m and l.startswith("_ZN") and l.split(";")[0].rstrip().endswith(":")):
            continue
        key = tuple(int(g or 0) for g in m.groups())
        end = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d = dict(valu=0, salu=0, exec=0, gload=0, lane=0)
        for raw in lines[a:end]:
            t = raw.split(";")[0].strip()
            if t.startswith("v_"):
                d["valu"] += 1
                d["lane"] += t.startswith(("v_readlane", "v_writelane"))
            elif t.startswith("s_") and not t.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_nop", "s_endpgm", "s_load", "s_buffer_load")):
                d["salu"] += 1
                d["exec"] += bool(re.search(r"\bexec(_lo|_hi)?\b", t) or "saveexec" in t)
            elif t.startswith("global_load"):
                d["gload"] += 1
        tail = "\n".join(lines[end:end + 60])
        for k, pat in SUMMARY.items():
            d[k] = int(re.search(pat, tail).group(1))
        out[key] = d
    return out


def main():
    parent_dir, tree_dir = sys.argv[1:3]
    P, T = figures(parent_dir), figures(tree_dir)
    cols = ("codeLenInByte", "vgpr", "sgpr", "scratch", "occ", "valu", "salu", "exec", "gload", "lane")
    print("%-34s" % "render_kernel<KV,1,ROOM,1,DARK>" + "".join("%14s" % c for c in cols))
    bad = []
    for key in sorted(k for k in T if k[3] == 1 and k[5] == 1):
        kv, shape, room, opq, dark, _ = key
        rows = (("parent", P.get(key[:5] + (0,))), ("tree, PHASED false", T.get(key[:5] + (0,))), ("tree, PHASED true", T[key]))
        for tag, r in rows:
            if r is None:
                continue
            print("%4d room %d dark %d %-18s" % (kv, room, dark, tag) + "".join("%14d" % r[c] for c in cols))
        par, new = rows[0][1], rows[2][1]
        if new["scratch"] != 0 or (par and (new["occ"] < par["occ"] or (par["vgpr"] <= 80) != (new["vgpr"] <= 80))):
            bad.append(key)
    print("ScratchSize 0 in every instantiation of this tree:", all(r["scratch"] == 0 for r in T.values()))
    print("phased builds that use scratch or leave their parent's VGPR class (waves per SIMD):", bad or "none")
    print()
    # the comparison kernel by kernel, PHASED = false dropped from this tree's names
    tmp = tempfile.mkdtemp()
    try:
        text = open(os.path.join(tree_dir, "render_kernel.s")).read()
        text = re.sub(r"(render_kernelILj\d+ELj\d+ELb\dELj\dELb\dE)Lb0E(EEv)", r"\1\2", text)
        open(os.path.join(tmp, "render_kernel.s"), "w").write(text)
        isa_diff.diff(parent_dir, tmp)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
