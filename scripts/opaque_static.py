#!/usr/bin/env python3
"""Resource table of the one-mesh render kernel instantiations from two compiler remark logs (parent, this tree).

Each log is the stderr of render_kernel.hip compiled with the flags of cutrace_amd/build.py plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`.  Prints, per instantiation render_kernel<KV, 1, ROOM, OPQ>,
VGPRs, SGPR spills, scratch, LDS per wave at bounces 5 (the recursion stack, plus the PARK granule where the build has one)
and the waves per SIMD the registers and that LDS allow; then whether every instantiation the parent also has kept its figures.

  python scripts/opaque_static.py parent_remarks.txt tree_remarks.txt
"""
import re
import sys

NAME = re.compile(r"render_kernelILj(\d+)ELj(\d+)ELb(\d)E(?:Lj(\d+)E)?E")
FIELDS = {"VGPRs": "vgpr", "SGPRs Spill": "sspill", "VGPRs Spill": "vspill", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ"}
KV_OCC6 = 64
LDS_CU, GRANULE = 160 * 1024, 1280


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        if "remark:" not in line:
            continue
        text = line.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if text.startswith("Function Name:"):
            m = NAME.search(text)
            cur = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4) or 0)) if m else None
            if cur:
                out[cur] = {}
            continue
        if cur is None:
            continue
        for label, key in FIELDS.items():
            if text.startswith(label + ":"):
                out[cur][key] = int(text.split(":")[1])
    return out


def lds_per_wave(kv, opq, bounces=5):
    return bounces * 4 * 256 + (GRANULE if kv & KV_OCC6 else 0)   # kernel_choice.h lds_bytes_per_wave: whatever the opaque build


def waves(r, kv, opq):
    by_lds = LDS_CU // (-(-lds_per_wave(kv, opq) // GRANULE) * GRANULE) // 4
    return min(r["occ"], by_lds)


def main():
    parent, tree = parse(sys.argv[1]), parse(sys.argv[2])
    print("build, room, opq      VGPRs  sgpr_spill  vgpr_spill  scratch  LDS/wave (b5)  waves/SIMD")
    for key in sorted(k for k in tree if k[1] == 1):
        kv, _, room, opq = key
        for tag, tab in (("parent", parent), ("tree", tree)):
            r = tab.get(key if tag == "tree" else key[:3] + (0,))
            if r is None or (tag == "parent" and opq != 0):
                continue
            print(f"{kv:4d} room {room} opq {opq} {tag:6s} {r['vgpr']:5d} {r['sspill']:11d} {r['vspill']:11d} {r['scratch']:8d} {lds_per_wave(kv, opq):14d} {waves(r, kv, opq):11d}")
    changed = [k for k in parent if tree.get(k) != parent[k]]
    print(f"instantiations of the parent: {len(parent)}; with other figures in this tree: {len(changed)} {sorted(changed) if changed else ''}")
    print(f"instantiations added by this tree: {len(tree) - len(parent)}")


if __name__ == "__main__":
    main()
