"""Host logic (CPU, no GPU): what ctr_scene_create builds before it touches a device — flatten_scene
(cutrace_amd/csrc/scene_flatten.cpp) and the guard of the BVH culling (cutrace_amd/csrc/guard.cpp: plan_guards,
apply_guards) — run through scripts/flatten_check.cpp on the project's own scenes.  Properties that hold by construction,
no digests."""
import json
import os

import numpy as np
import pytest

import cutrace_amd
from cutrace_amd import scenes
from tests.checkers import CSRC, harness, run  # noqa: F401  (harness: the fixture that builds scripts/flatten_check.cpp)
from tests.util import _random_scene, _multi_mesh_scene, parse

GUARD_SLOTS = 64          # CTR_GUARD_SLOTS
LEAF, PAD = 0x80000000, 0xFFFFFFFF   # BVH_LEAF_FLAG, CTR_PLANE_PAD
OBJ_TRIANGLE, OBJ_MESH, OBJ_PLANE, OBJ_SPHERE, OBJ_MERGED = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- flatten_scene

def check_flat(flat, desc):
    """The layout rules of scene_device.h / scene_flatten.h on one flattened scene."""
    objs, sc = flat["objs"], flat["scalars"]
    n_obj = len(objs)
    assert n_obj == desc.n_objects and list(objs["index"]) == list(range(n_obj))
    # every object lands in exactly one of plane records, oloop and meshes[0:n_mesh]; empty meshes land in none
    in_planes = [int(i) for i in flat["planes"]["index"].ravel() if i != PAD]
    in_oloop = [int(i) for i in flat["oloop"]["index"]]
    in_meshes = [int(i) for i in flat["meshes"]["index"][:sc["n_mesh"]]]
    assert sorted(in_planes) == [i for i in range(n_obj) if objs["type"][i] == OBJ_PLANE]
    assert in_oloop == [i for i in range(n_obj) if objs["type"][i] in (OBJ_TRIANGLE, OBJ_SPHERE)]   # scene order
    assert sorted(in_meshes) == [i for i in range(n_obj) if objs["type"][i] == OBJ_MESH and objs["tri_count"][i] > 0]
    assert sc["has_mesh"] == int((objs["type"] == OBJ_MESH).any())
    assert sc["mesh_tris"] == int(objs["tri_count"][objs["type"] == OBJ_MESH].sum())
    # meshes: leaf order is a permutation of the file order, normals in file order, spare records, child descriptors in range
    tris, gn, nodes4 = flat["tris"], flat["gn"].reshape(-1, 4), flat["nodes4"]
    guards = {g["obj_index"]: g for g in flat["guards"]}
    for i in range(n_obj):
        if objs["type"][i] != OBJ_MESH:
            continue
        O, g = objs[i], guards[i]
        n, t0 = int(O["tri_count"]), int(O["tri_begin"])
        assert (g["tri_begin"], g["tri_count"], g["node_begin"], g["node_count"]) == (t0, n, O["node_begin"], O["node_count"])
        assert (g["mesh_pos"] == PAD) == (n == 0) and O["bvh_root"] == 0
        if n == 0:
            continue
        assert flat["meshes"]["index"][g["mesh_pos"]] == i
        orig = tris["orig"][t0:t0 + n]
        assert sorted(orig) == list(range(n))
        src = np.array([[[getattr(getattr(desc.triangles[desc.objects[i].tri_begin + int(k)], p), c) for c in "xyz"] for p in ("p1", "p2", "p3")]
                        for k in range(n)], np.float32)
        assert np.array_equal(tris["p"][t0:t0 + n], src[orig, 1])                       # the record of file triangle orig[k]: p2 ...
        assert np.array_equal(tris["ab"][t0:t0 + n, :, 0], src[orig, 1] - src[orig, 0])  # ... a = p2 - p1 ...
        assert np.array_equal(tris["ab"][t0:t0 + n, :, 1], src[orig, 1] - src[orig, 2])  # ... b = p2 - p3, each rounded once
        # gn[tri_begin + file index] = -normalize((p2 - p3) x (p1 - p3)) = -normalize(a x b) of THAT file triangle
        nrm = np.cross((src[:, 1] - src[:, 0]).astype(np.float64), (src[:, 1] - src[:, 2]).astype(np.float64))
        ok = np.linalg.norm(nrm, axis=1) > 1e-12
        want = -nrm[ok] / np.linalg.norm(nrm[ok], axis=1)[:, None]
        assert np.abs(gn[t0:t0 + n, :3][ok] - want).max() < 1e-3 and (gn[t0:t0 + n, 3] == 0).all()
        for k in range(GUARD_SLOTS):                                                     # unused guard records repeat the first triangle
            assert tris[t0 + n + k].tobytes() == tris[t0].tobytes() and gn[t0 + n + k].tobytes() == gn[t0].tobytes()
        nb, nc = int(O["node_begin"]), int(O["node_count"])
        assert nc >= 1 and not nodes4[nb + nc].tobytes().strip(b"\0")                    # the spare node: all zero until a guard needs it
        covered = np.zeros(n, int)
        for c in nodes4["child"][nb:nb + nc].ravel():
            if c & LEAF:
                first, cnt = int(c & 0xFFFFFF), int((c >> 24) & 0x7F)
                assert first + cnt <= n
                covered[first:first + cnt] += 1
            else:
                assert 0 < c < nc
        assert (covered == 1).all()
    # stand-alone triangles: one record each, file index 0
    for i in range(n_obj):
        if objs["type"][i] == OBJ_TRIANGLE:
            assert objs["tri_count"][i] == 1 and tris["orig"][objs["tri_begin"][i]] == 0
    check_planes(flat)
    # the merged tree's room: 2..255 non-empty meshes
    n_mesh = sc["n_mesh"]
    assert sc["merged_reserved"] == int(2 <= n_mesh <= 255)
    if sc["merged_reserved"]:
        assert len(flat["meshes"]) == 2 * n_mesh + 1 and flat["meshes"]["type"][n_mesh] == OBJ_MERGED
        assert [int(i) for i in flat["meshes"]["index"][n_mesh + 1:]] == sorted(in_meshes)   # scene order
        assert sc["merged_tri_count"] == sc["mesh_tris"] and sc["merged_tri_begin"] + sc["merged_tri_count"] + GUARD_SLOTS == len(tris)
    else:
        assert len(flat["meshes"]) == n_mesh
    assert len(gn) == len(tris)
    assert sc["mesh_bytes"] == 64 * len(tris) + len(flat["nodes"]) + 128 * len(nodes4)
    # materials: the thresholds scene_flatten.h documents
    tr, rf = flat["mats"]["transparency"].astype(np.float64), flat["mats"]["reflexivity"].astype(np.float64)
    assert sc["all_opaque"] == int((flat["mats"]["transparency"] == 0).all())
    assert sc["need_cold"] == int(((tr >= 1e-6) & (rf >= 1e-6)).any())
    assert sc["any_bounce"] == int(((tr >= 1e-6) | (rf >= 1e-6)).any())
    for i in range(n_obj):                                                               # f[7]: the object's material is transparent
        assert objs["f"][i, 7:8].view("u4")[0] == int(tr[objs["mat"][i]] >= 1e-6)


def worst_stack(child, root):
    """The highest the walk of ray_walk.h can stack on a tree: a visited node pushes all of its entered inner children but
    the one it goes to next, so no lane holds more than the maximum over root-to-node paths of the sum of
    (inner children - 1) along the path.  `child`: the (n, 4) child descriptors of one mesh, spare node included."""
    worst, todo = 0, [(int(root), 0)]
    while todo:
        n, above = todo.pop()
        inner = [int(c) for c in child[n] if not c & LEAF]
        here = above + max(len(inner) - 1, 0)
        worst = max(worst, here)
        todo += [(c, here) for c in inner]
    return worst


def check_ray_slots(flat, stages):
    """FlatScene::ray_slots is what every mesh's tree can stack, in every stage, from the record's own bvh_root (the spare
    node where the mesh is guarded).  Returns the worst height met."""
    slots, n_mesh, worst = flat["scalars"]["ray_slots"], flat["scalars"]["n_mesh"], 0
    for st in [flat] + list(stages):
        for M in st["meshes"][:n_mesh]:
            nb, nc = int(M["node_begin"]), int(M["node_count"])
            h = worst_stack(st["nodes4"]["child"][nb:nb + nc + 1], M["bvh_root"])
            assert h <= slots, f"stage {st['what']}: mesh {int(M['index'])} can stack {h} entries, ray_slots is {slots}: the walk would drop a subtree"
            worst = max(worst, h)
    return worst


def check_planes(flat):
    objs, planes, n_axis = flat["objs"], flat["planes"], flat["scalars"]["n_axis_recs"]
    assert n_axis % 3 == 0 and n_axis <= len(planes)

    def is_axis(O):
        f = O["f"]
        return bool(np.isfinite(f[:6]).all() and (np.abs(f[:3]) <= np.float32(1e37)).all() and (f[3:6] != 0).sum() == 1)
    plane_objs = [O for O in objs if O["type"] == OBJ_PLANE]
    n_axis_planes = sum(is_axis(O) for O in plane_objs)
    if n_axis_planes < 3:
        assert n_axis == 0                                                               # fewer than three: all planes are general
    for r, pr in enumerate(planes):
        for slot in range(2):
            i = int(pr["index"][slot])
            if i == PAD:
                # an empty slot copies its neighbour's numbers (a record that is empty altogether: harmless numbers)
                assert slot == 1 or pr["index"][1] == PAD
                if pr["index"][0] != PAD:
                    assert np.array_equal(pr["p"][:, 1], pr["p"][:, 0]) and np.array_equal(pr["n"][:, 1], pr["n"][:, 0])
                continue
            O = objs[i]
            assert np.array_equal(pr["p"][:, slot], O["f"][:3]) and np.array_equal(pr["n"][:, slot], O["f"][3:6])
            assert pr["transparent"][slot] == O["f"][7:8].view("u4")[0]
            if r < n_axis:
                assert is_axis(O) and O["f"][3 + r % 3] != 0                             # record r of a triple: normal along axis r % 3
            else:
                assert n_axis == 0 or not is_axis(O)
    # general records: filled in scene order, two per record, only the last may be half empty
    general = planes["index"][n_axis:].ravel()
    assert (general[:-1] != PAD).all() if len(general) else True
    assert list(general[general != PAD]) == sorted(general[general != PAD])


def test_shipped_scenes_flatten_by_the_rules(harness, tmp_path, ca):
    for name in ("bunny", "mirror", "sphere_plane", "triangle"):
        s = ca.HostScene.load(f"scene/{name}.json")
        assert s.ok
        flat, stages = run(harness, tmp_path, s)
        check_flat(flat, s.desc.contents)
        check_ray_slots(flat, stages)
    grid = ca.HostScene.load(scenes.make_bunny_grid(str(tmp_path), 4, width=64, height=64))
    flat, stages = run(harness, tmp_path, grid)
    check_flat(flat, grid.desc.contents)
    check_ray_slots(flat, stages)
    assert flat["scalars"]["n_mesh"] == 16 and flat["scalars"]["merged_reserved"] == 1


@pytest.mark.parametrize("seed", range(12))
def test_random_scenes_flatten_by_the_rules(harness, tmp_path, seed):
    s = parse(cutrace_amd, _random_scene(seed, extra_planes=seed % 2 == 1))
    flat, stages = run(harness, tmp_path, s)
    check_flat(flat, s.desc.contents)
    check_ray_slots(flat, stages)
    s = parse(cutrace_amd, _multi_mesh_scene(tmp_path, seed, opaque=seed % 2 == 0, n_mesh=2 + seed % 4))
    flat, stages = run(harness, tmp_path, s, merge=True)
    check_flat(flat, s.desc.contents)
    check_ray_slots(flat, stages)
    # the merged tree, built: its keys are (rank << 24 | file index), every triangle of every mesh once
    last = stages[-1]
    sc, n_mesh = flat["scalars"], flat["scalars"]["n_mesh"]
    keys = last["tris"]["orig"][sc["merged_tri_begin"]:sc["merged_tri_begin"] + sc["merged_tri_count"]]
    counts = [int(c) for c in last["meshes"]["tri_count"][n_mesh + 1:]]
    assert sorted(keys) == [(r << 24) | k for r, c in enumerate(counts) for k in range(c)]
    assert last["merged"][0] == 1 and 0 < last["meshes"]["node_count"][n_mesh] <= sc["merged_node_cap"]


def test_ray_slots_hold_the_deepest_walk(harness, tmp_path, ca):
    """the trees this project builds deepest: the 64 000-triangle bunny, a mesh whose triangles span 24 octaves of size, and
    guarded meshes, whose walk starts at the spare node"""
    dense = ca.HostScene.load(scenes.make_dense_bunny(str(tmp_path), rounds=3, width=32, height=32))
    assert dense.ok
    flat, stages = run(harness, tmp_path, dense)
    worst = check_ray_slots(flat, stages)
    print(f"dense bunny: worst stack {worst}, ray_slots {flat['scalars']['ray_slots']}")
    # the deepest this project builds: tests/test_gpu_query_ranges.py makes the largest LDS launch with this mesh
    assert worst >= 26 and flat["scalars"]["ray_slots"] >= 33
    rng = np.random.RandomState(4)
    tris = []
    for i in range(6000):
        c, r = rng.uniform(-1, 1, 3), 2.0 ** -(i % 24)
        tris.append([c + r * rng.uniform(-0.3, 0.3, 3) for _ in range(3)])
    scenes.write_stl(str(tmp_path / "cluster.stl"), np.asarray(tris, np.float32))
    flat, stages = run(harness, tmp_path, _scene([{"type": "mesh", "file": str(tmp_path / "cluster.stl"), "material": 0}]))
    worst = check_ray_slots(flat, stages)
    print(f"geometric cluster: worst stack {worst}, ray_slots {flat['scalars']['ray_slots']}")
    for k in (7, GUARD_SLOTS):
        flat, stages = run(harness, tmp_path, _scene([_guard_mesh(tmp_path, k, n_other=400)]), eyes=[[IN_PLANE], [OFF_PLANE]])
        assert _selected(flat, stages[0]) == list(range(k)) and stages[0]["meshes"]["bvh_root"][0] != 0   # walked from the spare node
        check_ray_slots(flat, stages)


def test_the_shade_kernels_lds_cap_is_unreachable():
    """ctr_shade_rays refuses a launch whose walk stack and recursion frames exceed CTR_SHADE_LDS_MAX.  From the headers'
    own constants no scene can get there today, so that CTR_E_INVALID branch has no test.  If this fails, the branch has
    become reachable: it now needs a test of its own (a scene that deep, bounces that high, the message checked)."""
    import re

    def const(header, name):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, open(os.path.join(CSRC, header)).read())
        assert m, f"{name} is no longer a #define of {header}"
        return int(m.group(1))
    depth, bounces, cap = const("bvh.h", "BVH4_MAX_DEPTH"), const("scene_device.h", "CTR_MAX_BOUNCES"), const("ray_shade.h", "CTR_SHADE_LDS_MAX")
    rs_threads = int(re.search(r"constexpr int RS_THREADS = (\d+);", open(os.path.join(CSRC, "ray_shade.hip")).read()).group(1))
    # scene_flatten.cpp ray_stack_slots: slots = 3 * (deepest level + 1), levels counted from 1 at the root
    m = re.search(r"return (\d+)u \* \(deepest \+ (\d+)u\);", open(os.path.join(CSRC, "scene_flatten.cpp")).read())
    assert m, "ray_stack_slots no longer returns a * (deepest + b): restate its formula here"
    per_level, extra = int(m.group(1)), int(m.group(2))
    levels = depth + 1 + 1                      # node depths 0 .. BVH4_MAX_DEPTH and, generously, the spare node above the root
    slots = per_level * (levels + extra)
    # ctr_rays.cpp: frame_dwords = need_cold ? 10 : 4 — the larger of the two
    m = re.search(r"frame_dwords = s->flat\.need_cold \? (\d+)u : (\d+)u;", open(os.path.join(CSRC, "ctr_rays.cpp")).read())
    assert m, "ctr_rays.cpp no longer sets frame_dwords from need_cold: restate it here"
    frame_dwords = max(int(m.group(1)), int(m.group(2)))
    worst = (slots + bounces * frame_dwords) * rs_threads * 4
    print(f"largest request: ({slots} + {bounces * frame_dwords}) dwords x {rs_threads} lanes = {worst} bytes of {cap}")
    assert worst <= cap, (f"a scene can now ask ctr_shade_rays for {worst} bytes of LDS, more than CTR_SHADE_LDS_MAX = {cap}: the "
                          "CTR_E_INVALID path of ctr_rays.cpp is reachable and needs a test of its own")


MATS = [{"type": "solid", "color": [0.8, 0.6, 0.3], "specular": 0.4, "reflect": 0.0, "phong": 40}]
CAM = {"eye": [0.3, 0.2, 0.5], "up": [0, 1, 0], "look": [0, 0, -1.0], "near_plane": 0.1, "far_plane": 100.0, "width": 32, "height": 32, "ambient": 0.1}
LIGHTS = [{"type": "point", "point": [5.0, 6.0, 7.03], "color": [0.8, 0.8, 0.8]}, {"type": "sun", "direction": [0.1, 0.2, -1.0], "color": [0.5, 0.5, 0.5]}]


def _scene(objs, mats=MATS, lights=LIGHTS, cam=CAM):
    return parse(cutrace_amd, json.dumps({"camera": cam, "lights": lights, "materials": mats, "objects": objs}))


def test_plane_records_and_empty_meshes(harness, tmp_path):
    scenes.write_stl(str(tmp_path / "one.stl"), np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]]))
    scenes.write_stl(str(tmp_path / "none.stl"), np.zeros((0, 3, 3), np.float32))
    one, none = {"type": "mesh", "file": str(tmp_path / "one.stl"), "material": 0}, {"type": "mesh", "file": str(tmp_path / "none.stl"), "material": 0}

    def plane(n, p=(0, -1, 0)):
        return {"type": "plane", "point": list(p), "normal": list(n), "material": 0}
    axis = [plane((0, 1, 0)), plane((0, -0.0, 2.0), (0, 0, -3)), plane((-1e-3, 0, 0), (4, 0, 0)), plane((0, 0.25, 0), (0, 3, 0)), plane((0, 3, 0), (0, 5, 0))]
    tilted = [plane((0.1, 1, 0)), plane((1, 1, 1), (-4, -4, -4)), plane((0, 1, 1e-6))]
    for objs, n_axis_recs, n_recs in (([none, plane((0, 1, 0)), one, plane((0, 0, 1), (0, 0, -3)), none], 0, 1),   # two axis planes: general records
                                      (axis[:3] + [one], 3, 3), (tilted + axis + [none], 6, 8), (tilted, 0, 2), ([one], 0, 0),
                                      ([plane((0, 1, 0), (0, 2e37, 0))] + axis[:3], 3, 4)):                        # a point beyond 1e37: general
        s = _scene(objs)
        flat, stages = run(harness, tmp_path, s)
        check_flat(flat, s.desc.contents)
        assert (flat["scalars"]["n_axis_recs"], len(flat["planes"])) == (n_axis_recs, n_recs), objs
        assert flat["scalars"]["n_mesh"] == sum(o is one for o in objs) and len(flat["guards"]) == sum(o["type"] == "mesh" for o in objs)
        for st in stages:
            assert len(st["dirty"]) == 0


BELOW, ABOVE = float(np.float32(1e-6)), float(np.nextafter(np.float32(1e-6), np.float32(1)))   # the floats either side of the double 1e-6


@pytest.mark.parametrize("tr,rf,want", [(0.0, 0.0, (1, 0, 0)), (BELOW, BELOW, (0, 0, 0)), (ABOVE, 0.0, (0, 0, 1)), (0.0, ABOVE, (1, 0, 1)),
                                        (ABOVE, BELOW, (0, 0, 1)), (ABOVE, ABOVE, (0, 1, 1)), (0.5, 0.3, (0, 1, 1))])
def test_material_flags_use_the_documented_thresholds(harness, tmp_path, tr, rf, want):
    """all_opaque: transparency == 0 exactly; need_cold: transparency AND reflexivity >= 1e-6, compared as doubles (the float
    nearest to 1e-6 lies below it); any_bounce: either."""
    assert BELOW < 1e-6 <= ABOVE
    s = _scene([{"type": "sphere", "center": [0, 0, 0], "radius": 0.5, "material": 1}], mats=[MATS[0], dict(MATS[0])])
    s.set_material(1, transparency=tr, reflexivity=rf)
    flat, _ = run(harness, tmp_path, s)
    assert (flat["scalars"]["all_opaque"], flat["scalars"]["need_cold"], flat["scalars"]["any_bounce"]) == want
    check_flat(flat, s.desc.contents)


# ---------------------------------------------------------------- the guard

def _guard_mesh(tmp_path, k, n_other=40, seed=0, zero_area=True):
    """A mesh of k triangles IN the plane z = 0.5 (file indices 0..k-1), n_other triangles in planes z = 2, 2.1, ... that hold neither
    the eye nor a light and are not parallel to the sun, and (zero_area) two triangles of no area in the plane z = 0.5."""
    rng = np.random.RandomState(seed)
    tris = []
    for _ in range(k):
        c = rng.uniform(-1, 1, 2)
        tris.append([[c[0] + dx, c[1] + dy, 0.5] for dx, dy in ((0, 0), (0.3, 0.05), (0.1, 0.35))])
    for j in range(n_other):
        c = rng.uniform(-1, 1, 2)
        tris.append([[c[0] + dx, c[1] + dy, 2.0 + 0.1 * j] for dx, dy in ((0, 0), (0.3, 0.05), (0.1, 0.35))])
    if zero_area:
        tris += [[[0.1, 0.1, 0.5]] * 3, [[0, 0, 0.5], [0.5, 0.5, 0.5], [1, 1, 0.5]]]     # a point, three points of a line
    path = str(tmp_path / f"guard_{k}_{seed}.stl")
    scenes.write_stl(path, np.asarray(tris, np.float32))
    return {"type": "mesh", "file": path, "material": 0}


def _selected(flat, stage, mesh=0):
    """file indices of the mesh's guarded triangles + checks that the records, the spare node and bvh_root say the same"""
    g = flat["guards"][mesh]
    guarded = [int(t) for t in stage["guarded"][mesh]]
    assert guarded == sorted(guarded) and len(set(guarded)) == len(guarded)             # leaf order
    t0, n = g["tri_begin"], g["tri_count"]
    tris, gn = stage["tris"], stage["gn"].reshape(-1, 4)
    for k, t in enumerate(guarded):
        assert tris[t0 + n + k].tobytes() == tris[t0 + t].tobytes() and gn[t0 + n + k].tobytes() == gn[t0 + t].tobytes()
    root = 0 if not guarded else g["node_count"]
    assert stage["objs"]["bvh_root"][g["obj_index"]] == root and stage["meshes"]["bvh_root"][g["mesh_pos"]] == root
    if guarded:
        spare = stage["nodes4"][g["node_begin"] + g["node_count"]]
        assert list(spare["child"]) == [LEAF | (len(guarded) << 24) | n, 0, LEAF, LEAF]
        assert (spare["lo"][:, :2] == np.float32(-3.0e38)).all() and (spare["hi"][:, :2] == np.float32(3.0e38)).all()
    return sorted(int(tris["orig"][t0 + t]) for t in guarded)


IN_PLANE, OFF_PLANE = [0.3, 0.2, 0.5], [0.3, 0.2, 0.5 + 1e-3 * 9.0]   # the scene is about 9 units across (the light is its far corner)


def test_guard_selects_exactly_the_in_plane_triangles(harness, tmp_path):
    k = 7
    s = _scene([_guard_mesh(tmp_path, k), {"type": "plane", "point": [0, -1, 0], "normal": [0, 1, 0], "material": 0}])
    flat, st = run(harness, tmp_path, s, eyes=[[IN_PLANE], [OFF_PLANE], [OFF_PLANE, IN_PLANE, [1, 1, 1]], [[0, 0, 9]]])
    check_flat(flat, s.desc.contents)
    first, again, off, off_again, path, path_again, away, away_again = st
    assert _selected(flat, first) == list(range(k)) and not first["linear"][0][0]      # not the zero-area ones, not the others
    assert len(first["dirty"]) > 0
    for twice in (again, off_again, path_again, away_again):
        assert len(twice["dirty"]) == 0                                                  # unchanged cameras: nothing to upload
    assert _selected(flat, off) == [] and len(off["dirty"]) > 0                          # 1e-3 of the scene size off the plane
    assert _selected(flat, path) == list(range(k))                                       # any camera of a path counts
    assert _selected(flat, away) == []
    assert [int(x) for x in first["plan"][:2]] == [1, 0] and int(path["plan"][0]) == 3   # origins, mirrors
    # what is uploaded: the records, their normals, the spare node, the two mesh records — nothing else
    g = flat["guards"][0]
    slot0 = g["tri_begin"] + g["tri_count"]
    TRIS, GNORM, NODES4, MESHES, OBJS = 2, 3, 4, 1, 0
    assert [tuple(int(x) for x in r) for r in first["dirty"]] == [(TRIS, slot0, k, 0), (GNORM, slot0, k, 0), (NODES4, g["node_begin"] + g["node_count"], 1, 0),
                                                                  (MESHES, g["mesh_pos"], 1, 0), (OBJS, g["obj_index"], 1, 0)]
    assert [tuple(int(x) for x in r) for r in off["dirty"]] == [(MESHES, g["mesh_pos"], 1, 0), (OBJS, g["obj_index"], 1, 0)]


def test_more_in_plane_triangles_than_guard_slots_means_linear(harness, tmp_path):
    for k, linear in ((GUARD_SLOTS, False), (GUARD_SLOTS + 1, True), (150, True)):
        s = _scene([_guard_mesh(tmp_path, k)])
        flat, st = run(harness, tmp_path, s, eyes=[[IN_PLANE], [OFF_PLANE]])
        first, again, off, off_again = st
        g = flat["guards"][0]
        assert bool(first["linear"][0][0]) == linear and bool(first["plan"][3]) == linear
        assert _selected(flat, first) == ([] if linear else list(range(k)))              # linear: no guard records
        assert len(again["dirty"]) == 0 and len(off_again["dirty"]) == 0
        assert not off["linear"][0][0] and _selected(flat, off) == []
        if linear:   # the nodes go to the device with unbounded boxes, and come back with the real ones; the host keeps the real ones
            assert [tuple(int(x) for x in r) for r in first["dirty"]] == [(4, g["node_begin"], g["node_count"], g["node_count"])]
            assert [tuple(int(x) for x in r) for r in off["dirty"]] == [(4, g["node_begin"], g["node_count"], g["node_count"])]
            assert first["nodes4"].tobytes() == flat["nodes4"].tobytes()


def test_lights_in_the_plane_select_too(harness, tmp_path):
    k = 5
    mesh = _guard_mesh(tmp_path, k)
    away = [[0.3, 0.2, 9.0]]
    for lights, want in (([{"type": "point", "point": [3.0, -2.0, 0.5], "color": [1, 1, 1]}], True),
                         ([{"type": "point", "point": [3.0, -2.0, 0.51], "color": [1, 1, 1]}], False),
                         ([{"type": "sun", "direction": [0.3, -0.8, 0.0], "color": [1, 1, 1]}], True),    # parallel to the plane
                         ([{"type": "sun", "direction": [0.3, -0.8, 0.01], "color": [1, 1, 1]}], False)):
        flat, st = run(harness, tmp_path, _scene([mesh], lights=lights), eyes=[away])
        # a sun parallel to z = 0.5 is parallel to every plane z = const: the other triangles qualify as well
        everything = lights[0]["type"] == "sun" and want
        assert _selected(flat, st[0]) == (list(range(k + 40)) if everything else list(range(k)) if want else []), lights
        assert len(st[1]["dirty"]) == 0


def test_mirror_images_of_the_eye_select_only_with_a_reflecting_mirror(harness, tmp_path):
    k = 6
    mesh = _guard_mesh(tmp_path, k)
    below = [[0.3, 0.2, -0.5]]                # its image in the plane z = 0 is (0.3, 0.2, 0.5): in the triangles' plane
    for reflect, want in ((0.9, True), (1e-5, True), (0.0, False), (5e-7, False)):
        mats = MATS + [dict(MATS[0], reflect=reflect)]
        s = _scene([mesh, {"type": "plane", "point": [0, 0, 0], "normal": [0, 0, 2.0], "material": 1}], mats=mats)
        flat, st = run(harness, tmp_path, s, eyes=[below, [[0.3, 0.2, -0.6]]])
        assert _selected(flat, st[0]) == (list(range(k)) if want else []), reflect
        assert [int(x) for x in st[0]["plan"][:2]] == ([2, 1] if want else [1, 0])       # eye + image, one mirror
        assert _selected(flat, st[2]) == []                                              # another eye: its image is off the plane
        assert len(st[1]["dirty"]) == 0 and len(st[3]["dirty"]) == 0
    # a stand-alone reflecting triangle in z = 0 is a mirror as well; two mirrors: images of images
    tri = {"type": "triangle", "p1": [-3, -3, 0], "p2": [3, -3, 0], "p3": [0, 3, 0], "material": 1}
    flat, st = run(harness, tmp_path, _scene([mesh, tri], mats=MATS + [dict(MATS[0], reflect=0.5)]), eyes=[below])
    assert _selected(flat, st[0]) == list(range(k))
    two = [{"type": "plane", "point": [0, 0, 0], "normal": [0, 0, 1], "material": 1}, {"type": "plane", "point": [0, 0, -1], "normal": [0, 0, 1], "material": 1}]
    # eye at z = -2.5: image in z = -1 is z = 0.5 ... first order; eye at z = -1.5: image in z = 0 is 1.5, in z = -1 is -0.5, whose image in z = 0 is 0.5
    flat, st = run(harness, tmp_path, _scene([mesh] + two, mats=MATS + [dict(MATS[0], reflect=0.5)]), eyes=[[[0.3, 0.2, -1.5]], [[0.3, 0.2, -1.4]]])
    assert _selected(flat, st[0]) == list(range(k)) and [int(x) for x in st[0]["plan"][:2]] == [5, 2]
    assert _selected(flat, st[2]) == []


def test_merged_tree_guard_follows_the_meshes(harness, tmp_path):
    a, b = _guard_mesh(tmp_path, 4, seed=1), _guard_mesh(tmp_path, 3, seed=2)
    s = _scene([a, {"type": "plane", "point": [0, -1, 0], "normal": [0, 1, 0], "material": 0}, b])
    flat, st = run(harness, tmp_path, s, eyes=[[IN_PLANE], [OFF_PLANE]], merge=True)
    check_flat(flat, s.desc.contents)
    first, again, merged, merged_again, off, off_again = st
    assert _selected(flat, first, 0) == [0, 1, 2, 3] and _selected(flat, first, 1) == [0, 1, 2]
    assert list(first["merged"]) == [0, 0] and list(merged["merged"]) == [1, 1]
    assert sorted(merged["merged_guarded"]) == [0, 1, 2, 3, (1 << 24) | 0, (1 << 24) | 1, (1 << 24) | 2]
    sc, n_mesh = flat["scalars"], flat["scalars"]["n_mesh"]
    P = merged["meshes"][n_mesh]
    assert P["bvh_root"] == P["node_count"] > 0
    slot0 = sc["merged_tri_begin"] + sc["merged_tri_count"]
    assert list(merged["tris"]["orig"][slot0:slot0 + 7]) == list(merged["merged_guarded"])
    spare = merged["nodes4"][sc["merged_node_begin"] + P["node_count"]]                 # the root behind it, then one guard leaf per mesh
    assert list(spare["child"]) == [0, LEAF | (4 << 24) | sc["merged_tri_count"], LEAF | (3 << 24) | (sc["merged_tri_count"] + 4), LEAF]
    for c, r in ((1, 0), (2, 1)):                                                        # each behind the box of its mesh
        box = merged["meshes"]["f"][n_mesh + 1 + r]
        assert np.array_equal(spare["lo"][:, c], box[:3]) and np.array_equal(spare["hi"][:, c], box[3:6])
    for twice in (again, merged_again, off_again):
        assert len(twice["dirty"]) == 0
    assert len(off["merged_guarded"]) == 0 and off["meshes"]["bvh_root"][n_mesh] == 0 and list(off["merged"]) == [1, 1]
