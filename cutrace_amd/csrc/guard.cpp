// guard.cpp — the guard of the BVH culling: selection and host-side edits (guard.h says why it exists).
#include "guard.h"

#include <cmath>
#include <cstdio>
#include <utility>

namespace {

struct P3 { double x, y, z; };
struct Mirror { P3 p, n; };  // a point of the plane, its unit normal

// the scene's flat mirrors: reflective planes, stand-alone triangles and triangles of small meshes, one entry per plane
std::vector<Mirror> flat_mirrors(const FlatScene &F) {
  std::vector<Mirror> mirrors;
  auto add_mirror = [&](double px, double py, double pz, double nx, double ny, double nz) {
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(len > 0.0)) return;
    nx /= len; ny /= len; nz /= len;
    const double c = px * nx + py * ny + pz * nz;
    for (const Mirror &m : mirrors) {  // one entry per plane (a mirror made of coplanar triangles)
      const double dot = m.n.x * nx + m.n.y * ny + m.n.z * nz, cm = m.p.x * m.n.x + m.p.y * m.n.y + m.p.z * m.n.z;
      if ((fabs(dot - 1.0) < 1e-9 && fabs(cm - c) < 1e-9 * (1.0 + fabs(c))) || (fabs(dot + 1.0) < 1e-9 && fabs(cm + c) < 1e-9 * (1.0 + fabs(c)))) return;
    }
    mirrors.push_back({{px, py, pz}, {nx, ny, nz}});
  };
  auto tri_plane = [&](const DTri &T) {
    const double ax = T.ab[0][0], ay = T.ab[1][0], az = T.ab[2][0], bx = T.ab[0][1], by = T.ab[1][1], bz = T.ab[2][1];
    add_mirror(T.px, T.py, T.pz, ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx);
  };
  for (const DObj &O : F.objs) {
    if (O.mat >= F.mats.size() || !((double)F.mats[O.mat].reflexivity >= 1e-6)) continue;
    if (O.type == CTR_OBJ_PLANE) add_mirror(O.f[0], O.f[1], O.f[2], O.f[3], O.f[4], O.f[5]);
    else if (O.type == CTR_OBJ_TRIANGLE) tri_plane(F.tris[O.tri_begin]);
    else if (O.type == CTR_OBJ_MESH && O.tri_count <= CTR_MIRROR_MESH_TRIS)
      for (uint32_t k = 0; k < O.tri_count; k++) tri_plane(F.tris[O.tri_begin + k]);
  }
  return mirrors;
}

// the points a family of rays can emanate from: eyes, and their images in the scene's flat mirrors
std::vector<P3> ray_origins(const std::vector<DCam> &cams, const std::vector<Mirror> &mirrors) {
  std::vector<P3> origins;
  for (const DCam &c : cams) origins.push_back({c.pos[0], c.pos[1], c.pos[2]});
  auto image = [](const P3 &e, const Mirror &m) {
    const double d = (e.x - m.p.x) * m.n.x + (e.y - m.p.y) * m.n.y + (e.z - m.p.z) * m.n.z;
    return P3{e.x - 2.0 * d * m.n.x, e.y - 2.0 * d * m.n.y, e.z - 2.0 * d * m.n.z};
  };
  const size_t n_eyes = origins.size();
  std::vector<std::pair<P3, size_t>> first;  // image, the mirror that made it
  for (size_t e = 0; e < n_eyes && first.size() < CTR_VIRTUAL_EYES_MAX; e++)
    for (size_t m = 0; m < mirrors.size() && first.size() < CTR_VIRTUAL_EYES_MAX; m++) first.push_back({image(origins[e], mirrors[m]), m});
  for (const auto &f : first) origins.push_back(f.first);
  if (n_eyes * mirrors.size() > first.size()) {
    static bool warned = false;
    if (!warned) fprintf(stderr, "cutrace_amd: %zu cameras x %zu flat mirrors exceed %u mirror images: the in-plane guard of reflected rays "
                                 "(DESIGN.md section 2) covers the first %zu only\n", n_eyes, mirrors.size(), CTR_VIRTUAL_EYES_MAX, first.size());
    warned = true;
  }
  // Images of images (two reflections in a row): for up to CTR_SECOND_ORDER_MAX_EYES cameras.  The guard records serve every
  // launch on the handle, whichever of its cameras the launch renders, so each camera's images cost every frame: with all
  // second-order images of a 90-camera path (2 340 points) the bunny room's frames ran 14 % slower for a handful of guard
  // triangles (bench.py config.campath_ms 1.17 -> 1.34 ms); first-order images of every camera stay.
  if (n_eyes <= CTR_SECOND_ORDER_MAX_EYES &&
      first.size() * (mirrors.size() ? mirrors.size() - 1 : 0) + origins.size() <= CTR_VIRTUAL_EYES_MAX)
    for (const auto &f : first)
      for (size_t m = 0; m < mirrors.size(); m++)
        if (m != f.second) origins.push_back(image(f.first, mirrors[m]));
  return origins;
}

// the triangles of one mesh (leaf order) whose plane holds an origin or a point light, or is parallel to a sun: guard_scan.h
std::vector<uint32_t> risky_triangles(const MeshGuard &g, const GuardProbes &P) {
  std::vector<uint32_t> risky;
  const size_t nt = g.planes.size() / CTR_PLANE_DOUBLES;
  for (size_t t = 0; t < nt; t++)
    if (plane_is_risky(&g.planes[CTR_PLANE_DOUBLES * t], P.probes.data(), (uint32_t)P.n_points, (uint32_t)P.probes.size())) risky.push_back((uint32_t)t);
  return risky;
}

// one mesh's guard records, spare node and bvh_root
void apply_mesh(FlatScene &F, MeshGuard &g, const std::vector<uint32_t> &risky, std::vector<DirtyRange> &dirty) {
  const uint32_t slot0 = g.tri_begin + g.tri_count;
  for (size_t k = 0; k < risky.size(); k++) {
    F.tris[slot0 + k] = F.tris[g.tri_begin + risky[k]];
    for (int q = 0; q < 4; q++) F.gn[4 * (slot0 + k) + q] = F.gn[4 * (g.tri_begin + risky[k]) + q];
  }
  if (!risky.empty()) {
    dirty.push_back({DirtyRange::TRIS, slot0, risky.size(), {}});
    dirty.push_back({DirtyRange::GNORM, slot0, risky.size(), {}});
    // the walk starts at node `bvh_root`: the root (0), or — with guard records — the mesh's extra node, whose
    // children are the guard leaf (relative to the mesh's first triangle) and the root, both with unbounded boxes
    DNode4 &gn4 = F.nodes4[g.node_begin + g.node_count];
    gn4 = empty_node4();
    unbounded_box(gn4, 0);
    unbounded_box(gn4, 1);
    gn4.child[0] = BVH_LEAF_FLAG | ((uint32_t)risky.size() << 24) | g.tri_count;
    gn4.child[1] = 0u;  // the root
    dirty.push_back({DirtyRange::NODES4, g.node_begin + g.node_count, 1, {}});
  }
  const uint32_t start = risky.empty() ? 0u : g.node_count;
  F.meshes[g.mesh_pos].bvh_root = start;
  F.objs[g.obj_index].bvh_root = start;
  dirty.push_back({DirtyRange::MESHES, (size_t)g.mesh_pos, 1, {}});
  dirty.push_back({DirtyRange::OBJS, g.obj_index, 1, {}});
  g.guarded = risky;
}

// the merged tree: the same guard, one set of spare records for the triangles of all meshes
void apply_merged(FlatScene &F, const std::vector<uint32_t> &keys, std::vector<DirtyRange> &dirty) {
  Merged &M = F.merged;
  const uint32_t slot0 = M.tri_begin + M.tri_count;
  for (size_t k = 0; k < keys.size(); k++)
    F.tris[slot0 + k] = F.tris[M.tri_begin + M.where[M.slot_of[keys[k] >> 24] + (keys[k] & 0xFFFFFFu)]];
  if (!keys.empty()) {
    dirty.push_back({DirtyRange::TRIS, slot0, keys.size(), {}});
    // The walk starts at a chain of spare nodes before the root.  A spare node holds the guard leaves of up to three
    // meshes, each behind the box of ITS MESH — the reference shows a mesh's triangles only to rays that pass that
    // box (default_schema.hpp:126), so the box is exactly as far as a guard record has to reach (behind an unbounded
    // box every cast of the frame would test every guard record of every mesh: a handful of them doubled the 16-mesh
    // frame's triangle tests) — and, as its fourth child, the next spare node or the root, unbounded.
    struct Group { uint32_t rank, first, count; };
    std::vector<Group> groups;
    for (size_t k = 0; k < keys.size(); k++) {
      const uint32_t r = keys[k] >> 24;
      if (groups.empty() || groups.back().rank != r) groups.push_back({r, (uint32_t)k, 0u});
      groups.back().count++;
    }
    const uint32_t n_spare = (uint32_t)((groups.size() + 2) / 3);
    for (uint32_t j = 0; j < n_spare; j++) {
      DNode4 &g4 = F.nodes4[M.node_begin + M.node_count + j];
      g4 = empty_node4();
      // (slot 0: the next spare node or the root; slots 1..3: guard leaves — unused slots last, the walk skips an empty second pair)
      unbounded_box(g4, 0);
      g4.child[0] = (j + 1 < n_spare) ? (M.node_count + j + 1) : 0u;
      for (int c = 0; c < 3; c++) {
        const size_t gi = (size_t)3 * j + c;
        if (gi >= groups.size()) break;
        const DObj &Rm = F.meshes[F.n_mesh + 1u + groups[gi].rank];
        for (int a = 0; a < 3; a++) { g4.lo[a][1 + c] = Rm.f[a]; g4.hi[a][1 + c] = Rm.f[3 + a]; }
        g4.child[1 + c] = BVH_LEAF_FLAG | (groups[gi].count << 24) | (M.tri_count + groups[gi].first);
      }
    }
    dirty.push_back({DirtyRange::NODES4, M.node_begin + M.node_count, n_spare, {}});
  }
  F.meshes[F.n_mesh].bvh_root = keys.empty() ? 0u : M.node_count;
  dirty.push_back({DirtyRange::MESHES, F.n_mesh, 1, {}});
  M.guarded = keys;
}

}  // namespace

GuardProbes guard_probes(const FlatScene &F, const std::vector<DCam> &cams) {
  GuardProbes P;
  const std::vector<Mirror> mirrors = flat_mirrors(F);
  const std::vector<P3> origins = ray_origins(cams, mirrors);
  P.n_mirrors = mirrors.size();
  P.n_origins = origins.size();
  P.probes.reserve(origins.size() + F.lights.size());
  for (const P3 &o : origins) P.probes.push_back({o.x, o.y, o.z, 0.0});
  for (const DLight &l : F.lights)
    if (l.type == CTR_LIGHT_POINT) P.probes.push_back({l.vx, l.vy, l.vz, 0.0});
  P.n_points = P.probes.size();
  for (const DLight &l : F.lights)
    if (l.type != CTR_LIGHT_POINT) P.probes.push_back({l.vx, l.vy, l.vz, sqrt((double)l.vx * l.vx + (double)l.vy * l.vy + (double)l.vz * l.vz)});
  return P;
}

uint64_t guard_plane_count(const FlatScene &F) {
  uint64_t n = 0;
  for (const MeshGuard &g : F.guards) n += g.planes.size() / CTR_PLANE_DOUBLES;
  return n;
}

GuardPlan plan_guards(const FlatScene &F, const GuardProbes &P, const uint64_t *words) {
  GuardPlan plan;
  plan.n_mirrors = P.n_mirrors;
  plan.n_origins = P.n_origins;
  plan.meshes.resize(F.guards.size());
  uint32_t rank = 0;  // of the current mesh among the non-empty meshes, scene order (guards are in scene order)
  uint64_t first = 0;  // the mesh's first plane in the flat array of all meshes' planes
  for (size_t i = 0; i < F.guards.size(); i++) {
    const MeshGuard &g = F.guards[i];
    const uint32_t n_planes = (uint32_t)(g.planes.size() / CTR_PLANE_DOUBLES);
    const uint64_t begin = first;
    first += n_planes;
    if (g.mesh_pos < 0) continue;
    const uint32_t g_rank = rank++;
    GuardPlan::Mesh &m = plan.meshes[i];
    m.risky = words ? guard_scan_cut(words, begin, n_planes) : risky_triangles(g, P);
    m.linear = m.risky.size() > CTR_GUARD_SLOTS;
    if (m.linear) {
      plan.any_linear = true;
      m.risky.clear();
    }
    for (uint32_t t : m.risky) plan.merged_keys.push_back((g_rank << 24) | F.tris[g.tri_begin + t].orig);
  }
  return plan;
}

GuardPlan plan_guards(const FlatScene &F, const std::vector<DCam> &cams) { return plan_guards(F, guard_probes(F, cams), nullptr); }

std::vector<DirtyRange> apply_guards(FlatScene &F, const GuardPlan &plan) {
  std::vector<DirtyRange> dirty;
  for (size_t i = 0; i < F.guards.size(); i++) {
    MeshGuard &g = F.guards[i];
    if (g.mesh_pos < 0) continue;
    const GuardPlan::Mesh &m = plan.meshes[i];
    if (m.linear != g.linear && g.node_count) {
      // the device's copy of the mesh's nodes: the real boxes, or every used slot unbounded (an unused slot stays what it is)
      std::vector<DNode4> nn(F.nodes4.begin() + g.node_begin, F.nodes4.begin() + g.node_begin + g.node_count);
      if (m.linear)
        for (DNode4 &n : nn)
          for (int c = 0; c < 4; c++)
            if (n.child[c] != BVH_LEAF_FLAG) unbounded_box(n, c);
      dirty.push_back({DirtyRange::NODES4, g.node_begin, g.node_count, std::move(nn)});
      g.linear = m.linear;
    }
    if (m.risky != g.guarded) apply_mesh(F, g, m.risky, dirty);
  }
  // a mesh that went linear or more risky triangles than records -> the merged tree is not walked (ctr_render.cpp kernel_facts: merged_usable)
  if (F.merged.built) {
    F.merged.usable = plan.merged_usable();
    if (F.merged.usable && plan.merged_keys != F.merged.guarded) apply_merged(F, plan.merged_keys, dirty);
  }
  return dirty;
}
