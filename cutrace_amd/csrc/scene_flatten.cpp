// scene_flatten.cpp — a scene description becomes the dense arrays of scene_device.h.  Pure host arithmetic, no HIP.
// Compile with -ffp-contract=off: the ray-independent triangle quantities computed here (a, b, geometric normal) must
// have the reference's bits.
#include "scene_flatten.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "tri_record.h"  // make_tri, guard_plane: shared with the device side of ctr_scene_update_mesh (mesh_update.hip)

namespace {

// what the BVH builders want to know of each triangle: its box and the box's centre
std::vector<BvhInput> tri_boxes(const ctr_triangle *src, size_t n) {
  std::vector<BvhInput> prims(n);
  for (size_t q = 0; q < n; q++) {
    const ctr_vec3 *v[3] = {&src[q].p1, &src[q].p2, &src[q].p3};
    BvhInput &b = prims[q];
    for (int a = 0; a < 3; a++) {
      const float c0 = (&v[0]->x)[a], c1 = (&v[1]->x)[a], c2 = (&v[2]->x)[a];
      b.mn[a] = fminf(c0, fminf(c1, c2));
      b.mx[a] = fmaxf(c0, fmaxf(c1, c2));
      b.c[a] = 0.5f * (b.mn[a] + b.mx[a]);
    }
  }
  return prims;
}

// The meshes' trees, several meshes at a time (a scene of 16 meshes of 1000 triangles: 2.5 -> 0.5 ms of ctr_scene_create; a
// mesh large enough to matter is built on several threads by the builder itself).  One entry per object, empty for what is
// not a mesh (or is one with too many triangles: mesh_record rejects it).
std::vector<MeshTree> mesh_trees(const ctr_scene_desc &d) {
  std::vector<MeshTree> trees(d.n_objects);
  std::vector<uint64_t> mesh_ids;
  for (uint64_t i = 0; i < d.n_objects; i++)
    if (d.objects[i].type == CTR_OBJ_MESH && d.objects[i].tri_count <= CTR_MESH_TRIS_MAX) mesh_ids.push_back(i);
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (size_t k; (k = next.fetch_add(1)) < mesh_ids.size();) {
      const ctr_object &o = d.objects[mesh_ids[k]];
      bvh4_build(tri_boxes(d.triangles + o.tri_begin, (uint32_t)o.tri_count), BVH_LEAF, trees[mesh_ids[k]].nodes, trees[mesh_ids[k]].order);
    }
  };
  const size_t n_thr = std::min<size_t>(mesh_ids.size() > 1 ? mesh_ids.size() : 1, std::max(1u, std::min(8u, std::thread::hardware_concurrency())));
  std::vector<std::thread> pool;
  for (size_t t = 1; t < n_thr; t++) pool.emplace_back(work);
  work();
  for (std::thread &t : pool) t.join();
  return trees;
}

// What the guard (guard.h) checks eyes and lights against: per triangle, in leaf order like the DTri records, its plane
// in double precision
std::vector<double> guard_planes(const ctr_triangle *src, const std::vector<uint32_t> &order) {
  std::vector<double> planes(CTR_PLANE_DOUBLES * order.size());
  for (size_t k = 0; k < order.size(); k++) {
    const ctr_triangle &t = src[order[k]];
    guard_plane(t.p1, t.p2, t.p3, &planes[CTR_PLANE_DOUBLES * k]);
  }
  return planes;
}

// One mesh: its tree's nodes + a spare node, its triangles in leaf order (each keeps its file index for tie-breaks) + the
// guard records, its normals, its MeshGuard
void mesh_record(const ctr_object &o, const ctr_triangle *src, const MeshTree &tree, DObj &O, FlatScene &F) {
  const uint32_t n = (uint32_t)o.tri_count;
  const std::vector<uint32_t> &order = tree.order;
  O.tri_begin = (uint32_t)F.tris.size();
  O.tri_count = n;
  O.node_begin = (uint32_t)F.nodes4.size();
  O.node_count = (uint32_t)tree.nodes.size();
  O.bvh_root = 0;  // node 0 of the mesh; child descriptors stay relative to the mesh's first node / first triangle
  F.nodes4.insert(F.nodes4.end(), tree.nodes.begin(), tree.nodes.end());
  F.nodes4.emplace_back();  // the mesh's spare node (guard records, apply_guards); unused = all zero
  memset(&F.nodes4.back(), 0, sizeof(DNode4));
  MeshGuard g;
  g.node_begin = O.node_begin;
  g.node_count = g.node_cap = O.node_count;
  g.tri_begin = O.tri_begin;
  g.tri_count = g.tri_cap = n;
  g.obj_index = O.index;
  g.planes = guard_planes(src, order);
  F.guards.push_back(std::move(g));
  F.tris.resize(F.tris.size() + n + (n ? CTR_GUARD_SLOTS : 0u));  // + the mesh's guard records (apply_guards)
  F.gn.resize(4 * F.tris.size());
  for (uint32_t k = 0; k < n; k++) {
    const ctr_triangle &t = src[order[k]];
    make_tri(t.p1, t.p2, t.p3, order[k], F.tris[O.tri_begin + k], &F.gn[4 * (O.tri_begin + order[k])]);  // normals in FILE order: the kernel keeps only the winner's original index
  }
  for (uint32_t k = 0; n && k < CTR_GUARD_SLOTS; k++) {  // unused guard records: copies of the first triangle
    F.tris[O.tri_begin + n + k] = F.tris[O.tri_begin];
    for (int q = 0; q < 4; q++) F.gn[4 * (O.tri_begin + n + k) + q] = F.gn[4 * O.tri_begin + q];
  }
}

// The analytic half of one object's records (flatten_scene through object_records, and objects_edited): the material index of
// any object; a sphere's, a plane's or a stand-alone triangle's parameters in its DObj; the triangle's DTri and normal at
// O.tri_begin, which the caller has set.  A mesh's triangles, tree and box are not touched here.
void analytic_record(const ctr_object &o, DObj &O, FlatScene &F) {
  O.mat = (uint32_t)o.mat_idx;
  switch (O.type) {
    case CTR_OBJ_TRIANGLE:
      make_tri(o.v0, o.v1, o.v2, 0, F.tris[O.tri_begin], &F.gn[4 * (size_t)O.tri_begin]);
      O.f[0] = o.v0.x; O.f[1] = o.v0.y; O.f[2] = o.v0.z;  // p1, p3: triangle::uv_for (KV_UV)
      O.f[3] = o.v2.x; O.f[4] = o.v2.y; O.f[5] = o.v2.z;
      break;
    case CTR_OBJ_MESH:
      break;
    case CTR_OBJ_PLANE:  // (a plane's point and normal)
      O.f[0] = o.v0.x; O.f[1] = o.v0.y; O.f[2] = o.v0.z;
      O.f[3] = o.v1.x; O.f[4] = o.v1.y; O.f[5] = o.v1.z;
      break;
    default:
      O.f[0] = o.v0.x; O.f[1] = o.v0.y; O.f[2] = o.v0.z;
      O.f[3] = o.f0;
      O.f[4] = o.f0 * o.f0;
      break;
  }
}

// objs: one record per object, scene order; meshes and stand-alone triangles add their DTri records as they come
int object_records(const ctr_scene_desc &d, const std::vector<MeshTree> &trees, FlatScene &F, std::string &err) {
  F.objs.resize(d.n_objects);
  F.tris.reserve(d.n_triangles + d.n_objects);
  for (uint64_t i = 0; i < d.n_objects; i++) {
    const ctr_object &o = d.objects[i];
    DObj &O = F.objs[i];
    memset(&O, 0, sizeof(O));
    O.type = o.type;
    O.index = (uint32_t)i;
    if (o.type == CTR_OBJ_TRIANGLE) {
      O.tri_begin = (uint32_t)F.tris.size();
      O.tri_count = 1;
      F.tris.emplace_back();
      F.gn.resize(4 * F.tris.size());
    } else if (o.type == CTR_OBJ_MESH) {
      F.has_mesh = true;
      if (o.tri_count > CTR_MESH_TRIS_MAX) {
        err = "object #" + std::to_string(i) + ": mesh has more than 2^24 triangles";
        return CTR_E_INVALID;
      }
      mesh_record(o, d.triangles + o.tri_begin, trees[i], O, F);
      O.f[0] = o.v0.x; O.f[1] = o.v0.y; O.f[2] = o.v0.z;  // the mesh's box
      O.f[3] = o.v1.x; O.f[4] = o.v1.y; O.f[5] = o.v1.z;
    }
    analytic_record(o, O, F);
  }
  return CTR_OK;
}

// planes: two per record, the axis-aligned ones first and in whole triples (scene_device.h DPlanePair); oloop: what is
// neither a plane nor a mesh
void plane_records(FlatScene &F) {
  F.oloop.clear();
  F.planes.clear();
  std::vector<const DObj *> axis_planes[3], general_planes;
  for (const DObj &O : F.objs) {
    if (O.type == CTR_OBJ_PLANE) {
      // axis-aligned: exactly one normal component is not zero (+0 and -0 both count as zero), everything finite
      int nz = 0, axis = -1;
      bool finite = true;
      for (int a = 0; a < 3; a++) {
        if (!std::isfinite(O.f[a]) || !std::isfinite(O.f[3 + a])) finite = false;
        if (O.f[3 + a] != 0.0f) { nz++; axis = a; }
      }
      // (and the point within 1e37: with the kernel's |origin| < 8.5e37 gate no component of point - origin overflows to
      //  inf, which the reference would multiply by the normal's zero into a NaN — ADVICE r03)
      for (int a = 0; a < 3; a++)
        if (!(fabsf(O.f[a]) <= 1e37f)) finite = false;
      if (finite && nz == 1) axis_planes[axis].push_back(&O);
      else general_planes.push_back(&O);
    } else if (O.type != CTR_OBJ_MESH) F.oloop.push_back(O);
  }
  auto empty_pair = [] {
    DPlanePair pr;
    for (int a = 0; a < 3; a++) { pr.p[a][0] = pr.p[a][1] = 0.0f; pr.n[a][0] = pr.n[a][1] = 1.0f; }
    pr.index[0] = pr.index[1] = CTR_PLANE_PAD;
    pr.transparent[0] = pr.transparent[1] = 0;
    return pr;
  };
  auto put = [](DPlanePair &pr, int slot, const DObj &O) {
    for (int a = 0; a < 3; a++) { pr.p[a][slot] = O.f[a]; pr.n[a][slot] = O.f[3 + a]; }
    pr.index[slot] = O.index;  // (.transparent: material_flags)
  };
  // fewer than three axis-aligned planes (a lone floor): one general record is less to fetch than a triple
  if (axis_planes[0].size() + axis_planes[1].size() + axis_planes[2].size() < 3) {
    general_planes.clear();
    for (int a = 0; a < 3; a++) axis_planes[a].clear();
    for (const DObj &O : F.objs)
      if (O.type == CTR_OBJ_PLANE) general_planes.push_back(&O);
  }
  // axis triples: as many as the busiest axis needs (a box room: one)
  size_t triples = 0;
  for (int a = 0; a < 3; a++) triples = std::max(triples, (axis_planes[a].size() + 1) / 2);
  for (size_t t = 0; t < triples; t++)
    for (int a = 0; a < 3; a++) {
      DPlanePair pr = empty_pair();
      for (int slot = 0; slot < 2; slot++)
        if (2 * t + slot < axis_planes[a].size()) put(pr, slot, *axis_planes[a][2 * t + slot]);
      // an empty slot copies its neighbour (same numbers, never tested)
      if (pr.index[0] != CTR_PLANE_PAD && pr.index[1] == CTR_PLANE_PAD)
        for (int q = 0; q < 3; q++) { pr.p[q][1] = pr.p[q][0]; pr.n[q][1] = pr.n[q][0]; }
      F.planes.push_back(pr);
    }
  F.n_axis_recs = (uint32_t)F.planes.size();
  for (size_t k = 0; k < general_planes.size(); k++) {
    if (k % 2 == 0) {
      DPlanePair pr = empty_pair();
      put(pr, 0, *general_planes[k]);
      for (int q = 0; q < 3; q++) { pr.p[q][1] = pr.p[q][0]; pr.n[q][1] = pr.n[q][0]; }
      F.planes.push_back(pr);
    } else {
      put(F.planes.back(), 1, *general_planes[k]);
    }
  }
}

// the meshes a ray can hit (an empty mesh is never hit), scene order
std::vector<DObj> nonempty_meshes(const FlatScene &F) {
  std::vector<DObj> m;
  for (const DObj &O : F.objs)
    if (O.type == CTR_OBJ_MESH && O.tri_count) m.push_back(O);
  return m;
}

// top-level BVH over the mesh boxes, one mesh per leaf (same node layout as the per-mesh trees)
void top_level(const std::vector<DObj> &meshes_in, FlatScene &F) {
  F.n_mesh = (uint32_t)meshes_in.size();  // (meshes[] may continue with the merged pseudo mesh and the meshes in scene order)
  F.tlas_begin = (uint32_t)F.nodes.size();
  if (meshes_in.empty()) return;
  std::vector<BvhInput> prims(meshes_in.size());
  for (int a = 0; a < 3; a++) { F.tl_mn[a] = INFINITY; F.tl_mx[a] = -INFINITY; }
  for (size_t k = 0; k < meshes_in.size(); k++) {
    for (int a = 0; a < 3; a++) {
      prims[k].mn[a] = meshes_in[k].f[a];
      prims[k].mx[a] = meshes_in[k].f[3 + a];
      prims[k].c[a] = 0.5f * (prims[k].mn[a] + prims[k].mx[a]);
      F.tl_mn[a] = fminf(F.tl_mn[a], prims[k].mn[a]);
      F.tl_mx[a] = fmaxf(F.tl_mx[a], prims[k].mx[a]);
    }
  }
  std::vector<DNode> tnodes;
  std::vector<uint32_t> order;
  bvh_build(prims, 1, tnodes, order, F.tlas_root);
  F.nodes.insert(F.nodes.end(), tnodes.begin(), tnodes.end());
  for (uint32_t k : order) F.meshes.push_back(meshes_in[k]);
  for (size_t pos = 0; pos < F.meshes.size(); pos++)
    for (MeshGuard &g : F.guards)
      if (g.obj_index == F.meshes[pos].index) g.mesh_pos = (int)pos;
}

// the merged tree (scene_flatten.h Merged): its room in the arrays is set aside and the triangles are kept
void reserve_merged(const ctr_scene_desc &d, const std::vector<DObj> &by_rank, FlatScene &F) {
  Merged &M = F.merged;
  uint64_t total = 0;
  for (const DObj &O : by_rank) total += O.tri_count;
  if (by_rank.size() < 2 || by_rank.size() > CTR_MERGE_MAX_MESHES || total > 0xFFFFFFull) return;
  M.reserved = true;
  M.src.reserve(total);
  for (uint32_t r = 0; r < by_rank.size(); r++) {
    M.slot_of.push_back((uint32_t)M.src.size());
    const ctr_object &o = d.objects[by_rank[r].index];
    M.src.insert(M.src.end(), d.triangles + o.tri_begin, d.triangles + o.tri_begin + o.tri_count);
  }
  M.slot_of.push_back((uint32_t)total);
  M.tri_begin = (uint32_t)F.tris.size();
  M.tri_count = (uint32_t)total;
  M.node_begin = (uint32_t)F.nodes4.size();
  M.node_cap = (uint32_t)(total / 2 + 64);  // (a four-wide node has at least two children: far fewer in practice)
  DNode4 zero4;
  memset(&zero4, 0, sizeof(zero4));
  F.nodes4.resize(F.nodes4.size() + M.node_cap + CTR_MERGED_SPARE_NODES, zero4);
  DTri zero_t;
  memset(&zero_t, 0, sizeof(zero_t));
  F.tris.resize(F.tris.size() + total + CTR_GUARD_SLOTS, zero_t);
  F.gn.resize(4 * F.tris.size());  // (unused for the merged records: normals are looked up in the mesh's own range)
  // the pseudo mesh record: the kernel's mesh code walks it like a mesh whose AABB every lane passes
  DObj P;
  memset(&P, 0, sizeof(P));
  P.type = CTR_OBJ_MERGED;
  P.tri_begin = M.tri_begin;
  P.tri_count = M.tri_count;
  P.node_begin = M.node_begin;
  P.node_count = 0;
  P.bvh_root = 0;
  P.index = 0xFFFFFFFFu;
  for (int a = 0; a < 3; a++) { P.f[a] = F.tl_mn[a]; P.f[3 + a] = F.tl_mx[a]; }  // (margin of the box tests: the box of all meshes)
  F.meshes.push_back(P);
  for (const DObj &O : by_rank) F.meshes.push_back(O);
}

// What the kernels' choice of build reads of the lights and materials (FlatScene: all_opaque, need_cold, any_bounce,
// fast_pow_ok), from the records alone and from the defaults: an edit can clear a flag as well as set it.
void shading_flags(FlatScene &F) {
  auto largest = [](float x, float y, float z) { return std::max(std::fabs((double)x), std::max(std::fabs((double)y), std::fabs((double)z))); };
  double lambda = 0.0, worst = 0.0;
  for (const DLight &l : F.lights) lambda += largest(l.cx, l.cy, l.cz);
  F.all_opaque = true;
  F.need_cold = F.any_bounce = false;
  for (const DMat &m : F.mats) {
    if (!(m.transparency == 0.0f)) F.all_opaque = false;
    if ((double)m.transparency >= 1e-6 && (double)m.reflexivity >= 1e-6) F.need_cold = true;
    if ((double)m.transparency >= 1e-6 || (double)m.reflexivity >= 1e-6) F.any_bounce = true;
    worst = std::max(worst, std::fabs((double)m.phong_exp * (double)m.specular) * largest(m.cx, m.cy, m.cz));
  }
  F.fast_pow_ok = fast_pow_in_bar(worst, lambda);
  const uint32_t facts = shade_facts(F.mats.data(), F.mats.size(), F.lights.data(), F.lights.size());
  F.shade_finite = (facts & 1u) != 0u;
  F.shade_bounded = (facts & 2u) != 0u;
}

}  // namespace

// FlatScene::ray_slots
uint32_t ray_stack_slots(const FlatScene &F) {
  uint32_t deepest = 0;
  std::vector<std::pair<uint32_t, uint32_t>> todo;  // (node relative to the mesh's first, its level)
  for (const MeshGuard &g : F.guards) {
    if (g.mesh_pos < 0 || g.node_count == 0) continue;
    todo.assign(1, {0u, 1u});
    while (!todo.empty()) {
      const auto [n, lvl] = todo.back();
      todo.pop_back();
      deepest = std::max(deepest, lvl);
      const DNode4 &N = F.nodes4[g.node_begin + n];
      for (int c = 0; c < 4; c++)
        if (!(N.child[c] & BVH_LEAF_FLAG) && N.child[c] < g.node_count) todo.push_back({N.child[c], lvl + 1});
    }
  }
  return 3u * (deepest + 1u);
}

DNode4 empty_node4() {
  DNode4 N;
  memset(&N, 0, sizeof(N));
  for (int c = 0; c < 4; c++) {
    for (int a = 0; a < 3; a++) { N.lo[a][c] = 3.4028235e38f; N.hi[a][c] = 3.4028235e38f; }
    N.child[c] = BVH_LEAF_FLAG;
  }
  return N;
}

void create_stamp(const char *what) {
  thread_local std::chrono::high_resolution_clock::time_point t0;
  const auto now = std::chrono::high_resolution_clock::now();
  if (what && getenv("CUTRACE_DEBUG_CREATE"))
    fprintf(stderr, "cutrace_amd scene_create: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
  t0 = now;
}

int validate_desc(const ctr_scene_desc &d, std::string &err) {
  auto bad = [&](const std::string &msg) { err = msg; return CTR_E_INVALID; };
  if (d.n_objects > 0xFFFFFFFFull || d.n_triangles > CTR_SCENE_TRIS_MAX || d.cam.w > 0x7FFFFFFFull ||
      d.cam.h > 0x7FFFFFFFull)
    return bad("scene too large for 32-bit device indices");
  if (d.cam.w * d.cam.h > 0x7FFFFFFFull * 2) return bad("image too large");
  for (uint64_t i = 0; i < d.n_objects; i++) {
    const ctr_object &o = d.objects[i];
    if (o.type > CTR_OBJ_SPHERE) return bad("object #" + std::to_string(i) + ": bad type");
    if (o.mat_idx >= d.n_materials) return bad("object #" + std::to_string(i) + ": material index out of range");
    if (o.type == CTR_OBJ_MESH && (o.tri_begin > d.n_triangles || o.tri_count > d.n_triangles - o.tri_begin))
      return bad("object #" + std::to_string(i) + ": triangle range out of bounds");
  }
  for (uint64_t i = 0; i < d.n_lights; i++)
    if (d.lights[i].type > CTR_LIGHT_POINT) return bad("light #" + std::to_string(i) + ": bad type");
  for (uint64_t i = 0; i < d.n_materials; i++)
    if (d.materials[i].type != CTR_MAT_PHONG) return bad("material #" + std::to_string(i) + ": bad type");
  return CTR_OK;
}

int flatten_scene(const ctr_scene_desc &d, FlatScene &F, std::string &err) {
  F = FlatScene();
  if (int st = object_records(d, mesh_trees(d), F, err)) return st;
  create_stamp("meshes: BVH + records");
  plane_records(F);
  const std::vector<DObj> in_scene_order = nonempty_meshes(F);
  top_level(in_scene_order, F);
  reserve_merged(d, in_scene_order, F);
  light_records(F, d.lights, d.n_lights);
  material_records(F, d.materials, d.n_materials);
  for (const MeshGuard &g : F.guards) F.mesh_tris += g.tri_count;
  F.mesh_bytes = F.tris.size() * sizeof(DTri) + F.nodes.size() * sizeof(DNode) + F.nodes4.size() * sizeof(DNode4);
  F.ray_slots = ray_stack_slots(F);
  create_stamp("planes, top level, materials");
  return CTR_OK;
}

std::vector<DirtyRange> build_merged_tree(FlatScene &F) {
  Merged &M = F.merged;
  if (!M.reserved || M.built) return {};
  const uint32_t total = M.tri_count, n_rank = (uint32_t)M.slot_of.size() - 1;
  std::vector<uint32_t> rank_of(total);
  for (uint32_t r = 0; r < n_rank; r++)
    for (uint32_t k = M.slot_of[r]; k < M.slot_of[r + 1]; k++) rank_of[k] = r;
  std::vector<DNode4> mnodes;
  std::vector<uint32_t> order;
  bvh4_build(tri_boxes(M.src.data(), total), BVH_LEAF, mnodes, order);
  if (mnodes.size() > M.node_cap) return {};  // (cannot happen for leaves of up to four triangles; then simply never used)
  M.node_count = (uint32_t)mnodes.size();
  std::copy(mnodes.begin(), mnodes.end(), F.nodes4.begin() + M.node_begin);
  M.where.assign(total, 0u);
  float dummy_gn[4];
  for (uint32_t k = 0; k < total; k++) {
    const uint32_t g = order[k], r = rank_of[g], f = g - M.slot_of[r];
    const ctr_triangle &t = M.src[g];
    make_tri(t.p1, t.p2, t.p3, (r << 24) | f, F.tris[M.tri_begin + k], dummy_gn);
    M.where[g] = k;
  }
  for (uint32_t k = 0; k < CTR_GUARD_SLOTS; k++) F.tris[M.tri_begin + total + k] = F.tris[M.tri_begin];
  DObj &P = F.meshes[F.n_mesh];
  P.node_count = M.node_count;
  P.bvh_root = 0;
  M.built = true;
  M.guarded.assign(1, 0xFFFFFFFFu);  // (no key: the first apply_guards writes the guard state, empty or not)
  return {{DirtyRange::TRIS, M.tri_begin, (size_t)total + CTR_GUARD_SLOTS, {}},
          {DirtyRange::NODES4, M.node_begin, M.node_count, {}},
          {DirtyRange::MESHES, F.n_mesh, 1, {}}};
}

namespace {
// the box of the subtree behind top-level descriptor `d`, its nodes' boxes recomputed on the way (same shape, new boxes)
void refit_top(FlatScene &F, uint32_t d, float *mn, float *mx) {
  for (int a = 0; a < 3; a++) { mn[a] = INFINITY; mx[a] = -INFINITY; }
  if (d & BVH_LEAF_FLAG) {
    const uint32_t first = d & 0xFFFFFFu, count = (d >> 24) & 0x7Fu;
    for (uint32_t k = first; k < first + count && k < F.n_mesh; k++)
      for (int a = 0; a < 3; a++) { mn[a] = fminf(mn[a], F.meshes[k].f[a]); mx[a] = fmaxf(mx[a], F.meshes[k].f[3 + a]); }
    return;
  }
  DNode &N = F.nodes[F.tlas_begin + d];
  const uint32_t kid[2] = {N.left, N.right};
  for (int c = 0; c < 2; c++) {
    float lo[3], hi[3];
    refit_top(F, kid[c], lo, hi);
    for (int a = 0; a < 3; a++) {
      N.mn[a][c] = lo[a]; N.mx[a][c] = hi[a];
      mn[a] = fminf(mn[a], lo[a]); mx[a] = fmaxf(mx[a], hi[a]);
    }
  }
}
}  // namespace

std::vector<DirtyRange> mesh_updated(FlatScene &F, size_t gi, const float *box) {
  std::vector<DirtyRange> dirty;
  MeshGuard &g = F.guards[gi];
  if (g.mesh_pos < 0) return dirty;
  // the mesh's box, wherever a record of the mesh is kept (apply_guards uploads objs[] and meshes[mesh_pos] with bvh_root)
  for (int q = 0; q < 6; q++) F.objs[g.obj_index].f[q] = F.meshes[g.mesh_pos].f[q] = box[q];
  for (size_t k = F.n_mesh + 1; k < F.meshes.size(); k++)
    if (F.meshes[k].index == g.obj_index) {
      for (int q = 0; q < 6; q++) F.meshes[k].f[q] = box[q];
      dirty.push_back({DirtyRange::MESHES, k, 1, {}});
    }
  dirty.push_back({DirtyRange::OBJS, g.obj_index, 1, {}});
  dirty.push_back({DirtyRange::MESHES, (size_t)g.mesh_pos, 1, {}});
  // the top-level tree over the meshes' boxes, and the box of all meshes
  refit_top(F, F.tlas_root, F.tl_mn, F.tl_mx);
  if (F.nodes.size() > F.tlas_begin) dirty.push_back({DirtyRange::NODES, F.tlas_begin, F.nodes.size() - F.tlas_begin, {}});
  if (F.meshes.size() > F.n_mesh) {  // the merged pseudo mesh carries the box of all meshes
    for (int a = 0; a < 3; a++) { F.meshes[F.n_mesh].f[a] = F.tl_mn[a]; F.meshes[F.n_mesh].f[3 + a] = F.tl_mx[a]; }
    dirty.push_back({DirtyRange::MESHES, F.n_mesh, 1, {}});
  }
  // unused guard records: copies of the first triangle, as mesh_record leaves them
  const uint32_t slot0 = g.tri_begin + g.tri_count;
  for (uint32_t k = 0; k < CTR_GUARD_SLOTS; k++) {
    F.tris[slot0 + k] = F.tris[g.tri_begin];
    for (int q = 0; q < 4; q++) F.gn[4 * (slot0 + k) + q] = F.gn[4 * g.tri_begin + q];
  }
  dirty.push_back({DirtyRange::TRIS, slot0, CTR_GUARD_SLOTS, {}});
  dirty.push_back({DirtyRange::GNORM, slot0, CTR_GUARD_SLOTS, {}});
  // The guard state describes records that no longer exist.  guarded: no list of triangles equals this one, so apply_guards
  // writes the mesh's guard records, spare node and bvh_root whatever the new plan says.  linear: the refit wrote REAL boxes
  // into the device's nodes, so a mesh that was linear is not any more — left at true, a plan that keeps it linear would find
  // nothing to do and the device would cull a mesh whose in-plane triangles need every lane.  At false the plan's `linear`
  // differs and apply_guards sends the unbounded payload again.
  g.guarded.assign(1, 0xFFFFFFFFu);
  g.linear = false;
  // the merged tree holds the old triangles: retired for good (ctr_set_variant: not reserved, so never built again;
  // kernel_facts: not usable, so CTR_VAR_MERGE takes the two-level walk)
  F.merged.reserved = F.merged.built = F.merged.usable = false;
  std::vector<ctr_triangle>().swap(F.merged.src);
  return dirty;
}

MeshTree host_mesh_tree(const ctr_triangle *tris, size_t n, uint32_t leaf_size) {
  MeshTree tree;
  bvh4_build(tri_boxes(tris, n), leaf_size, tree.nodes, tree.order);
  return tree;
}

namespace {
// `tree` becomes the tree of mesh guards[gi]: in place when it fits the mesh's node range, else in a new range at the end of
// nodes4 with room for `cap_if_moved` nodes and the spare node.  The ranges and the root go wherever a record of the mesh keeps
// them, the records' `orig` take the leaf order (over the guard's CURRENT triangle range and count).
std::vector<DirtyRange> install_tree(FlatScene &F, size_t gi, const MeshTree &tree, uint32_t cap_if_moved, bool *moved) {
  MeshGuard &g = F.guards[gi];
  const uint32_t count = (uint32_t)tree.nodes.size();
  *moved = count > g.node_cap;
  if (*moved) {  // a new range at the end: the tree's nodes and, right behind them, its spare node
    g.node_begin = (uint32_t)F.nodes4.size();
    g.node_cap = cap_if_moved;
    F.nodes4.resize(F.nodes4.size() + cap_if_moved + 1u);
  }
  std::copy(tree.nodes.begin(), tree.nodes.end(), F.nodes4.begin() + g.node_begin);
  memset(&F.nodes4[g.node_begin + count], 0, sizeof(DNode4));  // the spare node, unused = all zero (mesh_record)
  for (uint32_t k = count + 1u; k <= g.node_cap; k++) F.nodes4[g.node_begin + k] = empty_node4();
  g.node_count = count;
  std::vector<DirtyRange> dirty{{DirtyRange::NODES4, g.node_begin, (size_t)g.node_cap + 1u, {}}};
  // the ranges and the root, wherever a record of the mesh is kept (mesh_updated's list)
  auto put = [&](DObj &O) { O.tri_begin = g.tri_begin; O.tri_count = g.tri_count; O.node_begin = g.node_begin; O.node_count = count; O.bvh_root = 0; };
  put(F.objs[g.obj_index]);
  dirty.push_back({DirtyRange::OBJS, g.obj_index, 1, {}});
  if (g.mesh_pos >= 0) {
    put(F.meshes[g.mesh_pos]);
    dirty.push_back({DirtyRange::MESHES, (size_t)g.mesh_pos, 1, {}});
  }
  for (size_t k = F.n_mesh + 1; k < F.meshes.size(); k++)
    if (F.meshes[k].index == g.obj_index) {
      put(F.meshes[k]);
      dirty.push_back({DirtyRange::MESHES, k, 1, {}});
    }
  for (uint32_t k = 0; k < g.tri_count; k++) F.tris[g.tri_begin + k].orig = tree.order[k];
  F.mesh_bytes = F.tris.size() * sizeof(DTri) + F.nodes.size() * sizeof(DNode) + F.nodes4.size() * sizeof(DNode4);
  F.ray_slots = ray_stack_slots(F);
  return dirty;
}
}  // namespace

std::vector<DirtyRange> mesh_rebuilt(FlatScene &F, size_t gi, const MeshTree &tree, bool *moved) {
  return install_tree(F, gi, tree, (uint32_t)tree.nodes.size(), moved);
}

ReplaceRoom replace_room(const FlatScene &F, size_t gi, uint32_t n, uint32_t node_count, uint32_t growth) {
  const MeshGuard &g = F.guards[gi];
  ReplaceRoom r;
  r.tris_move = n > g.tri_cap;
  r.tri_cap = r.tris_move ? std::max(n, growth * g.tri_cap) : g.tri_cap;
  r.tris_after = F.tris.size() + (r.tris_move ? (size_t)r.tri_cap + CTR_GUARD_SLOTS : 0u);
  r.nodes_move = node_count > g.node_cap;
  r.node_cap = r.nodes_move ? std::max(node_count, growth * g.node_cap) : g.node_cap;
  r.nodes4_after = F.nodes4.size() + (r.nodes_move ? (size_t)r.node_cap + 1u : 0u);
  return r;
}

size_t live_mesh_bytes(const FlatScene &F) {
  size_t tris = 0, nodes4 = 0;
  for (const DObj &O : F.objs) tris += O.type == CTR_OBJ_TRIANGLE;
  for (const MeshGuard &g : F.guards) {
    tris += g.tri_count + (g.tri_count ? CTR_GUARD_SLOTS : 0u);
    nodes4 += g.node_count + 1u;
  }
  return tris * sizeof(DTri) + F.nodes.size() * sizeof(DNode) + nodes4 * sizeof(DNode4);
}

std::vector<DirtyRange> mesh_replaced(FlatScene &F, size_t gi, uint32_t n, const MeshTree &tree, bool *tris_moved, bool *nodes_moved) {
  MeshGuard &g = F.guards[gi];
  const ReplaceRoom room = replace_room(F, gi, n, (uint32_t)tree.nodes.size());
  *tris_moved = room.tris_move;
  if (room.tris_move) {  // a new range at the end: the records and, right behind them, the spare records
    DTri zero;
    memset(&zero, 0, sizeof(zero));
    g.tri_begin = (uint32_t)F.tris.size();
    g.tri_cap = room.tri_cap;
    F.tris.resize(room.tris_after, zero);
    F.gn.resize(4 * room.tris_after, 0.0f);
  }
  F.mesh_tris = F.mesh_tris - g.tri_count + n;
  g.tri_count = n;
  g.planes.assign((size_t)CTR_PLANE_DOUBLES * n, 0.0);  // (the update's steps fill them)
  std::vector<DirtyRange> dirty = install_tree(F, gi, tree, room.node_cap, nodes_moved);
  F.mesh_bytes = live_mesh_bytes(F);
  return dirty;
}

void light_records(FlatScene &F, const ctr_light *lights, uint64_t n) {
  F.lights.resize(n);
  for (uint64_t i = 0; i < n; i++) {
    const ctr_light &l = lights[i];
    F.lights[i] = DLight{l.type, l.v.x, l.v.y, l.v.z, l.color.x, l.color.y, l.color.z, 0.f};
  }
  shading_flags(F);
}

namespace {
// material::is_transparent (default_schema.hpp:334: `transparency >= 1e-6`, a double comparison), ray_cast's
// ignore_transparent: the bit travels with every record of an object.  Returns what the device has to receive, nothing when
// no bit changed.
std::vector<DirtyRange> transparency_bits(FlatScene &F) {
  bool changed = false;
  auto bit_of = [&](uint32_t obj) { return ((double)F.mats[F.objs[obj].mat].transparency >= 1e-6) ? 1u : 0u; };
  auto put = [&](uint32_t &word, uint32_t tr) { changed |= word != tr; word = tr; };
  auto put_obj = [&](DObj &O) {
    if (O.index >= F.objs.size()) return;  // (the merged pseudo mesh)
    uint32_t word;
    memcpy(&word, &O.f[7], sizeof(word));
    put(word, bit_of(O.index));
    memcpy(&O.f[7], &word, sizeof(word));
  };
  for (DObj &O : F.objs) put_obj(O);
  for (DObj &O : F.oloop) put_obj(O);
  for (DObj &O : F.meshes) put_obj(O);
  for (DPlanePair &pr : F.planes)
    for (int slot = 0; slot < 2; slot++)
      if (pr.index[slot] != CTR_PLANE_PAD) put(pr.transparent[slot], bit_of(pr.index[slot]));
  if (!changed) return {};
  return {{DirtyRange::OBJS, 0, F.objs.size(), {}}, {DirtyRange::OLOOP, 0, F.oloop.size(), {}},
          {DirtyRange::MESHES, 0, F.meshes.size(), {}}, {DirtyRange::PLANES, 0, F.planes.size(), {}}};
}
}  // namespace

std::vector<DirtyRange> material_records(FlatScene &F, const ctr_material *mats, uint64_t n) {
  F.mats.resize(n);
  for (uint64_t i = 0; i < n; i++) {
    const ctr_material &m = mats[i];
    F.mats[i] = DMat{m.color.x, m.color.y, m.color.z, m.specular, m.reflexivity, m.phong_exp, m.transparency, 0.f};
  }
  shading_flags(F);
  return transparency_bits(F);
}

int check_objects(const FlatScene &F, const ctr_object *objects, uint64_t n, std::string &err) {
  auto bad = [&](const std::string &msg) { err = msg; return CTR_E_INVALID; };
  if (!objects && n) return bad("null argument");
  if (n != F.objs.size()) return bad(std::to_string(n) + " objects for a scene of " + std::to_string(F.objs.size()) + ": the count is fixed");
  for (uint64_t i = 0; i < n; i++) {
    const ctr_object &o = objects[i];
    const DObj &O = F.objs[i];
    const std::string who = "object #" + std::to_string(i) + ": ";
    if (o.type > CTR_OBJ_SPHERE) return bad(who + "bad type");
    if (o.type != O.type) return bad(who + "type " + std::to_string(o.type) + " for an object of type " + std::to_string(O.type) + ": the type is fixed");
    if (o.type == CTR_OBJ_MESH && o.tri_count != O.tri_count)
      return bad(who + std::to_string(o.tri_count) + " triangles for a mesh of " + std::to_string(O.tri_count) + ": the count is fixed");
    if (o.mat_idx >= F.mats.size()) return bad(who + "material index out of range");
  }
  return CTR_OK;
}

std::vector<DirtyRange> objects_edited(FlatScene &F, const ctr_object *objects, uint64_t n) {
  std::vector<DirtyRange> dirty;
  for (uint64_t i = 0; i < n; i++) {
    DObj &O = F.objs[i];
    analytic_record(objects[i], O, F);
    if (O.type == CTR_OBJ_TRIANGLE) {
      dirty.push_back({DirtyRange::TRIS, O.tri_begin, 1, {}});
      dirty.push_back({DirtyRange::GNORM, O.tri_begin, 1, {}});
    }
    // a mesh's material, wherever a record of the mesh is kept (top-level leaf order, and scene order behind the merged pseudo mesh)
    if (O.type == CTR_OBJ_MESH)
      for (DObj &M : F.meshes)
        if (M.index == O.index) M.mat = O.mat;
  }
  plane_records(F);  // oloop: copies of the edited records; planes: which records exist, their order and their number
  transparency_bits(F);
  dirty.push_back({DirtyRange::OBJS, 0, F.objs.size(), {}});
  dirty.push_back({DirtyRange::OLOOP, 0, F.oloop.size(), {}});
  dirty.push_back({DirtyRange::MESHES, 0, F.meshes.size(), {}});
  dirty.push_back({DirtyRange::PLANES, 0, F.planes.size(), {}});
  return dirty;
}

ctr_object object_of(const FlatScene &F, size_t i) {
  const DObj &O = F.objs[i];
  ctr_object o{};
  o.type = O.type;
  o.mat_idx = O.mat;
  o.v0 = ctr_vec3{O.f[0], O.f[1], O.f[2]};
  switch (O.type) {
    case CTR_OBJ_TRIANGLE: {
      const DTri &T = F.tris[O.tri_begin];
      o.v1 = ctr_vec3{T.px, T.py, T.pz};
      o.v2 = ctr_vec3{O.f[3], O.f[4], O.f[5]};
      break;
    }
    case CTR_OBJ_MESH:
      o.tri_count = O.tri_count;
      [[fallthrough]];
    case CTR_OBJ_PLANE:
      o.v1 = ctr_vec3{O.f[3], O.f[4], O.f[5]};
      break;
    default:
      o.f0 = O.f[3];
      break;
  }
  return o;
}

size_t plane_records_at_most(const FlatScene &F) {
  size_t n = 0;
  for (const DObj &O : F.objs) n += O.type == CTR_OBJ_PLANE;
  return plane_records_at_most(n);
}

size_t plane_records_at_most(size_t n) {
  // `a` planes on the busiest axis cost 3 * ceil(a / 2) records (planes on the other two axes ride in the same triples), the
  // n - a general ones ceil((n - a) / 2); fewer than three axis-aligned planes: general pairs only.  Not monotonic in `a`: four
  // planes need 7 records with three on one axis beside a general one, 6 with all four on it.
  size_t most = (n + 1) / 2;
  for (size_t a = 3; a <= n; a++) most = std::max(most, 3 * ((a + 1) / 2) + (n - a + 1) / 2);
  return most;
}

namespace {
// the merged tree, retired as mesh_updated retires it, and its records behind meshes[n_mesh] dropped: they name objects by index
void retire_merged(FlatScene &F) {
  F.merged.reserved = F.merged.built = F.merged.usable = false;
  std::vector<ctr_triangle>().swap(F.merged.src);
  F.meshes.resize(F.n_mesh);
}

// the top-level tree over the meshes' current boxes in scene order, and every guard's place in it; the merged tree is retired
void top_level_again(FlatScene &F) {
  F.nodes.clear();
  F.meshes.clear();
  F.tlas_root = BVH_LEAF_FLAG;
  for (int a = 0; a < 3; a++) F.tl_mn[a] = F.tl_mx[a] = 0.0f;
  F.has_mesh = false;
  for (const DObj &O : F.objs) F.has_mesh |= O.type == CTR_OBJ_MESH;
  for (MeshGuard &g : F.guards) g.mesh_pos = -1;
  top_level(nonempty_meshes(F), F);
  retire_merged(F);
}

// the counters flatten_scene ends with, derived anew (mesh_bytes: of the live records, as mesh_replaced leaves it)
void derived_counters(FlatScene &F) {
  F.mesh_tris = 0;
  for (const MeshGuard &g : F.guards) F.mesh_tris += g.tri_count;
  F.mesh_bytes = live_mesh_bytes(F);
  F.ray_slots = ray_stack_slots(F);
}

// every record of the arrays that hold one per object, per plane pair, per mesh or per top-level node
void whole_lists(const FlatScene &F, std::vector<DirtyRange> &dirty) {
  dirty.push_back({DirtyRange::OBJS, 0, F.objs.size(), {}});
  dirty.push_back({DirtyRange::OLOOP, 0, F.oloop.size(), {}});
  dirty.push_back({DirtyRange::MESHES, 0, F.meshes.size(), {}});
  dirty.push_back({DirtyRange::PLANES, 0, F.planes.size(), {}});
  dirty.push_back({DirtyRange::NODES, 0, F.nodes.size(), {}});
}

void give_back(std::vector<FlatScene::FreeRange> &list, uint32_t begin, uint32_t count) {
  auto at = list.begin();
  while (at != list.end() && at->begin < begin) ++at;
  list.insert(at, FlatScene::FreeRange{begin, count});
}

// the lowest-addressed freed range of at least `need` records (exactly: of `need` records and no more), or list.size()
size_t fitting(const std::vector<FlatScene::FreeRange> &list, size_t need, bool exactly = false) {
  size_t k = 0;
  while (k < list.size() && (exactly ? list[k].count != need : list[k].count < need)) k++;
  return k;
}
}  // namespace

int check_new_object(const FlatScene &F, const ctr_object &o, std::string &err) {
  auto bad = [&](const std::string &msg) { err = msg; return CTR_E_INVALID; };
  if (o.type > CTR_OBJ_SPHERE) return bad("bad type");
  if (o.type == CTR_OBJ_MESH) return bad("a mesh is added by ctr_scene_add_mesh");
  if (o.mat_idx >= F.mats.size()) return bad("material index out of range");
  if (F.objs.size() >= 0xFFFFFFFFull) return bad("scene too large for 32-bit device indices");
  return CTR_OK;
}

std::vector<DirtyRange> object_added(FlatScene &F, const ctr_object &o, bool *tri_reused) {
  std::vector<DirtyRange> dirty;
  DObj O;
  memset(&O, 0, sizeof(O));
  O.type = o.type;
  O.index = (uint32_t)F.objs.size();
  if (tri_reused) *tri_reused = false;
  if (o.type == CTR_OBJ_TRIANGLE) {
    const size_t k = fitting(F.free_tris, 1, true);
    if (k < F.free_tris.size()) {
      O.tri_begin = F.free_tris[k].begin;
      F.free_tris.erase(F.free_tris.begin() + k);
      if (tri_reused) *tri_reused = true;
    } else {
      O.tri_begin = (uint32_t)F.tris.size();
      F.tris.emplace_back();
      F.gn.resize(4 * F.tris.size());
    }
    O.tri_count = 1;
    dirty.push_back({DirtyRange::TRIS, O.tri_begin, 1, {}});
    dirty.push_back({DirtyRange::GNORM, O.tri_begin, 1, {}});
  }
  F.objs.push_back(O);
  analytic_record(o, F.objs.back(), F);
  plane_records(F);
  retire_merged(F);
  transparency_bits(F);
  derived_counters(F);
  whole_lists(F, dirty);
  return dirty;
}

AddRoom add_room(const FlatScene &F, uint32_t n, uint32_t node_count) {
  AddRoom r;
  const size_t kt = fitting(F.free_tris, (size_t)n + CTR_GUARD_SLOTS), kn = fitting(F.free_nodes4, (size_t)node_count + 1u);
  r.tris_reused = kt < F.free_tris.size();
  r.tri_begin = r.tris_reused ? F.free_tris[kt].begin : (uint32_t)F.tris.size();
  r.tri_cap = r.tris_reused ? F.free_tris[kt].count - CTR_GUARD_SLOTS : n;
  r.tris_after = F.tris.size() + (r.tris_reused ? 0u : (size_t)n + CTR_GUARD_SLOTS);
  r.nodes_reused = kn < F.free_nodes4.size();
  r.node_begin = r.nodes_reused ? F.free_nodes4[kn].begin : (uint32_t)F.nodes4.size();
  r.node_cap = r.nodes_reused ? F.free_nodes4[kn].count - 1u : node_count;
  r.nodes4_after = F.nodes4.size() + (r.nodes_reused ? 0u : (size_t)node_count + 1u);
  return r;
}

std::vector<DirtyRange> mesh_added(FlatScene &F, uint64_t mat_idx, uint32_t n, const MeshTree &tree) {
  const AddRoom room = add_room(F, n, (uint32_t)tree.nodes.size());
  DObj O;
  memset(&O, 0, sizeof(O));
  O.type = CTR_OBJ_MESH;
  O.index = (uint32_t)F.objs.size();
  O.mat = (uint32_t)mat_idx;
  F.objs.push_back(O);
  F.has_mesh = true;
  transparency_bits(F);
  // A guard entry of no room takes the freed ranges as its own, and mesh_replaced then finds that the mesh fits them; what is not
  // reused it moves to the end of the arrays, with exactly the room needed (twice no room is no room).
  MeshGuard g;
  g.obj_index = O.index;
  if (room.tris_reused) {
    g.tri_begin = room.tri_begin;
    g.tri_cap = room.tri_cap;
    F.free_tris.erase(F.free_tris.begin() + fitting(F.free_tris, (size_t)n + CTR_GUARD_SLOTS));
  }
  if (room.nodes_reused) {
    g.node_begin = room.node_begin;
    g.node_cap = room.node_cap;
    F.free_nodes4.erase(F.free_nodes4.begin() + fitting(F.free_nodes4, tree.nodes.size() + 1u));
  }
  F.guards.push_back(std::move(g));
  bool tris_moved = false, nodes_moved = false;
  std::vector<DirtyRange> dirty = mesh_replaced(F, F.guards.size() - 1, n, tree, &tris_moved, &nodes_moved);
  dirty.push_back({DirtyRange::OBJS, 0, F.objs.size(), {}});
  return dirty;
}

std::vector<DirtyRange> mesh_joined(FlatScene &F, size_t gi, const float *box) {
  for (int q = 0; q < 6; q++) F.objs[F.guards[gi].obj_index].f[q] = box[q];
  top_level_again(F);
  std::vector<DirtyRange> dirty;
  whole_lists(F, dirty);
  const std::vector<DirtyRange> more = mesh_updated(F, gi, box);
  dirty.insert(dirty.end(), more.begin(), more.end());
  derived_counters(F);
  return dirty;
}

std::vector<DirtyRange> object_removed(FlatScene &F, size_t i, long *guard_removed) {
  const DObj gone = F.objs[i];
  *guard_removed = -1;
  if (gone.type == CTR_OBJ_TRIANGLE) give_back(F.free_tris, gone.tri_begin, 1);
  if (gone.type == CTR_OBJ_MESH) {
    size_t gi = 0;
    while (gi < F.guards.size() && F.guards[gi].obj_index != i) gi++;
    if (gi < F.guards.size()) {
      const MeshGuard &g = F.guards[gi];
      if (g.tri_cap) give_back(F.free_tris, g.tri_begin, g.tri_cap + CTR_GUARD_SLOTS);
      give_back(F.free_nodes4, g.node_begin, g.node_cap + 1u);
      F.guards.erase(F.guards.begin() + gi);
      *guard_removed = (long)gi;
    }
  }
  F.objs.erase(F.objs.begin() + i);
  for (size_t k = i; k < F.objs.size(); k++) F.objs[k].index = (uint32_t)k;
  for (MeshGuard &g : F.guards)
    if (g.obj_index > i) g.obj_index--;
  plane_records(F);
  top_level_again(F);
  transparency_bits(F);
  derived_counters(F);
  std::vector<DirtyRange> dirty;
  whole_lists(F, dirty);
  return dirty;
}

SceneRoom scene_room(const FlatScene &F) {
  SceneRoom r{0, F.tris.size(), 0, F.nodes4.size()};
  for (const DObj &O : F.objs) r.tris_live += O.type == CTR_OBJ_TRIANGLE;
  for (const MeshGuard &g : F.guards) {
    r.tris_live += g.tri_cap + (g.tri_cap ? CTR_GUARD_SLOTS : 0u);
    r.nodes4_live += g.node_cap + 1u;
  }
  return r;
}

void fill_scene_counts(const FlatScene &F, DScene &D) {
  D.n_mesh = F.n_mesh;
  D.tlas_root = D.tlas_root_regular = F.tlas_root;  // (a launch of a build that walks the merged tree puts that tree into tlas_root)
  D.tlas_begin = F.tlas_begin;
  for (int q = 0; q < 3; q++) { D.tl_mn[q] = F.tl_mn[q]; D.tl_mx[q] = F.tl_mx[q]; }
  D.n_oloop = (uint32_t)F.oloop.size(); D.n_plane_recs = (uint32_t)F.planes.size(); D.n_axis_recs = F.n_axis_recs;
  D.n_obj = (uint32_t)F.objs.size(); D.n_light = (uint32_t)F.lights.size(); D.n_mat = (uint32_t)F.mats.size();
  D.has_mesh = F.has_mesh ? 1u : 0u; D.need_cold_frames = F.need_cold ? 1u : 0u; D.any_bounce = F.any_bounce ? 1u : 0u;
}

void fill_scene_head(const FlatScene &F, uint32_t tlas_root, DSceneHead &H) {
  H = DSceneHead{};
  if (F.n_axis_recs >= 3u && F.planes.size() >= 3u) {
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 2; k++) {
        H.ax[2 * r][k] = F.planes[r].p[r][k];
        H.ax[2 * r + 1][k] = F.planes[r].n[r][k];
        H.ax_index[2 * r + k] = F.planes[r].index[k];
        H.ax_transparent[2 * r + k] = F.planes[r].transparent[k];
      }
    H.n_axis_recs = 3u;
  }
  const uint32_t leaf = tlas_root & 0xFFFFFFu;
  if (F.n_mesh != 0u && (tlas_root & BVH_LEAF_FLAG) && leaf < F.meshes.size()) {
    H.mesh = F.meshes[leaf];
    H.mesh_dark |= CTR_HEAD_MESH;
  }
}

// DESIGN.md "Shadow casts from inside a plane room" has the derivation; the names are its names.
void room_facts(DSceneHead &H, const DLight *lights, size_t n_light, const RoomTuning &tune) {
  for (int a = 0; a < 3; a++) H.room_c[a] = 0.0f;
  H.room_r = H.room_delta = 0.0f;
  H.room_lights = 0u;
  if (H.n_axis_recs != 3u || n_light == 0 || n_light > 32) return;
  // the filled slots: axis, point coordinate, normal component
  struct Slot { int a; double p, n; };
  Slot slots[6];
  int n_slots = 0;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = 0; k < 6; k++) {
    if (H.ax_index[k] == CTR_PLANE_PAD) continue;
    const int a = k / 2;
    const double p = H.ax[2 * a][k & 1], n = H.ax[2 * a + 1][k & 1];
    // (magnitudes at which no product or quotient of the kernel's leaves the normal float range)
    if (!std::isfinite(p) || !(std::fabs(n) >= 1e-6 && std::fabs(n) <= 1e6) || !(std::fabs(p) <= 1e9)) return;
    slots[n_slots++] = {a, p, n};
    lo[a] = std::min(lo[a], p); hi[a] = std::max(hi[a], p);
  }
  if (n_slots == 0) return;
  bool any_point = false;
  for (size_t i = 0; i < n_light; i++) {
    if (lights[i].type != CTR_LIGHT_POINT) continue;
    const double v[3] = {lights[i].vx, lights[i].vy, lights[i].vz};
    if (!(std::fabs(v[0]) <= 1e9 && std::fabs(v[1]) <= 1e9 && std::fabs(v[2]) <= 1e9)) return;  // (also: not finite)
    for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    any_point = true;
  }
  if (!any_point) return;
  // the origin box: centred on the plane points and point lights, twice their largest half extent
  double half = 0.0;
  float c[3];
  for (int a = 0; a < 3; a++) {
    c[a] = (float)(0.5 * (lo[a] + hi[a]));
    half = std::max(half, std::max(hi[a] - (double)c[a], (double)c[a] - lo[a]));
  }
  const float r = (float)(2.0 * half);
  if (!(r >= 1e-9f && r <= 1e9f)) return;
  // what the kernel's float test |o - c| <= r lets through: the subtraction rounds once
  const double r_eff = (double)r * (1.0 + 0x1p-20);
  uint32_t mask = 0u;
  double t_max = 0.0, den_min = INFINITY;
  for (size_t i = 0; i < n_light; i++) {
    if (lights[i].type != CTR_LIGHT_POINT) continue;
    const double v[3] = {lights[i].vx, lights[i].vy, lights[i].vz};
    double t2 = 0.0;
    for (int a = 0; a < 3; a++) { const double e = std::fabs(v[a] - (double)c[a]) + r_eff; t2 += e * e; }
    t_max = std::max(t_max, std::sqrt(t2));
  }
  for (size_t i = 0; i < n_light; i++) {
    if (lights[i].type != CTR_LIGHT_POINT) continue;
    const double v[3] = {lights[i].vx, lights[i].vy, lights[i].vz};
    bool ok = true;
    double den_i = INFINITY;
    for (int k = 0; k < n_slots && ok; k++) {
      const Slot &S = slots[k];
      const double s_l = (v[S.a] - S.p) * S.n;                                        // the light's side of the plane, and how far
      const double s_max = (std::fabs((double)c[S.a] - S.p) + r_eff) * std::fabs(S.n);  // the same of any origin of the box, at most
      ok = s_l > 0.0 && s_l >= tune.k * 0x1p-24 * (t_max * std::fabs(S.n) + s_max);    // case b
      den_i = std::min(den_i, s_l / t_max);                                             // case c: the smallest den of a ray to it
    }
    if (ok) { mask |= 1u << i; den_min = std::min(den_min, den_i); }
  }
  if (mask == 0u) return;
  // case c: t0 <= delta / den <= min_t / 2, min_t = (float)1e-3 of every any-hit shadow ray; rounded down
  const float delta = (float)(0.5 * (double)(float)1e-3 * den_min * (1.0 - 0x1p-20) * tune.delta_scale);
  if (!(delta >= 1e-30f) || !std::isfinite(delta)) return;
  for (int a = 0; a < 3; a++) H.room_c[a] = c[a];
  H.room_r = r;
  H.room_delta = delta;
  H.room_lights = mask;
}

uint32_t shade_facts(const DMat *mats, size_t n_mat, const DLight *lights, size_t n_light) {
  bool finite = true, bounded = true;
  auto look = [&](float v) {
    if (!std::isfinite(v)) finite = false;
    if (!(std::fabs(v) <= CTR_SHADE_BOUND)) bounded = false;  // (a NaN is not bounded either)
  };
  for (size_t i = 0; i < n_mat; i++) { look(mats[i].cx); look(mats[i].cy); look(mats[i].cz); look(mats[i].specular); }
  for (size_t i = 0; i < n_light; i++) { look(lights[i].cx); look(lights[i].cy); look(lights[i].cz); }
  return (finite ? 1u : 0u) | (bounded ? 2u : 0u);
}

void fill_dark_skip(const FlatScene &F, DSceneHead &H, bool switched_off) {
  const bool holds = !switched_off && F.shade_finite && F.shade_bounded && F.all_opaque;
  H.mesh_dark = (H.mesh_dark & ~CTR_HEAD_DARK) | (holds ? CTR_HEAD_DARK : 0u);
}

void fill_room_facts(const FlatScene &F, DSceneHead &H, bool switched_off) {
  if (!switched_off && F.planes.size() == 3u && F.n_axis_recs == 3u && F.all_opaque) room_facts(H, F.lights.data(), F.lights.size());
  else room_facts(H, nullptr, 0);
}

bool env_switch(const char *name) {
  const char *e = getenv(name);
  return e && atoi(e) != 0;
}
