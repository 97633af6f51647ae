// scene_flatten.h — a ctr_scene_desc flattened into the arrays of scene_device.h, on the host, without a device.
//
// Everything ctr_scene_create (ctr_scene.cpp) uploads is built here, and stays here as the host copy that the guard of
// the BVH culling (guard.h) and the ray queries read and edit.  No HIP: scripts/flatten_check.cpp and
// tests/test_scene_flatten.py run this code on any CPU.
#ifndef CUTRACE_AMD_SCENE_FLATTEN_H
#define CUTRACE_AMD_SCENE_FLATTEN_H

#include <stdint.h>
#include <string>
#include <vector>

#include "bvh.h"
#include "cutrace_amd.h"
#include "scene_device.h"

#ifndef CTR_BVH_LEAF
#define CTR_BVH_LEAF 4
#endif
constexpr uint32_t BVH_LEAF = CTR_BVH_LEAF;  // triangles per BVH leaf

#define CTR_GUARD_SLOTS 64u  // spare DTri records per mesh (guard.h)
// The two limits on triangle counts, stated HERE alone (validate_desc and flatten_scene at create, ctr_scene_replace_mesh later):
// a leaf descriptor and a merged key keep a triangle's position inside its mesh in 24 bits, and every index into the record
// array must fit the device's 32-bit arithmetic with room to spare.
constexpr uint64_t CTR_MESH_TRIS_MAX = 0xFFFFFFull;     // triangles of one mesh
constexpr uint64_t CTR_SCENE_TRIS_MAX = 0x7FFFFFFFull;  // triangles of a description; records of FlatScene::tris after a replace
#define CTR_MERGED_SPARE_NODES ((CTR_GUARD_SLOTS + 2u) / 3u)  // the merged tree: three meshes' guard leaves per spare node

// Guard of the BVH culling (guard.h): what it needs to know of one mesh, and what it currently has on the device
struct MeshGuard {
  uint32_t node_begin = 0, node_count = 0;
  uint32_t node_cap = 0;  // tree nodes the mesh's range of nodes4 has room for (+ the spare node): the count it was created or moved with (mesh_rebuilt)
  uint32_t tri_begin = 0, tri_count = 0;  // the mesh's DTri range (leaf order); CTR_GUARD_SLOTS spare records follow it
  uint32_t tri_cap = 0;  // triangle records the range has room for, the spare records not counted: the count it was created or moved with (mesh_replaced)
  uint32_t obj_index = 0;                 // position in objs
  int mesh_pos = -1;                      // position in meshes (-1: an empty mesh, never walked)
  std::vector<double> planes;  // per triangle (leaf order): unit normal (3), a point of the plane (3), extent
  std::vector<uint32_t> guarded;          // triangles currently copied into the spare records
  bool linear = false;         // its nodes currently carry unbounded boxes
};

// ONE four-wide tree over the triangles of ALL meshes (scenes with 2..255 non-empty meshes; render_kernel.hip "merged
// walk"): its records are appended to tris / nodes4, a pseudo mesh record at meshes[n_mesh] leads to them, and
// meshes[n_mesh + 1 + r] is mesh r in SCENE order (a merged triangle's key names r in its upper 8 bits).
// With several meshes a cast otherwise walks the top-level tree, runs the reference's AABB test per mesh it reaches and
// sets up a walk per mesh it enters (a fifth of the vector and the densest scalar code of the 16-mesh frame).  The merged
// tree's records carry (mesh rank << 24 | file index) as their tie-break key — the reference's (object, triangle) order
// as one integer — and the mesh's own AABB test (default_schema.hpp:99-114: a ray that fails it misses the mesh whatever
// its triangles say) is applied afterwards, to the lanes the walk found something for.
// Built on demand (build_merged_tree, at the first ctr_set_variant with CTR_VAR_MERGE): flatten_scene only sets its room in
// the arrays aside and keeps the triangles.
struct Merged {
  bool reserved = false;   // the scene qualifies (2..255 non-empty meshes) and the arrays have room for the tree
  bool built = false;      // the structures exist (build_merged_tree: at the first ctr_set_variant with CTR_VAR_MERGE)
  uint32_t node_cap = 0;   // room for the tree's nodes in nodes4 (the spare nodes follow)
  std::vector<ctr_triangle> src;  // the meshes' triangles, scene order then file order (kept for the build)
  bool usable = false;     // ... and may be walked (apply_guards: no mesh went linear, the guard records fit)
  uint32_t tri_begin = 0, tri_count = 0, node_begin = 0, node_count = 0;
  std::vector<uint32_t> slot_of;  // per mesh rank: first index of its triangles in a (rank, file index) numbering (+ one past the last)
  std::vector<uint32_t> where;    // merged position of triangle (rank, file index) -> tri_begin-relative record index
  std::vector<uint32_t> guarded;  // keys currently in the guard records
};

// Records of a FlatScene array that a host-side edit changed: what the device copy has to receive, in this order.
struct DirtyRange {
  enum Array { OBJS, MESHES, TRIS, GNORM, NODES4, NODES, OLOOP, PLANES } array;
  size_t begin, count;          // in records (GNORM: four floats per record)
  std::vector<DNode4> payload;  // not empty: the device gets THESE nodes, FlatScene::nodes4 keeps the real boxes (a linear mesh)
};

struct FlatScene {
  std::vector<DObj> objs;      // every object, scene order
  std::vector<DObj> oloop;     // spheres and stand-alone triangles
  std::vector<DObj> meshes;    // non-empty meshes in top-level leaf order (+ the merged pseudo mesh and the meshes in scene order)
  std::vector<DPlanePair> planes;
  std::vector<DTri> tris;
  std::vector<DNode> nodes;    // top-level tree
  std::vector<DNode4> nodes4;  // per-mesh trees (the real boxes), each followed by its spare node; the merged tree's room
  std::vector<float> gn;
  std::vector<DLight> lights;
  std::vector<DMat> mats;
  uint32_t n_mesh = 0, tlas_root = BVH_LEAF_FLAG, tlas_begin = 0;
  float tl_mn[3] = {0, 0, 0}, tl_mx[3] = {0, 0, 0};
  uint32_t n_axis_recs = 0;
  bool has_mesh = false;
  bool all_opaque = true;
  bool need_cold = false;   // some material both reflects and transmits (>= 1e-6 each)
  bool any_bounce = false;  // some material reflects or transmits (>= 1e-6): the recursion can go below depth 0
  // the fast specular path, exp2(e * log2(x)) on a half vector normalised with v_rsq_f32, stays inside the colour tolerance:
  // x^e has condition number e, so its error is CTR_FAST_POW_KAPPA * e per unit of specular colour and light colour
  // (fast_pow_in_bar below; DESIGN.md "Shading parameters the kernels are pinned over")
  bool fast_pow_ok = true;
  // what lets a render skip the shadow casts of lights that cannot change a pixel (shade_facts below; DESIGN.md "Dark lights"):
  // shade_finite: every material's colour and `specular` and every light's colour is finite; shade_bounded: none of them exceeds
  // CTR_SHADE_BOUND in magnitude, so no product colour * specular * light colour overflows
  bool shade_finite = true, shade_bounded = true;
  uint64_t mesh_tris = 0;   // triangles in meshes
  size_t mesh_bytes = 0;    // triangles + BVH nodes
  std::vector<MeshGuard> guards;  // one per mesh object, scene order
  Merged merged;
  // Ranges of tris / gn and of nodes4 that a removed object left behind (object_removed), lowest address first: what
  // object_added and mesh_added place a new object in before the arrays grow.  A range is taken whole, never split or merged.
  struct FreeRange { uint32_t begin, count; };
  std::vector<FreeRange> free_tris, free_nodes4;
  // LDS stack entries per lane that the ray-query walk (ray_query.hip) can need: a node pushes at most three of its
  // children (the fourth is visited next), so the stack holds at most three entries per level above the current node.
  // The depth counts the inner nodes of the longest path of any mesh tree, plus the spare node in front of a guarded
  // root.  A tree's SHAPE changes only in mesh_rebuilt, which computes this anew (ray_stack_slots); boxes and guard leaves do
  // not count.  The query kernels size their LDS stacks from it per call.
  uint32_t ray_slots = 0;
};

// max |fs_fast - fs_reference| / e of the specular term fs = x^e, measured on one MI355X over the highlight rays of
// tests/test_gpu_shading_ranges.py at e = 32 ... 100 000: 2.38e-7 ... 2.41e-7 (profiles/shading_ranges/fastpow.txt; below e = 32
// the difference is the colour's own last bit, 2.4e-7 ... 4.8e-7 whatever e, and has nothing to do with the exponent)
constexpr double CTR_FAST_POW_KAPPA = 2.42e-7;
constexpr double CTR_COLOUR_TOL = 1e-4;  // the parity bar of the colour, per channel
// worst: the largest phong_exp * specular * colour channel of any material; lambda: the sum over the lights of the largest
// |colour channel| (the colour is linear in both).  The factor 2: a finite sample of highlight geometries underestimates
// the maximum.
inline bool fast_pow_in_bar(double worst, double lambda) { return 2.0 * CTR_FAST_POW_KAPPA * worst * lambda <= CTR_COLOUR_TOL; }

// The checks the kernel relies on (it trusts these indices).  CTR_OK, or CTR_E_INVALID and the message in `err`.
int validate_desc(const ctr_scene_desc &d, std::string &err);
// Flattens a description that passed validate_desc.  CTR_OK, or CTR_E_INVALID and the message in `err`.
int flatten_scene(const ctr_scene_desc &d, FlatScene &F, std::string &err);
// The merged tree of a scene that has room for it (Merged::reserved), built into the reserved ranges.  Returns the
// ranges it filled; none when there is nothing to build (not reserved, built already, or the tree outgrew its room).
std::vector<DirtyRange> build_merged_tree(FlatScene &F);

// After the triangle records, normals, guard planes and node boxes of mesh guards[gi] were replaced (ctr_scene_update_mesh,
// ctr_update.cpp: the device computed them, the host copy received them back) and `box` is the mesh's new box (min, max):
// everything else the host copy derives from them.  The box goes into the mesh's records (objs, meshes, its scene-order copy
// behind the merged pseudo mesh); the top-level tree keeps its shape and gets its boxes recomputed bottom-up, tl_mn / tl_mx
// with it; the mesh's unused guard records repeat its first triangle again, and its guard state is forgotten so that the next
// apply_guards writes the records, the spare node and — for a mesh that is linear — the unbounded payload anew; the merged
// tree is retired for the life of the scene (its triangles are stale: no room reserved, nothing built, nothing usable).
// Returns what the device has to receive.  ray_slots stays: no tree changed its shape.
std::vector<DirtyRange> mesh_updated(FlatScene &F, size_t gi, const float *box);

// A mesh's tree as a builder hands it over: nodes (node 0 the root, child descriptors relative to it, a parent before its
// children) and the leaf order, order[k] = the file index of the triangle at leaf position k.
struct MeshTree { std::vector<DNode4> nodes; std::vector<uint32_t> order; };
// the host's binned-SAH tree (bvh4_build) over `n` triangles, leaves of at most `leaf_size`: what flatten_scene builds per mesh
MeshTree host_mesh_tree(const ctr_triangle *tris, size_t n, uint32_t leaf_size = BVH_LEAF);
// FlatScene::ray_slots of the trees F holds now
uint32_t ray_stack_slots(const FlatScene &F);

// Another tree SHAPE for mesh guards[gi] (ctr_scene_rebuild_mesh, include/cutrace_rebuild.h): `tree` has passed level_schedule and
// its order is a permutation of the mesh's triangles.  The mesh owns node_cap + 1 records of nodes4.  A tree that fits is
// installed in place: its nodes, the spare node right behind the last of them (all zero, as mesh_record leaves it; apply_guards
// fills it), and empty_node4() in what remains of the range.  A tree that does not fit gets a new range at the END of nodes4,
// which grows by its nodes and its spare node (*moved = true; the old range is dead, nothing names it any more).  node_begin,
// node_count and bvh_root = 0 go wherever a record of the mesh keeps them (objs, meshes, the scene-order copy behind the merged
// pseudo mesh, the MeshGuard); the records' `orig` take the new leaf order; ray_slots and mesh_bytes are derived anew.
// The nodes' BOXES are whatever `tree` holds and the triangle records are stale but for `orig`: the update's steps follow
// (update_tris, refit_level with the NEW schedule, mesh_box, then mesh_updated, which also resets the guard state).
// Returns what the device has to receive of this step: the mesh's node range and its records in objs and meshes.
std::vector<DirtyRange> mesh_rebuilt(FlatScene &F, size_t gi, const MeshTree &tree, bool *moved);

// Another triangle COUNT for mesh guards[gi] (ctr_scene_replace_mesh, include/cutrace_replace.h): `tree` is a tree over the `n` new
// triangles (1 .. CTR_MESH_TRIS_MAX) that has passed level_schedule, its order a permutation of them.  The mesh owns tri_cap +
// CTR_GUARD_SLOTS records of tris / gn and node_cap + 1 records of nodes4.
//   n <= tri_cap   the triangle range stays where it is; the spare records follow the new count, at tri_begin + n; what lies
//                  behind them is dead
//   n >  tri_cap   a new range at the END of tris and gn, of max(n, CTR_REPLACE_GROWTH * tri_cap) + CTR_GUARD_SLOTS records
//                  (*tris_moved = true; the old range is dead, nothing names it any more)
// and the node range by the same rule with the same factor (mesh_rebuilt's move, with room to grow into; *nodes_moved).  Nothing
// else moves: a stand-alone triangle's record between two mesh ranges and the merged tree's room stay where they are.
// tri_begin and tri_count go wherever a record of the mesh keeps them, next to node_begin, node_count and bvh_root = 0 (objs,
// meshes, the scene-order copy behind the merged pseudo mesh, the MeshGuard); planes takes the new length; the records' `orig`
// take the tree's leaf order; mesh_tris and ray_slots are derived anew, and mesh_bytes counts the LIVE records only (the
// ranges the meshes name, the stand-alone triangles, the top-level tree; not the dead ranges, not the merged tree's room, which
// mesh_updated retires).  As after mesh_rebuilt the records are stale but for `orig` and the update's steps follow.
// replace_room says beforehand what the call will do, so that the device arrays can grow before anything is written; `growth`
// 1 is mesh_rebuilt's rule (a tree that does not fit gets exactly its room).
// Returns what the device has to receive of this step: the mesh's node range and its records in objs and meshes.
constexpr uint32_t CTR_REPLACE_GROWTH = 2;
struct ReplaceRoom {
  bool tris_move, nodes_move;
  uint32_t tri_cap, node_cap;        // of the mesh afterwards
  size_t tris_after, nodes4_after;   // records of FlatScene::tris (gn: four floats each) and ::nodes4 afterwards
};
ReplaceRoom replace_room(const FlatScene &F, size_t gi, uint32_t n, uint32_t node_count, uint32_t growth = CTR_REPLACE_GROWTH);
std::vector<DirtyRange> mesh_replaced(FlatScene &F, size_t gi, uint32_t n, const MeshTree &tree, bool *tris_moved, bool *nodes_moved);
// FlatScene::mesh_bytes of the live records, as mesh_replaced leaves it
size_t live_mesh_bytes(const FlatScene &F);

// The lights, or the materials, of a flattened scene replaced (flatten_scene itself, and ctr_scene_set_lights and
// ctr_scene_set_materials of include/cutrace_edit.h): the records, and all_opaque, need_cold, any_bounce and fast_pow_ok derived
// anew from both arrays.  The caller has checked what validate_desc checks: the types, and for materials that every object's
// index stays below `n`.  material_records also sets the "material is transparent" bit of every record of an object (objs,
// oloop, meshes, planes) and returns what the device has to receive of those, nothing when no bit changed.  Neither touches
// the guard: a light is a probe and a reflecting material makes a mirror, so plan_guards / apply_guards (guard.h) follow.
void light_records(FlatScene &F, const ctr_light *lights, uint64_t n);
std::vector<DirtyRange> material_records(FlatScene &F, const ctr_material *mats, uint64_t n);

// The parameters of a flattened scene's objects replaced (ctr_scene_set_objects of include/cutrace_objects.h); topology is fixed.
// check_objects: what validate_desc checks of an object, and that nothing but parameters differs — `n` is the scene's count,
// every type is the object's own, a mesh keeps its triangle count, every material index is below the scene's material count.
// CTR_OK, or CTR_E_INVALID and the message in `err`; F is not written.
// objects_edited, for objects that passed: a sphere's centre and radius, a plane's point and normal, a stand-alone triangle's
// three points (its DObj, its DTri and its normal at the tri_begin it has) and every object's material index through the text
// flatten_scene runs; a mesh's material into its `meshes` records as well, its triangles, tree and box staying what they are
// (tri_begin, v0 and v1 of a mesh are ignored); then, again with flatten_scene's text, oloop rebuilt (same count), planes and
// n_axis_recs re-packed — a plane that becomes or stops being axis-aligned changes which records exist, their order and their
// NUMBER, at most plane_records_at_most(F) — and the "material is transparent" bit of every record of an object.  Nothing else
// holds an analytic object's parameter or a material index (scripts/object_edit_check.cpp compares every array with
// flatten_scene of the edited description).  Returns what the device has to receive.  Does not touch the guard: a flat object
// that moves, or gains or loses a reflecting material, moves the eyes' images, so plan_guards / apply_guards (guard.h) follow.
// object_of: object `i` as a ctr_object that objects_edited would take back unchanged — a mesh with its CURRENT box in v0 / v1
// (after mesh_updated: the refitted one), its tri_count, and tri_begin 0.
int check_objects(const FlatScene &F, const ctr_object *objects, uint64_t n, std::string &err);
std::vector<DirtyRange> objects_edited(FlatScene &F, const ctr_object *objects, uint64_t n);
ctr_object object_of(const FlatScene &F, size_t i);
// the most plane records any edit of the scene's planes can need: the maximum, over how many of them share the busiest axis, of
// that axis's triples plus the general pairs of the rest (for an even count >= 4 one more than every plane on one axis)
size_t plane_records_at_most(const FlatScene &F);
size_t plane_records_at_most(size_t n_planes);  // ... of a scene with that many planes

// The object LIST of a flattened scene changes (include/cutrace_topology.h: ctr_scene_add_object, ctr_scene_add_mesh,
// ctr_scene_remove_object).  Afterwards the host copy is what flatten_scene gives for the edited description — the removed object
// deleted, an added one appended — but for where the ranges of tris / gn / nodes4 begin, and for the merged tree, which is retired
// as mesh_updated retires it (scripts/topology_check.cpp compares every array).  What holds an object index or a per-mesh slot, and
// is therefore written anew, with flatten_scene's own text:
//   objs            the record erased or appended, DObj::index renumbered
//   oloop, planes   copies of object records: plane_records (n_axis_recs with them; at most plane_records_at_most of the NEW plane
//                   set, which the caller gives d_planes room for)
//   guards          the entry erased or appended, obj_index renumbered, mesh_pos from the new top-level tree.  The caller keeps
//                   what it indexes by guard in step (ctr_scene::refit, the device scan's flat plane array)
//   nodes, meshes, n_mesh, tlas_root, tl_mn, tl_mx, has_mesh
//                   the top-level tree over the meshes' CURRENT boxes in scene order: top_level
//   merged          retired
//   mesh_tris, mesh_bytes (live_mesh_bytes), ray_slots, the "material is transparent" bits
// None of them touches the guard STATE of a mesh that stays (its guard records, spare node and bvh_root travel with its records):
// a flat mirror that comes or goes moves the eyes' images, so plan_guards / apply_guards (guard.h) follow.
//
// Ranges.  A removed mesh's tri_cap + CTR_GUARD_SLOTS triangle records (none for a mesh created empty) and node_cap + 1 nodes, and a
// removed stand-alone triangle's one record, go on FlatScene::free_tris / free_nodes4.  An added mesh takes, per array, the
// lowest-addressed freed range with enough room, whole — its tri_cap / node_cap are then the range's — and otherwise a new range at
// the end with exactly the room it needs; an added stand-alone triangle takes the lowest-addressed freed range of ONE record.
//
// check_new_object: what validate_desc checks of an object that ctr_scene_add_object takes (no mesh); F is not written.
int check_new_object(const FlatScene &F, const ctr_object &o, std::string &err);
// a sphere, a plane or a stand-alone triangle that passed, appended.  *tri_reused: a triangle's record is a freed one
std::vector<DirtyRange> object_added(FlatScene &F, const ctr_object &o, bool *tri_reused = nullptr);
// where mesh_added will put a mesh of `n` triangles under a tree of `node_count` nodes, so that the device arrays can grow first
struct AddRoom {
  bool tris_reused, nodes_reused;
  uint32_t tri_begin, tri_cap, node_begin, node_cap;
  size_t tris_after, nodes4_after;  // records of FlatScene::tris (gn: four floats each) and ::nodes4 afterwards
};
AddRoom add_room(const FlatScene &F, uint32_t n, uint32_t node_count);
// A mesh of `n` triangles (1 .. CTR_MESH_TRIS_MAX) with material `mat_idx` appended: its object record and MeshGuard (the last of
// both), its ranges where add_room says, and `tree` installed in them by mesh_replaced.  As after mesh_replaced the records are
// stale but for `orig`, and the mesh has no box and no place in the top-level tree yet (mesh_pos -1: nothing walks it): the
// update's steps follow (update_tris, refit_level, mesh_box), then mesh_joined.
std::vector<DirtyRange> mesh_added(FlatScene &F, uint64_t mat_idx, uint32_t n, const MeshTree &tree);
// ... and once `box` is known: the box into the mesh's object record, the top-level tree over all meshes, then mesh_updated
std::vector<DirtyRange> mesh_joined(FlatScene &F, size_t gi, const float *box);
// object `i` (any type, an empty mesh included) removed.  *guard_removed: the position its MeshGuard had, -1 for what is no mesh
std::vector<DirtyRange> object_removed(FlatScene &F, size_t i, long *guard_removed);
// records of tris and nodes4 in all, and inside a range some object owns (capacity plus spare records)
struct SceneRoom { uint64_t tris_live, tris_total, nodes4_live, nodes4_total; };
SceneRoom scene_room(const FlatScene &F);

// The counts and flags of a device scene record (scene_device.h DScene) from the host copy its arrays mirror; the ten pointers
// stay as they are.  Called per launch and per query, so that it is right after build_merged_tree and every guard refresh.
__attribute__((visibility("hidden"))) void fill_scene_counts(const FlatScene &F, DScene &D);

// The scene head of a launch whose top-level walk starts at `tlas_root` (scene_device.h DSceneHead): copies of planes[0..2]
// and of the mesh record behind a leaf root, as far as the scene has them; everything else zero.
void fill_scene_head(const FlatScene &F, uint32_t tlas_root, DSceneHead &H);

// The room facts of a head whose axis triple is filled (scene_device.h DSceneHead::room_*; DESIGN.md "Shadow casts from inside
// a plane room"), computed in double from the triple as the head holds it and the `n_light` records of `lights`: the origin box
// around the triple's plane points and the point lights, the numerator tolerance, and the bit of every point light that lies
// on the normal side of every filled slot by more than the margin.  All six words zero: no triple in the head, no point light,
// more than 32 lights, no light that qualifies, or numbers outside the range the derivation covers.  RoomTuning is what
// scripts/room_facts_check.cpp mutates; the library uses the defaults.
struct RoomTuning {
  double k = 16.0;           // case b: s_L >= k * 2^-24 * (T_max * |n| + S_max); the roundings between t0 and light_dist add up to 10 * 2^-24
  double delta_scale = 1.0;  // case c: room_delta = delta_scale * min_t / 2 * (smallest den)
};
void room_facts(DSceneHead &H, const DLight *lights, size_t n_light, const RoomTuning &tune = RoomTuning());
// ... of a launch of an any-hit build: zero unless the head's triple holds ALL of the scene's planes (three plane records, all
// of them the axis triple), no material is transparent and the handle's switch is not set
void fill_room_facts(const FlatScene &F, DSceneHead &H, bool switched_off);
// The two scene facts behind the dark-light skip (FlatScene::shade_finite, shade_bounded), from the records alone: with both, a
// light term whose factors fd and fs are zero is a signed zero in every channel — a zero times a FINITE product of colours; a
// product that overflowed would make it NaN.  bit 0: shade_finite, bit 1: shade_bounded.
#define CTR_SHADE_BOUND 0x1p40f  /* three factors: 2^120 < FLT_MAX */
uint32_t shade_facts(const DMat *mats, size_t n_mat, const DLight *lights, size_t n_light);
// The dark-skip fact of a launch's scene head (scene_device.h CTR_HEAD_DARK in DSceneHead::mesh_dark): set when both facts hold, no
// material transmits and the handle's switch is not set, else clear
void fill_dark_skip(const FlatScene &F, DSceneHead &H, bool switched_off);
// A switch of the environment that a handle reads when it is created (A/B runs and tests), NAME=<an integer other than 0>:
// CUTRACE_NO_SCENE_HEAD, CUTRACE_NO_SHAPE_BUILD, CUTRACE_NO_WALL_SKIP (that handle's launches carry zero room facts) and CUTRACE_NO_DARK_SKIP (... a zero dark-skip word)
bool env_switch(const char *name);

// a node whose four slots are empty: a far-away point box and a leaf of no triangles each
DNode4 empty_node4();
// slot `c` of `N` gets a box that every ray passes
inline void unbounded_box(DNode4 &N, int c) {
  for (int a = 0; a < 3; a++) { N.lo[a][c] = -3.0e38f; N.hi[a][c] = 3.0e38f; }
}

// CUTRACE_DEBUG_CREATE=1: where ctr_scene_create spends its time (stderr): the time since the previous stamp of this
// thread.  what == nullptr only restarts the clock.
void create_stamp(const char *what);

#endif
