// guard.h — the guard of the BVH culling: which triangles every lane that enters a mesh must meet whatever their box,
// and which meshes are walked linearly.  Host only, no HIP (the scan of the planes may have run on the device: guard_scan.h): a plan is a pure function of the flattened scene and the
// cameras, and applying it edits the host copy and names the records the device has to receive.
//
// The per-mesh BVH lets a cast skip triangles whose (widened) box its ray cannot touch.  That is the
// reference's result except in ONE regime: a ray that lies IN the plane of a triangle to within rounding
// has alpha = det[a b c] (default_schema.hpp:59) and all three numerators at noise level, and the
// reference's float test may then accept the triangle for a ray that passes far from it — a hit the
// culling would drop (tests/test_gpu_parity.py::test_rays_coplanar_with_triangles).  Such a ray has its
// ORIGIN in the triangle's plane and its direction parallel to it, both to ~1e-6 relative (a direction
// that leaves the plane by more makes t0 = noise/alpha < min_t): for primary rays the eye must lie in
// the plane, for shadow rays the light must (or a sun must be parallel to it).  So at upload, and
// whenever the cameras change, every triangle plane of every mesh is checked against the eyes, the point
// lights and the sun directions (tolerance 2^-17, an order of magnitude above the rounding that matters), and the
// triangles that qualify are copied into the mesh's GUARD records, which the walk tests for every lane
// that passes the mesh's own AABB test, whatever their box (a duplicate test cannot change the
// lexicographic minimum of (t, file index)).  More than CTR_GUARD_SLOTS of them: every node of the mesh
// gets unbounded boxes instead — the reference's linear walk through the same code.
// Secondary rays (round 3; tests/test_gpu_parity.py::test_secondary_rays_coplanar_with_triangles showed the hole is real:
// one pixel of a purpose-built scene differed).  A ray reflected by a PLANAR mirror lies on the line through the
// mirror image of its parent's origin, so the rays a flat mirror makes of the primary rays all pass through the
// mirror image of the eye — a VIRTUAL eye — and fall into a triangle's plane only if that point lies in it.  The
// same check therefore runs for the virtual eyes too: every eye mirrored in every reflective plane, stand-alone
// triangle and triangle of a small mesh (<= CTR_MIRROR_MESH_TRIS: mirrors built from a few triangles, like
// scene/mirror.stl), and those images mirrored once more (reflections of reflections) while the list stays short.
// Pass-through rays continue their parent's line and need no entry; shadow rays run from a surface to a light, whose
// position is checked already; a sphere keeps a pencil of rays planar only in a plane through its centre and the
// pencil's apex, which the apex's own entry covers.  NOT covered: chains of more than two reflections, mirrors that
// are large meshes, and single rays (not families) that meet a triangle's plane by numerical coincidence — per (ray,
// triangle) pair a ~1e-9 event that no full-size comparison or fuzz run has shown yet.
#ifndef CUTRACE_AMD_GUARD_H
#define CUTRACE_AMD_GUARD_H

#include "guard_scan.h"
#include "scene_flatten.h"

#define CTR_MIRROR_MESH_TRIS 16u
#define CTR_SECOND_ORDER_MAX_EYES 8u
#define CTR_VIRTUAL_EYES_MAX 4096u  // (round 3: 96 — a 90-camera path through a room of five reflecting walls got images for its first 16 cameras only)

struct GuardPlan {
  struct Mesh {
    std::vector<uint32_t> risky;  // triangles (leaf order) that go into the mesh's guard records; none for a linear mesh
    bool linear = false;          // more than CTR_GUARD_SLOTS of them: the mesh's nodes get unbounded boxes
  };
  std::vector<Mesh> meshes;             // one per FlatScene::guards entry (an empty mesh: nothing)
  std::vector<uint32_t> merged_keys;    // merged tree: the keys (mesh rank << 24 | file index) of every mesh's risky triangles
  bool any_linear = false;
  bool merged_usable() const { return !any_linear && merged_keys.size() <= CTR_GUARD_SLOTS; }
  size_t n_origins = 0, n_mirrors = 0;  // eyes + mirror images, flat mirrors (CUTRACE_DEBUG_GUARDS)
};

// What the planes are checked against (guard_scan.h), built once per plan: the eyes, their images in the scene's flat mirrors,
// then the point lights, then the suns (each kind in the scene's order).
struct GuardProbes {
  std::vector<GuardProbe> probes;
  size_t n_points = 0;  // probes[0 .. n_points) are points, the rest suns
  size_t n_origins = 0, n_mirrors = 0;
};
GuardProbes guard_probes(const FlatScene &F, const std::vector<DCam> &cams);
// the planes of all meshes, FlatScene::guards order: the length of the flat array the device scan runs over
uint64_t guard_plane_count(const FlatScene &F);

// `words`: the bits of a scan of that flat array against P.probes (guard_scan.h; the device's, read back), cut here at each
// mesh's range; nullptr: the planes are scanned here, on the host.  The same plan either way.
GuardPlan plan_guards(const FlatScene &F, const GuardProbes &P, const uint64_t *words);
// guard_probes, then the host scan
GuardPlan plan_guards(const FlatScene &F, const std::vector<DCam> &cams);

// Makes the host copy what the plan asks for, touching only what differs from the guard state the scene already has
// (MeshGuard::guarded / linear, Merged::guarded): the same cameras again give no dirty range.
std::vector<DirtyRange> apply_guards(FlatScene &F, const GuardPlan &plan);

#endif
