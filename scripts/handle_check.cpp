// handle_check.cpp — what the scene handle's memory does when an allocation fails, as a program of its own (meant for ASan/UBSan;
// the record of a run: profiles/handle_arrays/sanitizers.txt).  It is meant for a machine WITHOUT a device, where every allocation
// of the runtime fails: GrowBuf and SceneBuf (ctr_internal.h) must then report a CTR_E_HIP_BASE + ... status and keep pointer and
// capacity, from empty and from a state set by hand; empty members are destroyed without a call that could fail; and
// ctr_scene_create of a valid description returns CTR_E_NO_DEVICE and no handle.  With a device present the allocations succeed,
// which this program says and does not check further.  Linked with ctr_scene.cpp and what that needs (guard_scan.hip's host
// half, scene_flatten.cpp, guard.cpp, bvh.cpp).  tests/test_handle_cpu.py builds and runs it.
//
//   handle_check        prints "handle_check: ok" and returns 0, or says what differed and returns 1
#include <cstdio>
#include <cstring>

#include "ctr_internal.h"

static int failures = 0;
static void expect(bool ok, const char *what) {
  if (!ok) { fprintf(stderr, "handle_check: %s\n", what); failures++; }
}
static bool hip_status(int st) { return st > CTR_E_HIP_BASE; }

// reserve and the keeping grow on `b`, which holds (p, cap): both fail, both leave it as it is
static void fails_and_keeps(GrowBuf &b, const char *what) {
  void *const p = b.p;
  const size_t cap = b.cap;
  expect(b.reserve(cap) == CTR_OK && b.grow(cap, cap) == CTR_OK && b.p == p && b.cap == cap, "what fits is no allocation");
  expect(hip_status(b.reserve(cap + 1)) && b.p == p && b.cap == cap, what);
  expect(strstr(ctr_last_error(), "hip") != nullptr, "the message names the runtime's error");
  expect(hip_status(b.grow(cap + 100, 0)) && b.p == p && b.cap == cap, what);
  expect(hip_status(b.grow(2 * cap + 3, cap)) && b.p == p && b.cap == cap, what);
  expect(hip_status(b.grow(cap + 1, cap + 7)) && b.p == p && b.cap == cap, what);  // (more to keep than there is)
}

int main() {
  if (ctr_device_count() > 0) {
    printf("handle_check: a device is present, allocations do not fail here: nothing checked\nhandle_check: ok\n");
    return 0;
  }
  // ---- from empty: device memory, page-locked memory, a scene array ----
  {
    GrowBuf dev(8), pinned(4, true);
    SceneBuf scene(16);
    expect(scene.tail == 256 && dev.tail == 0 && pinned.tail == 0 && scene.elem == 16 && !scene.pinned, "a scene array has 256 bytes behind its end");
    fails_and_keeps(dev, "device memory, empty");
    fails_and_keeps(pinned, "page-locked memory, empty");
    fails_and_keeps(scene, "scene array, empty");
    expect(!dev.p && !pinned.p && !scene.p && dev.as<float>() == nullptr, "empty stays empty");
  }  // (destroyed empty: nothing to release)
  // ---- from a state set by hand: the block is never touched, freed or replaced ----
  {
    static unsigned char block[64 + 256];
    GrowBuf dev(8), pinned(4, true);
    SceneBuf scene(16), other(16);
    for (GrowBuf *b : {&dev, &pinned, (GrowBuf *)&scene}) { b->p = block; b->cap = 4; }
    fails_and_keeps(dev, "device memory, 4 records");
    fails_and_keeps(pinned, "page-locked memory, 4 records");
    fails_and_keeps(scene, "scene array, 4 records");
    scene.swap(other);
    expect(!scene.p && scene.cap == 0 && other.p == block && other.cap == 4, "swap");
    for (GrowBuf *b : {&dev, &pinned, (GrowBuf *)&scene, (GrowBuf *)&other}) { b->p = nullptr; b->cap = 0; }  // (not the runtime's: not for release())
  }
  {
    GrowBuf b(4);
    b.release();
    b.release();
    expect(!b.p && b.cap == 0, "release of an empty member");
  }
  // ---- ctr_scene_create of a valid two-object description ----
  ctr_material mat{};
  mat.type = CTR_MAT_PHONG;
  mat.color = ctr_vec3{0.5f, 0.5f, 0.5f};
  ctr_light light{};
  light.type = CTR_LIGHT_POINT;
  light.v = ctr_vec3{1.f, 2.f, -3.f};
  light.color = ctr_vec3{1.f, 1.f, 1.f};
  ctr_object objects[2] = {};
  objects[0].type = CTR_OBJ_SPHERE;
  objects[0].v0 = ctr_vec3{0.f, 0.f, 3.f};
  objects[0].f0 = 1.f;
  objects[1].type = CTR_OBJ_PLANE;
  objects[1].v0 = ctr_vec3{0.f, -1.f, 0.f};
  objects[1].v1 = ctr_vec3{0.f, 1.f, 0.f};
  ctr_scene_desc d{};
  d.objects = objects; d.n_objects = 2;
  d.lights = &light; d.n_lights = 1;
  d.materials = &mat; d.n_materials = 1;
  d.cam.forward = ctr_vec3{0.f, 0.f, 1.f};
  d.cam.up = ctr_vec3{0.f, 1.f, 0.f};
  d.cam.right = ctr_vec3{1.f, 0.f, 0.f};
  d.cam.w = d.cam.h = 16;
  std::string err;
  expect(validate_desc(d, err) == CTR_OK, "the description is valid");
  ctr_scene *out = reinterpret_cast<ctr_scene *>(&d);  // (anything but null)
  const int st = ctr_scene_create(&d, 0, &out);
  expect(st == CTR_E_NO_DEVICE && out == nullptr, "ctr_scene_create: CTR_E_NO_DEVICE and no handle");
  ctr_scene_destroy(nullptr);

  if (!failures) printf("handle_check: ok\n");
  return failures ? 1 : 0;
}
