"""Dark lights (cutrace_amd/csrc/render_kernel.hip "dark lights", CTR_HEAD_DARK of the scene head; DESIGN.md "Dark lights"): in an opaque
build a lane whose light term is a signed zero in every channel — fd and fs both zero, every colour of the scene finite and
bounded, no channel of phong's `final` equal to -0 — sits the light's shadow trip out, because the cast could only decide
whether that zero is added.  Nothing a pixel can show changes, so every case renders with two handles — A created normally,
B under CUTRACE_NO_DARK_SKIP=1 (read when a handle is created: a zero word, every cast made) — and compares depth, normal and
colour BITWISE and the ray count; the frames are also held against the CPU oracle.  The scene is the flagship room at 64 x 40
(8 x 5 tiles), as in tests/test_gpu_opaque_build.py, and variants of it: the four lights moved behind the mesh (the case in
which most of the mesh's shadow casts are dark: the statistics build's count of dark (lane, light) pairs must equal the count
made here on the CPU from the oracle's hits), a negative light colour, a negative ambient factor on a black mesh (final = -0:
the guard must refuse), the mesh's phong exponent 0, 2 and 1000, colours made infinite and finite again on a live handle, and
a transparent material.

What no case here can show: that an opaque build really leaves a lane out.  On against off is bit-equal by construction — also
if the predicate never fired — and the pair count comes from the statistics build, which retires nothing.  A change that
silently disabled the skip would show in time alone (profiles/r08/dark_ab.txt: kernel cycles per dispatch against the parent
commit); which instantiation a launch took is visible through dark_skip(): 1 = the build with the code."""
import json
import os

import numpy as np
import pytest

import oracle
from tests import ray_ref, shade_ref
from tests.gpu_support import assert_same_frame, env, gpu, held  # noqa: F401  (gpu: the fixture)
from tests.live import desc_lights
from tests.ray_ref import M1, smax, vadd, vdot, vnormalized, vscale, vsub
from tests.util import ROOT, TOL, assert_parity, fast_pow_kept, light_scale, parse, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
DEFAULT = 1 | 2 | 8 | 32   # scene_device.h KV_*: the default variant; | 64: its 6-wave build
W, H = 64, 40
NT = 4
# behind the mesh as the camera at (1, 0, 2) sees it, inside the room: chosen on the CPU, where 87 % of the primary mesh hits'
# (pixel, light) pairs come out dark (the share the test below requires is 25 %)
BACK_LIGHTS = [[-0.6, 0.5, -0.7], [-0.8, -0.3, -0.2], [-0.3, 0.8, -0.8], [-0.9, 0.1, -0.6]]
MESH = 0   # the mesh's object index and its material's
FS_MARGIN = 0.01   # dark_pairs: no pair's e * log2 x may lie this close to -126


def bunny_json():
    text = json.load(open(os.path.join(ROOT, "scene", "bunny.json")))
    for o in text["objects"]:
        if o["type"] == "mesh":
            o["file"] = os.path.join(ROOT, o["file"])
    return text


def scene(ca, change=None):
    text = bunny_json()
    if change:
        change(text)
    s = parse(ca, text)
    s.set_size(W, H)
    return s


def back_lit(text):
    for l, p in zip(text["lights"], BACK_LIGHTS):
        l["point"] = p


def handles(ca, s):
    a = ca.DeviceScene(s)
    with env("CUTRACE_NO_DARK_SKIP"):
        b = ca.DeviceScene(s)
    return a, b


def compare(a, b, what, bounces, opaque=1):
    """the frame of A and of B at `bounces`: the same bits and ray count, the same build; the word set for A alone.  A's frame."""
    got, ref = held(a.render(bounces=bounces)), held(b.render(bounces=bounces))
    assert_same_frame(got, ref, f"{what}, bounces {bounces}: dark skip on / off")
    assert (a.last_kernel(), a.last_shape(), a.last_opaque()) == (b.last_kernel(), b.last_shape(), b.last_opaque()), what
    assert a.last_opaque() == opaque, (what, hex(a.last_kernel()), a.last_shape())
    assert (a.dark_skip(), b.dark_skip()) == (opaque, 0), (what, a.dark_skip(), b.dark_skip())
    return got


class Case:
    """a scene, its two handles and its oracle frames, made once per module"""

    def __init__(self, ca, change=None):
        self.s = scene(ca, change)
        self.a, self.b = handles(ca, self.s)
        self._want = {}

    def want(self, bounces, **kw):
        key = (bounces, tuple(sorted(kw.items())))
        if key not in self._want:
            self._want[key] = oracle.oracle_render(self.s, fudge=1e-3, bounces=bounces, threads=NT, **kw)
        return self._want[key]

    def close(self):
        self.a.close()
        self.b.close()


@pytest.fixture(scope="module")
def bunny(gpu):
    c = Case(gpu)
    yield c
    c.close()


@pytest.fixture(scope="module")
def backlit(gpu):
    c = Case(gpu, back_lit)
    yield c
    c.close()


def dark_pairs(s, want):
    """The predicate D for the primary hits of the oracle frame `want` (bounces 0 or more: the first cast's hits), on the CPU
    with tests/shade_ref.py's arithmetic — phong's per-light vectors and fd exactly as shade_ref.phong forms them.  fs is zero as
    the build that evaluates the predicate makes it: every such build (the opaque builds, the any-hit statistics build) takes
    the fast specular path, exp2(e * log2 x) on the transcendental pipe, whose v_exp_f32 has no denormal results: +0 for x = 0
    and wherever e * log2 x < -126, the smallest normal's exponent (e != 0; the f64 power rounded once keeps a denormal there).
    A pair within FS_MARGIN of that threshold would make the count depend on the last bits of v_log_f32 and of the half
    vector's v_rsq_f32 (e * 2^-22 is 5e-5 at the mesh's exponent 200, 1.2e-4 at the walls' 500); the scene must have none,
    which is asserted — a condition on the input.
    Returns (object index per hit pixel, (hits, lights) booleans).  The guard on `final` cannot refuse in the scenes this is
    used for — every colour and the ambient factor are >= 0, so no channel is ever -0 — and is asserted so."""
    sc = shade_ref.ShadeScene(s)
    assert sc.ambient >= 0 and not np.signbit(sc.ambient) and (sc.mat_color >= 0).all() and not np.signbit(sc.mat_color).any()
    assert all((l["color"] >= 0).all() and not np.signbit(l["color"]).any() for l in sc.lights) and (sc.mat_specular >= 0).all()
    ro, rd = ray_ref.camera_rays(sc.cam)
    hit_id = want["hit_id"].reshape(-1)
    idx = np.nonzero(hit_id >= 0)[0]
    hit = vadd(ro[idx], vscale(rd[idx], want["depth"].reshape(-1)[idx]))
    nn = vnormalized(want["normal"].reshape(-1, 3)[idx])
    in_dn = vnormalized(rd[idx])
    e = sc.mat_phong_exp[sc.obj_mat[hit_id[idx]]]
    dark = np.zeros((len(idx), len(sc.lights)), bool)
    zero = np.zeros(len(idx), f32)
    with np.errstate(all="ignore"):
        for k, l in enumerate(sc.lights):
            assert l["type"] == shade_ref.LIGHT_POINT
            nd = vnormalized(vnormalized(vsub(np.broadcast_to(l["v"], hit.shape), hit)))   # default_schema.hpp:305-308, shading.hpp:80
            fd = smax(zero, vdot(nn, nd))
            h = vnormalized(vadd(vscale(in_dn, M1), nd))
            sx = smax(zero, vdot(nn, h))
            x = e.astype(np.float64) * np.log2(sx.astype(np.float64))   # (-inf for sx = 0)
            fd_zero = (fd.view(np.uint32) & 0x7FFFFFFF) == 0
            assert (e > 0).all() and not (fd_zero & (np.abs(x + 126.0) < FS_MARGIN)).any(), "a pair at the underflow threshold of fs: move the lights"
            dark[:, k] = fd_zero & (x < -126.0)
    return hit_id[idx], dark


# ---- the flagship room ----
@pytest.mark.parametrize("bounces", [0, 1, 5])
def test_switch_on_against_off(bunny, bounces):
    got = compare(bunny.a, bunny.b, "bunny", bounces)
    assert bunny.a.last_kernel() == DEFAULT | 64 and got["ray_count"] == bunny.want(bounces)["ray_count"]


def test_default_build_against_the_oracle(bunny):
    """the launch every caller gets: depth, normal and ray count bit for bit, the colour within the parity bar"""
    got = held(bunny.a.render(bounces=5))
    assert bunny.a.last_opaque() == 1 and bunny.a.dark_skip() == 1 and bunny.a.last_kernel() == DEFAULT | 64
    want = bunny.want(5)
    assert_parity(got, want, what="bunny 64x40 b5: dark skip / oracle")
    assert got["ray_count"] == want["ray_count"]


def test_exact_pow_build_against_the_oracle_with_the_pow_rounded_once(gpu, bunny):
    """VAR_EXACT_POW has no opaque build: the parent's code, the word zero, and the oracle's frame bit for bit"""
    bunny.a.set_variant(gpu.VAR_EXACT_POW)
    try:
        got = held(bunny.a.render(bounces=5))
        assert not bunny.a.last_kernel() & 32 and bunny.a.last_opaque() == 0 and bunny.a.dark_skip() == 0, hex(bunny.a.last_kernel())
    finally:
        bunny.a.set_variant(gpu.VAR_AUTO)
    assert_same_frame(got, bunny.want(5, pow_rounded_once=True), "bunny b5, exact pow / oracle with the pow rounded once")


# ---- the lights behind the mesh: the case that exercises the skip ----
def test_back_lit_most_mesh_pairs_are_dark_and_the_kernel_counts_the_same(gpu, backlit):
    want = backlit.want(0)
    obj, dark = dark_pairs(backlit.s, want)
    share = dark[obj == MESH].mean()
    print(f"back-lit: {int((obj == MESH).sum())} mesh pixels, dark share of their pairs {share:.3f}, dark pairs of all hits {int(dark.sum())}")
    assert (obj == MESH).sum() > 400 and share >= 0.25, share   # a condition on the input: the reference alone meets it
    # the statistics build evaluates the kernel's predicate for every shaded hit and retires nothing; at bounces 0 the shaded
    # hits are the primary hits
    ds = gpu.DeviceScene(backlit.s)
    try:
        ds.set_variant(gpu.VAR_STATS)
        gpu.DeviceScene.lane_stats(reset=True)
        got = held(ds.render(bounces=0))
        counted = gpu.DeviceScene.lane_stats(reset=True)["dark_lights"]
        assert ds.dark_skip() == 1 and ds.last_opaque() == 0 and ds.last_kernel() & 32, hex(ds.last_kernel())
    finally:
        ds.close()
    print("back-lit, statistics build:", counted)
    assert counted["lane_light_pairs"] == int(dark.sum()), (counted, int(dark.sum()))
    assert counted["shadow_trips_all_dark"] > 0 and counted["mesh_entries_with_a_dark_lane"] > 0, counted
    assert_parity(got, want, what="back-lit b0, statistics build / oracle")
    assert got["ray_count"] == want["ray_count"]


@pytest.mark.parametrize("bounces", [0, 5])
def test_back_lit_switch_on_against_off_and_the_oracle(backlit, bounces):
    got = compare(backlit.a, backlit.b, "back-lit", bounces)
    want = backlit.want(bounces)
    assert_parity(got, want, what=f"back-lit b{bounces}: dark skip / oracle")
    assert got["ray_count"] == want["ray_count"]


# ---- further scenes ----
def run_case(ca, change, what, bounces=(0, 1, 5)):
    """on against off and against the oracle; an opaque build with the word set wherever the fast specular path is kept"""
    c = Case(ca, change)
    try:
        opaque = 1 if fast_pow_kept(c.s) else 0   # (outside the fast path's domain the launch is VAR_EXACT_POW's: no opaque build)
        tol = TOL * max(1.0, light_scale(c.s))
        frames = {}
        for b in bounces:
            got = compare(c.a, c.b, what, b, opaque=opaque)
            want = c.want(b)
            assert_parity(got, want, what=f"{what} b{b}: dark skip / oracle", color_tol=tol)
            assert got["ray_count"] == want["ray_count"], what
            frames[b] = (got, want)
        return frames, opaque
    finally:
        c.close()


def test_a_negative_light_colour(gpu):
    def change(text):
        back_lit(text)
        text["lights"][1]["color"] = [0.5, -0.7, 0.2]
    _, opaque = run_case(gpu, change, "light colour (0.5, -0.7, 0.2)")
    assert opaque == 1


def test_negative_ambient_on_a_black_mesh_the_guard_refuses(gpu):
    """final = 0 * -0.25 = -0 in every channel of a mesh hit, and every light's term is +0 (the colours are zero): the reference
    ends with +0 where some light is unoccluded and -0 where none is.  A lane skipped in spite of the guard would keep -0."""
    def change(text):
        back_lit(text)
        text["camera"]["ambient"] = -0.25
        text["materials"][MESH]["color"] = [0.0, 0.0, 0.0]
    frames, opaque = run_case(gpu, change, "ambient -0.25, black mesh", bounces=(0, 1))
    assert opaque == 1
    got, want = frames[0]
    mesh = want["hit_id"] == MESH
    assert mesh.sum() > 400 and (got["color"][mesh] == 0).all()
    assert same_bits(got["color"][mesh], want["color"][mesh]), "the zeros' signs on the mesh"
    assert np.signbit(want["color"][mesh]).any() and not np.signbit(want["color"][mesh]).all(), "both signs occur"


@pytest.mark.parametrize("phong", [0, 2, 1000])
def test_phong_exponents_on_the_mesh(gpu, phong):
    """0: fs = 1, no lane is dark; 2: fs is zero only where nn.h is; 1000: fs underflows almost everywhere"""
    def change(text):
        back_lit(text)
        text["materials"][MESH]["phong"] = phong
    run_case(gpu, change, f"phong {phong}", bounces=(0, 5))


# ---- live edits ----
def test_colours_made_infinite_and_finite_again_on_a_live_handle(gpu):
    """a material's `specular`, then a light's colour, set to inf and back: head word and frame are a fresh handle's each time"""
    inf = float("inf")
    base = scene(gpu, back_lit)   # (kept: desc_lights returns views of its records)
    ds = gpu.DeviceScene(base)
    seen = []
    try:
        def step(what, edit_live, edit_host):
            edit_live()
            got = held(ds.render(bounces=3))
            fresh_scene = scene(gpu, back_lit)
            edit_host(fresh_scene)
            fresh = gpu.DeviceScene(fresh_scene)
            try:
                assert_same_frame(got, held(fresh.render(bounces=3)), f"{what}: edited / fresh handle")
                assert (ds.last_kernel(), ds.last_opaque(), ds.dark_skip()) == (fresh.last_kernel(), fresh.last_opaque(), fresh.dark_skip()), what
            finally:
                fresh.close()
            seen.append(ds.dark_skip())

        def lights_with(colour):
            ls = [gpu.Light.from_buffer_copy(l) for l in desc_lights(base)]
            ls[2].color = gpu.Vec3(*colour)
            return ls

        def host_light(hs, colour):   # (the description's own record: the scene text has no way to write inf)
            hs.desc.contents.lights[2].color = gpu.Vec3(*colour)

        step("as created", lambda: None, lambda hs: None)
        step("specular inf", lambda: ds.set_material(MESH, specular=inf), lambda hs: hs.set_material(MESH, specular=inf))
        step("specular back", lambda: ds.set_material(MESH, specular=0.3), lambda hs: None)
        step("light colour inf", lambda: ds.set_lights(lights_with((0.3, inf, 0.3))), lambda hs: host_light(hs, (0.3, inf, 0.3)))
        step("light colour back", lambda: ds.set_lights(lights_with((0.3, 0.3, 0.3))), lambda hs: None)
    finally:
        ds.close()
    assert seen == [1, 0, 1, 0, 1], seen


# ---- a scene the skip is not for ----
def test_a_transparent_material_runs_the_parents_code(gpu):
    def change(text):
        back_lit(text)
        text["materials"][1]["transparency"] = 0.25
    c = Case(gpu, change)
    try:
        got = compare(c.a, c.b, "a transparent wall material", 3, opaque=0)
        assert not c.a.last_kernel() & 2, hex(c.a.last_kernel())
        want = c.want(3)
        assert_parity(got, want, what="transparent wall b3 / oracle")
        assert got["ray_count"] == want["ray_count"]
    finally:
        c.close()
