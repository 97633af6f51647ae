"""What ctr_cast_rays, ctr_shade_rays and ctr_shade_points check before they look at the scene (csrc/ctr_rays.cpp): called with a
null scene handle, so no GPU.  Every case: status CTR_E_INVALID and the whole text of ctr_last_error().  The texts were
recorded from the library before the three preambles became one; which error wins when several apply is part of them."""
import ctypes as C

import pytest

from cutrace_amd import _lib

SOME = C.addressof(C.create_string_buffer(64))  # a non-null address: nothing is read through it before the scene is looked at

RAY_SHADOW_ONLY = "ctr_cast_rays: CTR_RAY_SHADOW writes d_shadow only, and needs it"
RAY_NEAREST = "ctr_cast_rays: a nearest-hit query needs at least one of its outputs and no d_shadow"
POINTS_PAIR = "ctr_shade_points: d_color needs d_normal and d_view"

# (entry point, fields of an otherwise valid query or None for a null query, ctr_last_error())
CASES = [
    ("ctr_cast_rays", None, "ctr_cast_rays: null query"),
    ("ctr_cast_rays", dict(flags=8), "ctr_cast_rays: unknown flag bits 8"),
    ("ctr_cast_rays", dict(flags=0xFFFFFFF0 | 2), "ctr_cast_rays: unknown flag bits 4294967280"),
    ("ctr_cast_rays", dict(flags=16, d_t=None), "ctr_cast_rays: unknown flag bits 16"),  # before the output rules
    ("ctr_cast_rays", dict(flags=4 | 1, d_t=None, d_shadow=SOME),
     "ctr_cast_rays: CTR_RAY_SHADOW and CTR_RAY_IGNORE_TRANSPARENT exclude each other"),
    ("ctr_cast_rays", dict(flags=4 | 1), "ctr_cast_rays: CTR_RAY_SHADOW and CTR_RAY_IGNORE_TRANSPARENT exclude each other"),
    ("ctr_cast_rays", dict(flags=4, d_shadow=SOME), RAY_SHADOW_ONLY),               # d_t is set too
    ("ctr_cast_rays", dict(flags=4 | 2, d_t=None, d_uv=SOME, d_shadow=SOME), RAY_SHADOW_ONLY),
    ("ctr_cast_rays", dict(flags=4, d_t=None), RAY_SHADOW_ONLY),                    # no d_shadow
    ("ctr_cast_rays", dict(d_t=None), RAY_NEAREST),                                 # no output at all
    ("ctr_cast_rays", dict(d_shadow=SOME), RAY_NEAREST),
    ("ctr_cast_rays", dict(flags=2, d_t=None, d_prim=SOME, d_shadow=SOME), RAY_NEAREST),
    ("ctr_cast_rays", dict(), "ctr_cast_rays: null scene"),
    ("ctr_cast_rays", dict(flags=4, d_t=None, d_shadow=SOME), "ctr_cast_rays: null scene"),
    ("ctr_cast_rays", dict(n_rays=1 << 31, d_origin=None), "ctr_cast_rays: null scene"),   # before the count and the rays
    ("ctr_shade_rays", None, "ctr_shade_rays: null query"),
    ("ctr_shade_rays", dict(flags=4), "ctr_shade_rays: unknown flag bits 4"),
    ("ctr_shade_rays", dict(flags=7, bounces=-1, d_color=None), "ctr_shade_rays: unknown flag bits 4"),
    ("ctr_shade_rays", dict(bounces=-1), "ctr_shade_rays: bounces -1 outside [0, 15]"),
    ("ctr_shade_rays", dict(bounces=16), "ctr_shade_rays: bounces 16 outside [0, 15]"),
    ("ctr_shade_rays", dict(bounces=16, d_color=None), "ctr_shade_rays: bounces 16 outside [0, 15]"),
    ("ctr_shade_rays", dict(d_color=None), "ctr_shade_rays: d_color is required"),
    ("ctr_shade_rays", dict(bounces=15, flags=3), "ctr_shade_rays: null scene"),
    ("ctr_shade_rays", dict(bounces=0, n_rays=1 << 31, d_dir=None), "ctr_shade_rays: null scene"),
    ("ctr_shade_points", None, "ctr_shade_points: null query"),
    ("ctr_shade_points", dict(flags=4), "ctr_shade_points: unknown flag bits 4"),
    ("ctr_shade_points", dict(flags=12, d_color=None, d_light_shadow=None), "ctr_shade_points: unknown flag bits 12"),
    ("ctr_shade_points", dict(d_color=None, d_light_shadow=None),
     "ctr_shade_points: no output: one of d_color and d_light_shadow is required"),
    ("ctr_shade_points", dict(d_normal=None), POINTS_PAIR),
    ("ctr_shade_points", dict(d_view=None), POINTS_PAIR),
    ("ctr_shade_points", dict(d_normal=None, d_view=None, d_light_shadow=None), POINTS_PAIR),
    ("ctr_shade_points", dict(d_normal=None, d_material=SOME, d_object=SOME), POINTS_PAIR),  # before the index arrays
    ("ctr_shade_points", dict(d_material=SOME, d_object=SOME), "ctr_shade_points: d_material and d_object exclude each other"),
    ("ctr_shade_points", dict(d_color=None, d_material=SOME, d_object=SOME),
     "ctr_shade_points: d_material and d_object exclude each other"),
    ("ctr_shade_points", dict(), "ctr_shade_points: null scene"),
    ("ctr_shade_points", dict(flags=3, material=-1, n_points=1 << 31, d_point=None), "ctr_shade_points: null scene"),
]


def valid_query(entry):
    """a query its entry point refuses for the null scene alone"""
    if entry == "ctr_cast_rays":
        return _lib.RayQuery(n_rays=2, min_t=1e-3, d_origin=SOME, d_dir=SOME, d_t=SOME)
    if entry == "ctr_shade_rays":
        return _lib.ShadeQuery(n_rays=2, bounces=5, min_t=1e-3, d_origin=SOME, d_dir=SOME, d_color=SOME)
    return _lib.PointQuery(n_points=2, d_point=SOME, d_normal=SOME, d_view=SOME, d_color=SOME, d_light_shadow=SOME)


@pytest.mark.parametrize("entry", ["ctr_cast_rays", "ctr_shade_rays", "ctr_shade_points"])
def test_checks_before_the_scene(entry):
    L = _lib.hip_lib()
    cases = [c for c in CASES if c[0] == entry]
    assert len(cases) >= 6
    for _, fields, text in cases:
        q = None
        if fields is not None:
            q = valid_query(entry)
            for k, v in fields.items():
                setattr(q, k, v)
        st = getattr(L, entry)(None, C.byref(q) if q is not None else None, None)
        assert (st, L.ctr_last_error().decode()) == (1, text), (fields, text)
