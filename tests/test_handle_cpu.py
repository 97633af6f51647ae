"""What the scene handle's memory does when an allocation fails (CPU, no GPU): the owning type of cutrace_amd/csrc/ctr_internal.h
(GrowBuf, SceneBuf) keeps pointer and capacity and reports the runtime's error, empty members are destroyed without harm, and
ctr_scene_create of a valid description returns CTR_E_NO_DEVICE and no handle — run through scripts/handle_check.cpp, which
states what it checks.  Where a device is present the allocations succeed, and the program says so instead."""
import os
import subprocess

from cutrace_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cutrace_amd", "csrc")


def test_failed_allocations_leave_the_handle_as_it_was(tmp_path):
    exe = str(tmp_path / "handle_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-pthread", "-Wno-unused-function",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "scripts", "handle_check.cpp"),
                           *(os.path.join(CSRC, f) for f in ("ctr_scene.cpp", "guard_scan.hip", "scene_flatten.cpp", "guard.cpp", "bvh.cpp"))],
                          stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "handle_check: ok", out.stdout[-2000:] + out.stderr[-4000:]
    assert "handle_check:" not in out.stderr, out.stderr[-4000:]
