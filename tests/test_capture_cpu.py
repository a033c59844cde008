"""CPU: the host-side rules of graph capture (include/pm.h, "Graph capture of the estimator calls") without a device.
tests/capture_host_main.cpp compiles csrc/pm_capi.cpp as it is against a stand-in HIP runtime that counts calls and can
claim that the stream is capturing: a call that would have to allocate is refused before any runtime call, a block carved
under capture is retired (and freed by pm_ctx_destroy) where every other block is freed at once, the sizes without a
capture are what they always were, and timing records no event on a capturing stream.  tests/test_capture_gpu.py checks
the same rules, and the replays themselves, on the device."""
import os
import subprocess

from points_matching_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "points_matching_amd", "csrc")


def build_and_run(out_dir, capi=os.path.join(CSRC, "pm_capi.cpp")):
    """Compile the stand-alone program around the given pm_capi.cpp and run it: (exit status, output)."""
    exe = os.path.join(str(out_dir), "capture_host")
    cmd = ["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-Wno-unused-result", "-Wno-deprecated-declarations",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "capture_host_main.cpp"), capi, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def test_capture_rules_on_the_host(tmp_path):
    rc, out = build_and_run(tmp_path)
    assert rc == 0 and out.strip().endswith("ALL OK"), out
    assert out.count("\nok ") + out.startswith("ok ") == 6, out


def test_scratch_query_is_declared_and_wrapped():
    assert "pm_ctx_scratch_info" in api.EXPORTS and hasattr(api.lib(), "pm_ctx_scratch_info")
    assert callable(api.Context.scratch_info)
