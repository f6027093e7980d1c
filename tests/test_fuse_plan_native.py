"""How abd_logp_dlogp_many cuts a call's steps into launches (abd_fuse_plan.hpp) on the CPU: a stand-alone program built
with AddressSanitizer and UBSan.  Every step once and in order, at most 16 rows per launch, no launch across a window of
the result ring, only the call's last launch shaped for an empty chip, 17 chains never fused, the forced value 1 = one
launch per step."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuse_plan_covers_every_step_once_within_the_ring_windows(tmp_path):
    exe = tmp_path / "fuse_plan_harness"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "abdpymc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "fuse_plan_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuse plan ok" in r.stdout
