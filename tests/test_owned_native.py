"""The owning handles of the host layer (abd_owned.hpp: DevBuf, MappedBuf, Stream, Event) on the CPU: a stand-alone program
built with AddressSanitizer and UBSan against malloc-backed HIP calls that count what is alive (tests/native/fake_hip)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handles_own_release_and_survive_failed_builds(tmp_path):
    exe = tmp_path / "owned_harness"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-Wno-self-move",
                           "-I", os.path.join(ROOT, "tests", "native", "fake_hip"), "-I", os.path.join(ROOT, "abdpymc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "owned_harness.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "owned ok" in r.stdout
