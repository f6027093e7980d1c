"""The C-ABI library loads without a GPU and exports every symbol include/abd_hip.h declares."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "abd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(abd_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from abdpymc_amd import _native

    lib = _native.load()
    names = header_functions()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), f"{name} declared in abd_hip.h but not exported"
    # and the binding table covers exactly the header
    assert sorted(_native.SYMBOLS) == names
    assert b"gfx950" in lib.abd_version()
    assert lib.abd_last_error() is not None


def test_argument_errors_need_no_gpu():
    from abdpymc_amd import _native

    lib = _native.load()
    out = ctypes.c_void_p()
    assert lib.abd_create(None, ctypes.byref(out)) == -1
    assert b"NULL" in lib.abd_last_error()


def test_gibbs_record_layout_matches_the_header():
    """abd_gibbs_record as include/abd_hip.h declares it, field by field, against the structured dtype gibbs_sweep(log=True) returns;
    the path codes against the header's enum; the logged call refuses NULL without a GPU."""
    import numpy as np

    from abdpymc_amd import _native

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "abd_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} abd_gibbs_record;", src).group(1)
    fields = re.findall(r"(double|int16_t|uint8_t)\s+(\w+);", body)
    ctype = {"double": "<f8", "int16_t": "<i2", "uint8_t": "u1"}
    assert np.dtype([(n, ctype[t]) for t, n in fields]) == _native.GIBBS_RECORD and _native.GIBBS_RECORD.itemsize == 24
    codes = {n.lower(): int(v) for n, v in re.findall(r"ABD_GIBBS_PATH_(\w+) = (\d+)", src)}
    assert codes == _native.GIBBS_PATHS and len(set(codes.values())) == 8
    lib = _native.load()
    assert lib.abd_gibbs_sweep_log(None, 0, None, None, 0, 0, None, None, None, 0, None) == -1
    assert b"NULL" in lib.abd_last_error()


def test_missing_library_fails_loudly():
    code = "import abdpymc_amd._native as n; n.load()"
    env = dict(os.environ, ABD_HIP_LIB="/nonexistent/libabd_hip.so", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode != 0
    assert "no CPU fallback" in r.stderr or "ImportError" in r.stderr


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "abdpymc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "libabd_oracle" not in txt, f


def _build_c_example(out):
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "abi_example.c"), "-L", os.path.join(ROOT, "abdpymc_amd"), "-labd_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "abdpymc_amd"), "-lm", "-o", str(out)]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_header_is_plain_c_and_the_example_links(tmp_path):
    """include/abd_hip.h compiles as C99 (-pedantic -Werror) and examples/abi_example.c links against the library."""
    from abdpymc_amd import _native

    _native.load()  # built
    r = _build_c_example(tmp_path / "abi_example")
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_c_example_runs(tmp_path):
    r = _build_c_example(tmp_path / "abi_example")
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(tmp_path / "abi_example")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "infection found" in run.stdout
