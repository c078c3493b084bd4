"""MetricDirect's index lists and pose batches at the boundaries: the C99 program tests/c/test_direct_lists_abi.c and the adapter
program tests/cpp/test_direct_lists.cpp, built the way tests/test_c_abi.py and tests/test_cpp_adapter.py build theirs.  Without a
GPU: the header is C99, the symbols are there, a null metric is an argument error with nothing written, the Eigen branch of the
adapter's overload is well formed, the build lists the new sources, and the new kernels' resources as built.  On the GPU: the sums
the two programs print have the bits of the Python calls on the same data."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")


def _build_c(tmp):
    from epipolarconsistency_amd import _lib
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = os.path.join(tmp, "test_direct_lists_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_direct_lists_abi.c"), "-o", exe, "-L" + libdir, "-lecc_hip", "-lm",
           "-Wl,-rpath," + libdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _build_cpp(tmp):
    exe = os.path.join(tmp, "test_direct_lists")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_direct_lists.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_header_is_c99_and_a_null_metric_is_refused(tmp_path):
    r = subprocess.run([_build_c(str(tmp_path)), "nodevice"], capture_output=True, text=True)
    assert r.returncode == 0 and "nodevice ok" in r.stdout, r.stdout + r.stderr


def test_adapter_program_compiles_and_links(tmp_path):
    assert subprocess.run([_build_cpp(str(tmp_path))]).returncode == 2  # usage: touches no device


def test_eigen_branch_of_the_list_overload_is_well_formed():
    """As tests/test_cpp_adapter.py checks the Radon metric's: tests/cpp/mock_eigen is NOT Eigen; it lets a compiler see the branch."""
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_direct_lists_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_python_layer_binds_the_calls():
    from epipolarconsistency_amd import _lib
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    lib = _lib.lib()
    assert lib.ecc_direct_evaluate_pairs.argtypes == [vp, vp, i64, vp, i, vp, vp]
    assert lib.ecc_direct_evaluate_pose_deltas.argtypes == [vp, i, vp, vp, vp, vp, vp, vp]
    assert lib.ecc_direct_pose_pairs_bound.argtypes == [vp, i, vp, C.POINTER(i64)]
    assert lib.ecc_debug_set_direct_batch.argtypes == [vp, i64]
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    for name in ("ecc_direct_evaluate_pairs", "ecc_direct_evaluate_pose_deltas", "ecc_direct_pose_pairs_bound", "ecc_debug_set_direct_batch"):
        assert "int %s(" % name in text and getattr(lib, name).restype is C.c_int


def test_source_list_and_flags():
    from epipolarconsistency_amd import build
    for s in ("direct_list_kernel.hip", "ecc_direct_lists.hip"):
        assert s in build.SOURCES and os.path.exists(os.path.join(PKG, "csrc", s)), s
    assert build.PER_SOURCE_FLAGS["direct_list_kernel.hip"] == build.PER_SOURCE_FLAGS["direct_kernel.hip"]  # the same walker
    for h in ("ecc_direct_lines.h", "ecc_direct_internal.h", "ecc_direct_lists_host.h"):
        assert h in build.HEADERS, h


def test_list_kernel_resources():
    """The list forms of the line-integral kernels are direct_kernel.hip's with another index source (the pieces:
    csrc/ecc_direct_lines.h): no more registers, LDS or scratch than those, as built -- whatever those are (the slab kernel has 36
    bytes of scratch in the parent's build already; the list form 28).  The slab form keeps amdgpu_waves_per_eu(4, 4): at most 128
    vector registers.  The segment sum: a 1024-thread workgroup, 128 bytes of LDS, no scratch."""
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ks = mod.kernels(os.path.join(PKG, "libecc_hip.so"))

    def one(part):
        found = mod.find(ks, part)
        assert len(found) == 1, (part, sorted(found))
        name, k = list(found.items())[0]
        print(name, {f: k[f] for f in (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")})
        return k

    for new, old in (("24direct_list_lines_kernel", "19direct_lines_kernel"), ("31direct_list_lines_gather_kernel", "26direct_lines_gather_kernel")):
        a, b = one(new), one(old)
        assert a[".vgpr_count"] <= 128 and a[".vgpr_count"] <= b[".vgpr_count"] + 8, (new, a[".vgpr_count"], b[".vgpr_count"])
        assert a[".group_segment_fixed_size"] == b[".group_segment_fixed_size"], new
        assert a[".private_segment_fixed_size"] <= b[".private_segment_fixed_size"], (new, a[".private_segment_fixed_size"])
    assert one("23direct_list_pair_kernel")[".private_segment_fixed_size"] == 0
    s = one("25direct_segment_sum_kernel")
    assert s[".max_flat_workgroup_size"] == 1024 and s[".group_segment_fixed_size"] == 128 and s[".private_segment_fixed_size"] == 0


# ---- on the GPU: the programs' sums are the Python calls' bits ---------------------------------------------------------------------
def _data_file(tmp_path, s):
    from epipolarconsistency_amd import pack_projection_matrices
    path = os.path.join(str(tmp_path), "scan.bin")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(pack_projection_matrices(s["Ps"]), np.float64).tobytes())
        f.write(np.ascontiguousarray(s["imgs"], np.float32).tobytes())
    return [path, str(len(s["Ps"])), str(s["n_u"]), str(s["n_v"])]


def _python_results(gpu_ctx, s):
    import epipolarconsistency_amd as E
    n, Ps = len(s["Ps"]), list(s["Ps"])
    candidate = 0.5 * (Ps[3] + Ps[4])  # (the programs make the same one)
    m = E.MetricDirect(gpu_ctx, Ps + [candidate], np.ascontiguousarray(s["imgs"], np.float32))
    idx = [[(i, row, i, 3) if i < 3 else (row, i, 3, i) for i in range(n) if i != 3] for row in (3, n)]
    sums, values = m.evaluate_pairs(idx[0] + idx[1], segments=[0, n - 1, 2 * (n - 1)], want_pairs=True)
    pose_sums, _, tuples = m.evaluate_pose_deltas([[3], [1, 3]], [[candidate], [Ps[3], Ps[1]]], want_pairs=True)
    out = dict(sums=sums, whole=m.evaluate_pairs(idx[0] + idx[1]), values=values, pose_sums=pose_sums, tuples=tuples, evaluate=m.evaluate())
    m.close()
    return out


def _hex(x):
    return float.fromhex(x)


def _lines(stdout):
    return {l.split()[0]: l.split()[1:] for l in stdout.strip().splitlines()}


@pytest.mark.gpu
def test_c_program_has_the_python_calls_bits(gpu_ctx, small_scan, tmp_path):
    want = _python_results(gpu_ctx, small_scan)
    r = subprocess.run([_build_c(str(tmp_path))] + _data_file(tmp_path, small_scan), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    got = _lines(r.stdout)
    assert [_hex(x) for x in got["segment_sums"]] == list(want["sums"])
    assert _hex(got["whole"][0]) == want["whole"]
    assert _hex(got["first_value"][0]) == want["values"][0] and _hex(got["last_value"][0]) == want["values"][-1]
    assert [_hex(x) for x in got["pose_sums"]] == list(want["pose_sums"])
    assert int(got["pose_pairs"][0]) == len(want["tuples"]) and [int(x) for x in got["last_tuple"]] == list(want["tuples"][-1])
    assert _hex(got["evaluate"][0]) == want["evaluate"]


@pytest.mark.gpu
def test_adapter_program_has_the_python_calls_bits(gpu_ctx, small_scan, tmp_path):
    want = _python_results(gpu_ctx, small_scan)
    r = subprocess.run([_build_cpp(str(tmp_path))] + _data_file(tmp_path, small_scan), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    got = _lines(r.stdout)
    assert _hex(got["list_sum"][0]) == want["sums"][1]
    assert _hex(got["first_value"][0]) == want["values"][len(small_scan["Ps"]) - 1]
    assert [_hex(x) for x in got["pose_sums"]] == list(want["pose_sums"])
    assert _hex(got["evaluate"][0]) == want["evaluate"]
