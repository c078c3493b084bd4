"""ecc_metric_evaluate_gradient / ecc_metric_last_gradient_path (csrc/ecc_gradient.hip, csrc/small_poses_kernel.hip) without a
GPU: the symbols and their argument errors, the prototypes from C99, the C++ adapter's evaluateGradient in both branches, and the
resources of the new kernel as DESIGN.md 4.11 plans them -- read from the built library's code object."""
import ctypes as C
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_the_gradient_entry_points():
    L = _cdll()
    for name in ("ecc_metric_evaluate_gradient", "ecc_metric_last_gradient_path", "ecc_debug_set_gradient_launch"):
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    buf = (C.c_double * 12)()
    path = C.c_int(-1)
    vp = C.c_void_p
    L.ecc_metric_evaluate_gradient.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    rc = L.ecc_metric_evaluate_gradient(None, 0, 1, C.addressof(buf), C.addressof(buf), C.addressof(buf), None, C.addressof(buf), None)
    assert rc == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
    L.ecc_metric_last_gradient_path.argtypes = [vp, C.POINTER(C.c_int)]
    assert L.ecc_metric_last_gradient_path(None, C.byref(path)) == ECC_ERR_INVALID_ARGUMENT and path.value == -1
    assert len(L.ecc_last_error()) > 0


def test_error_code_matches_the_header():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert "ECC_ERR_INVALID_ARGUMENT = %d" % ECC_ERR_INVALID_ARGUMENT in text or \
        "#define ECC_ERR_INVALID_ARGUMENT %d" % ECC_ERR_INVALID_ARGUMENT in text


def test_python_layer_binds_the_calls():
    from epipolarconsistency_amd import _lib, api
    for name in ("ecc_metric_evaluate_gradient", "ecc_metric_last_gradient_path", "ecc_debug_set_gradient_launch"):
        assert getattr(_lib.lib(), name).argtypes is not None, name
    for name in ("evaluate_gradient", "evaluate_gradient_rigid", "last_gradient_path"):
        assert callable(getattr(api.MetricRadonIntermediate, name)), name


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_gradient_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_gradient_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gradient abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_gradient_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_gradient")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_gradient.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_of_evaluate_gradient_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_gradient_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_gradient_kernel_resources():
    """small_poses_kernel runs with the record fit and the sampling loops in one set of registers -- at most 88
    vector registers (five waves per SIMD: the 1 197 four-wave workgroups of twelve probes on 400 views are resident at once, five
    per compute unit), no scratch, at most 3 200 bytes of static LDS (the eight record slots and tables of k01_fit_block<8>;
    the staged terms of the several-waves-per-pair forms are dynamic).  msgpack missing is a failure, not a skip."""
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    ks = mod.find(mod.kernels(lib), "18small_poses_kernel")
    assert len(ks) == 7, sorted(ks)   # DERIV x {1, 2, 4} waves per pair, and the reference arithmetic
    for name, k in ks.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 88, (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] <= 3200, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
