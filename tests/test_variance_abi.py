"""ecc_metric_evaluate_variance and its index-list, pose-delta and transform forms (csrc/ecc_variance.hip, csrc/variance_kernel.hip)
without a GPU: the symbols and their argument errors, the prototypes from C99, the C++ adapter's evaluateVariance* in both
branches, the Python layer, ecc_host_variance_floor's values and refusals (also as the stand-alone sanitizer program
tests/c/variance_host.cpp), and the resources of the new kernels as DESIGN.md 4.28 plans them -- read from the built library's
code object."""
import ctypes as C
import importlib.util
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1
NAMES = ("ecc_metric_evaluate_variance", "ecc_metric_evaluate_variance_pairs", "ecc_metric_evaluate_variance_pose_deltas",
         "ecc_metric_evaluate_variance_transforms", "ecc_host_variance_floor")


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entry_points():
    """The four calls and the host helper are exported; a null metric is refused first, with a message, whatever the other arguments
    are, and nothing is written -- no device is needed."""
    L = _cdll()
    for name in NAMES:
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    vp, fl, i = C.c_void_p, C.c_float, C.c_int
    value, mean_weight = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    pairs = (C.c_float * 6)(*([-1.0] * 6))
    idx4, off, views = (C.c_int32 * 4)(0, 1, 0, 1), (C.c_int32 * 2)(0, 1), (C.c_int32 * 1)(0)
    P, T = (C.c_double * 12)(), (C.c_double * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    adr = C.addressof
    f = L.ecc_metric_evaluate_variance
    f.argtypes = [vp, fl, vp, vp, vp]
    assert f(None, 1.0, adr(value), adr(mean_weight), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"null" in L.ecc_last_error()   # the metric is checked first
    for args in ((None, 1.0, None, None, None), (None, 0.0, adr(value), None, None), (None, float("nan"), None, adr(mean_weight), adr(pairs))):
        assert f(*args) == ECC_ERR_INVALID_ARGUMENT and len(L.ecc_last_error()) > 0, args
    g = L.ecc_metric_evaluate_variance_pairs
    g.argtypes = [vp, vp, i, fl, vp, vp, vp]
    assert g(None, adr(idx4), 1, 1.0, adr(value), adr(mean_weight), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    h = L.ecc_metric_evaluate_variance_pose_deltas
    h.argtypes = [vp, i, vp, vp, vp, fl, vp, vp]
    assert h(None, 1, adr(off), adr(views), adr(P), 1.0, adr(value), adr(mean_weight)) == ECC_ERR_INVALID_ARGUMENT
    t = L.ecc_metric_evaluate_variance_transforms
    t.argtypes = [vp, i, i, vp, fl, vp, vp, vp]
    assert t(None, 1, 1, adr(T), 1.0, adr(value), adr(mean_weight), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"null" in L.ecc_last_error()
    assert value[0] == -1.0 and mean_weight[0] == -1.0 and list(pairs) == [-1.0] * 6   # nothing written


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = " ".join(f.read().split())
    for proto in (
            "int ecc_metric_evaluate_variance(ecc_metric* m, float floor, double* value, double* mean_weight, float* pair_terms);",
            "int ecc_metric_evaluate_variance_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float floor, double* value, "
            "double* mean_weight, float* pair_terms);",
            "int ecc_metric_evaluate_variance_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views, "
            "const double* moved_Ps, float floor, double* values, double* mean_weights);",
            "int ecc_metric_evaluate_variance_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, float floor, "
            "double* values, double* mean_weights, float* pair_terms);",
            "int ecc_host_variance_floor(const float* v, int64_t count, double fraction, float* floor);"):
        assert proto in text, proto
    for phrase in ("1.0f / (s < floor ? floor : s)", "one correctly rounded IEEE float32 division", "never applied to a variance sample"):
        assert phrase in text, phrase


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in NAMES:
        assert getattr(_lib.lib(), name).argtypes is not None, name
    M = api.MetricRadonIntermediate

    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(M.evaluate_variance)[1:] == ["floor", "want_pairs"]
    assert params(M.evaluate_variance_pairs)[1:] == ["idx4", "floor", "want_pairs"]
    assert params(M.evaluate_variance_pose_deltas)[1:] == ["moved_views", "moved_Ps", "floor"]
    assert params(M.evaluate_variance_pose_deltas_packed)[1:] == ["moved_offsets", "moved_views", "moved_Ps", "floor"]
    assert params(M.evaluate_variance_transforms)[1:] == ["n_source", "Ts", "floor", "want_pairs"]
    assert params(api.variance_intermediates) == ["ctx", "pixel_variances", "size_alpha", "size_t"]
    assert params(api.variance_floor) == ["fields", "fraction"]
    assert inspect.signature(api.variance_floor).parameters["fraction"].default == 1e-3
    for name in ("variance_intermediates", "variance_floor"):
        assert getattr(E, name) is getattr(api, name) and name in E.__all__
    doc = " ".join(api.variance_intermediates.__doc__.split())
    assert "line integral of the pixel variances" in doc and "constant factor that cancels in value" in doc
    assert "ignores the correlation of the two neighbouring lines of the finite difference" in doc


def test_a_null_metric_is_refused_without_a_device():
    """Through the Python bindings' argument types: every call returns ECC_ERR_INVALID_ARGUMENT for a null handle."""
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    v, u = C.c_double(-1.0), C.c_double(-1.0)
    assert L.ecc_metric_evaluate_variance(None, 1.0, C.byref(v), C.byref(u), None) == ECC_ERR_INVALID_ARGUMENT
    idx = np.array([[0, 1, 0, 1]], np.int32)
    assert L.ecc_metric_evaluate_variance_pairs(None, C.c_void_p(idx.ctypes.data), 1, 1.0, C.byref(v), C.byref(u), None) == ECC_ERR_INVALID_ARGUMENT
    off, out = np.array([0, 0], np.int32), np.full(2, -1.0)
    assert L.ecc_metric_evaluate_variance_pose_deltas(None, 1, C.c_void_p(off.ctypes.data), None, None, 1.0, C.c_void_p(out.ctypes.data),
                                                      None) == ECC_ERR_INVALID_ARGUMENT
    T = np.eye(4).reshape(-1)
    assert L.ecc_metric_evaluate_variance_transforms(None, 1, 1, C.c_void_p(T.ctypes.data), 1.0, C.c_void_p(out.ctypes.data), None,
                                                     None) == ECC_ERR_INVALID_ARGUMENT
    assert v.value == -1.0 and u.value == -1.0 and np.all(out == -1.0)


def test_variance_floor_values_and_refusals():
    """ecc_host_variance_floor (through variance_floor) against numpy.median over the strictly positive finite entries: odd and even
    counts, several fields, entries that do not count; the refusals raise and write nothing."""
    import epipolarconsistency_amd as E
    rng = np.random.default_rng(17)
    for count in (1, 2, 7, 1000, 1001):
        v = rng.uniform(-1.0, 3.0, count).astype(np.float32)
        v[0] = 2.5   # at least one positive entry
        if count > 4:
            v[1:4] = (0.0, np.inf, np.nan)
        good = v[np.isfinite(v) & (v > 0)].astype(np.float64)
        for fraction in (1.0, 1e-3, 0.37):
            want = np.float32(fraction * np.median(good))
            got = E.variance_floor(v, fraction)
            assert np.float32(got) == want, (count, fraction, got, want)
    halves = [np.array([[4.0, 0.0], [1.0, -3.0]], np.float32), np.array([2.0, 8.0])]
    assert E.variance_floor(halves, 1.0) == 3.0 and E.variance_floor(halves) == float(np.float32(3e-3))
    for bad in (np.zeros(5, np.float32), np.array([-1.0, np.nan, np.inf], np.float32), np.zeros(0, np.float32), []):
        with pytest.raises(E.EccError) as e:
            E.variance_floor(bad)
        assert e.value.code == ECC_ERR_INVALID_ARGUMENT
    for fraction in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(E.EccError):
            E.variance_floor(np.ones(3, np.float32), fraction)
    L = _cdll()
    L.ecc_host_variance_floor.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
    v, out = (C.c_float * 3)(1.0, 2.0, 3.0), (C.c_float * 1)(-1.0)
    assert L.ecc_host_variance_floor(C.addressof(v), -1, 1.0, C.addressof(out)) == ECC_ERR_INVALID_ARGUMENT
    assert L.ecc_host_variance_floor(None, 3, 1.0, C.addressof(out)) == ECC_ERR_INVALID_ARGUMENT
    assert L.ecc_host_variance_floor(C.addressof(v), 3, 1.0, None) == ECC_ERR_INVALID_ARGUMENT
    assert out[0] == -1.0
    assert L.ecc_host_variance_floor(C.addressof(v), 3, 1.0, C.addressof(out)) == 0 and out[0] == 2.0


def test_host_helper_is_clean_under_the_sanitizers(tmp_path):
    """csrc/ecc_variance_host.h built alone into tests/c/variance_host.cpp (its own main, no HIP, no library) with
    -fsanitize=address,undefined and run directly."""
    exe = os.path.join(str(tmp_path), "variance_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "c", "variance_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "variance host ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_variance_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_variance_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "variance abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_variance")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_variance.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and the host helper, and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_variance_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_variance_kernel_resources():
    """pairs_variance_kernel<DERIV> holds pairs_weighted_kernel's live values plus the temporaries of two float32
    divisions.  The plan: at most 96 allocated vector registers (five waves per SIMD), no scratch, no LDS.  Built: 73 (DERIV) and 69
    vector registers, pairs_weighted_kernel's own figures -- the allocation block of 80, six waves per SIMD, one more than planned;
    that block is pinned, with at most 106 scalar registers."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "21pairs_variance_kernel")
    assert len(ks) == 2, sorted(ks)   # DERIV true and false
    seen = set()
    for name, k in ks.items():
        seen.add("ILb1E" in name)
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 96, (name, k[".vgpr_count"])   # the plan
        assert k[".vgpr_count"] <= 80, (name, k[".vgpr_count"])   # built: six waves per SIMD
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
    assert seen == {True, False}


def test_reference_kernel_resources():
    """pairs_variance_reference_kernel<SPLIT>: no scratch; LDS only for the 3 x 4 float64 wave sums of the four-wave form."""
    mod, all_kernels = _kernel_resources()
    rs = mod.find(all_kernels, "31pairs_variance_reference_kernel")
    assert len(rs) == 2, sorted(rs)   # one wave, four waves per pair
    seen = set()
    for name, k in rs.items():
        split = [s for s in (1, 4) if "ILi%dEEEv" % s in name]
        assert len(split) == 1, name
        seen.add(split[0])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == (3 * 4 * 8 if split[0] == 4 else 0), (name, k[".group_segment_fixed_size"])
    assert seen == {1, 4}
