"""ecc_metric_evaluate_variance_robust and its index-list, pose-delta and transform forms (csrc/ecc_variance_robust.hip,
csrc/variance_robust_kernel.hip) without a GPU: the symbols and their argument errors, the prototypes from C99, the C++ adapter's
evaluateVarianceRobust* in both branches, the Python layer, ecc_host_variance_robust_scale's values (also as the stand-alone sanitizer
program tests/c/variance_robust_host.cpp), and the resources of the new kernels as DESIGN.md 4.30 plans them -- read from the built
library's code object."""
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
NAMES = ("ecc_metric_evaluate_variance_robust", "ecc_metric_evaluate_variance_robust_pairs", "ecc_metric_evaluate_variance_robust_pose_deltas",
         "ecc_metric_evaluate_variance_robust_transforms", "ecc_host_variance_robust_scale")


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
    value, mean_weight, inlier_mass = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    pairs = (C.c_float * 8)(*([-1.0] * 8))
    idx4, off, views = (C.c_int32 * 4)(0, 1, 0, 1), (C.c_int32 * 2)(0, 1), (C.c_int32 * 1)(0)
    P, T = (C.c_double * 12)(), (C.c_double * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    adr = C.addressof
    f = L.ecc_metric_evaluate_variance_robust
    f.argtypes = [vp, i, fl, fl, vp, vp, vp, vp]
    assert f(None, 1, 2.0, 1.0, adr(value), adr(mean_weight), adr(inlier_mass), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"null" in L.ecc_last_error()   # the metric is checked first
    for args in ((None, 1, 2.0, 1.0, None, None, None, None), (None, 7, 2.0, 1.0, adr(value), None, None, None),
                 (None, 0, -1.0, 1.0, adr(value), None, None, None), (None, 2, float("nan"), 0.0, None, adr(mean_weight), adr(inlier_mass), adr(pairs))):
        assert f(*args) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error(), args
    g = L.ecc_metric_evaluate_variance_robust_pairs
    g.argtypes = [vp, vp, i, i, fl, fl, vp, vp, vp, vp]
    assert g(None, adr(idx4), 1, 1, 2.0, 1.0, adr(value), adr(mean_weight), adr(inlier_mass), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert g(None, None, -1, 1, 2.0, 1.0, None, None, None, None) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error()
    h = L.ecc_metric_evaluate_variance_robust_pose_deltas
    h.argtypes = [vp, i, vp, vp, vp, i, fl, fl, vp, vp, vp]
    assert h(None, 1, adr(off), adr(views), adr(P), 1, 2.0, 1.0, adr(value), adr(mean_weight), adr(inlier_mass)) == ECC_ERR_INVALID_ARGUMENT
    assert b"metric is null" in L.ecc_last_error()
    t = L.ecc_metric_evaluate_variance_robust_transforms
    t.argtypes = [vp, i, i, vp, i, fl, fl, vp, vp, vp, vp]
    assert t(None, 1, 1, adr(T), 1, 2.0, 1.0, adr(value), adr(mean_weight), adr(inlier_mass), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"metric is null" in L.ecc_last_error()
    assert value[0] == -1.0 and mean_weight[0] == -1.0 and inlier_mass[0] == -1.0 and list(pairs) == [-1.0] * 8   # nothing written


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = " ".join(f.read().split())
    for proto in (
            "int ecc_metric_evaluate_variance_robust(ecc_metric* m, int loss, float delta, float floor, double* value, double* mean_weight, "
            "double* inlier_mass, float* pair_terms);",
            "int ecc_metric_evaluate_variance_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, float floor, "
            "double* value, double* mean_weight, double* inlier_mass, float* pair_terms);",
            "int ecc_metric_evaluate_variance_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views, "
            "const double* moved_Ps, int loss, float delta, float floor, double* values, double* mean_weights, double* inlier_masses);",
            "int ecc_metric_evaluate_variance_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta, "
            "float floor, double* values, double* mean_weights, double* inlier_masses, float* pair_terms);",
            "double ecc_host_variance_robust_scale(const float* pair_terms, int64_t n_pairs, double k);"):
        assert proto in text, proto
    for phrase in ("sc = s < floor ? floor : s", "om = 1.0f / sc", "thr = delta * sqrtf(sc); t = fminf(1.0f, thr / a); w = t * (2.0f - t) | t * t",
                   "q = a * inv_delta; w = 1.0f / fmaf(q * om, q, 1.0f)", "f = om * w", "(double)(om_p * (dp * dp)) + (double)(om_m * (dm * dm))",
                   "inv_delta = (float)(1.0 / (double)delta) is formed on the host", "never divided by the kept mass", "{0, 1, 1, 0}",
                   "This block supersedes", "the maps of this form", "a covariance-aware model for derivative data"):
        assert phrase in text, phrase
    # the older blocks stand as they were
    assert "its combination with the robust * loss" in text and "a 1 / (sigma0^2 + sigma1^2) variance form" in text


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in NAMES:
        assert getattr(_lib.lib(), name).argtypes is not None, name
    assert _lib.lib().ecc_host_variance_robust_scale.restype is C.c_double
    M = api.MetricRadonIntermediate

    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(M.evaluate_variance_robust)[1:] == ["loss", "delta", "floor", "want_pairs"]
    assert params(M.evaluate_variance_robust_pairs)[1:] == ["idx4", "loss", "delta", "floor", "want_pairs"]
    assert params(M.evaluate_variance_robust_pose_deltas)[1:] == ["moved_views", "moved_Ps", "loss", "delta", "floor"]
    assert params(M.evaluate_variance_robust_pose_deltas_packed)[1:] == ["moved_offsets", "moved_views", "moved_Ps", "loss", "delta", "floor"]
    assert params(M.evaluate_variance_robust_transforms)[1:] == ["n_source", "Ts", "loss", "delta", "floor", "want_pairs"]
    for fn in (M.evaluate_variance_robust, M.evaluate_variance_robust_pairs, M.evaluate_variance_robust_transforms):
        assert inspect.signature(fn).parameters["want_pairs"].default is False
    assert params(api.variance_robust_scale) == ["pair_terms", "k"]
    assert inspect.signature(api.variance_robust_scale).parameters["k"].default == 1.0
    assert E.variance_robust_scale is api.variance_robust_scale and "variance_robust_scale" in E.__all__


def test_a_null_metric_is_refused_without_a_device():
    """Through the Python bindings' argument types: every call returns ECC_ERR_INVALID_ARGUMENT for a null handle."""
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    v, u, k = C.c_double(-1.0), C.c_double(-1.0), C.c_double(-1.0)
    assert L.ecc_metric_evaluate_variance_robust(None, 1, 2.0, 1.0, C.byref(v), C.byref(u), C.byref(k), None) == ECC_ERR_INVALID_ARGUMENT
    idx = np.array([[0, 1, 0, 1]], np.int32)
    assert L.ecc_metric_evaluate_variance_robust_pairs(None, C.c_void_p(idx.ctypes.data), 1, 1, 2.0, 1.0, C.byref(v), C.byref(u), C.byref(k),
                                                       None) == ECC_ERR_INVALID_ARGUMENT
    off, out = np.array([0, 0], np.int32), np.full(2, -1.0)
    assert L.ecc_metric_evaluate_variance_robust_pose_deltas(None, 1, C.c_void_p(off.ctypes.data), None, None, 1, 2.0, 1.0,
                                                             C.c_void_p(out.ctypes.data), None, None) == ECC_ERR_INVALID_ARGUMENT
    T = np.eye(4).reshape(-1)
    assert L.ecc_metric_evaluate_variance_robust_transforms(None, 1, 1, C.c_void_p(T.ctypes.data), 1, 2.0, 1.0, C.c_void_p(out.ctypes.data), None,
                                                            None, None) == ECC_ERR_INVALID_ARGUMENT
    assert v.value == -1.0 and u.value == -1.0 and k.value == -1.0 and np.all(out == -1.0)


def test_variance_robust_scale_against_numpy():
    """ecc_host_variance_robust_scale (through variance_robust_scale) against numpy.median of the float64 roots over the rows with
    r > 0: odd and even counts of live rows, rows with r == 0 among them, no live row -> 0.0, no row -> 0.0; only column 3 is read."""
    import epipolarconsistency_amd as E
    rng = np.random.default_rng(23)
    for count, dead in ((1, 0), (2, 0), (7, 2), (8, 3), (1000, 17), (1001, 18), (1001, 17)):
        rows = rng.uniform(0.1, 50.0, (count, 4)).astype(np.float32)
        rows[:, :3] = rng.uniform(-5.0, 5.0, (count, 3)).astype(np.float32)   # c, u, k do not matter
        rows[rng.permutation(count)[:dead], 3] = 0.0
        live = rows[rows[:, 3] > 0, 3].astype(np.float64)
        assert len(live) == count - dead
        for k in (1.0, 2.0, 0.37):
            want = k * float(np.median(np.sqrt(live)))
            got = E.variance_robust_scale(rows, k)
            assert got == want or abs(got - want) <= 4 * np.finfo(np.float64).eps * want, (count, dead, k, got, want)
    rows = np.array([[9, 9, 9, 4.0], [9, 9, 9, 0.0], [9, 9, 9, 16.0], [9, 9, 9, 9.0]], np.float32)
    assert E.variance_robust_scale(rows) == 3.0 and E.variance_robust_scale(rows, 2.0) == 6.0
    assert E.variance_robust_scale(rows[:3]) == 3.0      # live: 2 and 4
    assert E.variance_robust_scale(rows[1:2]) == 0.0     # no live row
    assert E.variance_robust_scale(np.zeros((5, 4), np.float32)) == 0.0
    assert E.variance_robust_scale(np.zeros((0, 4), np.float32)) == 0.0
    for bad in (np.zeros((3, 3), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            E.variance_robust_scale(bad)
    L = _cdll()
    L.ecc_host_variance_robust_scale.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.ecc_host_variance_robust_scale.restype = C.c_double
    assert L.ecc_host_variance_robust_scale(None, 4, 1.0) == 0.0
    assert L.ecc_host_variance_robust_scale(C.c_void_p(rows.ctypes.data), -1, 1.0) == 0.0


def test_host_helper_is_clean_under_the_sanitizers(tmp_path):
    """csrc/ecc_variance_robust_host.h built alone into tests/c/variance_robust_host.cpp (its own main, no HIP, no library) with
    -fsanitize=address,undefined and run directly."""
    exe = os.path.join(str(tmp_path), "variance_robust_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "c", "variance_robust_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "variance robust host ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_variance_robust_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_variance_robust_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "variance robust abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_variance_robust")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_variance_robust.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and the host helper, and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_variance_robust_eigen_syntax.cpp")]
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


def test_variance_robust_kernel_resources():
    """pairs_variance_robust_kernel<DERIV> holds pairs_weighted_robust_kernel's live values (78 / 75 vector registers
    built) plus the temporaries of two square roots and two more divisions.  The plan: at most 96 allocated vector registers (five
    waves per SIMD), no scratch, no LDS.  Built: 80 (DERIV) and 77 vector registers -- the allocation block of 80, six waves per SIMD,
    one more than planned; that block is pinned, with at most 106 scalar registers."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "28pairs_variance_robust_kernel")
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
    """pairs_variance_robust_reference_kernel<SPLIT>: no scratch; LDS only for the 5 x 4 float64 wave sums of the four-wave form."""
    mod, all_kernels = _kernel_resources()
    rs = mod.find(all_kernels, "38pairs_variance_robust_reference_kernel")
    assert len(rs) == 2, sorted(rs)   # one wave, four waves per pair
    seen = set()
    for name, k in rs.items():
        split = [s for s in (1, 4) if "ILi%dEEEv" % s in name]
        assert len(split) == 1, name
        seen.add(split[0])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 96, (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == (5 * 4 * 8 if split[0] == 4 else 0), (name, k[".group_segment_fixed_size"])
    assert seen == {1, 4}
