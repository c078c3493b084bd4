"""ecc_metric_evaluate_robust, ecc_metric_evaluate_robust_pairs and ecc_host_robust_scale (csrc/ecc_robust.hip,
csrc/robust_kernel.hip) without a GPU: the symbols and their argument errors, the prototypes from C99, the C++ adapter's
evaluateRobust / evaluateRobustPairs / robustScale in both branches, the Python layer, the scale against numpy.median, and the
resources of the new kernels as DESIGN.md 4.19 plans them -- read from the built library's code object."""
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


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entry_points():
    """A null metric is an argument error, checked first: whatever the other arguments are -- good ones, nulls, a loss outside 0..2,
    a delta that is 0, negative or NaN, a negative list length -- and nothing is written."""
    L = _cdll()
    for name in ("ecc_metric_evaluate_robust", "ecc_metric_evaluate_robust_pairs", "ecc_host_robust_scale"):
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    vp, f32 = C.c_void_p, C.c_float
    f, g = L.ecc_metric_evaluate_robust, L.ecc_metric_evaluate_robust_pairs
    f.argtypes = [vp, C.c_int, f32, vp, vp, vp]
    g.argtypes = [vp, vp, C.c_int, C.c_int, f32, vp, vp, vp]
    value, mass = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    pairs = (C.c_float * 6)(*([-1.0] * 6))
    idx = (C.c_int32 * 8)(0, 1, 0, 1, 1, 2, 1, 2)
    adr = C.addressof
    assert f(None, 0, 1.0, adr(value), adr(mass), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"null" in L.ecc_last_error()   # the metric is checked first
    for loss, delta in ((0, 1.0), (3, 1.0), (-1, 1.0), (1, 0.0), (2, -2.0), (0, float("nan")), (0, float("inf"))):
        for out in ((adr(value), adr(mass), adr(pairs)), (None, None, None), (adr(value), None, None), (None, adr(mass), adr(pairs))):
            assert f(None, loss, delta, *out) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error(), (loss, delta, out)
            for lst, count in ((adr(idx), 2), (None, 2), (adr(idx), 0), (None, 0), (adr(idx), -1)):
                assert g(None, lst, count, loss, delta, *out) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
    assert value[0] == -1.0 and mass[0] == -1.0 and list(pairs) == [-1.0] * 6   # nothing written


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert "enum { ECC_LOSS_HUBER = 0, ECC_LOSS_TRUNCATED = 1, ECC_LOSS_GEMAN_MCCLURE = 2 };" in text
    assert "int ecc_metric_evaluate_robust(ecc_metric* m, int loss, float delta, double* value, double* inlier_mass, float* pair_terms);" in text
    assert ("int ecc_metric_evaluate_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, double* value,\n"
            "                                     double* inlier_mass, float* pair_terms);") in text
    assert "double ecc_host_robust_scale(const float* pair_terms, int64_t n_pairs, double k);" in text


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in ("ecc_metric_evaluate_robust", "ecc_metric_evaluate_robust_pairs", "ecc_host_robust_scale"):
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.lib().ecc_host_robust_scale.restype is C.c_double
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.evaluate_robust).parameters)[1:] == ["loss", "delta", "want_pairs"]
    assert list(inspect.signature(M.evaluate_robust_pairs).parameters)[1:] == ["idx4", "loss", "delta", "want_pairs"]
    assert inspect.signature(M.evaluate_robust).parameters["want_pairs"].default is False
    assert inspect.signature(M.evaluate_robust_pairs).parameters["want_pairs"].default is False
    assert list(inspect.signature(api.robust_scale).parameters) == ["pair_terms", "k"]
    assert inspect.signature(api.robust_scale).parameters["k"].default == 1.0
    assert E.robust_scale is api.robust_scale and "robust_scale" in E.__all__
    assert (E.LOSS_HUBER, E.LOSS_TRUNCATED, E.LOSS_GEMAN_MCCLURE) == (0, 1, 2)
    for name in ("LOSS_HUBER", "LOSS_TRUNCATED", "LOSS_GEMAN_MCCLURE"):
        assert name in E.__all__ and getattr(E, name) == getattr(_lib, name)


def test_robust_scale_is_the_median_rule():
    """ecc_host_robust_scale (through robust_scale) against numpy.median of sqrt(r) over the rows with r > 0: odd and even counts,
    rows with r == 0 skipped, every row skipped, no rows; the c and u columns are not read."""
    from epipolarconsistency_amd import robust_scale
    rng = np.random.default_rng(19)
    for count, zeros in ((1, 0), (2, 0), (7, 0), (8, 0), (9, 4), (10, 4), (33, 32), (1000, 137), (1001, 0)):
        rows = rng.uniform(0.0, 50.0, (count, 3)).astype(np.float32)
        rows[:, :2] = np.nan                                   # never read
        rows[rng.permutation(count)[:zeros], 2] = 0.0
        live = rows[:, 2][rows[:, 2] > 0].astype(np.float64)
        assert len(live) == count - zeros
        for k in (1.0, 1.4826):
            want = k * float(np.median(np.sqrt(live)))
            got = robust_scale(rows, k)
            assert abs(got - want) <= 4e-16 * want, (count, zeros, k, got, want)
        assert robust_scale(rows) == robust_scale(rows, 1.0)
    dead = np.ones((5, 3), np.float32)
    dead[:, 2] = 0.0
    assert robust_scale(dead) == 0.0 and robust_scale(np.zeros((0, 3), np.float32)) == 0.0
    dead[2, 2] = -4.0                                          # not > 0: skipped as well
    assert robust_scale(dead) == 0.0
    for bad in (np.zeros(6, np.float32), np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError):
            robust_scale(bad)


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_robust_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_robust_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "robust abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_robust")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_robust.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and the static scale, and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_robust_eigen_syntax.cpp")]
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


def test_robust_kernel_resources():
    """pairs_robust_kernel<DERIV> is pairs_weighted_kernel<DERIV> with half as many gather results in flight (4 for
    8) and 8 accumulator registers for its 6: strictly fewer live values, so strictly fewer vector registers than that kernel as
    built and at most its allocation block of 80; at most 106 scalar registers, no scratch, no LDS.  Built: 60 (DERIV) and 57
    vector registers -- pairs_kernel's own 60 / 57 --, 99 / 98 scalar registers."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "19pairs_robust_kernel")
    assert len(ks) == 2, sorted(ks)   # DERIV true and false; the loss is a launch-uniform select, not a template parameter
    weighted = mod.find(all_kernels, "21pairs_weighted_kernel")
    assert len(weighted) == 2, sorted(weighted)
    seen = set()
    for name, k in ks.items():
        deriv = "ILb1E" in name
        seen.add(deriv)
        sibling = [w for wname, w in weighted.items() if ("ILb1E" in wname) == deriv]
        assert len(sibling) == 1
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 80, (name, k[".vgpr_count"])
        assert k[".vgpr_count"] < sibling[0][".vgpr_count"], (name, k[".vgpr_count"], sibling[0][".vgpr_count"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
    assert seen == {True, False}


def test_reference_kernel_resources():
    """pairs_robust_reference_kernel<SPLIT>: no scratch; LDS only for the 4 x 4 float64 wave sums of the four-wave form, 128 bytes."""
    mod, all_kernels = _kernel_resources()
    rs = mod.find(all_kernels, "29pairs_robust_reference_kernel")
    assert len(rs) == 2, sorted(rs)   # one wave, four waves per pair
    seen = set()
    for name, k in rs.items():
        split = [s for s in (1, 4) if "ILi%dEEEv" % s in name]
        assert len(split) == 1, name
        seen.add(split[0])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == (4 * 4 * 8 if split[0] == 4 else 0), (name, k[".group_segment_fixed_size"])
    assert seen == {1, 4}
