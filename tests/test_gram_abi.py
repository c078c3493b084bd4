"""ecc_metric_evaluate_gram (csrc/ecc_gram.hip, csrc/gram_kernel.hip) without a GPU: the symbol and its argument errors, the
prototype from C99, the C++ adapter's evaluateGram in both branches, the Python layer and its host helpers (gram_minimizer,
gram_value), and the resources of the new kernels as DESIGN.md 4.12 plans them -- read from the built library's code object."""
import ctypes as C
import importlib.util
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


def test_library_exports_the_gram_entry_point():
    L = _cdll()
    assert hasattr(L, "ecc_metric_evaluate_gram")
    L.ecc_last_error.restype = C.c_char_p
    vp = C.c_void_p
    L.ecc_metric_evaluate_gram.argtypes = [vp, C.c_int, vp, vp]
    G = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    assert L.ecc_metric_evaluate_gram(None, 2, None, C.addressof(G)) == ECC_ERR_INVALID_ARGUMENT
    assert len(L.ecc_last_error()) > 0 and b"null" in L.ecc_last_error()
    assert L.ecc_metric_evaluate_gram(None, 2, None, None) == ECC_ERR_INVALID_ARGUMENT
    assert len(L.ecc_last_error()) > 0
    assert list(G) == [-1.0] * 4   # nothing written


def test_header_states_the_channel_bound():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert "#define ECC_GRAM_MAX_CHANNELS 4" in text
    assert "int ecc_metric_evaluate_gram(ecc_metric* m, int n_channels, float* pair_grams, double* gram);" in text


def test_python_layer_binds_the_call():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    assert getattr(_lib.lib(), "ecc_metric_evaluate_gram").argtypes is not None
    assert callable(api.MetricRadonIntermediate.evaluate_gram)
    assert callable(api.gram_minimizer) and callable(api.gram_value)
    assert E.gram_minimizer is api.gram_minimizer and E.gram_value is api.gram_value


def test_prototype_is_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_gram_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_gram_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gram abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_gram_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_gram")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_gram.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C call and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_of_evaluate_gram_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_gram_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def _spd(rng, K):
    A = rng.standard_normal((K, K + 2))
    return A @ A.T + 0.1 * np.eye(K)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_gram_minimizer_on_positive_definite_forms(K):
    from epipolarconsistency_amd import gram_minimizer, gram_value
    rng = np.random.default_rng(100 + K)
    for trial in range(20):
        G = _spd(rng, K)
        fixed = trial % K
        value = [1.0, -2.5, 0.75][trial % 3]
        a, v = gram_minimizer(G, fixed=fixed, value=value)
        assert a.dtype == np.float64 and a.shape == (K,)
        assert a[fixed] == value   # kept exactly
        assert v == gram_value(G, a) and abs(v - float(a @ G @ a)) <= 8 * np.finfo(np.float64).eps * float(np.abs(a) @ np.abs(G) @ np.abs(a))
        grad = 2.0 * (G @ a)       # of a^T G a; zero on the free coordinates
        free = [c for c in range(K) if c != fixed]
        scale = 2.0 * np.abs(G) @ np.abs(a)   # the magnitudes the rounded sum is made of
        assert np.all(np.abs(grad[free]) <= 64 * np.finfo(np.float64).eps * np.linalg.cond(G[np.ix_(free, free)]) * scale[free]), (grad, scale)
        for _ in range(5):         # a minimum: every other vector with the same fixed coordinate is worse
            b = a + rng.standard_normal(K) * 0.1
            b[fixed] = value
            assert gram_value(G, b) >= v
    a, v = gram_minimizer(_spd(rng, K))   # defaults: a[0] = 1
    assert a[0] == 1.0


@pytest.mark.parametrize("K", [2, 3, 4])
def test_gram_minimizer_refuses_an_indefinite_block(K):
    from epipolarconsistency_amd import gram_minimizer
    G = np.eye(K)
    G[K - 1, K - 1] = -1.0   # the free block of fixed = 0 has a negative direction: no minimum
    with pytest.raises(np.linalg.LinAlgError):
        gram_minimizer(G, fixed=0)
    G[K - 1, K - 1] = 0.0    # semi-definite: no unique minimiser either
    with pytest.raises(np.linalg.LinAlgError):
        gram_minimizer(G, fixed=0)
    with pytest.raises(ValueError):
        gram_minimizer(np.eye(K), fixed=K)


def test_gram_value_checks_its_shapes():
    from epipolarconsistency_amd import gram_value
    G = np.array([[2.0, 0.5], [0.5, 1.0]])
    assert gram_value(G, [1.0, -1.0]) == 2.0
    with pytest.raises(ValueError):
        gram_value(G, [1.0, 2.0, 3.0])


def test_gram_kernel_resources():
    """pairs_gram_kernel<DERIV, NC> keeps 4 NC gathers of 16 bytes in flight per kappa step and carries NC (NC + 1)
    float64 accumulator registers, so it does not run at pairs_kernel's seven waves per SIMD.  The plan, in allocation blocks of 8
    vector registers: NC = 2 at most 80 (six waves per SIMD), NC = 3 at most 112 (four), NC = 4 at most 152 (three); no scratch in
    any instantiation (a condition), no LDS (one wave per pair, no barrier).  The reference-arithmetic kernels
    (pairs_gram_reference_kernel<NC, SPLIT>) are for evaluations of a few thousand pairs: no scratch, at most 160 vector registers,
    LDS only for the wave sums of the four-waves-per-pair form (T x 4 doubles).  msgpack missing is a failure, not a skip."""
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    ks = mod.find(mod.kernels(lib), "17pairs_gram_kernel")
    assert len(ks) == 6, sorted(ks)   # DERIV x NC in {2, 3, 4}
    ceiling = {2: 80, 3: 112, 4: 152}
    seen = set()
    for name, k in ks.items():
        nc = [c for c in (2, 3, 4) if "ELi%dEEEv" % c in name]
        assert len(nc) == 1, name
        seen.add((("ILb1E" in name), nc[0]))
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= ceiling[nc[0]], (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
    assert len(seen) == 6, sorted(seen)
    rs = mod.find(mod.kernels(lib), "27pairs_gram_reference_kernel")
    assert len(rs) == 6, sorted(rs)   # NC in {2, 3, 4} x {one wave, four waves} per pair
    for name, k in rs.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 160, (name, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] <= 10 * 4 * 8, (name, k[".group_segment_fixed_size"])
    ss = mod.find(mod.kernels(lib), "15sum_gram_kernel")
    assert len(ss) == 1, sorted(ss)
    for name, k in ss.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] == 1024, name
