"""ecc_metric_evaluate_weighted (csrc/ecc_weighted.hip, csrc/weighted_kernel.hip) without a GPU: the symbol and its argument errors,
the prototype from C99, the C++ adapter's evaluateWeighted in both branches, the Python layer, the host half of line_weights, and
the resources of the new kernels as DESIGN.md 4.15 plans them -- read from the built library's code object."""
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


def test_library_exports_the_entry_point():
    L = _cdll()
    assert hasattr(L, "ecc_metric_evaluate_weighted")
    L.ecc_last_error.restype = C.c_char_p
    vp = C.c_void_p
    f = L.ecc_metric_evaluate_weighted
    f.argtypes = [vp, vp, vp, vp]
    value, coverage = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    pairs = (C.c_float * 6)(*([-1.0] * 6))
    adr = C.addressof
    assert f(None, adr(value), adr(coverage), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"null" in L.ecc_last_error()   # the metric is checked first
    for args in ((None, None, None, None), (None, adr(value), None, None), (None, None, adr(coverage), adr(pairs))):
        assert f(*args) == ECC_ERR_INVALID_ARGUMENT and len(L.ecc_last_error()) > 0, args
    assert value[0] == -1.0 and coverage[0] == -1.0 and list(pairs) == [-1.0] * 6   # nothing written


def test_header_states_the_call():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert "int ecc_metric_evaluate_weighted(ecc_metric* m, double* value, double* coverage, float* pair_terms);" in text


def test_python_layer_binds_the_call():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    assert getattr(_lib.lib(), "ecc_metric_evaluate_weighted").argtypes is not None
    assert callable(api.MetricRadonIntermediate.evaluate_weighted)
    assert list(inspect.signature(api.MetricRadonIntermediate.evaluate_weighted).parameters)[1:] == ["want_pairs"]
    assert list(inspect.signature(api.line_weights).parameters) == ["ctx", "flagged", "size_alpha", "size_t", "zero_at_px", "guard_bins"]
    assert inspect.signature(api.line_weights).parameters["zero_at_px"].default == 1.0
    assert inspect.signature(api.line_weights).parameters["guard_bins"].default == 1
    for name in ("line_weights", "line_weights_from_lengths"):
        assert getattr(E, name) is getattr(api, name) and name in E.__all__


def test_prototype_is_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_weighted_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_weighted_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "weighted abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_weighted")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C call and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the host half of line_weights -----------------------------------------------------------------------------------------
def test_line_weights_from_lengths():
    """clip(1 - L / zero_at_px, 0, 1) in float32, then the minimum over the (2 g + 1)^2 neighbourhood with clamped edges: against a
    direct loop, bit for bit; after it every bin with a weight above 0 has no neighbour within g bins with L >= zero_at_px."""
    from epipolarconsistency_amd import line_weights_from_lengths
    rng = np.random.default_rng(3)
    L = np.where(rng.random((13, 17)) < 0.2, rng.uniform(0.0, 3.0, (13, 17)), 0.0).astype(np.float32)
    L[0, 0], L[12, 16] = 5.0, 0.25   # the corners: the clamped edges
    for zero_at, g in ((1.0, 0), (1.0, 1), (2.5, 2)):
        raw = np.clip(np.float32(1.0) - L / np.float32(zero_at), np.float32(0.0), np.float32(1.0)).astype(np.float32)
        want = np.empty_like(raw)
        for j in range(13):
            for i in range(17):
                want[j, i] = raw[max(j - g, 0):j + g + 1, max(i - g, 0):i + g + 1].min()
        got = line_weights_from_lengths(L, zero_at, g)
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (zero_at, g)
        assert got.min() >= 0.0 and got.max() <= 1.0
        for j, i in np.argwhere(got > 0):
            assert L[max(j - g, 0):j + g + 1, max(i - g, 0):i + g + 1].max() < zero_at
    assert np.array_equal(line_weights_from_lengths(np.zeros((4, 5), np.float32)), np.ones((4, 5), np.float32))
    for bad in (dict(zero_at_px=0.0), dict(guard_bins=-1)):
        with pytest.raises(ValueError):
            line_weights_from_lengths(L, **bad)
    with pytest.raises(ValueError):
        line_weights_from_lengths(L[0])


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_weighted_kernel_resources():
    """pairs_weighted_kernel<DERIV> keeps the 8 gathers of a kappa step in flight as pairs_coeff_kernel<DERIV, 2> does,
    with 6 accumulator registers against its 10 and no coefficient registers: strictly fewer live values, so at most that kernel's built
    86 vector registers (five waves per SIMD) and at most 106 scalar registers, no scratch, no LDS.  Built: 73 (DERIV) and 69 vector
    registers, 104 scalar registers -- the allocation block of 80, six waves per SIMD, one more than planned; the block is pinned."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "21pairs_weighted_kernel")
    assert len(ks) == 2, sorted(ks)   # DERIV true and false
    coeff = mod.find(all_kernels, "18pairs_coeff_kernelILb1ELi2E")
    assert len(coeff) == 1, sorted(coeff)
    coeff_vgprs = list(coeff.values())[0][".vgpr_count"]
    assert coeff_vgprs <= 86, coeff_vgprs
    seen = set()
    for name, k in ks.items():
        seen.add("ILb1E" in name)
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 80, (name, k[".vgpr_count"])          # built: six waves per SIMD
        assert k[".vgpr_count"] <= coeff_vgprs, (name, k[".vgpr_count"])  # the plan: no more than the two-channel coefficient kernel
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
    assert seen == {True, False}


def test_reference_kernel_resources():
    """pairs_weighted_reference_kernel<SPLIT>: no scratch; LDS only for the 3 x 4 float64 wave sums of the four-wave form."""
    mod, all_kernels = _kernel_resources()
    rs = mod.find(all_kernels, "31pairs_weighted_reference_kernel")
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
