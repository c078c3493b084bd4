"""ecc_metric_evaluate_residual_histogram[_pairs], ecc_metric_evaluate_variance_residual_histogram[_pairs] and
ecc_host_histogram_quantile (csrc/ecc_residual_histogram.hip, csrc/residual_histogram_kernel.hip, csrc/ecc_histogram_host.h) without
a GPU: the symbols and the argument errors that need no device, the prototypes in the header, the Python layer, the quantile's
values (also as the stand-alone sanitizer program tests/c/histogram_host.cpp), and the resources of the new kernels as DESIGN.md
4.34 plans them -- read from the built library's code object."""
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
CALLS = ("ecc_metric_evaluate_residual_histogram", "ecc_metric_evaluate_residual_histogram_pairs",
         "ecc_metric_evaluate_variance_residual_histogram", "ecc_metric_evaluate_variance_residual_histogram_pairs")
NAMES = CALLS + ("ecc_host_histogram_quantile",)


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entry_points():
    """A null metric is an argument error, checked first, whatever the other arguments are, and nothing is written."""
    L = _cdll()
    for name in NAMES:
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    vp, f32, i = C.c_void_p, C.c_float, C.c_int
    raw, raw_pairs, var, var_pairs = (getattr(L, name) for name in CALLS)
    raw.argtypes = [vp, f32, i, vp]
    raw_pairs.argtypes = [vp, vp, i, f32, i, vp]
    var.argtypes = [vp, f32, f32, i, vp]
    var_pairs.argtypes = [vp, vp, i, f32, f32, i, vp]
    counts = (C.c_uint64 * 128)(*([7] * 128))
    idx = (C.c_int32 * 8)(0, 1, 0, 1, 1, 2, 1, 2)
    adr = C.addressof
    for width in (0.5, 0.0, -1.0, float("inf"), float("nan")):
        for n_bins in (64, 0, 63, 2048, -64):
            for out in (adr(counts), None):
                assert raw(None, width, n_bins, out) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error()
                for floor in (1.5, 0.0, float("nan")):
                    assert var(None, floor, width, n_bins, out) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error()
                for lst, count in ((adr(idx), 2), (None, 2), (adr(idx), 0), (adr(idx), -1)):
                    assert raw_pairs(None, lst, count, width, n_bins, out) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error()
                    assert var_pairs(None, lst, count, 1.5, width, n_bins, out) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error()
    assert list(counts) == [7] * 128


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = " ".join(f.read().split())
    for proto in ("int ecc_metric_evaluate_residual_histogram(ecc_metric* m, float width, int n_bins, uint64_t* counts);",
                  "int ecc_metric_evaluate_residual_histogram_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float width, int n_bins, "
                  "uint64_t* counts);",
                  "int ecc_metric_evaluate_variance_residual_histogram(ecc_metric* m, float floor, float width, int n_bins, uint64_t* counts);",
                  "int ecc_metric_evaluate_variance_residual_histogram_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, float floor, float width, "
                  "int n_bins, uint64_t* counts);",
                  "double ecc_host_histogram_quantile(const uint64_t* counts, int n_bins, double width, double q);"):
        assert proto in text, proto
    for phrase in ("a = fabsf(d)", "x = a * inv_width", "bin = x < (float)(n_bins - 1) ? (int)x : n_bins - 1", "the last bin is the OVERFLOW bin",
                   "inv_width = (float)(1.0 / (double)width), formed on the host", "sc = s < floor ? floor : s", "a = fabsf(d) / sqrtf(sc)",
                   "WRITTEN COMPLETELY", "a multiple of 64 with 64 <= n_bins <= 1024", "counts is all zeros",
                   "Not built: pose-delta and transform batches; the form under line weights (counts would not be integers);"):
        assert phrase in text, phrase


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in NAMES:
        assert getattr(_lib.lib(), name).argtypes is not None, name
    assert _lib.lib().ecc_host_histogram_quantile.restype is C.c_double
    M = api.MetricRadonIntermediate

    def params(fn):
        return list(inspect.signature(fn).parameters)
    assert params(M.evaluate_residual_histogram)[1:] == ["width", "n_bins"]
    assert params(M.evaluate_residual_histogram_pairs)[1:] == ["idx4", "width", "n_bins"]
    assert params(M.evaluate_variance_residual_histogram)[1:] == ["floor", "width", "n_bins"]
    assert params(M.evaluate_variance_residual_histogram_pairs)[1:] == ["idx4", "floor", "width", "n_bins"]
    for fn in (M.evaluate_residual_histogram, M.evaluate_residual_histogram_pairs, M.evaluate_variance_residual_histogram,
               M.evaluate_variance_residual_histogram_pairs):
        assert inspect.signature(fn).parameters["n_bins"].default == 256
    assert params(api.histogram_quantile) == ["counts", "width", "q"]
    p = inspect.signature(api.sample_robust_scale).parameters
    assert list(p) == ["metric", "q", "k", "n_bins", "floor", "first_width"]
    assert [p[k].default for k in list(p)[1:]] == [0.5, 1.4826, 256, None, None]
    for name in ("histogram_quantile", "sample_robust_scale"):
        assert getattr(E, name) is getattr(api, name) and name in E.__all__


def test_histogram_quantile_values():
    """ecc_host_histogram_quantile (through histogram_quantile) on rows whose answer is known in closed form, against the numpy
    statement of residual_histogram_terms, and on a sum of rows; the edge cases of the header."""
    import epipolarconsistency_amd as E
    import residual_histogram_terms as H
    row = np.array([10, 30, 40, 20], np.uint64)
    for q, want in ((0.0, 0.0), (0.05, 0.25), (0.1, 0.5), (0.25, 0.75), (0.5, 1.125), (0.8, 1.5), (0.81, np.inf), (1.0, np.inf)):
        assert E.histogram_quantile(row, 0.5, q) == want == H.quantile(row, 0.5, q), (q, want)
    table = np.array([[10, 0, 40, 0], [0, 30, 0, 20]], np.uint64)   # the rows are added first
    assert E.histogram_quantile(table, 0.5, 0.5) == 1.125
    assert E.histogram_quantile(np.zeros(64, np.uint64), 1.0, 0.5) == 0.0
    for q in (-0.1, 1.1, float("nan")):
        assert np.isnan(E.histogram_quantile(row, 0.5, q))
    for w in (0.0, -1.0, float("inf"), float("nan")):
        assert np.isnan(E.histogram_quantile(row, w, 0.5))
    rng = np.random.default_rng(29)
    for n_bins in (64, 256, 1024):
        counts = rng.integers(0, 1000, n_bins).astype(np.uint64)
        for q in (0.0, 0.01, 0.37, 0.5, 0.9, 0.999, 1.0):
            got, want = E.histogram_quantile(counts, 0.031, q), H.quantile(counts, 0.031, q)
            assert got == want or abs(got - want) <= 1e-12 * want, (n_bins, q, got, want)
    with pytest.raises(ValueError):
        E.histogram_quantile(np.zeros((3, 0), np.uint64), 1.0, 0.5)
    L = _cdll()
    L.ecc_host_histogram_quantile.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    L.ecc_host_histogram_quantile.restype = C.c_double
    assert L.ecc_host_histogram_quantile(None, 4, 0.5, 0.5) == 0.0
    assert L.ecc_host_histogram_quantile(C.c_void_p(row.ctypes.data), 0, 0.5, 0.5) == 0.0
    assert np.isnan(L.ecc_host_histogram_quantile(None, 4, 0.5, 2.0))


def test_host_helper_is_clean_under_the_sanitizers(tmp_path):
    """csrc/ecc_histogram_host.h built alone into tests/c/histogram_host.cpp (its own main, no HIP, no library) with
    -fsanitize=address,undefined and run directly."""
    exe = os.path.join(str(tmp_path), "histogram_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "c", "histogram_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "histogram host ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])


def test_the_counters_are_stated_once():
    """the bin rule, the wave's counters and their ordering are in ecc_residual_histogram.h alone; the kernel file
    takes them from there, sits on the frames of ecc_pair_forms.h and contains no inline assembly and no float atomic."""
    csrc = os.path.join(PKG, "csrc")
    texts = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(csrc, name)) as f:
                texts[name] = f.read()
    for definition in ("struct WaveCounters", "void wave_counters_order()", "float studentised_residual("):
        assert {name: t.count(definition) for name, t in texts.items() if definition in t} == {"ecc_residual_histogram.h": 1}, definition
    kernel = texts["residual_histogram_kernel.hip"].split("#include <hip/hip_runtime.h>")[-1]
    assert '#include "ecc_pair_forms.h"' in kernel and '#include "ecc_residual_histogram.h"' in kernel
    assert "form_main_sums<DERIV>(" in kernel and "form_reference_sums<SPLIT>(" in kernel and "launch_pair_form(" in kernel
    assert "asm" not in kernel and "__syncthreads" not in kernel and "atomicAdd" not in kernel
    header = texts["ecc_residual_histogram.h"]
    assert "asm" not in header.replace("__ATOMIC", "") and "__syncthreads" not in header
    assert "__builtin_amdgcn_wave_barrier()" in header and '__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront")' in header
    assert "x < last_f ? (int)x : last" in header   # the clamp in float, before the conversion


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


MAIN = (("31pairs_residual_histogram_kernel", 48), ("40pairs_variance_residual_histogram_kernel", 64))
REFERENCE = ("41pairs_residual_histogram_reference_kernel", "50pairs_variance_residual_histogram_reference_kernel")


def test_main_kernel_resources():
    """DESIGN.md 4.34, the plan: no scratch; at most 96 vector registers, the siblings' plan; at most 106 scalar registers; 256
    threads; NO static LDS -- the 4 x n_bins counters are the launch's dynamic LDS (ecc_residual_histogram_lds_bytes), sized by the
    call and not by the largest table.  Built: 44 (DERIV) and 43 vector registers for the raw form -- no float64 sums to keep --, the
    allocation block of 48 pinned (ten waves per SIMD); the variance form 64 and 61, the block of 64 pinned (eight)."""
    mod, all_kernels = _kernel_resources()
    for mangled, block in MAIN:
        ks = mod.find(all_kernels, mangled)
        assert len(ks) == 2, sorted(ks)   # DERIV true and false
        seen = set()
        for name, k in ks.items():
            seen.add("ILb1E" in name)
            assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
            assert k[".vgpr_count"] <= 96, (name, k[".vgpr_count"])      # the plan
            assert k[".vgpr_count"] <= block, (name, k[".vgpr_count"])   # built
            assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
            assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
            assert k[".max_flat_workgroup_size"] == 256, name
        assert seen == {True, False}


def test_reference_kernel_resources():
    """The reference kernels: no scratch, at most 96 vector registers, 256 threads.  Static LDS: at most the frame's wave-sum slots
    of the four-wave form (form_reference_sums: 4 float64 for the one sum these forms hand it); that sum is never added to, the
    compiler drops the slots, and 0 bytes were built -- the counters are dynamic LDS here as well."""
    mod, all_kernels = _kernel_resources()
    for mangled in REFERENCE:
        rs = mod.find(all_kernels, mangled)
        assert len(rs) == 2, sorted(rs)   # one wave, four waves per pair
        seen = set()
        for name, k in rs.items():
            split = [s for s in (1, 4) if "ILi%dEEEv" % s in name]
            assert len(split) == 1, name
            seen.add(split[0])
            assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
            assert k[".vgpr_count"] <= 96, (name, k[".vgpr_count"])
            assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
            assert k[".group_segment_fixed_size"] <= (4 * 8 if split[0] == 4 else 0), (name, k[".group_segment_fixed_size"])
            assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])   # built
            assert k[".max_flat_workgroup_size"] == 256, name
        assert seen == {1, 4}
