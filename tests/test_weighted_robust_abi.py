"""ecc_metric_evaluate_weighted_robust, ecc_metric_evaluate_weighted_robust_pairs and ecc_host_weighted_robust_scale
(csrc/ecc_weighted_robust.hip, csrc/weighted_robust_kernel.hip) without a GPU: the symbols and their argument errors, the prototypes
from C99, the Python layer, the scale against numpy.median, the source list, and the resources of the new kernels as DESIGN.md 4.23
plans them -- read from the built library's code object through scripts/kernel_resources.py, as tests/test_weighted_abi.py reads
them.  (The C++ adapter: tests/test_cpp_adapter_weighted_robust.py.)"""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1
NAMES = ("ecc_metric_evaluate_weighted_robust", "ecc_metric_evaluate_weighted_robust_pairs", "ecc_host_weighted_robust_scale")


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entry_points():
    """A null metric is an argument error, checked first: whatever the other arguments are -- good ones, nulls, a loss outside 0..2,
    a delta that is 0, negative or NaN, a null list, a negative list length -- and nothing is written.  (Every later error of the
    documented precedence needs a live metric: tests/test_gpu_weighted_robust.py::test_errors_in_the_documented_order.)"""
    L = _cdll()
    for name in NAMES:
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    vp, f32 = C.c_void_p, C.c_float
    f, g = L.ecc_metric_evaluate_weighted_robust, L.ecc_metric_evaluate_weighted_robust_pairs
    f.argtypes = [vp, C.c_int, f32, vp, vp, vp, vp]
    g.argtypes = [vp, vp, C.c_int, C.c_int, f32, vp, vp, vp, vp]
    value, cover, mass = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    pairs = (C.c_float * 8)(*([-1.0] * 8))
    idx = (C.c_int32 * 8)(0, 1, 0, 1, 1, 2, 1, 2)
    adr = C.addressof
    assert f(None, 0, 1.0, adr(value), adr(cover), adr(mass), adr(pairs)) == ECC_ERR_INVALID_ARGUMENT
    assert b"metric is null" in L.ecc_last_error()   # the metric is checked first
    for loss, delta in ((0, 1.0), (3, 1.0), (-1, 1.0), (1, 0.0), (2, -2.0), (0, float("nan")), (0, float("inf"))):
        for out in ((adr(value), adr(cover), adr(mass), adr(pairs)), (None, None, None, None), (adr(value), None, None, None),
                    (None, adr(cover), adr(mass), adr(pairs))):
            assert f(None, loss, delta, *out) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error(), (loss, delta, out)
            for lst, count in ((adr(idx), 2), (None, 2), (adr(idx), 0), (None, 0), (adr(idx), -1)):
                assert g(None, lst, count, loss, delta, *out) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error()
    assert value[0] == -1.0 and cover[0] == -1.0 and mass[0] == -1.0 and list(pairs) == [-1.0] * 8   # nothing written


def test_header_states_the_calls_and_their_precedence():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert ("int ecc_metric_evaluate_weighted_robust(ecc_metric* m, int loss, float delta, double* value, double* coverage,\n"
            "                                        double* inlier_mass, float* pair_terms);") in text
    assert ("int ecc_metric_evaluate_weighted_robust_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta,\n"
            "                                              double* value, double* coverage, double* inlier_mass, float* pair_terms);") in text
    assert "double ecc_host_weighted_robust_scale(const float* pair_terms, int64_t n_pairs, double k);" in text
    block = text[text.index("LINE WEIGHTS AND THE ROBUST LOSS TOGETHER"):text.index("int ecc_metric_evaluate_weighted_robust(")]
    block = " ".join(block.replace("\n *", "\n").split())
    order = [block.index(s) for s in ("(1) m == NULL", "(2) the list form: n_pairs < 0", "(3) ecc_metric_evaluate_robust's conditions",
                                      "use_corr: ECC_ERR_UNSUPPORTED", "(4) n_dtrs != 2 * n_views", "(5) the list form: a tuple")]
    assert order == sorted(order)
    not_built = block[block.index("Not built:"):]
    for what in ("pose-delta and transform batches", "range, group and RCCL forms", "use_corr", "Tukey's biweight", "variance form"):
        assert what in not_built, what


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in NAMES:
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib.lib().ecc_host_weighted_robust_scale.restype is C.c_double
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.evaluate_weighted_robust).parameters)[1:] == ["loss", "delta", "want_pairs"]
    assert list(inspect.signature(M.evaluate_weighted_robust_pairs).parameters)[1:] == ["idx4", "loss", "delta", "want_pairs"]
    assert inspect.signature(M.evaluate_weighted_robust).parameters["want_pairs"].default is False
    assert inspect.signature(M.evaluate_weighted_robust_pairs).parameters["want_pairs"].default is False
    assert list(inspect.signature(api.weighted_robust_scale).parameters) == ["pair_terms", "k"]
    assert inspect.signature(api.weighted_robust_scale).parameters["k"].default == 1.0
    assert E.weighted_robust_scale is api.weighted_robust_scale and "weighted_robust_scale" in E.__all__


def test_weighted_robust_scale_is_the_median_rule():
    """ecc_host_weighted_robust_scale (through weighted_robust_scale) against numpy.median of sqrt(r / u) over the rows with r > 0 and
    u > 0, both widened to float64 before the division: odd and even counts, rows with r == 0 or u == 0 skipped, every row skipped, no
    rows; the c and k columns are not read; at u == 1 it is ecc_host_robust_scale of the rows {c, k, r}, to the bit."""
    from epipolarconsistency_amd import robust_scale, weighted_robust_scale
    rng = np.random.default_rng(29)
    for count, zero_r, zero_u in ((1, 0, 0), (2, 0, 0), (7, 0, 0), (8, 0, 0), (9, 4, 0), (10, 2, 2), (33, 16, 16), (1000, 137, 60), (1001, 0, 1)):
        rows = rng.uniform(0.0, 50.0, (count, 4)).astype(np.float32)
        rows[:, 1] = rng.uniform(0.01, 1.0, count).astype(np.float32)
        rows[:, (0, 2)] = np.nan                                   # never read
        perm = rng.permutation(count)
        rows[perm[:zero_r], 3] = 0.0
        rows[perm[zero_r:zero_r + zero_u], 1] = 0.0
        live = (rows[:, 3] > 0) & (rows[:, 1] > 0)
        assert live.sum() == count - zero_r - zero_u
        rms = np.sqrt(rows[live, 3].astype(np.float64) / rows[live, 1].astype(np.float64))
        for k in (1.0, 1.4826):
            want = k * float(np.median(rms))
            got = weighted_robust_scale(rows, k)
            assert abs(got - want) <= 4e-16 * want, (count, zero_r, zero_u, k, got, want)
        assert weighted_robust_scale(rows) == weighted_robust_scale(rows, 1.0)
        ones = rows.copy()
        ones[:, 1] = 1.0
        for k in (1.0, 0.5):
            assert weighted_robust_scale(ones, k) == robust_scale(ones[:, (0, 2, 3)], k), (count, k)
    dead = np.ones((5, 4), np.float32)
    dead[:, 3] = 0.0
    assert weighted_robust_scale(dead) == 0.0 and weighted_robust_scale(np.zeros((0, 4), np.float32)) == 0.0
    dead[2, 3] = -4.0                                              # not > 0: skipped as well
    dead[3] = (1.0, 0.0, 0.0, 9.0)                                 # u == 0
    dead[4] = (1.0, -1.0, 0.0, 9.0)                                # u < 0
    assert weighted_robust_scale(dead) == 0.0
    for bad in (np.zeros(8, np.float32), np.zeros((2, 3), np.float32)):
        with pytest.raises(ValueError):
            weighted_robust_scale(bad)


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_weighted_robust_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_weighted_robust_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "weighted robust abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_source_list_and_flags():
    """The new files are in the build's lists; the kernel file is built without the SLP vectoriser, like its siblings."""
    from epipolarconsistency_amd import build
    assert "weighted_robust_kernel.hip" in build.SOURCES and "ecc_weighted_robust.hip" in build.SOURCES
    assert "ecc_robust_weight.h" in build.HEADERS and "ecc_loss_forms.h" in build.HEADERS
    assert build.PER_SOURCE_FLAGS.get("weighted_robust_kernel.hip") == ["-fno-slp-vectorize"]


LOSS_KERNEL_FILES = ("robust_kernel.hip", "robust_map_kernel.hip", "weighted_robust_kernel.hip", "weighted_robust_map_kernel.hip",
                     "variance_robust_kernel.hip", "variance_robust_map_kernel.hip")


def _csrc_texts():
    csrc = os.path.join(PKG, "csrc")
    texts = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(csrc, name)) as f:
                texts[name] = f.read()
    return texts


def test_robust_weight_is_stated_once():
    """robust_weight is defined once in all of csrc/, in ecc_robust_weight.h; none of the six loss kernel files restates it, they
    take it through the forms header (ecc_loss_forms.h), which includes ecc_robust_weight.h and calls it."""
    texts = _csrc_texts()
    assert {name: t.count("float robust_weight(") for name, t in texts.items() if "float robust_weight(" in t} == {"ecc_robust_weight.h": 1}
    for name in LOSS_KERNEL_FILES:
        assert "float robust_weight(" not in texts[name] and '#include "ecc_loss_forms.h"' in texts[name], name
    forms = texts["ecc_loss_forms.h"]
    assert '#include "ecc_robust_weight.h"' in forms and "robust_weight(L, dp)" in forms and "robust_weight(L, d)" in forms


def test_the_trips_are_stated_once():
    """none of the six loss kernel files states a trip; the forms header states each of the three once per form
    template (RobustForm, FieldLossForm); the deposits are called from ecc_robust_map.h alone, so a map kernel can differ from its
    evaluation in the deposits only."""
    texts = _csrc_texts()
    trips = ("poly_trip(", "exact_trip(", "reference_trip(")
    for name in LOSS_KERNEL_FILES:
        for trip in trips:
            assert trip not in texts[name], (name, trip)
    forms = texts["ecc_loss_forms.h"]
    templates = re.findall(r"\ntemplate <[^>]*>\nstruct (\w+Form) ", forms)
    assert templates == ["RobustForm", "FieldLossForm"], templates
    for trip in trips:
        assert forms.count(trip) == len(templates), (trip, forms.count(trip))
    assert sorted(name for name, t in texts.items() if "deposit_at(" in t) == ["ecc_robust_map.h"]


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_weighted_robust_kernel_resources():
    """pairs_weighted_robust_kernel<DERIV> is pairs_weighted_kernel<DERIV> (built at 73 / 69 vector registers) with
    four more accumulator registers and the loss arithmetic.  The plan was at most 96 vector registers, five waves per SIMD, the
    occupancy of the two-channel coefficient kernel; built it has 78 (DERIV) and 75, inside the allocation block of 80, six waves per
    SIMD -- so 80 is what is pinned.  106 / 106 scalar registers, at most 106 allowed; no scratch, no LDS, 256 threads."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "28pairs_weighted_robust_kernel")
    assert len(ks) == 2, sorted(ks)   # DERIV true and false; the loss is a launch-uniform select, not a template parameter
    seen = set()
    for name, k in ks.items():
        seen.add("ILb1E" in name)
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 80, (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
    assert seen == {True, False}


def test_reference_kernel_resources():
    """pairs_weighted_robust_reference_kernel<SPLIT>: no scratch; LDS only for the 4 x 5 float64 wave sums of the four-wave form, 160
    bytes."""
    mod, all_kernels = _kernel_resources()
    rs = mod.find(all_kernels, "38pairs_weighted_robust_reference_kernel")
    assert len(rs) == 2, sorted(rs)   # one wave, four waves per pair
    seen = set()
    for name, k in rs.items():
        split = [s for s in (1, 4) if "ILi%dEEEv" % s in name]
        assert len(split) == 1, name
        seen.add(split[0])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == (4 * 5 * 8 if split[0] == 4 else 0), (name, k[".group_segment_fixed_size"])
    assert seen == {1, 4}
