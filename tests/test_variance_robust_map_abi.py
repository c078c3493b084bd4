"""ecc_metric_evaluate_variance_robust_map, ecc_metric_evaluate_variance_robust_map_pairs and ecc_metric_variance_robust_map_variances
(csrc/ecc_variance_robust_map.hip, csrc/variance_robust_map_kernel.hip) without a GPU: the symbols and the argument errors that need
no device, the prototypes in the header, the Python layer, and the resources of the new kernels as DESIGN.md 4.31 plans them -- read
from the built library's code object."""
import ctypes as C
import importlib.util
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1
NAMES = ("ecc_metric_evaluate_variance_robust_map", "ecc_metric_evaluate_variance_robust_map_pairs", "ecc_metric_variance_robust_map_variances")


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
    f, g, w = (getattr(L, name) for name in NAMES)
    f.argtypes = [vp, i, f32, f32, vp, i, vp, vp, vp, vp, vp, vp]
    g.argtypes = [vp, vp, i, i, f32, f32, vp, i, vp, vp, vp, vp, vp, vp]
    w.argtypes = [vp, f32, f32, f32, f32, vp]
    value, weight, mass = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    pairs, planes = (C.c_float * 8)(*([-1.0] * 8)), (C.c_float * 8)(*([-1.0] * 8))
    idx, views, dup = (C.c_int32 * 8)(0, 1, 0, 1, 1, 2, 1, 2), (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 1)
    adr = C.addressof
    for loss, delta, floor in ((0, 1.0, 1.5), (3, 1.0, 1.5), (1, 0.0, 1.5), (2, -2.0, 0.0), (0, float("nan"), float("nan")), (0, float("inf"), -1.0)):
        for vs, k in ((None, 0), (adr(views), 2), (adr(dup), 2), (None, 2), (adr(views), -1)):
            for out in ((adr(planes), adr(planes), adr(value), adr(weight), adr(mass), adr(pairs)), (None, None, None, None, None, None)):
                assert f(None, loss, delta, floor, vs, k, *out) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
                for lst, count in ((adr(idx), 2), (None, 2), (adr(idx), 0), (adr(idx), -1)):
                    assert g(None, lst, count, loss, delta, floor, vs, k, *out) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
    handles = (C.c_void_p * 2)(None, None)
    for floor, min_hits, gain, max_factor in ((1.5, 1.0, 1.0, 1e4), (0.0, -1.0, 1.0, 0.5), (1.5, 1.0, float("nan"), 1e4), (float("inf"), float("inf"), 1.0, 1.0)):
        for out in (adr(handles), None):
            assert w(None, floor, min_hits, gain, max_factor, out) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
    assert value[0] == -1.0 and weight[0] == -1.0 and mass[0] == -1.0 and list(pairs) == [-1.0] * 8 and list(planes) == [-1.0] * 8
    assert handles[0] is None and handles[1] is None


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = " ".join(f.read().split())
    for proto in ("int ecc_metric_evaluate_variance_robust_map(ecc_metric* m, int loss, float delta, float floor, const int32_t* views, "
                  "int n_mapped, float* hits, float* rejected, double* value, double* mean_weight, double* inlier_mass, float* pair_terms);",
                  "int ecc_metric_evaluate_variance_robust_map_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, int loss, float delta, "
                  "float floor, const int32_t* views, int n_mapped, float* hits, float* rejected, double* value, double* mean_weight, "
                  "double* inlier_mass, float* pair_terms);",
                  "int ecc_metric_variance_robust_map_variances(ecc_metric* m, float floor, float min_hits, float gain, float max_factor, "
                  "ecc_dtr** out);"):
        assert proto in text, proto
    assert "COUNT units" in text and "factor == 1.0f ? old : (old < half ? half : old) * factor" in text


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in NAMES:
        assert getattr(_lib.lib(), name).argtypes is not None
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.evaluate_variance_robust_map).parameters)[1:] == ["loss", "delta", "floor", "views", "want_pairs"]
    assert list(inspect.signature(M.evaluate_variance_robust_map_pairs).parameters)[1:] == ["idx4", "loss", "delta", "floor", "views", "want_pairs"]
    assert inspect.signature(M.evaluate_variance_robust_map).parameters["views"].default is None
    assert inspect.signature(M.evaluate_variance_robust_map).parameters["want_pairs"].default is False
    p = inspect.signature(M.variance_robust_map_variances).parameters
    assert list(p)[1:] == ["floor", "min_hits", "gain", "max_factor"]
    assert (p["min_hits"].default, p["gain"].default, p["max_factor"].default) == (1.0, 1.0, 1e4)
    p = inspect.signature(E.refine_variances).parameters
    assert list(p) == ["ctx", "Ps", "data", "variances", "floor", "loss", "k", "passes", "min_hits", "gain", "max_factor", "sampling"]
    assert [p[k].default for k in list(p)[5:]] == [E.LOSS_TRUNCATED, 2.0, 2, 1.0, 1.0, 1e4, "auto"]
    assert "refine_variances" in E.__all__


def test_the_studentised_weight_is_stated_once():
    """the weight is defined once in all of csrc/, in ecc_studentised_weight.h; no .hip file and not the forms
    header (ecc_loss_forms.h), through which both kernel files take it, states its arithmetic again."""
    csrc = os.path.join(PKG, "csrc")
    texts = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(csrc, name)) as f:
                texts[name] = f.read()
    definition = "StudentisedWeight studentised_weight("
    assert {name: t.count(definition) for name, t in texts.items() if definition in t} == {"ecc_studentised_weight.h": 1}
    for name, text in texts.items():
        if name.endswith(".hip") or name == "ecc_loss_forms.h":
            code = text.split("#include <hip/hip_runtime.h>")[-1] if name.endswith(".hip") else text
            assert "sqrtf(sc)" not in code, name
    for name in ("variance_robust_kernel.hip", "variance_robust_map_kernel.hip"):
        assert '#include "ecc_loss_forms.h"' in texts[name] and definition not in texts[name], name
    forms = texts["ecc_loss_forms.h"]
    assert '#include "ecc_studentised_weight.h"' in forms and "studentised_weight(L, " in forms


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_map_kernel_resources():
    """pairs_variance_robust_map_kernel<DERIV> is pairs_variance_robust_kernel<DERIV> plus the deposit addresses and
    products of a footprint.  The plan: pairs_variance_robust_kernel's 80 vector registers plus the 13 the deposits cost
    pairs_robust_map_kernel over pairs_robust_kernel, 93, rounded up to the allocation block of 8: at most 96 (five waves per SIMD,
    one fewer than pairs_variance_robust_kernel's six); at most 106 scalar registers, 256 threads, no scratch, no LDS; more vector
    registers than pairs_variance_robust_kernel as built.  Built: 95 (DERIV) and 93 vector registers, 106 scalar."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "32pairs_variance_robust_map_kernel")
    assert len(ks) == 2, sorted(ks)   # DERIV true and false
    plain = mod.find(all_kernels, "28pairs_variance_robust_kernel")
    assert len(plain) == 2, sorted(plain)
    seen = set()
    for name, k in ks.items():
        deriv = "ILb1E" in name
        seen.add(deriv)
        sibling = [w for wname, w in plain.items() if ("ILb1E" in wname) == deriv]
        assert len(sibling) == 1
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 96, (name, k[".vgpr_count"])
        assert k[".vgpr_count"] > sibling[0][".vgpr_count"], (name, k[".vgpr_count"], sibling[0][".vgpr_count"])
        assert k[".sgpr_count"] <= 106, (name, k[".sgpr_count"])
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
    assert seen == {True, False}


def test_reference_and_variances_kernel_resources():
    """pairs_variance_robust_map_reference_kernel<SPLIT>: no scratch; LDS only for the 4 x 5 float64 wave sums of the four-wave form,
    160 bytes (what form_reference_sums declares, as for pairs_variance_robust_reference_kernel).
    variance_robust_map_variances_kernel: nothing.  robust_map_finish_kernel is reused as it is: still one kernel, its 32 x 33 tile."""
    mod, all_kernels = _kernel_resources()
    rs = mod.find(all_kernels, "42pairs_variance_robust_map_reference_kernel")
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
    for mangled, lds in (("24robust_map_finish_kernel", 32 * 33 * 4), ("36variance_robust_map_variances_kernel", 0)):
        ks = mod.find(all_kernels, mangled)
        assert len(ks) == 1, sorted(ks)
        k = list(ks.values())[0]
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == lds and k[".max_flat_workgroup_size"] == 256
