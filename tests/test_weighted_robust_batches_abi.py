"""ecc_metric_evaluate_weighted_robust_pose_deltas / ecc_metric_evaluate_weighted_robust_transforms
(csrc/ecc_weighted_robust_batches.hip, csrc/form_sums_kernel.hip) without a GPU: the header's declarations and its "Not built"
sentence, the symbols and the argument error of a null metric -- checked first, whatever the other arguments are, with nothing written
--, the Python layer's bindings, argument handling and return shapes, the adapter's methods, the build's source list, the host
emulation of the S-column sums (tests/c/form_sums.cpp, also under the address and undefined-behaviour sanitizers) and the resources of
the new kernels as built."""
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
NAMES = ("ecc_metric_evaluate_weighted_robust_pose_deltas", "ecc_metric_evaluate_weighted_robust_transforms")


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def _header():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        return f.read()


def test_header_states_the_calls():
    text = _header()
    assert ("int ecc_metric_evaluate_weighted_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,\n"
            "                                                    const double* moved_Ps, int loss, float delta, double* values, double* coverages,\n"
            "                                                    double* inlier_masses);") in text
    assert ("int ecc_metric_evaluate_weighted_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,\n"
            "                                                   double* values, double* coverages, double* inlier_masses, float* pair_terms);") in text


def test_header_says_what_is_not_built():
    """The new block has its own sentence and says that it supersedes the older blocks', which stay as they were written."""
    text = " ".join(_header().replace("\n *", "\n").split())   # (the comment's line starts are no part of its sentences)
    block = text[text.index("Line weights and the robust loss together, for optimisers"):
                 text.index("int ecc_metric_evaluate_weighted_robust_pose_deltas(")]
    assert "supersedes" in block
    not_built = block[block.index("Not built:"):]
    for what in ("kept base columns", "full-matrices and strided pose forms", "range, group and RCCL forms", "use_corr", "batches of the maps"):
        assert what in not_built, what
    assert "pose-delta and transform batches" not in not_built


def test_library_exports_the_entry_points():
    """A null metric is an argument error, checked first: whatever the other arguments are -- good ones, nulls, a loss outside 0..2, a
    delta that is 0, negative or NaN, negative counts -- and nothing is written."""
    L = _cdll()
    for name in NAMES:
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    vp, f32, adr = C.c_void_p, C.c_float, C.addressof
    poses, transforms = L.ecc_metric_evaluate_weighted_robust_pose_deltas, L.ecc_metric_evaluate_weighted_robust_transforms
    poses.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, f32, vp, vp, vp]
    transforms.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, f32, vp, vp, vp, vp]
    off, views = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 2)(0, 1)
    Ps = (C.c_double * 24)(*([0.0] * 24))
    Ts = (C.c_double * 32)(*([0.0] * 32))
    values, coverages, masses = (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(-1.0, -1.0)
    terms = (C.c_float * 16)(*([-1.0] * 16))
    for loss, delta in ((0, 1.0), (3, 1.0), (-1, 1.0), (1, 0.0), (2, -2.0), (0, float("nan")), (0, float("inf"))):
        for out in ((adr(values), adr(coverages), adr(masses)), (None, None, None), (adr(values), None, None), (None, adr(coverages), adr(masses)),
                    (adr(values), adr(coverages), None), (adr(values), None, adr(masses))):
            for n_poses, lists in ((2, (adr(off), adr(views), adr(Ps))), (2, (None, None, None)), (0, (None, None, None)),
                                   (-1, (adr(off), adr(views), adr(Ps))), (2, (adr(off), None, None))):
                assert poses(None, n_poses, *lists, loss, delta, *out) == ECC_ERR_INVALID_ARGUMENT, (loss, delta, out, n_poses)
                assert b"null" in L.ecc_last_error()
            for ns, K, T in ((1, 2, adr(Ts)), (1, 2, None), (0, 2, adr(Ts)), (1, 0, None), (1, -1, adr(Ts)), (-3, 2, adr(Ts))):
                for t in (adr(terms), None):
                    assert transforms(None, ns, K, T, loss, delta, *out, t) == ECC_ERR_INVALID_ARGUMENT, (loss, delta, out, ns, K)
                    assert b"null" in L.ecc_last_error()
    assert list(values) == [-1.0, -1.0] and list(coverages) == [-1.0, -1.0] and list(masses) == [-1.0, -1.0]   # nothing written
    assert list(terms) == [-1.0] * 16


def test_python_layer_binds_the_calls():
    from epipolarconsistency_amd import _lib, api
    vp, i, f32 = C.c_void_p, C.c_int, C.c_float
    lib = _lib.lib()
    assert lib.ecc_metric_evaluate_weighted_robust_pose_deltas.argtypes == [vp, i, vp, vp, vp, i, f32, vp, vp, vp]
    assert lib.ecc_metric_evaluate_weighted_robust_transforms.argtypes == [vp, i, i, vp, i, f32, vp, vp, vp, vp]
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.evaluate_weighted_robust_pose_deltas).parameters) \
        == list(inspect.signature(M.evaluate_robust_pose_deltas).parameters) == ["self", "moved_views", "moved_Ps", "loss", "delta"]
    assert list(inspect.signature(M.evaluate_weighted_robust_pose_deltas_packed).parameters) \
        == list(inspect.signature(M.evaluate_robust_pose_deltas_packed).parameters) \
        == ["self", "moved_offsets", "moved_views", "moved_Ps", "loss", "delta"]
    assert list(inspect.signature(M.evaluate_weighted_robust_transforms).parameters)[1:] == ["n_source", "Ts", "loss", "delta", "want_pairs"]
    assert inspect.signature(M.evaluate_weighted_robust_transforms).parameters["want_pairs"].default is False


class _NoDevice:
    """The binding's own argument handling: a stand-in whose handle never reaches a metric."""
    _h = None
    _Ps = None

    def __init__(self, n=5):
        self.n = n

    def getNumberOfProjetions(self):
        return self.n

    def evaluate_weighted_robust_pose_deltas_packed(self, *args):
        from epipolarconsistency_amd import api
        return api.MetricRadonIntermediate.evaluate_weighted_robust_pose_deltas_packed(self, *args)


def test_python_layer_checks_shapes_before_the_library():
    """Inconsistent lists and transforms that are no (K, 4, 4) array raise ValueError in the binding; consistent ones reach the library,
    which (handle null) reports its argument error -- the shapes were accepted."""
    from epipolarconsistency_amd import api
    M = api.MetricRadonIntermediate
    P = np.zeros((2, 12))
    for off, views, Ps in (([0, 1], [0, 1], P), ([0, 2], [0, 1], P[:1]), ([], [], P[:0]), ([0, 1, 3], [0, 1], P)):
        with pytest.raises(ValueError):
            M.evaluate_weighted_robust_pose_deltas_packed(_NoDevice(), off, views, Ps, 0, 1.0)
    for bad in (np.zeros((3, 3)), np.zeros((2, 4, 3)), np.zeros(16)):
        with pytest.raises(ValueError):
            M.evaluate_weighted_robust_transforms(_NoDevice(), 2, bad, 0, 1.0)
    for call in (lambda: M.evaluate_weighted_robust_pose_deltas(_NoDevice(), [[1]], [P[:1]], 0, 1.0),
                 lambda: M.evaluate_weighted_robust_pose_deltas_packed(_NoDevice(), [0, 1, 2], [0, 1], P, 2, float("inf")),
                 lambda: M.evaluate_weighted_robust_transforms(_NoDevice(), 2, np.eye(4), 1, 2.5),
                 lambda: M.evaluate_weighted_robust_transforms(_NoDevice(), 2, np.zeros((0, 4, 4)), 1, 2.5, want_pairs=True)):
        with pytest.raises(api.EccError) as e:
            call()
        assert e.value.code == ECC_ERR_INVALID_ARGUMENT


def test_adapter_has_the_methods():
    """Behind evaluateRobustTransforms, single-device only: each throws on a group before anything else and forwards to its C call with
    a coverages vector.  (tests/test_cpp_adapter_weighted_robust_batches.py compiles both branches and runs them.)"""
    with open(os.path.join(PKG, "cpp", "EpipolarConsistencyHip.hxx")) as f:
        text = f.read()
    for method, call in (("evaluateWeightedRobustPoseDeltas", "ecc_metric_evaluate_weighted_robust_pose_deltas"),
                         ("evaluateWeightedRobustTransforms", "ecc_metric_evaluate_weighted_robust_transforms")):
        at = text.index("void %s(" % method)
        body = text[at:text.index("\n    }\n", at)]
        assert 'if (m_gh) throw std::runtime_error("%s: not available on a device group");' % method in body
        assert body.index("if (m_gh) throw") < body.index("values.assign(")       # before anything else
        assert "detail::check(%s(m_h, " % call in body
        assert "int loss, float delta" in body
        assert "std::vector<double>* coverages = 0x0" in body and "std::vector<double>* inlier_masses = 0x0" in body
    assert text.index("void evaluateRobustTransforms(") < text.index("void evaluateWeightedRobustPoseDeltas(") \
        < text.index("void evaluateWeightedRobustTransforms(") < text.index("void evaluateViewHessian(")


def test_source_list_and_flags():
    """The new host file and the new kernel file are in the build's source list; the kernel file is built without the SLP vectoriser,
    as the other sum files are."""
    from epipolarconsistency_amd import build
    assert "ecc_weighted_robust_batches.hip" in build.SOURCES and "form_sums_kernel.hip" in build.SOURCES
    for s in ("form_sums_kernel.hip", "weighted_poses_kernel.hip", "weighted_transforms_kernel.hip", "weighted_robust_kernel.hip", "sum_kernel.hip"):
        assert build.PER_SOURCE_FLAGS.get(s) == ["-fno-slp-vectorize"], s
    for s in ("form_sums_kernel.hip", "ecc_weighted_robust_batches.hip"):
        assert os.path.exists(os.path.join(PKG, "csrc", s)), s


# ---- the sums on the host ------------------------------------------------------------------------------------------------------------
def _build_and_run(tmp_path, name, flags):
    exe = os.path.join(str(tmp_path), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "c", "form_sums.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok: 8 pair counts x 3 columns summed per pose, 15 grids x 3 columns per transform" in r.stdout, r.stdout + r.stderr
    return r


def test_form_sums_on_the_host(tmp_path):
    """The S-column walk and the strided read, thread by thread, against ecc_sum::sum_on_host per column (tests/c/form_sums.cpp says
    what is checked)."""
    _build_and_run(tmp_path, "form_sums", ["-O2"])


def test_form_sums_on_the_host_under_sanitizers(tmp_path):
    """The same program, stand-alone, with -fsanitize=address,undefined: every column is a vector of exactly the needed size, so a read
    past a column's end is found here and not on a GPU."""
    r = _build_and_run(tmp_path, "form_sums_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ---- resources ---------------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_sum_kernel_resources():
    """sum_form_poses_kernel<1 | 16, 3> and sum_form_transforms_kernel<1 | 16, 3>, as built: exactly two instantiations each, no
    scratch, 1024-thread workgroups.
    LDS, the 48 KiB form (a chunk of ecc_sum::THREADS float4 per column):
      poses       49 712 bytes = 3 x 16 384 stage + 3 x 16 tail + 128 moved views + 3 x 128 wave sums -- under 64 KiB, two workgroups
                  per CU;
      transforms  432 bytes = 3 x 16 tail + 3 x 128 wave sums.
    Registers as built: poses 52 vector registers in both forms, 66 / 67 scalar; transforms 65 / 66 vector, 35 / 37 scalar -- pinned at
    the allocation blocks they fall into (poses 56 vector, 72 scalar; transforms 72 vector, 40 scalar; a 1024-thread workgroup may have
    128 vector registers).  The two-column kernels still count two instantiations each."""
    mod, all_kernels = _kernel_resources()
    for part, lds, vgpr, sgpr in (("21sum_form_poses_kernel", 3 * 16384 + 3 * 16 + 128 + 3 * 128, 56, 72),
                                  ("26sum_form_transforms_kernel", 3 * 16 + 3 * 128, 72, 40)):
        ks = mod.find(all_kernels, part)
        assert len(ks) == 2, sorted(ks)
        seen = set()
        for name, k in ks.items():
            assert "ILi1ELi3E" in name or "ILi16ELi3E" in name, name       # S = 3 only
            seen.add("ILi16E" in name)
            print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
            assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
            assert k[".group_segment_fixed_size"] == lds, (name, k[".group_segment_fixed_size"], lds)
            assert k[".max_flat_workgroup_size"] == 1024, name
            assert vgpr - 8 < k[".vgpr_count"] <= vgpr, (name, k[".vgpr_count"])
            assert sgpr - 8 < k[".sgpr_count"] <= sgpr, (name, k[".sgpr_count"])
        assert seen == {True, False}
    fin = mod.find(all_kernels, "23finish_form_sums_kernel")
    assert len(fin) == 1 and list(fin.values())[0][".private_segment_fixed_size"] == 0
    assert len(mod.find(all_kernels, "25sum_weighted_poses_kernel")) == 2
    assert len(mod.find(all_kernels, "30sum_weighted_transforms_kernel")) == 2
