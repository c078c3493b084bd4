"""ecc_metric_evaluate_robust_pose_deltas / ecc_metric_evaluate_robust_transforms (csrc/ecc_robust_batches.hip) without a GPU: the
header's declarations, the symbols and the argument error of a null metric -- checked first, whatever the other arguments are, with
nothing written --, the Python layer's bindings, argument handling and return shapes, the adapter's methods, and the "Not built"
sentences of the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1
NAMES = ("ecc_metric_evaluate_robust_pose_deltas", "ecc_metric_evaluate_robust_transforms")


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def _header():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        return f.read()


def test_header_states_the_calls():
    text = _header()
    assert ("int ecc_metric_evaluate_robust_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, const int32_t* moved_views,\n"
            "                                           const double* moved_Ps, int loss, float delta, double* values, double* inlier_masses);") in text
    assert ("int ecc_metric_evaluate_robust_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, int loss, float delta,\n"
            "                                          double* values, double* inlier_masses, float* pair_terms);") in text


def test_header_says_what_is_not_built():
    """The robust block no longer lists the pose-delta and transform forms as missing; the new block lists what it leaves out."""
    text = " ".join(_header().replace("\n *", "\n").split())   # (the comment's line starts are no part of its sentences)
    for sentence in re.findall(r"Not built:[^/]*?\*/", text):
        assert "pose-delta, transform" not in sentence, sentence
    block = text[text.index("The robust loss for optimisers"):text.index("int ecc_metric_evaluate_robust_pose_deltas(")]
    not_built = block[block.index("Not built:"):]
    for what in ("kept base columns", "full-matrices and strided pose forms", "range, group and RCCL forms", "combined with line weights",
                 "under use_corr"):
        assert what in not_built, what


def test_library_exports_the_entry_points():
    """A null metric is an argument error, checked first: whatever the other arguments are -- good ones, nulls, a loss outside 0..2, a
    delta that is 0, negative or NaN, negative counts -- and nothing is written."""
    L = _cdll()
    for name in NAMES:
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    vp, f32, adr = C.c_void_p, C.c_float, C.addressof
    poses, transforms = L.ecc_metric_evaluate_robust_pose_deltas, L.ecc_metric_evaluate_robust_transforms
    poses.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, f32, vp, vp]
    transforms.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, f32, vp, vp, vp]
    off, views = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 2)(0, 1)
    Ps = (C.c_double * 24)(*([0.0] * 24))
    Ts = (C.c_double * 32)(*([0.0] * 32))
    values, masses = (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(-1.0, -1.0)
    terms = (C.c_float * 12)(*([-1.0] * 12))
    for loss, delta in ((0, 1.0), (3, 1.0), (-1, 1.0), (1, 0.0), (2, -2.0), (0, float("nan")), (0, float("inf"))):
        for out in ((adr(values), adr(masses)), (None, None), (adr(values), None), (None, adr(masses))):
            for n_poses, lists in ((2, (adr(off), adr(views), adr(Ps))), (2, (None, None, None)), (0, (None, None, None)),
                                   (-1, (adr(off), adr(views), adr(Ps))), (2, (adr(off), None, None))):
                assert poses(None, n_poses, *lists, loss, delta, *out) == ECC_ERR_INVALID_ARGUMENT, (loss, delta, out, n_poses)
                assert b"null" in L.ecc_last_error()
            for ns, K, T in ((1, 2, adr(Ts)), (1, 2, None), (0, 2, adr(Ts)), (1, 0, None), (1, -1, adr(Ts)), (-3, 2, adr(Ts))):
                for t in (adr(terms), None):
                    assert transforms(None, ns, K, T, loss, delta, *out, t) == ECC_ERR_INVALID_ARGUMENT, (loss, delta, out, ns, K)
                    assert b"null" in L.ecc_last_error()
    assert list(values) == [-1.0, -1.0] and list(masses) == [-1.0, -1.0] and list(terms) == [-1.0] * 12   # nothing written


def test_python_layer_binds_the_calls():
    from epipolarconsistency_amd import _lib, api
    vp, i, f32 = C.c_void_p, C.c_int, C.c_float
    lib = _lib.lib()
    assert lib.ecc_metric_evaluate_robust_pose_deltas.argtypes == [vp, i, vp, vp, vp, i, f32, vp, vp]
    assert lib.ecc_metric_evaluate_robust_transforms.argtypes == [vp, i, i, vp, i, f32, vp, vp, vp]
    for name in NAMES:
        assert getattr(lib, name).restype is C.c_int
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.evaluate_robust_pose_deltas).parameters) \
        == list(inspect.signature(M.evaluate_weighted_pose_deltas).parameters) + ["loss", "delta"]
    assert list(inspect.signature(M.evaluate_robust_pose_deltas_packed).parameters) \
        == list(inspect.signature(M.evaluate_weighted_pose_deltas_packed).parameters) + ["loss", "delta"]
    assert list(inspect.signature(M.evaluate_robust_transforms).parameters)[1:] == ["n_source", "Ts", "loss", "delta", "want_pairs"]
    assert inspect.signature(M.evaluate_robust_transforms).parameters["want_pairs"].default is False


class _NoDevice:
    """The binding's own argument handling: a stand-in whose handle never reaches a metric."""
    _h = None
    _Ps = None

    def __init__(self, n=5):
        self.n = n

    def getNumberOfProjetions(self):
        return self.n

    def evaluate_robust_pose_deltas_packed(self, *args):
        from epipolarconsistency_amd import api
        return api.MetricRadonIntermediate.evaluate_robust_pose_deltas_packed(self, *args)


def test_python_layer_checks_shapes_before_the_library():
    """Inconsistent lists and transforms that are no (K, 4, 4) array raise ValueError in the binding; consistent ones reach the library,
    which (handle null) reports its argument error -- the shapes were accepted."""
    from epipolarconsistency_amd import api
    M = api.MetricRadonIntermediate
    P = np.zeros((2, 12))
    for off, views, Ps in (([0, 1], [0, 1], P), ([0, 2], [0, 1], P[:1]), ([], [], P[:0]), ([0, 1, 3], [0, 1], P)):
        with pytest.raises(ValueError):
            M.evaluate_robust_pose_deltas_packed(_NoDevice(), off, views, Ps, 0, 1.0)
    for bad in (np.zeros((3, 3)), np.zeros((2, 4, 3)), np.zeros(16)):
        with pytest.raises(ValueError):
            M.evaluate_robust_transforms(_NoDevice(), 2, bad, 0, 1.0)
    for call in (lambda: M.evaluate_robust_pose_deltas(_NoDevice(), [[1]], [P[:1]], 0, 1.0),
                 lambda: M.evaluate_robust_pose_deltas_packed(_NoDevice(), [0, 1, 2], [0, 1], P, 2, float("inf")),
                 lambda: M.evaluate_robust_transforms(_NoDevice(), 2, np.eye(4), 1, 2.5),
                 lambda: M.evaluate_robust_transforms(_NoDevice(), 2, np.zeros((0, 4, 4)), 1, 2.5, want_pairs=True)):
        with pytest.raises(api.EccError) as e:
            call()
        assert e.value.code == ECC_ERR_INVALID_ARGUMENT


def test_adapter_has_the_methods():
    """Beside evaluateWeightedPoseDeltas / evaluateWeightedTransforms, single-device only: each throws on a group before anything else.
    (tests/test_cpp_adapter_robust_batches.py compiles both branches and runs them.)"""
    with open(os.path.join(PKG, "cpp", "EpipolarConsistencyHip.hxx")) as f:
        text = f.read()
    for method, call in (("evaluateRobustPoseDeltas", "ecc_metric_evaluate_robust_pose_deltas"),
                         ("evaluateRobustTransforms", "ecc_metric_evaluate_robust_transforms")):
        at = text.index("void %s(" % method)
        body = text[at:text.index("\n    }\n", at)]
        assert 'if (m_gh) throw std::runtime_error("%s: not available on a device group");' % method in body
        assert "detail::check(%s(m_h, " % call in body
        assert "int loss, float delta" in body
    assert text.index("void evaluateWeightedTransforms(") < text.index("void evaluateRobustPoseDeltas(") < text.index("void evaluateRobustTransforms(")


def test_source_list_and_flags():
    """The new host file is in the build's source list; every device file the feature touches is built without the SLP vectoriser."""
    from epipolarconsistency_amd import build
    assert "ecc_robust_batches.hip" in build.SOURCES
    for s in ("weighted_poses_kernel.hip", "weighted_transforms_kernel.hip", "robust_kernel.hip"):
        assert build.PER_SOURCE_FLAGS.get(s) == ["-fno-slp-vectorize"], s
