"""ecc_metric_evaluate_weighted_pairs / ecc_metric_evaluate_weighted_pose_deltas (csrc/ecc_weighted_poses.hip,
csrc/weighted_poses_kernel.hip, csrc/ecc_pose_scatter.h) without a GPU: the symbols and the argument errors that return before the
device is touched, the prototypes from C99, the C++ adapter in both branches, the Python layer's shapes and its ValueError on
inconsistent lists, the grid -> all-pairs mapping and the chunked sum's order on the host (tests/c/pose_scatter.cpp), and the
resources of the new sum kernel read from the built library's code object."""
import ctypes as C
import importlib.util
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_OK, ECC_ERR_INVALID_ARGUMENT = 0, 1


def _cdll():
    from epipolarconsistency_amd import _lib
    return C.CDLL(_lib.LIB_PATH)


def test_library_exports_the_entry_points():
    L = _cdll()
    L.ecc_last_error.restype = C.c_char_p
    vp, adr = C.c_void_p, C.addressof
    pairs_call, poses_call = L.ecc_metric_evaluate_weighted_pairs, L.ecc_metric_evaluate_weighted_pose_deltas
    pairs_call.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    poses_call.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    idx = (C.c_int32 * 8)(0, 1, 0, 1, 1, 2, 1, 2)
    off, views = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 2)(0, 1)
    Ps = (C.c_double * 24)(*([0.0] * 24))
    value, coverage = (C.c_double * 1)(-1.0), (C.c_double * 1)(-1.0)
    terms = (C.c_float * 4)(*([-1.0] * 4))
    values, coverages = (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(-1.0, -1.0)
    # a null metric is checked first, whatever else is null or empty
    for args in ((None, adr(idx), 2, adr(value), adr(coverage), adr(terms)), (None, None, 0, None, None, None),
                 (None, adr(idx), 0, adr(value), None, None), (None, None, 2, adr(value), None, None)):
        assert pairs_call(*args) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error(), args
    for args in ((None, 2, adr(off), adr(views), adr(Ps), adr(values), adr(coverages)), (None, 0, None, None, None, None, None),
                 (None, 2, adr(off), None, None, adr(values), None)):
        assert poses_call(*args) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error(), args
    assert value[0] == -1.0 and coverage[0] == -1.0 and list(terms) == [-1.0] * 4   # nothing written
    assert list(values) == [-1.0, -1.0] and list(coverages) == [-1.0, -1.0]


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert ("int ecc_metric_evaluate_weighted_pairs(ecc_metric* m, const int32_t* idx4, int n_pairs, double* value, double* coverage, "
            "float* pair_terms);") in text
    assert ("int ecc_metric_evaluate_weighted_pose_deltas(ecc_metric* m, int n_poses, const int32_t* moved_offsets, "
            "const int32_t* moved_views,\n                                             const double* moved_Ps, double* values, "
            "double* coverages);") in text


def test_python_layer_binds_the_calls():
    from epipolarconsistency_amd import _lib, api
    for name in ("ecc_metric_evaluate_weighted_pairs", "ecc_metric_evaluate_weighted_pose_deltas"):
        assert getattr(_lib.lib(), name).argtypes is not None
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.evaluate_weighted_pairs).parameters)[1:] == ["idx4", "want_pairs"]
    assert inspect.signature(M.evaluate_weighted_pairs).parameters["want_pairs"].default is False
    assert list(inspect.signature(M.evaluate_weighted_pose_deltas).parameters) == list(inspect.signature(M.evaluate_pose_deltas).parameters)
    assert list(inspect.signature(M.evaluate_weighted_pose_deltas_packed).parameters) \
        == list(inspect.signature(M.evaluate_pose_deltas_packed).parameters)


class _NoDevice:
    """The binding's own argument handling: a stand-in whose handle never reaches the library."""
    _h = None
    _Ps = None

    def evaluate_weighted_pose_deltas_packed(self, *args):
        from epipolarconsistency_amd import api
        return api.MetricRadonIntermediate.evaluate_weighted_pose_deltas_packed(self, *args)


def test_python_layer_checks_shapes_before_the_library():
    """Inconsistent lists and a list that is no (n, 4) array raise ValueError in the binding; an empty pose list and an empty index list
    reach the library, which (handle null) reports its argument error -- the shapes were accepted."""
    from epipolarconsistency_amd import api
    M = api.MetricRadonIntermediate
    P = np.zeros((2, 12))
    for off, views, Ps in (([0, 1], [0, 1], P), ([0, 2], [0, 1], P[:1]), ([], [], P[:0]), ([0, 1, 3], [0, 1], P)):
        with pytest.raises(ValueError):
            M.evaluate_weighted_pose_deltas_packed(_NoDevice(), off, views, Ps)
    for bad in (np.zeros((3, 3), np.int32), np.zeros(6, np.int32), np.zeros((1, 2, 4), np.int32)):
        with pytest.raises(ValueError):
            M.evaluate_weighted_pairs(_NoDevice(), bad)
    with pytest.raises(api.EccError) as e:
        M.evaluate_weighted_pose_deltas(_NoDevice(), [[1]], [P[:1]])
    assert e.value.code == ECC_ERR_INVALID_ARGUMENT
    with pytest.raises(api.EccError) as e:
        M.evaluate_weighted_pairs(_NoDevice(), np.zeros((0, 4), np.int32), want_pairs=True)
    assert e.value.code == ECC_ERR_INVALID_ARGUMENT
    # the packing of the per-pose form is the unweighted call's
    off, views, flat = api._pack_pose_lists([[1, 3], [], [2]], [np.ones((2, 12)), np.zeros((0, 12)), [np.arange(12.0).reshape(3, 4)]])
    assert off == [0, 2, 2, 3] and views == [1, 3, 2] and flat.shape == (3, 12)
    assert np.array_equal(flat[2], np.arange(12.0).reshape(3, 4).T.reshape(12))   # column-major per matrix


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_weighted_poses_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_weighted_poses_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "weighted poses abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_weighted_poses")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_poses.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_poses_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_pose_scatter_on_the_host(tmp_path):
    """csrc/ecc_pose_scatter.h compiled for the host: the mapping over n = 2 .. 40 and the chunked substitute-and-add against
    ecc_sum::sum_on_host (tests/c/pose_scatter.cpp says what is checked)."""
    exe = os.path.join(str(tmp_path), "pose_scatter")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "pose_scatter.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok: 39 view counts mapped, 8 pair counts summed" in r.stdout, r.stdout + r.stderr


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_sum_kernel_resources():
    """sum_weighted_poses_kernel<1 | 16>: sum_poses_kernel's staging with two more arguments -- no scratch, LDS at most that kernel's
    plus 64 bytes (built: the same 33 040 bytes: 32 768 stage, 16 tail, 128 moved views, 128 wave sums), one 1024-thread workgroup.
    Registers as built: 36 vector registers in both forms (sum_poses_kernel: 36), 67 / 68 scalar (sum_poses_kernel: 65 / 66) -- pinned
    with the allocation blocks they fall into (40 vector, 72 scalar; a 1024-thread workgroup may have 128 vector registers)."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "25sum_weighted_poses_kernel")
    ref = mod.find(all_kernels, "16sum_poses_kernel")
    assert len(ks) == 2 and len(ref) == 2, (sorted(ks), sorted(ref))
    ref_lds = max(k[".group_segment_fixed_size"] for k in ref.values())
    seen = set()
    for name, k in ks.items():
        seen.add("ILi16E" in name)
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".group_segment_fixed_size"] <= ref_lds + 64, (name, k[".group_segment_fixed_size"], ref_lds)
        assert k[".max_flat_workgroup_size"] == 1024, name
        assert k[".vgpr_count"] <= 40, (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 72, (name, k[".sgpr_count"])
    assert seen == {True, False}
    fin = mod.find(all_kernels, "28finish_weighted_poses_kernel")
    assert len(fin) == 1 and list(fin.values())[0][".private_segment_fixed_size"] == 0
