"""ecc_metric_evaluate_weighted_transforms (csrc/ecc_weighted_transforms.hip, csrc/weighted_transforms_kernel.hip,
csrc/ecc_transform_grid.h) without a GPU: the symbol and the argument errors that return before the device is touched, the prototype
from C99, the C++ adapter in both branches, the Python layer's signature and its ValueError on a Ts that is not (K, 4, 4), the
grid's entry rule and the strided sum's order on the host (tests/c/transform_grid.cpp), and the resources of the new sum kernel read
from the built library's code object.  (The errors that need a live metric are in tests/test_gpu_weighted_transforms.py.)"""
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


def test_library_exports_the_entry_point():
    L = _cdll()
    L.ecc_last_error.restype = C.c_char_p
    vp, adr = C.c_void_p, C.addressof
    call = L.ecc_metric_evaluate_weighted_transforms
    call.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    Ts = (C.c_double * 32)(*([1.0 if q % 5 == 0 else 0.0 for q in range(16)] * 2))
    values, coverages = (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(-1.0, -1.0)
    terms = (C.c_float * 8)(*([-1.0] * 8))
    # a null metric is checked first, whatever else is null, negative, empty or out of range
    for args in ((None, 1, 2, adr(Ts), adr(values), adr(coverages), adr(terms)), (None, 1, 0, None, None, None, None),
                 (None, 1, -1, adr(Ts), adr(values), None, None), (None, 1, 2, None, adr(values), None, None),
                 (None, 1, 2, adr(Ts), None, None, None), (None, 0, 2, adr(Ts), adr(values), None, None),
                 (None, -3, 2, adr(Ts), adr(values), adr(coverages), None)):
        assert call(*args) == ECC_ERR_INVALID_ARGUMENT and b"metric is null" in L.ecc_last_error(), args
    assert list(values) == [-1.0, -1.0] and list(coverages) == [-1.0, -1.0] and list(terms) == [-1.0] * 8   # nothing written


def test_header_states_the_call():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    assert ("int ecc_metric_evaluate_weighted_transforms(ecc_metric* m, int n_source, int n_transforms, const double* Ts, double* values,\n"
            "                                            double* coverages, float* pair_terms);") in text
    # the calls this one completes no longer list it as missing
    assert "the transform form" not in text


def test_python_layer_binds_the_call():
    from epipolarconsistency_amd import _lib, api
    assert _lib.lib().ecc_metric_evaluate_weighted_transforms.argtypes is not None
    assert len(_lib.SIGNATURES["ecc_metric_evaluate_weighted_transforms"][1]) == 7
    M = api.MetricRadonIntermediate
    sig = inspect.signature(M.evaluate_weighted_transforms)
    assert list(sig.parameters) == list(inspect.signature(M.evaluate_transforms).parameters) == ["self", "n_source", "Ts", "want_pairs"]
    assert sig.parameters["want_pairs"].default is False


class _NoDevice:
    """The binding's own argument handling: a stand-in whose handle never reaches a device."""
    _h = None
    _Ps = None

    def getNumberOfProjetions(self):
        return 0


def test_python_layer_checks_shapes_before_the_library():
    """A Ts that is not (K, 4, 4) (or one (4, 4) matrix) raises ValueError in the binding; a well-shaped one reaches the library, which
    (handle null) reports its argument error -- the shape was accepted."""
    from epipolarconsistency_amd import api
    M = api.MetricRadonIntermediate
    for bad in (np.zeros((3, 3)), np.zeros(16), np.zeros((2, 4, 3)), np.zeros((1, 2, 4, 4)), np.zeros((2, 16))):
        with pytest.raises(ValueError):
            M.evaluate_weighted_transforms(_NoDevice(), 1, bad)
    for good in (np.eye(4), np.zeros((2, 4, 4)), [np.eye(4)] * 3, np.zeros((0, 4, 4))):
        with pytest.raises(api.EccError) as e:
            M.evaluate_weighted_transforms(_NoDevice(), 1, good, want_pairs=True)
        assert e.value.code == ECC_ERR_INVALID_ARGUMENT


def test_prototype_is_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_weighted_transforms_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_weighted_transforms_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "weighted transforms abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_weighted_transforms")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_transforms.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C call and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_transforms_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_transform_grid_on_the_host(tmp_path):
    """csrc/ecc_transform_grid.h compiled for the host: the entry rule against the list kernel's statement, and the strided
    gather-and-add against ecc_sum::sum_on_host of the transposed column, bit for bit, over count in {1, 6, 506, 529, 2 211, 4 160,
    32 942} x K in {1, 5, 9} (tests/c/transform_grid.cpp says what is checked)."""
    exe = os.path.join(str(tmp_path), "transform_grid")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "transform_grid.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok: 21 grids, every transform's two forms summed" in r.stdout, r.stdout + r.stderr


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
    """sum_weighted_transforms_kernel<1 | 16>: sum_transforms_kernel reading K floats apart -- no scratch, one 1024-thread workgroup,
    144 bytes of LDS (128 wave sums + the 16 of the tail; sum_transforms_kernel: 128).  Registers as built: 31 vector registers in
    both forms (sum_transforms_kernel: 22; the four strided addresses), 34 scalar -- pinned with the allocation blocks they fall into
    (32 vector: blocks of 8; 40 scalar: blocks of 8; a 1024-thread workgroup may have 128 vector registers)."""
    mod, all_kernels = _kernel_resources()
    ks = mod.find(all_kernels, "30sum_weighted_transforms_kernel")
    assert len(ks) == 2, sorted(ks)
    seen = set()
    for name, k in ks.items():
        seen.add("ILi16E" in name)
        print(name, k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".group_segment_fixed_size"] == 144, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 1024, name
        assert k[".vgpr_count"] <= 32, (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 40, (name, k[".sgpr_count"])
    assert seen == {True, False}
    fin = mod.find(all_kernels, "33finish_weighted_transforms_kernel")
    assert len(fin) == 1 and list(fin.values())[0][".private_segment_fixed_size"] == 0
