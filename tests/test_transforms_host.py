"""The host side of ecc_metric_evaluate_transforms (csrc/ecc_transforms.hip; the registration of two scans, ref:
tools/Registration/Registration3D3D.hxx:104-110 `Ps[i] * T_input`): ecc_host_compose_transform is defined operation by
operation -- out[r][c] = ((P[r][0] T[0][c] + P[r][1] T[1][c]) + P[r][2] T[2][c]) + P[r][3] T[3][c], every product and every sum
rounded to binary64 on its own -- so that host, device and tests agree on the bits of the composed matrices.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import geometry_catalog as cat


def _compose_numpy(P, T):
    """The stated order with elementwise float64 operations (not `@`, which may fuse or reorder)."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.empty((3, 4), np.float64)
    for r in range(3):
        for c in range(4):
            p0 = np.float64(P[r, 0]) * np.float64(T[0, c])
            p1 = np.float64(P[r, 1]) * np.float64(T[1, c])
            p2 = np.float64(P[r, 2]) * np.float64(T[2, c])
            p3 = np.float64(P[r, 3]) * np.float64(T[3, c])
            out[r, c] = ((p0 + p1) + p2) + p3
    return out


def _transforms():
    from epipolarconsistency_amd import geometry
    rng = np.random.default_rng(11)
    Ts = [np.eye(4)]
    Ts += [geometry.rigid_transform(rx=a, ry=b, rz=c) for a, b, c in [(0.3, 0, 0), (0, -1.1, 0), (0, 0, 2.7), (0.02, -0.013, 0.4)]]
    Ts += [geometry.rigid_transform(tx=a, ty=b, tz=c) for a, b, c in [(6.0, -3.0, 0.0), (1e-3, 250.0, -77.7), (0, 0, 1e4)]]
    Ts += [geometry.rigid_transform(tx=6, ty=-3, tz=0.5, rx=0.01, ry=-0.02, rz=0.02)]
    H = rng.standard_normal((4, 4)) * np.array([1.0, 1e-3, 1e3, 1.0])  # a general homography, entries of mixed magnitude
    Ts.append(H)
    Ts.append(rng.standard_normal((4, 4)))
    return Ts


@pytest.mark.parametrize("name", cat.NAMES)
def test_compose_transform_has_the_stated_bits(name):
    from epipolarconsistency_amd import geometry
    Ps = cat.make(name, 12)[0]
    for T in _transforms():
        for P in Ps:
            got = geometry.compose_transform(P, T)
            want = _compose_numpy(P, T)
            assert got.shape == (3, 4) and got.dtype == np.float64
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, got - want)


@pytest.mark.parametrize("name", cat.NAMES)
def test_identity_returns_the_matrix_bit_for_bit(name):
    """T = I returns P bit for bit -- with the one exception the stated arithmetic itself makes: an entry that is -0.0 (the
    "mirrored" catalog has two) comes back as +0.0, because (-0.0 * 1 + x * 0) is +0.0 in IEEE arithmetic whatever performs it
    (test_compose_transform_has_the_stated_bits holds the helper to exactly that on the same inputs).  So: equal as numbers
    everywhere, equal bits wherever P is not a negative zero, and a negative zero becomes a positive one."""
    from epipolarconsistency_amd import geometry
    for P in cat.make(name, 12)[0]:
        P = np.ascontiguousarray(P, np.float64)
        got = geometry.compose_transform(P, np.eye(4))
        neg_zero = (P == 0.0) & np.signbit(P)
        assert np.array_equal(got, P)
        assert np.array_equal(got.view(np.uint64)[~neg_zero], P.view(np.uint64)[~neg_zero])
        assert not np.signbit(got[neg_zero]).any()


def test_compose_transform_in_place_and_column_major():
    """The C entry point itself: column-major 12 / 16 doubles; out12 may be P12."""
    from epipolarconsistency_amd import _lib, geometry
    L = _lib.lib()
    P = np.arange(1.0, 13.0).reshape(3, 4) * 0.37
    T = geometry.rigid_transform(tx=1.5, ty=-2.5, tz=0.25, rx=0.1, ry=0.2, rz=0.3)
    buf = np.ascontiguousarray(P.T).reshape(12).copy()
    Tc = np.ascontiguousarray(T.T).reshape(16)
    L.ecc_host_compose_transform(C.c_void_p(buf.ctypes.data), C.c_void_p(Tc.ctypes.data), C.c_void_p(buf.ctypes.data))
    assert np.array_equal(buf.reshape(4, 3).T, _compose_numpy(P, T))


def test_symbols_are_exported_and_bound():
    from epipolarconsistency_amd import _lib
    import epipolarconsistency_amd as E
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("ecc_host_compose_transform", "ecc_metric_evaluate_transforms", "ecc_metric_last_batched_transforms"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert callable(E.MetricRadonIntermediate.evaluate_transforms) and callable(E.MetricRadonIntermediate.last_batched_transforms)
    assert callable(E.geometry.compose_transform)


def test_argument_checks_without_a_device():
    """Null handles are refused with ECC_ERR_INVALID_ARGUMENT and a message before anything touches a device."""
    from epipolarconsistency_amd import _lib
    L = _lib.lib()
    T = np.eye(4).reshape(16)
    means = np.zeros(1)
    rc = L.ecc_metric_evaluate_transforms(None, 1, 1, C.c_void_p(T.ctypes.data), C.c_void_p(means.ctypes.data), None)
    assert rc == 1 and b"null" in L.ecc_last_error()
    v = C.c_int64(7)
    assert L.ecc_metric_last_batched_transforms(None, C.byref(v)) == 1 and b"null" in L.ecc_last_error()


def test_device_code_of_compose_transform_has_no_fused_multiply_add(tmp_path):
    """The device ISA of ecc_host::compose_transform (csrc/ecc_host_geometry.h), compiled for gfx950 on its own so that
    the divisions and square roots of E1 -- which the compiler expands with v_fma_f64 -- do not blur the count: 48 products and 36
    sums, none fused, with the library's -ffp-contract=off and with hipcc's default contraction (the pragma in the function)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(str(tmp_path), "compose_only.hip")
    with open(src, "w") as f:
        f.write('#include <hip/hip_runtime.h>\n#include "ecc_host_geometry.h"\n'
                '__global__ void compose_only(const double* P, const double* T, double* out)\n{\n'
                '    double p[12], t[16], o[12];\n'
                '    for (int q = 0; q < 12; ++q) p[q] = P[12 * threadIdx.x + q];\n'
                '    for (int q = 0; q < 16; ++q) t[q] = T[q];\n'
                '    ecc_host::compose_transform(p, t, o);\n'
                '    for (int q = 0; q < 12; ++q) out[12 * threadIdx.x + q] = o[q];\n}\n')
    for flags in (["-ffp-contract=off"], []):
        asm = os.path.join(str(tmp_path), "compose_only.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17"] + flags +
                           ["-I" + os.path.join(root, "epipolarconsistency_amd", "csrc"), "--cuda-device-only", "-S", src, "-o", asm],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(asm).read()
        assert "fma" not in text.replace("compose_transform", ""), flags
        assert text.count("v_mul_f64") == 48 and text.count("v_add_f64") == 36, (flags, text.count("v_mul_f64"), text.count("v_add_f64"))
