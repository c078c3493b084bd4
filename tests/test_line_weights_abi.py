"""The device-made line weights (csrc/ecc_line_weights.hip, csrc/line_weights_kernel.hip) without a GPU: the four symbols and their
argument errors in order, the config caps on each of the three calls, the prototypes from C99, the C++ adapter's lineWeights, the
Python layer, and the resources of the two kernels as DESIGN.md 4.18 states them -- read from the built library's code object."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1

PROTOTYPES = """
typedef struct ecc_line_weights_config { int32_t dilate_px; int32_t guard_bins; float zero_at_px; } ecc_line_weights_config;
void ecc_line_weights_defaults(ecc_line_weights_config* cfg);
int ecc_radon_line_weights(ecc_ctx* ctx, const float* flagged, int on_device, int n, int n_u, int n_v,
                           int n_alpha, int n_t, const ecc_line_weights_config* cfg, ecc_dtr** out);
int ecc_radon_line_weights_into(ecc_ctx* ctx, const float* flagged_d, int n, int n_u, int n_v,
                                int n_alpha, int n_t, const ecc_line_weights_config* cfg, float* slabs_d);
int ecc_dtr_line_weights(ecc_ctx* ctx, const ecc_dtr* lengths, const ecc_line_weights_config* cfg, ecc_dtr** out);
"""


class Config(C.Structure):
    _fields_ = [("dilate_px", C.c_int32), ("guard_bins", C.c_int32), ("zero_at_px", C.c_float)]


def _cdll():
    from epipolarconsistency_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    vp, i = C.c_void_p, C.c_int
    L.ecc_last_error.restype = C.c_char_p
    L.ecc_line_weights_defaults.restype = None
    L.ecc_line_weights_defaults.argtypes = [vp]
    L.ecc_radon_line_weights.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp]
    L.ecc_radon_line_weights_into.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    L.ecc_dtr_line_weights.argtypes = [vp, vp, vp, vp]
    return L


def test_defaults():
    L = _cdll()
    cfg = Config(7, 7, 7.0)
    L.ecc_line_weights_defaults(C.byref(cfg))
    assert (cfg.dilate_px, cfg.guard_bins, cfg.zero_at_px) == (0, 1, 1.0)
    L.ecc_line_weights_defaults(None)   # tolerated


def test_null_context_first_and_nothing_written():
    L = _cdll()
    adr = C.addressof
    image = (C.c_float * 4)(0.0, 1.0, 0.0, 0.0)
    slab = (C.c_float * 8)(*([-1.0] * 8))
    out = (C.c_void_p * 2)(0x1234, 0x1234)
    cfg = Config(0, 1, 1.0)
    calls = [lambda *a: L.ecc_radon_line_weights(None, *a), lambda *a: L.ecc_radon_line_weights_into(None, *a), lambda *a: L.ecc_dtr_line_weights(None, *a)]
    good = [(adr(image), 0, 1, 2, 2, 4, 4, adr(cfg), adr(out)), (adr(image), 1, 2, 2, 4, 4, adr(cfg), adr(slab)), (adr(image), adr(cfg), adr(out))]
    null = [(None, 0, 0, 0, 0, 0, 0, None, None), (None, 0, 0, 0, 0, 0, None, None), (None, None, None)]
    for call, a, b in zip(calls, good, null):
        for args in (a, b):
            assert call(*args) == ECC_ERR_INVALID_ARGUMENT
            assert b"context is null" in L.ecc_last_error(), L.ecc_last_error()   # whatever else is wrong: the context is named
    assert list(slab) == [-1.0] * 8 and list(out) == [0x1234, 0x1234]


def test_null_arguments_ranges_and_caps_on_every_call():
    """Behind the null context: null images / outputs / slabs, check_radon_args' ranges, then the config's caps -- each with a
    message of its own, before anything is launched, allocated or written.  None of these checks reads the context, so a block of
    zeros stands in for one here (no device is needed; the same checks run with a real context in tests/test_gpu_line_weights.py)."""
    L = _cdll()
    adr = C.addressof
    ctx = (C.c_char * 4096)()
    fake_dtr = (C.c_char * 4096)()
    image = (C.c_float * 4)(0.0, 1.0, 0.0, 0.0)
    slab = (C.c_float * 8)(*([-1.0] * 8))
    out = (C.c_void_p * 2)(0x1234, 0x1234)
    ok = Config(0, 1, 1.0)

    def stack(image=adr(image), n=1, n_u=2, n_v=2, n_alpha=4, n_t=4, cfg=ok, out=adr(out)):
        return L.ecc_radon_line_weights(adr(ctx), image, 0, n, n_u, n_v, n_alpha, n_t, C.byref(cfg), out)

    def into(image=adr(image), n=1, n_u=2, n_v=2, n_alpha=4, n_t=4, cfg=ok, out=adr(slab)):
        return L.ecc_radon_line_weights_into(adr(ctx), image, n, n_u, n_v, n_alpha, n_t, C.byref(cfg), out)

    def from_lengths(cfg=ok, lengths=adr(fake_dtr), out=adr(out)):
        return L.ecc_dtr_line_weights(adr(ctx), lengths, C.byref(cfg), out)

    def refused(rc, word):
        assert rc == ECC_ERR_INVALID_ARGUMENT and word in L.ecc_last_error(), (rc, word, L.ecc_last_error())

    for call in (stack, into):
        refused(call(image=None), b"flagged")
        refused(call(out=None), b"output")
        refused(call(n=0), b"batch size")
        refused(call(n=65536), b"batch size")
        refused(call(n_u=1), b"image size")
        refused(call(n_v=16385), b"image size")
        refused(call(n_alpha=0), b"bin counts")
        refused(call(n_t=16385), b"bin counts")
    refused(from_lengths(lengths=None), b"length intermediate")
    refused(from_lengths(out=None), b"output")
    nan, inf = float("nan"), float("inf")
    for call in (stack, into, from_lengths):
        for cfg, word in ((Config(-1, 1, 1.0), b"dilate_px"), (Config(17, 1, 1.0), b"dilate_px"), (Config(0, -1, 1.0), b"guard_bins"),
                          (Config(0, 9, 1.0), b"guard_bins"), (Config(0, 1, 0.0), b"zero_at_px"), (Config(0, 1, -1.0), b"zero_at_px"),
                          (Config(0, 1, nan), b"zero_at_px"), (Config(0, 1, inf), b"zero_at_px")):
            refused(call(cfg=cfg), word)
    assert list(slab) == [-1.0] * 8 and list(out) == [0x1234, 0x1234]
    assert bytes(ctx) == bytes(4096) and bytes(fake_dtr) == bytes(4096)


def test_header_states_the_calls():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        text = f.read()
    for line in PROTOTYPES.strip().split(";\n"):
        line = line.strip().rstrip(";") + ";"
        if line.startswith("typedef"):
            assert line in text, line
        else:
            assert re.sub(r"\s+", " ", line) in re.sub(r"\s+", " ", text), line
    assert PROTOTYPES.strip().split("\n", 2)[2].strip() in text   # the three calls, verbatim with their line breaks


def test_python_layer_binds_the_calls():
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import _lib, api
    for name in ("ecc_line_weights_defaults", "ecc_radon_line_weights", "ecc_radon_line_weights_into", "ecc_dtr_line_weights"):
        assert getattr(_lib.lib(), name).argtypes is not None and name in _lib.SIGNATURES
    assert [f[0] for f in _lib.LineWeightsConfig._fields_] == ["dilate_px", "guard_bins", "zero_at_px"] and C.sizeof(_lib.LineWeightsConfig) == 12
    sig = inspect.signature(api.line_weights_device)
    assert list(sig.parameters) == ["ctx", "flagged", "size_alpha", "size_t", "zero_at_px", "guard_bins", "dilate_px", "out"]
    assert [sig.parameters[k].default for k in ("zero_at_px", "guard_bins", "dilate_px", "out")] == [1.0, 1, 0, None]
    assert E.line_weights_device is api.line_weights_device and "line_weights_device" in E.__all__
    sig = inspect.signature(api.RadonIntermediate.line_weights_from)
    assert list(sig.parameters)[:3] == ["lengths_dtr", "zero_at_px", "guard_bins"]
    assert [sig.parameters[k].default for k in ("zero_at_px", "guard_bins")] == [1.0, 1]
    # the existing door is as it was
    assert list(inspect.signature(api.line_weights).parameters) == ["ctx", "flagged", "size_alpha", "size_t", "zero_at_px", "guard_bins"]


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_line_weights_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_line_weights_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "line weights abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_adapter_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_line_weights")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_line_weights.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_is_well_formed():
    """lineWeights takes no matrix, but it sits in a class whose other members switch on Eigen: the same source under the mock."""
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_line_weights.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- resources ---------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    return mod, mod.kernels(lib)


def test_kernel_resources():
    """16 x 64 outputs per 256-thread workgroup; LDS = the loaded tile with its halo plus the row pass's result, sized
    for the caps -- dilate_max_kernel: halo 16, (48 x 96 + 48 x 64) floats = 30720 bytes, five workgroups per CU; clip_min_kernel:
    halo 8 + 1 border position, (34 x 82 + 34 x 64) floats = 19856 bytes, eight workgroups per CU.  No scratch; few enough registers
    for eight waves per SIMD, so that the LDS alone sets the occupancy."""
    mod, all_kernels = _kernel_resources()
    for name, lds in (("17dilate_max_kernel", 4 * (48 * 96 + 48 * 64)), ("15clip_min_kernel", 4 * (34 * 82 + 34 * 64))):
        ks = mod.find(all_kernels, name)
        assert len(ks) == 1, (name, sorted(ks))
        k = list(ks.values())[0]
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".group_segment_fixed_size"] == lds, (name, k[".group_segment_fixed_size"])
        assert k[".max_flat_workgroup_size"] == 256, name
        assert k[".vgpr_count"] <= 64, (name, k[".vgpr_count"])
        assert k[".sgpr_count"] <= 96, (name, k[".sgpr_count"])
    assert (4 * (48 * 96 + 48 * 64), 4 * (34 * 82 + 34 * 64)) == (30720, 19856)
