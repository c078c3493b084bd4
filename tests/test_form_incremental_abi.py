"""ecc_metric_set_form_incremental / ecc_metric_last_form_base_pairs (csrc/ecc_form_base.h, csrc/ecc_form_call.h,
csrc/form_base_scatter_kernel.hip) without a GPU: the symbols and their argument errors, the prototypes from C99, the
adapter's two methods in both of its branches, the Python layer, the header's contract, and -- as a stand-alone program under
AddressSanitizer and UBSan, tests/c/form_base.cpp -- the decision between miss, hit and refresh and the position rule the copy kernel
scatters by.  (What the mode computes is tests/test_gpu_form_incremental.py's.)"""
import ctypes as C
import inspect
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")
ECC_ERR_INVALID_ARGUMENT = 1
NAMES = ("ecc_metric_set_form_incremental", "ecc_metric_last_form_base_pairs")


def test_library_exports_the_entry_points():
    """Both symbols are exported and listed in _lib.SIGNATURES; a null metric -- and a null result pointer -- is an argument error with
    a message, and nothing is written.  No device is needed."""
    from epipolarconsistency_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES["ecc_metric_set_form_incremental"] == (i, [vp, i])
    assert _lib.SIGNATURES["ecc_metric_last_form_base_pairs"] == (i, [vp, C.POINTER(i64)])
    for name in NAMES:
        assert hasattr(L, name), name
    L.ecc_last_error.restype = C.c_char_p
    L.ecc_metric_set_form_incremental.argtypes = [vp, i]
    L.ecc_metric_last_form_base_pairs.argtypes = [vp, vp]
    for enable in (0, 1, -3, 7):
        assert L.ecc_metric_set_form_incremental(None, enable) == ECC_ERR_INVALID_ARGUMENT
        assert b"metric is null" in L.ecc_last_error()
    pairs = i64(-7)
    assert L.ecc_metric_last_form_base_pairs(None, C.addressof(pairs)) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
    assert L.ecc_metric_last_form_base_pairs(None, None) == ECC_ERR_INVALID_ARGUMENT and b"null" in L.ecc_last_error()
    assert pairs.value == -7
    # through the binding's own argument types
    lib = _lib.lib()
    assert lib.ecc_metric_set_form_incremental(None, 1) == ECC_ERR_INVALID_ARGUMENT
    assert lib.ecc_metric_last_form_base_pairs(None, C.byref(pairs)) == ECC_ERR_INVALID_ARGUMENT and pairs.value == -7


def test_header_states_the_contract():
    with open(os.path.join(ROOT, "include", "ecc_hip.h")) as f:
        raw = f.read()
    text = " ".join(raw.replace("\n *", "\n").split())
    for proto in ("int ecc_metric_set_form_incremental(ecc_metric* m, int enable);",
                  "int ecc_metric_last_form_base_pairs(const ecc_metric* m, int64_t* pairs);"):
        assert proto in text, proto
    block = text[text.index("The form batches' base columns kept between pose-delta calls"):text.index("int ecc_metric_set_form_incremental(")]
    for phrase in ("default off", "This block supersedes", "miss", "hit", "refresh", "NOTHING IS EVER KEPT", "ECC_SAMPLING_REFERENCE",
                   "min(ECC_POSE_BATCH_MAX_MOVED, n_views / 4)", "the automatic object radius moved with it",
                   "HAS THE BITS OF THE SAME CALL WITH THE MODE OFF", "ecc_metric_refresh_dtrs", "ecc_metric_set_params",
                   "ecc_metric_set_sampling", "ecc_debug_set_poly_tolerance", "a change of n_views", "other_bytes",
                   "c (n - 1) - c (c - 1) / 2", "0 on a hit", "ecc_metric_set_pose_batching(m, 0)", "Not built:"):
        assert phrase in block, phrase
    # the older blocks stand as they were written
    assert raw.count("kept base columns") >= 6


def test_python_layer_binds_the_calls():
    from epipolarconsistency_amd import _lib, api
    for name in NAMES:
        assert getattr(_lib.lib(), name).restype is C.c_int
    M = api.MetricRadonIntermediate
    assert list(inspect.signature(M.setFormIncremental).parameters) == ["self", "enable"]
    assert inspect.signature(M.setFormIncremental).parameters["enable"].default is True
    assert list(inspect.signature(M.last_form_base_pairs).parameters) == ["self"]
    src = inspect.getsource(M.last_form_base_pairs)
    assert "_last_count(_lib.lib().ecc_metric_last_form_base_pairs, self._h)" in src
    # a stand-in library: the switch passes 0 / 1 and returns the metric itself, like setPoseBatching
    calls = []

    class _Lib:
        def ecc_metric_set_form_incremental(self, h, enable):
            calls.append((h, enable))
            return 0

        def ecc_metric_last_form_base_pairs(self, h, ref):
            ref._obj.value = 54
            return 0
    keep = api._lib.lib
    try:
        api._lib.lib = lambda: _Lib()
        m = object.__new__(M)
        m._h = "handle"
        assert m.setFormIncremental() is m and m.setFormIncremental(False) is m and m.setFormIncremental(enable=2) is m
        assert calls == [("handle", 1), ("handle", 0), ("handle", 1)]
        assert m.last_form_base_pairs() == 54
    finally:
        api._lib.lib = keep
        m._h = None


def test_prototypes_are_c99(tmp_path):
    exe = os.path.join(str(tmp_path), "test_form_incremental_abi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "test_form_incremental_abi.c"), "-o", exe, "-L" + PKG, "-lecc_hip", "-lm", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "form incremental abi ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def _syntax(*more):
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", *more, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_form_incremental_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_adapter_eigen_branch_is_well_formed():
    _syntax("-DECC_TEST_MOCK_EIGEN", "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"))


def test_adapter_plain_branch_is_well_formed():
    _syntax("-DECC_TEST_PLAIN_BRANCH")


def test_adapter_has_the_methods():
    """Beside the other switches; the switch goes through push_params on a single-device metric, the counter reads 0 on a group."""
    with open(os.path.join(PKG, "cpp", "EpipolarConsistencyHip.hxx")) as f:
        text = f.read()
    assert "MetricRadonIntermediate& setFormIncremental(bool on = true) { form_incremental = on ? 1 : 0; push_params(); return *this; }" in text
    assert "if (form_incremental >= 0) detail::check(ecc_metric_set_form_incremental(m_h, form_incremental));" in text
    at = text.index("long long lastFormBasePairs() const")
    assert "if (m_h && !m_gh) detail::check(ecc_metric_last_form_base_pairs(m_h, &v));" in text[at:text.index("\n    }\n", at)]


def test_decision_and_positions_are_clean_under_the_sanitizers(tmp_path):
    """csrc/ecc_form_base.h and csrc/ecc_pose_scatter.h built alone into tests/c/form_base.cpp (its own main, no HIP, no library) with
    -fsanitize=address,undefined and run directly: nothing kept -> miss; identical -> hit; one, two and the limit's number of changed
    views -> refresh with exactly those views, ascending; limit + 1 -> miss; each single key field -> miss; REFERENCE -> miss and
    nothing kept; and for n = 12 and the changed sets {0}, {11}, {0, 11}, {3, 4, 5} the non-hole grid entries map one-to-one onto
    exactly the pairs that contain a changed view."""
    exe = os.path.join(str(tmp_path), "form_base")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "c", "form_base.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "form base ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])


def test_source_list_and_kernel_resources():
    """The copy kernel and the decision header are in the build's lists; the kernel as built: no scratch, no LDS beyond the changed
    views (32 ints), no spills -- read from the built library's code object."""
    import importlib.util
    import msgpack  # noqa: F401  (scripts/kernel_resources.py decodes the AMDGPU metadata notes with it; missing: a failure)
    from epipolarconsistency_amd import build
    assert "form_base_scatter_kernel.hip" in build.SOURCES and "ecc_form_base.h" in build.HEADERS
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = os.path.join(PKG, "libecc_hip.so")
    assert os.path.exists(lib), "libecc_hip.so not built"
    mine = mod.find(mod.kernels(lib), "form_base_scatter_kernel")
    assert len(mine) == 1, sorted(mine)
    for name, k in mine.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".group_segment_fixed_size"] == 32 * 4, (name, k[".group_segment_fixed_size"])
        assert k[".vgpr_count"] <= 32 and k[".max_flat_workgroup_size"] == 256, (name, k[".vgpr_count"])
