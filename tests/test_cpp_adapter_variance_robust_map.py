"""evaluateVarianceRobustMap, evaluateVarianceRobustMapPairs and varianceRobustMapVariances of the header-only C++ adapter
(epipolarconsistency_amd/cpp/EpipolarConsistencyHip.hxx), in the manner of tests/test_cpp_adapter_weighted_robust_map.py: the
non-Eigen branch compiled and linked with g++ -Wall -Werror; on the GPU the methods return what
ecc_metric_evaluate_variance_robust_map[_pairs] and ecc_metric_variance_robust_map_variances return for the same arguments."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")


def _build(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_variance_robust_map")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_variance_robust_map.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_adapter_variance_robust_map_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # without arguments the driver checks the argument errors of the C calls and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_adapter_members_throw_on_a_group():
    """Single-device only: each member throws on a group before anything else and then makes its C call."""
    with open(os.path.join(PKG, "cpp", "EpipolarConsistencyHip.hxx")) as f:
        text = f.read()
    for head, method, call in (("double evaluateVarianceRobustMap(int loss, float delta, float floor, const std::vector<int>& views,",
                                "evaluateVarianceRobustMap", "ecc_metric_evaluate_variance_robust_map(m_h, loss, delta, floor,"),
                               ("double evaluateVarianceRobustMapPairs(const std::vector<int>& indices, int loss, float delta, float floor,",
                                "evaluateVarianceRobustMapPairs", "ecc_metric_evaluate_variance_robust_map_pairs(m_h, "),
                               ("std::vector<RadonIntermediate*> varianceRobustMapVariances(float floor, float min_hits = 1.0f, float gain = 1.0f, "
                                "float max_factor = 1e4f)", "varianceRobustMapVariances",
                                "ecc_metric_variance_robust_map_variances(m_h, floor, min_hits, gain, max_factor,")):
        at = text.index(head)
        body = text[at:text.index("\n    }\n", at)]
        first = body[body.index("{") + 1:].strip()
        assert first.startswith('if (m_gh) throw std::runtime_error("%s: not available on a device group");' % method), method   # the first statement
        assert body.index("if (m_gh) throw") < body.index("detail::check(" + call)


@pytest.mark.gpu
def test_adapter_returns_what_the_c_calls_return(tmp_path, gpu_ctx):
    """Eight views of the small scan with DESIGN.md 4.30's noise and block, intermediates and variance fields computed by the adapter,
    delta = varianceRobustScale(rows at infinity, 2.0); on the 2 n metric, each of the three losses: every view, two unordered views
    with only the REJ planes, and a list of three pairs -- values, mean weights, inlier masses, planes and pair terms of the
    adapter's methods against the C calls on a second metric over the same intermediates, bit for bit; the variance fields of the
    held map against the C call's, read back."""
    import epipolarconsistency_amd as E
    import variance_robust_terms as VR
    import variance_terms as V
    from conftest import make_small_scan
    exe = _build(tmp_path)
    Ps, imgs = make_small_scan()
    _, both, var = VR.demo_images(imgs)
    var_d = E.variance_intermediates(gpu_ctx, var, 96, 96)
    floor = E.variance_floor(var_d[V.DEMO_VIEW].readback(), V.DEMO_FLOOR_FRACTION)
    for d in var_d:
        d.close()
    n, (n_v, n_u) = len(Ps), imgs[0].shape
    ipath, ppath, vpath = (os.path.join(str(tmp_path), name) for name in ("imgs.f32", "Ps.f64", "vars.f32"))
    np.ascontiguousarray(both, np.float32).tofile(ipath)
    np.ascontiguousarray(var, np.float32).tofile(vpath)
    np.ascontiguousarray(E.pack_projection_matrices(Ps), np.float64).tofile(ppath)
    r = subprocess.run([exe, ipath, str(n), str(n_u), str(n_v), "96", "96", ppath, vpath, "%.9g" % floor], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "maps: 0 results differ" in r.stdout and "variances: 0 results differ, 2 handles" in r.stdout, r.stdout
    assert "variance robust map adapter ok" in r.stdout
