"""evaluateResidualHistogram[Pairs], evaluateVarianceResidualHistogram[Pairs] and histogramQuantile of the header-only C++ adapter
(epipolarconsistency_amd/cpp/EpipolarConsistencyHip.hxx), in the manner of tests/test_cpp_adapter_variance_robust_map.py: the
non-Eigen branch compiled and linked with g++ -Wall -Werror; on the GPU the methods return what the C calls return for the same
arguments."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")


def _build(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_residual_histogram")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_residual_histogram.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_adapter_residual_histogram_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    # without arguments the driver checks the argument errors of the C calls and the host helper, and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_adapter_members_throw_on_a_group():
    """Single-device only: each member throws on a group before anything else and then makes its C call."""
    with open(os.path.join(PKG, "cpp", "EpipolarConsistencyHip.hxx")) as f:
        text = f.read()
    for head, method, call in (("void evaluateResidualHistogram(float width, int n_bins, std::vector<uint64_t>& counts)",
                                "evaluateResidualHistogram", "ecc_metric_evaluate_residual_histogram(m_h, width, n_bins,"),
                               ("void evaluateResidualHistogramPairs(const std::vector<int>& indices, float width, int n_bins,",
                                "evaluateResidualHistogramPairs", "ecc_metric_evaluate_residual_histogram_pairs(m_h, "),
                               ("void evaluateVarianceResidualHistogram(float floor, float width, int n_bins, std::vector<uint64_t>& counts)",
                                "evaluateVarianceResidualHistogram", "ecc_metric_evaluate_variance_residual_histogram(m_h, floor, width, n_bins,"),
                               ("void evaluateVarianceResidualHistogramPairs(const std::vector<int>& indices, float floor, float width, int n_bins,",
                                "evaluateVarianceResidualHistogramPairs", "ecc_metric_evaluate_variance_residual_histogram_pairs(m_h, ")):
        at = text.index(head)
        body = text[at:text.index("\n    }\n", at)]
        first = body[body.index("{") + 1:].strip()
        assert first.startswith('if (m_gh) throw std::runtime_error("%s: not available on a device group");' % method), method   # the first statement
        assert body.index("if (m_gh) throw") < body.index("detail::check(" + call)
    assert "static double histogramQuantile(const std::vector<uint64_t>& row, double width, double q)" in text


@pytest.mark.gpu
def test_adapter_returns_what_the_c_calls_return(tmp_path, gpu_ctx):
    """Eight views of the small scan with DESIGN.md 4.30's noise and block, intermediates and variance fields computed by the
    adapter; the raw form on the n metric and the variance form on the 2 n metric, all pairs and a list of three pairs, at 64 and
    256 bins: the adapter's tables against the C calls' on second metrics over the same intermediates, bit for bit; an empty list;
    the median through the adapter and through the C helper; refused arguments arrive as exceptions."""
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
    data = E.RadonIntermediate.compute_batch(gpu_ctx, np.ascontiguousarray(both, np.float32), 96, 96)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, data)
    width = 4.0 * E.robust_scale(m.evaluate_robust(E.LOSS_TRUNCATED, float("inf"), want_pairs=True)[-1]) / 64
    m.close()
    for d in data:
        d.close()
    n, (n_v, n_u) = len(Ps), imgs[0].shape
    ipath, ppath, vpath = (os.path.join(str(tmp_path), name) for name in ("imgs.f32", "Ps.f64", "vars.f32"))
    np.ascontiguousarray(both, np.float32).tofile(ipath)
    np.ascontiguousarray(var, np.float32).tofile(vpath)
    np.ascontiguousarray(E.pack_projection_matrices(Ps), np.float64).tofile(ppath)
    r = subprocess.run([exe, ipath, str(n), str(n_u), str(n_v), "96", "96", ppath, vpath, "%.9g" % floor, "%.9g" % width], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "histograms: 0 results differ" in r.stdout and "refused: 2 of 2" in r.stdout, r.stdout
    assert "residual histogram adapter ok" in r.stdout
