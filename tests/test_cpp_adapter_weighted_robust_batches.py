"""evaluateWeightedRobustPoseDeltas and evaluateWeightedRobustTransforms of the header-only C++ adapter
(epipolarconsistency_amd/cpp/EpipolarConsistencyHip.hxx), in the manner of tests/test_cpp_adapter_robust_batches.py: the non-Eigen
branch compiled and linked with g++ -Wall -Werror, the Eigen branch -fsyntax-only against tests/cpp/mock_eigen; on the GPU both methods
return what ecc_metric_evaluate_weighted_robust_pose_deltas / ecc_metric_evaluate_weighted_robust_transforms return for the same
arguments."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")


def _build(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_weighted_robust_batches")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_robust_batches.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_adapter_weighted_robust_batches_compile_and_link(tmp_path):
    exe = _build(tmp_path)
    # without arguments the driver checks the argument errors of the C calls and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_of_the_weighted_robust_batches_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_robust_batches_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
def test_adapter_returns_what_the_c_calls_return(tmp_path):
    """Eight views of the small scan, intermediates and per-view line weights (a flagged block) computed by the adapter: four poses
    (one view, two views, the base, the last view) and three transforms of 4 x 4 views under each of the three losses, delta =
    weightedRobustScale(rows at infinity, 0.5) -- values, coverages, inlier masses and pair terms of the adapter's methods against the
    C calls on a second metric over the same intermediates, bit for bit."""
    import epipolarconsistency_amd as E
    from conftest import make_small_scan
    exe = _build(tmp_path)
    Ps, imgs = make_small_scan()
    n, (n_v, n_u) = len(Ps), imgs[0].shape
    ipath, ppath = os.path.join(str(tmp_path), "imgs.f32"), os.path.join(str(tmp_path), "Ps.f64")
    np.ascontiguousarray(imgs, np.float32).tofile(ipath)
    np.ascontiguousarray(E.pack_projection_matrices(Ps), np.float64).tofile(ppath)
    r = subprocess.run([exe, ipath, str(n), str(n_u), str(n_v), "96", "96", ppath], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pose deltas: 0 results differ" in r.stdout and "transforms: 0 results differ, 3 batched" in r.stdout, r.stdout
    assert "weighted robust batches adapter ok" in r.stdout
