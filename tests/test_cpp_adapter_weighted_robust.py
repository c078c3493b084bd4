"""evaluateWeightedRobust, evaluateWeightedRobustPairs and weightedRobustScale of the header-only C++ adapter
(epipolarconsistency_amd/cpp/EpipolarConsistencyHip.hxx), in the manner of tests/test_cpp_adapter_robust_batches.py: the non-Eigen
branch compiled and linked with g++ -Wall -Werror and run for what needs no device, the Eigen branch -fsyntax-only against
tests/cpp/mock_eigen; the members are single-device only and throw on a group before anything else."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")


def test_adapter_weighted_robust_compiles_and_links(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_weighted_robust")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_robust.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the argument errors of the C calls and the static scale, and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_of_weighted_robust_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_weighted_robust_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_adapter_members_throw_on_a_group():
    """Beside evaluateRobust / evaluateRobustPairs / robustScale, single-device only: each member throws on a group before anything
    else and then makes its C call with coverage and inlier_mass passed through."""
    with open(os.path.join(PKG, "cpp", "EpipolarConsistencyHip.hxx")) as f:
        text = f.read()
    for head, method, call in (("double evaluateWeightedRobust(int loss, float delta, double* coverage = 0x0, double* inlier_mass = 0x0,",
                                "evaluateWeightedRobust", "ecc_metric_evaluate_weighted_robust(m_h, loss, delta, &value, coverage, inlier_mass,"),
                               ("double evaluateWeightedRobustPairs(const std::vector<int>& indices, int loss, float delta, double* coverage = 0x0,",
                                "evaluateWeightedRobustPairs", "ecc_metric_evaluate_weighted_robust_pairs(m_h, ")):
        at = text.index(head)
        body = text[at:text.index("\n    }\n", at)]
        assert 'if (m_gh) throw std::runtime_error("%s: not available on a device group");' % method in body
        assert body.index("if (m_gh) throw") < body.index("detail::check(" + call)
    eigen = text.index("double evaluateWeightedRobustPairs(const std::vector<Eigen::Vector4i>& indices")
    assert "return evaluateWeightedRobustPairs(idx, loss, delta, coverage, inlier_mass, pair_terms);" in text[eigen:text.index("#endif", eigen)]
    assert "static double weightedRobustScale(const std::vector<float>& pair_terms, double k = 1.0)" in text
    assert text.index("static double robustScale(") < text.index("double evaluateWeightedRobust(") < text.index("static double weightedRobustScale(")
