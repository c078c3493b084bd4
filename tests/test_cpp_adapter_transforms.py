"""evaluateTransforms and the two added virtuals of the Metric base in the header-only C++ adapter
(epipolarconsistency_amd/cpp/EpipolarConsistencyHip.hxx), built in the manner of tests/test_cpp_adapter.py: the non-Eigen
branch compiled and linked with g++ -Wall -Werror, the Eigen branch -fsyntax-only against tests/cpp/mock_eigen."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "epipolarconsistency_amd")


def test_adapter_transforms_compile_and_link(tmp_path):
    exe = os.path.join(str(tmp_path), "test_adapter_transforms")
    cmd = ["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_transforms.cpp"), "-L" + PKG, "-lecc_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without arguments the driver checks the host parts (identity homography, P * I == P) and touches no device
    assert subprocess.run([exe]).returncode == 2


def test_eigen_branch_of_evaluate_transforms_is_well_formed():
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror", "-DECC_TEST_MOCK_EIGEN",
           "-I" + os.path.join(ROOT, "tests", "cpp", "mock_eigen"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_adapter_transforms_eigen_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
