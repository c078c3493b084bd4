"""direct_pose_pairs: the tuples MetricDirect.evaluate_pose_deltas evaluates for one pose, against a brute-force enumeration; and
the C++ statement of the same enumeration and of the list checks (csrc/ecc_direct_lists_host.h), compiled into a stand-alone
program and run on the CPU (tests/c/direct_lists_host.cpp; scripts/sanitize.sh runs the same program under ASan and UBSan)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(n, moved):
    out = []
    for ij in range(n * n):
        i, j = divmod(ij, n)
        if i < j and (i in moved or j in moved):
            out.append((i, j, i, j))
    return np.asarray(out, np.int32).reshape(-1, 4)


@pytest.mark.parametrize("n,moved", [(8, [3]), (8, [0]), (8, [7]), (2, [1]), (8, [6, 2]), (5, [1, 2]), (9, [8, 0, 4])])
def test_moved_views_against_brute_force(n, moved):
    from epipolarconsistency_amd import direct_pose_pairs
    got = direct_pose_pairs(n, moved)
    assert got.dtype == np.int32 and np.array_equal(got, brute_force(n, set(moved)))
    m = len(moved)
    assert len(got) == m * (n - 1) - m * (m - 1) // 2  # the shared pairs appear once
    assert len({tuple(t) for t in got}) == len(got)


def test_one_and_two_moved_views():
    from epipolarconsistency_amd import direct_pose_pairs
    assert direct_pose_pairs(4, 2).tolist() == [[0, 2, 0, 2], [1, 2, 1, 2], [2, 3, 2, 3]]
    two = direct_pose_pairs(4, [3, 1]).tolist()
    assert two == [[0, 1, 0, 1], [0, 3, 0, 3], [1, 2, 1, 2], [1, 3, 1, 3], [2, 3, 2, 3]] and two.count([1, 3, 1, 3]) == 1


def test_all_views_moved_is_get_ij_order():
    from epipolarconsistency_amd import direct_pose_pairs
    n = 6
    i, j = np.triu_indices(n, 1)  # row-major over i < j: the order of get_ij (ref: EpipolarConsistencyCommon.hxx:52-79)
    assert np.array_equal(direct_pose_pairs(n, range(n)), np.stack([i, j, i, j], 1))
    assert direct_pose_pairs(n, []).shape == (0, 4)
    with pytest.raises(ValueError):
        direct_pose_pairs(n, [n])


def test_host_header_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "direct_lists_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "epipolarconsistency_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "direct_lists_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "direct_lists_host ok" in out
