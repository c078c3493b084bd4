"""csrc/ecc_extremum_tile.h on the host: tests/c/extremum_tile.cpp walks the header's tile, halo and clamp arithmetic tile by tile as
line_weights_kernel.hip does and compares with a brute-force window loop, bit for bit -- the maximum form and the clip + minimum form,
arrays that are no multiple of the tile, radii up to the caps and beyond the array.  The clip + minimum form must also reproduce
line_weights_from_lengths on the seeded lengths of tests/test_weighted_abi.py::test_line_weights_from_lengths (same recipe, made
here) and on a few more grids."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epipolarconsistency_amd", "csrc")


def _records(path):
    from epipolarconsistency_amd import line_weights_from_lengths
    rng = np.random.default_rng(3)
    L = np.where(rng.random((13, 17)) < 0.2, rng.uniform(0.0, 3.0, (13, 17)), 0.0).astype(np.float32)
    L[0, 0], L[12, 16] = 5.0, 0.25   # the corners: the clamped edges
    cases = [(L, zero_at, g) for zero_at, g in ((1.0, 0), (1.0, 1), (2.5, 2))]
    more = np.random.default_rng(5)
    for n_t, n_alpha, zero_at, g in ((30, 33, 1.0, 8), (31, 7, 0.7, 3), (97, 20, 3.0, 1), (5, 3, 1.0, 8), (1, 1, 1.0, 1)):
        M = np.where(more.random((n_t, n_alpha)) < 0.3, more.uniform(0.0, 4.0, (n_t, n_alpha)), 0.0).astype(np.float32)
        cases.append((M, zero_at, g))
    with open(path, "wb") as f:
        for lengths, zero_at, g in cases:
            want = line_weights_from_lengths(lengths, zero_at, g)
            assert want.shape == lengths.shape and want.min() >= 0.0 and want.max() <= 1.0
            f.write(np.array([lengths.shape[0], lengths.shape[1], g], np.int32).tobytes())
            f.write(np.array([zero_at], np.float32).tobytes())
            f.write(np.ascontiguousarray(lengths, np.float32).tobytes())
            f.write(np.ascontiguousarray(want, np.float32).tobytes())
    return len(cases)


def test_tile_walk_matches_brute_force_and_numpy(tmp_path):
    exe = os.path.join(str(tmp_path), "extremum_tile")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "c", "extremum_tile.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    data = os.path.join(str(tmp_path), "records.bin")
    n = _records(data)
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0 and "extremum tile ok" in r.stdout and "%d records from numpy" % n in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr)
