"""The oracle of MetricDirect (oracle.direct_pair) against a second statement of it (tests/direct_terms.py), on the CPU.

tests/test_gpu_direct_lines.py holds the device to oracle.direct_pair line for line; these tests hold oracle.direct_pair to the
numpy float32 line integral (bit for bit) and to lines formed from geometry in float64 (within the line bar), and check the two
ways in which the oracle takes input that it would otherwise compute itself: a caller's kappa grid and a caller's lines."""
import functools
import os
import subprocess

import numpy as np
import pytest

import direct_terms as dt
import geometry_catalog as gc

N_U, N_V = 96, 72


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def small(name):
    """A 4-view catalogue geometry with its detector scaled to 96 px wide, textured projections and the radius."""
    import oracle
    from epipolarconsistency_amd import synthetic
    Ps, n_u, n_v = gc.make(name, 4)
    s = N_U / n_u
    n_v = int(round(n_v * s))
    Ps = [np.diag([s, s, 1.0]) @ P for P in Ps]
    imgs = dt.textured(synthetic.projections_numpy(Ps, N_U, n_v, gc.phantom()), 3)
    return Ps, imgs, n_v, oracle.object_radius(Ps[0], N_U, n_v)


def handmade_lines(n_u, n_v):
    """(n, 3) float32: exactly horizontal and vertical lines (inside, on and one float to either side of the `inside` boundary),
    lines through every corner of the detector, of the pixel centres and of the clipping box, pencils sliding off each corner,
    and lines that miss the image by far."""
    f = np.float32
    out = []
    for edge, flat in ((n_v, (0.0, 1.0)), (n_u, (1.0, 0.0))):
        cs = [f(0), np.nextafter(f(0), f(1)), np.nextafter(f(0), f(-1)), f(edge), np.nextafter(f(edge), f(0)),
              np.nextafter(f(edge), f(2 * edge)), f(0.5), f(1), f(edge - 1), f(edge - 0.5), f(0.37 * edge), f(-3), f(edge + 3)]
        for c in cs:
            for sign in (1.0, -1.0):  # the same line with either normal: d = (l1, -l0) turns round, and 0 becomes -0
                out.append((sign * flat[0], sign * flat[1], -sign * float(c)))
    corners = [(0, 0), (n_u, 0), (0, n_v), (n_u, n_v), (n_u - 1, n_v - 1), (1, 1), (n_u - 1, 1), (1, n_v - 1), (0.5, 0.5)]
    for (cx, cy) in corners:
        for th in np.linspace(0.0, np.pi, 13, endpoint=False) + 0.01:
            out.append((np.cos(th), np.sin(th), -(cx * np.cos(th) + cy * np.sin(th))))
    # pencils of parallel lines sliding off a corner of the detector in steps of 1/64 px: somewhere along each the reference's
    # `inside` test turns from true to false
    for (cx, cy, th) in ((0, 0, 0.8), (n_u, 0, 2.3), (0, n_v, 2.4), (n_u, n_v, 0.75)):
        n = np.array([np.cos(th), np.sin(th)])
        away = np.sign((cx - 0.5 * n_u) * n[0] + (cy - 0.5 * n_v) * n[1])
        for step in np.arange(-96, 96) / 64.0:
            out.append((n[0], n[1], -(cx * n[0] + cy * n[1] + away * step)))
    for th in (0.3, 1.2, 2.0, 2.9):
        out.append((np.cos(th), np.sin(th), 500.0))
        out.append((np.cos(th), np.sin(th), -500.0))
    return np.ascontiguousarray(np.array(out, np.float64), np.float32)


def test_handmade_lines_cover_their_cases():
    L = handmade_lines(N_U, N_V)
    c = dt.clip_f32(L, N_U, N_V)
    assert np.any(L[:, 0] == 0) and np.any(L[:, 1] == 0)              # d1 == 0 and d0 == 0
    assert np.any(c["inside"]) and np.any(~c["inside"])
    # one float to either side of the boundary decides: the horizontal lines at v = n_v and the next float above
    top = dt.clip_f32(np.array([[0, 1, -N_V], [0, 1, -np.nextafter(np.float32(N_V), np.float32(1e9))]], np.float32), N_U, N_V)
    assert top["inside"].tolist() == [True, False]
    low = dt.clip_f32(np.array([[1, 0, -0.0], [1, 0, np.nextafter(np.float32(0), np.float32(1))]], np.float32), N_U, N_V)
    assert low["inside"].tolist() == [True, False]
    # every sliding pencil crosses the boundary
    pencils = c["inside"][-(4 * 192 + 8):-8].reshape(4, 192)
    assert np.all(pencils.any(axis=1) & ~pencils.all(axis=1))


@pytest.mark.parametrize("name", ["angulated", "rolled"])
def test_numpy_line_integral_equals_the_oracle_bit_for_bit(oracle_mod, name):
    Ps, imgs, n_v, radius = small(name)
    assert n_v == N_V
    auto = oracle_mod.direct_pair(Ps[0], Ps[3], imgs[0], imgs[3], 0.0, radius)
    hand = handmade_lines(N_U, N_V)
    lines = np.concatenate([auto["lines"], np.hstack([hand, hand[::-1]])])
    want = oracle_mod.direct_pair(Ps[0], Ps[3], imgs[0], imgs[3], 0.0, radius, lines=lines)
    assert len(want["samples0"]) == len(lines) and np.array_equal(_bits(want["lines"]), _bits(lines))
    assert np.array_equal(_bits(want["samples0"][:len(auto["lines"])]), _bits(auto["samples0"]))
    for which, img in ((0, imgs[0]), (1, imgs[3])):
        got = dt.line_integral_f32(img, lines[:, 3 * which:3 * which + 3])
        w = want["samples%d" % which]
        assert np.array_equal(_bits(got), _bits(w)), np.nonzero(_bits(got) != _bits(w))[0][:8]
        inside = dt.clip_f32(lines[:, 3 * which:3 * which + 3], N_U, N_V)["inside"]
        # the comparison is not one of zeros (lines along the clamped border integrate to 0: both offset samples are equal)
        n_auto = len(auto["lines"])
        assert np.all(w[~inside] == 0) and np.mean(w[:n_auto][inside[:n_auto]] != 0) > 0.99 and np.mean(w[inside] != 0) > 0.9
    # a single line takes the same way
    assert dt.line_integral_f32(imgs[0], lines[7, :3]) == want["samples0"][7]


def test_numpy_texel_rule_is_the_normative_one(oracle_mod):
    img = small("angulated")[1][1]
    rng = np.random.default_rng(5)
    x = rng.uniform(-2, N_U + 2, 400).astype(np.float32)
    y = rng.uniform(-2, N_V + 2, 400).astype(np.float32)
    x[:8] = [0, 0.5, 1, N_U - 0.5, N_U, 17, 17.5, -0.5]
    got = dt._tex2d(img, x, y)
    want = np.array([oracle_mod.tex2d(img, a, b) for a, b in zip(x, y)], np.float32)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("fbcc", [False, True])
@pytest.mark.parametrize("name", ["angulated", "scattered"])
def test_own_lines_and_own_grid_reproduce_the_bits(oracle_mod, name, fbcc):
    Ps, imgs, n_v, radius = small(name)
    for (i, j) in ((0, 3), (2, 1)):
        args = (Ps[i], Ps[j], imgs[i], imgs[j], 0.0, radius)
        auto = oracle_mod.direct_pair(*args, fbcc=fbcc)
        assert len(auto["kappas"]) > 200
        again = [oracle_mod.direct_pair(*args, fbcc=fbcc, lines=auto["lines"]),
                 oracle_mod.direct_pair(*args, fbcc=fbcc, kappas=auto["kappas"]),
                 oracle_mod.direct_pair(*args, fbcc=fbcc, kappas=auto["kappas"], lines=auto["lines"])]
        for b in again:
            for key in ("samples0", "samples1", "kappas", "lines"):
                assert np.array_equal(_bits(b[key]), _bits(auto[key])), key
            assert b["metric"] == auto["metric"] or (np.isnan(b["metric"]) and np.isnan(auto["metric"]))
        # a thinned grid picks out those lines; its lines handed in alone give the same samples
        thin = oracle_mod.direct_pair(*args, fbcc=fbcc, kappas=auto["kappas"][::3])
        assert np.array_equal(_bits(thin["samples1"]), _bits(auto["samples1"][::3]))
        assert np.array_equal(_bits(thin["lines"]), _bits(auto["lines"][::3]))
        only = oracle_mod.direct_pair(*args, fbcc=fbcc, lines=auto["lines"][::3])
        assert np.array_equal(_bits(only["samples0"]), _bits(auto["samples0"][::3]))
        d = (thin["samples0"] - thin["samples1"]).astype(np.float32)
        dk = dt.plane_range(Ps[i], Ps[j], N_U, n_v, radius)[1]
        if np.isfinite(thin["metric"]):
            assert abs(thin["metric"] - np.sum((d * d).astype(np.float64) * dk)) <= 1e-12 * thin["metric"]  # dkappa unchanged
    with pytest.raises(ValueError):
        oracle_mod.direct_pair(*args, kappas=auto["kappas"][:5], lines=auto["lines"])
    with pytest.raises(ValueError):
        oracle_mod.direct_pair(*args, kappas=np.zeros(0, np.float32))


@pytest.mark.parametrize("name", gc.NAMES)
def test_oracle_lines_agree_with_the_float64_statement(oracle_mod, name):
    """The oracle's float32 lines against lines_f64 at the oracle's own plane angles: within the line bar (the float64 line
    rounds to the oracle's float32 or to its neighbour).  The automatic grids agree to float64 rounding of the range: bit for
    bit except where an angle cancels to near 0 in the middle of the grid."""
    Ps, imgs, n_v, radius = small(name)
    worst, equal, total = 0.0, 0, 0
    for i in range(4):
        for j in range(i + 1, 4):
            want = oracle_mod.direct_pair(Ps[i], Ps[j], imgs[i], imgs[j], 0.0, radius)
            k_max, dkappa, n = dt.plane_range(Ps[i], Ps[j], N_U, n_v, radius)
            assert n == len(want["kappas"]) > 200
            grid, _ = dt.lines_f64(Ps[i], Ps[j], None, N_U, n_v, radius)
            off = grid != want["kappas"]
            assert off.mean() <= 0.01
            assert np.all(np.abs(grid.astype(np.float64) - want["kappas"])[off] <= 8 * np.finfo(np.float64).eps * k_max)
            kap, lines = dt.lines_f64(Ps[i], Ps[j], want["kappas"], N_U, n_v, radius)
            assert np.array_equal(kap, want["kappas"])
            assert np.allclose(np.hypot(lines[:, [0, 3]], lines[:, [1, 4]]), 1.0, rtol=0, atol=1e-14)
            worst = max(worst, dt.line_difference_in_bars(want["lines"], lines).max())
            equal += int(np.all(want["lines"] == lines.astype(np.float32), axis=1).sum())
            total += len(lines)
    print("%s: worst line difference %.3f bars, %d of %d rows equal the rounded float64 line" % (name, worst, equal, total))
    assert worst <= 1.0
    assert equal >= 0.9 * total


def test_line_bar_is_sharp():
    """One float32 step is inside the bar, two are outside; a direction error of 1e-6 rad is far outside."""
    l = np.array([[0.6, -0.8, -321.5, 0.8, 0.6, 12.25]], np.float32)
    up = np.nextafter(l, np.float32(1e9))
    assert dt.line_difference_in_bars(up, l).max() <= 1.0
    assert dt.line_difference_in_bars(np.nextafter(up, np.float32(1e9)), l).min() > 1.0
    th = np.arctan2(-0.8, 0.6) + 1e-6
    turned = l.copy()
    turned[0, :2] = [np.cos(th), np.sin(th)]
    assert dt.line_difference_in_bars(turned, l).max() > 5.0


def test_textured_recipe():
    Ps, imgs, n_v, radius = small("rolled")
    from epipolarconsistency_amd import synthetic
    raw = synthetic.projections_numpy(Ps, N_U, n_v, gc.phantom())
    assert (raw == 0).mean() > 0.05 and imgs.min() > 0 and imgs.dtype == np.float32 and imgs.flags["C_CONTIGUOUS"]
    assert np.array_equal(imgs, dt.textured(raw, 3)) and not np.array_equal(imgs, dt.textured(raw, 4))
    top = raw.max()
    assert np.all(imgs - raw <= np.float32(0.121 * top)) and np.all(imgs - raw >= -1e-3 * top)


def test_a_stale_oracle_library_cannot_answer(oracle_mod, tmp_path, monkeypatch):
    """A libecc_oracle.so from before eccor_direct_pair_with: named by ECC_ORACLE_LIB it is refused; in the oracle's own
    directory it is rebuilt from ecc_oracle.c."""
    here = os.path.dirname(os.path.abspath(oracle_mod.__file__))
    src = tmp_path / "old.c"
    src.write_text("int eccor_direct_pair(void) { return 0; }\n")
    stale = tmp_path / "libstale.so"
    subprocess.run([os.environ.get("CC", "gcc"), "-shared", "-fPIC", str(src), "-o", str(stale)], check=True)
    monkeypatch.setenv("ECC_ORACLE_LIB", str(stale))
    with pytest.raises(RuntimeError, match="stale"):
        oracle_mod._load("libecc_oracle.so")
    monkeypatch.delenv("ECC_ORACLE_LIB")
    work = tmp_path / "oracle"
    work.mkdir()
    for name in ("Makefile", "ecc_oracle.c"):
        (work / name).write_bytes(open(os.path.join(here, name), "rb").read())
    (work / "libecc_oracle.so").write_bytes(stale.read_bytes())
    os.utime(work / "ecc_oracle.c", (1e9, 1e9))  # the library is newer than its source: make alone would leave it
    monkeypatch.setattr(oracle_mod, "_HERE", str(work))
    L = oracle_mod._load("libecc_oracle.so")
    assert hasattr(L, "eccor_direct_pair_with")


def test_the_package_does_not_import_the_oracle():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epipolarconsistency_amd")
    for base, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
