"""MetricDirect's line integrals per line on general C-arm geometries (tests/geometry_catalog.py), against oracle.direct_pair.

Every compared pair goes through `check_pair`: the kappa grid bit for bit, the lines within one float32 step of the oracle's,
the samples of BOTH images bit for bit on ALL lines (the oracle integrates along the device's own float32 lines, so neither
libm's sin / cos enters), the reduction recomputed from the device's own samples, and the metric.  The images are the
catalogue phantom's projections with a texture added (direct_terms.textured): the sphere phantom alone leaves a quarter to a
half of the reference integrals at exactly 0, where a wrong tap reads 0 as well.

All catalogue detectors are at least 384 px on both sides, so everything here but the threshold test's small sizes runs
direct_lines_kernel, the LDS slab walker (csrc/ecc_slab_tile.h), whose tile orientation, walking direction and window slope
come from a workgroup's first line.  The pairs are chosen on the CPU for what that rule is sensitive to (`select_pairs`)."""
import functools

import numpy as np
import pytest

import direct_terms as dt
import geometry_catalog as gc

pytestmark = pytest.mark.gpu

N_VIEWS = 12
CLASSES = ("epipole_inside", "mixed_workgroup", "all_plain", "all_transposed")
# totals over the tests of this module that ran, printed by each test (pytest -s)
TOTAL = {"lines": 0, "pairs": 0}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@functools.lru_cache(maxsize=None)
def scene(name, n_views=N_VIEWS, size=None):
    """Matrices, textured images, detector size and object radius of a catalogue geometry; size (n_u, n_v): the same
    geometry with the detector resampled to that many pixels over the same field of view."""
    import oracle
    from epipolarconsistency_amd import synthetic
    Ps, n_u, n_v = gc.make(name, n_views)
    if size is not None:
        Ps = [np.diag([size[0] / n_u, size[1] / n_v, 1.0]) @ P for P in Ps]
        n_u, n_v = size
    imgs = dt.textured(synthetic.projections_numpy(Ps, n_u, n_v, gc.phantom()), 3)
    return dict(Ps=Ps, imgs=imgs, n_u=n_u, n_v=n_v, radius=oracle.object_radius(Ps[0], n_u, n_v))


def transposed_workgroups(lines3):
    """Per workgroup of 256 consecutive lines: (any, all) of `the line's normal is closer to y than to x`, the slab kernel's
    rule for staging from the transposed image."""
    t = np.abs(lines3[:, 1]) > np.abs(lines3[:, 0])
    groups = [t[k:k + 256] for k in range(0, len(t), 256)]
    return np.array([g.any() for g in groups]), np.array([g.all() for g in groups])


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """The oracle's derivative-form result of all 66 pairs of a geometry and each pair's classes."""
    import oracle
    s = scene(name)
    ij = gc.pair_indices(N_VIEWS)
    ep = gc.epipoles(s["Ps"])
    out = []
    for q, (i, j) in enumerate(ij):
        w = oracle.direct_pair(s["Ps"][i], s["Ps"][j], s["imgs"][i], s["imgs"][j], 0.0, s["radius"])
        inside = bool(np.any((ep[q, :, 0] >= 0) & (ep[q, :, 0] <= s["n_u"]) & (ep[q, :, 1] >= 0) & (ep[q, :, 1] <= s["n_v"])))
        any0, all0 = transposed_workgroups(w["lines"][:, :3])
        any1, all1 = transposed_workgroups(w["lines"][:, 3:])
        cls = set()
        if inside:
            cls.add("epipole_inside")
        if np.any(any0 & ~all0) or np.any(any1 & ~all1):
            cls.add("mixed_workgroup")
        if not any0.any() and not any1.any():
            cls.add("all_plain")
        if all0.all() and all1.all():
            cls.add("all_transposed")
        first = bool(dt.clip_f32(w["lines"][:1].reshape(2, 3), s["n_u"], s["n_v"])["inside"].all())
        out.append(dict(i=int(i), j=int(j), metric=w["metric"], n=len(w["kappas"]), classes=cls, first_line_inside=first))
    return out


@functools.lru_cache(maxsize=None)
def select_pairs(name):
    """At most 10 pairs: every pair with an epipole inside a detector, two with a mixed-orientation workgroup, one that never
    uses the transposed tile, one that uses nothing else, (0, 1) and (0, 11) -- as far as the geometry has them."""
    cat = catalogue(name)
    picked = [(c["i"], c["j"]) for c in cat if "epipole_inside" in c["classes"]]
    for cls, count in (("mixed_workgroup", 2), ("all_plain", 1), ("all_transposed", 1)):
        more = [(c["i"], c["j"]) for c in cat if cls in c["classes"] and (c["i"], c["j"]) not in picked]
        picked += more[:count]
    for p in ((0, 1), (0, 11)):
        if p not in picked:
            picked.append(p)
    return tuple(picked[:10])


def classes_of(name, i, j):
    return next(c["classes"] for c in catalogue(name) if (c["i"], c["j"]) == (i, j))


def check_pair(m, Ps, imgs, i, j, fbcc, kappas=None):
    """One pair of MetricDirect `m` (built on Ps, imgs) against the oracle; returns the device's result and the figures.

    a. the kappa grid and the line count equal the oracle's bit for bit;
    b. the lines: at least 90 % of the rows bit-equal, every component within one float32 step of the oracle's or within
       1e-12 max(1, |l2|) (direct_terms.line_difference_in_bars <= 1: both sides round a float64 line once);
    c. the samples of both images on ALL lines, bit for bit against the oracle integrating along the device's own lines;
       where the fan-beam weights are not finite (epipole inside the detector) the non-finite positions coincide and the finite
       samples are bit-equal;
    d. float64 sum of float32(v0 - v1)^2 dkappa over the device's own samples equals the returned metric to 1e-12 (only the
       order of summation differs: n eps / 2 < 2e-13 for the 3200 lines at most used here);
    e. the metric against the oracle's own (own lines) to 1e-5.
    Condition on the reference side: at most 25 % of its integrals are exactly 0, and at most 1 % of those on lines that pass
    its own float32 clip test (direct_terms.clip_f32)."""
    import oracle
    n_v, n_u = imgs[i].shape
    radius = oracle.object_radius(Ps[0], n_u, n_v)
    m.setFanBeamConsistency(fbcc)
    val, got = m.evaluateForImagePair(i, j, kappas=kappas)
    args = (Ps[i], Ps[j], imgs[i], imgs[j], 0.0, radius)
    want = oracle.direct_pair(*args, fbcc=fbcc, kappas=kappas)
    tag = "pair (%d, %d)%s" % (i, j, " fbcc" if fbcc else "")
    # a
    n = len(want["kappas"])
    assert len(got["kappas"]) == n and len(got["lines"]) == n, (tag, len(got["kappas"]), n)
    assert np.array_equal(_bits(got["kappas"]), _bits(want["kappas"])), tag
    fig = dict(n=n, worst_bars=0.0, same=1.0, zero=0.0, zero_inside=0.0, finite=True)
    if n == 0:
        assert val == 0.0 and want["metric"] == 0.0, tag
        return val, got, fig
    # b
    same = np.all(_bits(got["lines"]) == _bits(want["lines"]), axis=1)
    bars = dt.line_difference_in_bars(got["lines"], want["lines"])
    fig["worst_bars"], fig["same"] = float(bars.max()), float(same.mean())
    print("%s: %d lines, %.4f of the rows bit-equal, worst line difference %.3f bars" % (tag, n, same.mean(), bars.max()))
    assert same.mean() >= 0.9, (tag, same.mean())
    assert bars.max() <= 1.0, (tag, bars.max(), np.argwhere(bars > 1.0)[:8].tolist())
    # c
    own = oracle.direct_pair(*args, fbcc=fbcc, lines=got["lines"], kappas=got["kappas"])
    zeros, zeros_inside, n_inside = 0, 0, 0
    for which in (0, 1):
        g, w = got["redundant_samples%d" % which], own["samples%d" % which]
        ok = np.isfinite(w)
        if not fbcc:
            assert ok.all(), tag
        assert np.array_equal(np.isfinite(g), ok), (tag, which, np.nonzero(np.isfinite(g) != ok)[0][:8].tolist())
        bad = np.nonzero(_bits(g)[ok] != _bits(w)[ok])[0]
        assert len(bad) == 0, (tag, "image %d: %d of %d samples differ, first at lines %s (workgroups %s)"
                               % (which, len(bad), n, np.nonzero(ok)[0][bad][:8].tolist(),
                                  sorted(set((np.nonzero(ok)[0][bad] // 256).tolist()))[:8]))
        inside = dt.clip_f32(got["lines"][:, 3 * which:3 * which + 3], n_u, n_v)["inside"]
        assert np.all(g[~inside] == 0), (tag, which)  # lines that miss the detector give exactly 0
        zeros += int(np.sum(w == 0))
        zeros_inside += int(np.sum(w[inside] == 0))
        n_inside += int(inside.sum())
        fig["finite"] = fig["finite"] and bool(ok.all())
    fig["zero"], fig["zero_inside"] = zeros / (2.0 * n), zeros_inside / max(n_inside, 1)
    assert fig["zero"] <= 0.25, (tag, fig["zero"])
    assert fig["zero_inside"] <= 0.01, (tag, fig["zero_inside"])
    # d
    dkappa = dt.plane_range(Ps[i], Ps[j], n_u, n_v, radius)[1]
    with np.errstate(all="ignore"):
        d = got["redundant_samples0"] - got["redundant_samples1"]
        red = float(np.sum((d * d).astype(np.float64) * dkappa))
    if np.isfinite(red):
        assert abs(val - red) <= 1e-12 * abs(red), (tag, val, red)
    else:
        assert not np.isfinite(val), (tag, val, red)
    # e
    if np.isfinite(want["metric"]):
        assert _rel(val, want["metric"]) < 1e-5, (tag, val, want["metric"])
    else:
        assert not np.isfinite(val), (tag, val, want["metric"])
    TOTAL["lines"] += 2 * n
    TOTAL["pairs"] += 1
    return val, got, fig


def _report(name, figs):
    print("%s: %d pairs, %d lines compared bit for bit in both images; exactly-zero reference integrals at most %.4f %% per "
          "pair (cap 25 %%), %.4f %% among lines inside the detector (cap 1 %%); rows bit-equal at least %.4f; worst line "
          "difference %.3f bars; module total so far %d line integrals in %d pairs"
          % (name, len(figs), sum(2 * f["n"] for f in figs), 100 * max(f["zero"] for f in figs),
             100 * max(f["zero_inside"] for f in figs), min(f["same"] for f in figs), max(f["worst_bars"] for f in figs),
             TOTAL["lines"], TOTAL["pairs"]))


@pytest.mark.parametrize("name", gc.NAMES)
def test_catalogue_derivative_form(gpu_ctx, name):
    """Measured on the MI355X: in all five geometries (7, 8, 6, 7 and 10 pairs; 115 998 line integrals) the share of rows bit-equal
    to the oracle's line is 1.0000 in every pair and the worst line difference is 0.000 bars (the device's sin / cos gave the
    host's bits on every one of these angles); exactly-zero reference integrals at most 13.9 / 21.2 / 3.3 / 13.9 / 13.8 % per pair
    (cap 25 %) and 0 % among lines that pass the clip test (cap 1 %)."""
    import epipolarconsistency_amd as E
    s = scene(name)
    m = E.MetricDirect(gpu_ctx, s["Ps"], s["imgs"])
    figs = [check_pair(m, s["Ps"], s["imgs"], i, j, False)[2] for (i, j) in select_pairs(name)]
    _report(name, figs)
    m.close()


@pytest.mark.parametrize("name", gc.NAMES)
def test_catalogue_fan_beam_form(gpu_ctx, name):
    """The same pairs in the fan-beam form.  Pairs with an epipole inside a detector have non-finite weights in the reference's
    own formula: there the non-finite positions coincide and the finite samples are bit-equal (check_pair, c); the others are
    finite throughout.  Measured on the MI355X: 3 of 7, 2 of 8, 6 of 6, 3 of 7 and 5 of 10 pairs finite; bit-equal rows 1.0000 and
    worst line difference 0.000 bars in every pair; zero shares as in the derivative form."""
    import epipolarconsistency_amd as E
    s = scene(name)
    m = E.MetricDirect(gpu_ctx, s["Ps"], s["imgs"])
    figs = []
    for (i, j) in select_pairs(name):
        fig = check_pair(m, s["Ps"], s["imgs"], i, j, True)[2]
        if "epipole_inside" not in classes_of(name, i, j):
            assert fig["finite"], (name, i, j)
        figs.append(fig)
    print(name, "finite pairs:", sum(f["finite"] for f in figs), "of", len(figs))
    assert any(f["finite"] for f in figs)
    _report(name, figs)
    m.close()


@pytest.mark.parametrize("name", ["angulated", "rolled"])
def test_all_pairs_and_the_cost_image(gpu_ctx, name):
    """evaluate(cost): 12 views, 66 pairs in one batch; the sum and every cost[j, i] against the oracle to 1e-5 (measured on the
    MI355X: worst entry 5.8e-8 and 5.2e-8 relative, the float32 rounding of the cost image)."""
    import epipolarconsistency_amd as E
    s = scene(name)
    cat = catalogue(name)
    m = E.MetricDirect(gpu_ctx, s["Ps"], s["imgs"])
    cost = np.full((N_VIEWS, N_VIEWS), -1.0, np.float32)
    got = m.evaluate(cost)
    want = np.zeros((N_VIEWS, N_VIEWS))
    for c in cat:
        want[c["j"], c["i"]] = c["metric"]
    assert _rel(got, sum(c["metric"] for c in cat)) < 1e-5
    il = np.tril_indices(N_VIEWS, -1)
    rel = np.abs(cost[il] - want[il]) / np.abs(want[il])
    print(name, "worst cost entry: %.3g relative" % rel.max())
    assert np.all(want[il] > 0) and rel.max() < 1e-5, np.argwhere(rel >= 1e-5)[:8].tolist()
    iu = np.triu_indices(N_VIEWS)  # the diagonal and above: untouched
    assert np.all(cost[iu] == -1.0)
    assert _rel(m.evaluate(), got) < 1e-12
    m.close()


@pytest.mark.parametrize("fbcc", [False, True])
@pytest.mark.parametrize("name", ["angulated", "scattered"])
def test_caller_grids_on_the_slab_kernel(gpu_ctx, name, fbcc):
    """A caller's grid need not be a pencil in order: permuted, no workgroup holds adjacent lines, the band of a workgroup is the
    whole image and runs fail the containment check; every line must still get the bits it gets in the automatic grid.
    Measured on the MI355X (angulated (0, 9), scattered (0, 3), both forms): bit-equal rows 1.0000, worst line difference 0.000
    bars in every grid; zero share at most 6.8 % (the grid reaching beyond the range)."""
    import epipolarconsistency_amd as E
    s = scene(name)
    Ps, imgs = s["Ps"], s["imgs"]
    if name == "angulated":
        i, j = next(p for p in select_pairs(name) if "epipole_inside" in classes_of(name, *p))
    else:
        # far epipoles, and the first line of the grid crosses both detectors: the prefix of length 1 is not a line that misses
        i, j = next((c["i"], c["j"]) for c in catalogue(name)
                    if "epipole_inside" not in c["classes"] and c["first_line_inside"] and (c["i"], c["j"]) in select_pairs(name))
    m = E.MetricDirect(gpu_ctx, Ps, imgs)
    _, a, _ = check_pair(m, Ps, imgs, i, j, fbcc)
    n = len(a["kappas"])
    assert n > 513

    def same_as(got, index):
        for key in ("redundant_samples0", "redundant_samples1", "lines", "kappas"):
            assert np.array_equal(_bits(got[key]), _bits(a[key][index])), key

    perm = np.random.default_rng(11).permutation(n)
    grids = [("permuted", perm), ("permuted, reversed", perm[::-1]), ("reversed", np.arange(n)[::-1])]
    grids += [("prefix %d" % k, np.arange(k)) for k in (1, 255, 256, 257, 513)]
    grids += [("every value twice", np.repeat(np.arange(n), 2))]
    figs = []
    for label, index in grids:
        print(label)
        _, got, fig = check_pair(m, Ps, imgs, i, j, fbcc, kappas=a["kappas"][index])
        same_as(got, index)
        figs.append(fig)
    if name == "scattered":
        # 0.3 rad beyond the range on both sides, 64 planes each: the planes no longer meet the object, most of their lines
        # miss the detector and give exactly 0 (asserted for every line that fails the clip test in check_pair)
        k_max = dt.plane_range(Ps[i], Ps[j], s["n_u"], s["n_v"], s["radius"])[0]
        assert k_max < 1.0
        beyond = np.linspace(0.0, 0.3, 65)[1:].astype(np.float32)
        grid = np.concatenate([(-k_max - beyond[::-1]).astype(np.float32), a["kappas"], (k_max + beyond).astype(np.float32)])
        _, got, fig = check_pair(m, Ps, imgs, i, j, fbcc, kappas=grid)
        same_as({k: v[64:64 + n] for k, v in got.items()}, np.arange(n))
        miss = ~(dt.clip_f32(got["lines"][:, :3], s["n_u"], s["n_v"])["inside"])
        assert miss[:64].sum() + miss[-64:].sum() >= 32 and np.all(got["redundant_samples0"][miss] == 0)
        figs.append(fig)
    _report("%s (%d, %d)" % (name, i, j), figs)
    m.close()


@pytest.mark.parametrize("size", [(384, 384), (383, 384), (384, 383), (385, 384), (1024, 384)])
def test_either_side_of_the_slab_threshold(gpu_ctx, size):
    """Images with a side below DIRECT_SLAB_MIN_SIZE = 384 take the gather kernel, the others the slab kernel: the same
    per-line statement on both sides, in both forms, with a non-square image on each side.  Measured on the MI355X: bit-equal
    rows 1.0000 and worst line difference 0.000 bars at every size; zero share at most 7.3 %."""
    import epipolarconsistency_amd as E
    s = scene("rolled", 4, size)
    assert s["imgs"].shape == (4, size[1], size[0])
    m = E.MetricDirect(gpu_ctx, s["Ps"], s["imgs"])
    figs = [check_pair(m, s["Ps"], s["imgs"], i, j, fbcc)[2] for fbcc in (False, True) for (i, j) in ((0, 3), (1, 2))]
    _report("rolled at %d x %d" % size, figs)
    m.close()


def test_a_pair_without_a_baseline(gpu_ctx):
    """The same matrix and image as two views: no baseline, no epipolar planes -- 0 lines and a metric of exactly 0, from the
    oracle and from the device; the sum over a set that contains the duplicate is that of the other pairs."""
    import epipolarconsistency_amd as E
    import oracle
    s = scene("angulated", 4)
    Ps = [s["Ps"][0], s["Ps"][1], s["Ps"][0].copy(), s["Ps"][3]]
    imgs = np.ascontiguousarray(s["imgs"][[0, 1, 0, 3]])
    want = oracle.direct_pair(Ps[0], Ps[2], imgs[0], imgs[2], 0.0, s["radius"])
    assert len(want["kappas"]) == 0 and want["metric"] == 0.0
    m = E.MetricDirect(gpu_ctx, Ps, imgs)
    for fbcc in (False, True):
        val, got, _ = check_pair(m, Ps, imgs, 0, 2, fbcc)
        assert val == 0.0 and len(got["kappas"]) == 0 and len(got["redundant_samples0"]) == 0
    m.setFanBeamConsistency(False)
    total = oracle.direct_evaluate(Ps, imgs)
    got = m.evaluate()
    assert np.isfinite(got) and total["cost"][2, 0] == 0.0 and _rel(got, total["sum"]) < 1e-5
    m.close()


def test_the_chosen_pairs_cover_every_class():
    """CPU only: over the five geometries the chosen pairs contain an epipole inside a detector, a workgroup of 256 lines
    with both tile orientations, a pair that never and a pair that only uses the transposed tile; (0, 1) and (0, 11) are
    there unless the cap of 10 cut them."""
    union = set()
    for name in gc.NAMES:
        pairs = select_pairs(name)
        assert 0 < len(pairs) <= 10 and len(set(pairs)) == len(pairs)
        inside = [(c["i"], c["j"]) for c in catalogue(name) if "epipole_inside" in c["classes"]]
        assert all(p in pairs for p in inside[:10])
        for (i, j) in pairs:
            union |= classes_of(name, i, j)
        print(name, pairs, {cls: sum(cls in c["classes"] for c in catalogue(name)) for cls in CLASSES},
              "n_lines %% 256:", sorted({c["n"] % 256 for c in catalogue(name)}))
    assert union == set(CLASSES)
