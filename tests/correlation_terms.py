"""The correlation form of the metric (useCorrelation(true)), stated directly in float64 (plain helper module, imported like
channel_terms and geometry_catalog; numpy only, no GPU).

For the pair i < j, over the pair's kappa grid and both +-kappa samples,

    w_k = K1[7] / kappa_k                       (the reference passes kappa_max / kappa as its "1 / n")
    xx  = sum w (x+^2 + x-^2)      yy = sum w (y+^2 + y-^2)      xy = sum w (x+ y+ + x- y-)
    cc  = xy / (sqrt(xx) sqrt(yy))              value = 1 - cc

x is the signed bilinear sample of view i -- signed by the sample's OWN fold sign where the data are derivative, not signed at all
where they are plain -- and y the same of view j.  (The squared-difference form sees only the product of the two signs; the cross
moment xy is where each sample's own sign matters, and the -kappa sample of a line carries the opposite sign of its +kappa sample.)

cc is invariant to a constant factor on w: what a comparison with this statement can see of the weight is its 1 / kappa SHAPE,
and that the polynomial part and the exact tail of one pair (kappa_max > 0.98) use the SAME factor, since one set of three moments
runs through both.  A library that scaled every weight of every loop by the same number would pass.  Likewise a common factor on x
(or on y) cancels; a sign on single samples does not.

The kappa grid, the taps and the bilinear rule are channel_terms' (SURVEY.md 8(a)/(c)); positions="float32" performs the float32
operations of the reference per sample (and the float32 quotient of the weight), positions="float64" the same mapping in binary64
from the same K01.  Everything after the tap positions and the weight is float64: samples, signs, products, sums, cc.  The pair
geometry K01 comes from oracle.evaluate_all(..., want_K01=True).  The reference rounds the three moments to float before it forms
cc and stores 1 - cc as a float: both are roundings of numbers of the size of 1, 6e-8 each, and are NOT restated;
tests/test_correlation_terms_oracle.py ties the statement to the C oracle, which has them, at 2e-7.

A pair without samples (kappa_max = 0) has cc = 0 / 0: value is NaN here, as in the reference's arithmetic.

`slip` states the mistakes tests/test_correlation_terms_oracle.py feeds to the comparison of tests/test_gpu_correlation.py; it is
for that file alone.

`CASES` is the table of tests/test_gpu_correlation.py.
"""
import functools

import numpy as np

import channel_terms as T

f32 = np.float32
KAPPA_FIT_MAX = f32(0.98)   # csrc/ecc_layout.h: ecc_kappa_fit -- where the polynomial part of a pair ends and its exact tail begins

SLIPS = ("no_weight",        # w = 1
         "no_sign_j",        # the fold sign of view j not applied (derivative data)
         "sign_on_plain",    # the fold signs applied to plain data
         "skip_trip",        # the last 64 samples of the grid left out
         "no_tail",          # the samples at kappa >= 0.98 left out
         "tail_factor")      # the samples at kappa >= 0.98 weighted 1 / kappa: another constant factor than the polynomial part's


def pair_moments(K01, D0, D1, n_u, n_v, derivative=True, positions="float32", slip=None):
    """One pair.  K01: 16 floats; D0, D1: (n_t, n_alpha), view i and view j.  Returns a dict: xx, yy, xy, cc, value = 1 - cc (NaN
    without samples), sign0 / sign1 (2 n_kappa,): the fold sign of every sample of view i / j (+kappa samples, then -kappa;
    independent of `derivative`), fold: channel_terms.fold_class of their product, n_kappa."""
    assert slip is None or slip in SLIPS, slip
    D0, D1 = np.asarray(D0, np.float64)[None], np.asarray(D1, np.float64)[None]
    n_t, n_alpha = D0.shape[1:]
    K01 = np.asarray(K01, f32)
    K0, K1 = K01[:8], K01[8:]
    kappa = T.kappa_grid(K01)
    if slip == "skip_trip":
        kappa = kappa[:max(len(kappa) - 64, 0)]
    elif slip == "no_tail":
        kappa = kappa[kappa < KAPPA_FIT_MAX]
    rt = T.range_t(n_u, n_v, n_t)
    cs, sn = np.cos(kappa.astype(np.float64)), np.sin(kappa.astype(np.float64))
    if positions == "float32":
        taps, cs, sn = T.taps_float32, cs.astype(f32), sn.astype(f32)
        w = (K1[7] / kappa).astype(np.float64)
    elif positions == "float64":
        taps = T.taps_float64
        w = np.float64(K1[7]) / kappa.astype(np.float64)
    else:
        raise ValueError("positions: 'float32' or 'float64'")
    if slip == "no_weight":
        w = np.ones_like(w)
    elif slip == "tail_factor":
        w = np.where(kappa < KAPPA_FIT_MAX, w, w / np.float64(K1[7]))
    sign_i = derivative or slip == "sign_on_plain"
    sign_j = sign_i and slip != "no_sign_j"
    xx = yy = xy = 0.0
    s0, s1 = [], []
    for c in (cs, -cs):
        t0, t1 = taps(K0, n_alpha, n_t, rt, c, sn), taps(K1, n_alpha, n_t, rt, c, sn)
        x, y = T._samples(D0, t0, sign_i)[0], T._samples(D1, t1, sign_j)[0]
        xx += float(np.sum(w * x * x))
        yy += float(np.sum(w * y * y))
        xy += float(np.sum(w * x * y))
        s0.append(t0[0])
        s1.append(t1[0])
    s0, s1 = np.concatenate(s0), np.concatenate(s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = float(np.float64(xy) / (np.sqrt(np.float64(xx)) * np.sqrt(np.float64(yy))))
    return dict(xx=xx, yy=yy, xy=xy, cc=cc, value=1.0 - cc, sign0=s0, sign1=s1, fold=T.fold_class(s0 * s1), n_kappa=len(kappa))


def scan_moments(Ps, host, n_u, n_v, pairs=None, object_radius_mm=0.0, dkappa=0.0, derivative=True, positions="float32", slip=None,
                 K01s=None, other_view=False):
    """pair_moments over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps with the intermediates host
    ((n_t, n_alpha) float32 each).  other_view: view j's DATA are taken from view (j + 1) % n, or (j + 2) % n where that is i (the
    slip "view j's data taken from another view"; the geometry stays the pair's).  Returns a dict of arrays over the listed pairs:
    pairs, ij (P, 2), xx, yy, xy, cc, value, n_kappa, kmax, fold (P,) of fold_class, opposite (P,): the fraction of samples whose
    two fold signs differ; K01s (all pairs), n_pairs; with all pairs listed also mean = sum value / N."""
    import oracle
    n = len(Ps)
    assert len(host) == n
    N = n * (n - 1) // 2
    if K01s is None:
        K01s = oracle.evaluate_all(Ps, host, n_u, n_v, object_radius_mm=object_radius_mm, dkappa=dkappa, is_derivative=derivative,
                                   want_K01=True)["K01s"]
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), fold=[], opposite=np.zeros(len(pairs)), K01s=K01s, n_pairs=N,
               n_kappa=np.zeros(len(pairs), np.int64), kmax=np.asarray(K01s, np.float64)[pairs, 15])
    for key in ("xx", "yy", "xy", "cc", "value"):
        out[key] = np.zeros(len(pairs))
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        dj = j
        if other_view:
            dj = (j + 1) % n if (j + 1) % n != i else (j + 2) % n
        t = pair_moments(K01s[q], host[i], host[dj], n_u, n_v, derivative, positions, slip)
        out["ij"][r] = (i, j)
        for key in ("xx", "yy", "xy", "cc", "value", "n_kappa"):
            out[key][r] = t[key]
        out["fold"].append(t["fold"])
        rel = t["sign0"] * t["sign1"]
        out["opposite"][r] = float((rel < 0).mean()) if len(rel) else 0.0
    out["fold"] = np.array(out["fold"])
    if len(pairs) == N:
        out["mean"] = out["value"].sum() / N
    return out


def distance(got, want):
    """|got - want| per pair, absolutely (the Cauchy-Schwarz scale of cc is 1); where the statement has no value (a pair without
    samples) the other must have none either: 0 if both are NaN, inf otherwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    both = np.isnan(got) & np.isnan(want)
    d = np.abs(got - want)
    return np.where(both, 0.0, np.where(np.isfinite(d), d, np.inf))


# ---- the cases of tests/test_gpu_correlation.py --------------------------------------------------------------------------------
# The data are white noise (standard normal, default_rng(5), a new field per view) made NON-STATIONARY, in one of two ways:
#   ("spikes", fraction, sigma)   on `fraction` of the bins a second normal of `sigma` is added;
#   ("patches", L, g)             the noise is multiplied by exp(g s), s a smooth standard-normal field of correlation length L bins
#                                 (white noise on an L-bin grid, interpolated bilinearly).
# On stationary noise every 64 samples of a pair carry the same share of the moments, and the last ones -- the largest kappa, the
# smallest weight -- so little of it that a dropped trip or a dropped exact tail moves cc by less than 20 x the throughput bar (8-fold
# and 18-fold measured at 768 x 768).  With spikes or patches single samples, or single stretches of a line, carry a visible share
# wherever they fall, the tail included.  Which pairs they fall on is chance: the kind and its two numbers were chosen per case,
# on the CPU, until the statement alone met the factors tests/test_correlation_terms_oracle.py::test_the_comparison_rejects_the_slips
# asserts (spikes of 0.2 % / 40 sigma, the first try, leave case d's dropped tail at 6-fold, case e's dropped trip at 20-fold and
# case f's one tail at 11-fold).
SPIKES = ("spikes", 0.0005, 150.0)
# key: (geometry, views, n_alpha, n_t, object radius mm (0: automatic), dkappa (0: automatic), (derivative, ...), [(sampling, quads)],
#       data)
CASES = {
    "a": ("mirrored", 16, 768, 768, 0.0, 0.0, (True,), [("polynomial", "off"), ("polynomial", "on"), ("per_sample", "off")], SPIKES),
    # a 10-mm object: ranges of 0.013 .. 0.19 rad, where the fit's degree is lowered to 4 and 6
    "a2": ("mirrored", 16, 768, 768, 10.0, 0.0, (True,), [("polynomial", "off")], SPIKES),
    "b": ("near_opposite", 16, 768, 768, 185.0, 0.0, (True,), [("polynomial", "off"), ("polynomial", "on"), ("per_sample", "off")], SPIKES),
    # plain data.  On `near_opposite` the two fold signs of a pair are equal on every sample, so signs applied to BOTH views of plain
    # data cancel in all three moments: c sees a sign on one view only, c2 (the scan of a: 46 opposite and 9 mixed pairs) sees both.
    "c": ("near_opposite", 16, 768, 768, 185.0, 0.0, (False,), [("polynomial", "off")], SPIKES),
    "c2": ("mirrored", 16, 768, 768, 0.0, 0.0, (False,), [("polynomial", "off"), ("per_sample", "off")], SPIKES),
    # scattered: see channel_terms.CASES g for the 450-mm object.  735 distance bins: a row pitch other than the 768-bin grid's
    # (767 bins have the same).  Every fit of d is refused (MI355X), so both its samplings run the exact loop; d2 (a 50-mm
    # object, ranges up to 0.11 rad) has the fits: degrees 6 and 8
    "d": ("scattered", 16, 1000, 735, 450.0, 0.0, (True,), [("polynomial", "auto"), ("per_sample", "auto")], ("patches", 48, 2.0)),
    "d2": ("scattered", 16, 1000, 735, 50.0, 0.0, (True,), [("polynomial", "auto")], ("patches", 48, 2.0)),
    "e": ("angulated", 4, 2621, 768, 0.0, 0.0, (True,), [("polynomial", "auto")], SPIKES),
    # a 25-mm object: degrees 6 and 8, both wide-offset loops
    "e2": ("angulated", 4, 2621, 768, 25.0, 0.0, (True,), [("polynomial", "auto")], ("patches", 24, 1.5)),
    "f": ("mirrored", 12, 96, 64, 60.0, 0.004, (True, False), [("polynomial", "auto"), ("reference", "auto")], ("patches", 24, 1.5)),
    "g": ("mirrored", 8, 96, 64, 0.0, 0.0, (True, False), [("auto", "auto")], SPIKES),
    "h": ("mirrored", 40, 96, 64, 0.0, 0.0, (True,), [("reference", "auto")], SPIKES),
    "i": ("mirrored", 66, 32, 32, 0.0, 0.0, (True,), [("reference", "auto")], SPIKES),
}


def _smooth(rng, shape, L):
    """White noise on an L-bin grid, interpolated bilinearly to `shape`."""
    g = rng.standard_normal((shape[0] // L + 3, shape[1] // L + 3))
    y, x = np.arange(shape[0]) / L, np.arange(shape[1]) / L
    iy, ix = y.astype(np.int64), x.astype(np.int64)
    fy, fx = (y - iy)[:, None], (x - ix)[None, :]
    return ((1 - fy) * ((1 - fx) * g[iy][:, ix] + fx * g[iy][:, ix + 1]) + fy * ((1 - fx) * g[iy + 1][:, ix] + fx * g[iy + 1][:, ix + 1]))


def field(rng, shape, data):
    """One view's intermediate, float64 (see above)."""
    h = rng.standard_normal(shape)
    if data[0] == "spikes":
        where = rng.random(shape) < data[1]
        return h + data[2] * where * rng.standard_normal(shape)
    assert data[0] == "patches", data
    return h * np.exp(data[2] * _smooth(rng, shape, data[1]))


def tolerance(sampling, n_pairs):
    """The per-pair bar on |got - (1 - cc)|: channel_terms' bars, absolute."""
    return T.tolerance(sampling, n_pairs)


def case_pairs(key):
    """The pairs the statement evaluates: all, but for case i (2 145 pairs): the subset of channel_terms.case_pairs("e")."""
    return T.case_pairs("e") if key == "i" else None


@functools.lru_cache(maxsize=3)
def case_data(key):
    """(Ps, n_u, n_v, host): the scan of a case and its n float32 intermediates.  Cached: shared, not to be changed."""
    import geometry_catalog
    name, n, n_alpha, n_t = CASES[key][:4]
    data = CASES[key][8]
    for other in sorted(CASES):
        if other < key and CASES[other][:4] + (CASES[other][8],) == CASES[key][:4] + (data,):
            return case_data(other)
    Ps, n_u, n_v = geometry_catalog.make(name, n)
    rng = np.random.default_rng(5)
    return Ps, n_u, n_v, [field(rng, (n_t, n_alpha), data).astype(np.float32) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def case_terms(key, derivative=True, positions="float32"):
    """scan_moments of a case for one of its data kinds (cached)."""
    name, n, n_alpha, n_t, radius, dkappa, kinds = CASES[key][:7]
    assert derivative in kinds
    Ps, n_u, n_v, host = case_data(key)
    return scan_moments(Ps, host, n_u, n_v, pairs=case_pairs(key), object_radius_mm=radius, dkappa=dkappa, derivative=derivative,
                        positions=positions)
