"""The per-pair sums of the metric with inverse-variance sample weights, stated directly in float64 (plain helper module, imported
like channel_terms and weighted_terms; numpy only, no GPU).

A metric over 2 n Radon intermediates: the data D_i of view i and its variance field V_i on the same bin grid.  For the pair i < j,
with w = K0[6] dkappa and the sums over both +-kappa samples of the pair's kappa grid (n_kappa steps, 2 n_kappa samples),

    d     = v0 - v1                            the difference of the two data samples, signed by the folds when `derivative` is set
    s     = V_i(sample) + V_j(sample)          the two variance samples at the same taps as the data, NEVER signed
    omega = 1 / max(s, floor)
    c     = w sum omega d^2                    (column 0 of evaluate_variance's pair rows)
    u     = sum omega / (2 n_kappa)            (column 1: the mean weight; a pair without samples has c = 0, u = 1)
    s     = w sum d^2                          (key "s"; the scale of c is s omega_max, that of u omega_max)

omega_max = 1 / max(floor, V_MIN + V_MIN) bounds every sample's weight on the fields below.  The kappa grid, the tap positions and
the bilinear rule are channel_terms' (kappa_grid, range_t, taps_float32 / taps_float64, _samples); everything behind the tap
positions is float64.  `SLIPS` are the mistakes the comparison of tests/test_gpu_variance.py must reject
(tests/test_variance_terms_oracle.py shows that it does).

The cases are weighted_terms.CASES (labels a .. j) with the data of channel 0.  The variance fields of a case come from
default_rng(13): every view's field is tiled with 8 x 8 blocks, each block exactly 0.5, exactly 2.0, or 0.25 * 16^U(0, 1) per bin,
so that flat regions of two levels, steps between them and rough fields over a 16-fold range are all sampled.  Two floors per case:
0.125 is never active (s >= 0.5), 1.5 is active on part of the samples."""
import functools

import numpy as np

from channel_terms import _samples, kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T
import weighted_terms as W

f32 = np.float32

CASES = W.CASES
settings = W.settings
FLOORS = (0.125, 1.5)
V_MIN = 0.25   # the least entry of variance_fields

SLIPS = ("vj_from_view_i", "fold_sign_on_variances", "omega_plus_for_both", "product_of_variances", "sum_of_reciprocals", "floor_added",
         "mean_weight_over_n_kappa")


def omega_max(floor):
    """No sample's weight exceeds this on variance_fields: s >= 2 V_MIN."""
    return 1.0 / max(float(floor), 2 * V_MIN)


def variance_fields(n, n_t, n_alpha, seed=13):
    """n float32 fields (n_t, n_alpha): 8 x 8 blocks of side ceil(n / 8) per view, each of one kind -- 0: exactly 0.5, 1: exactly 2.0,
    2: 0.25 * 16^U(0, 1) per bin, in [0.25, 4)."""
    rng = np.random.default_rng(seed)
    bt, ba = -(-n_t // 8), -(-n_alpha // 8)
    out = []
    for _ in range(n):
        kinds = rng.integers(0, 3, (8, 8))
        rough = np.maximum((0.25 * 16.0 ** rng.random((n_t, n_alpha))).astype(f32), f32(V_MIN))
        kind = np.repeat(np.repeat(kinds, bt, axis=0), ba, axis=1)[:n_t, :n_alpha]
        out.append(np.where(kind == 2, rough, np.where(kind == 1, f32(2.0), f32(0.5))).astype(f32))
    return out


def pair_terms(K01, D0, D1, V0, V1, floor, n_u, n_v, derivative=True, positions="float32", slip=None):
    """One pair.  K01: 16 floats; D0, D1, V0, V1: (n_t, n_alpha), data and variance fields of view i and of view j; floor > 0.
    Returns a dict: c, u, s, n_kappa, rel_sign (2 n_kappa,): the product of the two fold signs per sample (+kappa samples, then
    -kappa).  slip: one of SLIPS (vj_from_view_i is the caller's: it passes V_i twice)."""
    D0, D1 = np.asarray(D0, np.float64)[None], np.asarray(D1, np.float64)[None]
    V0, V1 = np.asarray(V0, np.float64)[None], np.asarray(V1, np.float64)[None]
    _, n_t, n_alpha = D0.shape
    K01 = np.asarray(K01, f32)
    K0, K1 = K01[:8], K01[8:]
    kappa = kappa_grid(K01)
    w = float(K0[6]) * float(K1[6])
    rt = range_t(n_u, n_v, n_t)
    floor = float(floor)
    cs, sn = np.cos(kappa.astype(np.float64)), np.sin(kappa.astype(np.float64))
    if positions == "float32":
        taps, cs, sn = taps_float32, cs.astype(f32), sn.astype(f32)
    elif positions == "float64":
        taps = taps_float64
    else:
        raise ValueError("positions: 'float32' or 'float64'")
    v0, v1, m0, m1, rel = [], [], [], [], []
    for c in (cs, -cs):
        t0, t1 = taps(K0, n_alpha, n_t, rt, c, sn), taps(K1, n_alpha, n_t, rt, c, sn)
        v0.append(_samples(D0, t0, derivative)[0])
        v1.append(_samples(D1, t1, derivative)[0])
        signed = slip == "fold_sign_on_variances" and derivative
        m0.append(_samples(V0, t0, signed)[0])   # unsigned always
        m1.append(_samples(V1, t1, signed)[0])
        rel.append(t0[0] * t1[0])
    n_kappa = len(kappa)
    v0, v1, m0, m1 = (np.concatenate(x) for x in (v0, v1, m0, m1))   # (2 n_kappa,)
    d = v0 - v1
    if slip == "product_of_variances":
        omega = 1.0 / np.maximum(m0 * m1, floor)
    elif slip == "sum_of_reciprocals":
        omega = 1.0 / np.maximum(m0, floor) + 1.0 / np.maximum(m1, floor)
    elif slip == "floor_added":
        omega = 1.0 / (m0 + m1 + floor)
    else:
        omega = 1.0 / np.maximum(m0 + m1, floor)
    if slip == "omega_plus_for_both":
        omega = np.concatenate([omega[:n_kappa], omega[:n_kappa]])
    s = w * float(d @ d)
    c_val = w * float(omega @ (d * d))
    if n_kappa == 0:
        u = 1.0
    else:
        u = float(omega.sum()) / (n_kappa if slip == "mean_weight_over_n_kappa" else 2 * n_kappa)
    return dict(c=c_val, u=u, s=s, n_kappa=n_kappa, rel_sign=np.concatenate(rel))


def scan_terms(Ps, data, variances, floor, n_u, n_v, K01s, pairs=None, derivative=True, positions="float32", slip=None):
    """pair_terms over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps.  data, variances: n fields each.
    Returns a dict of arrays over the listed pairs: pairs, ij (P, 2), c, u, s, n_kappa, fold (channel_terms.fold_class), opposite (the
    fraction of samples with opposite fold signs); with all
    pairs listed also value = sum c / sum u and mean_weight = sum u / N (sum u == 0: both 0)."""
    import oracle
    n = len(Ps)
    assert len(data) == n and len(variances) == n
    N = n * (n - 1) // 2
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), c=np.zeros(len(pairs)), u=np.zeros(len(pairs)), s=np.zeros(len(pairs)),
               n_kappa=np.zeros(len(pairs), np.int64), fold=[], opposite=np.zeros(len(pairs)), n_pairs=N, floor=float(floor))
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        t = pair_terms(K01s[q], data[i], data[j], variances[i], variances[i if slip == "vj_from_view_i" else j], floor, n_u, n_v,
                       derivative, positions, slip)
        out["ij"][r] = (i, j)
        for key in ("c", "u", "s", "n_kappa"):
            out[key][r] = t[key]
        out["fold"].append(T.fold_class(t["rel_sign"]))
        out["opposite"][r] = float((t["rel_sign"] < 0).mean()) if len(t["rel_sign"]) else 0.0
    out["fold"] = np.array(out["fold"])
    if len(pairs) == N:
        su = out["u"].sum()
        out.update(value=out["c"].sum() / su if su else 0.0, mean_weight=su / N if su else 0.0)
    return out


def columns(t):
    """The statement's terms in the layout of evaluate_variance's pair rows, (P, 2): c, u -- and their scales on variance_fields:
    s omega_max for c, omega_max for u."""
    om = omega_max(t["floor"])
    return np.stack([t["c"], t["u"]], axis=1), np.stack([t["s"] * om, np.full(len(t["s"]), om)], axis=1)


def _earlier(label):
    for other in sorted(CASES):
        if other < label and settings(other)[:7] == settings(label)[:7]:
            return other
    return None


@functools.lru_cache(maxsize=2)
def case_inputs(label):
    """(Ps, n_u, n_v, data, variances, K01s) of a case: scan, data and pair geometry are weighted_terms.case_inputs', the variances
    variance_fields.  Cached: the arrays are shared and must not be changed."""
    if _earlier(label):
        return case_inputs(_earlier(label))
    Ps, n_u, n_v, data, _, K01s = W.case_inputs(label)
    _, n, n_alpha, n_t = settings(label)[:4]
    return Ps, n_u, n_v, data, variance_fields(n, n_t, n_alpha), K01s


@functools.lru_cache(maxsize=32)
def case_terms(label, floor, positions="float32"):
    """scan_terms of a case with its variance fields at `floor` (cached; cases a, b and c share one scan and use the entry of a)."""
    if _earlier(label):
        return case_terms(_earlier(label), floor, positions)
    Ps, n_u, n_v, data, variances, K01s = case_inputs(label)
    return scan_terms(Ps, data, variances, floor, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=settings(label)[6],
                      positions=positions)


# ---- the demonstration of DESIGN.md 4.28 -----------------------------------------------------------------------------------------
DEMO_VIEW, DEMO_SIGMA, DEMO_BINS, DEMO_FLOOR_FRACTION = 3, 0.05, 96, 1e-3


def demo_images(imgs):
    """(noisy images, pixel-variance images) of the 8-view sphere scan `imgs`: Gaussian noise of sigma = 5 % of the view's maximum on
    the left half of view 3 only (default_rng(5)); the variance image is sigma^2 there and 0 elsewhere."""
    imgs = np.asarray(imgs, np.float32)
    n, n_v, n_u = imgs.shape
    sigma = DEMO_SIGMA * float(imgs[DEMO_VIEW].max())
    noisy = imgs.copy()
    noise = np.random.default_rng(5).standard_normal((n_v, n_u // 2)) * sigma
    noisy[DEMO_VIEW][:, :n_u // 2] = (imgs[DEMO_VIEW][:, :n_u // 2].astype(np.float64) + noise).astype(f32)
    var = np.zeros_like(imgs)
    var[DEMO_VIEW][:, :n_u // 2] = f32(sigma * sigma)
    return noisy, var


def demo_floor(variances):
    """DEMO_FLOOR_FRACTION x the median of the positive entries of V of the noisy view, as float32 (ecc_host_variance_floor's rule)."""
    v = np.asarray(variances[DEMO_VIEW], f32).reshape(-1)
    return float(f32(DEMO_FLOOR_FRACTION * float(np.median(v[v > 0].astype(np.float64)))))


def demo_ratios(Ps, clean, noisy, variances, floor, n_u, n_v, K01s_clean, K01s_noisy):
    """(plain clean, plain noisy, variance clean, variance noisy): evaluate() as mean of s, evaluate_variance's value as sum c / sum u,
    both by the statement, on the clean and the noisy intermediates with the same variance fields."""
    out = []
    for data, K01s in ((clean, K01s_clean), (noisy, K01s_noisy)):
        t = scan_terms(Ps, data, variances, floor, n_u, n_v, K01s)
        out.append((t["s"].sum() / t["n_pairs"], t["value"]))
    return out[0][0], out[1][0], out[0][1], out[1][1]
