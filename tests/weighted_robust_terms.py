"""The per-pair sums of the metric with per-line weights AND a per-sample robust loss, stated directly in float64 (plain helper
module, imported like channel_terms, weighted_terms and robust_terms; numpy only, no GPU).

A metric over 2 n Radon intermediates: the data D_i of view i and its line weights W_i on the same bin grid.  For the pair i < j, with
w06 = K0[6] dkappa and the sums over both +-kappa samples of the pair's kappa grid (n_kappa steps, 2 n_kappa samples),

    d  = v0 - v1                       the residual of weighted_terms.pair_terms (signed by the folds when `derivative` is set)
    mu = W_i(sample) W_j(sample)       its mu: the two weight samples at the same taps as the data, NEVER signed
    w  = robust_terms.loss_weight(|d|) the IRLS weight of the RAW residual at the scale delta: a line weight says how far a line is
                                       trusted, it does not rescale its residual
    c  = w06 sum mu w d^2              (column 0 of evaluate_weighted_robust's pair rows)
    u  = sum mu / (2 n_kappa)          (column 1: the coverage)
    k  = sum mu w / (2 n_kappa)        (column 2: the weight mass the loss keeps, k <= u)
    r  = sum mu d^2 / (2 n_kappa)      (column 3: the weighted mean squared raw residual, no loss and no delta in it)
    s  = w06 sum d^2                   (the scale of c: no weight in [0, 1] can make c larger)
    a pair without samples has {0, 1, 1, 0}

and over all pairs value = sum c / sum u, coverage = sum u / N, inlier_mass = sum k / sum u (sum u == 0: all 0).  The scales of the
comparison: s for c, 1 for u and k, and for r the unweighted raw mean sum d^2 / (2 n_kappa), which no weight in [0, 1] exceeds.

The kappa grid, the tap positions and the bilinear rule are channel_terms' (kappa_grid, range_t, taps_float32 / taps_float64,
_samples); everything behind the tap positions is float64.  `SLIPS` are the mistakes the comparison of
tests/test_gpu_weighted_robust.py must reject (tests/test_weighted_robust_terms_oracle.py shows that it does).

The cases are weighted_terms.CASES with weighted_terms.case_inputs' weights; the scales robust_terms.case_delta(label, "median" |
"p90") -- the median and the 90th percentile of |d| over ALL samples of the case, whatever their weight."""
import functools

import numpy as np

from channel_terms import _samples, kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T
import robust_terms as R
import weighted_terms as W

f32 = np.float32

CASES = W.CASES
LOSSES = R.LOSSES
SCALES = R.SCALES

# per-pair slips change columns; scan slips change value / inlier_mass alone
PAIR_SLIPS = ("w_of_weighted_residual", "k_without_mu", "r_without_mu", "wj_from_view_i")
SCAN_SLIPS = ("inlier_mass_over_n_pairs", "value_over_kept")
SLIPS = PAIR_SLIPS + SCAN_SLIPS


def pair_samples(K01, D0, D1, W0, W1, n_u, n_v, derivative=True, positions="float32"):
    """One pair: (d, mu, w06).  d, mu (2 n_kappa,) float64: the residual and the weight product of every sample as
    weighted_terms.pair_terms forms them, +kappa samples first, then -kappa; w06 = K0[6] dkappa."""
    D0, D1 = np.asarray(D0, np.float64)[None], np.asarray(D1, np.float64)[None]
    W0, W1 = np.asarray(W0, np.float64)[None], np.asarray(W1, np.float64)[None]
    _, n_t, n_alpha = D0.shape
    K01 = np.asarray(K01, f32)
    K0, K1 = K01[:8], K01[8:]
    kappa = kappa_grid(K01)
    rt = range_t(n_u, n_v, n_t)
    cs, sn = np.cos(kappa.astype(np.float64)), np.sin(kappa.astype(np.float64))
    if positions == "float32":
        taps, cs, sn = taps_float32, cs.astype(f32), sn.astype(f32)
    elif positions == "float64":
        taps = taps_float64
    else:
        raise ValueError("positions: 'float32' or 'float64'")
    d, mu = [], []
    for c in (cs, -cs):
        t0, t1 = taps(K0, n_alpha, n_t, rt, c, sn), taps(K1, n_alpha, n_t, rt, c, sn)
        d.append(_samples(D0, t0, derivative)[0] - _samples(D1, t1, derivative)[0])
        mu.append(_samples(W0, t0, False)[0] * _samples(W1, t1, False)[0])   # unsigned always
    return np.concatenate(d), np.concatenate(mu), float(K0[6]) * float(K1[6])


def terms_of(d, mu, w06, loss, delta, slip=None):
    """{c, u, k, r, s, raw, n_kappa} of one pair from its residuals and weight products.  raw: sum d^2 / (2 n_kappa), r's scale."""
    n2 = len(d)
    if n2 == 0:
        return dict(c=0.0, u=1.0, k=1.0, r=0.0, s=0.0, raw=0.0, n_kappa=0)
    sq = d * d
    a = np.sqrt(mu) * np.abs(d) if slip == "w_of_weighted_residual" else np.abs(d)
    w = R.loss_weight(a, loss, delta)
    f = mu * w
    return dict(c=w06 * float(f @ sq), u=float(mu.sum()) / n2, k=float((w if slip == "k_without_mu" else f).sum()) / n2,
                r=float(sq.sum() if slip == "r_without_mu" else mu @ sq) / n2, s=w06 * float(sq.sum()), raw=float(sq.sum()) / n2,
                n_kappa=n2 // 2)


def scan_samples(Ps, data, weights, n_u, n_v, K01s, pairs=None, derivative=True, positions="float32", slip=None):
    """pair_samples over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps.  Returns a dict: pairs (P,),
    ij (P, 2), d, mu (lists of P arrays), w06 (P,), n_pairs.  slip "wj_from_view_i": the weight of view j taken from view i."""
    import oracle
    n = len(Ps)
    assert len(data) >= n and len(weights) == n
    N = n * (n - 1) // 2
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), d=[], mu=[], w06=np.zeros(len(pairs)), n_pairs=N)
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        d, mu, w06 = pair_samples(K01s[q], data[i], data[j], weights[i], weights[i if slip == "wj_from_view_i" else j], n_u, n_v,
                                  derivative, positions)
        out["ij"][r] = (i, j)
        out["d"].append(d)
        out["mu"].append(mu)
        out["w06"][r] = w06
    return out


def scan_terms(smp, loss, delta, slip=None):
    """terms_of over the pairs of scan_samples' result.  Returns a dict of arrays over the listed pairs: pairs, ij, c, u, k, r, s, raw,
    n_kappa; with all pairs listed also value = sum c / sum u, coverage = sum u / N and inlier_mass = sum k / sum u (sum u == 0: all
    0).  (slip "wj_from_view_i" is scan_samples'.)"""
    P = len(smp["pairs"])
    keys = ("c", "u", "k", "r", "s", "raw")
    out = dict(pairs=smp["pairs"], ij=smp["ij"], n_pairs=smp["n_pairs"], n_kappa=np.zeros(P, np.int64), **{key: np.zeros(P) for key in keys})
    for q in range(P):
        t = terms_of(smp["d"][q], smp["mu"][q], smp["w06"][q], loss, delta, slip if slip in PAIR_SLIPS else None)
        for key in keys + ("n_kappa",):
            out[key][q] = t[key]
    if P == smp["n_pairs"]:
        su, sk, sc = out["u"].sum(), out["k"].sum(), out["c"].sum()
        if su:
            out.update(value=sc / (sk if slip == "value_over_kept" else su), coverage=su / P,
                       inlier_mass=sk / (P if slip == "inlier_mass_over_n_pairs" else su))
        else:
            out.update(value=0.0, coverage=0.0, inlier_mass=0.0)
    return out


def columns(t):
    """The oracle's terms in the layout of evaluate_weighted_robust's pair rows, (P, 4): c, u, k, r -- and their scales: s for c, 1 for
    u and k, the unweighted raw mean for r."""
    one = np.ones(len(t["s"]))
    return np.stack([t["c"], t["u"], t["k"], t["r"]], axis=1), np.stack([t["s"], one, one, t["raw"]], axis=1)


def means(t):
    """(value, coverage, inlier_mass) of a scan with all pairs listed."""
    return np.array([t["value"], t["coverage"], t["inlier_mass"]])


def weighted_robust_scale(rows, k=1.0):
    """ecc_host_weighted_robust_scale in numpy: k x the median of sqrt(r_q / u_q) over the rows {c, u, k, r} with r_q > 0 and
    u_q > 0; none: 0."""
    rows = np.asarray(rows, np.float64)
    live = (rows[:, 3] > 0) & (rows[:, 1] > 0)
    return float(k * np.median(np.sqrt(rows[live, 3] / rows[live, 1]))) if live.any() else 0.0


@functools.lru_cache(maxsize=8)
def case_samples(label, positions="float32"):
    """scan_samples of a case with its weights (cached; cases a, b and c share one scan and use the entry of a)."""
    for other in sorted(CASES):
        if other < label and W.settings(other)[:7] == W.settings(label)[:7]:
            return case_samples(other, positions)
    Ps, n_u, n_v, data, weights, K01s = W.case_inputs(label)
    return scan_samples(Ps, data, weights, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=W.settings(label)[6], positions=positions)


@functools.lru_cache(maxsize=None)
def _case_terms(label, loss, scale, positions):
    return scan_terms(case_samples(label, positions), loss, float(R.case_delta(label, scale)))


def case_terms(label, loss, scale, positions="float32"):
    """scan_terms of a case at one of its two scales (cached; the arrays are shared and must not be changed)."""
    return _case_terms(label, loss, scale, positions)
