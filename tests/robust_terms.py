"""The per-pair sums of the metric under a per-sample robust loss, stated directly in float64 (plain helper module, imported like
channel_terms and weighted_terms; numpy only, no GPU).

A metric over one Radon intermediate per view.  For the pair i < j, with w06 = K0[6] dkappa and the sums over both +-kappa samples of
the pair's kappa grid (n_kappa steps, 2 n_kappa samples),

    d  = v0 - v1                       the difference of the two data samples, signed by the folds when `derivative` is set
    w  = w(d)                          the IRLS weight of the loss at the scale delta, in (0, 1]:
           huber           1 for |d| <= delta, else t (2 - t), t = delta / |d|        rho = d^2 | 2 delta |d| - delta^2
           truncated       1 for |d| <= delta, else t^2                               rho = min(d^2, delta^2)
           geman_mcclure   1 / (1 + (d / delta)^2)                                    rho = d^2 delta^2 / (delta^2 + d^2)
    c  = w06 sum w d^2                 (column 0 of evaluate_robust's pair rows)
    u  = sum w / (2 n_kappa)           (column 1: the inlier mass; a pair without samples has {0, 1, 0})
    r  = sum d^2 / (2 n_kappa)         (column 2: the mean squared raw residual, no loss and no delta in it)
    s  = w06 sum d^2                   (the scale of c: no weight in (0, 1] can make c larger; in r's units it is r itself)

The kappa grid, the tap positions and the bilinear rule are channel_terms' (kappa_grid, range_t, taps_float32 / taps_float64,
_samples); everything behind the tap positions is float64.  `SLIPS` are the mistakes the comparison of tests/test_gpu_robust.py must
reject (tests/test_robust_terms_oracle.py shows that it does).

The cases are weighted_terms.CASES (labels a .. j of DESIGN.md 4.15 / 4.19) with the data of channel 0.  Every case has two scales,
each rounded to float32: the median and the 90th percentile of |d| over the case's samples in the float32-position statement, so
that half, or a tenth, of the samples lie outside delta."""
import functools

import numpy as np

from channel_terms import _samples, kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T
import weighted_terms as W

f32 = np.float32

CASES = W.CASES
LOSSES = ("huber", "truncated", "geman_mcclure")          # the codes 0, 1, 2 of ECC_LOSS_* in this order
SCALES = ("median", "p90")
OUTSIDE = {"median": 0.5, "p90": 0.1}                      # the share of samples with |d| > delta, by construction

# slip -> the losses it changes (the others are untouched by it)
SLIPS = {"huber_without_offset": ("huber",), "threshold_on_square": ("huber", "truncated"), "w_plus_for_both": LOSSES,
         "loss_of_the_step": LOSSES, "u_counts_inliers": LOSSES, "gm_first_power": ("geman_mcclure",)}


def loss_weight(a, loss, delta, slip=None):
    """w(|d|) in float64.  a: |d| >= 0; delta > 0, inf allowed."""
    a = np.asarray(a, np.float64)
    delta = float(delta)
    if loss == "geman_mcclure":
        q = a / delta
        return 1.0 / (1.0 + q) if slip == "gm_first_power" else 1.0 / (1.0 + q * q)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(a > 0, delta / np.where(a > 0, a, 1.0), np.inf)
    inlier = (a * a <= delta) if slip == "threshold_on_square" else (a <= delta)
    t = np.where(np.isfinite(t), t, 1.0)
    if loss == "huber":
        out = 2.0 * t if slip == "huber_without_offset" else t * (2.0 - t)
    elif loss == "truncated":
        out = t * t
    else:
        raise ValueError("loss: one of %s" % (LOSSES,))
    return np.where(inlier, 1.0, out)


def pair_residuals(K01, D0, D1, n_u, n_v, derivative=True, positions="float32"):
    """One pair: (d, w06).  d (2 n_kappa,) float64: the residual of every sample, +kappa samples first, then -kappa; w06 = K0[6]
    dkappa.  K01: 16 floats; D0, D1: (n_t, n_alpha), the data of view i and of view j."""
    D0, D1 = np.asarray(D0, np.float64)[None], np.asarray(D1, np.float64)[None]
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
    d = []
    for c in (cs, -cs):
        t0, t1 = taps(K0, n_alpha, n_t, rt, c, sn), taps(K1, n_alpha, n_t, rt, c, sn)
        d.append(_samples(D0, t0, derivative)[0] - _samples(D1, t1, derivative)[0])
    return np.concatenate(d), float(K0[6]) * float(K1[6])


def terms_of(d, w06, loss, delta, slip=None):
    """{c, u, r, s, n_kappa, outside} of one pair from its residuals.  outside: the number of samples with |d| > delta."""
    n2 = len(d)
    n_kappa = n2 // 2
    if n2 == 0:
        return dict(c=0.0, u=1.0, r=0.0, s=0.0, n_kappa=0, outside=0)
    a = np.abs(d)
    if slip == "loss_of_the_step":
        step = np.sqrt(d[:n_kappa] ** 2 + d[n_kappa:] ** 2)
        w = np.tile(loss_weight(step, loss, delta), 2)
    else:
        w = loss_weight(a, loss, delta, slip)
    if slip == "w_plus_for_both":
        w = np.tile(w[:n_kappa], 2)
    sq = d * d
    u = float((a <= delta).mean()) if slip == "u_counts_inliers" else float(w.sum()) / n2
    return dict(c=w06 * float(w @ sq), u=u, r=float(sq.sum()) / n2, s=w06 * float(sq.sum()), n_kappa=n_kappa, outside=int((a > delta).sum()))


def scan_residuals(Ps, data, n_u, n_v, K01s, pairs=None, derivative=True, positions="float32"):
    """pair_residuals over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps with one field per view.
    Returns a dict: pairs (P,), ij (P, 2), d (list of P arrays), w06 (P,), n_pairs."""
    import oracle
    n = len(Ps)
    assert len(data) >= n
    N = n * (n - 1) // 2
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), d=[], w06=np.zeros(len(pairs)), n_pairs=N)
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        d, w06 = pair_residuals(K01s[q], data[i], data[j], n_u, n_v, derivative, positions)
        out["ij"][r] = (i, j)
        out["d"].append(d)
        out["w06"][r] = w06
    return out


def scan_terms(res, loss, delta, slip=None):
    """terms_of over the pairs of scan_residuals' result.  Returns a dict of arrays over the listed pairs: pairs, ij, c, u, r, s,
    n_kappa, outside; with all pairs listed also value = sum c / N and inlier_mass = sum u / N."""
    P = len(res["pairs"])
    out = dict(pairs=res["pairs"], ij=res["ij"], n_pairs=res["n_pairs"], c=np.zeros(P), u=np.zeros(P), r=np.zeros(P), s=np.zeros(P),
               n_kappa=np.zeros(P, np.int64), outside=np.zeros(P, np.int64))
    for k in range(P):
        t = terms_of(res["d"][k], res["w06"][k], loss, delta, slip)
        for key in ("c", "u", "r", "s", "n_kappa", "outside"):
            out[key][k] = t[key]
    if P == res["n_pairs"]:
        out.update(value=out["c"].sum() / P, inlier_mass=out["u"].sum() / P)
    return out


def columns(t):
    """The oracle's terms in the layout of evaluate_robust's pair rows, (P, 3): c, u, r -- and their scales: s for c, 1 for u, and
    for r the same raw sum in r's units, s / (w06 2 n_kappa) = r."""
    return np.stack([t["c"], t["u"], t["r"]], axis=1), np.stack([t["s"], np.ones(len(t["s"])), t["r"]], axis=1)


def robust_scale(r, k=1.0):
    """ecc_host_robust_scale in numpy: k x the median of sqrt(r_q) over the pairs with r_q > 0; none: 0."""
    r = np.asarray(r, np.float64)
    live = r[r > 0]
    return float(k * np.median(np.sqrt(live))) if len(live) else 0.0


@functools.lru_cache(maxsize=8)
def case_residuals(label, positions="float32"):
    """scan_residuals of a case (cached; cases a, b and c share one scan and use the entry of a)."""
    for other in sorted(CASES):
        if other < label and W.settings(other)[:7] == W.settings(label)[:7]:
            return case_residuals(other, positions)
    Ps, n_u, n_v, data, _, K01s = W.case_inputs(label)
    return scan_residuals(Ps, data, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=W.settings(label)[6], positions=positions)


@functools.lru_cache(maxsize=None)
def case_delta(label, scale):
    """The scale of a case, a float32: the median ("median") or the 90th percentile ("p90") of |d| over the samples of its listed
    pairs in the float32-position statement."""
    a = np.abs(np.concatenate(case_residuals(label)["d"]))
    return f32(np.median(a) if scale == "median" else np.percentile(a, 90.0))


@functools.lru_cache(maxsize=None)
def _case_terms(label, loss, scale, positions):
    return scan_terms(case_residuals(label, positions), loss, float(case_delta(label, scale)))


def case_terms(label, loss, scale, positions="float32"):
    """scan_terms of a case at one of its two scales (cached; the arrays are shared and must not be changed)."""
    return _case_terms(label, loss, scale, positions)
