"""The per-pair sums of the metric with inverse-variance sample weights AND a robust loss of the studentised residual, stated directly
in float64 (plain helper module, imported like variance_terms and robust_terms; numpy only, no GPU).

A metric over 2 n Radon intermediates: the data D_i of view i and its variance field V_i on the same bin grid.  For the pair i < j,
with w06 = K0[6] dkappa and the sums over both +-kappa samples of the pair's kappa grid (n_kappa steps, 2 n_kappa samples),

    d     = v0 - v1                            the difference of the two data samples, signed by the folds when `derivative` is set
    s     = V_i(sample) + V_j(sample)          the two variance samples at the same taps as the data, NEVER signed
    omega = 1 / max(s, floor)
    z     = |d| / sqrt(max(s, floor))          the studentised residual
    w     = robust_terms.loss_weight(z, loss, delta)      delta counts sigmas
    c     = w06 sum omega w d^2                (column 0 of evaluate_variance_robust's pair rows)
    u     = sum omega / (2 n_kappa)            (column 1: the mean weight)
    k     = sum omega w / (2 n_kappa)          (column 2: the weight mass the loss keeps)
    r     = sum omega d^2 / (2 n_kappa)        (column 3: the mean squared studentised residual, no loss and no delta in it)
    s     = w06 sum d^2,  raw = sum d^2 / (2 n_kappa)     (the scales: s omega_max for c, omega_max for u and k, raw omega_max for r)

a pair without samples has {0, 1, 1, 0}.  Over all pairs value = sum c / sum u, mean_weight = sum u / N, inlier_mass = sum k / sum u
(sum u == 0: all 0).  The kappa grid, the tap positions and the bilinear rule are channel_terms'; everything behind the tap positions
is float64.  `SLIPS` are the mistakes the comparison of tests/test_gpu_variance_robust.py must reject
(tests/test_variance_robust_terms_oracle.py shows that it does).

The cases, data, variance fields and floors are variance_terms'.  Every case has two scales, each rounded to float32: the median of
z over the case's samples at floor 0.125 and the 90th percentile of z at floor 1.5, in the float32-position statement; with the
three losses that is six (loss, floor, scale) combinations per case, COMBOS."""
import functools

import numpy as np

from channel_terms import _samples, kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T
import robust_terms as R
import variance_terms as V

f32 = np.float32

CASES = V.CASES
settings = V.settings
LOSSES = R.LOSSES
FLOORS = V.FLOORS
PAIRINGS = ((FLOORS[0], "median"), (FLOORS[1], "p90"))                       # the floor a scale is taken and used at
COMBOS = tuple((loss, floor, scale) for loss in LOSSES for floor, scale in PAIRINGS)
OUTSIDE = R.OUTSIDE

HT = ("huber", "truncated")
# slip -> (the losses it changes, the floors it changes); the two scan-level slips change no pair row
SLIPS = {"loss_on_raw_residual": (LOSSES, FLOORS), "sigma_from_unclamped_s": (LOSSES, FLOORS[1:]), "threshold_without_root": (HT, FLOORS),
         "k_without_omega": (LOSSES, FLOORS), "r_without_omega": (LOSSES, FLOORS), "vj_from_view_i": (LOSSES, FLOORS)}
SCAN_SLIPS = ("inlier_mass_over_n_pairs", "value_over_kept_mass")


def pair_samples(K01, D0, D1, V0, V1, n_u, n_v, derivative=True, positions="float32"):
    """One pair: (d, s, w06, rel_sign).  d, s (2 n_kappa,) float64: the residual and the sum of the two variance samples of every
    sample, +kappa samples first, then -kappa; w06 = K0[6] dkappa; rel_sign: the product of the two fold signs per sample."""
    D0, D1 = np.asarray(D0, np.float64)[None], np.asarray(D1, np.float64)[None]
    V0, V1 = np.asarray(V0, np.float64)[None], np.asarray(V1, np.float64)[None]
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
    d, s, rel = [], [], []
    for c in (cs, -cs):
        t0, t1 = taps(K0, n_alpha, n_t, rt, c, sn), taps(K1, n_alpha, n_t, rt, c, sn)
        d.append(_samples(D0, t0, derivative)[0] - _samples(D1, t1, derivative)[0])
        s.append(_samples(V0, t0, False)[0] + _samples(V1, t1, False)[0])   # unsigned always
        rel.append(t0[0] * t1[0])
    return np.concatenate(d), np.concatenate(s), float(K0[6]) * float(K1[6]), np.concatenate(rel)


def studentised(d, s, floor, slip=None):
    """z = |d| / sigma per sample."""
    sc = np.maximum(s, float(floor))
    if slip == "loss_on_raw_residual":
        return np.abs(d)
    if slip == "sigma_from_unclamped_s":
        return np.abs(d) / np.sqrt(s)
    if slip == "threshold_without_root":
        return np.abs(d) / sc
    return np.abs(d) / np.sqrt(sc)


def terms_of(d, s, w06, loss, delta, floor, slip=None):
    """{c, u, k, r, s, raw, n_kappa, outside} of one pair from its samples.  outside: the number of samples with z > delta."""
    n2 = len(d)
    if n2 == 0:
        return dict(c=0.0, u=1.0, k=1.0, r=0.0, s=0.0, raw=0.0, n_kappa=0, outside=0)
    omega = 1.0 / np.maximum(s, float(floor))
    z = studentised(d, s, floor, slip)
    if loss == "geman_mcclure" and slip == "threshold_without_root":
        z = studentised(d, s, floor)   # the slip is in thr, which this loss does not form
    w = R.loss_weight(z, loss, delta)
    sq = d * d
    return dict(c=w06 * float((omega * w) @ sq), u=float(omega.sum()) / n2,
                k=float(w.sum() if slip == "k_without_omega" else (omega * w).sum()) / n2,
                r=float(sq.sum() if slip == "r_without_omega" else omega @ sq) / n2,
                s=w06 * float(sq.sum()), raw=float(sq.sum()) / n2, n_kappa=n2 // 2, outside=int((z > delta).sum()))


def scan_samples(Ps, data, variances, n_u, n_v, K01s, pairs=None, derivative=True, positions="float32", slip=None):
    """pair_samples over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps.  data, variances: n fields
    each.  Returns a dict: pairs (P,), ij (P, 2), d, s (lists of P arrays), w06 (P,), fold (P,: channel_terms.fold_class), opposite (P,:
    the fraction of samples with opposite fold signs), n_pairs.  slip "vj_from_view_i" takes the second variance sample from view i's
    field."""
    import oracle
    n = len(Ps)
    assert len(data) >= n and len(variances) == n
    N = n * (n - 1) // 2
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), d=[], s=[], w06=np.zeros(len(pairs)), fold=[], opposite=np.zeros(len(pairs)),
               n_pairs=N)
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        d, s, w06, rel = pair_samples(K01s[q], data[i], data[j], variances[i], variances[i if slip == "vj_from_view_i" else j], n_u, n_v,
                                      derivative, positions)
        out["ij"][r] = (i, j)
        out["d"].append(d)
        out["s"].append(s)
        out["w06"][r] = w06
        out["fold"].append(T.fold_class(rel))
        out["opposite"][r] = float((rel < 0).mean()) if len(rel) else 0.0
    out["fold"] = np.array(out["fold"])
    return out


KEYS = ("c", "u", "k", "r", "s", "raw", "n_kappa", "outside")


def scan_terms(smp, loss, delta, floor, slip=None):
    """terms_of over the pairs of scan_samples' result.  Returns a dict of arrays over the listed pairs: pairs, ij, fold, opposite, c, u, k, r,
    s, raw, n_kappa, outside, floor; with all pairs listed also value, mean_weight and inlier_mass."""
    P = len(smp["pairs"])
    out = dict(pairs=smp["pairs"], ij=smp["ij"], n_pairs=smp["n_pairs"], floor=float(floor), fold=smp["fold"], opposite=smp["opposite"])
    out.update({key: np.zeros(P, np.int64 if key in ("n_kappa", "outside") else np.float64) for key in KEYS})
    for q in range(P):
        t = terms_of(smp["d"][q], smp["s"][q], smp["w06"][q], loss, delta, floor, slip)
        for key in KEYS:
            out[key][q] = t[key]
    if P == smp["n_pairs"]:
        out.update(results(out["c"], out["u"], out["k"], P, slip))
    return out


def results(c, u, k, count, slip=None):
    """The three results from columns over `count` pairs: value = sum c / sum u, mean_weight = sum u / count, inlier_mass =
    sum k / sum u; sum u == 0: all 0."""
    sc, su, sk = float(np.sum(c, dtype=np.float64)), float(np.sum(u, dtype=np.float64)), float(np.sum(k, dtype=np.float64))
    if su == 0.0:
        return dict(value=0.0, mean_weight=0.0, inlier_mass=0.0)
    return dict(value=sc / (sk if slip == "value_over_kept_mass" else su), mean_weight=su / count,
                inlier_mass=sk / (count if slip == "inlier_mass_over_n_pairs" else su))


def columns(t):
    """The statement's terms in the layout of evaluate_variance_robust's pair rows, (P, 4): c, u, k, r -- and their scales on
    variance_fields: s omega_max for c, omega_max for u and k, the mean raw square x omega_max for r."""
    om = V.omega_max(t["floor"])
    full = np.full(len(t["s"]), om)
    return np.stack([t["c"], t["u"], t["k"], t["r"]], axis=1), np.stack([t["s"] * om, full, full, t["raw"] * om], axis=1)


def variance_robust_scale(r, k=1.0):
    """ecc_host_variance_robust_scale in numpy: k x the median of sqrt(r_q) over the pairs with r_q > 0; none: 0."""
    r = np.asarray(r, np.float64)
    live = r[r > 0]
    return float(k * np.median(np.sqrt(live))) if len(live) else 0.0


def _earlier(label):
    for other in sorted(CASES):
        if other < label and settings(other)[:7] == settings(label)[:7]:
            return other
    return None


@functools.lru_cache(maxsize=4)
def case_samples(label, positions="float32"):
    """scan_samples of a case with variance_terms' inputs (cached; cases a, b and c share one scan and use the entry of a).  The
    arrays are shared and must not be changed."""
    if _earlier(label):
        return case_samples(_earlier(label), positions)
    Ps, n_u, n_v, data, variances, K01s = V.case_inputs(label)
    return scan_samples(Ps, data, variances, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=settings(label)[6], positions=positions)


@functools.lru_cache(maxsize=None)
def case_delta(label, scale):
    """The scale of a case, a float32: the median of z at floor 0.125 ("median") or its 90th percentile at floor 1.5 ("p90") over
    the samples of the case's listed pairs in the float32-position statement."""
    floor = dict((s, f) for f, s in PAIRINGS)[scale]
    smp = case_samples(label)
    z = np.concatenate([studentised(d, s, floor) for d, s in zip(smp["d"], smp["s"])])
    return f32(np.median(z) if scale == "median" else np.percentile(z, 90.0))


@functools.lru_cache(maxsize=None)
def _case_terms(label, loss, floor, scale, positions):
    return scan_terms(case_samples(label, positions), loss, float(case_delta(label, scale)), floor)


def case_terms(label, loss, floor, scale, positions="float32"):
    """scan_terms of a case at one of COMBOS (cached; the arrays are shared and must not be changed)."""
    return _case_terms(label, loss, float(floor), scale, positions)


# ---- the demonstration of DESIGN.md 4.30 -----------------------------------------------------------------------------------------
DEMO_BLOCK = (slice(50, 62), slice(58, 68))   # rows (v), columns (u): the opaque block of DESIGN.md 4.15 / 4.23
DEMO_BLOCK_VIEW, DEMO_BLOCK_GAIN, DEMO_K = 5, 4.0, 2.0


def demo_images(imgs):
    """(noisy, noisy_block, pixel variances) of the 8-view sphere scan `imgs`: variance_terms.demo_images' noise in the left half of
    view 3, and on top of it the opaque block, + 4 x the view's maximum, pasted unflagged into view 5."""
    noisy, var = V.demo_images(imgs)
    both = noisy.copy()
    both[DEMO_BLOCK_VIEW][DEMO_BLOCK] += f32(DEMO_BLOCK_GAIN * float(np.max(np.asarray(imgs, f32)[DEMO_BLOCK_VIEW])))
    return noisy, both, var


def demo_forms(Ps, clean, bad, variances, floor, n_u, n_v, K01s_clean, K01s_bad, delta=None, raw_delta=None):
    """The four forms on the clean and on a corrupted scan with the same variance fields, by the statement: a dict form -> (clean,
    corrupted) for "evaluate" (mean of s), "variance" (sum c / sum u at delta = inf), "raw_truncated" (robust_terms' truncated loss on
    the raw residual) and "studentised_truncated" (this form's).  delta: this form's scale as a float32 (None: DEMO_K x
    variance_robust_scale of the corrupted scan's own rows at delta = inf); raw_delta: the raw loss's (None: DEMO_K x
    robust_terms.robust_scale of the corrupted scan).  Also "delta" and "raw_delta", as used, and "own_delta", "own_raw_delta", the statement's own."""
    smp = [scan_samples(Ps, data, variances, n_u, n_v, K01s) for data, K01s in ((clean, K01s_clean), (bad, K01s_bad))]
    open_ = [scan_terms(x, "truncated", np.inf, floor) for x in smp]
    own = f32(variance_robust_scale(f32(open_[1]["r"]), DEMO_K)), f32(R.robust_scale(f32(open_[1]["raw"]), DEMO_K))
    delta, raw_delta = float(f32(own[0] if delta is None else delta)), float(f32(own[1] if raw_delta is None else raw_delta))
    out = dict(delta=delta, raw_delta=raw_delta, own_delta=float(own[0]), own_raw_delta=float(own[1]))
    out["evaluate"] = tuple(t["s"].sum() / t["n_pairs"] for t in open_)
    out["variance"] = tuple(t["value"] for t in open_)
    raw = []
    for x in smp:
        w = [R.loss_weight(np.abs(d), "truncated", raw_delta) for d in x["d"]]
        raw.append(sum(w06 * float(wq @ (d * d)) for w06, wq, d in zip(x["w06"], w, x["d"])) / x["n_pairs"])
    out["raw_truncated"] = tuple(raw)
    out["studentised_truncated"] = tuple(scan_terms(x, "truncated", delta, floor)["value"] for x in smp)
    return out


def demo_ratio(forms, key):
    return forms[key][1] / forms[key][0]
