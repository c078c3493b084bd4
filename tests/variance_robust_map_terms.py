"""Where the robust loss rejects in sigma units, stated directly in float64 (plain helper module, imported like robust_map_terms and
variance_robust_terms; numpy only, no GPU).

A metric over 2 n Radon intermediates: the data D_i of view i and its variance field V_i.  Every +-kappa sample of the pair (i, j)
has a residual d and a variance sum s = V_i(sample) + V_j(sample) (variance_robust_terms.scan_samples), a studentised residual
z = |d| / sqrt(max(s, floor)) (variance_robust_terms.studentised), a loss weight w(z) (robust_terms.loss_weight, delta in sigmas)
and two bilinear footprints, one in view i and one in view j (robust_map_terms.pair_taps).  With b the four footprint products,

    HITS_v[cell] += b               REJ_v[cell] += b (1 - w)

for v = i with view i's footprint and v = j with view j's, np.add.at.  The deposits are in COUNT units: w is the loss weight alone,
not f = omega w, and b is not multiplied by omega.  Planes are (n_t, n_alpha), as the data are.

The SCALE of a bin is robust_map_terms.bin_scale of the statement's HITS: HITS has no variance, no loss and no delta in it.

map_variances is ecc_metric_variance_robust_map_variances in numpy, float32 where the rule says float32.

`SLIPS` are the mistakes the comparison of tests/test_gpu_variance_robust_map.py must reject, RULE_SLIPS those of the variances rule
(tests/test_variance_robust_map_terms_oracle.py shows that it does).  The cases, data, variance fields, floors and scales are
variance_robust_terms'."""
import functools

import numpy as np

import channel_terms as T
import robust_map_terms as M
import robust_terms as R
import variance_robust_terms as VR
import variance_terms as V

f32 = np.float32

CASES = VR.CASES
LOSSES = VR.LOSSES
COMBOS = VR.COMBOS

SLIPS = ("loss_on_raw_residual",       # w of |d|, as the n-metric's map forms it
         "one_minus_f",                # REJ += b (1 - omega w)
         "deposits_times_omega",       # HITS += b omega, REJ += b omega (1 - w)
         "vj_from_view_i",             # V_j taken from view i (variance_robust_terms.scan_samples' slip)
         "sigma_from_unclamped_s")     # z = |d| / sqrt(s)

RULE_SLIPS = ("raise_left_out",              # V * factor, a field of zeros stays at zero
              "raise_where_factor_is_one")   # max(V, floor / 2) * factor everywhere, an untouched bin loses its bits


def scan_map(smp, K01s, n, n_alpha, n_t, n_u, n_v, loss, delta, floor, positions="float32", slip=None):
    """HITS and REJ of every view, (n, n_t, n_alpha) float64 each, over the pairs of variance_robust_terms.scan_samples' result `smp`
    (made with the same `positions`; for the slip "vj_from_view_i" with that slip)."""
    hits, rej = np.zeros((n, n_t, n_alpha)), np.zeros((n, n_t, n_alpha))
    sample_slip = slip if slip in ("loss_on_raw_residual", "sigma_from_unclamped_s") else None
    for r, q in enumerate(smp["pairs"]):
        i, j = (int(v) for v in smp["ij"][r])
        d, s = smp["d"][r], smp["s"][r]
        if len(d) == 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            w = R.loss_weight(VR.studentised(d, s, floor, sample_slip), loss, delta)
        omega = 1.0 / np.maximum(s, float(floor))
        x_hits = omega if slip == "deposits_times_omega" else np.ones_like(d)
        x_rej = x_hits * (1.0 - (omega * w if slip == "one_minus_f" else w))
        ti, tj = M.pair_taps(K01s[q], n_alpha, n_t, n_u, n_v, positions)
        for v, t in ((i, ti), (j, tj)):
            deposit(hits[v], rej[v], t, x_hits, x_rej)
    return hits, rej


def deposit(hits, rej, taps, x_hits, x_rej):
    """One view's footprints `taps` into its planes hits, rej (n_t, n_alpha), in place: b x_hits and b x_rej per cell."""
    i0, i1, j0, j1, fx, fy = taps
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    for j, i, b in ((j0, i0, (1.0 - fx) * (1.0 - fy)), (j0, i1, fx * (1.0 - fy)), (j1, i0, (1.0 - fx) * fy), (j1, i1, fx * fy)):
        np.add.at(hits, (j, i), b * x_hits)
        np.add.at(rej, (j, i), b * x_rej)


def map_variances(v_old, hits, rej, floor, min_hits=1.0, gain=1.0, max_factor=1e4, slip=None):
    """ecc_metric_variance_robust_map_variances in numpy, bit for bit from float32 planes:
        mu     = robust_map_terms.map_weights(hits, rej, min_hits, gain)                   float32 of a float64 expression
        factor = max_factor where mu * max_factor <= 1, else 1 / mu                         float32
        out    = V where factor == 1, else max(V, half) * factor, half = 0.5f * floor       float32"""
    old = np.asarray(v_old, f32)
    mu = M.map_weights(hits, rej, min_hits, gain)
    top, one = f32(max_factor), f32(1.0)
    with np.errstate(divide="ignore", over="ignore"):
        factor = np.where((mu * top).astype(f32) <= one, top, (one / mu).astype(f32)).astype(f32)
    half = f32(0.5) * f32(floor)
    raised = np.where(old < half, half, old).astype(f32)
    if slip == "raise_left_out":
        raised = old
    grown = (raised * factor).astype(f32)
    if slip == "raise_where_factor_is_one":
        return grown
    return np.where(factor == one, old, grown).astype(f32)


def rejected_share(hits, rej):
    """sum REJ / sum HITS per view, 0 where a view has no hits (float64 sums of the planes as given)."""
    h, r = np.asarray(hits, np.float64).sum(axis=(1, 2)), np.asarray(rej, np.float64).sum(axis=(1, 2))
    return np.where(h > 0, r / np.where(h > 0, h, 1.0), 0.0)


def conserved(t, n):
    """Per view, from the terms of variance_robust_terms.scan_terms: the number of samples taken in it, sum of 2 n_kappa over the pairs
    of the view -- what sum HITS of the view must be."""
    count = np.zeros(n)
    for r in range(len(t["pairs"])):
        i, j = t["ij"][r]
        count[[i, j]] += 2 * t["n_kappa"][r]
    return count


@functools.lru_cache(maxsize=4)
def _slipped_samples(label, positions):
    Ps, n_u, n_v, data, variances, K01s = V.case_inputs(label)
    return VR.scan_samples(Ps, data, variances, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=V.settings(label)[6],
                           positions=positions, slip="vj_from_view_i")


@functools.lru_cache(maxsize=None)
def _case_map(label, loss, floor, scale, positions, slip):
    Ps, n_u, n_v, data, variances, K01s = V.case_inputs(label)
    _, n, n_alpha, n_t = V.settings(label)[:4]
    smp = _slipped_samples(label, positions) if slip == "vj_from_view_i" else VR.case_samples(label, positions)
    return scan_map(smp, K01s, n, n_alpha, n_t, n_u, n_v, loss, float(VR.case_delta(label, scale)), floor, positions, slip)


def case_map(label, loss, floor, scale, positions="float32", slip=None):
    """scan_map of a case at one of variance_robust_terms.COMBOS (cached; the arrays are shared and must not be changed).  Case e:
    over the oracle's sample of the pairs (channel_terms.case_pairs)."""
    return _case_map(label, loss, float(floor), scale, positions, slip)


def case_scale(label, loss, floor, scale):
    """The per-bin scale of a case: robust_map_terms.bin_scale of the statement's HITS."""
    return M.bin_scale(case_map(label, loss, floor, scale)[0])


def constant_map(label, value, loss, delta, floor, factor=1.0, positions="float32"):
    """scan_map of a case's data with every variance field the constant `value` x factor, at floor x factor."""
    Ps, n_u, n_v, data, _, K01s = V.case_inputs(label)
    _, n, n_alpha, n_t = V.settings(label)[:4]
    fields = [np.full((n_t, n_alpha), float(value) * factor)] * n
    smp = VR.scan_samples(Ps, data, fields, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=V.settings(label)[6], positions=positions)
    return scan_map(smp, K01s, n, n_alpha, n_t, n_u, n_v, loss, delta, floor * factor, positions)


# ---- the demonstration of DESIGN.md 4.31 -----------------------------------------------------------------------------------------
DEMO_LOSS, DEMO_MIN_HITS, DEMO_GAIN, DEMO_MAX_FACTOR = "truncated", 1.0, 1.0, 1e4


def demo_pass(Ps, bad, fields, floor, n_u, n_v, K01s, delta=None):
    """One pass of the feedback on the scan `bad` under the variance fields `fields`: the map at delta (None: DEMO_K x
    variance_robust_scale of the scan's own rows at delta = inf, as a float32) and the fields the rule returns from its float32
    planes.  Returns (delta, hits, rej, new fields)."""
    n = len(Ps)
    n_t, n_alpha = np.asarray(fields[0]).shape
    smp = VR.scan_samples(Ps, bad, fields, n_u, n_v, K01s)
    if delta is None:
        delta = float(f32(VR.variance_robust_scale(f32(VR.scan_terms(smp, DEMO_LOSS, np.inf, floor)["r"]), VR.DEMO_K)))
    hits, rej = scan_map(smp, K01s, n, n_alpha, n_t, n_u, n_v, DEMO_LOSS, delta, floor)
    new = [map_variances(fields[v], hits[v].astype(f32), rej[v].astype(f32), floor, DEMO_MIN_HITS, DEMO_GAIN, DEMO_MAX_FACTOR) for v in range(n)]
    return delta, hits, rej, new


def demo_ratio(Ps, clean, bad, fields, floor, n_u, n_v, K01s_clean, K01s_bad):
    """corrupted / clean of evaluate_variance's value (no loss) under the same variance fields."""
    return (V.scan_terms(Ps, bad, fields, floor, n_u, n_v, K01s_bad)["value"] /
            V.scan_terms(Ps, clean, fields, floor, n_u, n_v, K01s_clean)["value"])
