"""Where the robust loss rejects on a metric that already carries line weights, stated directly in float64 (plain helper module,
imported like robust_map_terms and weighted_robust_terms; numpy only, no GPU).

A metric over 2 n Radon intermediates: the data D_i of view i and its line weights W_i.  Every +-kappa sample of the pair (i, j)
has a residual d, a weight product mu = W_i(sample) W_j(sample) (weighted_robust_terms.scan_samples), an IRLS weight w(|d|) of the
RAW residual (robust_terms.loss_weight) and two bilinear footprints, one in view i and one in view j (robust_map_terms.pair_taps).
With b the four footprint products,

    HITS_v[cell] += b mu            REJ_v[cell] += b mu (1 - w)

for v = i with view i's footprint and v = j with view j's, np.add.at; mu is the product of BOTH views' weights in either view.
Planes are (n_t, n_alpha), as the data are.

The SCALE of a bin is robust_map_terms.bin_scale of the UNWEIGHTED HITS of the same case (robust_map_terms.case_map): a bin of
weight 0 still has a scale, and a position error eps moves at most 2 eps of each sample whatever mu <= 1 is.

`SLIPS` are the mistakes the comparison of tests/test_gpu_weighted_robust_map.py must reject
(tests/test_weighted_robust_map_terms_oracle.py shows that it does).  The cases are weighted_terms.CASES with
weighted_terms.case_inputs' weights and robust_terms' two scales and three losses."""
import functools

import numpy as np

from channel_terms import _samples, kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T
import robust_map_terms as M
import robust_terms as R
import weighted_robust_terms as WR
import weighted_terms as W

f32 = np.float32

CASES = WR.CASES
LOSSES = R.LOSSES
SCALES = R.SCALES

SLIPS = ("mu_left_out_of_hits",        # HITS += b
         "mu_left_out_of_rej",         # REJ += b (1 - w)
         "own_weight_only",            # a view's deposits under that view's weight alone
         "wj_from_view_i",             # W_j taken from view i (weighted_robust_terms.scan_samples' slip)
         "w_of_weighted_residual")     # w of sqrt(mu) |d|


def pair_weights(K01, W0, W1, n_u, n_v, positions="float32"):
    """The two weight samples of every sample of one pair, in weighted_robust_terms.pair_samples' order: (W_i(sample), W_j(sample)),
    whose product is its mu."""
    W0, W1 = np.asarray(W0, np.float64)[None], np.asarray(W1, np.float64)[None]
    _, n_t, n_alpha = W0.shape
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
    wi, wj = [], []
    for c in (cs, -cs):
        wi.append(_samples(W0, taps(K0, n_alpha, n_t, rt, c, sn), False)[0])
        wj.append(_samples(W1, taps(K1, n_alpha, n_t, rt, c, sn), False)[0])
    return np.concatenate(wi), np.concatenate(wj)


def deposit(hits, rej, taps, x_hits, x_rej):
    """One view's footprints `taps` into its planes hits, rej (n_t, n_alpha), in place: b x_hits and b x_rej per cell."""
    i0, i1, j0, j1, fx, fy = taps
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    for j, i, b in ((j0, i0, (1.0 - fx) * (1.0 - fy)), (j0, i1, fx * (1.0 - fy)), (j1, i0, (1.0 - fx) * fy), (j1, i1, fx * fy)):
        np.add.at(hits, (j, i), b * x_hits)
        np.add.at(rej, (j, i), b * x_rej)


def scan_map(smp, K01s, n, n_alpha, n_t, n_u, n_v, loss, delta, positions="float32", slip=None, weights=None):
    """HITS and REJ of every view, (n, n_t, n_alpha) float64 each, over the pairs of weighted_robust_terms.scan_samples' result `smp`
    (made with the same `positions`; for the slip "wj_from_view_i" with that slip).  weights: the n weight fields, needed by the
    slip "own_weight_only" alone."""
    hits, rej = np.zeros((n, n_t, n_alpha)), np.zeros((n, n_t, n_alpha))
    for r, q in enumerate(smp["pairs"]):
        i, j = (int(v) for v in smp["ij"][r])
        d, mu = smp["d"][r], smp["mu"][r]
        if len(d) == 0:
            continue
        a = np.sqrt(mu) * np.abs(d) if slip == "w_of_weighted_residual" else np.abs(d)
        q1 = 1.0 - R.loss_weight(a, loss, delta)
        ti, tj = M.pair_taps(K01s[q], n_alpha, n_t, n_u, n_v, positions)
        mu_i = mu_j = mu
        if slip == "own_weight_only":
            mu_i, mu_j = pair_weights(K01s[q], weights[i], weights[j], n_u, n_v, positions)
        for v, t, m in ((i, ti, mu_i), (j, tj, mu_j)):
            one = np.ones_like(m)
            deposit(hits[v], rej[v], t, one if slip == "mu_left_out_of_hits" else m, (one if slip == "mu_left_out_of_rej" else m) * q1)
    return hits, rej


def map_weights(w_old, hits, rej, min_hits=1.0, gain=1.0):
    """ecc_metric_weighted_robust_map_weights in numpy, bit for bit from float32 planes: float32(W_old) * the factor of
    robust_map_terms.map_weights, one float32 multiply."""
    return (np.asarray(w_old, f32) * M.map_weights(hits, rej, min_hits, gain)).astype(f32)


def conserved(t, n):
    """Per view, from the terms of weighted_robust_terms.scan_terms: (sum u 2 n_kappa, sum (u - k) 2 n_kappa) over the pairs of the
    view -- what sum HITS and sum REJ of the view must be."""
    mass, refused = np.zeros(n), np.zeros(n)
    for r in range(len(t["pairs"])):
        i, j = t["ij"][r]
        mass[[i, j]] += t["u"][r] * 2 * t["n_kappa"][r]
        refused[[i, j]] += (t["u"][r] - t["k"][r]) * 2 * t["n_kappa"][r]
    return mass, refused


@functools.lru_cache(maxsize=4)
def _slipped_samples(label, positions):
    Ps, n_u, n_v, data, weights, K01s = W.case_inputs(label)
    return WR.scan_samples(Ps, data, weights, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=W.settings(label)[6],
                           positions=positions, slip="wj_from_view_i")


@functools.lru_cache(maxsize=None)
def _case_map(label, loss, scale, positions, slip):
    Ps, n_u, n_v, data, weights, K01s = W.case_inputs(label)
    _, n, n_alpha, n_t = W.settings(label)[:4]
    smp = _slipped_samples(label, positions) if slip == "wj_from_view_i" else WR.case_samples(label, positions)
    return scan_map(smp, K01s, n, n_alpha, n_t, n_u, n_v, loss, float(R.case_delta(label, scale)), positions, slip, weights)


def case_map(label, loss, scale, positions="float32", slip=None):
    """scan_map of a case at one of its two scales (cached; the arrays are shared and must not be changed).  Case e: over the
    oracle's sample of the pairs (channel_terms.case_pairs)."""
    return _case_map(label, loss, scale, positions, slip)


def case_scale(label, loss, scale):
    """The per-bin scale of a case: robust_map_terms.bin_scale of its UNWEIGHTED HITS."""
    return M.bin_scale(M.case_map(label, loss, scale)[0])
