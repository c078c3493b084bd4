"""Where the robust loss rejects, stated directly in float64 (plain helper module, imported like robust_terms; numpy only, no GPU).

A metric over one Radon intermediate per view.  Every +-kappa sample of the pair (i, j) has a residual d and an IRLS weight w(d)
(robust_terms.pair_residuals, loss_weight) and two bilinear footprints, one in view i and one in view j: the clamped cells
(i0, i1) x (j0, j1) with the fractions fx (angle) and fy (distance) of channel_terms.taps_float32 / taps_float64.  With
b = (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy at (j0, i0), (j0, i1), (j1, i0), (j1, i1),

    HITS_v[cell] += b            REJ_v[cell] += b (1 - w)

for v = i with view i's footprint and v = j with view j's: the adjoint of the sampling, np.add.at, so clamped cells that coincide
receive both deposits.  Planes are (n_t, n_alpha), as the data are.

The SCALE of a bin is the statement's HITS summed over the bin and its eight neighbours: every sample that touches a bin has its
whole footprint inside that neighbourhood, so the scale is at least the number of samples touching the bin, and a position error
eps moves at most 2 eps of each.  `compare` is channel_terms.compare per bin against that scale.

`SLIPS` are the mistakes the comparison of tests/test_gpu_robust_map.py must reject (tests/test_robust_map_terms_oracle.py shows
that it does).  The cases are weighted_terms.CASES with robust_terms' two scales and three losses."""
import functools

import numpy as np

from channel_terms import kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T
import robust_terms as R
import weighted_terms as W

f32 = np.float32

CASES = R.CASES
LOSSES = R.LOSSES
SCALES = R.SCALES

SLIPS = ("nearest_cell_only",          # the whole deposit at the nearest cell
         "w_instead_of_rejection",     # w deposited instead of 1 - w
         "both_at_view_i",             # both views' deposits at view i's positions
         "minus_kappa_left_out",       # the -kappa samples left out
         "fx_fy_swapped",              # the fractions swapped
         "planes_swapped_in_tuple",    # the plane of view j filed under view i: every second listed pair
         "clamped_duplicates_once")    # a clamped footprint whose cells coincide deposited once


def pair_taps(K01, n_alpha, n_t, n_u, n_v, positions="float32"):
    """The footprints of one pair, in the sample order of robust_terms.pair_residuals (+kappa samples, then -kappa): two tuples
    (i0, i1, j0, j1, fx, fy) of arrays (2 n_kappa,), for view i and for view j."""
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
    out = []
    for K in (K0, K1):
        parts = [taps(K, n_alpha, n_t, rt, c, sn)[1:] for c in (cs, -cs)]
        out.append(tuple(np.concatenate([p[k] for p in parts]) for k in range(6)))
    return out[0], out[1]


def deposit(hits, rej, taps, q, slip=None):
    """One view's footprints `taps` with the rejections q = 1 - w into its planes hits, rej (n_t, n_alpha), in place."""
    i0, i1, j0, j1, fx, fy = taps
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    if slip == "fx_fy_swapped":
        fx, fy = fy, fx
    if slip == "nearest_cell_only":
        i, j = np.where(fx < 0.5, i0, i1), np.where(fy < 0.5, j0, j1)
        np.add.at(hits, (j, i), 1.0)
        np.add.at(rej, (j, i), q)
        return
    cells = [(j0, i0, (1.0 - fx) * (1.0 - fy)), (j0, i1, fx * (1.0 - fy)), (j1, i0, (1.0 - fx) * fy), (j1, i1, fx * fy)]
    if slip == "clamped_duplicates_once":
        same_i, same_j = i0 == i1, j0 == j1
        keep = [np.ones(len(fx), bool), ~same_i, ~same_j, ~same_i & ~same_j]
        cells = [(j[k], i[k], b[k]) for (j, i, b), k in zip(cells, keep)]
        qs = [q[k] for k in keep]
    else:
        qs = [q] * 4
    for (j, i, b), qq in zip(cells, qs):
        np.add.at(hits, (j, i), b)
        np.add.at(rej, (j, i), b * qq)


def scan_map(res, K01s, n, n_alpha, n_t, n_u, n_v, loss, delta, positions="float32", slip=None):
    """HITS and REJ of every view, (n, n_t, n_alpha) float64 each, over the pairs of robust_terms.scan_residuals' result `res` (made
    with the same `positions`)."""
    hits, rej = np.zeros((n, n_t, n_alpha)), np.zeros((n, n_t, n_alpha))
    for r, q in enumerate(res["pairs"]):
        i, j = (int(v) for v in res["ij"][r])
        d = res["d"][r]
        if len(d) == 0:
            continue
        w = R.loss_weight(np.abs(d), loss, delta)
        rejection = w if slip == "w_instead_of_rejection" else 1.0 - w
        ti, tj = pair_taps(K01s[q], n_alpha, n_t, n_u, n_v, positions)
        if slip == "both_at_view_i":
            tj = ti
        if slip == "minus_kappa_left_out":
            h = len(d) // 2
            ti, tj, rejection = tuple(t[:h] for t in ti), tuple(t[:h] for t in tj), rejection[:h]
        if slip == "planes_swapped_in_tuple" and r % 2:
            i, j = j, i
        deposit(hits[i], rej[i], ti, rejection, slip)
        deposit(hits[j], rej[j], tj, rejection, slip)
    return hits, rej


def bin_scale(hits):
    """The scale of every bin: the statement's HITS over the bin and its eight neighbours.  hits: (..., n_t, n_alpha)."""
    h = np.asarray(hits, np.float64)
    p = np.pad(h, [(0, 0)] * (h.ndim - 2) + [(1, 1), (1, 1)])
    n_t, n_alpha = h.shape[-2:]
    return sum(p[..., a:a + n_t, b:b + n_alpha] for a in range(3) for b in range(3))


def compare(got, want, scale, tol):
    """The worst of |got - want| / (tol scale) over the bins: at most 1 where the bar holds; a bin without scale must be 0 in both."""
    return float(T.compare(np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1),
                           np.asarray(scale, np.float64).reshape(-1), tol))


def sample_counts(res, n):
    """Per view: the number of samples taken in it over the pairs of `res`, sum of 2 n_kappa."""
    out = np.zeros(n)
    for r in range(len(res["pairs"])):
        i, j = res["ij"][r]
        out[i] += len(res["d"][r])
        out[j] += len(res["d"][r])
    return out


def map_weights(hits, rej, min_hits=1.0, gain=1.0):
    """ecc_metric_robust_map_weights in numpy, bit for bit from float32 planes: 1 where h < min_hits, else
    float32(fmax(0, 1 - float64(float32(gain)) r / h))."""
    h, r = np.asarray(hits, f32).astype(np.float64), np.asarray(rej, f32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.fmax(0.0, 1.0 - np.float64(f32(gain)) * (r / h)).astype(f32)
    return np.where(np.asarray(hits, f32) < f32(min_hits), f32(1.0), mu).astype(f32)


@functools.lru_cache(maxsize=None)
def _case_map(label, loss, scale, positions, slip):
    Ps, n_u, n_v, data, _, K01s = W.case_inputs(label)
    _, n, n_alpha, n_t = W.settings(label)[:4]
    res = R.case_residuals(label, positions)
    return scan_map(res, K01s, n, n_alpha, n_t, n_u, n_v, loss, float(R.case_delta(label, scale)), positions, slip)


def case_map(label, loss, scale, positions="float32", slip=None):
    """scan_map of a case at one of its two scales (cached; the arrays are shared and must not be changed).  Case e: over the
    oracle's sample of the pairs (channel_terms.case_pairs)."""
    return _case_map(label, loss, scale, positions, slip)
