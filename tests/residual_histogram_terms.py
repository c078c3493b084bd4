"""The per-view histograms of the per-sample residual, stated directly in float64 (plain helper module, imported like robust_terms
and variance_robust_terms; numpy only, no GPU).

For every +-kappa sample of the pair i < j the binned quantity is

    raw        a = |d|                                  d: robust_terms' residual of the sample
    variance   a = |d| / sqrt(max(s, floor))            d, s: variance_robust_terms' residual and sum of the two variance samples

and the sample is counted in bin  min(trunc(a / width), n_bins - 1)  (NaN: the last bin) of row i AND of row j of an n_views x n_bins
table: the last bin is the overflow bin.  The edge below bin k is e_k = k / inv_width with inv_width = float32(1 / width), the
factor the device multiplies by.  The samples are robust_terms.case_residuals(label)["d"] and variance_robust_terms.case_samples(label)
(d and s); case e, of which those hold a sample of the pairs only, is stated here over ALL of its 2 145 pairs (a second or two), so
that an all-pairs call -- the only way to one wave per pair under the reference arithmetic -- has a statement.

What a device table is held to is a BRACKET on cumulative counts, per view row v and per bin edge e_k, k = 1 .. n_bins - 1:

    C_v(e_k - tau)  <=  sum of the device's bins < k of row v  <=  C_v(e_k + tau)         C_v(t) = the statement's samples of v below t

with tau an absolute tolerance on the binned quantity (`bracket`, `needed_tau`), and exact equality of the row sums.  `SLIPS` are the
mistakes that comparison must reject (tests/test_residual_histogram_terms_oracle.py shows that it does); `band_share` is the share
of a row's samples that lie within tau of an edge, which must stay small or the bracket could hide a wrong bin."""
import functools

import numpy as np

import robust_terms as R
import variance_robust_terms as VR
import variance_terms as V
import weighted_terms as W

f32 = np.float32

CASES = W.CASES
LABELS = ("a", "b", "c", "d", "e", "i", "j")      # polynomial, per-sample, row-quad copies, reference x 4 waves, reference x 1 wave, plain data, user dkappa
KINDS = ("raw", "variance")
FLOOR = VR.FLOORS[1]                               # 1.5: active on part of the samples
N_BINS = (64, 256)
OVERFLOW = {"tenth": 0.10, "rare": 0.005}          # the share of all samples the overflow bin holds, by construction of the width

# tau: an absolute tolerance on the binned quantity, as a fraction of the case's largest value.  The project's per-pair bars (1e-6
# under the reference arithmetic, 1e-3 on the throughput paths) were the starting point; a GPU run measured
# the smallest tau at which every table of a path passes against this statement (needed_tau; DESIGN.md 4.34 has the table): 5.3e-8
# under the reference arithmetic (case e; a few float32 roundings of d), 9.2e-5 on the throughput paths (case b).  Chosen: 2 x that,
# for the rounding that depends on the build, not on the run.
TAU_REFERENCE = 1.1e-7
TAU_THROUGHPUT = 2e-4
MAX_BAND_SHARE = 0.02

# slip -> the kinds it changes
SLIPS = {"signed_residual": KINDS, "plus_sample_only": KINDS, "one_row_only": KINDS, "edges_off_by_one": KINDS,
         "z_from_unclamped_s": ("variance",), "z_without_root": ("variance",), "round_to_nearest": KINDS}


def _all_pairs_of_e(kind, positions):
    """Case e over all of its pairs (robust_terms and variance_robust_terms hold the oracle's sample of them)."""
    if kind == "raw":
        Ps, n_u, n_v, data, _, K01s = W.case_inputs("e")
        return R.scan_residuals(Ps, data, n_u, n_v, K01s, pairs=None, derivative=W.settings("e")[6], positions=positions)
    Ps, n_u, n_v, data, variances, K01s = V.case_inputs("e")
    return VR.scan_samples(Ps, data, variances, n_u, n_v, K01s, pairs=None, derivative=W.settings("e")[6], positions=positions)


def _first(label):
    """The first label with the same scan, data and settings (a for b and c): the statement does not depend on the sampling mode."""
    for other in sorted(CASES):
        if W.settings(other)[:7] == W.settings(label)[:7]:
            return other
    return label


def case_samples(label, kind, positions="float32"):
    """{ij (P, 2), d, s (lists of P arrays; s None for "raw"), n_views} of a case: every pair's samples, +kappa first, then -kappa.
    Cached: the arrays are shared and must not be changed."""
    return _case_samples(_first(label), kind, positions)


@functools.lru_cache(maxsize=8)
def _case_samples(label, kind, positions):
    if kind not in KINDS:
        raise ValueError("kind: one of %s" % (KINDS,))
    if label == "e":
        smp = _all_pairs_of_e(kind, positions)
    else:
        smp = R.case_residuals(label, positions) if kind == "raw" else VR.case_samples(label, positions)
    assert len(smp["pairs"]) == smp["n_pairs"]
    return dict(ij=smp["ij"], d=smp["d"], s=smp.get("s"), n_views=W.settings(label)[1])


def binned_quantity(d, s=None, floor=FLOOR, slip=None):
    """a per sample (signed under the slip that forgets the absolute value)."""
    if slip == "signed_residual":
        top = np.asarray(d, np.float64)
    else:
        top = np.abs(d)
    if s is None:
        return top
    if slip == "z_from_unclamped_s":
        return top / np.sqrt(s)
    sc = np.maximum(s, float(floor))
    return top / sc if slip == "z_without_root" else top / np.sqrt(sc)


def inv_width_of(width):
    """The factor the device multiplies by: float32(1 / width), formed in float64."""
    return float(f32(1.0 / float(f32(width))))


def edges(width, n_bins):
    """e_k for k = 1 .. n_bins - 1."""
    return np.arange(1, n_bins, dtype=np.float64) / inv_width_of(width)


def bins_of(a, width, n_bins, slip=None):
    """The bin of every value: trunc(a * inv_width) below n_bins - 1, else (and for NaN) the last bin.  A negative value (the slip
    without the absolute value) truncates towards zero and is kept inside the table: bin 0."""
    x = np.asarray(a, np.float64) * inv_width_of(width)
    if slip == "round_to_nearest":
        k = np.rint(x)
    elif slip == "edges_off_by_one":
        k = np.trunc(x) + 1.0
    else:
        k = np.trunc(x)
    k = np.where(x < n_bins - 1, k, n_bins - 1)            # NaN fails the comparison
    return np.clip(k, 0, n_bins - 1).astype(np.int64)


def rows(label, kind, width, n_bins, positions="float32", slip=None, pairs=None):
    """The table of a case, (n_views, n_bins) int64.  pairs: indices into the case's pairs (None: all)."""
    smp = case_samples(label, kind, positions)
    out = np.zeros((smp["n_views"], n_bins), np.int64)
    for q in (range(len(smp["d"])) if pairs is None else pairs):
        d, s = smp["d"][q], (None if smp["s"] is None else smp["s"][q])
        if slip == "plus_sample_only":
            d, s = d[:len(d) // 2], (None if s is None else s[:len(s) // 2])
        h = np.bincount(bins_of(binned_quantity(d, s, FLOOR, slip), width, n_bins, slip), minlength=n_bins)
        i, j = smp["ij"][q]
        out[i] += h
        if slip != "one_row_only":
            out[j] += h
    return out


def view_values(label, kind, positions="float32"):
    """Per view, the sorted binned quantities of every sample of every pair the view is in (a tuple of n_views float64 arrays)."""
    return _view_values(_first(label), kind, positions)


@functools.lru_cache(maxsize=8)
def _view_values(label, kind, positions):
    smp = case_samples(label, kind, positions)
    per_view = [[] for _ in range(smp["n_views"])]
    for q, (i, j) in enumerate(smp["ij"]):
        a = binned_quantity(smp["d"][q], None if smp["s"] is None else smp["s"][q])
        per_view[i].append(a)
        per_view[j].append(a)
    return tuple(np.sort(np.concatenate(x)) if x else np.zeros(0) for x in per_view)


def count_below(label, kind, thresholds, positions="float32", inclusive=False):
    """C_v(t) for every view and every threshold: (n_views, len(thresholds)) int64, the samples with a < t (inclusive: a <= t)."""
    t = np.asarray(thresholds, np.float64)
    side = "right" if inclusive else "left"
    return np.stack([np.searchsorted(a, t, side=side) for a in view_values(label, kind, positions)])


def all_values(label, kind, positions="float32"):
    """The binned quantity of every sample of the case, each once (unsorted)."""
    smp = case_samples(label, kind, positions)
    return np.concatenate([binned_quantity(smp["d"][q], None if smp["s"] is None else smp["s"][q]) for q in range(len(smp["d"]))])


def case_width(label, kind, n_bins, share):
    """The width, a float32, at which the overflow bin of an n_bins table holds the share OVERFLOW[share] of the case's samples in
    the float32-position statement: that quantile / (n_bins - 1)."""
    return _case_width(_first(label), kind, n_bins, share)


@functools.lru_cache(maxsize=None)
def _case_width(label, kind, n_bins, share):
    q = np.percentile(all_values(label, kind), 100.0 * (1.0 - OVERFLOW[share]))
    return f32(q / (n_bins - 1))


def case_scale(label, kind):
    """The case's largest binned quantity: what the bars are applied to."""
    return _case_scale(_first(label), kind)


@functools.lru_cache(maxsize=None)
def _case_scale(label, kind):
    return float(np.max(all_values(label, kind)))


def tau_of(label, kind, reference):
    """The tolerance of a case on a path: the bar x the case's largest value."""
    return (TAU_REFERENCE if reference else TAU_THROUGHPUT) * case_scale(label, kind)


def _below(table):
    """sum of the bins < k of every row, k = 1 .. n_bins - 1."""
    return np.cumsum(np.asarray(table, np.int64), axis=1)[:, :-1]


def bracket(table, label, kind, width, tau, positions="float32"):
    """How many (row, edge) cells of `table` break the bracket at tau against the statement, and how many rows have another sum
    than the statement's: (cells, rows).  (0, 0): the table passes."""
    table = np.asarray(table, np.int64)
    e = edges(width, table.shape[1])
    got = _below(table)
    lo = count_below(label, kind, e - tau, positions)
    hi = count_below(label, kind, e + tau, positions, inclusive=True)
    totals = np.array([len(a) for a in view_values(label, kind, positions)])
    return int(((got < lo) | (got > hi)).sum()), int((table.sum(axis=1) != totals).sum())


def needed_tau(table, label, kind, width, positions="float32"):
    """The smallest tau at which `table` passes the bracket (its row sums aside): the largest distance, over rows and edges, from the
    edge to the statement value that would have to lie on the other side of it.  inf when a row holds more samples than the statement."""
    table = np.asarray(table, np.int64)
    e = edges(width, table.shape[1])
    got = _below(table)
    worst = 0.0
    for v, a in enumerate(view_values(label, kind, positions)):
        m = got[v]
        if len(a) == 0:
            if m.any():
                return np.inf
            continue
        if m.max() > len(a):
            return np.inf
        below = np.searchsorted(a, e, side="left")
        up = m > below           # the device counts more below e_k: the statement's m-th smallest value must lie below e_k + tau
        down = m < below         # fewer: the statement's (m + 1)-th smallest value must lie at or above e_k - tau
        need = np.zeros(len(e))
        need[up] = a[m[up] - 1] - e[up]
        need[down] = e[down] - a[m[down]]
        worst = max(worst, float(need.max()))
    return worst


def band_share(label, kind, width, n_bins, tau, positions="float32"):
    """The largest share, over rows and edges, of a row's samples that lie within tau of the edge."""
    e = edges(width, n_bins)
    inside = count_below(label, kind, e + tau, positions, inclusive=True) - count_below(label, kind, e - tau, positions)
    totals = np.array([max(len(a), 1) for a in view_values(label, kind, positions)])
    return float((inside / totals[:, None]).max())


def quantile(row, width, q):
    """ecc_host_histogram_quantile in numpy, on one row (or a sum of rows) of counts."""
    row = np.asarray(row, np.float64).reshape(-1)
    if not 0.0 <= q <= 1.0:
        return float("nan")
    total = row.sum()
    if total == 0:
        return 0.0
    target, below = q * total, 0.0
    for k, c in enumerate(row):
        if c > 0 and below + c >= target:
            return float("inf") if k == len(row) - 1 else (k + (target - below) / c) * float(width)
        below += c
    return float("inf")
