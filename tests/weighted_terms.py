"""The per-pair sums of the metric with per-line weights, stated directly in float64 (plain helper module, imported like
channel_terms; numpy only, no GPU).

A metric over 2 n Radon intermediates: the data D_i of view i and its line weights W_i on the same bin grid.  For the pair i < j,
with w = K0[6] dkappa and the sums over both +-kappa samples of the pair's kappa grid (n_kappa steps, 2 n_kappa samples),

    d  = v0 - v1                       the difference of the two data samples, signed by the folds when `derivative` is set
    mu = W_i(sample) W_j(sample)       the two weight samples at the same taps as the data, NEVER signed
    c  = w sum mu d^2                  (column 0 of evaluate_weighted's pair rows)
    u  = sum mu / (2 n_kappa)          (column 1: the coverage; a pair without samples has c = 0, u = 1)
    s  = w sum d^2                     (the scale of c: no weight in [0, 1] can make c larger)

The kappa grid, the tap positions and the bilinear rule are channel_terms' (kappa_grid, range_t, taps_float32 / taps_float64,
_samples); everything behind the tap positions is float64.  `SLIPS` are the mistakes the comparison of tests/test_gpu_weighted.py
must reject (tests/test_weighted_terms_oracle.py shows that it does).

The cases are channel_terms.CASES with the data of channel 0 (`CASES` below maps the labels a .. j of DESIGN.md 4.15 to them).  The
weights of a case come from default_rng(11): every view's field is tiled with blocks of side 1/8 of the grid, each block exactly
0.0, exactly 1.0, or U(0, 1) per bin, so that 0 <-> 1 edges, interiors of both kinds and rough fields are all sampled."""
import functools

import numpy as np

from channel_terms import CASES as CHANNEL_CASES
from channel_terms import _samples, case_data, kappa_grid, range_t, taps_float32, taps_float64
import channel_terms as T

f32 = np.float32

# label -> key of channel_terms.CASES (j: the single-channel entry; the data are channel 0 either way)
CASES = {"a": "a", "b": "b", "c": "c", "d": "d", "e": "e", "f": "f", "g": "g", "h": "h", "i": "i", "j": "j1"}
assert all(v in CHANNEL_CASES for v in CASES.values())

SLIPS = ("wj_from_view_i", "fold_sign_on_weights", "mu_plus_for_both", "difference_of_weighted", "coverage_over_n_kappa")


def weight_fields(n, n_t, n_alpha, seed=11):
    """n float32 fields (n_t, n_alpha): 8 x 8 blocks of side ceil(n / 8) per view, each of one kind -- 0: exactly 0.0, 1: exactly 1.0,
    2: U(0, 1) per bin."""
    rng = np.random.default_rng(seed)
    bt, ba = -(-n_t // 8), -(-n_alpha // 8)
    out = []
    for _ in range(n):
        kinds = rng.integers(0, 3, (8, 8))
        rough = rng.random((n_t, n_alpha)).astype(f32)
        kind = np.repeat(np.repeat(kinds, bt, axis=0), ba, axis=1)[:n_t, :n_alpha]
        out.append(np.where(kind == 2, rough, kind.astype(f32)).astype(f32))
    return out


def pair_terms(K01, D0, D1, W0, W1, n_u, n_v, derivative=True, positions="float32", slip=None):
    """One pair.  K01: 16 floats; D0, D1, W0, W1: (n_t, n_alpha), data and weights of view i and of view j.  Returns a dict: c, u, s,
    n_kappa, rel_sign (2 n_kappa,): the product of the two fold signs per sample (+kappa samples, then -kappa).  slip: one of SLIPS
    (wj_from_view_i is the caller's: it passes W_i twice)."""
    D0, D1 = np.asarray(D0, np.float64)[None], np.asarray(D1, np.float64)[None]
    W0, W1 = np.asarray(W0, np.float64)[None], np.asarray(W1, np.float64)[None]
    _, n_t, n_alpha = D0.shape
    K01 = np.asarray(K01, f32)
    K0, K1 = K01[:8], K01[8:]
    kappa = kappa_grid(K01)
    w = float(K0[6]) * float(K1[6])
    rt = range_t(n_u, n_v, n_t)
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
        signed = slip == "fold_sign_on_weights" and derivative
        m0.append(_samples(W0, t0, signed)[0])   # unsigned always
        m1.append(_samples(W1, t1, signed)[0])
        rel.append(t0[0] * t1[0])
    n_kappa = len(kappa)
    v0, v1, m0, m1 = (np.concatenate(x) for x in (v0, v1, m0, m1))   # (2 n_kappa,)
    d = v0 - v1
    mu = m0 * m1
    if slip == "mu_plus_for_both":
        mu = np.concatenate([mu[:n_kappa], mu[:n_kappa]])
    s = w * float(d @ d)
    if slip == "difference_of_weighted":
        e = m0 * v0 - m1 * v1
        c_val = w * float(e @ e)
    else:
        c_val = w * float(mu @ (d * d))
    if n_kappa == 0:
        u = 1.0
    else:
        u = float(mu.sum()) / (n_kappa if slip == "coverage_over_n_kappa" else 2 * n_kappa)
    return dict(c=c_val, u=u, s=s, n_kappa=n_kappa, rel_sign=np.concatenate(rel))


def scan_terms(Ps, data, weights, n_u, n_v, K01s, pairs=None, derivative=True, positions="float32", slip=None):
    """pair_terms over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps.  data, weights: n fields each.
    Returns a dict of arrays over the listed pairs: pairs, ij (P, 2), c, u, s, n_kappa, fold (channel_terms.fold_class), opposite (the
    fraction of samples with opposite fold signs); with all
    pairs listed also value = sum c / sum u and coverage = sum u / N (sum u == 0: both 0)."""
    import oracle
    n = len(Ps)
    assert len(data) == n and len(weights) == n
    N = n * (n - 1) // 2
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), c=np.zeros(len(pairs)), u=np.zeros(len(pairs)), s=np.zeros(len(pairs)),
               n_kappa=np.zeros(len(pairs), np.int64), fold=[], opposite=np.zeros(len(pairs)), n_pairs=N)
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        t = pair_terms(K01s[q], data[i], data[j], weights[i], weights[i if slip == "wj_from_view_i" else j], n_u, n_v, derivative,
                       positions, slip)
        out["ij"][r] = (i, j)
        for key in ("c", "u", "s", "n_kappa"):
            out[key][r] = t[key]
        out["fold"].append(T.fold_class(t["rel_sign"]))
        out["opposite"][r] = float((t["rel_sign"] < 0).mean()) if len(t["rel_sign"]) else 0.0
    out["fold"] = np.array(out["fold"])
    if len(pairs) == N:
        su = out["u"].sum()
        out.update(value=out["c"].sum() / su if su else 0.0, coverage=su / N if su else 0.0)
    return out


def columns(t):
    """The oracle's terms in the layout of evaluate_weighted's pair rows, (P, 2): c, u -- and their scales: s for c, 1 for u."""
    return np.stack([t["c"], t["u"]], axis=1), np.stack([t["s"], np.ones(len(t["s"]))], axis=1)


def settings(label):
    """(name, n, n_alpha, n_t, radius, dkappa, derivative, [(sampling, quads)]) of a case."""
    name, n, n_alpha, n_t, _, radius, dkappa, derivative, setups = CHANNEL_CASES[CASES[label]]
    return name, n, n_alpha, n_t, radius, dkappa, derivative, setups


@functools.lru_cache(maxsize=2)
def case_inputs(label):
    """(Ps, n_u, n_v, data, weights, K01s) of a case: the data are channel 0 of channel_terms.case_data, the weights weight_fields,
    the pair geometry the C oracle's.  Cached: the arrays are shared and must not be changed."""
    import oracle
    name, n, n_alpha, n_t, radius, dkappa, derivative, _ = settings(label)
    for other in sorted(CASES):
        if other < label and settings(other)[:7] == settings(label)[:7]:
            return case_inputs(other)
    Ps, n_u, n_v, host, _ = case_data(CASES[label])
    data = host[:n]
    K01s = oracle.evaluate_all(Ps, data, n_u, n_v, object_radius_mm=radius, dkappa=dkappa, is_derivative=derivative, want_K01=True)["K01s"]
    return Ps, n_u, n_v, data, weight_fields(n, n_t, n_alpha), K01s


@functools.lru_cache(maxsize=8)
def case_terms(label, positions="float32"):
    """scan_terms of a case with its weights (cached; cases a, b and c share one scan and use the entry of a)."""
    for other in sorted(CASES):
        if other < label and settings(other)[:7] == settings(label)[:7]:
            return case_terms(other, positions)
    Ps, n_u, n_v, data, weights, K01s = case_inputs(label)
    return scan_terms(Ps, data, weights, n_u, n_v, K01s, pairs=T.case_pairs(CASES[label]), derivative=settings(label)[6], positions=positions)
