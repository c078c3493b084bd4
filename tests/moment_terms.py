"""The three moment blocks per pair of ecc_metric_evaluate_view_hessian, stated directly in float64 (plain helper module like
channel_terms, whose kappa grid, taps and samples it imports; numpy only, no GPU).

For the pair i < j with the signed samples v0_c / v1_c of channel c in view i / view j over both +-kappa samples of the pair's
kappa grid, and w = K0[6] dkappa:

    P00[c, d] = w sum v0_c v0_d        P11[c, d] = w sum v1_c v1_d        P01[c, d] = -w sum v0_c v1_d     (P01 is not symmetric)

so that the pair value at coefficients (a_i, a_j) is a_i^T P00 a_i + a_j^T P11 a_j + 2 a_i^T P01 a_j, and the Cauchy-Schwarz scales
no entry can exceed: sqrt(P00_cc P00_dd), sqrt(P11_cc P11_dd), sqrt(P00_cc P11_dd).  tests/test_moment_terms_oracle.py holds this
statement to channel_terms.pair_terms through the one-hot identity and to the C oracle through zeroed intermediates.

The layout of the call's pair rows (T2 = K (K + 1) + K^2 columns): P00's upper triangle in evaluate_gram's entry order, P11's upper
triangle, P01 row-major -- `columns`."""
import functools

import numpy as np

import channel_terms as T


def pair_moments(K01, D0, D1, n_u, n_v, derivative=True, positions="float32", skip_last=0):
    """One pair.  K01: 16 floats; D0, D1: (K, n_t, n_alpha) float64, the channels of view i and of view j.  Returns a dict: P00, P11,
    P01 (K, K) and their scales S00, S11, S01 (K, K)."""
    D0, D1 = np.asarray(D0, np.float64), np.asarray(D1, np.float64)
    Kc, n_t, n_alpha = D0.shape
    K01 = np.asarray(K01, T.f32)
    K0, K1 = K01[:8], K01[8:]
    kappa = T.kappa_grid(K01, skip_last)
    w = float(K0[6]) * float(K1[6])
    rt = T.range_t(n_u, n_v, n_t)
    cs, sn = np.cos(kappa.astype(np.float64)), np.sin(kappa.astype(np.float64))
    if positions == "float32":
        taps, cs, sn = T.taps_float32, cs.astype(T.f32), sn.astype(T.f32)
    elif positions == "float64":
        taps = T.taps_float64
    else:
        raise ValueError("positions: 'float32' or 'float64'")
    V0, V1 = [], []
    for c in (cs, -cs):
        V0.append(T._samples(D0, taps(K0, n_alpha, n_t, rt, c, sn), derivative))
        V1.append(T._samples(D1, taps(K1, n_alpha, n_t, rt, c, sn), derivative))
    V0, V1 = np.concatenate(V0, axis=1), np.concatenate(V1, axis=1)   # (K, 2 n_kappa)
    P00, P11, P01 = w * (V0 @ V0.T), w * (V1 @ V1.T), -w * (V0 @ V1.T)
    d0, d1 = np.diag(P00), np.diag(P11)
    return dict(P00=P00, P11=P11, P01=P01, S00=np.sqrt(np.outer(d0, d0)), S11=np.sqrt(np.outer(d1, d1)), S01=np.sqrt(np.outer(d0, d1)))


def scan_moments(Ps, host, K, n_u, n_v, pairs=None, object_radius_mm=0.0, dkappa=0.0, derivative=True, positions="float32",
                 skip_last=0, K01s=None):
    """pair_moments over the pairs `pairs` (indices in oracle.get_ij order; None: all) of the scan Ps with the K * n channel-major
    intermediates host.  Returns a dict of arrays over the listed pairs: pairs (P,), ij (P, 2), P00 / P11 / P01 / S00 / S11 / S01
    (P, K, K), K01s."""
    import oracle
    n = len(Ps)
    assert len(host) == K * n
    N = n * (n - 1) // 2
    if K01s is None:
        K01s = oracle.evaluate_all(Ps, host[:n], n_u, n_v, object_radius_mm=object_radius_mm, dkappa=dkappa,
                                   is_derivative=derivative, want_K01=True)["K01s"]
    pairs = np.arange(N) if pairs is None else np.asarray(sorted(set(int(q) for q in pairs)), np.int64)
    D = {}

    def channels(i):
        if i not in D:
            D[i] = np.stack([np.asarray(host[c * n + i], np.float64) for c in range(K)])
        return D[i]
    out = dict(pairs=pairs, ij=np.zeros((len(pairs), 2), np.int64), K01s=K01s, n_pairs=N)
    for key in ("P00", "P11", "P01", "S00", "S11", "S01"):
        out[key] = np.zeros((len(pairs), K, K))
    for r, q in enumerate(pairs):
        i, j = oracle.get_ij(int(q), n)
        t = pair_moments(K01s[q], channels(i), channels(j), n_u, n_v, derivative, positions, skip_last)
        out["ij"][r] = (i, j)
        for key in ("P00", "P11", "P01", "S00", "S11", "S01"):
            out[key][r] = t[key]
    return out


def n_columns(K):
    return K * (K + 1) + K * K


def columns(t):
    """The oracle's blocks in the layout of evaluate_view_hessian's pair rows, (P, T2), and their scales."""
    K = t["P00"].shape[1]
    iu = np.triu_indices(K)
    P = len(t["P00"])
    return (np.concatenate([t["P00"][:, iu[0], iu[1]], t["P11"][:, iu[0], iu[1]], t["P01"].reshape(P, K * K)], axis=1),
            np.concatenate([t["S00"][:, iu[0], iu[1]], t["S11"][:, iu[0], iu[1]], t["S01"].reshape(P, K * K)], axis=1))


def blocks(rows, K):
    """The inverse of `columns` for rows of the call: (P, T2) -> P00, P11 (symmetric, (P, K, K)) and P01 (P, K, K)."""
    rows = np.asarray(rows, np.float64)
    P, tri = len(rows), K * (K + 1) // 2
    iu = np.triu_indices(K)
    P00, P11 = np.zeros((P, K, K)), np.zeros((P, K, K))
    P00[:, iu[0], iu[1]] = rows[:, :tri]
    P00[:, iu[1], iu[0]] = rows[:, :tri]
    P11[:, iu[0], iu[1]] = rows[:, tri:2 * tri]
    P11[:, iu[1], iu[0]] = rows[:, tri:2 * tri]
    return P00, P11, rows[:, 2 * tri:].reshape(P, K, K).copy()


def column_names(K):
    tri = [(c, d) for c in range(K) for d in range(c, K)]
    return (["P00_%d%d" % cd for cd in tri] + ["P11_%d%d" % cd for cd in tri] + ["P01_%d%d" % (c, d) for c in range(K) for d in range(K)])


def assemble(rows, n, K):
    """H (n K, n K) in float64 from the call's pair rows (all pairs, get_ij order), as include/ecc_hip.h defines it, and the same
    sums of the entries' magnitudes (A): numpy's sums, in no particular order."""
    P00, P11, P01 = blocks(rows, K)
    N = n * (n - 1) // 2
    assert len(rows) == N
    iu = np.triu_indices(n, 1)   # get_ij order: i ascending, then j
    H, A = np.zeros((K, n, K, n)), np.zeros((K, n, K, n))
    for c in range(K):
        for d in range(K):
            H[c, iu[0], d, iu[1]] = P01[:, c, d] / N
            H[d, iu[1], c, iu[0]] = P01[:, c, d] / N
            A[c, iu[0], d, iu[1]] = np.abs(P01[:, c, d]) / N
            A[d, iu[1], c, iu[0]] = np.abs(P01[:, c, d]) / N
            diag, mag = np.zeros(n), np.zeros(n)
            np.add.at(diag, iu[0], P00[:, c, d])
            np.add.at(diag, iu[1], P11[:, c, d])
            np.add.at(mag, iu[0], np.abs(P00[:, c, d]))
            np.add.at(mag, iu[1], np.abs(P11[:, c, d]))
            H[c, np.arange(n), d, np.arange(n)] = diag / N
            A[c, np.arange(n), d, np.arange(n)] = mag / N
    return H.reshape(n * K, n * K), A.reshape(n * K, n * K)


@functools.lru_cache(maxsize=8)
def case_moments(key, positions="float32"):
    """scan_moments of a case of channel_terms.CASES, on the K01 of channel_terms.case_terms (cached; cases a, b and c share one)."""
    name, n, n_alpha, n_t, K, radius, dkappa, derivative, _ = T.CASES[key]
    for other in sorted(T.CASES):
        if other < key and T.CASES[other][:8] == T.CASES[key][:8]:
            return case_moments(other, positions)
    Ps, n_u, n_v, host, a = T.case_data(key)
    return scan_moments(Ps, host, K, n_u, n_v, pairs=T.case_pairs(key), object_radius_mm=radius, dkappa=dkappa, derivative=derivative,
                        positions=positions, K01s=T.case_terms(key, positions)["K01s"])
