"""The statement of the residual histograms (tests/residual_histogram_terms.py) without a GPU: the float32- and the float64-position
statement agree within the bracket; every slip in SLIPS is rejected by the bracket at the tolerance tests/test_gpu_residual_histogram.py
uses; the statement alone keeps at most 2 % of a row's samples within tau of any edge, for every case, table size and width used;
the quantile helper agrees with numpy's percentile of the binned values to within a bin."""
import numpy as np
import pytest

import residual_histogram_terms as H

SMALL = ("d", "i", "j")          # every check; a and e (16 views of 768^2, 2 145 pairs) take the checks that need them
CONFIGS = [(B, share) for B in H.N_BINS for share in H.OVERFLOW]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


def _paths(label):
    """(reference?, tau) of the arithmetic classes a case is evaluated under on the GPU."""
    import channel_terms as T
    n = H.W.settings(label)[1]
    out = {T.tolerance(sampling, n * (n - 1) // 2) == T.TOL_REFERENCE for sampling, _ in H.W.settings(label)[7]}
    return sorted(out)


@pytest.mark.parametrize("label", H.LABELS)
def test_the_statement_passes_its_own_bracket_and_the_band_is_thin(label):
    """The statement's table passes at tau = 0 (the bracket is closed at both ends), its row sums are its sample counts, the widths
    put the intended share into the overflow bin, and for every path the case runs on, every table size and every width the share of
    a row's samples within tau of an edge is at most 2 %."""
    for kind in H.KINDS:
        total = len(H.all_values(label, kind))
        assert total > 0 and total % 2 == 0
        for B, share in CONFIGS:
            w = H.case_width(label, kind, B, share)
            table = H.rows(label, kind, w, B)
            assert table.sum() == 2 * total
            assert H.bracket(table, label, kind, w, 0.0) == (0, 0)
            assert H.needed_tau(table, label, kind, w) == 0.0
            assert abs(table[:, -1].sum() / table.sum() - H.OVERFLOW[share]) <= 0.1 * H.OVERFLOW[share] + 2.0 / total, (label, kind, B, share)
            for reference in _paths(label):
                band = H.band_share(label, kind, w, B, H.tau_of(label, kind, reference))
                assert band <= H.MAX_BAND_SHARE, (label, kind, B, share, reference, band)


@pytest.mark.parametrize("label", SMALL + ("a",))
def test_float32_and_float64_positions_agree_within_the_bracket(label):
    """The table over float64 tap positions against the statement over float32 positions, at the throughput tau: the two differ by
    the rounding of the positions, which is what the throughput paths' polynomials are held to."""
    for kind in H.KINDS:
        tau = H.tau_of(label, kind, reference=False)
        for B, share in CONFIGS:
            w = H.case_width(label, kind, B, share)
            table = H.rows(label, kind, w, B, positions="float64")
            assert H.bracket(table, label, kind, w, tau) == (0, 0), (label, kind, B, share, H.needed_tau(table, label, kind, w), tau)


@pytest.mark.parametrize("label", SMALL + ("a", "e"))
def test_every_slip_is_rejected(label):
    """Each slip's table, made by the statement itself, against the statement: for every kind the slip changes, on every path the
    case runs on, at every table size and width, the bracket (or the row sums) rejects it.  round_to_nearest moves every edge by half
    a bin and can only be seen where half a bin exceeds tau: that holds for every table used (asserted: half a bin is at least
    0.0019, tau at most 0.0011)."""
    for slip, kinds in H.SLIPS.items():
        for kind in kinds:
            for reference in _paths(label):
                tau = H.tau_of(label, kind, reference)
                for B, share in CONFIGS:
                    w = H.case_width(label, kind, B, share)
                    assert 0.5 / H.inv_width_of(w) > tau, (label, kind, reference, B, share)
                    cells, sums = H.bracket(H.rows(label, kind, w, B, slip=slip), label, kind, w, tau)
                    assert cells + sums > 0, (label, slip, kind, reference, B, share)
                    if slip in ("plus_sample_only", "one_row_only"):
                        assert sums > 0, (label, slip, kind)


@pytest.mark.parametrize("label", SMALL)
def test_quantile_against_numpy(label):
    """histogram quantile of the summed rows (every sample twice: the same distribution) against numpy.percentile of the samples'
    bin midpoints, to within one bin width, on the cases' own samples; inf where the quantile lies in the overflow bin."""
    for kind in H.KINDS:
        a = H.all_values(label, kind)
        for B, share in CONFIGS:
            w = float(H.case_width(label, kind, B, share))
            table = H.rows(label, kind, w, B)
            mid = (H.bins_of(a, w, B) + 0.5) / H.inv_width_of(w)
            for q in (0.05, 0.25, 0.5, 0.75, 0.85):
                got, want = H.quantile(table.sum(axis=0), w, q), float(np.percentile(mid, 100.0 * q))
                assert abs(got - want) <= w, (label, kind, B, share, q, got, want)
            assert H.quantile(table.sum(axis=0), w, 1.0 - 0.5 * H.OVERFLOW[share]) == np.inf
            for v in range(table.shape[0]):
                assert H.quantile(table[v], w, 0.5) <= H.quantile(table[v], w, 0.75)
