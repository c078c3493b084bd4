"""MetricDirect over index lists and pose batches (include/ecc_hip.h: ecc_direct_evaluate_pairs,
ecc_direct_evaluate_pose_deltas).  The contract: a list entry (P0, P1, I0, I1) has THE BITS of evaluateForImagePair on a metric
whose matrices of views I0, I1 are rows P0, P1; a segment's sum is a fixed function of its values, the one evaluate() applies to
a batch; a pose's terms are the entries of its pairs with the candidate rows.  Shapes: the 8-view 128^2 scan (the gather kernel)
and the 448 x 400 4-view scan of tests/test_gpu_direct.py with its steep pair (the slab kernel, plain and transposed tile)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONFIGS = [(scan, dkappa, fbcc) for scan in ("small", "large") for dkappa in (0.0, 0.002) for fbcc in (False, True)]


@functools.lru_cache(maxsize=None)
def _large_scan():
    from epipolarconsistency_amd import geometry, synthetic
    n_u, n_v = 448, 400
    Ps = synthetic.short_scan(4, n_u, n_v, 0.308 * 1024 / n_u)
    Ps[2] = Ps[2] @ geometry.rigid_transform(tz=40.0, rx=0.5)  # a pair whose epipolar lines are steep in the image
    imgs = np.ascontiguousarray(synthetic.projections_numpy(Ps, n_u, n_v, synthetic.sphere_phantom()), np.float32)
    return dict(Ps=Ps, imgs=imgs, n_u=n_u, n_v=n_v)


def _scan(name, small_scan):
    if name == "large":
        return _large_scan()
    return dict(Ps=small_scan["Ps"], imgs=np.ascontiguousarray(small_scan["imgs"], np.float32), n_u=small_scan["n_u"],
                n_v=small_scan["n_v"])


def _metric(ctx, s, dkappa=0.0, fbcc=False, Ps=None):
    import epipolarconsistency_amd as E
    return E.MetricDirect(ctx, s["Ps"] if Ps is None else Ps, s["imgs"]).setEpipolarPlaneStep(dkappa).setFanBeamConsistency(fbcc)


def _shuffled_list(n, count=12, seed=7):
    """`count` ordered pairs (i, j), i != j, shuffled: reversed tuples (j, i) among them, the large scan's steep pairs included.
    Not the pairs six views apart of the 8-view scan: the reference's fan-beam weighting is not finite on some of their lines
    (oracle and evaluateForImagePair both return NaN for (0, 6) and (1, 7)), and NaN equals nothing, itself included."""
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j and abs(i - j) != 6]
    rng = np.random.RandomState(seed)
    rng.shuffle(pairs)
    pairs = pairs[:count]
    assert any(i > j for i, j in pairs) and any(i < j for i, j in pairs)
    return np.asarray([(i, j, i, j) for i, j in pairs], np.int32)


def _perturbed(P, k=0):
    from epipolarconsistency_amd import geometry
    return P @ geometry.rigid_transform(tx=1.5 + 0.5 * k, ty=-0.7, rz=0.01 * (k + 1))


def kernel_sum(vals):
    """direct_sum_kernel's order in numpy: 1024 strided partials, the shuffle tree of every wave, the 16 wave sums in order."""
    vals = np.asarray(vals, np.float64)
    part = np.zeros(1024, np.float64)
    for k, v in enumerate(vals):
        part[k % 1024] += v
    tot = np.float64(0.0)
    lane = np.arange(64)
    for w in range(16):
        a = part[64 * w:64 * w + 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            a = a + np.where(lane + off < 64, a[np.minimum(lane + off, 63)], a)  # __shfl_down: the own value past the wave's end
        tot += a[0]
    return float(tot)


@pytest.mark.parametrize("scan,dkappa,fbcc", CONFIGS)
def test_entries_have_the_bits_of_the_single_pair_call(gpu_ctx, small_scan, scan, dkappa, fbcc):
    s = _scan(scan, small_scan)
    n = len(s["Ps"])
    m = _metric(gpu_ctx, s, dkappa, fbcc)
    idx = _shuffled_list(n)
    total, vals = m.evaluate_pairs(idx, want_pairs=True)
    assert vals.dtype == np.float64 and len(vals) == len(idx) and np.all(vals > 0)  # (NaN fails this)
    for q, (i, j, _, _) in enumerate(idx):
        assert vals[q] == m.evaluateForImagePair(int(i), int(j))[0], (q, i, j)
    assert total == kernel_sum(vals)
    cost = np.zeros((n, n), np.float32)
    m.evaluate(cost)
    fwd = [q for q, t in enumerate(idx) if t[0] < t[1]]
    assert len(fwd) >= 2
    for q in fwd:
        assert np.float32(vals[q]) == cost[idx[q][1], idx[q][0]], q
    m.close()


@pytest.mark.parametrize("scan,partner", [("small", 5), ("large", 1)])
def test_matrix_and_image_indices_are_independent(gpu_ctx, small_scan, scan, partner):
    s = _scan(scan, small_scan)
    n = len(s["Ps"])
    table = list(s["Ps"]) + [_perturbed(s["Ps"][3], 0), _perturbed(s["Ps"][3], 1)]
    m = _metric(gpu_ctx, s, Ps=table)
    _, vals = m.evaluate_pairs([(n, partner, 3, partner), (3, partner, 3, partner), (partner, n + 1, partner, 3)], want_pairs=True)
    for row, q, (i, j) in ((n, 0, (3, partner)), (n + 1, 2, (partner, 3))):
        Ps = list(s["Ps"])
        Ps[3] = table[row]
        other = _metric(gpu_ctx, s, Ps=Ps)
        assert vals[q] == other.evaluateForImagePair(i, j)[0]
        other.close()
    assert vals[0] != vals[1]
    assert vals[1] == m.evaluateForImagePair(3, partner)[0]
    assert m.getNumberOfProjetions() == n and m.evaluate() > 0  # the longer table leaves the all-pairs call to the n images
    m.close()


@pytest.mark.parametrize("scan,dkappa,fbcc", CONFIGS)
def test_entries_against_the_oracle(gpu_ctx, oracle_mod, small_scan, scan, dkappa, fbcc):
    s = _scan(scan, small_scan)
    n = len(s["Ps"])
    table = list(s["Ps"]) + [_perturbed(s["Ps"][3], 0)]
    m = _metric(gpu_ctx, s, dkappa, fbcc, Ps=table)
    idx = np.concatenate([_shuffled_list(n, count=5, seed=11), np.asarray([(n, 1, 3, 1), (0, n, 2, 3)], np.int32)])
    _, vals = m.evaluate_pairs(idx, want_pairs=True)
    radius = oracle_mod.object_radius(table[0], s["n_u"], s["n_v"])
    for q, (p0, p1, i0, i1) in enumerate(idx):
        want = oracle_mod.direct_pair(table[p0], table[p1], s["imgs"][i0], s["imgs"][i1], dkappa, radius, fbcc=fbcc)["metric"]
        rel = abs(vals[q] - want) / abs(want)
        print("entry %d (%d, %d, %d, %d): %.9g, oracle %.9g, rel %.2e" % (q, p0, p1, i0, i1, vals[q], want, rel))
        assert rel < 1e-5, (q, vals[q], want)
    m.close()


def test_segment_sums(gpu_ctx, small_scan):
    import epipolarconsistency_amd as E
    s = _scan("small", small_scan)
    n = 5
    m = E.MetricDirect(gpu_ctx, s["Ps"][:n], s["imgs"][:n])
    all_pairs = np.asarray([E.get_ij(ij, n) * 2 for ij in range(n * (n - 1) // 2)], np.int32)
    assert m.evaluate_pairs(all_pairs) == m.evaluate()  # one segment, one batch: the all-pairs sum, bit for bit
    assert m.evaluate_pairs(all_pairs, segments=[0, len(all_pairs)])[0] == m.evaluate()
    idx = np.concatenate([all_pairs[::-1], all_pairs[::-1], all_pairs[3:8]])
    sums, vals = m.evaluate_pairs(idx, segments=[0, 0, 10, 10, 20, 25, 25], want_pairs=True)
    assert sums[1] == sums[3] and sums[1] > 0  # identical segments, identical sums
    assert list(sums[[0, 2, 5]]) == [0.0, 0.0, 0.0]  # empty segments
    for k, (a, b) in enumerate(((0, 0), (0, 10), (10, 10), (10, 20), (20, 25), (25, 25))):
        assert sums[k] == kernel_sum(vals[a:b]), k
    only_sums = m.evaluate_pairs(idx, segments=[0, 10, 25])
    assert only_sums[0] == sums[1] and only_sums[1] == kernel_sum(vals[10:25])
    m.close()


def test_a_long_segment_is_added_in_the_kernels_order(gpu_ctx, small_scan):
    """More values than the summing workgroup has threads: strided partials of two values, every wave's tree in play."""
    s = _scan("small", small_scan)
    m = _metric(gpu_ctx, s, dkappa=0.02)  # (few lines per pair: 1100 entries stay a fraction of a second)
    idx = np.tile(_shuffled_list(8, count=11, seed=3), (100, 1))
    total, vals = m.evaluate_pairs(idx, want_pairs=True)
    assert np.array_equal(vals[:11], vals[-11:]) and total == kernel_sum(vals)
    m.close()


def test_batch_borders(gpu_ctx, small_scan):
    s = _scan("small", small_scan)
    m = _metric(gpu_ctx, s)
    idx = _shuffled_list(8, count=10, seed=5)
    segments = [0, 2, 7, 10]  # against batches [0, 3), [3, 6), [6, 9), [9, 10)
    want_sums, want_vals = m.evaluate_pairs(idx, segments=segments, want_pairs=True)
    got_sums, got_vals = m.debug_set_batch(3).evaluate_pairs(idx, segments=segments, want_pairs=True)
    assert np.array_equal(got_vals, want_vals) and np.array_equal(got_sums, want_sums)
    back_sums, back_vals = m.debug_set_batch(0).evaluate_pairs(idx, segments=segments, want_pairs=True)
    assert np.array_equal(back_vals, want_vals) and np.array_equal(back_sums, want_sums)
    m.close()


def test_pose_deltas(gpu_ctx, small_scan):
    import epipolarconsistency_amd as E
    s = _scan("small", small_scan)
    n = len(s["Ps"])
    m = _metric(gpu_ctx, s)
    before = m.evaluate()
    moved_views = [[3]] * 5 + [[6, 2]]
    moved_Ps = [[_perturbed(s["Ps"][3], k)] for k in range(5)] + [[_perturbed(s["Ps"][6], 1), _perturbed(s["Ps"][2], 2)]]
    sums, terms, tuples = m.evaluate_pose_deltas(moved_views, moved_Ps, want_pairs=True)
    assert m.evaluate() == before  # the set matrices were not disturbed
    counts = [len(E.direct_pose_pairs(n, v)) for v in moved_views]
    assert counts == [7] * 5 + [13] and len(terms) == sum(counts) == len(tuples)
    assert np.array_equal(tuples, np.concatenate([E.direct_pose_pairs(n, v) for v in moved_views]))
    # the same terms from evaluate_pairs with the candidates as further rows of the matrix table
    candidates = [P for Pk in moved_Ps for P in Pk]
    table = _metric(gpu_ctx, s, Ps=list(s["Ps"]) + candidates)
    idx, segments, row = [], [0], n
    for views in moved_views:
        row_of = {v: row + q for q, v in enumerate(views)}
        row += len(views)
        for (i, j, _, _) in E.direct_pose_pairs(n, views):
            idx.append((row_of.get(i, i), row_of.get(j, j), i, j))
        segments.append(len(idx))
    want_sums, want_terms = table.evaluate_pairs(idx, segments=segments, want_pairs=True)
    assert np.array_equal(terms, want_terms) and np.array_equal(sums, want_sums)
    table.close()
    # ... and from setProjectionMatrices(pose k) + evaluateForImagePair
    at = 0
    for views, Pk in zip(moved_views, moved_Ps):
        Ps = list(s["Ps"])
        for v, P in zip(views, Pk):
            Ps[v] = P
        seq = _metric(gpu_ctx, s, Ps=Ps)
        for (i, j, _, _) in E.direct_pose_pairs(n, views):
            assert terms[at] == seq.evaluateForImagePair(int(i), int(j))[0], (views, i, j)
            at += 1
        seq.close()
    assert np.array_equal(m.evaluate_pose_deltas(moved_views, moved_Ps), sums) and m.evaluate() == before
    m.close()


def test_a_pose_that_moves_view_0_takes_its_own_object_radius(gpu_ctx, small_scan):
    """Under the automatic radius Metric::getObjectRadius is the FIRST view's estimate: the pose's own, where it moves view 0."""
    from epipolarconsistency_amd import geometry
    s = _scan("small", small_scan)
    m = _metric(gpu_ctx, s)
    P0 = s["Ps"][0] @ geometry.rigid_transform(tz=25.0, tx=3.0)
    seq = _metric(gpu_ctx, s, Ps=[P0] + list(s["Ps"][1:]))
    assert seq.getObjectRadius() != m.getObjectRadius()
    sums, terms, tuples = m.evaluate_pose_deltas([[0]], [[P0]], want_pairs=True)
    for q, (i, j, _, _) in enumerate(tuples):
        assert terms[q] == seq.evaluateForImagePair(int(i), int(j))[0]
    assert sums[0] == kernel_sum(terms)
    seq.close()
    m.close()


def test_refusals_and_empties(gpu_ctx, small_scan):
    import epipolarconsistency_amd as E
    s = _scan("small", small_scan)
    n = len(s["Ps"])
    unset = E.MetricDirect(gpu_ctx, None, s["imgs"])
    with pytest.raises(E.EccError, match="have not been set"):
        unset.evaluate_pairs([(0, 1, 0, 1)])
    with pytest.raises(E.EccError, match="have not been set"):
        unset.evaluate_pose_deltas([[1]], [[s["Ps"][1]]])
    unset.close()
    m = _metric(gpu_ctx, s)
    before = m.evaluate()
    good = (0, 1, 0, 1)
    for bad, text in (((n, 1, 0, 1), "entry 1: matrix index %d out of range" % n), ((0, -1, 0, 1), "entry 1: matrix index -1"),
                      ((0, 1, n, 1), "entry 1: image index %d out of range" % n), ((0, 1, 0, -2), "entry 1: image index -2"),
                      ((4, 4, 0, 1), r"entry 1: P0 == P1 \(4\)")):
        with pytest.raises(E.EccError, match=text):
            m.evaluate_pairs([good, bad])
    for segments, text in (([0, 2, 1, 3], "segment offsets decrease at entry 2"), ([0, 1, 2], "end at 2, not at the list length 3"),
                           ([1, 3], "do not start at 0")):
        with pytest.raises(E.EccError, match=text):
            m.evaluate_pairs([good] * 3, segments=segments)
    with pytest.raises(E.EccError, match="more than 2\\^20 pairs"):
        m.evaluate_pairs(np.tile(np.asarray(good, np.int32), ((1 << 20) + 1, 1)))
    P = [s["Ps"][2], s["Ps"][2]]
    with pytest.raises(E.EccError, match="pose 1 names view 2 twice"):
        m.evaluate_pose_deltas([[2], [2, 2]], [P[:1], P])
    with pytest.raises(E.EccError, match="pose 0: view index %d out of range" % n):
        m.evaluate_pose_deltas([[n]], [P[:1]])
    flat = np.repeat(np.asarray(E.pack_projection_matrices(P[:1]), np.float64).reshape(1, 12), 3, axis=0)
    with pytest.raises(E.EccError, match="pose offsets decrease at entry 2"):
        m.evaluate_pose_deltas_packed([0, 2, 1, 3], [1, 2, 3], flat)
    K = (1 << 20) // (n - 1) + 1
    with pytest.raises(E.EccError, match="more than 2\\^20 pairs"):
        m.evaluate_pose_deltas_packed(np.arange(K + 1), np.full(K, 2), np.repeat(flat[:1], K, axis=0))
    # empties
    assert m.evaluate_pairs(np.zeros((0, 4), np.int32)) == 0.0
    sums, vals = m.evaluate_pairs([], segments=[0, 0, 0], want_pairs=True)
    assert list(sums) == [0.0, 0.0] and len(vals) == 0
    assert len(m.evaluate_pose_deltas([], [])) == 0
    sums, vals, tuples = m.evaluate_pose_deltas([[], []], [[], []], want_pairs=True)
    assert list(sums) == [0.0, 0.0] and len(vals) == 0 and tuples.shape == (0, 4)
    # a metric that refused still evaluates
    assert m.evaluate() == before and m.evaluate_pairs([good]) == m.evaluateForImagePair(0, 1)[0]
    m.close()
