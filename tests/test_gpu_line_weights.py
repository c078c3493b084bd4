"""Line weights made on the device (csrc/ecc_line_weights.hip, csrc/line_weights_kernel.hip) on the GPU.  Every
comparison is on uint32 / uint64 views, bit for bit.

  1  line_weights_device == line_weights on the numpy-dilated image: two image shapes, eight grids (window larger than the grid,
     pitch with no padding beyond the border and with 31 floats of it), single image and stack of 2, host and torch input; with
     out= the WHOLE slab -- elements, replicated border, zero padding -- against the slab built in numpy;
  2  a stack of 65 images crosses the 64-image sub-batch of the scratch;
  3  one case against the oracle's transform (exact Radon arithmetic);
  4  a metric over device-made weights == a metric over uploaded weights, in three sampling modes, with a flagged region at the
     detector's edge;
  5  the tracker's sequence: out= into the slab of one view + refreshRadonIntermediates, two frames;
  6  RadonIntermediate.line_weights_from (ecc_dtr_line_weights);
  7  repeatability, nothing else moved, argument errors with a real context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _close(dtrs):
    for d in dtrs:
        d.close()


def numpy_dilate(flagged, r):
    """Maximum over the (2 r + 1)^2 square, indices clamped to the image (pad(mode="edge")); (n_v, n_u) or (n, n_v, n_u)."""
    f = np.asarray(flagged, np.float32)
    if r == 0:
        return f.copy()
    if f.ndim == 3:
        return np.stack([numpy_dilate(x, r) for x in f])
    p = np.pad(f, r, mode="edge")
    n_v, n_u = f.shape
    out = f.copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.maximum(out, p[dy:dy + n_v, dx:dx + n_u])
    return out


def numpy_slab(field, slab_floats):
    """(n_t, n_alpha) weights -> the private layout of csrc/ecc_layout.h: element (ix, iy) at [(ix + 1) * pitch + iy + 1], one
    replicated border row / column on every side, zeros in the pitch padding."""
    n_t, n_alpha = field.shape
    pitch = slab_floats // (n_alpha + 2)
    assert pitch * (n_alpha + 2) == slab_floats and pitch % 32 == 0 and n_t + 2 <= pitch < n_t + 2 + 32
    s = np.zeros((n_alpha + 2, pitch), np.float32)
    s[:, :n_t + 2] = np.pad(np.ascontiguousarray(field.T), 1, mode="edge")
    return s.reshape(-1)


def _images(key):
    """Two flagged images of one shape: [0] the one the issue names, [1] a companion for the stack."""
    if key == "128":
        a = np.zeros((128, 128), np.float32)
        a[47:65, 55:71] = 1.0                  # a block
        b = np.zeros((128, 128), np.float32)
        b[:, 90:92] = 1.0                      # a defective column pair
        b[100:128, 0:9] = 1.0                  # and a blade in a corner
    else:
        a = np.zeros((96, 72), np.float32)     # n_v x n_u
        a[:, 40:42] = 1.0                      # a two-column defect
        a[0, 0] = 1.0                          # a flagged corner pixel
        b = np.zeros((96, 72), np.float32)
        b[30:50, 60:72] = 1.0                  # a block at the right edge
        b[95, 71] = 1.0
    return np.stack([a, b])


# (n_alpha, n_t, zero_at, guard, dilate); n_t = 30 and 62: the pitch (32, 64) has no padding beyond the border; n_t = 31: 31 floats of it
GRIDS = [(96, 96, 1.0, 1, 0), (80, 56, 2.5, 2, 3), (48, 40, 1.0, 0, 0), (33, 97, 1.0, 8, 16), (3, 5, 1.0, 8, 1),
         (24, 30, 1.0, 1, 0), (20, 62, 1.5, 1, 2), (24, 31, 1.0, 2, 1)]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d_z%g_g%d_d%d" % g)
@pytest.mark.parametrize("key", ["128", "96x72"])
def test_equals_line_weights(gpu_ctx, key, grid):
    import torch
    import epipolarconsistency_amd as E
    n_alpha, n_t, zero_at, guard, dilate = grid
    stack = _images(key)
    n_v, n_u = stack.shape[1:]
    ref = E.line_weights(gpu_ctx, numpy_dilate(stack, dilate), n_alpha, n_t, zero_at, guard)
    want = [d.readback().copy() for d in ref]
    _close(ref)
    assert all(w.shape == (n_t, n_alpha) for w in want) and want[0].min() < 1.0

    def same(dtrs, fields, what):
        for k, (d, w) in enumerate(zip(dtrs, fields)):
            assert d.getFilter() == E.FILTER_NONE, what
            assert (d.getRadonBinNumber(0), d.getRadonBinNumber(1), d.getOriginalImageSize(0), d.getOriginalImageSize(1)) == (n_alpha, n_t, n_u, n_v)
            got = d.readback()
            assert np.array_equal(_u32(got), _u32(w)), (what, k, int((_u32(got) != _u32(w)).sum()), float(np.abs(got - w).max()))

    kw = dict(zero_at_px=zero_at, guard_bins=guard, dilate_px=dilate)
    one = E.line_weights_device(gpu_ctx, stack[0], n_alpha, n_t, **kw)                       # host, single
    assert isinstance(one, E.RadonIntermediate)
    same([one], want[:1], "host single")
    both = E.line_weights_device(gpu_ctx, stack, n_alpha, n_t, **kw)                         # host, stack of 2
    assert isinstance(both, list) and len(both) == 2
    same(both, want, "host stack")
    dev = torch.from_numpy(stack).cuda()
    one_t = E.line_weights_device(gpu_ctx, dev[0].contiguous(), n_alpha, n_t, **kw)          # torch, single
    same([one_t], want[:1], "torch single")
    both_t = E.line_weights_device(gpu_ctx, dev, n_alpha, n_t, **kw)                         # torch, stack of 2
    same(both_t, want, "torch stack")
    # out=: caller-owned slabs, every float of them written
    floats = E.slab_floats(n_alpha, n_t)
    slabs = torch.full((2, floats), float("nan"), dtype=torch.float32, device="cuda")
    into = E.line_weights_device(gpu_ctx, dev, n_alpha, n_t, out=slabs, **kw)
    same(into, want, "out=")
    got = slabs.cpu().numpy()
    for k in range(2):
        assert np.array_equal(_u32(got[k]), _u32(numpy_slab(want[k], floats))), ("slab", k)
    _close([one] + both + [one_t] + both_t + into)


def test_sub_batches(gpu_ctx):
    """65 images of 16 x 12 at 12 x 10 bins: the 65th goes through the scratch (lengths and dilated images) in a second sub-batch.
    Every handle equals the result of its image alone, and that of line_weights on the dilated image."""
    import epipolarconsistency_amd as E
    rng = np.random.default_rng(17)
    stack = (rng.random((65, 16, 12)) < 0.04).astype(np.float32)
    stack[64, 3:6, 8:12] = 1.0
    stack[0, 10:12, 0:2] = 1.0
    kw = dict(zero_at_px=1.0, guard_bins=1, dilate_px=1)
    all_at_once = E.line_weights_device(gpu_ctx, stack, 12, 10, **kw)
    got = [d.readback().copy() for d in all_at_once]
    assert len(got) == 65 and len(set(g.tobytes() for g in got)) > 32    # the images differ, and so do their weights
    for k in range(65):
        alone = E.line_weights_device(gpu_ctx, stack[k], 12, 10, **kw)
        assert np.array_equal(_u32(got[k]), _u32(alone.readback())), k
        alone.close()
    for k in (0, 31, 63, 64):
        ref = E.line_weights(gpu_ctx, numpy_dilate(stack[k], 1), 12, 10, 1.0, 1)
        assert np.array_equal(_u32(got[k]), _u32(ref.readback())), k
        ref.close()
    _close(all_at_once)


def test_against_the_oracles_transform(gpu_ctx, oracle_mod):
    """In the exact Radon arithmetic: the oracle's FILTER_NONE transform of the numpy-dilated image put through
    line_weights_from_lengths, bit for bit."""
    import epipolarconsistency_amd as E
    assert gpu_ctx.getRadonArithmetic() == "exact"
    flagged = _images("128")[1]
    n_alpha, n_t, zero_at, guard, dilate = 80, 56, 2.5, 2, 3
    want = E.line_weights_from_lengths(oracle_mod.radon(numpy_dilate(flagged, dilate), n_alpha, n_t, filter=E.FILTER_NONE), zero_at, guard)
    d = E.line_weights_device(gpu_ctx, flagged, n_alpha, n_t, zero_at, guard, dilate)
    assert np.array_equal(_u32(d.readback()), _u32(want)) and 0.0 < (want == 0).mean() < 1.0
    d.close()


# ---- the slab, not only its elements: a metric over the weights ----------------------------------------------------------------------
BAD_VIEW, BINS, MARGIN = 3, 96, 3


def _mask(frame):
    """A flagged region that reaches the detector's edge and a corner (frame 0), another one (frame 1)."""
    f = np.zeros((128, 128), np.float32)
    if frame == 0:
        f[0:40, 100:128] = 1.0
    else:
        f[70:128, 0:22] = 1.0
        f[20:30, 60:70] = 1.0
    return f


def _uploaded(ctx, frame):
    """The weights of a frame the existing way: numpy dilation, line_weights (readback, numpy, from_host)."""
    import epipolarconsistency_amd as E
    return E.line_weights(ctx, numpy_dilate(_mask(frame), MARGIN), BINS, BINS, guard_bins=1)


def _ones(ctx, n):
    import epipolarconsistency_amd as E
    return [E.RadonIntermediate.from_host(ctx, np.ones((BINS, BINS), np.float32), 128, 128, filter=E.FILTER_NONE) for _ in range(n)]


def _weighted(ctx, Ps, data, ws, sampling):
    import epipolarconsistency_amd as E
    m = E.MetricRadonIntermediate(ctx, Ps, data + ws).setSampling(sampling)
    out = m.evaluate_weighted(want_pairs=True)
    m.close()
    return out


def _same_result(a, b, what):
    assert _u64(a[0])[()] == _u64(b[0])[()] and _u64(a[1])[()] == _u64(b[1])[()], (what, a[:2], b[:2])
    assert np.array_equal(_u32(a[2]), _u32(b[2])), (what, int((_u32(a[2]) != _u32(b[2])).sum()))


@pytest.mark.parametrize("sampling", ["polynomial", "per_sample", "auto"])
def test_a_metric_sees_the_same_slab(gpu_ctx, small_scan, sampling):
    """8 views at 96^2 bins, weights for view 3 from a region at the detector's edge (ones elsewhere): device-made against uploaded.
    "auto" resolves to the reference arithmetic for 28 pairs, which samples the slabs themselves, border rows and columns included."""
    import epipolarconsistency_amd as E
    Ps, imgs = small_scan["Ps"], small_scan["imgs"]
    n = len(Ps)
    data = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), BINS, BINS)
    ones = _ones(gpu_ctx, n)
    up = _uploaded(gpu_ctx, 0)
    dev = E.line_weights_device(gpu_ctx, _mask(0), BINS, BINS, guard_bins=1, dilate_px=MARGIN)
    field = dev.readback()
    # the angle bins at both ends of the grid (and with them the border rows of the slab) carry weights other than 1
    assert field[:, 0].min() < 1.0 and field[:, -1].min() < 1.0 and field.max() == 1.0 and field.min() == 0.0
    print("distance bins at the grid's ends: min weight %.3g / %.3g" % (field[0].min(), field[-1].min()))
    res = {}
    for key, w in (("uploaded", up), ("device", dev)):
        res[key] = _weighted(gpu_ctx, Ps, data, ones[:BAD_VIEW] + [w] + ones[BAD_VIEW + 1:], sampling)
    _same_result(res["device"], res["uploaded"], sampling)
    plain = _weighted(gpu_ctx, Ps, data, ones, sampling)
    assert res["device"][1] < 1.0 == plain[1] and not np.array_equal(_u32(res["device"][2]), _u32(plain[2]))   # the weights are seen
    _close(data + ones + [up, dev])


def test_into_and_refresh_is_the_fresh_metric(gpu_ctx, small_scan):
    """The tracker's sequence: a metric over wrapped torch slabs with all weights 1; per frame line_weights_device(out=the slab of
    view 3), refreshRadonIntermediates(n + 3, 1), evaluate_weighted -- the bits of a fresh metric over uploaded weights, twice."""
    import torch
    import epipolarconsistency_amd as E
    Ps, imgs = small_scan["Ps"], small_scan["imgs"]
    n = len(Ps)
    floats = E.slab_floats(BINS, BINS)
    images_t = torch.from_numpy(np.asarray(imgs, np.float32)).cuda()
    data_slabs = torch.empty((n, floats), dtype=torch.float32, device="cuda")
    data = E.RadonIntermediate.compute_into(gpu_ctx, images_t, data_slabs, BINS, BINS)
    weight_slabs = torch.full((n, floats), float("nan"), dtype=torch.float32, device="cuda")
    nothing = torch.zeros((n, 128, 128), dtype=torch.float32, device="cuda")
    ws = E.line_weights_device(gpu_ctx, nothing, BINS, BINS, out=weight_slabs)      # nothing flagged: every weight 1
    assert bool((weight_slabs.reshape(n, BINS + 2, -1)[:, :, :BINS + 2] == 1.0).all())
    ones = _ones(gpu_ctx, n)
    for sampling in ("polynomial", "auto"):
        m = E.MetricRadonIntermediate(gpu_ctx, Ps, data + ws).setSampling(sampling)
        _same_result(m.evaluate_weighted(want_pairs=True), _weighted(gpu_ctx, Ps, data, ones, sampling), "all ones " + sampling)
        for frame in (0, 1, 0):
            mask_t = torch.from_numpy(_mask(frame)).cuda()
            h = E.line_weights_device(gpu_ctx, mask_t, BINS, BINS, guard_bins=1, dilate_px=MARGIN, out=weight_slabs[BAD_VIEW:BAD_VIEW + 1])
            m.refreshRadonIntermediates(n + BAD_VIEW, 1)
            got = m.evaluate_weighted(want_pairs=True)
            up = _uploaded(gpu_ctx, frame)
            fresh = _weighted(gpu_ctx, Ps, data, ones[:BAD_VIEW] + [up] + ones[BAD_VIEW + 1:], sampling)
            _same_result(got, fresh, "%s frame %d" % (sampling, frame))
            assert got[1] < 1.0
            _close([h, up])
        m.close()
        E.line_weights_device(gpu_ctx, nothing[BAD_VIEW], BINS, BINS, out=weight_slabs[BAD_VIEW:BAD_VIEW + 1]).close()   # ones again
    _close(data + ws + ones)


def test_line_weights_from_a_length_intermediate(gpu_ctx):
    """ecc_dtr_line_weights on a FILTER_NONE intermediate == line_weights_from_lengths of its readback; a derivative one is refused."""
    import epipolarconsistency_amd as E
    stack = _images("96x72")
    for n_alpha, n_t, zero_at, guard in ((48, 40, 1.0, 0), (33, 31, 2.5, 2), (3, 5, 1.0, 8), (80, 62, 0.5, 8)):
        lengths = E.RadonIntermediate.compute_batch(gpu_ctx, stack, n_alpha, n_t, E.FILTER_NONE)
        for d in lengths:
            want = E.line_weights_from_lengths(d.readback(), zero_at, guard)
            w = E.RadonIntermediate.line_weights_from(d, zero_at, guard)
            assert w.getFilter() == E.FILTER_NONE and (w.getOriginalImageSize(0), w.getOriginalImageSize(1)) == (72, 96)
            assert np.array_equal(_u32(w.readback()), _u32(want)), (n_alpha, n_t, zero_at, guard)
            w.close()
        _close(lengths)
    deriv = E.RadonIntermediate.compute(gpu_ctx, stack[0], 48, 40)
    with pytest.raises(E.EccError) as e:
        E.RadonIntermediate.line_weights_from(deriv)
    assert e.value.code == 1 and "ECC_FILTER_NONE" in str(e.value)
    deriv.close()


def test_repeatable_and_nothing_else_moved(gpu_ctx, small_scan):
    """Two calls give the same bits; evaluate(), evaluate_weighted() and a RadonIntermediate.compute of a data image around the calls
    return what they returned before (the Radon kernel's transposed-image scratch in the context is shared)."""
    import epipolarconsistency_amd as E
    Ps, imgs = small_scan["Ps"], small_scan["imgs"]
    n = len(Ps)
    data = E.RadonIntermediate.compute_batch(gpu_ctx, np.asarray(imgs, np.float32), BINS, BINS)
    ones = _ones(gpu_ctx, n)
    up = _uploaded(gpu_ctx, 1)
    m = E.MetricRadonIntermediate(gpu_ctx, Ps, data + ones[:BAD_VIEW] + [up] + ones[BAD_VIEW + 1:])

    def observe():
        d = E.RadonIntermediate.compute(gpu_ctx, np.asarray(imgs[5], np.float32), BINS, BINS)
        field = d.readback().copy()
        d.close()
        return m.evaluate(), m.evaluate_weighted(want_pairs=True), field
    before = observe()
    kw = dict(zero_at_px=1.0, guard_bins=2, dilate_px=MARGIN)
    first = E.line_weights_device(gpu_ctx, np.stack([_mask(0), _mask(1)]), 80, 56, **kw)
    second = E.line_weights_device(gpu_ctx, np.stack([_mask(0), _mask(1)]), 80, 56, **kw)
    for a, b in zip(first, second):
        assert np.array_equal(_u32(a.readback()), _u32(b.readback()))
    after = observe()
    assert _u64(before[0])[()] == _u64(after[0])[()]
    _same_result(before[1], after[1], "evaluate_weighted around the call")
    assert np.array_equal(_u32(before[2]), _u32(after[2])) and np.array_equal(_u32(before[2]), _u32(data[5].readback()))
    m.close()
    _close(data + ones + [up] + first + second)


def test_errors_with_a_context(gpu_ctx):
    import torch
    import epipolarconsistency_amd as E
    flagged = _images("96x72")[0]
    lengths = E.RadonIntermediate.compute(gpu_ctx, flagged, 24, 30, E.FILTER_NONE)
    slab = torch.full((1, E.slab_floats(24, 30)), -1.0, dtype=torch.float32, device="cuda")
    dev = torch.from_numpy(flagged).cuda()
    for bad in (dict(dilate_px=-1), dict(dilate_px=17), dict(guard_bins=-1), dict(guard_bins=9), dict(zero_at_px=0.0),
                dict(zero_at_px=-2.0), dict(zero_at_px=float("nan")), dict(zero_at_px=float("inf"))):
        calls = [lambda: E.line_weights_device(gpu_ctx, flagged, 24, 30, **bad),
                 lambda: E.line_weights_device(gpu_ctx, dev, 24, 30, out=slab, **bad)]
        if "dilate_px" not in bad:   # line_weights_from has no dilate_px to pass
            calls.append(lambda: E.RadonIntermediate.line_weights_from(lengths, **bad))
        for call in calls:
            with pytest.raises(E.EccError) as e:
                call()
            assert e.value.code == 1 and list(bad)[0] in str(e.value), (bad, e.value)
    with pytest.raises(E.EccError):
        E.line_weights_device(gpu_ctx, flagged, 0, 30)
    with pytest.raises(ValueError):
        E.line_weights_device(gpu_ctx, flagged, 24, 30, out=slab)   # out= needs the image on the device
    assert bool((slab == -1.0).all())   # nothing written
    lengths.close()
