"""Host-side mirror of the reference's operator interface for the hot path, on top of the C ABI.

Same names, argument meaning and error behaviour as
  EpipolarConsistency::RadonIntermediate        ref: code/LibEpipolarConsistency/RadonIntermediate.h:18-128
  EpipolarConsistency::MetricRadonIntermediate  ref: code/LibEpipolarConsistency/EpipolarConsistencyRadonIntermediate.h:21-106
  EpipolarConsistency::Metric                   ref: code/LibEpipolarConsistency/EpipolarConsistency.h:49-94
(the reference is C++; the C++ adapter with the same class names is cpp/EpipolarConsistencyHip.hxx --
this module is the Python face used by tests/ and bench.py).  All arithmetic happens in
libecc_hip.so; numpy/torch only carry buffers.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (FILTER_DERIVATIVE, FILTER_NONE, FILTER_RAMP, POST_IDENTITY, POST_LOGARITHM,
                   POST_SQUARE_ROOT, EccError, check)


def pack_projection_matrices(Ps):
    """Public alias: list of 3x4 -> (n, 12) float64 column-major per view."""
    return _Ps_colmajor(Ps)


def _Ps_colmajor(Ps):
    """List/array of 3x4 matrices -> contiguous n x 12 float64, column-major per view (Eigen)."""
    A = np.asarray(Ps, dtype=np.float64).reshape(-1, 3, 4)
    return np.ascontiguousarray(A.transpose(0, 2, 1)).reshape(-1, 12)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Context:
    """One (device, stream) pair; replaces the reference's implicit current device + default
    stream + cudaDeviceSynchronize after each launch."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        check(_lib.lib().ecc_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(self._h)))
        self.device = int(device)

    def synchronize(self):
        check(_lib.lib().ecc_ctx_synchronize(self._h))

    def enable_timing(self, on=True):
        check(_lib.lib().ecc_ctx_enable_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self, which):
        """which: 'pairs', 'radon' or 'preprocess' -- HIP-event time of the last such kernel on this stream."""
        ms = C.c_float()
        check(_lib.lib().ecc_ctx_last_kernel_ms(self._h, {"pairs": 0, "radon": 1, "preprocess": 2}[which], C.byref(ms)))
        return ms.value

    def debugSetQuadCopies(self, on=True):
        """ecc_debug_set_quad_copies (experiments' old name): setQuadCopies("on" / "off")."""
        check(_lib.lib().ecc_debug_set_quad_copies(self._h, 1 if on else 0))
        return self

    def setQuadCopies(self, mode="auto"):
        """ecc_ctx_set_quad_copies: whether metrics created from this context afterwards build row-quad copies of their Radon
        intermediates (4x the slab memory; the exact part of the kappa_max = pi/2 pairs samples them; same bits): "auto"
        (default: while they fit a quarter of the free device memory), "off", "on"."""
        check(_lib.lib().ecc_ctx_set_quad_copies(self._h, {"auto": -1, "off": 0, "on": 1}[mode]))
        return self

    def setRadonArithmetic(self, mode="exact"):
        """ecc_radon_set_arithmetic: "exact" (default; unfused fp32, bit-identical to the oracle's normative variant) or
        "fma" (contracted sampling loop, bit-identical to the oracle's contracted variant, ~25 % faster)."""
        check(_lib.lib().ecc_radon_set_arithmetic(self._h, {"exact": _lib.RADON_EXACT, "fma": _lib.RADON_FMA}[mode]))
        return self

    def getRadonArithmetic(self):
        v = C.c_int()
        check(_lib.lib().ecc_radon_get_arithmetic(self._h, C.byref(v)))
        return {_lib.RADON_EXACT: "exact", _lib.RADON_FMA: "fma"}[v.value]

    def close(self):
        if self._h:
            _lib.lib().ecc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreProccess:  # sic, ref: struct EpipolarConsistency::PreProccess (Gui/PreProccess.h:14-50)
    """Pre-processing of X-ray projection images, same fields and defaults as the reference's struct
    (intensity.*, lowpass.*, image_geometry.*, border.*).  process() = PreProccess::process followed by
    apply_weight_cos_principal_ray when projection matrices are given (call order of
    Gui/InputDataDirect.cpp:85-86), fused into one device kernel for a whole stack."""

    class _NS:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    def __init__(self):
        self.intensity = self._NS(normalize=False, bias=0.0, scale=1.0, apply_log=False)
        self.lowpass = self._NS(gaussian_sigma=1.84, half_kernel_width=5)
        self.image_geometry = self._NS(flip_u=False, flip_v=False)
        self.border = self._NS(zero=[1, 1, 1, 1], feather=[16, 16, 16, 16], blanks=[])

    def _config(self, process=True):
        cfg = _lib.PreprocessConfig()
        _lib.lib().ecc_preprocess_defaults(C.byref(cfg))
        cfg.process = 1 if process else 0
        cfg.normalize, cfg.bias, cfg.scale = int(self.intensity.normalize), self.intensity.bias, self.intensity.scale
        cfg.apply_log = int(self.intensity.apply_log)
        cfg.gaussian_sigma, cfg.half_kernel_width = self.lowpass.gaussian_sigma, int(self.lowpass.half_kernel_width)
        cfg.flip_u, cfg.flip_v = int(self.image_geometry.flip_u), int(self.image_geometry.flip_v)
        cfg.zero = (C.c_int32 * 4)(*[int(v) for v in self.border.zero])
        cfg.feather = (C.c_int32 * 4)(*[int(v) for v in self.border.feather])
        bl = np.ascontiguousarray(np.asarray(self.border.blanks, np.int32).reshape(-1, 4))
        cfg.n_blanks = len(bl)
        cfg.blanks = bl.ctypes.data if len(bl) else None
        return cfg, bl

    def _run(self, ctx, images, Ps, out, process):
        cfg, keep = self._config(process)
        Pp = None if Ps is None else _Ps_colmajor(Ps)
        if _is_torch(images):
            import torch
            assert images.dtype == torch.float32 and images.is_contiguous() and images.is_cuda and images.dim() == 3
            out = images if out is None else out
            assert out.shape == images.shape and out.is_contiguous() and out.is_cuda
            n, n_v, n_u = images.shape
            a, b, on_dev = images.data_ptr(), out.data_ptr(), 1
        else:
            images = np.ascontiguousarray(images, np.float32)
            assert images.ndim == 3
            out = np.empty_like(images) if out is None else out
            n, n_v, n_u = images.shape
            a, b, on_dev = images.ctypes.data, out.ctypes.data, 0
        assert Pp is None or len(Pp) == n
        check(_lib.lib().ecc_preprocess(ctx._h, C.c_void_p(a), on_dev, C.c_void_p(b), n, n_u, n_v, C.byref(cfg),
                                        C.c_void_p(Pp.ctypes.data) if Pp is not None else None))
        del keep
        return out

    def process(self, ctx, images, Ps=None, out=None):
        """images: (n, n_v, n_u) float32, numpy (host; returns a new array) or torch on ctx's device (in place
        unless `out` is given).  Ps: n projection matrices -> cosine weighting is applied as well."""
        return self._run(ctx, images, Ps, out, True)

    def apply_weight_cos_principal_ray(self, ctx, images, Ps, out=None):
        """ref: PreProccess::apply_weight_cos_principal_ray alone (Gui/PreProccess.cpp:146-166)."""
        return self._run(ctx, images, Ps, out, False)


class RadonIntermediate:
    """ref: class RadonIntermediate (RadonIntermediate.h:18-128)."""
    Derivative, Ramp, None_ = FILTER_DERIVATIVE, FILTER_RAMP, FILTER_NONE
    Identity, SquareRoot, Logarithm = POST_IDENTITY, POST_SQUARE_ROOT, POST_LOGARITHM

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle
        self._keep = None  # caller-owned device memory (torch tensor) when wrapping

    # -- constructors --------------------------------------------------------------------------
    @classmethod
    def compute(cls, ctx, image, size_alpha, size_t, filter=FILTER_DERIVATIVE, post_process=POST_IDENTITY):
        """ref: RadonIntermediate(projectionData, size_alpha, size_t, filter, post_process).
        image: (n_v, n_u) float32 numpy array (host) or torch tensor on ctx's device."""
        return cls.compute_batch(ctx, image[None] if not _is_torch(image) else image.unsqueeze(0),
                                 size_alpha, size_t, filter, post_process)[0]

    @classmethod
    def compute_batch(cls, ctx, images, size_alpha, size_t, filter=FILTER_DERIVATIVE, post_process=POST_IDENTITY):
        """images: (n, n_v, n_u) float32, numpy (host) or torch (device)."""
        if _is_torch(images):
            import torch
            assert images.dtype == torch.float32 and images.is_contiguous() and images.is_cuda
            n, n_v, n_u = images.shape
            ptr, on_dev, keep = images.data_ptr(), 1, images
        else:
            keep = np.ascontiguousarray(images, np.float32)
            n, n_v, n_u = keep.shape
            ptr, on_dev = keep.ctypes.data, 0
        hs = (C.c_void_p * n)()
        check(_lib.lib().ecc_radon_compute_batch(ctx._h, C.c_void_p(ptr), on_dev, n, n_u, n_v, size_alpha,
                                                 size_t, filter, post_process, hs))
        if on_dev:
            ctx.synchronize()  # the input tensor may be freed by the caller right after
        return [cls(ctx, C.c_void_p(h)) for h in hs]

    @classmethod
    def compute_into(cls, ctx, images, slabs, size_alpha, size_t, filter=FILTER_DERIVATIVE,
                     post_process=POST_IDENTITY):
        """Device-resident, asynchronous form: images (n, n_v, n_u) and slabs (n, slab_floats) are
        float32 torch tensors on ctx's device; returns handles that alias `slabs`."""
        n, n_v, n_u = images.shape
        assert images.is_contiguous() and slabs.is_contiguous()
        assert slabs.shape[0] == n and slabs.shape[1] == slab_floats(size_alpha, size_t)
        check(_lib.lib().ecc_radon_compute_into(ctx._h, C.c_void_p(images.data_ptr()), n, n_u, n_v, size_alpha,
                                                size_t, filter, post_process, C.c_void_p(slabs.data_ptr())))
        return [cls.wrap_device(ctx, slabs[k], size_alpha, size_t, n_u, n_v, filter) for k in range(n)]

    @classmethod
    def from_host(cls, ctx, data, n_u, n_v, filter=FILTER_DERIVATIVE):
        """ref: RadonIntermediate(const NRRD::ImageView<float>&) -- data is (n_t, n_alpha) float32."""
        data = np.ascontiguousarray(data, np.float32)
        n_t, n_alpha = data.shape
        h = C.c_void_p()
        check(_lib.lib().ecc_dtr_from_host(ctx._h, C.c_void_p(data.ctypes.data), n_alpha, n_t, n_u, n_v, filter,
                                           C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def line_weights_from(cls, lengths_dtr, zero_at_px=1.0, guard_bins=1, ctx=None):
        """ecc_dtr_line_weights: the clip and the guard minimum of line_weights_device alone, on the device, for a FILTER_NONE
        intermediate of lengths that exists already (e.g. loaded from a file); bit-identical to
        from_host(line_weights_from_lengths(lengths_dtr.readback(), zero_at_px, guard_bins)).  ctx: a context on the same device
        (default: the intermediate's own)."""
        ctx = lengths_dtr.ctx if ctx is None else ctx
        cfg = _line_weights_config(zero_at_px, guard_bins, 0)
        h = C.c_void_p()
        check(_lib.lib().ecc_dtr_line_weights(ctx._h, lengths_dtr._h, C.byref(cfg), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def load(cls, ctx, path):
        """ref: RadonIntermediate(const std::string path): a dtr NRRD written by the reference's tools
        (or by save()); returns (RadonIntermediate, info) where info carries the optional
        "Original Image/Projection Matrix"."""
        from . import nrrd
        data, info = nrrd.read_dtr(path)
        return cls.from_host(ctx, data, info["n_u"], info["n_v"], info["filter"]), info

    def save(self, path, projection_matrix=None):
        """ref: readback() + NRRD save with writePropertiesToMeta (RadonIntermediate.cpp:95-103,148-163)."""
        from . import nrrd
        nrrd.write_dtr(path, self.readback(), self.getOriginalImageSize(0), self.getOriginalImageSize(1),
                       self.getFilter(), projection_matrix)

    @classmethod
    def wrap_device(cls, ctx, slab, n_alpha, n_t, n_u, n_v, filter=FILTER_DERIVATIVE):
        """Adopt a torch tensor that already holds a dtr in the private layout (e.g. after an all-gather)."""
        h = C.c_void_p()
        check(_lib.lib().ecc_dtr_wrap_device(ctx._h, C.c_void_p(slab.data_ptr()), n_alpha, n_t, n_u, n_v, filter,
                                             C.byref(h)))
        r = cls(ctx, h)
        r._keep = slab
        return r

    # -- accessors -----------------------------------------------------------------------------
    def _info(self):
        a, t, u, v, f = (C.c_int() for _ in range(5))
        ba, bd = C.c_double(), C.c_double()
        check(_lib.lib().ecc_dtr_info(self._h, C.byref(a), C.byref(t), C.byref(u), C.byref(v), C.byref(f),
                                      C.byref(ba), C.byref(bd)))
        return a.value, t.value, u.value, v.value, f.value, ba.value, bd.value

    def getRadonBinNumber(self, dim):
        a, t = self._info()[:2]
        return t if dim else a

    def getOriginalImageSize(self, dim):
        u, v = self._info()[2:4]
        return v if dim else u

    def getRadonBinSize(self, dim=1):
        ba, bd = self._info()[5:7]
        return bd if dim else ba

    def getFilter(self):
        return self._info()[4]

    def isDerivative(self):
        return self.getFilter() == FILTER_DERIVATIVE

    def readback(self):
        """ref: readback() + data(): (n_t, n_alpha) float32, alpha fastest."""
        a, t = self._info()[:2]
        out = np.empty((t, a), np.float32)
        check(_lib.lib().ecc_dtr_readback(self._h, C.c_void_p(out.ctypes.data)))
        self._raw_cpu = out
        return out

    def clearRawData(self):
        """ref: clearRawData(): drop the host copy."""
        self._raw_cpu = None

    def data(self):
        """ref: data(): the host copy made by the last readback() (None before)."""
        return getattr(self, "_raw_cpu", None)

    def replaceRadonIntermediateData(self, radon_intermediate_image):
        """ref: replaceRadonIntermediateData(image) (RadonIntermediate.cpp:105-123): new dtr data from host memory,
        (n_t, n_alpha) float32, alpha fastest; original image size and filter are kept, the bin sizes follow the new
        shape.  Like in the reference a metric that already holds this object must be given the dtrs again
        (setRadonIntermediates)."""
        a = np.ascontiguousarray(radon_intermediate_image, np.float32)
        assert a.ndim == 2
        info = self._info()
        fresh = RadonIntermediate.from_host(self.ctx, a, info[2], info[3], filter=info[4])
        self.close()
        self._h, fresh._h = fresh._h, C.c_void_p()
        self._keep = None
        self._raw_cpu = a.copy()

    def tex2D(self, s, t):
        """ref: tex2D(s, t) (RadonIntermediate.h:108): HOST sample of the read-back data in texture coordinates
        [0, 1]^2 -- bilinear in binary64 on the (n - 1)-scaled grid with NRRD::ImageView's edge rule
        (HeaderOnly/NRRD/nrrd_image_view.hxx:159-205).  Call readback() first."""
        raw = self.data()
        if raw is None:
            raise ValueError("call readback() first")
        n_t, n_alpha = raw.shape
        x, y = (n_alpha - 1) * float(np.float32(s)), (n_t - 1) * float(np.float32(t))

        def cell(v, n):
            i = int(v)  # truncation, like the reference's (int)x
            f = v - i
            if i < 0:
                i, f = 0, 0.0
            if i > n - 2:
                i, f = n - 2, 1.0
            return i, f
        ix, fx = cell(x, n_alpha)
        iy, fy = cell(y, n_t)
        if fx == 0 and fy == 0:
            return float(np.float32(raw[iy, ix]))
        r = ((1.0 - fy) * ((1.0 - fx) * float(raw[iy, ix]) + fx * float(raw[iy, ix + 1]))
             + fy * ((1.0 - fx) * float(raw[iy + 1, ix]) + fx * float(raw[iy + 1, ix + 1])))
        return float(np.float32(r))

    def sample(self, line):
        """ref: sample(line) (RadonIntermediate.h:86-105): HOST sample for a line (l0, l1, l2) relative to the image
        centre; `line` (3 floats) is overwritten with the sample location like in the reference.  Returns the value,
        negated on the folded branch of a derivative dtr -- the evident intent, as for evaluateForImagePair: the
        reference's own flip test comes after lineToSampleDtr has already folded the angle and can never fire
        (RadonIntermediate.h:91-100)."""
        l = np.ascontiguousarray(line, np.float32).reshape(3).copy()
        range_t = np.float32(self.getRadonBinSize(1)) * np.float32(self.getRadonBinNumber(1))
        folded = _lib.lib().ecc_host_line_to_sample_dtr(C.c_void_p(l.ctypes.data), C.c_float(float(range_t)))
        try:
            line[:3] = l
        except TypeError:
            pass
        v = self.tex2D(l[0], l[1])
        return -v if (folded and self.isDerivative()) else v

    def device_view(self):
        base, pitch, rows = C.c_void_p(), C.c_int(), C.c_int()
        check(_lib.lib().ecc_dtr_device_view(self._h, C.byref(base), C.byref(pitch), C.byref(rows)))
        return base.value, pitch.value, rows.value

    def close(self):
        if self._h and self.ctx._h:  # after the context is gone its objects must not be touched any more
            _lib.lib().ecc_dtr_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pack_pose_lists(moved_views, moved_Ps):
    """Per-pose sequences of moved views and their matrices -> the packed (moved_offsets, moved_views, moved_Ps) of the C calls."""
    off = [0]
    views = []
    rows = []
    for vk, Pk in zip(moved_views, moved_Ps):
        vk = [int(v) for v in np.atleast_1d(vk)]
        Pk = np.asarray(Pk, np.float64)
        Pk = Pk.reshape(len(vk), 12) if (Pk.shape[-1] == 12 and Pk.ndim <= 2) else _Ps_colmajor(Pk)
        views += vk
        rows.append(Pk)
        off.append(len(views))
    flat = np.concatenate(rows) if rows and len(views) else np.zeros((0, 12))
    return off, views, flat


def _check_pose_lists(moved_offsets, moved_views, moved_Ps):
    off = np.ascontiguousarray(moved_offsets, np.int32)
    views = np.ascontiguousarray(moved_views, np.int32)
    flat = np.ascontiguousarray(moved_Ps, np.float64).reshape(-1, 12)
    if len(off) < 1 or int(off[-1]) != len(views) or len(flat) != len(views):
        raise ValueError("moved_offsets / moved_views / moved_Ps disagree")
    return off, views, flat


def _ptr(a, null=None):
    """The address of an optional array for a C call: `null` (None) for no array and for an empty one."""
    return C.c_void_p(a.ctypes.data) if (a is not None and a.size) else null


def _idx4_list(idx4):
    idx = np.ascontiguousarray(idx4, np.int32)
    if idx.size % 4 or (idx.ndim == 2 and idx.shape[1] != 4) or idx.ndim > 2:
        raise ValueError("idx4 must hold (P0, P1, D0, D1) tuples")
    return idx.reshape(-1, 4)


def _transforms_colmajor(Ts):
    """Anything np.asarray turns into (K, 4, 4) or (4, 4) -> (K, 16) float64, column-major per transform."""
    T = np.asarray(Ts, dtype=np.float64)
    if T.ndim == 2 and T.shape == (4, 4):
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError("Ts must be (K, 4, 4)")
    return np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)


def _with_pairs(results, pairs, want_pairs):
    return results + (pairs,) if want_pairs else results


def _pose_lists_call(fn, handle, moved_offsets, moved_views, moved_Ps, extra, n_results):
    """fn(handle, K, offsets, views, matrices, *extra, results...) over checked pose lists -> the n_results float64 arrays of K."""
    off, views, flat = _check_pose_lists(moved_offsets, moved_views, moved_Ps)
    results = tuple(np.zeros(len(off) - 1, np.float64) for _ in range(n_results))
    check(fn(handle, len(off) - 1, C.c_void_p(off.ctypes.data), _ptr(views), _ptr(flat), *extra,
             *[C.c_void_p(r.ctypes.data) for r in results]))
    return results


def _n_all_pairs(Ps):
    n = 0 if Ps is None else len(Ps)  # (no matrices: the library reports it)
    return n * (n - 1) // 2


def _scalar_form_call(fn, handle, lead, extra, n_scalars, n_rows, n_columns, want_pairs, mid=(), planes=()):
    """fn(handle, *lead, *extra, *mid, scalar results..., pairs) -> the n_scalars floats, then `planes` -- with want_pairs also pairs,
    (n_rows, n_columns) float32.  lead: () for all pairs, (the index list's address, its length) for a list; mid: what a map call
    passes between the scalars going in and those coming out."""
    scalars = [C.c_double(0.0) for _ in range(n_scalars)]
    pairs = np.zeros((n_rows, n_columns), np.float32) if want_pairs else None
    check(fn(handle, *lead, *extra, *mid, *[C.byref(s) for s in scalars], _ptr(pairs)))
    return _with_pairs(tuple(s.value for s in scalars) + tuple(planes), pairs, want_pairs)


def _map_form_call(fn, metric, lead, extra, views, k, n_scalars, n_rows, n_columns, want_pairs):
    """_scalar_form_call with the views to map (an int32 array, None: all) and their k HITS and k REJ planes; the metric remembers k
    for its *_map_weights once the call has succeeded.  Returns (scalars..., hits, rejected[, pairs])."""
    hits, rejected = metric._robust_map_planes(k)
    out = _scalar_form_call(fn, metric._h, lead, extra, n_scalars, n_rows, n_columns, want_pairs,
                            (_ptr(views), 0 if views is None else len(views), _ptr(hits), _ptr(rejected)), (hits, rejected))
    metric._robust_map_count = k
    return out


def _map_weights_call(fn, metric, *rule):
    """fn(handle, *rule, handles) for the map the metric holds -> one RadonIntermediate per mapped view.  rule: the floats of the
    feedback rule, (min_hits, gain) for the two weights calls, (floor, min_hits, gain, max_factor) for the variances call."""
    k = getattr(metric, "_robust_map_count", 0)
    hs = (C.c_void_p * max(k, 1))()
    check(fn(metric._h, *[float(x) for x in rule], hs))
    return [RadonIntermediate(metric.ctx, C.c_void_p(h)) for h in hs[:k]]


_NULL = C.c_void_p(0)  # what the transforms calls pass for an empty array (the other families: None)


def _transforms_call(fn, handle, n, n_source, flat, extra, n_results, n_columns, want_pairs):
    """fn(handle, n_source, K, transforms, *extra, results..., pairs) over the (K, 16) rows of _transforms_colmajor on a metric of n
    views -> the n_results float64 arrays of K -- with want_pairs also pairs, (K, n_target, n_source, n_columns) float32 (n_columns
    None: no trailing axis)."""
    n_source, K = int(n_source), len(flat)
    results = tuple(np.zeros(K, np.float64) for _ in range(n_results))
    shape = (K, max(n - n_source, 0), max(n_source, 0)) + (() if n_columns is None else (n_columns,))
    pairs = np.zeros(shape, np.float32) if want_pairs else None
    check(fn(handle, n_source, K, _ptr(flat, _NULL), *extra, *[_ptr(r, _NULL) for r in results], _ptr(pairs)))
    return _with_pairs(results, pairs, want_pairs)


def _last_count(fn, handle, ctype=C.c_int64):
    """fn(handle, &v) of the last_* getters -> v."""
    v = ctype(0)
    check(fn(handle, C.byref(v)))
    return v.value


class MetricRadonIntermediate:
    """ref: class MetricRadonIntermediate : public Metric."""

    def __init__(self, ctx, Ps=None, dtrs=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        self._dtrs = []
        self._Ps = None
        self._params = [0.0, 0.0, 0]
        d = type(self).default_sampling
        self._sampling = 0 if d is None else (self._SAMPLING[d] if isinstance(d, str) else int(d))
        self._incremental = False
        self._record_reuse = None  # library default (on unless ECC_RECORD_REUSE=0)
        self._small_eval = None    # library default (on)
        self._host_join = None     # library default (on)
        self._debug = {}         # ecc_debug_* settings of this object (experiments), re-applied to a new handle
        # the optimiser loop's two calls, setProjectionMatrices + evaluate(): data pointers of the caller's (n, 12) arrays by
        # array object (ndarray.ctypes costs 1.2 us per call; the arrays are kept alive here, at most 1024 of them), and the
        # result cell of evaluate()
        self._ptr_cache = {}
        self._mean = C.c_double()
        self._mean_ref = C.byref(self._mean)
        if dtrs is not None:
            self.setRadonIntermediates(dtrs)
        if Ps is not None:
            self.setProjectionMatrices(Ps)

    def setRadonIntermediates(self, dtrs):
        if self._h:
            _lib.lib().ecc_metric_destroy(self._h)
            self._h = C.c_void_p()
        self._dtrs = list(dtrs)  # borrowed, kept alive here
        hs = (C.c_void_p * len(self._dtrs))(*[d._h for d in self._dtrs])
        check(_lib.lib().ecc_metric_create(self.ctx._h, len(self._dtrs), hs, C.byref(self._h)))
        check(_lib.lib().ecc_metric_set_params(self._h, *self._params))
        check(_lib.lib().ecc_metric_set_sampling(self._h, self._sampling))
        check(_lib.lib().ecc_metric_set_incremental(self._h, int(self._incremental)))
        if self._record_reuse is not None:
            check(_lib.lib().ecc_metric_set_record_reuse(self._h, int(self._record_reuse)))
        if self._small_eval is not None:
            check(_lib.lib().ecc_metric_set_small_eval(self._h, int(self._small_eval)))
        if self._host_join is not None:
            check(_lib.lib().ecc_metric_set_host_join(self._h, int(self._host_join)))
        self._apply_debug()
        if self._Ps is not None:
            self.setProjectionMatrices(self._Ps)
        return self

    def _apply_debug(self):
        if "poly_tolerance" in self._debug:
            check(_lib.lib().ecc_debug_set_poly_tolerance(self._h, float(self._debug["poly_tolerance"])))
        if "small_eval_bound" in self._debug:
            check(_lib.lib().ecc_debug_set_small_eval_bound(self._h, int(self._debug["small_eval_bound"])))
        if "gradient_launch" in self._debug:
            check(_lib.lib().ecc_debug_set_gradient_launch(self._h, int(self._debug["gradient_launch"])))

    def debugSetGradientLaunch(self, on=True):
        """ecc_debug_set_gradient_launch (experiments; off by default): on = evaluate_gradient takes the probes' own launch
        (path 2, small_poses_kernel) where it applies; off = the pose batch (path 1).  Same bits."""
        self._debug["gradient_launch"] = 1 if on else 0
        if self._h:
            self._apply_debug()
        return self

    def debugSetPolyTolerance(self, tol_bins):
        """ecc_debug_set_poly_tolerance (experiments): economisation bound of the polynomial path in Radon bins."""
        self._debug["poly_tolerance"] = float(tol_bins)
        if self._h:
            self._apply_debug()
        return self

    def debugSetSmallEvalBound(self, max_pairs):
        """ecc_debug_set_small_eval_bound (experiments): size bound of the one-launch path, -1 = default."""
        self._debug["small_eval_bound"] = int(max_pairs)
        if self._h:
            self._apply_debug()
        return self

    def getRadonIntermediates(self):
        return self._dtrs

    def refreshRadonIntermediates(self, first=0, count=None):
        """Not in the reference (ecc_metric_refresh_dtrs): the metric samples private row-paired copies of its dtrs;
        after the slabs behind dtrs [first, first+count) were recomputed in place, re-copy them (asynchronous)."""
        count = len(self._dtrs) - first if count is None else count
        check(_lib.lib().ecc_metric_refresh_dtrs(self._h, int(first), int(count)))
        return self

    def setProjectionMatrices(self, Ps):
        """Ps: list of 3x4 matrices, or (fast path) an (n, 12) float64 C-contiguous array that is
        already column-major per view (what Eigen's Ps[i].data() holds)."""
        hit = self._ptr_cache.get(id(Ps))
        if hit is not None and hit[0] is Ps and hit[2] == Ps.shape:  # this very array object has passed the checks below
            self._Ps = Ps
            if self._h:
                check(_lib.lib().ecc_metric_set_projections(self._h, hit[1], hit[2][0]))
            return self
        if isinstance(Ps, np.ndarray) and Ps.ndim == 2 and Ps.shape[1] == 12 and Ps.dtype == np.float64 \
                and Ps.flags["C_CONTIGUOUS"]:
            self._Ps = Ps
            if len(self._ptr_cache) >= 1024:
                self._ptr_cache.clear()
            self._ptr_cache[id(Ps)] = (Ps, C.c_void_p(Ps.ctypes.data), Ps.shape)  # (an ndarray's buffer does not move while it is referenced)
        else:
            self._Ps = _Ps_colmajor(Ps)
        if self._h:
            check(_lib.lib().ecc_metric_set_projections(self._h, C.c_void_p(self._Ps.ctypes.data), len(self._Ps)))
        return self

    def getProjectionMatrices(self):
        return [] if self._Ps is None else [p.reshape(4, 3).T.copy() for p in self._Ps]

    def getNumberOfProjetions(self):  # sic, ref: ...RadonIntermediate.h:64
        return 0 if self._Ps is None else len(self._Ps)

    def _push_params(self):
        if self._h:
            check(_lib.lib().ecc_metric_set_params(self._h, *self._params))

    def setObjectRadius(self, radius_mm=0.0):
        self._params[0] = float(radius_mm)
        self._push_params()
        return self

    def getObjectRadius(self):
        r = C.c_double()
        check(_lib.lib().ecc_metric_get_object_radius(self._h, C.byref(r)))
        return r.value

    def setEpipolarPlaneStep(self, dkappa_rad=0.0):
        self._params[1] = float(dkappa_rad)
        self._push_params()
        return self

    setdKappa = setEpipolarPlaneStep

    def useCorrelation(self, corr=True):
        self._params[2] = 1 if corr else 0
        self._push_params()
        return self

    # class-wide default for new objects: None = the library's default (ECC_SAMPLING_AUTO)
    default_sampling = None
    _SAMPLING = {"auto": 0, "polynomial": 1, "per_sample": 2, "reference": 3}

    def setSampling(self, mode="auto"):
        """Not in the reference (ecc_metric_set_sampling): "auto" (reference arithmetic for evaluations of at most
        512 pairs, fitted polynomials above), "polynomial", "per_sample" or "reference"."""
        self._sampling = self._SAMPLING[mode] if isinstance(mode, str) else int(mode)
        if self._h:
            check(_lib.lib().ecc_metric_set_sampling(self._h, self._sampling))
        return self

    def setIncremental(self, enable=True):
        """Not in the reference (ecc_metric_set_incremental): keep the pair values of the last all-pairs / range
        evaluation on the device and re-evaluate only the pairs of views whose matrix changed since -- the optimiser
        pattern of Gui/SingleImageMotion.h (one view moves per call).  Results are bit-identical to full evaluations."""
        self._incremental = bool(enable)
        if self._h:
            check(_lib.lib().ecc_metric_set_incremental(self._h, int(self._incremental)))
        return self

    def setRecordReuse(self, on=True, always=False):
        """Not in the reference (ecc_metric_set_record_reuse, default on): keep the per-pair geometry records of the last
        all-pairs / range evaluation and refit only the pairs whose matrices changed; every pair is still sampled and
        results are bit-identical either way.  on=True: for ranges of more than 4096 pairs (smaller evaluations are
        faster refitting everything); always=True: for every size."""
        self._record_reuse = (2 if always else 1) if on else 0
        if self._h:
            check(_lib.lib().ecc_metric_set_record_reuse(self._h, int(self._record_reuse)))
        return self

    def setSmallEval(self, on=True):
        """ecc_metric_set_small_eval: evaluations of at most 192 pairs (ECC_SMALL_EVAL_MAX_PAIRS) as ONE launch, and E1 in
        the record kernel's arguments for launches of at most 4096 pairs (default on; bit-identical results).  Kept
        across setRadonIntermediates like the other settings."""
        self._small_eval = 1 if on else 0
        if self._h:
            check(_lib.lib().ecc_metric_set_small_eval(self._h, self._small_eval))
        return self

    def setHostJoin(self, on=True):
        """ecc_metric_set_host_join (default on): evaluate() and evaluate_range() of the two-stream record-reuse form wait on the
        host for the moved views' launches and then queue the sum, instead of ordering it with an event on the device; the same
        launches and bit-identical results either way.  Kept across setRadonIntermediates like the other settings."""
        self._host_join = 1 if on else 0
        if self._h:
            check(_lib.lib().ecc_metric_set_host_join(self._h, self._host_join))
        return self

    def device_bytes(self):
        """ecc_metric_device_bytes ->{"paired_copies", "quad_copies", "other"}: device memory this metric owns right now (the
        Radon intermediates themselves belong to their RadonIntermediate objects)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(_lib.lib().ecc_metric_device_bytes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"paired_copies": a.value, "quad_copies": b.value, "other": c.value}

    def last_evaluated_pairs(self):
        """Pairs the last evaluate() / evaluate_range() actually recomputed."""
        return _last_count(_lib.lib().ecc_metric_last_evaluated_pairs, self._h)

    # -- evaluation ----------------------------------------------------------------------------
    def evaluate(self, arg=None, out=None):
        """evaluate()                      -> mean over all pairs
        evaluate(cost)  cost: (n,n) float32 C-contiguous array, entry [j, i] (= index i + j*n), i<j, is written
        evaluate(set_of_views[, out])   -> mean over all pairs inside the subset
        evaluate(indices[, out])        -> mean over explicit (P0,P1,dtr0,dtr1) tuples
        ref: ...RadonIntermediate.cpp:166-225, :228-245, :267-322."""
        L = _lib.lib()
        if arg is None:
            check(L.ecc_metric_evaluate_all(self._h, None, self._mean_ref))
            return self._mean.value
        mean = C.c_double()
        if arg is None or (isinstance(arg, np.ndarray) and arg.dtype == np.float32 and arg.ndim == 2
                           and out is None and arg.shape[0] == arg.shape[1] == self.getNumberOfProjetions()):
            cost = arg
            if cost is not None and not cost.flags["C_CONTIGUOUS"]:
                raise ValueError("cost image must be C-contiguous float32")
            check(L.ecc_metric_evaluate_all(self._h, C.c_void_p(cost.ctypes.data if cost is not None else 0),
                                            C.byref(mean)))
            return mean.value
        if isinstance(arg, (set, frozenset)):
            views = sorted(arg)
            idx = [(a, b, a, b) for k, a in enumerate(views) for b in views[k + 1:]]
        else:
            idx = arg
        hit_i, hit_o = self._ptr_cache.get(id(idx)), self._ptr_cache.get(id(out))
        if hit_i is not None and hit_o is not None and hit_i[0] is idx and hit_o[0] is out and hit_i[2] == idx.shape \
                and hit_o[2] == out.shape:  # these very arrays have passed the checks below
            check(L.ecc_metric_evaluate_pairs(self._h, hit_i[1], hit_i[2][0], hit_o[1], self._mean_ref))
            return self._mean.value
        cacheable = isinstance(idx, np.ndarray) and idx.dtype == np.int32 and idx.ndim == 2 and idx.shape[1] == 4 \
            and idx.flags["C_CONTIGUOUS"] and isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"]
        idx0 = idx
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 4)
        if out is None:
            out = np.empty(len(idx), np.float32)
        assert out.dtype == np.float32 and out.size >= len(idx)
        pi, po = C.c_void_p(idx.ctypes.data), C.c_void_p(out.ctypes.data)
        if cacheable:  # (idx is a view of idx0 then: the same buffer)
            if len(self._ptr_cache) >= 1024:
                self._ptr_cache.clear()
            self._ptr_cache[id(idx0)] = (idx0, pi, idx0.shape)
            self._ptr_cache[id(out)] = (out, po, out.shape)
        check(L.ecc_metric_evaluate_pairs(self._h, pi, len(idx), po, C.byref(mean)))
        return mean.value

    def evaluate_poses(self, poses, first=0, stride=1):
        """ecc_metric_evaluate_poses[_strided]: independent all-pairs evaluations of several poses on this metric; poses: a
        sequence of (n, 12) column-major arrays (pack_projection_matrices) or lists of 3x4 matrices; returns the means
        (bit-identical to evaluating them one by one).  Poses that differ from the current matrices (or from the first pose)
        in a few views go through ONE batched record / pair / sum launch each (setPoseBatching(False): all of them two deep on
        the stream, as in rounds 4-5).  first / stride: only the poses first, first + stride, ... (the others' means stay 0).
        The last evaluated pose's matrices stay current."""
        if isinstance(poses, np.ndarray) and poses.ndim == 3 and poses.shape[2] == 12 and poses.dtype == np.float64 \
                and poses.flags["C_CONTIGUOUS"]:
            flat = poses  # (K, n, 12) already packed: no copy (600 poses of 400 views are 23 MB)
        else:
            flat = np.ascontiguousarray(np.stack([p if (isinstance(p, np.ndarray) and p.ndim == 2 and p.shape[1] == 12)
                                                  else _Ps_colmajor(p) for p in poses]), np.float64)
        means = np.zeros(len(flat), np.float64)
        check(_lib.lib().ecc_metric_evaluate_poses_strided(self._h, len(flat), C.c_void_p(flat.ctypes.data), flat.shape[1],
                                                           int(first), int(stride), C.c_void_p(means.ctypes.data)))
        mine = range(int(first), len(flat), int(stride))
        if len(mine):
            self._Ps = flat[mine[-1]]
        return means

    def evaluate_pose_deltas(self, moved_views, moved_Ps):
        """ecc_metric_evaluate_pose_deltas: pose k = the current matrices with the views moved_views[k] (a sequence of view
        indices, strictly ascending) replaced by moved_Ps[k] (the same number of 3x4 matrices, or (c, 12) column-major rows).
        Returns the means, every one bit-identical to setProjectionMatrices + evaluate of that pose; the current matrices stay."""
        return self.evaluate_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps))

    def evaluate_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps):
        """The C signature itself: moved_offsets (K + 1 int32, [0] = 0), moved_views (Q int32, ascending within a pose), moved_Ps
        ((Q, 12) float64, column-major per matrix).  No per-pose Python work."""
        return _pose_lists_call(_lib.lib().ecc_metric_evaluate_pose_deltas, self._h, moved_offsets, moved_views, moved_Ps, (), 1)[0]

    def evaluate_weighted_pose_deltas(self, moved_views, moved_Ps):
        """ecc_metric_evaluate_weighted_pose_deltas: evaluate_pose_deltas for the metric with per-line weights (evaluate_weighted: the
        metric holds the data of every view, then its line weights).  The same arguments; returns (values, coverages), every entry
        bit-identical to setProjectionMatrices + evaluate_weighted of that pose; the current matrices stay."""
        return self.evaluate_weighted_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps))

    def evaluate_weighted_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps):
        """The C signature itself, with the arguments of evaluate_pose_deltas_packed; returns (values, coverages)."""
        return _pose_lists_call(_lib.lib().ecc_metric_evaluate_weighted_pose_deltas, self._h, moved_offsets, moved_views, moved_Ps, (), 2)

    def evaluate_robust_pose_deltas(self, moved_views, moved_Ps, loss, delta):
        """ecc_metric_evaluate_robust_pose_deltas: evaluate_pose_deltas under the per-sample robust loss of evaluate_robust (loss,
        delta as there).  The same lists; returns (values, inlier_masses), every entry bit-identical to setProjectionMatrices +
        evaluate_robust(loss, delta) of that pose; the current matrices stay."""
        return self.evaluate_robust_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps), loss, delta)

    def evaluate_robust_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps, loss, delta):
        """The C signature itself, with the arguments of evaluate_pose_deltas_packed, then loss and delta; returns (values,
        inlier_masses)."""
        return _pose_lists_call(_lib.lib().ecc_metric_evaluate_robust_pose_deltas, self._h, moved_offsets, moved_views, moved_Ps,
                                (int(loss), float(delta)), 2)

    def evaluate_weighted_robust_pose_deltas(self, moved_views, moved_Ps, loss, delta):
        """ecc_metric_evaluate_weighted_robust_pose_deltas: evaluate_pose_deltas under line weights and the robust loss together
        (evaluate_weighted_robust: the metric holds the data of every view, then its line weights; loss, delta as there).  The same
        lists; returns (values, coverages, inlier_masses), every entry bit-identical to setProjectionMatrices +
        evaluate_weighted_robust(loss, delta) of that pose; the current matrices stay."""
        return self.evaluate_weighted_robust_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps), loss, delta)

    def evaluate_weighted_robust_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps, loss, delta):
        """The C signature itself, with the arguments of evaluate_pose_deltas_packed, then loss and delta; returns (values,
        coverages, inlier_masses)."""
        return _pose_lists_call(_lib.lib().ecc_metric_evaluate_weighted_robust_pose_deltas, self._h, moved_offsets, moved_views, moved_Ps,
                                (int(loss), float(delta)), 3)

    def evaluate_weighted_pairs(self, idx4, want_pairs=False):
        """ecc_metric_evaluate_weighted_pairs: evaluate_weighted over an index list of (P0, P1, D0, D1) tuples -- matrices P*, data
        intermediates D* in [0, n_views); the weights of a sample come from intermediate n_views + D*.  Returns (value, coverage) =
        (sum c / sum u, sum u / n_pairs) over the list -- with want_pairs (value, coverage, pairs), pairs (n_pairs, 2) float32 rows
        {c, u} in list order.  The sampling mode resolves from the list's length, as evaluate(indices) resolves it."""
        idx = _idx4_list(idx4)
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_weighted_pairs, self._h, (_ptr(idx), len(idx)), (), 2, len(idx), 2, want_pairs)

    def evaluate_variance_pairs(self, idx4, floor, want_pairs=False):
        """ecc_metric_evaluate_variance_pairs: evaluate_variance over an index list of (P0, P1, D0, D1) tuples -- matrices P*, data
        intermediates D* in [0, n_views); the variance of a sample comes from intermediate n_views + D*.  Returns (value, mean_weight)
        = (sum c / sum u, sum u / n_pairs) over the list -- with want_pairs (value, mean_weight, pairs), pairs (n_pairs, 2) float32
        rows {c, u} in list order.  The sampling mode resolves from the list's length, as evaluate(indices) resolves it."""
        idx = _idx4_list(idx4)
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_variance_pairs, self._h, (_ptr(idx), len(idx)), (float(floor),), 2, len(idx), 2,
                                 want_pairs)

    def evaluate_variance_pose_deltas(self, moved_views, moved_Ps, floor):
        """ecc_metric_evaluate_variance_pose_deltas: evaluate_pose_deltas for the metric with inverse-variance sample weights
        (evaluate_variance: the metric holds the data of every view, then its variance field; floor as there).  The same lists;
        returns (values, mean_weights), every entry bit-identical to setProjectionMatrices + evaluate_variance(floor) of that pose;
        the current matrices stay."""
        return self.evaluate_variance_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps), floor)

    def evaluate_variance_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps, floor):
        """The C signature itself, with the arguments of evaluate_pose_deltas_packed, then the floor; returns (values,
        mean_weights)."""
        return _pose_lists_call(_lib.lib().ecc_metric_evaluate_variance_pose_deltas, self._h, moved_offsets, moved_views, moved_Ps,
                                (float(floor),), 2)

    def evaluate_variance_robust_pairs(self, idx4, loss, delta, floor, want_pairs=False):
        """ecc_metric_evaluate_variance_robust_pairs: evaluate_variance_robust over an index list of (P0, P1, D0, D1) tuples as
        evaluate_variance_pairs takes them: D0, D1 index the data intermediates, in [0, n_views), and the variance follows the data
        index.  Returns (value, mean_weight, inlier_mass) over the list -- with want_pairs also pairs (n_pairs, 4) float32 rows
        {c, u, k, r} in list order.  The sampling mode resolves from the list's length; an empty list writes nothing
        (0.0, 0.0, 0.0)."""
        idx = _idx4_list(idx4)
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_variance_robust_pairs, self._h, (_ptr(idx), len(idx)),
                                 (int(loss), float(delta), float(floor)), 3, len(idx), 4, want_pairs)

    def evaluate_variance_robust_pose_deltas(self, moved_views, moved_Ps, loss, delta, floor):
        """ecc_metric_evaluate_variance_robust_pose_deltas: evaluate_pose_deltas under inverse-variance weights and the robust loss
        of the studentised residual (evaluate_variance_robust: the metric holds the data of every view, then its variance field;
        loss, delta, floor as there).  The same lists; returns (values, mean_weights, inlier_masses), every entry bit-identical to
        setProjectionMatrices + evaluate_variance_robust(loss, delta, floor) of that pose; the current matrices stay."""
        return self.evaluate_variance_robust_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps), loss, delta, floor)

    def evaluate_variance_robust_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps, loss, delta, floor):
        """The C signature itself, with the arguments of evaluate_pose_deltas_packed, then loss, delta and the floor; returns
        (values, mean_weights, inlier_masses)."""
        return _pose_lists_call(_lib.lib().ecc_metric_evaluate_variance_robust_pose_deltas, self._h, moved_offsets, moved_views, moved_Ps,
                                (int(loss), float(delta), float(floor)), 3)

    def setPoseBatching(self, on=True):
        """ecc_metric_set_pose_batching: off = evaluate_poses runs every pose as its own stream-ordered evaluation."""
        check(_lib.lib().ecc_metric_set_pose_batching(self._h, 1 if on else 0))
        return self

    def last_batched_poses(self):
        return _last_count(_lib.lib().ecc_metric_last_batched_poses, self._h)

    def setFormIncremental(self, enable=True):
        """Not in the reference (ecc_metric_set_form_incremental, default off): the evaluate_{weighted, robust, weighted_robust,
        variance, variance_robust}_pose_deltas calls keep their base columns on the device between calls and re-evaluate only the
        pairs of views whose matrix changed since -- the optimiser pattern (set one view, probe).  Every result keeps the bits of
        the call with the mode off; any change of the setting drops what is kept."""
        check(_lib.lib().ecc_metric_set_form_incremental(self._h, 1 if enable else 0))
        return self

    def last_form_base_pairs(self):
        """ecc_metric_last_form_base_pairs: base pairs the last such call evaluated -- n (n - 1) / 2 with the mode off or on a miss,
        the pairs of the c refreshed views, 0 on a hit or with pose batching off."""
        return _last_count(_lib.lib().ecc_metric_last_form_base_pairs, self._h)

    def evaluate_gradient(self, view, Ps_plus, Ps_minus, h, want_probes=False):
        """ecc_metric_evaluate_gradient: the metric at the current matrices and its central-difference gradient over p pose
        parameters of one view.  Ps_plus / Ps_minus: the view's 3x4 matrix at x + h[k] e_k and at x - h[k] e_k, p matrices each
        (or (p, 12) column-major rows); h: the p step lengths (finite, not zero).  Returns (value, grad) -- with want_probes
        (value, grad, probes), probes = the 2 p means plus_0, minus_0, plus_1, ...: every probe has the bits of
        evaluate_pose_deltas / setProjectionMatrices + evaluate on its matrices, value those of evaluate(), and
        grad[k] = (probes[2k] - probes[2k + 1]) / (2.0 * h[k]).  The current matrices stay.  last_gradient_path() says which
        launches the call took."""
        def rows(Ps):
            Ps = np.asarray(Ps, np.float64)
            return np.ascontiguousarray(Ps.reshape(-1, 12) if (Ps.shape[-1] == 12 and Ps.ndim <= 2) else _Ps_colmajor(Ps))
        plus, minus = rows(Ps_plus), rows(Ps_minus)
        h = np.ascontiguousarray(np.atleast_1d(h), np.float64)
        p = len(h)
        if p < 1 or len(plus) != p or len(minus) != p:
            raise ValueError("Ps_plus / Ps_minus / h disagree")
        value = C.c_double(0.0)
        grad, probes = np.zeros(p, np.float64), np.zeros(2 * p, np.float64)
        check(_lib.lib().ecc_metric_evaluate_gradient(self._h, int(view), p, C.c_void_p(plus.ctypes.data), C.c_void_p(minus.ctypes.data),
                                                      C.c_void_p(h.ctypes.data), C.byref(value), C.c_void_p(grad.ctypes.data),
                                                      C.c_void_p(probes.ctypes.data) if want_probes else None))
        return (value.value, grad, probes) if want_probes else (value.value, grad)

    def evaluate_gradient_rigid(self, view, steps, want_probes=False):
        """evaluate_gradient over the six parameters (tx, ty, tz, rx, ry, rz) of geometry.rigid_transform for one view: probe
        +-k is geometry.compose_transform(P_view, rigid_transform(+-steps[k] e_k)); steps: six step lengths (mm, mm, mm, rad,
        rad, rad)."""
        from .geometry import compose_transform, rigid_transform
        steps = np.asarray(steps, np.float64)
        if steps.shape != (6,):
            raise ValueError("steps: (tx, ty, tz, rx, ry, rz)")
        if self._Ps is None or not 0 <= int(view) < len(self._Ps):
            raise ValueError("view outside the projection matrices")
        P = self._Ps[int(view)].reshape(4, 3).T
        names = ("tx", "ty", "tz", "rx", "ry", "rz")
        plus = [compose_transform(P, rigid_transform(**{names[k]: steps[k]})) for k in range(6)]
        minus = [compose_transform(P, rigid_transform(**{names[k]: -steps[k]})) for k in range(6)]
        return self.evaluate_gradient(view, plus, minus, steps, want_probes)

    def last_gradient_path(self):
        """ecc_metric_last_gradient_path: 1 = the pose batch (evaluate_pose_deltas; the default), 0 = every probe sequentially
        (setPoseBatching(False)), 2 = the probes' records and sampling as one launch (debugSetGradientLaunch(True))."""
        return _last_count(_lib.lib().ecc_metric_last_gradient_path, self._h, C.c_int)

    def evaluate_gram(self, n_channels, want_pairs=False):
        """ecc_metric_evaluate_gram: the metric as a quadratic form of the coefficients of n_channels fixed channel images per view
        (corrected image of view i = sum_c a_c I_c,i).  The metric holds n_channels * n_views Radon intermediates, channel-major
        (channel c of view i is dtr c * n_views + i), computed with POST_IDENTITY.  Returns G, (K, K) float64 and symmetric, with
        metric(a) = gram_value(G, a) -- with want_pairs (G, pairs), pairs (n_pairs, K (K + 1) / 2) float32 in the pair order of
        evaluate(cost) and the entry order (0,0), (0,1) .. (K-1,K-1).  Diagonal entries have the bits of evaluate(cost) on a metric
        of that channel's intermediates alone.  The current matrices and everything the metric keeps stay."""
        K = int(n_channels)
        n = 0 if self._Ps is None else len(self._Ps)  # (no matrices: the library reports it)
        G = np.zeros((max(K, 0), max(K, 0)), np.float64)
        pairs = np.zeros((n * (n - 1) // 2, max(K, 0) * (max(K, 0) + 1) // 2), np.float32) if want_pairs else None
        check(_lib.lib().ecc_metric_evaluate_gram(self._h, K, _ptr(pairs),
                                                  C.c_void_p(G.ctypes.data) if G.size else None))
        return (G, pairs) if want_pairs else G

    def evaluate_view_coefficients(self, coeffs, want_pairs=False):
        """ecc_metric_evaluate_view_coefficients: the metric at per-view channel coefficients and its gradient.  coeffs: (K, n) --
        a[c, i] multiplies channel c of view i; the metric holds K * n Radon intermediates, channel-major, computed with
        POST_IDENTITY, as for evaluate_gram; the coefficients are passed as float32.  Returns (value, grad), grad (K, n) float64 =
        d value / d a -- with want_pairs (value, grad, pairs), pairs (n_pairs, 1 + 2 K) float32 in the pair order of evaluate(cost):
        per pair i < j its value, then h0[c] = 1/2 d (pair value) / d a[c, i] and h1[c] = 1/2 d (pair value) / d a[c, j].  The metric
        is a quadratic form of a, so grad is linear in a and the same call at a direction v returns the Hessian-vector product
        (minimize_view_coefficients).  The current matrices and everything the metric keeps stay."""
        a = np.ascontiguousarray(coeffs, np.float32)
        if a.ndim != 2:
            raise ValueError("coeffs must be (n_channels, n_views)")
        K, n = a.shape
        if self._Ps is not None and n != len(self._Ps):
            raise ValueError("coeffs must be (n_channels, n_views)")
        value = C.c_double(0.0)
        grad = np.zeros((K, n), np.float64)
        pairs = np.zeros((n * (n - 1) // 2, 1 + 2 * K), np.float32) if want_pairs else None
        check(_lib.lib().ecc_metric_evaluate_view_coefficients(self._h, K, C.c_void_p(a.ctypes.data) if a.size else None, C.byref(value),
                                                               C.c_void_p(grad.ctypes.data) if grad.size else None,
                                                               _ptr(pairs)))
        return (value.value, grad, pairs) if want_pairs else (value.value, grad)

    def evaluate_view_hessian(self, n_channels, want_pairs=False, want_matrix=True):
        """ecc_metric_evaluate_view_hessian: the quadratic form of per-view channel coefficients as a matrix.  The metric holds
        n_channels * n_views Radon intermediates as for evaluate_view_coefficients.  Returns H, (n K, n K) float64 and symmetric bit
        for bit, with the index c * n + i of coeffs.reshape(-1): metric(a) = view_hessian_value(H, a), gradient 2 H a -- with
        want_pairs (H, blocks), blocks (n_pairs, K (K + 1) + K^2) float64 in the pair order of evaluate(cost): per pair i < j the upper
        triangle of P00 (view i with itself) in evaluate_gram's entry order, the upper triangle of P11 (view j with itself), then P01
        row-major, pair value = a_i^T P00 a_i + a_j^T P11 a_j + 2 a_i^T P01 a_j.  want_matrix=False (with want_pairs): the blocks alone
        -- H is neither assembled nor copied, and n K may exceed ECC_VIEW_HESSIAN_MAX_DIM.  Every product of two samples is formed
        exactly in float64, so the form keeps its digits where it is a small difference of large moments.  The current matrices and
        everything the metric keeps stay."""
        if not want_pairs and not want_matrix:
            raise ValueError("nothing asked for: want_matrix or want_pairs")
        K = int(n_channels)
        n = 0 if self._Ps is None else len(self._Ps)  # (no matrices: the library reports it)
        Kp = max(K, 0)
        H = np.zeros((n * Kp, n * Kp) if n * Kp else (1, 1), np.float64) if want_matrix else None  # (never a null where one was asked for)
        blocks = None
        if want_pairs:
            blocks = np.zeros((n * (n - 1) // 2, Kp * (Kp + 1) + Kp * Kp) if n > 1 and Kp else (1, 1), np.float64)
        check(_lib.lib().ecc_metric_evaluate_view_hessian(self._h, K, C.c_void_p(H.ctypes.data) if want_matrix else None,
                                                          C.c_void_p(blocks.ctypes.data) if want_pairs else None))
        return (H, blocks) if (want_pairs and want_matrix) else (H if want_matrix else blocks)

    def evaluate_weighted(self, want_pairs=False):
        """ecc_metric_evaluate_weighted: the metric with per-line weights in Radon space.  The metric holds 2 * n_views Radon
        intermediates, channel-major: the data of every view, then the line weights of every view on the same bin grid (line_weights;
        FILTER_NONE, values in [0, 1]).  Per +-kappa sample of the pair i < j the squared difference of evaluate() counts with
        mu = W_i(sample) * W_j(sample).  Returns (value, coverage): value = sum c / sum u over the pairs, coverage = sum u / n_pairs --
        with want_pairs (value, coverage, pairs), pairs (n_pairs, 2) float32 in the pair order of evaluate(cost): per pair c, its
        weighted value, and u = (sum mu) / (number of samples), its coverage.  All weights 1: the bits of evaluate() and coverage 1.
        The current matrices and everything the metric keeps stay."""
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_weighted, self._h, (), (), 2, _n_all_pairs(self._Ps), 2, want_pairs)

    def evaluate_variance(self, floor, want_pairs=False):
        """ecc_metric_evaluate_variance: the metric with inverse-variance sample weights.  The metric holds 2 * n_views Radon
        intermediates, channel-major: the data of every view, then the variance field V of every view on the same bin grid
        (variance_intermediates; FILTER_NONE).  Per +-kappa sample of the pair i < j the squared difference of evaluate() counts with
        omega = 1 / max(V_i(sample) + V_j(sample), floor), floor > 0 in the units of V (variance_floor proposes one).  Returns (value,
        mean_weight): value = sum c / sum u over the pairs, mean_weight = sum u / n_pairs -- with want_pairs (value, mean_weight,
        pairs), pairs (n_pairs, 2) float32 in the pair order of evaluate(cost): per pair c, its weighted value, and u = (sum omega) /
        (number of samples), its mean weight.  V == 0.5 with floor <= 1: the bits of evaluate() and mean weight 1; a common factor on
        all V and the floor leaves value as it is.  The current matrices and everything the metric keeps stay."""
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_variance, self._h, (), (float(floor),), 2, _n_all_pairs(self._Ps), 2, want_pairs)

    def evaluate_robust(self, loss, delta, want_pairs=False):
        """ecc_metric_evaluate_robust: the metric under a per-sample robust loss rho(d) = w(d) d^2 -- loss one of LOSS_HUBER,
        LOSS_TRUNCATED, LOSS_GEMAN_MCCLURE, delta > 0 its scale in the units of the data (float32; inf down-weights nothing and
        gives the bits of evaluate()).  For data in which nobody has said which lines are bad.  Returns (value, inlier_mass): value =
        sum c / n_pairs, inlier_mass = sum u / n_pairs -- with want_pairs (value, inlier_mass, pairs), pairs (n_pairs, 3) float32 in
        the pair order of evaluate(cost): per pair c, its value, u, the mean IRLS weight of its samples in (0, 1], and r, their mean
        squared raw residual (robust_scale takes delta from it).  The current matrices and everything the metric keeps stay."""
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_robust, self._h, (), (int(loss), float(delta)), 2, _n_all_pairs(self._Ps), 3,
                                 want_pairs)

    def evaluate_robust_pairs(self, idx4, loss, delta, want_pairs=False):
        """ecc_metric_evaluate_robust_pairs: evaluate_robust over an index list of (P0, P1, D0, D1) tuples, as evaluate(indices)
        takes them.  Returns (value, inlier_mass) over the list -- with want_pairs (value, inlier_mass, pairs), pairs (n_pairs, 3)
        float32 rows {c, u, r} in list order.  The sampling mode resolves from the list's length; an empty list writes nothing
        (0.0, 0.0)."""
        idx = _idx4_list(idx4)
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_robust_pairs, self._h, (_ptr(idx), len(idx)), (int(loss), float(delta)), 2,
                                 len(idx), 3, want_pairs)

    def _robust_map_views(self, views):
        """(the int32 list or None, how many planes a map call returns)"""
        if views is None:
            return None, len(self._dtrs)
        v = np.ascontiguousarray(views, np.int32).reshape(-1)
        if len(v) == 0:
            raise ValueError("views: None for every view, or at least one index")
        return v, len(v)

    def _robust_map_planes(self, k):
        n_alpha, n_t = (self._dtrs[0].getRadonBinNumber(0), self._dtrs[0].getRadonBinNumber(1)) if self._dtrs else (0, 0)
        return np.zeros((k, n_t, n_alpha), np.float32), np.zeros((k, n_t, n_alpha), np.float32)

    def evaluate_robust_map(self, loss, delta, views=None, want_pairs=False):
        """ecc_metric_evaluate_robust_map: evaluate_robust(loss, delta) -- the same bits in value, inlier_mass and pairs -- and WHERE
        the loss rejected: per mapped view a HITS plane (the bilinear footprints of every sample taken in that view) and a REJ plane
        (the same footprints times 1 - w, the sample's distrust).  views: indices of the views to map (distinct), None: every view in
        order.  Returns (value, inlier_mass, hits, rejected[, pairs]); hits, rejected: (len(views), n_t, n_alpha) float32.  The sums
        are fixed point on the device: the same call gives the same bits.  REJ / HITS is the mean distrust of a line;
        robust_map_weights turns the held map into line weights.  delta = inf: rejected is all zeros."""
        v, k = self._robust_map_views(views)
        if views is None:
            k = 0 if self._Ps is None else len(self._Ps)
        return _map_form_call(_lib.lib().ecc_metric_evaluate_robust_map, self, (), (int(loss), float(delta)), v, k, 2,
                              _n_all_pairs(self._Ps), 3, want_pairs)

    def evaluate_robust_map_pairs(self, idx4, loss, delta, views=None, want_pairs=False):
        """ecc_metric_evaluate_robust_map_pairs: evaluate_robust_map over an index list of (P0, P1, D0, D1) tuples; the view of a
        sample is the tuple's data index, views (None: every intermediate of the metric) index the intermediates.  A pair listed
        twice deposits twice; the planes do not depend on the order of the list."""
        idx = _idx4_list(idx4)
        v, k = self._robust_map_views(views)
        return _map_form_call(_lib.lib().ecc_metric_evaluate_robust_map_pairs, self, (_ptr(idx), len(idx)), (int(loss), float(delta)), v, k, 2,
                              len(idx), 3, want_pairs)

    def robust_map_weights(self, min_hits=1.0, gain=1.0):
        """ecc_metric_robust_map_weights: the map the last evaluate_robust_map[_pairs] call left on the device as line weights, a list of
        RadonIntermediate (FILTER_NONE, values in [0, 1]), one per mapped view in the order of `views`: the second half of a 2 n
        metric for evaluate_weighted / evaluate_weighted_robust.  Per bin with the float32 plane values h and r: 1 where h < min_hits,
        else float32(max(0, 1 - gain * r / h)) in float64.  Raises if no map is held (refresh_dtrs and set_params drop it)."""
        return _map_weights_call(_lib.lib().ecc_metric_robust_map_weights, self, min_hits, gain)

    def robust_map_fixed(self):
        """ecc_debug_robust_map_fixed: the held map's fixed-point sums (quantum 2^-32) folded to bins, (hits, rejected) of
        (n_mapped, n_t, n_alpha) uint64 -- integers, so that maps of disjoint lists add exactly."""
        k = getattr(self, "_robust_map_count", 0)
        n_alpha, n_t = self._dtrs[0].getRadonBinNumber(0), self._dtrs[0].getRadonBinNumber(1)
        pitch = slab_floats(n_alpha, n_t) // (n_alpha + 2)
        raw = np.zeros((2 * max(k, 1), n_alpha + 2, pitch), np.uint64)
        check(_lib.lib().ecc_debug_robust_map_fixed(self._h, _ptr(raw), raw.size))
        q = raw[:, :, :n_t + 2].copy()
        q[:, 1] += q[:, 0]
        q[:, -2] += q[:, -1]
        q[:, :, 1] += q[:, :, 0]
        q[:, :, -2] += q[:, :, -1]
        bins = np.ascontiguousarray(q[:2 * k, 1:-1, 1:-1].transpose(0, 2, 1))
        return bins[:k], bins[k:]

    def _weighted_map_views(self, views):
        """(the int32 list or None, how many planes a weighted map call returns): None maps the n_views data intermediates"""
        if views is None:
            return None, len(self._dtrs) // 2
        return self._robust_map_views(views)

    def evaluate_weighted_robust_map(self, loss, delta, views=None, want_pairs=False):
        """ecc_metric_evaluate_weighted_robust_map: evaluate_weighted_robust(loss, delta) on a 2 * n_views metric -- the same bits in
        value, coverage, inlier_mass and pairs -- and WHERE the loss rejected under the metric's line weights: per mapped view a
        HITS plane, the bilinear footprints of every sample taken in that view times the sample's weight product mu = W_i W_j, and a
        REJ plane, the same times 1 - w.  REJ / HITS is the rejected share among the lines the weights trust.  views: data indices
        in [0, n_views) (distinct), None: every view in order.  Returns (value, coverage, inlier_mass, hits, rejected[, pairs]);
        hits, rejected: (len(views), n_t, n_alpha) float32, pairs (n_pairs, 4) rows {c, u, k, r}.  Fixed-point sums on the device:
        the same call gives the same bits.  weighted_robust_map_weights multiplies the held map's factor into the weights it was
        made under.  Weights outside [0, 1]: value, coverage, inlier_mass and pairs as evaluate_weighted_robust, planes unspecified."""
        v, k = self._weighted_map_views(views)
        return _map_form_call(_lib.lib().ecc_metric_evaluate_weighted_robust_map, self, (), (int(loss), float(delta)), v, k, 3,
                              _n_all_pairs(self._Ps), 4, want_pairs)

    def evaluate_weighted_robust_map_pairs(self, idx4, loss, delta, views=None, want_pairs=False):
        """ecc_metric_evaluate_weighted_robust_map_pairs: evaluate_weighted_robust_map over an index list of (P0, P1, D0, D1) tuples
        as evaluate_weighted_robust_pairs takes them: D0, D1 and `views` index the data intermediates, in [0, n_views); weight and
        map follow the data index.  A pair listed twice deposits twice; the planes do not depend on the order of the list."""
        idx = _idx4_list(idx4)
        v, k = self._weighted_map_views(views)
        return _map_form_call(_lib.lib().ecc_metric_evaluate_weighted_robust_map_pairs, self, (_ptr(idx), len(idx)), (int(loss), float(delta)),
                              v, k, 3, len(idx), 4, want_pairs)

    def weighted_robust_map_weights(self, min_hits=1.0, gain=1.0):
        """ecc_metric_weighted_robust_map_weights: the next pass's line weights from the map the last
        evaluate_weighted_robust_map[_pairs] call left on the device -- a list of RadonIntermediate (FILTER_NONE), one per mapped
        view in the order of `views`: W_v * factor in float32, W_v the metric's current weights of that view and factor
        robust_map_weights' rule on the held planes (1 where h < min_hits, else float32(max(0, 1 - gain * r / h)) in float64).
        Raises if no map is held or the held map is evaluate_robust_map's."""
        return _map_weights_call(_lib.lib().ecc_metric_weighted_robust_map_weights, self, min_hits, gain)

    def evaluate_weighted_robust(self, loss, delta, want_pairs=False):
        """ecc_metric_evaluate_weighted_robust: line weights and the robust loss together, for scans that have both kinds of bad
        data -- lines somebody flagged (line_weights) and an instrument nobody did.  The metric holds 2 * n_views Radon
        intermediates as for evaluate_weighted; loss and delta as for evaluate_robust.  Per sample f = mu * w(d): mu the product of
        the two line weights, w the IRLS weight of the raw residual d.  Returns (value, coverage, inlier_mass): value = sum c /
        sum u (normalised by the coverage, never by the mass the loss keeps), coverage = sum u / n_pairs, inlier_mass = sum k / sum u
        -- with want_pairs (value, coverage, inlier_mass, pairs), pairs (n_pairs, 4) float32 in the pair order of evaluate(cost):
        per pair c, its value, u, its coverage, k, the weight mass the loss keeps, and r, the weighted mean squared raw residual
        (weighted_robust_scale takes delta from r / u).  delta = inf: the bits of evaluate_weighted; all weights 1: the bits of
        evaluate_robust.  The current matrices and everything the metric keeps stay."""
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_weighted_robust, self._h, (), (int(loss), float(delta)), 3,
                                 _n_all_pairs(self._Ps), 4, want_pairs)

    def evaluate_weighted_robust_pairs(self, idx4, loss, delta, want_pairs=False):
        """ecc_metric_evaluate_weighted_robust_pairs: evaluate_weighted_robust over an index list of (P0, P1, D0, D1) tuples as
        evaluate_weighted_pairs takes them: D0, D1 index the data intermediates, in [0, n_views), and the weight follows the data
        index.  Returns (value, coverage, inlier_mass) over the list -- with want_pairs also pairs (n_pairs, 4) float32 rows
        {c, u, k, r} in list order.  The sampling mode resolves from the list's length; an empty list writes nothing
        (0.0, 0.0, 0.0)."""
        idx = _idx4_list(idx4)
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_weighted_robust_pairs, self._h, (_ptr(idx), len(idx)), (int(loss), float(delta)),
                                 3, len(idx), 4, want_pairs)

    def evaluate_variance_robust(self, loss, delta, floor, want_pairs=False):
        """ecc_metric_evaluate_variance_robust: inverse-variance weights and the robust loss together, the loss in sigma units --
        for scans with lines whose noise is known (variance_intermediates) and an instrument nobody flagged.  The metric holds
        2 * n_views Radon intermediates as for evaluate_variance; loss as for evaluate_robust; floor as for evaluate_variance.  Per
        sample f = omega * w(|d| / sigma): omega = 1 / max(V_i + V_j, floor), sigma its root, w the IRLS weight of the STUDENTISED
        residual, so delta counts sigmas and a line that is merely noisy, and known to be, is not rejected for it.  Returns (value,
        mean_weight, inlier_mass): value = sum c / sum u (never divided by the mass the loss keeps), mean_weight = sum u / n_pairs,
        inlier_mass = sum k / sum u -- with want_pairs (value, mean_weight, inlier_mass, pairs), pairs (n_pairs, 4) float32 in the
        pair order of evaluate(cost): per pair c, its value, u, its mean weight, k, the weight mass the loss keeps, and r, the mean
        squared studentised residual (variance_robust_scale takes delta from r: V is a variance only up to a constant factor).
        delta = inf: the bits of evaluate_variance; V = 0.5 everywhere and floor <= 1: the bits of evaluate_robust.  The current
        matrices and everything the metric keeps stay."""
        return _scalar_form_call(_lib.lib().ecc_metric_evaluate_variance_robust, self._h, (), (int(loss), float(delta), float(floor)), 3,
                                 _n_all_pairs(self._Ps), 4, want_pairs)

    def _histogram_call(self, fn, lead, extra, n_bins):
        """fn(handle, *lead, *extra, n_bins, counts) -> counts, (n_views, n_bins) uint64, written completely."""
        n = 0 if self._Ps is None else len(self._Ps)
        counts = np.zeros((max(n, 1), max(int(n_bins), 1)), np.uint64)  # (no matrices, a bad n_bins: the library reports it)
        check(fn(self._h, *lead, *extra, int(n_bins), C.c_void_p(counts.ctypes.data)))
        return counts[:n]

    def evaluate_residual_histogram(self, width, n_bins=256):
        """ecc_metric_evaluate_residual_histogram: how the per-sample residuals of evaluate_robust are distributed, per view, from
        one pair launch -- before any delta exists.  Every +-kappa sample of every pair i < j, with evaluate_robust's positions and
        residual d in the metric's sampling mode, is counted in bin min(int(|d| / width), n_bins - 1) of row i AND of row j.
        width > 0 in the units of the data (float32); n_bins a multiple of 64 in [64, 1024]; the last bin is the overflow bin (NaN
        lands there).  Returns counts, (n_views, n_bins) uint64: a row's sum is that view's sample count, the sum of all cells twice
        the samples.  Integer sums on the device: the same call gives the same bits.  histogram_quantile reads a quantile off a row
        or a sum of rows, sample_robust_scale a delta.  The current matrices and everything the metric keeps stay."""
        return self._histogram_call(_lib.lib().ecc_metric_evaluate_residual_histogram, (), (float(width),), n_bins)

    def evaluate_residual_histogram_pairs(self, idx4, width, n_bins=256):
        """ecc_metric_evaluate_residual_histogram_pairs: evaluate_residual_histogram over an index list of (P0, P1, D0, D1) tuples;
        D0 and D1 lie in [0, n_views) and name the two rows a tuple's samples are counted in.  The sampling mode resolves from the
        list's length; a pair listed twice counts twice; an empty list gives zeros."""
        idx = _idx4_list(idx4)
        return self._histogram_call(_lib.lib().ecc_metric_evaluate_residual_histogram_pairs, (_ptr(idx), len(idx)), (float(width),), n_bins)

    def evaluate_variance_residual_histogram(self, floor, width, n_bins=256):
        """ecc_metric_evaluate_variance_residual_histogram: evaluate_residual_histogram in sigma units, on a 2 * n_views metric as
        evaluate_variance_robust takes it -- the binned quantity is |z| = |d| / sqrt(max(V_i + V_j, floor)), width counts sigmas.
        The share of a row below 1 (and 2, 3) is the calibration check of the variance fields: 68 % (95 %, 99.7 %) for Gaussian noise
        of the stated variance.  V = 0.5 everywhere and floor <= 1: the bits of evaluate_residual_histogram on the data alone."""
        return self._histogram_call(_lib.lib().ecc_metric_evaluate_variance_residual_histogram, (), (float(floor), float(width)), n_bins)

    def evaluate_variance_residual_histogram_pairs(self, idx4, floor, width, n_bins=256):
        """ecc_metric_evaluate_variance_residual_histogram_pairs: evaluate_variance_residual_histogram over an index list as
        evaluate_variance_robust_pairs takes it."""
        idx = _idx4_list(idx4)
        return self._histogram_call(_lib.lib().ecc_metric_evaluate_variance_residual_histogram_pairs, (_ptr(idx), len(idx)),
                                    (float(floor), float(width)), n_bins)

    def evaluate_variance_robust_map(self, loss, delta, floor, views=None, want_pairs=False):
        """ecc_metric_evaluate_variance_robust_map: evaluate_variance_robust(loss, delta, floor) on a 2 * n_views metric -- the same
        bits in value, mean_weight, inlier_mass and pairs -- and WHERE the loss rejected, in sigma units: per mapped view a HITS
        plane, the bilinear footprints of every sample taken in that view, and a REJ plane, the same times 1 - w, w the loss weight
        of the STUDENTISED residual.  The deposits are in count units (not multiplied by omega): REJ / HITS is the share of a bin's
        samples whose |z| exceeded delta.  views: data indices in [0, n_views) (distinct), None: every view in order.  Returns
        (value, mean_weight, inlier_mass, hits, rejected[, pairs]); hits, rejected: (len(views), n_t, n_alpha) float32, pairs
        (n_pairs, 4) rows {c, u, k, r}.  Fixed-point sums on the device: the same call gives the same bits.  delta = inf: rejected
        is all zeros and hits is evaluate_robust_map's on the n-metric.  variance_robust_map_variances turns the held map into the
        next pass's variance fields."""
        v, k = self._weighted_map_views(views)
        return _map_form_call(_lib.lib().ecc_metric_evaluate_variance_robust_map, self, (), (int(loss), float(delta), float(floor)), v, k, 3,
                              _n_all_pairs(self._Ps), 4, want_pairs)

    def evaluate_variance_robust_map_pairs(self, idx4, loss, delta, floor, views=None, want_pairs=False):
        """ecc_metric_evaluate_variance_robust_map_pairs: evaluate_variance_robust_map over an index list of (P0, P1, D0, D1) tuples
        as evaluate_variance_robust_pairs takes them: D0, D1 and `views` index the data intermediates, in [0, n_views); variance
        and map follow the data index.  A pair listed twice deposits twice; the planes do not depend on the order of the list."""
        idx = _idx4_list(idx4)
        v, k = self._weighted_map_views(views)
        return _map_form_call(_lib.lib().ecc_metric_evaluate_variance_robust_map_pairs, self, (_ptr(idx), len(idx)),
                              (int(loss), float(delta), float(floor)), v, k, 3, len(idx), 4, want_pairs)

    def variance_robust_map_variances(self, floor, min_hits=1.0, gain=1.0, max_factor=1e4):
        """ecc_metric_variance_robust_map_variances: the next pass's variance fields from the map the last
        evaluate_variance_robust_map[_pairs] call left on the device -- a list of RadonIntermediate (FILTER_NONE), one per mapped
        view in the order of `views`.  Per bin mu is robust_map_weights' rule on the held planes (1 where h < min_hits, else
        float32(max(0, 1 - gain * r / h)) in float64), factor = max_factor where mu * max_factor <= 1, else 1 / mu (float32), and the
        field is V where factor == 1, else max(V, floor / 2) * factor (float32), V the metric's current variance of that view.
        V / mu is the IRLS reading of the loss weight; the raise to floor / 2 lets a clean view's zeros be raised at all.  Raises if
        no map is held or the held map is another kind's."""
        return _map_weights_call(_lib.lib().ecc_metric_variance_robust_map_variances, self, floor, min_hits, gain, max_factor)

    def evaluate_transforms(self, n_source, Ts, want_pairs=False):
        """ecc_metric_evaluate_transforms: the registration of two scans (ref: tools/Registration/Registration3D3D.hxx).  The
        current matrices are the base, views [0, n_source) the source scan, the rest the target scan; Ts: anything np.asarray
        turns into (K, 4, 4) float64 in the mathematical (row, column) sense.  Transform k evaluates the source matrices
        geometry.compose_transform(P_i, Ts[k]) against the unchanged target matrices over the n_source x n_target cross pairs.
        Returns the K means (float64), with want_pairs also the pair values as (K, n_target, n_source) float32: every number
        bit-identical to setProjectionMatrices(composed) + evaluate(index list) per transform; the current matrices stay.
        Fix the object radius (setObjectRadius) for a sweep whose values are compared with each other."""
        flat = _transforms_colmajor(Ts)
        out = _transforms_call(_lib.lib().ecc_metric_evaluate_transforms, self._h, self.getNumberOfProjetions(), n_source, flat, (), 1, None,
                               want_pairs)
        return out if want_pairs else out[0]

    def evaluate_weighted_transforms(self, n_source, Ts, want_pairs=False):
        """ecc_metric_evaluate_weighted_transforms: evaluate_transforms for the metric with per-line weights (evaluate_weighted: the
        metric holds the data of every view, then its line weights; the weights follow the data, not the transformed matrix).  n_source
        and Ts as for evaluate_transforms.  Returns (values, coverages) = per transform (sum c / sum u, sum u / (n_source n_target))
        over the cross pairs -- with want_pairs (values, coverages, pairs), pairs (K, n_target, n_source, 2) float32 rows {c, u}: every
        number bit-identical to setProjectionMatrices(composed) + evaluate_weighted_pairs(the cross list) per transform; the current
        matrices stay."""
        flat = _transforms_colmajor(Ts)
        return _transforms_call(_lib.lib().ecc_metric_evaluate_weighted_transforms, self._h, self.getNumberOfProjetions(), n_source, flat, (), 2,
                                2, want_pairs)

    def evaluate_variance_transforms(self, n_source, Ts, floor, want_pairs=False):
        """ecc_metric_evaluate_variance_transforms: evaluate_transforms for the metric with inverse-variance sample weights
        (evaluate_variance: 2 * n_views intermediates; floor as there; the variance follows the data, not the transformed matrix).
        n_source and Ts as for evaluate_transforms.  Returns (values, mean_weights) = per transform (sum c / sum u, sum u / (n_source
        n_target)) over the cross pairs -- with want_pairs (values, mean_weights, pairs), pairs (K, n_target, n_source, 2) float32 rows
        {c, u}: every number bit-identical to setProjectionMatrices(composed) + evaluate_variance_pairs(the cross list, floor) per
        transform; the current matrices stay."""
        flat = _transforms_colmajor(Ts)
        return _transforms_call(_lib.lib().ecc_metric_evaluate_variance_transforms, self._h, self.getNumberOfProjetions(), n_source, flat,
                                (float(floor),), 2, 2, want_pairs)

    def evaluate_robust_transforms(self, n_source, Ts, loss, delta, want_pairs=False):
        """ecc_metric_evaluate_robust_transforms: evaluate_transforms under the per-sample robust loss of evaluate_robust (loss, delta
        as there; one intermediate per view).  n_source and Ts as for evaluate_transforms.  Returns (values, inlier_masses) = per
        transform (sum c, sum u) / (n_source n_target) over the cross pairs -- with want_pairs (values, inlier_masses, pairs), pairs
        (K, n_target, n_source, 3) float32 rows {c, u, r}: every number bit-identical to setProjectionMatrices(composed) +
        evaluate_robust_pairs(the cross list, loss, delta) per transform; the current matrices stay."""
        flat = _transforms_colmajor(Ts)
        return _transforms_call(_lib.lib().ecc_metric_evaluate_robust_transforms, self._h, self.getNumberOfProjetions(), n_source, flat,
                                (int(loss), float(delta)), 2, 3, want_pairs)

    def evaluate_weighted_robust_transforms(self, n_source, Ts, loss, delta, want_pairs=False):
        """ecc_metric_evaluate_weighted_robust_transforms: evaluate_transforms under line weights and the robust loss together
        (evaluate_weighted_robust: 2 * n_views intermediates; loss, delta as there).  n_source and Ts as for evaluate_transforms.
        Returns (values, coverages, inlier_masses) = per transform (sum c / sum u, sum u / (n_source n_target), sum k / sum u) over the
        cross pairs -- with want_pairs also pairs (K, n_target, n_source, 4) float32 rows {c, u, k, r}: every number bit-identical to
        setProjectionMatrices(composed) + evaluate_weighted_robust_pairs(the cross list, loss, delta) per transform; the current
        matrices stay."""
        flat = _transforms_colmajor(Ts)
        return _transforms_call(_lib.lib().ecc_metric_evaluate_weighted_robust_transforms, self._h, self.getNumberOfProjetions(), n_source, flat,
                                (int(loss), float(delta)), 3, 4, want_pairs)

    def evaluate_variance_robust_transforms(self, n_source, Ts, loss, delta, floor, want_pairs=False):
        """ecc_metric_evaluate_variance_robust_transforms: evaluate_transforms under inverse-variance weights and the robust loss of
        the studentised residual (evaluate_variance_robust: 2 * n_views intermediates; loss, delta, floor as there; the variance
        follows the data, not the transformed matrix).  n_source and Ts as for evaluate_transforms.  Returns (values, mean_weights,
        inlier_masses) = per transform (sum c / sum u, sum u / (n_source n_target), sum k / sum u) over the cross pairs -- with
        want_pairs also pairs (K, n_target, n_source, 4) float32 rows {c, u, k, r}: every number bit-identical to
        setProjectionMatrices(composed) + evaluate_variance_robust_pairs(the cross list, loss, delta, floor) per transform; the
        current matrices stay."""
        flat = _transforms_colmajor(Ts)
        return _transforms_call(_lib.lib().ecc_metric_evaluate_variance_robust_transforms, self._h, self.getNumberOfProjetions(), n_source, flat,
                                (int(loss), float(delta), float(floor)), 3, 4, want_pairs)

    def last_batched_transforms(self):
        """Transforms of the last evaluate_transforms / evaluate_weighted_transforms / evaluate_robust_transforms /
        evaluate_weighted_robust_transforms call that went through the batch (0: the sequential way)."""
        return _last_count(_lib.lib().ecc_metric_last_batched_transforms, self._h)

    def evaluateForImagePair(self, i, j):
        """ref: evaluateForImagePair(i, j, redundant_samples0, redundant_samples1, kappas, radon_samples0,
        radon_samples1) (...RadonIntermediate.cpp:324-393, visualisation).  Returns (ecc, dict) with the
        reference's five output vectors (radon_samples as (n, 2) arrays of (angle, distance) texture
        coordinates) and K01."""
        L = _lib.lib()
        cap = C.c_int()
        check(L.ecc_metric_pair_samples_bound(self._h, C.byref(cap)))
        cap = cap.value
        s0, s1, kap = (np.empty(cap, np.float32) for _ in range(3))
        r0, r1 = np.empty((cap, 2), np.float32), np.empty((cap, 2), np.float32)
        K01 = np.empty(16, np.float32)
        n, ecc = C.c_int(), C.c_double()
        check(L.ecc_metric_evaluate_for_image_pair(
            self._h, int(i), int(j), cap, C.byref(n), C.c_void_p(s0.ctypes.data), C.c_void_p(s1.ctypes.data),
            C.c_void_p(kap.ctypes.data), C.c_void_p(r0.ctypes.data), C.c_void_p(r1.ctypes.data),
            C.c_void_p(K01.ctypes.data), C.byref(ecc)))
        n = n.value
        return ecc.value, dict(redundant_samples0=s0[:n], redundant_samples1=s1[:n], kappas=kap[:n],
                               radon_samples0=r0[:n], radon_samples1=r1[:n], K01=K01)

    def balanced_shards(self, world):
        """ecc_metric_balanced_shards: cost-balanced shard boundaries for the current matrices and object radius."""
        b = np.zeros(int(world) + 1, np.int64)
        check(_lib.lib().ecc_metric_balanced_shards(self._h, int(world), C.c_void_p(b.ctypes.data)))
        return [int(v) for v in b]

    def evaluate_range(self, first, count, want_pairs=False):
        """Partial sum over pairs [first, first+count) of the get_ij order (multi-GPU shard)."""
        s = C.c_double()
        vals = np.empty(count, np.float32) if want_pairs else None
        check(_lib.lib().ecc_metric_evaluate_range(self._h, int(first), int(count),
                                                   C.c_void_p(vals.ctypes.data if want_pairs else 0), C.byref(s)))
        return (s.value, vals) if want_pairs else s.value

    def evaluate_range_allreduce(self, comm, first, count):
        """ecc_metric_evaluate_range_allreduce: this rank's pairs, then the RCCL all-reduce of the partial sums over the ranks of
        `comm` (sharding.RcclComm), all stream-ordered inside one call; returns the sum over ALL ranks' pairs."""
        check(_lib.lib().ecc_metric_evaluate_range_allreduce(self._h, comm._h, int(first), int(count), self._mean_ref))
        return self._mean.value

    def evaluate_range_async(self, first, count, sum_tensor, pair_tensor=None):
        """Device-resident, non-synchronising form: sum_tensor is a 1-element float64 torch tensor."""
        check(_lib.lib().ecc_metric_evaluate_range_async(
            self._h, int(first), int(count), C.c_void_p(pair_tensor.data_ptr() if pair_tensor is not None else 0),
            C.c_void_p(sum_tensor.data_ptr())))

    def publish_scalar(self, value_tensor):
        """ecc_metric_publish_scalar: queue the hand-over of a 1-element float64 device tensor (e.g. an all-reduced partial
        sum) to the metric's pinned result slot on the context's stream; wait_scalar() returns it."""
        check(_lib.lib().ecc_metric_publish_scalar(self._h, C.c_void_p(value_tensor.data_ptr())))

    def wait_scalar(self):
        v = C.c_double()
        check(_lib.lib().ecc_metric_wait_scalar(self._h, C.byref(v)))
        return v.value

    def debug_geometry(self):
        n = self.getNumberOfProjetions()
        PinvTs, Cs = np.empty((n, 12), np.float32), np.empty((n, 4), np.float32)
        check(_lib.lib().ecc_metric_debug_geometry(self._h, C.c_void_p(PinvTs.ctypes.data), C.c_void_p(Cs.ctypes.data)))
        return PinvTs, Cs

    def debug_K01(self, first, count):
        out = np.empty((count, 16), np.float32)
        check(_lib.lib().ecc_metric_debug_K01(self._h, int(first), int(count), C.c_void_p(out.ctypes.data)))
        return out

    def debug_polynomials(self, first, count):
        """The sample-coordinate polynomials the pair-geometry kernel fitted: list of dicts with
        poly_ok, degree (the pair kernel evaluates the polynomials up to it), clamp_free (no sample can reach a clamp), x_scale, fold (2,), ca (2, 13), cd (2, 12)."""
        n = 4 + 2 * 13 + 2 * 12
        out = np.empty((count, n), np.float32)
        check(_lib.lib().ecc_metric_debug_polynomials(self._h, int(first), int(count), C.c_void_p(out.ctypes.data)))
        return [dict(poly_ok=bool(r[0]), degree=int(r[0]), clamp_free=bool(r[0] != int(r[0])), x_scale=float(r[1]), fold=r[2:4] > 0, ca=r[4:30].reshape(2, 13).astype(np.float64),
                     cd=r[30:54].reshape(2, 12).astype(np.float64)) for r in out]

    def close(self):
        if self._h and self.ctx._h:
            _lib.lib().ecc_metric_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedContext:
    """A context owned by a Group (never destroyed from here)."""

    def __init__(self, handle, device, group):
        self._h, self.device, self._group = handle, device, group  # keeps the group (and so the context) alive

    def synchronize(self):
        check(_lib.lib().ecc_ctx_synchronize(self._h))

    def close(self):
        self._h = C.c_void_p()


class Group:
    """Single-process multi-GPU: one context, stream and host thread per device (ecc_group_* of the C ABI).
    devices: list of HIP device indices (an index may repeat: rehearsal of the multi-rank path on one GPU)."""

    def __init__(self, devices):
        devices = [int(d) for d in devices]
        arr = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        check(_lib.lib().ecc_group_create(len(devices), arr, C.byref(self._h)))
        self.devices = devices
        self._ctxs = {}

    def __len__(self):
        return _lib.lib().ecc_group_size(self._h)

    def context(self, rank):
        if rank not in self._ctxs:
            h = C.c_void_p()
            check(_lib.lib().ecc_group_ctx(self._h, int(rank), C.byref(h)))
            self._ctxs[rank] = _BorrowedContext(h, self.devices[rank], self)
        return self._ctxs[rank]

    def compute_batch(self, images, size_alpha, size_t, filter=FILTER_DERIVATIVE, post_process=POST_IDENTITY):
        """Radon intermediates of host images (n, n_v, n_u), data-parallel over the group's devices."""
        keep = np.ascontiguousarray(images, np.float32)
        n, n_v, n_u = keep.shape
        hs = (C.c_void_p * n)()
        check(_lib.lib().ecc_group_radon_compute_batch(self._h, C.c_void_p(keep.ctypes.data), n, n_u, n_v, size_alpha,
                                                       size_t, filter, post_process, hs))
        chunk = (n + len(self.devices) - 1) // len(self.devices)
        ctxs = [self.context(r) for r in range(len(self.devices))]
        return [RadonIntermediate(ctxs[k // chunk], C.c_void_p(h)) for k, h in enumerate(hs)]

    def close(self):
        """Destroy group metrics and Radon intermediates made from the group's contexts first."""
        if self._h:
            for c in self._ctxs.values():
                c.close()  # objects that still hold one of these contexts will not touch it any more
            self._ctxs = {}
            _lib.lib().ecc_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pair_shard(n_pairs, world, rank):
    """ecc_pair_shard: (first, count) of `rank`'s contiguous chunk of the get_ij order."""
    a, b = C.c_int64(), C.c_int64()
    _lib.lib().ecc_pair_shard(int(n_pairs), int(world), int(rank), C.byref(a), C.byref(b))
    return a.value, b.value


def pair_shards_balanced(Ps, object_radius_mm, world):
    """ecc_pair_shards_balanced: world + 1 boundaries of contiguous, cost-balanced chunks of the get_ij order (rank r
    evaluates [b[r], b[r+1])).  Ps: list of 3x4 matrices or an (n, 12) column-major array."""
    if isinstance(Ps, np.ndarray) and Ps.ndim == 2 and Ps.shape[1] == 12:
        flat = np.ascontiguousarray(Ps, np.float64)
    else:
        flat = _Ps_colmajor(Ps)
    b = np.zeros(int(world) + 1, np.int64)
    check(_lib.lib().ecc_pair_shards_balanced(C.c_void_p(flat.ctypes.data), len(flat), float(object_radius_mm), int(world),
                                              C.c_void_p(b.ctypes.data)))
    return [int(v) for v in b]


class GroupMetricRadonIntermediate:
    """MetricRadonIntermediate over a Group: the same setProjectionMatrices / evaluate calls, every device of the
    group evaluating a contiguous shard of the pair range (ecc_group_metric_* of the C ABI)."""

    def __init__(self, group, Ps=None, dtrs=None):
        self.group = group
        self._h = C.c_void_p()
        self._dtrs = []
        self._Ps = None
        if dtrs is not None:
            self.setRadonIntermediates(dtrs)
        if Ps is not None:
            self.setProjectionMatrices(Ps)

    def setRadonIntermediates(self, dtrs):
        self.close()
        self._dtrs = list(dtrs)
        hs = (C.c_void_p * len(self._dtrs))(*[d._h for d in self._dtrs])
        check(_lib.lib().ecc_group_metric_create(self.group._h, len(self._dtrs), hs, C.byref(self._h)))
        d = MetricRadonIntermediate.default_sampling
        if d is not None:
            self.setSampling(d)
        if self._Ps is not None:
            self.setProjectionMatrices(self._Ps)
        return self

    def setProjectionMatrices(self, Ps):
        if isinstance(Ps, np.ndarray) and Ps.ndim == 2 and Ps.shape[1] == 12 and Ps.dtype == np.float64 \
                and Ps.flags["C_CONTIGUOUS"]:
            self._Ps = Ps
        else:
            self._Ps = _Ps_colmajor(Ps)
        if self._h:
            check(_lib.lib().ecc_group_metric_set_projections(self._h, C.c_void_p(self._Ps.ctypes.data), len(self._Ps)))
        return self

    def getNumberOfProjetions(self):  # sic
        return 0 if self._Ps is None else len(self._Ps)

    def setObjectRadius(self, radius_mm=0.0, dkappa=0.0, use_corr=False):
        check(_lib.lib().ecc_group_metric_set_params(self._h, float(radius_mm), float(dkappa), 1 if use_corr else 0))
        return self

    def getObjectRadius(self):
        r = C.c_double()
        check(_lib.lib().ecc_group_metric_get_object_radius(self._h, C.byref(r)))
        return r.value

    def setSampling(self, mode="auto"):
        mode = MetricRadonIntermediate._SAMPLING[mode] if isinstance(mode, str) else int(mode)
        check(_lib.lib().ecc_group_metric_set_sampling(self._h, mode))
        return self

    def setIncremental(self, enable=True):
        """ecc_group_metric_set_incremental: every rank keeps the pair values of its shard (see
        MetricRadonIntermediate.setIncremental)."""
        check(_lib.lib().ecc_group_metric_set_incremental(self._h, int(bool(enable))))
        return self

    def last_evaluated_pairs(self):
        """Pairs the ranks recomputed in the last evaluation, summed over the ranks."""
        total = 0
        for r in range(len(self.group)):
            m, v = C.c_void_p(), C.c_int64()
            check(_lib.lib().ecc_group_metric_rank_metric(self._h, r, C.byref(m)))
            check(_lib.lib().ecc_metric_last_evaluated_pairs(m, C.byref(v)))
            total += v.value
        return total

    def evaluate_poses(self, poses):
        """Independent all-pairs evaluations of several poses (ecc_group_metric_evaluate_poses): poses is a sequence of
        (n, 12) column-major arrays (pack_projection_matrices) or lists of 3x4 matrices; returns the means.  Pose p runs
        entirely on rank p mod G."""
        flat = np.ascontiguousarray(np.stack([p if (isinstance(p, np.ndarray) and p.ndim == 2 and p.shape[1] == 12)
                                              else _Ps_colmajor(p) for p in poses]), np.float64)
        means = np.zeros(len(flat), np.float64)
        check(_lib.lib().ecc_group_metric_evaluate_poses(self._h, len(flat), C.c_void_p(flat.ctypes.data), flat.shape[1],
                                                         C.c_void_p(means.ctypes.data)))
        return means

    def rebalance(self):
        """Recompute the cost-balanced shard boundaries at the next evaluation (ecc_group_metric_rebalance)."""
        check(_lib.lib().ecc_group_metric_rebalance(self._h))
        return self

    def evaluate(self, cost=None):
        mean = C.c_double()
        if cost is not None:
            n = self.getNumberOfProjetions()
            assert cost.dtype == np.float32 and cost.flags["C_CONTIGUOUS"] and cost.shape == (n, n)
        check(_lib.lib().ecc_group_metric_evaluate_all(self._h, C.c_void_p(cost.ctypes.data if cost is not None else 0),
                                                       C.byref(mean)))
        return mean.value

    def close(self):
        if self._h and self.group._h:
            _lib.lib().ecc_group_metric_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MetricDirect:
    """ref: class MetricDirect : public Metric (EpipolarConsistencyDirect.h:28-60): epipolar consistency straight
    from the projection images.  images: (n, n_v, n_u) float32, numpy (uploaded, owned) or a torch tensor on ctx's
    device (borrowed, like the reference borrows its textures)."""

    def __init__(self, ctx, Ps, images):
        self.ctx = ctx
        self._h = C.c_void_p()
        self._params = [0.0, 0.0, 0]
        self._Ps = None
        self.setProjectionImages(images)
        if Ps is not None:
            self.setProjectionMatrices(Ps)

    def setProjectionImages(self, images):
        if self._h:
            _lib.lib().ecc_direct_destroy(self._h)
            self._h = C.c_void_p()
        if _is_torch(images):
            import torch
            assert images.dtype == torch.float32 and images.is_contiguous() and images.is_cuda and images.dim() == 3
            self._keep, ptr, on_dev = images, images.data_ptr(), 1
        else:
            self._keep = np.ascontiguousarray(images, np.float32)
            assert self._keep.ndim == 3
            ptr, on_dev = self._keep.ctypes.data, 0
        n, n_v, n_u = self._keep.shape
        self._n = n
        check(_lib.lib().ecc_direct_create(self.ctx._h, n, C.c_void_p(ptr), on_dev, n_u, n_v, C.byref(self._h)))
        check(_lib.lib().ecc_direct_set_params(self._h, *self._params))
        if self._Ps is not None:
            self.setProjectionMatrices(self._Ps)
        return self

    def setProjectionMatrices(self, Ps):
        self._Ps = _Ps_colmajor(Ps)
        check(_lib.lib().ecc_direct_set_projections(self._h, C.c_void_p(self._Ps.ctypes.data), len(self._Ps)))
        return self

    def getNumberOfProjetions(self):  # sic
        return self._n

    def updateImages(self):
        """Call after changing the pixels of borrowed device images (refreshes the transposed copy)."""
        check(_lib.lib().ecc_direct_update_images(self._h))
        return self

    def _push(self):
        check(_lib.lib().ecc_direct_set_params(self._h, *self._params))
        return self

    def setObjectRadius(self, radius_mm=0.0):
        self._params[0] = float(radius_mm)
        return self._push()

    def getObjectRadius(self):
        r = C.c_double()
        check(_lib.lib().ecc_direct_get_object_radius(self._h, C.byref(r)))
        return r.value

    def setEpipolarPlaneStep(self, dkappa_rad=0.0):
        self._params[1] = float(dkappa_rad)
        return self._push()

    def setFanBeamConsistency(self, fbcc=True):
        self._params[2] = 1 if fbcc else 0
        return self._push()

    def evaluate(self, cost=None):
        """ref: MetricDirect::evaluate(float* out): the SUM over all pairs; cost (n,n) float32: entry [j, i], i<j."""
        s = C.c_double()
        if cost is not None:
            assert cost.dtype == np.float32 and cost.flags["C_CONTIGUOUS"] and cost.shape == (self._n, self._n)
        check(_lib.lib().ecc_direct_evaluate(self._h, C.c_void_p(cost.ctypes.data if cost is not None else 0), C.byref(s)))
        return s.value

    def evaluateForImagePair(self, i, j, kappas=None):
        """ref: evaluateForImagePair(i, j, redundant_samples0, redundant_samples1, kappas); also returns the lines.
        kappas: optional caller-provided grid of plane angles (the reference takes a non-empty `kappas` as input)."""
        L = _lib.lib()
        if kappas is not None:
            kap = np.ascontiguousarray(kappas, np.float32).reshape(-1)
            s0, s1, lines = np.empty(len(kap), np.float32), np.empty(len(kap), np.float32), np.empty((len(kap), 6), np.float32)
            m = C.c_double()
            check(L.ecc_direct_evaluate_for_image_pair_kappas(self._h, int(i), int(j), len(kap), C.c_void_p(kap.ctypes.data),
                                                              C.c_void_p(s0.ctypes.data), C.c_void_p(s1.ctypes.data),
                                                              C.c_void_p(lines.ctypes.data), C.byref(m)))
            return m.value, dict(redundant_samples0=s0, redundant_samples1=s1, kappas=kap, lines=lines)
        cap = C.c_int()
        check(L.ecc_direct_lines_bound(self._h, C.byref(cap)))
        cap = cap.value
        s0, s1, kap = (np.empty(cap, np.float32) for _ in range(3))
        lines = np.empty((cap, 6), np.float32)
        n, m = C.c_int(), C.c_double()
        check(L.ecc_direct_evaluate_for_image_pair(self._h, int(i), int(j), cap, C.byref(n), C.c_void_p(s0.ctypes.data),
                                                   C.c_void_p(s1.ctypes.data), C.c_void_p(kap.ctypes.data),
                                                   C.c_void_p(lines.ctypes.data), C.byref(m)))
        n = n.value
        return m.value, dict(redundant_samples0=s0[:n], redundant_samples1=s1[:n], kappas=kap[:n], lines=lines[:n])

    def evaluate_pairs(self, idx4, segments=None, want_pairs=False):
        """ecc_direct_evaluate_pairs: the reference's index list of (P0, P1, I0, I1) tuples -- P* rows of the matrix table given to
        setProjectionMatrices (it may hold more matrices than there are images: candidates), I* images.  Every entry has the bits of
        evaluateForImagePair's metric.  segments: S + 1 non-decreasing offsets into the list (first 0, last its length) -> the S
        float64 sums; None -> the sum of the whole list as a float.  With want_pairs: (sums, pair values in list order)."""
        idx = _idx4_list(idx4)
        off = None if segments is None else np.ascontiguousarray(segments, np.int64).reshape(-1)
        if off is not None and len(off) < 1:
            raise ValueError("segments must hold at least one offset")
        sums = np.zeros(1 if off is None else len(off) - 1, np.float64)
        pairs = np.zeros(len(idx), np.float64) if want_pairs else None
        # (an empty output still has an address here: the C call refuses only two null outputs)
        check(_lib.lib().ecc_direct_evaluate_pairs(self._h, _ptr(idx), len(idx), None if off is None else C.c_void_p(off.ctypes.data),
                                                   len(sums), None if pairs is None else C.c_void_p(pairs.ctypes.data),
                                                   C.c_void_p(sums.ctypes.data)))
        total = float(sums[0]) if off is None else sums
        return (total, pairs) if want_pairs else total

    def evaluate_pose_deltas(self, moved_views, moved_Ps, want_pairs=False):
        """ecc_direct_evaluate_pose_deltas: pose k = the set matrices with the views moved_views[k] replaced by moved_Ps[k] (as
        MetricRadonIntermediate.evaluate_pose_deltas takes them).  Returns the K sums over the pairs that contain a moved view --
        the pairs without one are a constant of the batch that the caller owns (evaluate_pairs over them, once).  With want_pairs:
        (sums, terms, their (i, j, i, j) tuples), pose after pose in direct_pose_pairs order.  The set matrices stay."""
        return self.evaluate_pose_deltas_packed(*_pack_pose_lists(moved_views, moved_Ps), want_pairs=want_pairs)

    def evaluate_pose_deltas_packed(self, moved_offsets, moved_views, moved_Ps, want_pairs=False):
        """The C signature itself: moved_offsets (K + 1 int32, [0] = 0), moved_views (Q int32), moved_Ps ((Q, 12) float64)."""
        off, views, flat = _check_pose_lists(moved_offsets, moved_views, moved_Ps)
        K = len(off) - 1
        sums = np.zeros(K, np.float64)
        pairs = tuples = None
        if want_pairs:
            n = C.c_int64()
            check(_lib.lib().ecc_direct_pose_pairs_bound(self._h, K, C.c_void_p(off.ctypes.data), C.byref(n)))
            pairs, tuples = np.zeros(n.value, np.float64), np.zeros((n.value, 4), np.int32)
        check(_lib.lib().ecc_direct_evaluate_pose_deltas(self._h, K, C.c_void_p(off.ctypes.data), _ptr(views), _ptr(flat),
                                                         _ptr(sums), _ptr(pairs), _ptr(tuples)))
        return (sums, pairs, tuples) if want_pairs else sums

    def debug_set_batch(self, max_pairs=0):
        """ecc_debug_set_direct_batch: at most max_pairs list entries per internal batch (0: the library's bound).  Same bits."""
        check(_lib.lib().ecc_debug_set_direct_batch(self._h, int(max_pairs)))
        return self

    def close(self):
        if self._h and self.ctx._h:
            _lib.lib().ecc_direct_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def direct_pose_pairs(n_images, moved_views):
    """The tuples MetricDirect.evaluate_pose_deltas evaluates for ONE pose that moves `moved_views`, in its order: (i, j, i, j) for
    every pair i < j < n_images with at least one moved view, each once, ascending in (i, j).  (n_pairs, 4) int32.  Pure Python."""
    moved = {int(v) for v in np.atleast_1d(moved_views)} if np.size(moved_views) else set()
    if any(v < 0 or v >= n_images for v in moved):
        raise ValueError("moved view out of range")
    rows = [(i, j, i, j) for i in range(n_images) for j in range(i + 1, n_images) if i in moved or j in moved]
    return np.asarray(rows, np.int32).reshape(-1, 4)


def slab_floats(n_alpha, n_t):
    """Floats per dtr in the private device layout (csrc/ecc_layout.h)."""
    return _lib.lib().ecc_dtr_slab_floats(int(n_alpha), int(n_t))


def get_ij(ij, n):
    i, j = C.c_int(), C.c_int()
    _lib.lib().ecc_get_ij(int(ij), int(n), C.byref(i), C.byref(j))
    return i.value, j.value


def host_pinvT(P):
    P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, 4).T).reshape(12)
    out = np.empty(12, np.float32)
    _lib.lib().ecc_host_pinvT(C.c_void_p(P.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def host_source_position(P):
    P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, 4).T).reshape(12)
    out = np.empty(4, np.float32)
    _lib.lib().ecc_host_source_position(C.c_void_p(P.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def host_object_radius(P, n_u, n_v):
    P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, 4).T).reshape(12)
    return _lib.lib().ecc_host_object_radius(C.c_void_p(P.ctypes.data), int(n_u), int(n_v))


def host_intrinsics(P):
    """(sdd_px, ppu, ppv) = K(0,0), K(0,2), K(1,2) of P = K[R|t] (ref: getCameraIntrinsics)."""
    P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, 4).T).reshape(12)
    a, b, c = C.c_float(), C.c_float(), C.c_float()
    _lib.lib().ecc_host_intrinsics(C.c_void_p(P.ctypes.data), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _P12(P):
    return np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, 4).T).reshape(12)


def estimateAngularRange(P0, P1, object_radius_mm):
    """ref: estimateAngularRange(join_pluecker(C0, C1), radius) (EpipolarConsistency.cpp:49-59)."""
    a, b, A, B = C.c_double(), C.c_double(), _P12(P0), _P12(P1)
    _lib.lib().ecc_host_angular_range(C.c_void_p(A.ctypes.data), C.c_void_p(B.ctypes.data), float(object_radius_mm),
                                      C.byref(a), C.byref(b))
    return a.value, b.value


def estimateAngularStep(P0, P1, n_u, n_v):
    """ref: estimateAngularStep (EpipolarConsistency.cpp:61-68)."""
    A, B = _P12(P0), _P12(P1)
    return _lib.lib().ecc_host_angular_step(C.c_void_p(A.ctypes.data), C.c_void_p(B.ctypes.data), int(n_u), int(n_v))


def estimateIsoCenter(Ps):
    """ref: estimateIsoCenter (EpipolarConsistency.cpp:8-33)."""
    flat = _Ps_colmajor(Ps)
    O = np.zeros(4)
    _lib.lib().ecc_host_iso_center(C.c_void_p(flat.ctypes.data), len(flat), C.c_void_p(O.ctypes.data))
    return O


estimateObjectRadius = host_object_radius  # ref: estimateObjectRadius (EpipolarConsistency.cpp:35-47)


def gram_value(G, a):
    """a^T G a in float64: the metric of the coefficient vector a under the Gram matrix of evaluate_gram."""
    G = np.asarray(G, np.float64)
    a = np.asarray(a, np.float64).reshape(-1)
    if G.ndim != 2 or G.shape != (len(a), len(a)):
        raise ValueError("G must be (K, K) and a (K,)")
    return float(a @ (G @ a))


def gram_minimizer(G, fixed=0, value=1.0):
    """The minimiser of a^T G a under a[fixed] = value: with F the free coordinates, G[F, F] a_F = -value * G[F, fixed] (one
    numpy.linalg.solve).  Returns (a, a^T G a).  Raises numpy.linalg.LinAlgError when G[F, F] is not positive definite -- the form
    has no minimum there."""
    G = np.asarray(G, np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1:
        raise ValueError("G must be (K, K)")
    K = G.shape[0]
    fixed = int(fixed)
    if not 0 <= fixed < K:
        raise ValueError("fixed outside [0, K)")
    free = [c for c in range(K) if c != fixed]
    a = np.zeros(K, np.float64)
    a[fixed] = float(value)
    if free:
        H = 0.5 * (G[np.ix_(free, free)] + G[np.ix_(free, free)].T)
        np.linalg.cholesky(H)  # raises LinAlgError unless positive definite
        a[free] = np.linalg.solve(H, -float(value) * 0.5 * (G[free, fixed] + G[fixed, free]))
    return a, gram_value(G, a)


def minimize_view_coefficients(metric, K, start, free, tol=1e-4, max_iter=None):
    """Conjugate gradients on the host over per-view channel coefficients (MetricRadonIntermediate.evaluate_view_coefficients).
    start: (K, n) coefficients; free: (K, n) boolean mask of the coefficients to minimise over, the others stay at `start`.  The
    metric is the quadratic form a^T G a, so with the free coordinates x (a = start + P x) the system is H x = -g0, H = the free
    block of 2 G, g0 = the free gradient at `start`; every product H p is ONE call of evaluate_view_coefficients at the direction
    P p (the gradient of a quadratic form is linear).  Returns (a, value, iterations) once |free gradient|_inf <= tol * |g0|_inf (the
    recurrence's residual; iterations = operator products); a is (K, n) float64 and the value is the metric's at a (rounded to
    float32 by the call).  Raises numpy.linalg.LinAlgError when a direction has p . H p <= 0 -- the form has no minimum over the
    free coordinates -- and RuntimeError when max_iter (default: twice the number of free coefficients plus ten) products did not
    reach the tolerance.  `metric` needs evaluate_view_coefficients only."""
    a = np.array(start, np.float64)
    mask = np.asarray(free, bool)
    if a.ndim != 2 or a.shape[0] != int(K) or mask.shape != a.shape:
        raise ValueError("start and free must be (K, n_views)")
    n_free = int(mask.sum())
    if max_iter is None:
        max_iter = 2 * n_free + 10

    def gradient(coeffs):
        value, grad = metric.evaluate_view_coefficients(coeffs)[:2]
        return float(value), np.asarray(grad, np.float64)[mask]
    value, g0 = gradient(a)
    scale = float(np.max(np.abs(g0))) if n_free else 0.0
    iterations = 0
    if scale == 0.0:
        return a, value, iterations
    r = -g0
    p = r.copy()
    rr = float(r @ r)
    direction = np.zeros_like(a)
    while np.max(np.abs(r)) > tol * scale:
        if iterations >= max_iter:
            raise RuntimeError("minimize_view_coefficients: %d products did not reach the tolerance" % iterations)
        direction[mask] = p
        Hp = gradient(direction)[1]
        iterations += 1
        pHp = float(p @ Hp)
        if not pHp > 0.0:
            raise np.linalg.LinAlgError("the metric has no minimum over the free coefficients: a direction with p . H p <= 0")
        alpha = rr / pHp
        a[mask] += alpha * p
        r -= alpha * Hp
        rr_new = float(r @ r)
        p = r + (rr_new / rr) * p
        rr = rr_new
    return a, metric.evaluate_view_coefficients(a)[0], iterations


def line_weights_from_lengths(lengths, zero_at_px=1.0, guard_bins=1):
    """The host half of line_weights: lengths (n_t, n_alpha) float32, the length of every bin's line inside flagged pixels ->
    float32 weights clip(1 - L / zero_at_px, 0, 1) (float32 operations), then the minimum over the (2 guard_bins + 1)^2 bin
    neighbourhood, the grid's edges clamped as the bilinear taps clamp them."""
    L = np.asarray(lengths, np.float32)
    if L.ndim != 2:
        raise ValueError("lengths must be (n_t, n_alpha)")
    if not zero_at_px > 0:
        raise ValueError("zero_at_px must be positive")
    g = int(guard_bins)
    if g < 0:
        raise ValueError("guard_bins must not be negative")
    w = np.clip(np.float32(1.0) - L / np.float32(zero_at_px), np.float32(0.0), np.float32(1.0)).astype(np.float32)
    if g:
        padded = np.pad(w, g, mode="edge")
        n_t, n_alpha = w.shape
        out = w
        for dj in range(2 * g + 1):
            for di in range(2 * g + 1):
                out = np.minimum(out, padded[dj:dj + n_t, di:di + n_alpha])
        w = out
    return np.ascontiguousarray(w, np.float32)


def line_weights(ctx, flagged, size_alpha, size_t, zero_at_px=1.0, guard_bins=1):
    """Line weights for MetricRadonIntermediate.evaluate_weighted from an image of flagged pixels.  flagged: (n_v, n_u) float32, 1
    where a pixel must not be trusted (an instrument, a collimator blade, a defective column) and 0 elsewhere -- or (n, n_v, n_u) /
    a list of such images, for which a list is returned.  L, the FILTER_NONE / POST_IDENTITY Radon intermediate of `flagged` from the
    Radon kernel, is the length in pixels of every bin's line inside flagged pixels; the weight is clip(1 - L / zero_at_px, 0, 1),
    followed by the minimum over the (2 guard_bins + 1)^2 bin neighbourhood (line_weights_from_lengths), so that with guard_bins >= 1
    a bilinear sample with a weight above 0 touches no bin with L >= zero_at_px.  Returns a RadonIntermediate with FILTER_NONE on
    the same bin grid.  Runs once per data set: one readback, numpy on the host, one upload."""
    arr = np.asarray(flagged, np.float32)
    single = arr.ndim == 2
    if arr.ndim not in (2, 3):
        raise ValueError("flagged must be (n_v, n_u) or (n, n_v, n_u)")
    stack = arr[None] if single else arr
    n_v, n_u = stack.shape[1:]
    out = []
    for d in RadonIntermediate.compute_batch(ctx, stack, size_alpha, size_t, FILTER_NONE, POST_IDENTITY):
        w = line_weights_from_lengths(d.readback(), zero_at_px, guard_bins)
        d.close()
        out.append(RadonIntermediate.from_host(ctx, w, n_u, n_v, FILTER_NONE))
    return out[0] if single else out


def variance_intermediates(ctx, pixel_variances, size_alpha, size_t):
    """Variance fields for MetricRadonIntermediate.evaluate_variance from images of pixel variances.  The model: V is the line
    integral of the pixel variances -- the variance of a line integral of independent pixels --, up to a constant factor that cancels
    in value.  For derivative data the same field is used, which ignores the correlation of the two neighbouring lines of the finite
    difference.  pixel_variances: (n_v, n_u) float32, or (n, n_v, n_u) / a list of such images, for which a list is returned.
    Returns RadonIntermediate(s) with FILTER_NONE on the bin grid size_alpha x size_t: RadonIntermediate.compute_batch with
    FILTER_NONE / POST_IDENTITY, nothing else."""
    arr = np.asarray(pixel_variances, np.float32)
    single = arr.ndim == 2
    if arr.ndim not in (2, 3):
        raise ValueError("pixel_variances must be (n_v, n_u) or (n, n_v, n_u)")
    out = RadonIntermediate.compute_batch(ctx, arr[None] if single else arr, size_alpha, size_t, FILTER_NONE, POST_IDENTITY)
    return out[0] if single else out


def variance_floor(fields, fraction=1e-3):
    """ecc_host_variance_floor: a floor for evaluate_variance from the variance fields themselves -- fraction x the median of their
    strictly positive finite entries (float32).  fields: one array or a sequence of arrays (RadonIntermediate.readback() of the
    variance intermediates).  Raises EccError when no entry is positive or the fraction is not in (0, inf)."""
    if isinstance(fields, np.ndarray):
        flat = np.ascontiguousarray(fields, np.float32).reshape(-1)
    else:
        parts = [np.asarray(f, np.float32).reshape(-1) for f in fields]
        flat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.float32))
    out = C.c_float(0.0)
    check(_lib.lib().ecc_host_variance_floor(C.c_void_p(flat.ctypes.data) if flat.size else None, flat.size, float(fraction),
                                             C.cast(C.byref(out), C.c_void_p)))
    return float(out.value)


def robust_scale(pair_terms, k=1.0):
    """ecc_host_robust_scale: a scale delta for evaluate_robust from the pair rows {c, u, r} of an earlier call (normally the one
    with delta = inf) -- k x the median over the pairs with r > 0 of sqrt(r), the pair's rms residual; 0.0 without such a pair.  A
    minority of corrupted views reaches a minority of the pairs, so the median stays put where the pooled rms does not."""
    rows = np.ascontiguousarray(pair_terms, np.float32)
    if rows.ndim != 2 or rows.shape[1] != 3:
        raise ValueError("pair_terms must be (n_pairs, 3) rows {c, u, r}")
    return float(_lib.lib().ecc_host_robust_scale(C.c_void_p(rows.ctypes.data) if len(rows) else None, len(rows), float(k)))


def weighted_robust_scale(pair_terms, k=1.0):
    """ecc_host_weighted_robust_scale: a scale delta for evaluate_weighted_robust from the pair rows {c, u, k, r} of an earlier call
    (normally the one with delta = inf) -- k x the median over the pairs with r > 0 and u > 0 of sqrt(r / u), the pair's rms residual
    over the lines its weights trust; 0.0 without such a pair.  With every u == 1 it is robust_scale of the rows {c, k, r}."""
    rows = np.ascontiguousarray(pair_terms, np.float32)
    if rows.ndim != 2 or rows.shape[1] != 4:
        raise ValueError("pair_terms must be (n_pairs, 4) rows {c, u, k, r}")
    return float(_lib.lib().ecc_host_weighted_robust_scale(C.c_void_p(rows.ctypes.data) if len(rows) else None, len(rows), float(k)))


def variance_robust_scale(pair_terms, k=1.0):
    """ecc_host_variance_robust_scale: a scale delta for evaluate_variance_robust from the pair rows {c, u, k, r} of an earlier call
    (normally the one with delta = inf) -- k x the median over the pairs with r > 0 of sqrt(r), the pair's rms studentised residual;
    0.0 without such a pair.  V is the line variance only up to a constant factor, so this is what one sigma measures on the data."""
    rows = np.ascontiguousarray(pair_terms, np.float32)
    if rows.ndim != 2 or rows.shape[1] != 4:
        raise ValueError("pair_terms must be (n_pairs, 4) rows {c, u, k, r}")
    return float(_lib.lib().ecc_host_variance_robust_scale(C.c_void_p(rows.ctypes.data) if len(rows) else None, len(rows), float(k)))


def histogram_quantile(counts, width, q):
    """ecc_host_histogram_quantile: the q-quantile (q in [0, 1]) of the binned quantity from the counts of
    evaluate_residual_histogram at the same width -- one row, or any (..., n_bins) array, whose rows are added first.  Linear
    interpolation inside the bin where the cumulative count crosses q x total; inf when that is the overflow bin (take a larger
    width); 0.0 for no samples; nan for q outside [0, 1]."""
    c = np.asarray(counts)
    if c.ndim < 1 or c.shape[-1] < 1:
        raise ValueError("counts must be (n_bins,) or (..., n_bins)")
    row = np.ascontiguousarray(c.reshape(-1, c.shape[-1]).sum(axis=0, dtype=np.uint64))
    return float(_lib.lib().ecc_host_histogram_quantile(C.c_void_p(row.ctypes.data), len(row), float(width), float(q)))


def sample_robust_scale(metric, q=0.5, k=1.4826, n_bins=256, floor=None, first_width=None):
    """A scale delta for evaluate_robust from the SAMPLES: k x the q-quantile of |d| over all samples of all pairs (the defaults:
    1.4826 x the median absolute residual, the Gaussian-consistent MAD).  robust_scale takes delta from per-pair rms figures, which
    the outliers themselves pull up; the loss is applied per sample.  floor: None for a metric as evaluate_robust takes it; a
    variance floor for a 2 * n_views metric, delta then counts sigmas (evaluate_variance_robust).  The first bin width spreads
    4 x robust_scale (variance_robust_scale) of the delta = inf rows over the bins (first_width: the caller's own first width
    instead, and no delta = inf call); while the quantile lies in the overflow bin the width doubles, at most 32 times, then
    RuntimeError (NaN data, which stays in the overflow bin, with a q that reaches it).  The answer is exact to within one bin of
    the last width.  q in [0, 1], else ValueError before anything is launched.  Returns 0.0 when every residual is zero."""
    q, k = float(q), float(k)
    if not 0.0 <= q <= 1.0:
        raise ValueError("sample_robust_scale: q must lie in [0, 1]")
    if floor is None:
        histogram = lambda w: metric.evaluate_residual_histogram(w, n_bins)
    else:
        histogram = lambda w: metric.evaluate_variance_residual_histogram(floor, w, n_bins)
    if first_width is None:
        if floor is None:
            first = robust_scale(metric.evaluate_robust(_lib.LOSS_TRUNCATED, float("inf"), want_pairs=True)[-1])
        else:
            first = variance_robust_scale(metric.evaluate_variance_robust(_lib.LOSS_TRUNCATED, float("inf"), floor, want_pairs=True)[-1])
        if not first > 0.0:
            return 0.0
        width = float(np.float32(4.0 * first / int(n_bins)))
    else:
        width = float(np.float32(first_width))
        if not (width > 0.0 and np.isfinite(width)):
            raise ValueError("sample_robust_scale: first_width must be finite and > 0")
    for _ in range(33):
        value = histogram_quantile(histogram(width), width, q)
        if np.isfinite(value):
            return k * value
        width *= 2.0
    raise RuntimeError("sample_robust_scale: the quantile stayed in the overflow bin after 32 doublings of the bin width")


def refine_line_weights(ctx, Ps, data, weights=None, loss=_lib.LOSS_TRUNCATED, k=0.5, passes=2, min_hits=1.0, gain=1.0, sampling="auto"):
    """Line weights from the robust loss, iterated: the loss says where it rejects, the map becomes line weights, and the next pass
    maps the metric under those weights.  data: the n Radon intermediates of the views Ps; weights: n line-weight
    intermediates to start from (a collimator flag from line_weights, say) or None.  Pass 1 is evaluate_robust_map +
    robust_map_weights on the n-metric when weights is None, otherwise evaluate_weighted_robust_map + weighted_robust_map_weights
    on the 2 n metric over `weights`; every later pass is the weighted map on a 2 n metric over the previous pass's weights.
    delta = k x robust_scale / weighted_robust_scale of the first pass's rows at delta = inf and is then held: a scale taken again
    from the weighted rows shrinks with the weights, and the iteration degrades from the third pass on.  Returns (the final n weight
    intermediates -- the caller closes them --, one dict per pass: delta, coverage, inlier_mass, rejected_share (n,) = sum REJ /
    sum HITS per view, 0 where a view has no hits).  Every metric and every intermediate weight set made here is closed."""
    data = list(data)
    n = len(data)
    if int(passes) < 1:
        raise ValueError("passes must be at least 1")
    if weights is not None and len(weights) != n:
        raise ValueError("weights: one intermediate per view, or None")
    current, owned = (None if weights is None else list(weights)), False
    delta, records = None, []
    try:
        for _ in range(int(passes)):
            m = MetricRadonIntermediate(ctx, Ps, data if current is None else data + current).setSampling(sampling)
            try:
                if current is None:
                    delta = robust_scale(m.evaluate_robust(loss, float("inf"), want_pairs=True)[2], k)
                    _, mass, hits, rej = m.evaluate_robust_map(loss, delta)
                    coverage, new = 1.0, m.robust_map_weights(min_hits, gain)
                else:
                    if delta is None:
                        delta = weighted_robust_scale(m.evaluate_weighted_robust(loss, float("inf"), want_pairs=True)[3], k)
                    _, coverage, mass, hits, rej = m.evaluate_weighted_robust_map(loss, delta)
                    new = m.weighted_robust_map_weights(min_hits, gain)
            finally:
                m.close()
            if owned:
                for w in current:
                    w.close()
            current, owned = new, True
            h, r = hits.astype(np.float64).sum(axis=(1, 2)), rej.astype(np.float64).sum(axis=(1, 2))
            records.append(dict(delta=delta, coverage=coverage, inlier_mass=mass, rejected_share=np.where(h > 0, r / np.where(h > 0, h, 1.0), 0.0)))
    except BaseException:
        if owned:
            for w in current:
                w.close()
        raise
    return current, records


def refine_variances(ctx, Ps, data, variances, floor, loss=_lib.LOSS_TRUNCATED, k=2.0, passes=2, min_hits=1.0, gain=1.0, max_factor=1e4,
                     sampling="auto"):
    """Variance fields from the robust loss in sigma units, iterated: the loss says where it rejects, the map raises the variance
    there, and the next pass maps the metric over those variances -- after which evaluate_variance alone, with no
    loss switched on, is robust.  data: the n Radon intermediates of the views Ps; variances: their n variance fields
    (variance_intermediates); floor as for evaluate_variance.  Every pass is evaluate_variance_robust_map +
    variance_robust_map_variances on a 2 n metric over the previous pass's variances.  delta = k x variance_robust_scale of the
    first pass's rows at delta = inf and is then held, as in refine_line_weights.  Returns (the final n variance intermediates --
    the caller closes them --, one dict per pass: delta, mean_weight, inlier_mass, rejected_share (n,) = sum REJ / sum HITS per
    view, 0 where a view has no hits).  Every metric and every intermediate field made here is closed; `variances` is not."""
    data, current, owned = list(data), list(variances), False
    n = len(data)
    if int(passes) < 1:
        raise ValueError("passes must be at least 1")
    if len(current) != n:
        raise ValueError("variances: one intermediate per view")
    delta, records = None, []
    try:
        for _ in range(int(passes)):
            m = MetricRadonIntermediate(ctx, Ps, data + current).setSampling(sampling)
            try:
                if delta is None:
                    delta = variance_robust_scale(m.evaluate_variance_robust(loss, float("inf"), floor, want_pairs=True)[3], k)
                _, mean_weight, mass, hits, rej = m.evaluate_variance_robust_map(loss, delta, floor)
                new = m.variance_robust_map_variances(floor, min_hits, gain, max_factor)
            finally:
                m.close()
            if owned:
                for v in current:
                    v.close()
            current, owned = new, True
            h, r = hits.astype(np.float64).sum(axis=(1, 2)), rej.astype(np.float64).sum(axis=(1, 2))
            records.append(dict(delta=delta, mean_weight=mean_weight, inlier_mass=mass,
                                rejected_share=np.where(h > 0, r / np.where(h > 0, h, 1.0), 0.0)))
    except BaseException:
        if owned:
            for v in current:
                v.close()
        raise
    return current, records


def _line_weights_config(zero_at_px, guard_bins, dilate_px):
    cfg = _lib.LineWeightsConfig()
    _lib.lib().ecc_line_weights_defaults(C.byref(cfg))
    cfg.zero_at_px, cfg.guard_bins, cfg.dilate_px = float(zero_at_px), int(guard_bins), int(dilate_px)
    return cfg


def line_weights_device(ctx, flagged, size_alpha, size_t, zero_at_px=1.0, guard_bins=1, dilate_px=0, out=None):
    """line_weights without the host round trip (ecc_radon_line_weights / ecc_radon_line_weights_into): the flagged
    image is dilated by dilate_px pixels (the maximum over the (2 dilate_px + 1)^2 square, edges clamped; 0: not at all), transformed
    by the Radon kernel, clipped and put through the guard minimum on the device.  Bit-identical to line_weights on the dilated
    image.  flagged: (n_v, n_u) or (n, n_v, n_u) float32, numpy on the host or torch on ctx's device, as compute_batch accepts; a 2-D
    input returns one RadonIntermediate, a stack a list.  out: a torch (n, slab_floats(size_alpha, size_t)) float32 tensor on ctx's
    device selects the asynchronous form for caller-owned slabs (flagged must be on the device too) and the returned handles alias
    it, as compute_into's do -- a tracker whose mask moves follows it with metric.refreshRadonIntermediates(n_views + i, 1).
    0 <= dilate_px <= 16, 0 <= guard_bins <= 8, zero_at_px finite and positive."""
    cfg = _line_weights_config(zero_at_px, guard_bins, dilate_px)
    if _is_torch(flagged):
        import torch
        assert flagged.dtype == torch.float32 and flagged.is_contiguous() and flagged.is_cuda
        stack, on_dev = flagged, 1
    else:
        stack, on_dev = np.ascontiguousarray(flagged, np.float32), 0
    if len(stack.shape) not in (2, 3):
        raise ValueError("flagged must be (n_v, n_u) or (n, n_v, n_u)")
    single = len(stack.shape) == 2
    if single:
        stack = stack[None]
    n, n_v, n_u = (int(v) for v in stack.shape)
    ptr = stack.data_ptr() if on_dev else stack.ctypes.data
    if out is not None:
        if not on_dev:
            raise ValueError("out= needs flagged on the device")
        assert out.is_contiguous() and out.is_cuda and tuple(out.shape) == (n, slab_floats(size_alpha, size_t))
        check(_lib.lib().ecc_radon_line_weights_into(ctx._h, C.c_void_p(ptr), n, n_u, n_v, size_alpha, size_t, C.byref(cfg),
                                                     C.c_void_p(out.data_ptr())))
        made = [RadonIntermediate.wrap_device(ctx, out[k], size_alpha, size_t, n_u, n_v, FILTER_NONE) for k in range(n)]
    else:
        hs = (C.c_void_p * n)()
        check(_lib.lib().ecc_radon_line_weights(ctx._h, C.c_void_p(ptr), on_dev, n, n_u, n_v, size_alpha, size_t, C.byref(cfg), hs))
        if on_dev:
            ctx.synchronize()  # the input tensor may be freed by the caller right after
        made = [RadonIntermediate(ctx, C.c_void_p(h)) for h in hs]
    return made[0] if single else made


def view_hessian_value(H, a):
    """a^T H a in float64: the metric of the per-view coefficients a, (K, n) or flat in the order c * n + i, under the matrix of
    MetricRadonIntermediate.evaluate_view_hessian."""
    H = np.asarray(H, np.float64)
    a = np.asarray(a, np.float64).reshape(-1)
    if H.ndim != 2 or H.shape != (len(a), len(a)):
        raise ValueError("H must be (n K, n K) and a hold n K coefficients")
    return float(a @ (H @ a))


def view_hessian_minimizer(H, start, free):
    """The minimiser of a^T H a over the free coefficients, the others kept at `start`: with F the free and X the fixed coordinates,
    H[F, F] a_F = -H[F, X] a_X (one dense numpy.linalg.solve; H from MetricRadonIntermediate.evaluate_view_hessian).  start: (K, n)
    coefficients; free: (K, n) boolean mask, as for minimize_view_coefficients.  Returns (a, a^T H a), a (K, n) float64 with the fixed
    coefficients' bits.  Raises numpy.linalg.LinAlgError when H[F, F] is not positive definite -- the form has no minimum there."""
    H = np.asarray(H, np.float64)
    a = np.array(start, np.float64)
    mask = np.asarray(free, bool)
    if a.ndim != 2 or mask.shape != a.shape or H.shape != (a.size, a.size):
        raise ValueError("start and free must be (K, n_views) and H (n K, n K)")
    F = mask.reshape(-1)
    if F.any():
        flat = a.reshape(-1)  # (a view: a is contiguous)
        HFF = 0.5 * (H[np.ix_(F, F)] + H[np.ix_(F, F)].T)
        np.linalg.cholesky(HFF)  # raises LinAlgError unless positive definite
        flat[F] = np.linalg.solve(HFF, -0.5 * (H[np.ix_(F, ~F)] + H[np.ix_(~F, F)].T) @ flat[~F])
    return a, view_hessian_value(H, a)
