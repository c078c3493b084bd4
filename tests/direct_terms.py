"""MetricDirect's lines and line integrals, stated a second time (plain helper module, imported like geometry_catalog and
channel_terms; numpy only, no GPU).

The C oracle (oracle/ecc_oracle.c, eccor_direct_pair) is what the device is compared with; this module is what the oracle is
compared with (tests/test_direct_lines_oracle.py), in two halves that share no code with it:

  line_integral_f32   the reference's derivative-form line integral (ref: EpipolarConsistencyDirect.cu:31-125) in numpy
                      float32, operation for operation and vectorised over lines: every intermediate is a float32 array, numpy
                      fuses nothing, so the bits are those of the unfused C statement.  `clip_f32` is its first half (origin,
                      direction, clipped parameter range, the `inside` test) and is what the GPU tests use to tell lines that
                      miss the detector from lines whose integral is 0.
  lines_f64           the kappa grid and the two epipolar lines per plane angle from geometry: source positions as null vectors
                      of P, the baseline through them, the plane through the baseline and the origin, the plane through the
                      baseline perpendicular to it, and the image line whose back-projected plane (the combination of P's rows
                      with the line's coefficients) is the epipolar plane.  float64 throughout; nothing is rounded to float32
                      but the plane angles, which are float32 by definition (ref: EpipolarConsistencyDirect.cpp:113-117).

`textured` is the image recipe of tests/test_gpu_direct_lines.py: the sphere phantoms leave most of a detector at exactly 0,
where a wrong tap reads 0 as well; the added texture is nowhere 0 and nowhere locally constant.
"""
import numpy as np

f32 = np.float32
STEP = f32(0.4)
HALF = f32(0.5)


def textured(imgs, seed=3):
    """imgs (n, n_v, n_u) + 0.05 max (1 + sin(0.11 x + 0.07 y) cos(0.05 x - 0.13 y)) + uniform(0, 0.02 max) noise from
    default_rng(seed); max is the largest pixel of the whole stack.  float32, C-contiguous."""
    imgs = np.asarray(imgs, np.float64)
    n, n_v, n_u = imgs.shape
    top = float(imgs.max())
    y, x = np.mgrid[0:n_v, 0:n_u].astype(np.float64)
    wave = 0.05 * top * (1.0 + np.sin(0.11 * x + 0.07 * y) * np.cos(0.05 * x - 0.13 * y))
    noise = np.random.default_rng(seed).uniform(0.0, 0.02 * top, size=imgs.shape)
    return np.ascontiguousarray(imgs + wave[None] + noise, np.float32)


# ---- the float32 line integral ------------------------------------------------------------------------------------

def _tex2d(img, x, y):
    """The un-normalised bilinear rule with clamp addressing (oracle.tex2d is the normative statement), float32 arrays."""
    n_v, n_u = img.shape
    xb, yb = x - HALF, y - HALF
    fi, fj = np.floor(xb), np.floor(yb)
    fx, fy = xb - fi, yb - fj
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    i0, i1 = np.clip(i, 0, n_u - 1), np.clip(i + 1, 0, n_u - 1)
    j0, j1 = np.clip(j, 0, n_v - 1), np.clip(j + 1, 0, n_v - 1)
    one = f32(1)
    r0 = (one - fx) * img[j0, i0] + fx * img[j0, i1]
    r1 = (one - fx) * img[j1, i0] + fx * img[j1, i1]
    return (one - fy) * r0 + fy * r1


def clip_f32(lines, n_u, n_v):
    """lines (n, 3) float32 in Hessian normal form -> dict(o0, o1, d0, d1, t_min, t_max, inside): the closest point to the pixel
    origin, the direction, the parameter range inside [1, n - 1] on both axes and the reference's test that the range's
    start lies on the detector (a line failing it integrates to exactly 0)."""
    l = np.ascontiguousarray(lines, f32).reshape(-1, 3)
    l0, l1, l2 = l[:, 0], l[:, 1], l[:, 2]
    with np.errstate(all="ignore"):
        o0, o1 = -l2 * l0, -l2 * l1
        d0, d1 = l1, -l0
        ts = [(f32(1) - o0) / d0, (f32(n_u - 1) - o0) / d0, (f32(1) - o1) / d1, (f32(n_v - 1) - o1) / d1]
        flat0 = (d0 * d0).astype(np.float64) < 1e-12
        flat1 = (d1 * d1).astype(np.float64) < 1e-12
        big = f32(1e10)
        ts[0], ts[1] = np.where(flat0, -big, ts[0]), np.where(flat0, big, ts[1])
        ts[2], ts[3] = np.where(flat1, -big, ts[2]), np.where(flat1, big, ts[3])
        for _ in range(3):  # the reference's three bubble passes, comparison for comparison (a NaN never swaps)
            for i in range(3):
                swap = ts[i] > ts[i + 1]
                ts[i], ts[i + 1] = np.where(swap, ts[i + 1], ts[i]), np.where(swap, ts[i], ts[i + 1])
        t_min, t_max = ts[1], ts[2]
        u, v = o0 + t_min * d0, o1 + t_min * d1
        inside = (u <= f32(n_u)) & (v <= f32(n_v)) & (u >= f32(0)) & (v >= f32(0))
    return dict(o0=o0, o1=o1, d0=d0, d1=d1, t_min=t_min, t_max=t_max, inside=inside)


def line_integral_f32(img, line):
    """The derivative-form integral of img (n_v, n_u) along each of `line` (n, 3) or (3,): two samples half a pixel to either
    side of the line every 0.4 px, each multiplied by the step before it is added, sump - summ.  float32, the bits of
    oracle.direct_pair's samples for the same lines."""
    img = np.ascontiguousarray(img, f32)
    n_v, n_u = img.shape
    l = np.ascontiguousarray(line, f32).reshape(-1, 3)
    c = clip_f32(l, n_u, n_v)
    o0, o1 = c["o0"] + HALF, c["o1"] + HALF
    d0, d1 = c["d0"], c["d1"]
    h0, h1 = l[:, 0] * HALF, l[:, 1] * HALF
    sump = np.zeros(len(l), f32)
    summ = np.zeros(len(l), f32)
    t = c["t_min"].copy()
    with np.errstate(all="ignore"):
        run = c["inside"] & (t <= c["t_max"])
        while run.any():
            k = np.nonzero(run)[0]
            u, v = o0[k] + t[k] * d0[k], o1[k] + t[k] * d1[k]
            sump[k] = sump[k] + _tex2d(img, u + h0[k], v + h1[k]) * STEP
            summ[k] = summ[k] + _tex2d(img, u - h0[k], v - h1[k]) * STEP
            t[k] = t[k] + STEP
            run[k] = t[k] <= c["t_max"][k]
    out = sump - summ
    return out if np.ndim(line) == 2 else out[0]


# ---- the lines in float64 -------------------------------------------------------------------------------------------

def source_position(P):
    """The Euclidean source position: the null vector of P (smallest right singular vector), dehomogenised."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    C = np.linalg.svd(P / np.linalg.norm(P))[2][3]
    return C[:3] / C[3]


def plane_range(P0, P1, n_u, n_v, radius, dkappa=0.0):
    """(kappa_max, dkappa, n_lines): half the angular range of the epipolar planes that meet a sphere of `radius` mm about the
    origin (pi/2 when the baseline passes through it; ref: estimateAngularRange, EpipolarConsistency.cpp:49-59), the plane
    step (given, or half the range's share of a detector diagonal in pixels) and the number of planes."""
    a, b = source_position(P0), source_position(P1)
    dist = np.linalg.norm(np.cross(a, b)) / np.linalg.norm(a - b)  # distance of the baseline from the origin
    k_max = 0.5 * np.pi if dist <= radius else abs(np.arcsin(radius / dist))
    if dkappa <= 0:
        dkappa = 0.5 * (k_max - -k_max) / np.sqrt(float(n_u * n_u + n_v * n_v))
    nl = (k_max - -k_max) / dkappa
    return k_max, dkappa, (int(nl) if nl >= 0 else 0)


def lines_f64(P0, P1, kappas, n_u, n_v, radius, dkappa=0.0):
    """(kappas float32 (n,), lines float64 (n, 6)): the plane angles (the automatic grid -kappa_max + k dkappa rounded to float32
    when `kappas` is None) and, per angle, the normalised line (l0, l1, l2 with l0^2 + l1^2 = 1) of that epipolar plane in image 0
    and in image 1.

    The plane at angle kappa is cos(kappa) E0 + sin(kappa) E90 with E0 the plane through both sources and the origin (unit
    normal along C0 x C1) and E90 the plane through both sources perpendicular to it (unit normal along (C0 x C1) x (C0 - C1)).  Its
    image in P is the line l with P^T l = E: a plane through the source is a combination of P's rows, and the coefficients are
    the line.  Solved as the consistent 4 x 3 system it is, with the rows scaled to unit length first."""
    a, b = source_position(P0), source_position(P1)
    k_max, dkappa, n = plane_range(P0, P1, n_u, n_v, radius, dkappa)
    if kappas is None:
        kappas = (-k_max + dkappa * np.arange(n, dtype=np.float64)).astype(f32)
    kappas = np.ascontiguousarray(kappas, f32).reshape(-1)
    n0 = np.cross(a, b)
    n0 /= np.linalg.norm(n0)
    n90 = np.cross(n0, a - b)
    n90 /= np.linalg.norm(n90)
    E0 = np.append(n0, 0.0)
    E90 = np.append(n90, -n90 @ a)
    k = kappas.astype(np.float64)
    E = np.cos(k)[:, None] * E0[None] + np.sin(k)[:, None] * E90[None]  # (n, 4)
    out = np.empty((len(k), 6), np.float64)
    for which, P in enumerate((P0, P1)):
        P = np.asarray(P, np.float64).reshape(3, 4)
        scale = np.linalg.norm(P, axis=1)
        l = np.linalg.lstsq((P / scale[:, None]).T, E.T, rcond=None)[0].T / scale[None]  # (n, 3)
        out[:, 3 * which:3 * which + 3] = l / np.hypot(l[:, 0], l[:, 1])[:, None]
    return kappas, out


def line_difference_in_bars(got, want):
    """|got - want| per component of two (n, 6) line arrays, in units of the bar on it: both sides form the line in float64 and
    round once to float32, so a float64 discrepancy moves a component to the neighbouring float32 at most (np.spacing of the
    larger magnitude); components that cancel to near 0 get 1e-12 max(1, |l2|) instead.  `want` may be float64 (a line not yet
    rounded).  A value above 1 is outside the bar."""
    got, want = np.asarray(got), np.asarray(want)
    big = np.maximum(np.abs(got).astype(f32), np.abs(want).astype(f32))
    l2 = np.abs(np.asarray(want, np.float64).reshape(-1, 2, 3)[:, :, 2])
    absolute = np.repeat(1e-12 * np.maximum(1.0, l2), 3, axis=1).reshape(want.shape)
    bar = np.maximum(np.spacing(big).astype(np.float64), absolute)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / bar
