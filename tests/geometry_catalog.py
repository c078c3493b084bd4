"""C-arm geometries beyond the planar short scan, for the parity tests (plain helper module, imported like conftest).

Every entry returns (Ps, n_u, n_v): float64 3x4 matrices and the detector size in pixels.  `well_posed(Ps)` is the pair mask
(get_ij order) the comparisons use: it leaves out pairs whose source positions coincide to within 1e-4 relative -- they have
no baseline and every implementation returns its own rounding noise for them (scripts/fuzz_parity.py) -- and nothing else.

  angulated       200 deg orbit whose cranial / caudal angulation varies along it (+-25 deg): the source path is not planar;
                  640x480 detector with the principal point off centre by (+40, -25) px.
  near_opposite   360 deg scan, no two views exactly 180 deg apart but many within 0.5 deg; alternate views lifted by 3 mm:
                  many pairs with kappa_max = pi/2, epipoles inside the detector, baselines that only just miss the object.
  scattered       fluoroscopy-like poses on a spherical cap (+-60 deg LAO/RAO, +-40 deg CRAN/CAUD), each with its own in-plane
                  roll, SID in 700-800 mm and SDD in 1000-1200 mm; some views repeated 1-5 mm to the side (far epipoles).
  mirrored        `angulated` with the u axis mirrored on some views (det M < 0) and the matrices multiplied by per-view
                  factors from {-1, 1e-3, 1e3}.
  rolled          200 deg planar orbit, detector rolled in its plane by up to +-80 deg per view.

The phantom (`phantom()`) lies inside every entry's field of view.
"""
import numpy as np

NAMES = ("angulated", "near_opposite", "scattered", "mirrored", "rolled")


def phantom():
    """Eight spheres within 58 mm of the origin (synthetic.sphere_phantom), inside every entry's field of view."""
    from epipolarconsistency_amd import synthetic
    return synthetic.sphere_phantom(seed=77, extent_mm=30.0, rmin=8.0, rmax=28.0)


def _view(source, n_u, n_v, pixel_mm, sdd, roll=0.0, pp_shift=(0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """P = K [R | -R C] for a source at `source` (mm) looking at the origin; detector `pixel_mm` per pixel at distance `sdd`,
    rolled by `roll` rad about the principal ray, principal point shifted by pp_shift px from the detector centre."""
    C = np.asarray(source, np.float64)
    fwd = -C / np.linalg.norm(C)
    left = np.cross(np.asarray(up, np.float64), fwd)
    left /= np.linalg.norm(left)
    upv = np.cross(fwd, left)
    cr, sr = np.cos(roll), np.sin(roll)
    ax_u, ax_v = cr * left + sr * upv, -sr * left + cr * upv
    R = np.stack([ax_u, ax_v, fwd])
    f = sdd / pixel_mm
    K = np.array([[f, 0.0, 0.5 * n_u + pp_shift[0]], [0.0, f, 0.5 * n_v + pp_shift[1]], [0.0, 0.0, 1.0]])
    P = K @ np.hstack([R, (-R @ C)[:, None]])
    return P / np.linalg.norm(P[2, :3])


def angulated(n=48):
    n_u, n_v = 640, 480
    Ps = []
    for k in range(n):
        t = k / (n - 1.0)
        theta = np.deg2rad(200.0 * t)
        phi = np.deg2rad(25.0 * np.sin(2.0 * np.pi * t + 0.3))  # cranial / caudal, +-25 deg along the orbit
        C = 750.0 * np.array([np.cos(phi) * np.cos(theta), np.sin(phi), np.cos(phi) * np.sin(theta)])
        Ps.append(_view(C, n_u, n_v, 0.62, 1100.0, pp_shift=(40.0, -25.0)))
    return Ps, n_u, n_v


def near_opposite(n=48):
    """n even; view k at 360 k / n + 0.2 sin(1.7 k) deg: opposite views differ from 180 deg by at most 0.4 deg, never by 0."""
    n_u, n_v = 512, 384
    Ps = []
    for k in range(n):
        theta = np.deg2rad(360.0 * k / n + 0.2 * np.sin(1.7 * k))
        lift = 3.0 if k % 2 else -3.0
        C = np.array([740.0 * np.cos(theta), lift, 740.0 * np.sin(theta)])
        Ps.append(_view(C, n_u, n_v, 0.8, 1150.0))
    return Ps, n_u, n_v


def scattered(n=48, seed=5):
    """n - n // 6 random poses, then n // 6 of them again with the source moved 1-5 mm sideways (perpendicular to the
    principal ray) and the same orientation."""
    n_u, n_v = 600, 500
    rng = np.random.default_rng(seed)
    n_near = n // 6
    base = []
    for _ in range(n - n_near):
        lao = np.deg2rad(rng.uniform(-60, 60))
        cran = np.deg2rad(rng.uniform(-40, 40))
        sid = rng.uniform(700, 800)
        sdd = rng.uniform(1000, 1200)
        roll = np.deg2rad(rng.uniform(-30, 30))
        C = sid * np.array([np.sin(lao) * np.cos(cran), np.sin(cran), np.cos(lao) * np.cos(cran)])
        base.append((C, sdd, roll))
    views = list(base)
    for q in range(n_near):
        C, sdd, roll = base[2 * q]
        fwd = -C / np.linalg.norm(C)
        side = np.cross(fwd, rng.normal(size=3))
        side /= np.linalg.norm(side)
        views.append((C + rng.uniform(1.0, 5.0) * side, sdd, roll, C))
    Ps = []
    for v in views:
        C, sdd, roll = v[:3]
        if len(v) == 4:  # same orientation as the view it repeats: look along that view's principal ray
            P = _view(v[3], n_u, n_v, 0.7, sdd, roll=roll)
            M = P[:, :3]
            P = np.hstack([M, (-M @ C)[:, None]])
        else:
            P = _view(C, n_u, n_v, 0.7, sdd, roll=roll)
        Ps.append(P)
    return Ps, n_u, n_v


MIRROR_FACTORS = (-1.0, 1e-3, 1e3, 1.0)


def mirrored(n=48):
    """angulated(n); every third view (k % 3 == 1) mirrored in u (u -> n_u - 1 - u), view k scaled by
    MIRROR_FACTORS[k % 4]."""
    Ps, n_u, n_v = angulated(n)
    flip = np.array([[-1.0, 0.0, n_u - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    out = []
    for k, P in enumerate(Ps):
        if k % 3 == 1:
            P = flip @ P
        out.append(P * MIRROR_FACTORS[k % 4])
    return out, n_u, n_v


def rolled(n=48, seed=9):
    n_u, n_v = 640, 480
    rng = np.random.default_rng(seed)
    rolls = np.deg2rad(rng.uniform(-80, 80, n))
    rolls[:2] = np.deg2rad([80.0, -80.0])
    Ps = []
    for k in range(n):
        theta = np.deg2rad(200.0 * k / (n - 1.0))
        C = 760.0 * np.array([np.cos(theta), 0.0, np.sin(theta)])
        Ps.append(_view(C, n_u, n_v, 0.62, 1120.0, roll=rolls[k]))
    return Ps, n_u, n_v


def make(name, n=48):
    return {"angulated": angulated, "near_opposite": near_opposite, "scattered": scattered, "mirrored": mirrored,
            "rolled": rolled}[name](n)


def source_positions(Ps):
    """Euclidean source positions (float64 null vectors of P)."""
    out = []
    for P in Ps:
        P = np.asarray(P, np.float64).reshape(3, 4)
        out.append(-np.linalg.solve(P[:, :3], P[:, 3]))
    return np.array(out)


def pair_indices(n):
    """(i, j) of every pair in the get_ij order (the order of the library's pair values and of the oracle's)."""
    import oracle
    return np.array([oracle.get_ij(q, n) for q in range(n * (n - 1) // 2)], np.int64).reshape(-1, 2)


def well_posed(Ps):
    """Pair mask (get_ij order): False where the two source positions coincide to within 1e-4 relative."""
    Cs = source_positions(Ps)
    ij = pair_indices(len(Ps))
    d = np.linalg.norm(Cs[ij[:, 0]] - Cs[ij[:, 1]], axis=1)
    return d >= 1e-4 * np.linalg.norm(Cs[ij[:, 0]], axis=1)


def epipoles(Ps):
    """(n_pairs, 2, 2): the epipole of view j in view i (px) and of view i in view j, get_ij order; inf where at infinity."""
    Cs = source_positions(Ps)
    ij = pair_indices(len(Ps))
    out = np.full((len(ij), 2, 2), np.inf)
    for q, (i, j) in enumerate(ij):
        for s, (a, b) in enumerate(((i, j), (j, i))):
            e = np.asarray(Ps[a], np.float64).reshape(3, 4) @ np.append(Cs[b], 1.0)
            if abs(e[2]) > 1e-12 * np.abs(e[:2]).max():
                out[q, s] = e[:2] / e[2]
    return out
