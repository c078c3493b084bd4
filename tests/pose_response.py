"""The oracle's response of the metric to a moved view (plain helper module, imported like geometry_catalog).

An optimiser compares the metric at nearby poses.  Between two poses that move the same view v, every pair without v keeps its
value bit for bit, so the difference of the two means is the difference of the float64 sums of the n - 1 pairs of v.
`moved_pair_response` evaluates exactly those pairs, for many poses, in ONE index-list call of the oracle per variant: the base
matrices, then the moved matrices of the poses, with the index rows of the pairs of v pointing at pose q's matrix n + q and at the
dtrs of the base views.  Variant 0 is the normative oracle, variant 1 its float64-geometry probe (oracle.set_variant), and "x"
variant 1 with exact sampling (oracle.set_probe(EXACT_SAMPLING)): variant 1 still rounds the angle and distance to float32 and
forms the texel position and weights in float32, as the reference does, so its differences carry that rounding; "x" keeps every
sample coordinate in binary64 up to the texels.

`device_case` makes the data the GPU parity tests use: projections made on the device, Radon intermediates from the HIP kernel,
read back for the oracle.
"""
import numpy as np

DOFS = ("tx", "ty", "tz", "rx", "ry", "rz")
EXACT_SAMPLING = 128  # oracle.set_probe bit: texel position and bilinear weights in binary64
VARIANTS = ((0, 0, 0), (1, 1, 0), ("x", 1, EXACT_SAMPLING))  # (key, oracle.set_variant, oracle.set_probe)
STEPS_MM = (1.0, 0.1, 0.01, 0.001)
STEPS_RAD = (1e-3, 1e-4, 1e-5, 1e-6)


def steps(dof):
    return STEPS_MM if dof[0] == "t" else STEPS_RAD


def pose_grid(P_v, dofs=DOFS):
    """The base pose, then P_v @ rigid_transform(dof = s h) for every dof, h (steps(dof)) and s in (+1, -1): a list of
    (dof, h, s) labels ((None, 0, 0) for the base) and the moved 3x4 matrices."""
    from epipolarconsistency_amd import geometry
    P_v = np.asarray(P_v, np.float64).reshape(3, 4)
    labels, mats = [(None, 0.0, 0)], [P_v.copy()]
    for dof in dofs:
        for h in steps(dof):
            for s in (1, -1):
                labels.append((dof, h, s))
                mats.append(P_v @ geometry.rigid_transform(**{dof: s * h}))
    return labels, mats


def cells(labels, S):
    """Per (dof, h) of the grid: the central difference S(+h) - S(-h) and the second difference S(+h) - 2 S(0) + S(-h).
    S: one float64 value per pose, labels as pose_grid.  Returns {(dof, h): (D, D2)}."""
    at = {lab: k for k, lab in enumerate(labels)}
    S0 = S[at[(None, 0.0, 0)]]
    out = {}
    for dof, h, s in labels[1:]:
        if s == 1:
            p, m = S[at[(dof, h, 1)]], S[at[(dof, h, -1)]]
            out[(dof, h)] = (p - m, p - 2.0 * S0 + m)
    return out


def pairs_of_view(n, v):
    """(get_ij index, i, j) of the n - 1 pairs that contain view v, in get_ij order (i < j)."""
    import oracle
    out = []
    for q in range(n * (n - 1) // 2):
        i, j = oracle.get_ij(q, n)
        if v in (i, j):
            out.append((q, i, j))
    return np.array(out, np.int64)


def moved_pair_response(oracle_mod, Ps, dtrs, n_u, n_v, v, moved, dkappa=0.0):
    """The n - 1 pairs of view v at every pose `moved` (3x4 matrices replacing Ps[v]), variants 0 and 1 of the oracle.
    Returns dict(pairs=(n - 1, 3) get_ij index, i, j; and per variant 0 / 1: values (K, n - 1) float32, sums (K,) float64 (the
    float64 sum of the moved pairs' values), K01s (K, n - 1, 16)).  v = 0 is refused: the automatic object radius follows the first
    matrix (ref: EpipolarConsistency.cpp:76-84), so moving view 0 changes every pair -- use oracle.evaluate_all there.
    The same for "x" (variant 1, exact sampling)."""
    n = len(Ps)
    if not 0 < v < n:
        raise ValueError("moved view %d: must be in 1 .. n - 1 (view 0 sets the object radius of every pair)" % v)
    pq = pairs_of_view(n, v)
    K = len(moved)
    ext = [np.asarray(P, np.float64).reshape(3, 4) for P in Ps] + [np.asarray(P, np.float64).reshape(3, 4) for P in moved]
    idx = np.empty((K, n - 1, 4), np.int32)
    for k in range(K):
        for r, (_, i, j) in enumerate(pq):
            idx[k, r] = (n + k if i == v else i, n + k if j == v else j, i, j)
    out = dict(pairs=pq)
    try:
        for key, var, probe in VARIANTS:
            oracle_mod.set_variant(var)
            oracle_mod.set_probe(probe)
            res = oracle_mod.evaluate_pairs(ext, dtrs, n_u, n_v, idx.reshape(-1, 4), dkappa=dkappa, want_K01=True)
            vals = res["pairs"].reshape(K, n - 1)
            out[key] = dict(values=vals, sums=vals.astype(np.float64).sum(axis=1), K01s=res["K01s"].reshape(K, n - 1, 16))
    finally:
        oracle_mod.set_probe(0)
        oracle_mod.set_variant(0)
    return out


def all_pairs_response(oracle_mod, Ps, dtrs, n_u, n_v, v, moved, dkappa=0.0):
    """moved_pair_response's form for any view (view 0 included): evaluate_all on every pose's full matrices.  pairs: all of them."""
    n = len(Ps)
    ij = np.array([(q,) + oracle_mod.get_ij(q, n) for q in range(n * (n - 1) // 2)], np.int64)
    out = dict(pairs=ij)
    try:
        for key, var, probe in VARIANTS:
            oracle_mod.set_variant(var)
            oracle_mod.set_probe(probe)
            vals, K01s = [], []
            for P in moved:
                full = [np.asarray(p, np.float64).reshape(3, 4) for p in Ps]
                full[v] = np.asarray(P, np.float64).reshape(3, 4)
                r = oracle_mod.evaluate_all(full, dtrs, n_u, n_v, dkappa=dkappa, want_K01=True)
                vals.append(r["pairs"])
                K01s.append(r["K01s"])
            vals = np.array(vals)
            out[key] = dict(values=vals, sums=vals.astype(np.float64).sum(axis=1), K01s=np.array(K01s))
    finally:
        oracle_mod.set_probe(0)
        oracle_mod.set_variant(0)
    return out


def kappa_samples(K01s, dkappa_user=0.0, n_u=None, n_v=None, n_t=None):
    """Number of kappa samples of each pair: the pair loops' rule in float32 (oracle or_pair, csrc/ecc_pairs_device.h kappa_step):
    kappa_k = dkappa * 0.5f + dkappa * k < kappa_max for k < k_limit, dkappa = K1[6], kappa_max = K1[7].  k_limit is the launch
    bound of ref: ...RadonIntermediate.cu:348-358 (csrc/ecc_evaluate.hip fill_pair_params)."""
    K01s = np.asarray(K01s, np.float32)
    f = np.float32
    if dkappa_user <= 0:
        step_t = f(np.sqrt(float(n_v) * n_v + float(n_u) * n_u) / n_t)
        max_num = int(f(f(n_t) * step_t) * f(2.0))
    else:
        max_num = int(f(f(3.14159265359) * f(0.5)) / f(dkappa_user))
    k_limit = (max_num + 255) // 256 * 256
    k = np.arange(k_limit, dtype=np.float32)
    dk = K01s[..., 14:15]
    kmax = K01s[..., 15:16]
    with np.errstate(invalid="ignore", over="ignore"):
        kappa = (dk * f(0.5)).astype(np.float32) + (dk * k).astype(np.float32)
        below = kappa < kmax
    # the loops stop at the first kappa >= kappa_max (kappa_k grows with k)
    return np.where(below.all(axis=-1), k_limit, np.argmin(below, axis=-1))


def device_case(gpu_ctx, Ps, n_u, n_v, n_alpha, n_t, phantom):
    """Device dtrs of the views Ps (aliasing the returned slabs) and their read-back copies: projections of `phantom` made on the
    device, Radon intermediates from the HIP kernel.  Returns slabs, dtrs, host."""
    import torch
    import epipolarconsistency_amd as E
    from epipolarconsistency_amd import synthetic
    n = len(Ps)
    dev = torch.device("cuda", gpu_ctx.device)
    slabs = torch.zeros((n, E.slab_floats(n_alpha, n_t)), dtype=torch.float32, device=dev)
    dtrs = []
    for a in range(0, n, 64):
        imgs = synthetic.projections_torch(Ps[a:a + 64], n_u, n_v, phantom, dev)
        torch.cuda.synchronize()
        dtrs += E.RadonIntermediate.compute_into(gpu_ctx, imgs, slabs[a:a + 64], n_alpha, n_t)
        gpu_ctx.synchronize()
        del imgs
    host = [d.readback() for d in dtrs]
    return slabs, dtrs, host
