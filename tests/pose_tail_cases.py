"""Seeded inputs and precondition checks for the pose tail: the rigid solve (vcr_rigid_svd_f32), the ICP loop (vcr_icp_f32) and
the pose step (vcr_pose_step_f32).  Shared by tests/test_pose_tail_inputs.py (CPU: the references alone stay inside every
condition stated here) and tests/test_hip_pose_tail.py (GPU: the kernels against those references).

References: the fp32 oracle (oracle.rigid_svd, oracle.icp_forward, oracle.transform_point_cloud) and its TWIN, the same
functions on .double() copies of the same fp32 inputs.  A kernel is held to the twin by the accuracy ledger's rule
(tests/test_hip_ledger.py): no further from it than 1.5x the fp32 reference's own distance on that sample, or than D, the
largest reference-to-twin distance over the case's FAMILY (all cases of the same offset and scale) -- the reference is
sometimes lucky on one sample.

Rigid cases are batches [B, K, 3] of rows; every sample has its own cloud, rotation and translation, so a wrong batch offset
shows.  ICP cases are channels-first clouds [B, 3, N] / [B, 3, M] built by grid_pair: a jittered lattice in random order (true
neighbours in every 2048-row tile of the kernel) and a subset of it moved back by a small rigid motion.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import oracle

EPS24 = 2.0 ** -24
AXIS = (0.36, 0.48, 0.8)                       # a unit vector that is no coordinate axis
PLANE = (0.3, -0.5, 0.8)                       # normal of the rank-2 case's plane
MARGIN = 32 * EPS24                            # x P: the fp32 roundings of the expanded score in two implementations


def rotation(axis, deg):
    """Rodrigues in float64; quarter turns about a coordinate axis come out exact (entries 0 and +-1)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.radians(float(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    if np.count_nonzero(a) == 1 and float(deg) % 90 == 0:
        R = np.round(R)
    return R


# ---------------------------------------------------------------------------------------------------------------------------
# rigid solve
# ---------------------------------------------------------------------------------------------------------------------------

TWELVE = np.concatenate([s * m * np.eye(3) for m in (1.0, 2.0) for s in (1.0, -1.0)])       # +-e_i, +-2 e_i


def rigid_case(name, seed, B=33, K=300, angle=None, axes=None, noise=0.02, offset=0.0, s_scale=1.0, c_scale=1.0,
               mirror=False, flatten=None, project=False, twelve=False, stride=4):
    """src, corr [B, K, 3] fp32.  corr = c_scale * (R s + t + noise) + offset for the fp32 source s * s_scale + offset;
    angle: degrees for every sample (default: one per sample from 20..160), axes: (axis, degrees) per sample, cycled."""
    rs = np.random.RandomState(seed)
    if twelve:
        K = 12
        unit = np.broadcast_to(TWELVE, (B, 12, 3)).copy()
    else:
        unit = rs.uniform(-1, 1, (B, K, 3))
    if mirror:
        unit *= (1.0, 0.75, 0.5)               # distinct singular values: the optimum under a reflection stays unique
    if flatten is not None:
        unit[:, :, 2] *= flatten
    ang = rs.uniform(20, 160, B) if angle is None else np.full(B, float(angle))
    trans = rs.uniform(-0.5, 0.5, (B, 3))
    if twelve:
        trans = np.round(trans * 8) / 8        # with integer points: corr and its mean are exact, a quarter turn's H has exact zeros
    src = (unit * s_scale + offset).astype(np.float32)
    back = (src.astype(np.float64) - offset) / s_scale                      # what the fp32 source holds, in unit coordinates
    corr = np.empty((B, K, 3))
    for b in range(B):
        R = rotation(AXIS if axes is None else axes[b % len(axes)][0], ang[b] if axes is None else axes[b % len(axes)][1])
        if mirror:
            R = R @ np.diag([1.0, 1.0, -1.0])
        corr[b] = back[b] @ R.T + trans[b]
    if noise:
        corr += noise * rs.standard_normal((B, K, 3))
    if project:
        n = np.asarray(PLANE) / np.linalg.norm(PLANE)
        corr -= (corr @ n)[..., None] * n
    corr = (corr * c_scale + offset).astype(np.float32)
    return SimpleNamespace(name=name, src=torch.from_numpy(src), corr=torch.from_numpy(corr), stride=stride,
                           family=(float(offset), float(s_scale), float(c_scale)), tscale=float(c_scale), B=B, K=K)


def _rigid_cases():
    c, seed = [], iter(range(1000, 2000))
    add = lambda name, **kw: c.append(rigid_case(name, next(seed), **kw))
    add("base")                                                             # stride 4, column 3 = NaN like every case
    c.append(rigid_case("base_stride3", 1000, stride=3))                    # the same inputs at other row strides
    c.append(rigid_case("base_stride7", 1000, stride=7))
    for K in (3, 4, 63, 64, 65, 255, 256, 257, 511, 1000, 4099):            # around the 256-thread block, multi-trip
        add(f"K{K}", B=5, K=K)
    add("angle0", angle=0, noise=0.0)                                       # corr = src + t
    for a in (30, 90, 179.9, 180):
        add(f"angle{a}", angle=a)
    for ax, e in (("x", (1, 0, 0)), ("y", (0, 1, 0)), ("z", (0, 0, 1))):    # exact quarter turns, no noise
        add(f"quarter_{ax}", axes=[(e, 90)], noise=0.0)
    add("mirror_noisy", mirror=True)
    add("flat_source", K=8, flatten=0.01, noise=0.01)                       # eight points: both signs of det(V U^T) occur
    quarter = [((1, 0, 0), 90), ((0, 1, 0), 90), ((0, 0, 1), 90), ((0, 0, 1), 180)]
    add("twelve_points", twelve=True, noise=0.0,                            # H = c R^T: three equal singular values
        axes=quarter + [(AXIS, a) for a in (0, 17, 70, 133, 180)])
    add("rank2_tilted", project=True)
    for off in (10, 100, 1000):
        add(f"offset{off}", offset=off)
    add("scale1e-4", s_scale=1e-4, c_scale=1e-4)
    add("scale1e4", s_scale=1e4, c_scale=1e4)
    add("scale_mixed", s_scale=1e-3, c_scale=1e3)
    for s in ("1e-8", "1e-10", "1e-15"):                                    # the absolute skip threshold of the sweeps
        add(f"small{s}", s_scale=float(s), c_scale=float(s))
    return c


RIGID_CASES = _rigid_cases()
RIGID = {c.name: c for c in RIGID_CASES}
assert len(RIGID) == len(RIGID_CASES)


@functools.lru_cache(maxsize=None)
def rigid_reference(name):
    """fp32 oracle and twin of a rigid case, and what the assertions need from the twin's covariance: per sample
    opt = s1 + s2 + d s3 (the largest tr(R H64) any rotation reaches), s1, margin = (s2 + d s3) / s1, d = sign det(V U^T);
    the reference's distances to the twin d32_R, d32_t (over the cloud scale) and d32_H."""
    c = RIGID[name]
    s, k = c.src.transpose(1, 2).contiguous(), c.corr.transpose(1, 2).contiguous()
    out = {}
    for tag, cast in (("32", lambda x: x), ("64", lambda x: x.double())):
        cfg = oracle.OracleConfig(record={})
        R, t = oracle.rigid_svd(cast(s), cast(k), cfg)
        out["R" + tag], out["t" + tag], out["H" + tag] = R.double().numpy(), t.double().numpy(), cfg.record["H"].double().numpy()
    U, S, Vt = np.linalg.svd(out["H64"])
    d = np.sign(np.linalg.det(np.swapaxes(U @ Vt, 1, 2)))                   # det(V U^T)
    out["d"], out["s1"] = d, S[:, 0]
    out["opt"] = S[:, 0] + S[:, 1] + d * S[:, 2]
    out["margin"] = (S[:, 1] + d * S[:, 2]) / S[:, 0]
    out["d32_R"] = np.abs(out["R32"] - out["R64"]).max(axis=(1, 2))
    out["d32_t"] = np.abs(out["t32"] - out["t64"]).max(axis=1) / c.tscale
    out["d32_H"] = np.abs(out["H32"] - out["H64"]).max(axis=(1, 2))
    return out


WELL = 1e-3                                    # rule (c) holds a case whose every sample has s2 + d s3 >= WELL * s1
MAY_BE_ILL = ("twelve_points", "flat_source")  # no other case may miss that (test_pose_tail_inputs.py)


def well_determined(name):
    return bool(rigid_reference(name)["margin"].min() >= WELL)


@functools.lru_cache(maxsize=None)
def rigid_family_floor(family):
    """D of rule (c) for R, t and H: the largest fp32-reference-to-twin distance over the well-determined cases of a family."""
    refs = [rigid_reference(c.name) for c in RIGID_CASES if c.family == family and well_determined(c.name)]
    return tuple(max(float(r[k].max()) for r in refs) for k in ("d32_R", "d32_t", "d32_H"))


def within_ledger_rule(hip, ref32, floor):
    """Rule (c), per sample: hip <= max(1.5 x the reference's own distance, D)."""
    return np.all(np.asarray(hip) <= np.maximum(1.5 * np.asarray(ref32), floor))


# ---------------------------------------------------------------------------------------------------------------------------
# ICP
# ---------------------------------------------------------------------------------------------------------------------------

def grid_pair(g, seed, N, degs, shift=0.03, noise=0.003):
    """One pair per entry of degs.  Target: the g^3 lattice on [-1, 1]^3, each point jittered by +-0.15/g per axis, in random
    order.  Source: N of its points (no repeats) moved BACK by a rotation of degs[b] degrees about AXIS and a translation of
    length <= shift * sqrt(3), plus N(0, noise).  -> src [B, 3, N], tgt [B, 3, g^3], fp32, channels first."""
    rs = np.random.RandomState(seed)
    line = -1 + (2 * np.arange(g) + 1) / g
    lat = np.stack(np.meshgrid(line, line, line, indexing="ij"), -1).reshape(-1, 3)
    src, tgt = [], []
    for deg in degs:
        pts = (lat + rs.uniform(-0.15 / g, 0.15 / g, lat.shape))[rs.permutation(len(lat))]
        R, t = rotation(AXIS, deg), rs.uniform(-shift, shift, 3) * (deg != 0)
        own = (pts[rs.choice(len(pts), N, replace=False)] - t) @ R          # R^T (p - t)
        if noise:
            own = own + noise * rs.standard_normal(own.shape)
        src.append(own.T)
        tgt.append(pts.T)
    f = lambda x: torch.from_numpy(np.stack(x).astype(np.float32))
    return f(src), f(tgt)


def _one_target(seed, B, N):
    """Every source point has the same candidate.  Its coordinates are multiples of 1/8: the fp32 mean of N copies is then
    the point itself, the centred correspondences and H are exactly zero in the reference too, and its R is I (with other
    coordinates the reference's mean is off by an ulp and its R is whatever LAPACK makes of that rounding noise)."""
    rs = np.random.RandomState(seed)
    f = lambda x: torch.from_numpy(x.astype(np.float32))
    return f(rs.uniform(-1, 1, (B, 3, N))), f(rs.randint(-8, 9, (B, 3, 1)) / 8.0)


# (builder, tolerance, max_iterations); the seeds are the first ones under which both preconditions hold
# (test_pose_tail_inputs.py asserts them)
ICP_SPECS = {
    "I1": (lambda: grid_pair(13, 0, 300, (6, 4, 5)), 1e-5, 30),             # two tiles, ragged second block, stops early
    "I2": (lambda: grid_pair(13, 0, 300, (6, 4, 5)), 1e-3, 30),             # the default tolerance: an earlier stop
    "I3": (lambda: grid_pair(17, 1, 513, (3, 2)), 0.0, 6),                  # three tiles, one live lane, never converges
    "I4": (lambda: grid_pair(5, 0, 77, (4, 3, 2, 5, 1), shift=0.02), 1e-5, 30),      # one partial block, M < 256
    "I5": (lambda: grid_pair(6, 0, 100, (0, 0), noise=0.0), 1e-3, 30),      # an exact subset: one iteration
    "I6": (lambda: grid_pair(13, 0, 300, (6, 4, 5)), 1e-5, 1),              # exactly one step
    "I7": (lambda: grid_pair(13, 2, 150, (0, 6)), 1e-5, 30),                # pair 0 aligned, pair 1 displaced
    "I8": (lambda: _one_target(3, 2, 50), 1e-3, 10),                        # one candidate: H = 0, R = I
}


@functools.lru_cache(maxsize=None)
def icp_case(name):
    build, tol, max_it = ICP_SPECS[name]
    src, tgt = build()
    return SimpleNamespace(name=name, src=src, tgt=tgt, tol=tol, max_it=max_it, B=src.shape[0], N=src.shape[2], M=tgt.shape[2])


def icp_run(src, tgt, max_it, tol):
    """oracle.icp_forward in the dtype of its inputs -> (final, R, t, R_ba, t_ba, error trace)."""
    trace = []
    _, fin, R, t, Rb, tb = oracle.icp_forward(src, tgt, max_iterations=max_it, tolerance=tol, trace=trace)
    return fin, R, t, Rb, tb, trace


@functools.lru_cache(maxsize=None)
def icp_reference(name):
    """fp32 oracle and twin of an ICP case as float64 numpy, the iteration counts, and the reference's distances to the twin."""
    c = icp_case(name)
    r32, r64 = icp_run(c.src, c.tgt, c.max_it, c.tol), icp_run(c.src.double(), c.tgt.double(), c.max_it, c.tol)
    out = {"iters32": len(r32[5]), "iters64": len(r64[5])}
    for tag, r in (("32", r32), ("64", r64)):
        for key, v in zip(("final", "R", "t", "R_ba", "t_ba"), r):
            out[key + tag] = v.double().numpy()
    out["d32_R"] = np.abs(out["R32"] - out["R64"]).max(axis=(1, 2))
    out["d32_t"] = np.abs(out["t32"] - out["t64"]).max(axis=1)
    return out


def icp_floor():
    """D of rule (c) over the ICP cases (R, t)."""
    refs = [icp_reference(n) for n in ICP_SPECS]
    return tuple(max(float(r[k].max()) for r in refs) for k in ("d32_R", "d32_t"))


def icp_preconditions(src, tgt, max_it, tol):
    """The ICP loop restated from the oracle's own pieces, recording what the oracle does not: per iteration the smallest gap
    between a source point's best and second-best score, and how far |prev - err| is from the tolerance.
    -> (error trace, smallest gap, smallest stop margin, P = the largest squared norm over both clouds).
    A tolerance of 0 has no stop margin: |x| < 0 is false whatever the rounding."""
    cur, prev, errs, gap, stop = src, 0, [], float("inf"), float("inf")
    P = float(max((src ** 2).sum(1).max(), (tgt ** 2).sum(1).max()))
    for _ in range(max_it):
        score = oracle.neg_sqdist_head(cur, tgt)
        if tgt.shape[2] > 1:
            top = score.topk(k=2, dim=-1).values
            gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
        err, corr = oracle.icp_nearest(cur, tgt)
        R, t = oracle.rigid_svd(cur, corr)
        cur = oracle.transform_point_cloud(cur, R, t)
        errs.append(float(err))
        if tol > 0:
            stop = min(stop, abs(abs(float(prev - err)) - tol))
        if torch.abs(prev - err) < tol:
            break
        prev = err
    return errs, gap, stop, P


# ---------------------------------------------------------------------------------------------------------------------------
# pose step
# ---------------------------------------------------------------------------------------------------------------------------

POSE_SHAPES = [(B, N) for B in (1, 33) for N in (1, 63, 64, 65, 257, 1000)]


def pose_inputs(B, N):
    """Two poses per sample (fp32 roundings of rotations about random axes, translations up to 1e3) and a cloud [B, 3, N]."""
    rs = np.random.RandomState(7000 + 1000 * B + N)
    rots = lambda: np.stack([rotation(rs.standard_normal(3), rs.uniform(0, 180)) for _ in range(B)])
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return SimpleNamespace(R1=f(rots()), t1=f(rs.uniform(-1e3, 1e3, (B, 3))), R2=f(rots()), t2=f(rs.uniform(-1e3, 1e3, (B, 3))),
                           cloud=f(rs.uniform(-1, 1, (B, 3, N))))
