"""Clouds far from the origin relative to their extent (metric LiDAR, map coordinates): the recipes of the registration
stack's tests moved there, shared by tests/test_far_cpu.py and tests/test_hip_far.py.  numpy only.

`translated` moves a recipe of refine_restated.batch / gicp_restated.batch / match_restated.planted / match_restated.surface by
c and carries its poses along; `gridded` puts a recipe's coordinates on the 2^-12 grid, on which every translation by an
offset of the same grid is EXACT in fp32 (`is_exact` checks it, nothing assumes it) -- so a kernel that works from coordinate
differences returns the same bits before and after; `at_cloud_error` measures a pose where the cloud is."""
import numpy as np

F32 = np.float32
F64 = np.float64
GRID = 2.0 ** -12
MODERATE = (16.0, -8.0, 4.0)
FAR_OFFSETS = ((128.0, -64.0, 32.0), (1024.0, -512.0, 256.0 + 5 * GRID))
OFFSETS = (MODERATE,) + FAR_OFFSETS
LIMIT = 2048.0                                              # |x + c| stays below: 11 + 12 bits, an fp32 significand


def _pose(R, t, c, dtype):
    """t + c - R c in float64, rounded once to dtype: x -> R x + t in a frame moved by c (both clouds)."""
    R64, t64 = np.asarray(R).astype(F64), np.asarray(t).astype(F64)
    return (t64 + c - np.einsum("...ij,j->...i", R64, c)).astype(dtype)


def translated(case, c):
    """A recipe dict (with or without a leading batch axis) -> the same with src + c and tgt + c, computed in float64 and
    rounded to fp32, the planted pose (R, t: float64) and the start (R0, t0: fp32) mapped by t + c - R c in float64.  Normals,
    corr, twin and everything else stay as they are.  The arrays are read-only."""
    c = np.asarray(c, F64)
    out = dict(case)
    for k in ("src", "tgt"):
        out[k] = np.ascontiguousarray((np.asarray(case[k]).astype(F64) + c[:, None]).astype(F32))
    out["t"] = _pose(case["R"], case["t"], c, F64)
    if "t0" in case:
        out["t0"] = _pose(case["R0"], case["t0"], c, F32)
    for k in ("src", "tgt", "t", "t0"):
        if k in out:
            out[k].setflags(write=False)
    return out


def moved_cloud(xyz, c):
    """xyz [..., 3, N] fp32 -> fp32(xyz + c), the sum in float64."""
    return np.ascontiguousarray((np.asarray(xyz).astype(F64) + np.asarray(c, F64)[:, None]).astype(F32))


def on_grid(xyz):
    """Every finite coordinate rounded to the nearest multiple of 2^-12 (non-finite ones stay)."""
    x = np.asarray(xyz, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), (np.round(x.astype(F64) / GRID) * GRID).astype(F32), x)


def gridded(case):
    """A recipe dict -> the same with src and tgt on the grid (the poses stay: the partners are then off by up to 2^-13 a
    coordinate, which the translation tests -- a run against the same run moved -- do not mind)."""
    out = dict(case)
    for k in ("src", "tgt"):
        out[k] = np.ascontiguousarray(on_grid(case[k]))
        out[k].setflags(write=False)
    return out


def is_exact(xyz, c):
    """True where the translation of xyz (fp32) by c is exact both ways: fp32(x + c) == x + c in float64, fp32(fp32(x + c) - c)
    == x, and |x + c| < 2048 -- over the finite coordinates (there must be some)."""
    x = np.asarray(xyz, F32)
    c = np.asarray(c, F64)
    ok = np.isfinite(x)
    far = moved_cloud(x, c)
    exact = x.astype(F64) + c[:, None]
    back = (far.astype(F64) - c[:, None]).astype(F32)
    c32 = c.astype(F32)
    in_fp32 = far - c32[:, None]                            # the subtraction as the device makes it
    return bool(ok.any() and (c32.astype(F64) == c).all() and (far.astype(F64)[ok] == exact[ok]).all()
                and (np.abs(exact[ok]) < LIMIT).all() and np.array_equal(back[ok], x[ok]) and np.array_equal(in_fp32[ok], x[ok]))


def at_cloud_error(R, t, R_true, t_true, pts):
    """max |R p + t - (R_true p + t_true)| in float64 over pts [3,n]: the largest displacement of a point from where the true
    pose puts it.  (|t - t_true| is measured at the origin: at a distance r it is the rotation error times r, and says
    nothing about the fit.)"""
    p = np.asarray(pts).astype(F64)
    a = np.asarray(R).astype(F64) @ p + np.asarray(t).astype(F64)[:, None]
    b = np.asarray(R_true).astype(F64) @ p + np.asarray(t_true).astype(F64)[:, None]
    return float(np.abs(a - b).max())


def ulp_at(*arrays):
    """One fp32 unit in the last place at the largest finite |coordinate| of the arrays."""
    top = max(float(np.abs(a[np.isfinite(a)]).max()) for a in map(np.asarray, arrays))
    return float(np.spacing(F32(top)))


def centre_of(xyz):
    """centred()'s default on the CPU: per axis the mean of the finite coordinates, summed in float64, rounded to fp32."""
    x = np.asarray(xyz, F32)
    ok = np.isfinite(x)
    return (np.where(ok, x, 0).astype(F64).sum(-1) / np.maximum(ok.sum(-1), 1)).astype(F32)


def centred_pose(R, t, c_src, c_tgt):
    """uncentred -> centred frames: t + R c_src - c_tgt in float64."""
    R, t = np.asarray(R).astype(F64), np.asarray(t).astype(F64)
    return R, t + R @ np.asarray(c_src).astype(F64) - np.asarray(c_tgt).astype(F64)


def uncentred_pose(R, t, c_src, c_tgt):
    """centred -> the caller's frame: t - R c_src + c_tgt in float64."""
    R, t = np.asarray(R).astype(F64), np.asarray(t).astype(F64)
    return R, t - R @ np.asarray(c_src).astype(F64) + np.asarray(c_tgt).astype(F64)


def knn_expansion_f32(x, k):
    """An fp32 emulation of the kNN's expansion on x [3,N] fp32: score = 2 x.y - |x|^2 - |y|^2 with every product and sum
    rounded to fp32, the k largest per row (the row itself among them) -> int [N,k].  What cancels far from the origin."""
    x = np.asarray(x, F32)
    sq = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    dot = (x[0][:, None] * x[0][None, :] + x[1][:, None] * x[1][None, :]) + x[2][:, None] * x[2][None, :]
    score = (F32(2) * dot - sq[:, None]) - sq[None, :]
    return np.argsort(-score, axis=1, kind="stable")[:, :k]


def kept_neighbours(x, k):
    """The share of the true k nearest neighbours (float64, of the fp32 points) the fp32 expansion keeps."""
    x = np.asarray(x, F32)
    x64 = x.astype(F64)
    d = ((x64[:, :, None] - x64[:, None, :]) ** 2).sum(0)
    true = np.argsort(d, axis=1, kind="stable")[:, :k]
    got = knn_expansion_f32(x, k)
    return float(np.mean([len(np.intersect1d(true[i], got[i])) for i in range(x.shape[1])])) / k
