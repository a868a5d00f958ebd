"""CPU restatement of vcr_nn_score_f32 (include/vcr_hip_score.h) in numpy -- what the GPU tests compare
the kernel with.  Two views of the same search:

  * float64 distances computed from the fp32 points (`d64`, `nearest_f64`): the yardstick for random clouds, where the
    kernel's fp32 d2 is held to it within bounds derived from the rounding steps;
  * the kernel's own fp32 chain (`moved`, `d2_f32`, `nearest_f32`): dx = p - q rounded, d2 = fmaf(dz, dz, fmaf(dy, dy, dx*dx)).
    numpy has no fmaf, so `fma32` takes the exact product in float64 and rounds the sum twice (to float64, then to fp32).  That
    equals fmaf unless the float64 sum lands exactly on an fp32 rounding boundary; the tests compare bit for bit only on
    inputs where every step is exact (the 0.25 lattice under signed permutations), and there the two agree trivially.

and the summary (`summary`), whose fp64 sum follows the kernel's order exactly: per 256 consecutive source points the wave
butterfly (lane + lane^32, then ^16 ... ^1), the four waves ascending, then the partials ascending."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                                             # fp32 unit roundoff


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def moved(src, R=None, t=None):
    """src [3, N] fp32, R [3, 3], t [3] -> [3, N]: pose_step's expression, p_c = fmaf(r_c2, z, fmaf(r_c1, y, r_c0 * x)) + t_c."""
    src = np.ascontiguousarray(src, dtype=F32)
    if R is None:
        return src
    R, t = np.asarray(R, F32), np.asarray(t, F32)
    x, y, z = src
    return np.stack([fma32(R[c, 2], z, fma32(R[c, 1], y, R[c, 0] * x)) + t[c] for c in range(3)]).astype(F32)


def d2_f32(p, q):
    """p [3, n], q [3, m] fp32 -> [n, m] fp32, the kernel's chain."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (p[c][:, None] - q[c][None, :] for c in range(3))
        return fma32(dz, dz, fma32(dy, dy, dx * dx))


def d64(p, q):
    """p [3, n], q [3, m] fp32 -> [n, m] float64 squared distances of those fp32 points."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return sum((p[c][:, None] - q[c][None, :]) ** 2 for c in range(3))


def _first_min(d):
    """Per row the kernel's rule: the smallest finite value, the first among equals; (-1, +inf) when there is none."""
    d = np.where(np.isfinite(d), d, np.inf)
    idx = np.argmin(d, axis=1)
    best = d[np.arange(d.shape[0]), idx]
    return np.where(np.isfinite(best), idx, -1).astype(np.int64), best


def _chunk(q):
    return max(1, (1 << 22) // q.shape[1])                  # rows per block of the distance matrix: <= 32 MB of float64


def nearest_f32(p, q):
    """(nn_idx int64 [n], nn_d2 fp32 [n]) by the kernel's fp32 chain and rule."""
    idx, best, chunk = [], [], _chunk(q)
    for i in range(0, p.shape[1], chunk):
        a, b = _first_min(d2_f32(p[:, i:i + chunk], q))
        idx.append(a); best.append(b.astype(F32))
    return np.concatenate(idx), np.concatenate(best)


def nearest_f64(p, q):
    """(arg-min int64 [n], D64 [n], second-smallest float64 distance [n] (inf when m == 1)) over the finite float64 distances."""
    idx, best, second, chunk = [], [], [], _chunk(q)
    for i in range(0, p.shape[1], chunk):
        d = d64(p[:, i:i + chunk], q)
        a, b = _first_min(d)
        d = np.where(np.isfinite(d), d, np.inf)
        d[np.arange(d.shape[0]), np.maximum(a, 0)] = np.inf
        idx.append(a); best.append(b); second.append(d.min(axis=1))
    return np.concatenate(idx), np.concatenate(best), np.concatenate(second)


def double_loop(p, q):
    """The definition, one pair at a time (tiny inputs): a candidate replaces the best only on d2 < best."""
    idx, best = [], []
    for i in range(p.shape[1]):
        bi, bd = -1, F32(np.inf)
        for j in range(q.shape[1]):
            dx, dy, dz = (F32(p[c, i]) - F32(q[c, j]) for c in range(3))
            d = F32(fma32(dz, dz, fma32(dy, dy, dx * dx)))
            if d < bd:
                bi, bd = j, d
        idx.append(bi); best.append(bd)
    return np.asarray(idx, np.int64), np.asarray(best, F32)


def block_partials(values):
    """float64 [n] -> one sum per 256 consecutive values in the kernel's order."""
    n = values.shape[0]
    v = np.zeros(((n + 255) // 256) * 256, np.float64)
    v[:n] = values
    v = v.reshape(-1, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def summary(nn_idx, nn_d2, max_dist):
    """One cloud's (inliers, sum_d2 float64, fitness fp32, rmse fp32) from its neighbours."""
    nn_d2 = np.asarray(nn_d2, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        limit = F32(max_dist) * F32(max_dist)
        inl = (np.asarray(nn_idx) >= 0) & (nn_d2 <= limit)
    total = np.float64(0.0)
    for s in block_partials(np.where(inl, nn_d2.astype(np.float64), 0.0)):
        total = total + s
    count = int(inl.sum())
    fitness = F32(count) / F32(nn_d2.shape[0])
    rmse = F32(np.sqrt(total / np.float64(count))) if count else F32(0.0)
    return count, total, fitness, rmse


def score(src, tgt, R=None, t=None, max_dist=0.0):
    """src [B,3,Ns], tgt [B,3,Nt] (R [B,3,3], t [B,3]) -> dict of stacked nn_idx, nn_d2, inliers, sum_d2, fitness, rmse by the
    fp32 chain."""
    out = {k: [] for k in ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse")}
    for b in range(src.shape[0]):
        p = moved(src[b], None if R is None else R[b], None if t is None else t[b])
        idx, d2 = nearest_f32(p, np.ascontiguousarray(tgt[b], dtype=F32))
        c, s, f, r = summary(idx, d2, max_dist)
        for k, v in zip(out, (idx, d2, c, s, f, r)):
            out[k].append(v)
    return {"nn_idx": np.stack(out["nn_idx"]), "nn_d2": np.stack(out["nn_d2"]), "inliers": np.asarray(out["inliers"], np.int32),
            "sum_d2": np.asarray(out["sum_d2"], np.float64), "fitness": np.asarray(out["fitness"], F32),
            "rmse": np.asarray(out["rmse"], F32)}
