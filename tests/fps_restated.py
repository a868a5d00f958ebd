"""CPU restatement of farthest-point sampling (the reference's farthest_point_sample, util/util.py:107-140) in plain IEEE fp32
numpy -- what the GPU tests compare vcr_fps_f32 with at sizes too large to commit as fixtures.  tests/test_fps_cpu.py holds
it to the recorded reference, index for index, on every fixture under tests/golden/fps_*.npz.

    d = (dx*dx + dy*dy) + dz*dz          every operation rounded to fp32 (numpy never contracts)
    dist[n] = d where d < dist[n]        (dist starts at fp32(1e10); false for a NaN d)
    far = the first n with the largest dist[n]

The start point is either given, or the reference's: the point farthest from the barycentre, the coordinate sums taken in
fp64 and rounded to fp32 once (the reference sums in fp32 in an order that depends on the host's vector width: `margin`
below says how far its decision is from depending on that), arg-max by torch.max's rule -- a NaN is the largest value, the
first one wins.
"""
import numpy as np

F32 = np.float32


def _first_argmax_nan_high(v):
    """torch.max's index: the first NaN if there is one, else the first maximum."""
    nan = np.isnan(v)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(v))


def _sq_dist(x, y, z, cx, cy, cz):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = x - cx, y - cy, z - cz
        return (dx * dx + dy * dy) + dz * dz


def barycentre_dist(cloud):
    """cloud [3, N] fp32 -> |p_n - c|^2 [N] fp32 with c = fp32(fp64 sum) / fp32(N)."""
    cloud = np.ascontiguousarray(cloud, dtype=F32)
    n = F32(cloud.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        c = [F32(cloud[k].astype(np.float64).sum()) / n for k in range(3)]
    return _sq_dist(cloud[0], cloud[1], cloud[2], c[0], c[1], c[2])


def barycentre_start(cloud):
    return _first_argmax_nan_high(barycentre_dist(cloud))


def margin(cloud):
    """Relative gap between the largest and the second-largest |p_n - c|^2 of a FINITE cloud -- the barycentre start is held
    to the reference where this is >= 1e-4 (rounding moves the values by ~1e-6)."""
    d = np.sort(barycentre_dist(cloud).astype(np.float64))
    if d.size < 2:
        return float("inf")
    return float((d[-1] - d[-2]) / d[-1]) if d[-1] > 0 else 0.0


def fps_one(cloud, npoint, start=None):
    """cloud [3, N] fp32 -> int64 [npoint]."""
    cloud = np.ascontiguousarray(cloud, dtype=F32)
    x, y, z = cloud
    N = x.shape[0]
    far = barycentre_start(cloud) if start is None else min(max(int(start), 0), N - 1)
    dist = np.full(N, 1e10, dtype=F32)
    out = np.empty(npoint, dtype=np.int64)
    for i in range(npoint):
        out[i] = far
        if i == npoint - 1:
            break
        d = _sq_dist(x, y, z, x[far], y[far], z[far])
        with np.errstate(invalid="ignore"):
            np.copyto(dist, d, where=d < dist)
        far = int(np.argmax(dist))                      # (dist never holds a NaN: np.argmax's first maximum is torch.max's)
    return out


def fps(xyz, npoint, start=None):
    """xyz [B, 3, N] (numpy or torch CPU) -> numpy int64 [B, npoint]; start: None or one index per cloud."""
    xyz = np.asarray(xyz, dtype=F32)
    return np.stack([fps_one(xyz[b], npoint, None if start is None else int(start[b])) for b in range(xyz.shape[0])])
