"""include/border/vcr_hip_border.h restated in numpy: the frame of a point, the angle of every entry of its
row (np.arctan2: the one library call), the largest gap between the counted angles, the flag, and the flags spread over rows --
every expression in the header's order, in IEEE doubles, one operation a numpy call so nothing is fused.

One cloud is x float32 [3,N] with normals float32 [3,N] and its rows as (idx int [total or more], row_start int64 [N+1]).  The
recipes the CPU and the GPU tests share (the jittered lattice, the closed and the capped sphere) are at the end."""
import math
import struct

import numpy as np

import dbscan_restated as dr
import iss_restated as ir
import radius_restated as rr

F32, I32 = np.float32, np.int32
NOT_SERVED = -2
TWO_PI = struct.unpack("<d", struct.pack("<Q", 0x401921FB54442D18))[0]
CHUNK = 256                                                 # VCR_BORDER_CHUNK
MARGIN = 1e-9                                               # no recipe's gap lies this close to its threshold (test_border_cpu)


def radians(degrees):
    """The threshold of the public call: degrees * (pi / 180), both factors doubles."""
    return float(degrees) * (math.pi / 180.0)


def frame(x_i, n):
    """-> (u, v) as lists of three Python floats, or None where the point has no frame."""
    n0, n1, n2 = float(n[0]), float(n[1]), float(n[2])
    s = (n0 * n0 + n1 * n1) + n2 * n2
    if not (np.isfinite(np.asarray(x_i, np.float64)).all() and math.isfinite(n0) and math.isfinite(n1) and math.isfinite(n2)):
        return None
    if not (s > 0.0 and math.isfinite(s)):
        return None
    inv = 1.0 / math.sqrt(s)
    h = [n0 * inv, n1 * inv, n2 * inv]
    a, am = 0, abs(h[0])
    if abs(h[1]) < am:
        a, am = 1, abs(h[1])
    if abs(h[2]) < am:
        a = 2
    e = [1.0 if a == 0 else 0.0, 1.0 if a == 1 else 0.0, 1.0 if a == 2 else 0.0]
    u = [h[1] * e[2] - h[2] * e[1], h[2] * e[0] - h[0] * e[2], h[0] * e[1] - h[1] * e[0]]
    v = [h[1] * u[2] - h[2] * u[1], h[2] * u[0] - h[0] * u[2], h[0] * u[1] - h[1] * u[0]]
    return u, v


def angles(x, normals, idx, row_start, capacity=None, d2=None, r2=None, atan2=np.arctan2):
    """vcr_border_angles_f32 for one served cloud -> (angle float64 [capacity], frame int32 [N], skipped bool [capacity])."""
    x, normals = np.asarray(x, F32), np.asarray(normals, F32)
    N = x.shape[1]
    row_start = np.asarray(row_start, np.int64)
    idx = np.asarray(idx).astype(np.int64)
    total = int(row_start[-1])
    out = np.full(total if capacity is None else capacity, np.nan)
    fr = np.zeros(N, I32)
    used = ir.used_lengths(row_start, d2, r2)
    with np.errstate(all="ignore"):
        for i in range(N):
            uv = frame(x[:, i], normals[:, i])
            fr[i] = uv is not None
            if uv is None or used[i] == 0:
                continue
            u, v = uv
            j = idx[row_start[i]:row_start[i] + used[i]]
            j = np.where((j >= 0) & (j < N), j, i)
            d = (x[:, j] - x[:, i:i + 1]).astype(np.float64)                # the fp32 differences, widened
            pu = (u[0] * d[0] + u[1] * d[1]) + u[2] * d[2]
            pv = (v[0] * d[0] + v[1] * d[1]) + v[2] * d[2]
            skip = ~np.isfinite(d).all(0) | ((d[0] == 0) & (d[1] == 0) & (d[2] == 0)) | ((pu == 0) & (pv == 0))
            out[row_start[i]:row_start[i] + used[i]] = np.where(skip, np.nan, atan2(pv, pu))
    return out, fr, np.isnan(out)


def gap_of(a, m, min_neighbors=3):
    """The gap of ONE row's angle slots (NaN: not counted), m = the row's entries + 1."""
    a = np.asarray(a, np.float64)
    a = np.unique(a[~np.isnan(a)])                          # ascending, copies once: succ is the next one
    if m < min_neighbors or len(a) == 0:
        return 0.0
    wrap = (TWO_PI - a[-1]) + a[0]
    return float(max(np.max(a[1:] - a[:-1]), wrap)) if len(a) > 1 else float(wrap)


def gaps(angle, row_start, min_neighbors=3, threshold=math.pi / 2, frame=None, d2=None, r2=None):
    """vcr_border_gap_f32 for one served cloud -> (gap float64 [N], flag int32 [N])."""
    row_start = np.asarray(row_start, np.int64)
    N = len(row_start) - 1
    used = ir.used_lengths(row_start, d2, r2)
    gap = np.zeros(N)
    for i in range(N):
        gap[i] = gap_of(angle[row_start[i]:row_start[i] + used[i]], used[i] + 1, min_neighbors)
    if frame is not None:
        gap[np.asarray(frame) == 0] = np.nan
    with np.errstate(invalid="ignore"):
        return gap, (gap > threshold).astype(I32)


def near(flag, idx, row_start, d2=None, r2=None):
    """vcr_border_near_f32 for one served cloud -> near int32 [N] (all -2 where a flag is -2)."""
    flag = np.asarray(flag)
    N = len(flag)
    if (flag == NOT_SERVED).any():
        return np.full(N, NOT_SERVED, I32)
    idx = np.asarray(idx).astype(np.int64)
    used = ir.used_lengths(row_start, d2, r2)
    out = np.zeros(N, I32)
    for i in range(N):
        j = idx[row_start[i]:row_start[i] + used[i]]
        j = np.where((j >= 0) & (j < N), j, i)
        out[i] = flag[i] > 0 or (flag[j] > 0).any()
    return out


def definition(x, normals, rows, min_neighbors=3, threshold=math.pi / 2, capacity=None, d2=None, r2=None, atan2=np.arctan2):
    """The two passes and the selection for one cloud.  rows = (idx, row_start[, total]); capacity enters "served" alone.
    -> dict of angle, frame, gap, flag, points, count, index."""
    x = np.asarray(x, F32)
    N = x.shape[1]
    total = int(rows[2]) if len(rows) > 2 else int(np.asarray(rows[1])[-1])
    cap = total if capacity is None else capacity
    if dr.served(rows[1], total, cap):
        ang, fr, _ = angles(x, normals, rows[0], rows[1], cap, d2, r2, atan2)
        gap, flag = gaps(ang, rows[1], min_neighbors, threshold, fr, d2, r2)
    else:
        ang, fr = np.full(cap, np.nan), np.full(N, NOT_SERVED, I32)
        gap, flag = np.full(N, np.nan), np.full(N, NOT_SERVED, I32)
    points, count, index = ir.select(x, flag)
    return {"angle": ang, "frame": fr, "gap": gap, "flag": flag, "points": points, "count": count, "index": index}


def hybrid_rows(x, radius, max_nn=30):
    """The definition's rows of the public call: all points within radius, cut to the nearest max_nn (None: all)."""
    res = rr.radius_rows(np.ascontiguousarray(x, F32), radius)
    return res if max_nn is None else rr.cut(res, max_nn)


def of_cloud(x, normals, radius, max_nn=30, angle_threshold=90.0, min_neighbors=3):
    """compute_boundary_points for one cloud with given normals, on the definition's rows."""
    res = hybrid_rows(x, radius, max_nn)
    return definition(x, normals, (res["idx"], res["row_start"]), min_neighbors, radians(angle_threshold))


# ------------------------------------------------------------------------------------------------------------------- the recipes

def lattice(n=16, seed=11):
    """An n x n planar lattice of spacing 1 with every coordinate in the plane moved by up to 0.05 and the height by up to 0.01
    -> (x [3,n n], normals: (0, 0, 1) for all, the outer ring bool [n n]).  At a radius of 1.6 an inner point sees exactly its
    eight lattice neighbours (a diagonal one at most 1.1 sqrt 2 = 1.56 away, the next lattice point at least 1.9) all around it,
    each direction within 9 degrees of its multiple of 45: no gap above 63 degrees.  A point of the ring has a half plane empty,
    a corner three quarters."""
    rs = np.random.RandomState(seed)
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = np.stack([gx.ravel() + rs.uniform(-0.05, 0.05, n * n), gy.ravel() + rs.uniform(-0.05, 0.05, n * n),
                  rs.uniform(-0.01, 0.01, n * n)]).astype(F32)
    nrm = np.zeros((3, n * n), F32)
    nrm[2] = 1
    ring = ((gx == 0) | (gx == n - 1) | (gy == 0) | (gy == n - 1)).ravel()
    return x, nrm, ring


def sphere(N=700):
    """The Fibonacci lattice on the unit sphere -> (x [3,N], normals = x)."""
    k = np.arange(N) + 0.5
    z = 1.0 - 2.0 * k / N
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    x = np.stack([r * np.cos(phi), r * np.sin(phi), z]).astype(F32)
    return x, x.copy()


SPHERE_RADIUS = 0.3                                         # about 15 neighbours among 700 points, never fewer than 10
CUT = 0.5                                                   # the capped sphere keeps z <= CUT


def capped(N=700):
    """The sphere without its cap z > CUT -> (x, normals, the kept points' indices in the closed sphere)."""
    x, nrm = sphere(N)
    keep = np.flatnonzero(x[2] <= F32(CUT))
    return np.ascontiguousarray(x[:, keep]), np.ascontiguousarray(nrm[:, keep]), keep


def touched(N=700, radius=SPHERE_RADIUS):
    """bool over the capped sphere's points: a REMOVED point lay within `radius` (the search's fp32 d2) of the point -- its row
    is not the closed sphere's.  Every other point keeps its row's points, hence its gap."""
    x, _ = sphere(N)
    keep = x[2] <= F32(CUT)
    d2 = rr.d2_all(x)
    return ((d2 <= rr.r2_of(radius)) & ~keep[None, :]).any(1)[keep]


def degenerate():
    """The lattice with a copy of a point, a NaN point, a normal of zero and a normal of NaN."""
    x, nrm, _ = lattice()
    x[:, 100] = x[:, 101]
    x[:, 50] = np.nan
    nrm[:, 7] = 0
    nrm[0, 9] = np.nan
    return x, nrm


RECIPES = {"lattice": (lambda: lattice()[:2], 1.6), "sphere": (sphere, SPHERE_RADIUS), "capped": (lambda: capped()[:2], SPHERE_RADIUS),
           "degenerate": (degenerate, 1.6)}


def rows_of_angles(lengths, seed=2, nan_rows=(), duplicates=True):
    """Angle rows for the gap pass alone: row i has lengths[i] slots of uniform angles in [-pi, pi], a tenth of them NaN, some
    copies of others; the rows in nan_rows hold NaN alone -> (angle float64 [total], row_start)."""
    rs = np.random.RandomState(seed)
    row_start = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=row_start[1:])
    a = rs.uniform(-math.pi, math.pi, int(row_start[-1]))
    a[rs.uniform(size=len(a)) < 0.1] = np.nan
    for i, L in enumerate(lengths):
        s = int(row_start[i])
        if duplicates and L >= 4 and i % 2 == 0:
            a[s + 1], a[s + L - 1] = a[s], a[s + 2]
        if i in nan_rows:
            a[s:s + L] = np.nan
    return a, row_start
