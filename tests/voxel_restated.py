"""CPU restatement of vcr_voxel_f32 (include/vcr_hip_voxel.h) in numpy -- what the GPU tests compare the
kernels with, bit for bit -- written twice:

  * `voxel_loop`: the definition read aloud, one loop over the points and a dict from cell to voxel (the reading copy);
  * `voxel_fast`: the same by keys, np.unique, a stable argsort and an explicit ordered sum in fp64 (the large clouds).

Both start a voxel's sum AS its first member (so a voxel of one point returns that point's bits, -0.0 included) and add the
others in ascending index order; np.add.reduceat is not used for that, since numpy sums a long contiguous run pairwise.
tests/test_voxel_cpu.py holds the two to each other on every recipe below, which tests/test_hip_voxel.py runs on the GPU."""
import numpy as np

F32 = np.float32
MAX_CELLS = 1 << 21
NAN_BITS = 0x7FC00000


def _cells(xyz, h):
    """xyz [3, N] fp32 -> (finite [N] bool, cells [3, N] float64 or None without a finite point)."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    hd = np.float64(F32(h))
    finite = np.isfinite(xyz).all(axis=0)
    if not finite.any():
        return finite, None
    lo = xyz[:, finite].min(axis=1)                                             # the fp32 minimum over the finite points
    origin = lo.astype(np.float64) - 0.5 * hd
    with np.errstate(invalid="ignore", over="ignore"):
        cells = np.floor((xyz.astype(np.float64) - origin[:, None]) / hd)       # one fp64 subtraction, one fp64 division
    return finite, cells


def _empty(N, count):
    return {"points": np.full((3, N), np.uint32(NAN_BITS).view(F32), F32), "count": np.int32(count),
            "point_voxel": np.full(N, -1, np.int32), "voxel_points": np.zeros(N, np.int32)}


def voxel_loop(xyz, h):
    """xyz [3, N] fp32, h -> dict of points fp32 [3, N], count, point_voxel int32 [N], voxel_points int32 [N]."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    finite, cells = _cells(xyz, h)
    if cells is None:
        return _empty(N, 0)
    if (cells[:, finite] >= MAX_CELLS).any():
        return _empty(N, -1)
    out = _empty(N, 0)
    number, sums, members = {}, [], []
    for i in range(N):
        if not finite[i]:
            continue
        cell = (int(cells[0, i]), int(cells[1, i]), int(cells[2, i]))
        p = xyz[:, i].astype(np.float64)
        if cell not in number:                                                  # the first to appear: the representative
            number[cell] = len(sums)
            sums.append(p)                                                      # the sum starts AS the first member
            members.append(1)
        else:
            v = number[cell]
            sums[v] = sums[v] + p
            members[v] += 1
        out["point_voxel"][i] = number[cell]
    for v, (s, n) in enumerate(zip(sums, members)):
        out["points"][:, v] = (s / np.float64(n)).astype(F32)
        out["voxel_points"][v] = n
    out["count"] = np.int32(len(sums))
    return out


def voxel_fast(xyz, h):
    """voxel_loop's result without a Python loop over the points."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    finite, cells = _cells(xyz, h)
    if cells is None:
        return _empty(N, 0)
    at = np.flatnonzero(finite)
    c = cells[:, at]
    if (c >= MAX_CELLS).any():
        return _empty(N, -1)
    c = c.astype(np.int64)
    keys = c[2] << 42 | c[1] << 21 | c[0]
    _, index, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(index, kind="stable")                                    # the voxels by first appearance
    number = np.empty(len(order), np.int64)
    number[order] = np.arange(len(order))
    vox = number[inverse.reshape(-1)]                                            # per finite point
    M = len(order)
    members = counts[order]
    by_voxel = at[np.argsort(vox, kind="stable")]                               # members of voxel 0 ascending, of voxel 1, ...
    first = np.concatenate([[0], np.cumsum(members)[:-1]])
    x64 = xyz.astype(np.float64)
    sums = x64[:, by_voxel[first]].copy()                                       # the sum starts AS the first member
    for k in range(1, int(members.max())):                                      # ... and takes the k-th member of every voxel that has one
        has = np.flatnonzero(members > k)
        sums[:, has] = sums[:, has] + x64[:, by_voxel[first[has] + k]]
    out = _empty(N, M)
    out["points"][:, :M] = (sums / members.astype(np.float64)).astype(F32)
    out["point_voxel"][at] = vox
    out["voxel_points"][:M] = members
    return out


def batch(xyz, h, fn=voxel_fast):
    """xyz [B, 3, N] -> the dict of stacked per-cloud results: every cloud's result is its own."""
    res = [fn(c, h) for c in xyz]
    return {k: np.stack([r[k] for r in res]) for k in res[0]}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    """Two results agree in every bit of every output (NaN padding and -0.0 count)."""
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("points", "count", "point_voxel", "voxel_points"))


# ---- the case recipes the CPU and GPU tests share: name -> (xyz [B, 3, N] fp32, voxel_size) ----

def edge_for(N, per_voxel=8.0, extent=2.0):
    """The edge at which a uniform cube of N points and that extent holds about per_voxel points a voxel."""
    return float(F32(extent * (per_voxel / N) ** (1.0 / 3.0)))


def uniform(seed, B, N):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, 3, N)).astype(F32)


def lattice(seed, B, N):
    """Multiples of 0.125 in [0, 2): on a grid of edge 0.25 from min - 0.125 every other value sits exactly on a cell face."""
    return (np.random.RandomState(seed).randint(0, 16, size=(B, 3, N)) * 0.125).astype(F32)


def non_finite(seed, N):
    x = uniform(seed, 1, N)
    x[0, :, 50] = x[0, :, 1]                                # 1, 50 and 51 share a voxel whose first point ...
    x[0, :, 51] = x[0, :, 1] + F32(1e-4)
    x[0, 0, 1] = np.nan                                     # ... is not finite: 50 is the representative
    x[0, 0, 0] = np.nan
    x[0, 1, 17] = np.inf
    x[0, 2, 300] = -np.inf
    x[0, :, N - 1] = np.nan
    x[0, 1, 256::97] = np.nan
    return x


FINE_H = float(F32(2.0 ** -10))
FINE_OVER = float((1 << 21) * 2.0 ** -10)                   # cell(max) = floor(2^21 + 0.5): one too many
FINE_UNDER = float(((1 << 21) - 1) * 2.0 ** -10)            # cell(max) = 2^21 - 1: the last one served


def fine_batch(seed, N):
    """Three clouds at h = 2^-10: a small one, one whose x extent is one cell too many (y, z just fit), one that just fits on all
    three axes."""
    rs = np.random.RandomState(seed)
    x = np.empty((3, 3, N), F32)
    x[0] = rs.uniform(0.0, 0.004, size=(3, N))
    for b, tops in ((1, (FINE_OVER, FINE_UNDER, FINE_UNDER)), (2, (FINE_UNDER,) * 3)):
        for c, top in enumerate(tops):
            x[b, c] = rs.uniform(0.0, top, size=N)
            x[b, c, 3 + c], x[b, c, 11 + c] = top, 0.0      # the extent is met exactly
    return x


def _duplicated(seed, N):
    half = uniform(seed, 1, N // 2)
    x = np.concatenate([half, half], axis=2)
    return x[:, :, np.random.RandomState(seed + 1).permutation(N)]


def _own_voxel(seed, N):
    x = uniform(seed, 1, N)
    x[0, 1, 5] = -0.0
    return x


def _three(seed, N):
    return np.concatenate([uniform(seed, 1, N), lattice(seed + 1, 1, N) - F32(1.0), non_finite(seed + 2, N)])


def _all_nan(N):
    x = np.full((1, 3, N), np.nan, F32)
    x[0, 1, ::3] = 1.0
    x[0, 0, ::5] = np.inf
    return x


RECIPES = {
    "n1": lambda: (uniform(1, 1, 1), 0.5),
    "n5_one_voxel": lambda: (uniform(2, 1, 5), 10.0),
    "n256": lambda: (uniform(3, 1, 256), edge_for(256)),
    "n257": lambda: (uniform(4, 1, 257), edge_for(257)),
    "n1024": lambda: (uniform(5, 1, 1024), edge_for(1024)),
    "n1025": lambda: (uniform(6, 1, 1025), edge_for(1025)),
    "n2049": lambda: (uniform(7, 1, 2049), edge_for(2049)),
    "three_clouds": lambda: (_three(8, 700), 0.25),
    "lattice_faces": lambda: (lattice(9, 2, 1500), 0.25),
    "duplicates": lambda: (_duplicated(10, 1200), edge_for(1200)),
    "own_voxel": lambda: (_own_voxel(11, 777), 1e-5),
    "one_voxel_1025": lambda: (uniform(12, 1, 1025), 100.0),
    "non_finite": lambda: (non_finite(13, 900), edge_for(900)),
    "all_nan": lambda: (_all_nan(300), 0.5),
    "fine_batch": lambda: (fine_batch(14, 500), FINE_H),
    "n70001": lambda: (uniform(15, 1, 70001), edge_for(70001)),
    "n131072": lambda: (uniform(16, 1, 131072), edge_for(131072)),
}
