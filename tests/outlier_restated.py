"""CPU restatement of vcr_outlier_stat_f32 and vcr_outlier_radius_f32 (include/vcr_hip_outlier.h) in
numpy -- what the GPU tests compare the kernels with -- each written twice:

  * `*_loop`: the definition read aloud, a plain double loop (the reading copy, small clouds);
  * `*_fast`: the same vectorised, on nnscore_restated's `d2_f32` (the kernel's fp32 chain) and `block_partials` (sum_d2's
    order); the sum over a point's neighbours is an explicit ordered sum, column by column (np.sum adds pairwise).

The statistical filter comes in the stages the GPU test checks one by one: `mean_dist_*` (coordinates and neighbours -> the fp32
mean distances), `decide` (mean distances -> n, mu, var, sigma, thr, keep) and `compact` (keep -> points, count, index), so that
everything behind mean_dist can be fed the DEVICE's values.  `neighbours` is a reference kNN (fp64 distances, scipy's k-d tree)
for the runs from coordinates alone.  tests/test_outlier_cpu.py holds the two routes to each other on every recipe below, which
tests/test_hip_outlier.py runs on the GPU."""
import numpy as np

import nnscore_restated as nr

F32 = np.float32
NAN_BITS = 0x7FC00000
BAND = 2.0 ** -20                                          # the relative band around a threshold the recipes keep empty


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.int8}[a.dtype.itemsize])


# ---------------------------------------------------------------- the shared tail

def compact(xyz, keep):
    """xyz [3, N] fp32, keep [N] bool -> points fp32 [3, N] (the kept in ascending order, NaN behind), count, index int32 [N]."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    at = np.flatnonzero(keep)
    points = np.full((3, N), np.uint32(NAN_BITS).view(F32), F32)
    index = np.full(N, -1, np.int32)
    points[:, :len(at)] = xyz[:, at]
    index[:len(at)] = at
    return {"points": points, "count": np.int32(len(at)), "index": index}


# ---------------------------------------------------------------- the radius filter

def _fma(a, b, c):
    """fmaf on fp32 scalars, as nnscore_restated.fma32: the exact product, the sum rounded to float64 and then to fp32."""
    return F32(float(a) * float(b) + float(c))


def radius_counts_loop(xyz, radius, rows=None):
    """c_i for the points `rows` (all of them by default), one pair at a time."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    r2 = F32(radius) * F32(radius)
    x, y, z = (list(xyz[c]) for c in range(3))              # fp32 scalars
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (range(N) if rows is None else rows):
            c = 0
            for j in range(N):
                dx, dy, dz = x[i] - x[j], y[i] - y[j], z[i] - z[j]
                if _fma(dz, dz, _fma(dy, dy, dx * dx)) <= r2:                   # (a comparison with NaN is false)
                    c += 1
            out.append(c)
    return np.asarray(out, np.int32)


def radius_loop(xyz, radius, nb_points):
    c = radius_counts_loop(xyz, radius)
    return {"neighbours": c, **compact(xyz, c > nb_points)}


def radius_counts(xyz, radius, rows=None):
    """c_i for the points `rows` (all of them by default) of xyz [3, N], by the kernel's fp32 chain."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    rows = np.arange(xyz.shape[1]) if rows is None else np.asarray(rows)
    r2 = F32(radius) * F32(radius)
    out, chunk = [], nr._chunk(xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, len(rows), chunk):
            out.append((nr.d2_f32(xyz[:, rows[i:i + chunk]], xyz) <= r2).sum(axis=1))
    return np.concatenate(out).astype(np.int32)


def radius_fast(xyz, radius, nb_points):
    c = radius_counts(xyz, radius)
    return {"neighbours": c, **compact(xyz, c > nb_points)}


def radius_band(xyz, radius, rows=None):
    """The smallest |d64(i, j) - r2| / r2 over the pairs (i in rows, j): how far the nearest pair is from the sphere."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    rows = np.arange(xyz.shape[1]) if rows is None else np.asarray(rows)
    r2 = np.float64(F32(radius) * F32(radius))
    best, chunk = np.inf, nr._chunk(xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(0, len(rows), chunk):
            d = np.abs(nr.d64(xyz[:, rows[i:i + chunk]], xyz) - r2)
            best = min(best, np.nanmin(d) if np.isfinite(d).any() else np.inf)
    return best / r2


# ---------------------------------------------------------------- the statistical filter

def neighbours(xyz, k):
    """A reference kNN of xyz [3, N]: int32 [N, k], every point's k nearest OTHER points by fp64 distance among the finite
    points, nearest first; a point that is not finite, and a list that runs short, names the point itself."""
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    idx = np.repeat(np.arange(N, dtype=np.int32)[:, None], k, axis=1)
    at = np.flatnonzero(np.isfinite(xyz).all(axis=0))
    if len(at) > 1:
        p = xyz[:, at].T.astype(np.float64)
        _, nn = cKDTree(p).query(p, k=min(k + 1, len(at)))
        for r, row in enumerate(nn):
            others = [at[j] for j in row if j != r and j < len(at)][:k]          # (among copies the point may not come first)
            idx[at[r], :len(others)] = others
    return idx


def _row(idx_ij, i, N):
    return idx_ij if 0 <= idx_ij < N else i                # an entry outside [0, N) reads as i


def mean_dist_loop(xyz, idx, rows=None):
    """mean_dist of the points `rows` (all of them by default), one neighbour at a time."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N, k = idx.shape
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in (range(N) if rows is None else rows):
            s = np.float64(0.0)
            for j in idx[i]:
                j = _row(int(j), i, N)
                dx, dy, dz = (np.float64(F32(xyz[c, j]) - F32(xyz[c, i])) for c in range(3))
                s = s + np.sqrt((dx * dx + dy * dy) + dz * dz)
            out.append(F32(s / np.float64(k + 1)))
    return np.asarray(out, F32)


def mean_dist_fast(xyz, idx):
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N, k = idx.shape
    me = np.arange(N)
    s = np.zeros(N, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for col in range(k):                                # idx's order, one neighbour at a time
            j = idx[:, col].astype(np.int64)
            j = np.where((j >= 0) & (j < N), j, me)
            dx, dy, dz = ((xyz[c, j] - xyz[c, me]).astype(np.float64) for c in range(3))
            s = s + np.sqrt((dx * dx + dy * dy) + dz * dz)
        return (s / np.float64(k + 1)).astype(F32)


def _ordered(values):
    """sum_d2's order: one partial per 256 values (the butterfly, the four waves), then the partials ascending."""
    total = np.float64(0.0)
    for s in nr.block_partials(values):
        total = total + s
    return total


def _ordered_loop(values):
    """_ordered read aloud: per 256 values every lane adds its partner's sum at offsets 32 ... 1, lane 0 of the four waves is
    added ascending, then the partials ascending."""
    total = np.float64(0.0)
    values = [np.float64(v) for v in values]
    for b0 in range(0, len(values), 256):
        blk = values[b0:b0 + 256] + [np.float64(0.0)] * (256 - len(values[b0:b0 + 256]))
        waves = []
        for w in range(4):
            lanes = blk[64 * w:64 * w + 64]
            for o in (32, 16, 8, 4, 2, 1):
                lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
            waves.append(lanes[0])
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return total


def decide(mean_dist, std_ratio, ordered=_ordered):
    """mean_dist fp32 [N] -> dict of valid (n), mu, var, sigma, thr (float64) and keep [N] bool."""
    mean_dist = np.asarray(mean_dist, F32)
    valid = np.isfinite(mean_dist)
    n = int(valid.sum())
    m64 = mean_dist.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mu = ordered(np.where(valid, m64, 0.0)) / np.float64(n)
        dev = np.where(valid, m64 - mu, 0.0)
        var = ordered(dev * dev) / np.float64(n - 1)
        sigma = np.sqrt(var) if n >= 2 else np.float64(0.0)
        thr = mu + np.float64(F32(std_ratio)) * sigma
        keep = valid & (m64 <= thr)
    return {"valid": np.int32(n), "mu": np.float64(mu), "var": np.float64(var), "sigma": np.float64(sigma),
            "thr": np.float64(thr), "keep": keep}


def stat_parts(md, xyz, std_ratio, ordered=_ordered):
    """Every output of vcr_outlier_stat_f32 (stats = mu, sigma, thr) and `var`, `keep`, from given mean distances."""
    d = decide(md, std_ratio, ordered)
    return {"mean_dist": md, "valid": d["valid"], "stats": np.asarray([d["mu"], d["sigma"], d["thr"]], np.float64),
            "var": d["var"], "keep": d["keep"], **compact(xyz, d["keep"])}


def stat(xyz, idx, std_ratio):
    return stat_parts(mean_dist_fast(xyz, idx), xyz, std_ratio)


def stat_band(mean_dist, thr):
    """The smallest |mean_dist_i - thr| / thr over the valid points (inf: thr is 0 or not finite, or nobody is valid)."""
    m = np.asarray(mean_dist, np.float64)
    m = m[np.isfinite(m)]
    if not (np.isfinite(thr) and thr > 0.0 and len(m)):
        return np.inf
    return np.abs(m - thr).min() / thr


def stat_loop(xyz, idx, std_ratio):
    return stat_parts(mean_dist_loop(xyz, idx), xyz, std_ratio, _ordered_loop)


def batch(fn, xyz, *args):
    """xyz [B, 3, N] (and per-cloud leading arguments stacked on B) -> the dict of stacked per-cloud results."""
    res = [fn(*([c] + [a[b] if isinstance(a, np.ndarray) and a.ndim == 3 else a for a in args])) for b, c in enumerate(xyz)]
    return {k: np.stack([np.asarray(r[k]) for r in res]) for k in res[0]}


# ---- the case recipes the CPU and GPU tests share ----

def uniform(seed, B, N):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, 3, N)).astype(F32)


def radius_for(N, inside=12.0, extent=2.0):
    """The radius at which a point inside a uniform cube of N points has about `inside` of them within reach, itself included."""
    return float(F32(extent * (3.0 * inside / (4.0 * np.pi * N)) ** (1.0 / 3.0)))


def blob_far(seed, N):
    """A dense blob and 5 % far points, spread among it in index: the far ones lie 10 apart on a line from x = 100."""
    x = uniform(seed, 1, N)
    far = np.random.RandomState(seed + 1).permutation(N)[:N // 20]
    x[0, :, far] = np.stack([100.0 + 10.0 * np.arange(len(far)), np.zeros(len(far)), np.zeros(len(far))], axis=1).astype(F32)
    return x, np.sort(far)


def copies(seed, N, times):
    part = uniform(seed, 1, N // times)
    x = np.concatenate([part] * times, axis=2)
    return x[:, :, np.random.RandomState(seed + 1).permutation(x.shape[2])]


def lattice(seed, N, cells=6):
    """Integer lattice points times 2^-6: every difference and every d2 is exact; at radius 2^-6 the six face neighbours lie ON
    the sphere.  Distinct points: a random subset of the cells^3 lattice."""
    pick = np.random.RandomState(seed).permutation(cells ** 3)[:N]
    x = np.stack([pick % cells, pick // cells % cells, pick // cells ** 2]).astype(F32) * F32(2.0 ** -6)
    return x[None]


def non_finite(seed, N, far=False):
    """A NaN point at index 0 and an inf point in the middle; with `far` the same cloud with the two moved far away instead."""
    x = uniform(seed, 1, N)
    x[0, :, 0] = (1e6, -1e6, 1e6) if far else (np.nan, 0.5, 0.5)
    x[0, :, N // 2] = (-1e6, 1e6, 2e6) if far else (0.25, np.inf, 0.25)
    return x


def _three(seed, N):
    return np.concatenate([uniform(seed, 1, N), blob_far(seed + 1, N)[0], non_finite(seed + 3, N)])


# name -> (xyz [B, 3, N] fp32, radius, nb_points); LARGE: compared on a sample of rows (rows_of)
RADIUS_RECIPES = {
    "n1_nb0": lambda: (uniform(1, 1, 1), 0.5, 0),
    "n1_nb1": lambda: (uniform(1, 1, 1), 0.5, 1),
    "n255": lambda: (uniform(2, 1, 255), radius_for(255), 9),
    "n256": lambda: (uniform(3, 1, 256), radius_for(256), 9),
    "n257": lambda: (uniform(4, 1, 257), radius_for(257), 9),
    "n1023": lambda: (uniform(5, 1, 1023), radius_for(1023), 9),
    "n1024": lambda: (uniform(6, 1, 1024), radius_for(1024), 9),
    "n1025": lambda: (uniform(7, 1, 1025), radius_for(1025), 9),
    "n2049": lambda: (uniform(8, 1, 2049), radius_for(2049), 9),
    "three_clouds": lambda: (_three(9, 700), radius_for(700), 7),
    "all_kept": lambda: (uniform(10, 1, 600), 10.0, 0),
    "none_kept": lambda: (uniform(11, 1, 600), 10.0, 600),
    "blob_far": lambda: (blob_far(12, 2000)[0], 0.5, 4),
    "copies": lambda: (copies(13, 900, 2), 1e-6, 1),
    "lattice": lambda: (lattice(14, 150), float(2.0 ** -6), 3),
    "non_finite": lambda: (non_finite(15, 900), radius_for(900), 7),
    "far_instead": lambda: (non_finite(15, 900, far=True), radius_for(900), 7),
    "n70001": lambda: (uniform(16, 1, 70001), radius_for(70001), 9),
    "n131072": lambda: (uniform(17, 1, 131072), radius_for(131072), 9),
}
LARGE = ("n70001", "n131072")
LATTICE = ("lattice",)                                     # excepted from the empty band by construction


def rows_of(name, N, count=96):
    """Sampled rows of a cloud too large to walk whole: the first and last points, the block and tile edges, and random ones."""
    fixed = [i for i in (0, 1, 255, 256, 1023, 1024, N - 1025, N - 257, N - 2, N - 1) if 0 <= i < N]
    rnd = np.random.RandomState(len(name) + N).randint(0, N, size=count - len(fixed))
    return np.unique(np.concatenate([fixed, rnd]))


# name -> (xyz [B, 3, N] fp32, k, std_ratio): the neighbours are `neighbours(cloud, k)` here, the device's kNN on the GPU
STAT_RECIPES = {
    "n2_k1": lambda: (uniform(21, 1, 2), 1, 1.0),
    "n255": lambda: (uniform(22, 1, 255), 8, 1.0),
    "n256": lambda: (uniform(23, 1, 256), 8, 1.0),
    "n257": lambda: (uniform(24, 1, 257), 8, 1.0),
    "n1023": lambda: (uniform(25, 1, 1023), 19, 2.0),
    "n1024": lambda: (uniform(26, 1, 1024), 19, 2.0),
    "n1025": lambda: (uniform(27, 1, 1025), 19, 2.0),
    "three_clouds": lambda: (_three(28, 700), 12, 1.5),
    "all_kept": lambda: (uniform(29, 1, 600), 8, 1e6),
    "ratio0": lambda: (uniform(30, 1, 600), 8, 0.0),
    "blob_far": lambda: (blob_far(31, 2000)[0], 8, 1.0),
    "copies": lambda: (np.concatenate([copies(32, 600, 3), uniform(33, 1, 300)], axis=2), 2, 2.0),
    "non_finite": lambda: (non_finite(34, 900), 10, 1.0),
    "all_nan": lambda: (np.full((1, 3, 300), np.nan, F32), 8, 1.0),
    "k62": lambda: (uniform(35, 1, 300), 62, 1.0),
    "n20000": lambda: (uniform(36, 1, 20000), 20, 2.0),
}
EQUAL = ("n2_k1",)                                         # every mean distance is the same value: excepted from the empty band by
                                                           # construction (two points are each other's only neighbour); the
                                                           # statistics are exact there -- mu IS that value, sigma 0, thr = mu
