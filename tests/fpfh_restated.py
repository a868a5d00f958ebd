"""CPU restatement of include/vcr_hip_fpfh.h in numpy -- what the tests compare the two kernels with --
and the inputs the CPU and GPU tests share.

`pairs` is the header's pair feature for every (point, idx entry) at once, operation by operation: fp32 differences widened,
every three-term sum as (a + b) + c, nothing fused, so all of it is the device's arithmetic bit for bit except numpy.arctan2,
whose last bit is the math library's.  `excluded` marks the pairs whose f0 coordinate lies so close to a bin boundary that this
last bit could decide.  `spfh` packs the counts as the header lays them out, `fpfh` is the second pass in the header's order
(neighbours in idx's order, bins ascending), one serial chain per (point, group) vectorised over the points."""
import numpy as np

import plane_restated as pr

F32 = np.float32
BINS = 11
ROW = 48
SHAPES = ((1, 5, 4), (2, 64, 20), (3, 257, 20), (2, 1000, 40), (1, 300, 62))      # (B, N, k) of both test files
NEAR = 2.0 ** -30                                           # an f0 coordinate this close to an integer: the pair is excluded


def r2_of(radius):
    """(double)(radius * radius), the product in fp32; no radius: +inf."""
    radius = F32(radius)
    return np.float64(np.inf) if radius == 0 else np.float64(radius * radius)


def geometry(x, idx):
    """x [3,N] fp32, idx int [N,k] -> (j [N,k] the rows read, d [3,N,k] float64, d2 [N,k])."""
    x = np.asarray(x, F32)
    idx = np.asarray(idx).astype(np.int64)
    N = x.shape[1]
    own = np.broadcast_to(np.arange(N)[:, None], idx.shape)
    j = np.where((idx >= 0) & (idx < N), idx, own)
    with np.errstate(all="ignore"):
        d = (x[:, j] - x[:, own]).astype(np.float64)        # the fp32 difference, widened
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return j, d, d2


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _bin(c):
    t = np.floor(c)
    return np.where(t >= 10, 10, np.where(t >= 0, t, 0)).astype(np.int64)       # a NaN fails both: bin 0


def pairs(x, nrm, idx, radius=0.0):
    """-> dict: counted bool [N,k], bins int [N,k,3], coord float64 [N,k,3] (the three values whose floors are the bins), d2,
    tie bool [N,k] (|a1| == |a2| exactly)."""
    nrm = np.asarray(nrm, F32)
    j, d, d2 = geometry(x, idx)
    N, k = j.shape
    own = np.broadcast_to(np.arange(N)[:, None], j.shape)
    n1, n2 = nrm[:, own].astype(np.float64), nrm[:, j].astype(np.float64)
    with np.errstate(all="ignore"):
        counted = np.isfinite(d2) & np.isfinite(n1).all(0) & np.isfinite(n2).all(0) & (d2 <= r2_of(radius))
        L = np.sqrt(d2)
        a1, a2 = _dot(n1, d) / L, _dot(n2, d) / L
        swap = np.abs(a1) < np.abs(a2)
        n1, n2 = np.where(swap, n2, n1), np.where(swap, n1, n2)
        d = np.where(swap, -d, d)
        f2 = np.where(swap, -a2, a1)
        v = _cross(d, n1)
        vn = np.sqrt(_dot(v, v))
        zero = (L == 0) | (vn == 0)
        v = v / vn
        w = _cross(n1, v)
        f1 = _dot(v, n2)
        f0 = np.arctan2(_dot(w, n2), _dot(n1, n2))
        f0, f1, f2 = (np.where(zero, 0.0, f) for f in (f0, f1, f2))
        coord = np.stack([(11.0 * (f0 + np.pi)) / (2.0 * np.pi), (11.0 * (f1 + 1.0)) * 0.5, (11.0 * (f2 + 1.0)) * 0.5], axis=2)
    return {"counted": counted, "bins": _bin(coord), "coord": coord, "d2": d2, "tie": counted & (np.abs(a1) == np.abs(a2)) & ~zero}


def excluded(p):
    """bool [N,k]: the counted pairs whose f0 coordinate lies within NEAR of an integer."""
    c = p["coord"][:, :, 0]
    with np.errstate(all="ignore"):
        return p["counted"] & (np.abs(c - np.round(c)) <= NEAR)


def pack(p):
    """The pairs' bins as the header's bytes: uint8 [N,48]."""
    N, k = p["counted"].shape
    h = np.zeros((N, 3, 16), np.int64)
    rows = np.arange(N)
    for jj in range(k):
        m = p["counted"][:, jj]
        for g in range(3):
            np.add.at(h[:, g, :], (rows[m], p["bins"][m, jj, g]), 1)
    h[:, :, BINS] = p["counted"].sum(1)[:, None]
    assert h.max() <= 255
    return h.astype(np.uint8).reshape(N, ROW)


def spfh(x, nrm, idx, radius=0.0):
    """vcr_spfh_f32 for one cloud: uint8 [N,48]."""
    return pack(pairs(x, nrm, idx, radius))


def fpfh(x, idx, sp, radius=0.0, rounded=True):
    """vcr_fpfh_f32 for one cloud from the SPFH bytes sp [N,48]: float32 [33,N]; rounded=False: the fp64 values in front of the
    final conversion."""
    j, _, d2 = geometry(x, idx)
    N, k = j.shape
    sp = np.asarray(sp, np.uint8).reshape(N, 3, 16)
    r2 = r2_of(radius)
    out = np.zeros((3 * BINS, N), F32 if rounded else np.float64)
    with np.errstate(all="ignore"):
        for g in range(3):
            acc, s = np.zeros((N, BINS)), np.zeros(N)
            for jj in range(k):
                r, dd = j[:, jj], d2[:, jj]
                cj = sp[r, g, BINS].astype(np.float64)
                ok = (dd > 0) & np.isfinite(dd) & (dd <= r2) & (cj != 0)
                sc = 100.0 / cj
                for b in range(BINS):
                    val = (sp[r, g, b].astype(np.float64) * sc) / dd
                    acc[:, b] = np.where(ok, acc[:, b] + val, acc[:, b])
                    s = np.where(ok, s + val, s)
            acc = np.where((s != 0)[:, None], acc * (100.0 / s)[:, None], acc)
            ci = sp[:, g, BINS].astype(np.float64)
            mine = np.where((ci != 0)[:, None], sp[:, g, :BINS].astype(np.float64) * (100.0 / ci)[:, None], 0.0)
            out[g * BINS:(g + 1) * BINS] = (acc + mine).T.astype(out.dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- the recipes

def cloud(B, N):
    """[B,3,N] fp32: the normals tests' jittered torus, one seed per (N, b)."""
    return np.stack([pr.jittered_torus(100 * N + b, N) for b in range(B)])


def neighbours(x, k):
    """x [3,N] -> int32 [N,k]: float64 neighbours, the row itself dropped."""
    return pr.knn_f64(x, k + 1)[:, 1:].astype(np.int32)


def normals(x, idx):
    """The restated normals [3,N] fp32 of x on idx (plane_restated.normal per point)."""
    C = pr.covariances(x, idx)
    return np.stack([pr.normal(c)[0] for c in C], axis=1)


def radius_between(dist, m):
    """A radius (fp32) between the m-th and the (m + 1)-th neighbour distance of the median point; dist [N,k] from any order."""
    near = np.sort(np.asarray(dist, np.float64), axis=1)
    return F32(0.5 * (np.median(near[:, m - 1]) + np.median(near[:, m])))


def plane_cloud(N=200, seed=21):
    """(x [3,N], normals [3,N]): z = 0.25 exactly, x and y uniform; every difference has dz = 0 and every normal is (0,0,1)."""
    rs = np.random.RandomState(seed)
    x = np.concatenate([rs.uniform(0, 1, (2, N)), np.full((1, N), 0.25)]).astype(F32)
    return x, np.tile(np.asarray([[0], [0], [1]], F32), (1, N))


def group_bins(sp):
    """uint8 [...,48] -> the 33 counts [...,33] and c [...]; asserts the layout's fixed bytes."""
    sp = np.asarray(sp, np.uint8)
    g = sp.reshape(sp.shape[:-1] + (3, 16))
    assert not g[..., 12:].any()
    assert (g[..., BINS] == g[..., :1, BINS]).all()
    return g[..., :BINS].reshape(sp.shape[:-1] + (3 * BINS,)).astype(np.int64), g[..., 0, BINS].astype(np.int64)
