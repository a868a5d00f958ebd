"""One table of the staged calls, for tests/test_stream_table_cpu.py (coverage and validity, no GPU) and tests/test_hip_streams.py
(a side stream, HIP graph capture).  INTEGRATION.md promises of every one of them: asynchronous on the caller's stream, no
allocation by the library, no synchronisation -- so the host never reads device data.

A row is (name, covers, make, call, outputs, ranges, csr):
  name      the test id
  covers    "module.function" of vcrnet_amd the row calls (two rows where a selector picks another launch form)
  make      make(seed) -> the call's keyword arguments as HOST values: numpy arrays (they become the static device buffers) and
            plain scalars.  make(1) and make(2) have the same keys, shapes, dtypes and scalars and different array contents, and
            both are valid inputs on their own AND IN ANY MIXTURE: a stale or mixed read then gives other numbers, never an
            out-of-range access.  That is why the rows' inputs are drawn here and not taken from an upstream call: a derived input
            (normals, histograms, labels, weights) is any caller's by the headers, and a drawn one keeps every index inside the
            shared shapes whichever seed it comes from.  The slots of idx behind a cloud's total hold 0, not -1, for the same
            reason: no correct call reads them, and a mixed one stays inside the cloud.
  call      call(**device tensors and scalars) -> dict of output name -> device tensor
  outputs   the names `call` returns
  ranges    input name -> (lo, hi): an index-typed input, every value in [lo, hi)
  csr       (idx, row_start, total) names of CSR triples: row_start ascends from 0 to total <= capacity = idx.shape[1]
            (in the place of idx, any [B,capacity] list the offsets index: border.gap_rows' angles)

The shapes are the smallest that take more than one workgroup a launch with a ragged last one (N = 300 or 257 of 256-thread
workgroups, the ICP loops and the pose graph at 4 iterations), never the workload's size."""
import functools
import math
from collections import namedtuple

import numpy as np

import colored_restated as cr
import posegraph_restated as pgr
import refine_restated as rr

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
Row = namedtuple("Row", "name covers make call outputs ranges csr")

B, N, M = 2, 300, 257                      # clouds, points a cloud, query positions / source points
K = 8                                      # neighbours of a fixed-width list
RADIUS = 0.17                              # rows of about six entries in the unit cube
CAP = 4000                                 # one capacity for both seeds' rows (asserted on the CPU)
NT, NS = 400, 257                          # the registration pairs
MAX_DIST = cr.MAX_DIST
POSE_OUT = ("R", "t", "R_ba", "t_ba", "fitness", "rmse", "inliers", "sum_d2", "iterations", "converged", "nn_idx", "nn_d2")
FILTER_OUT = ("points", "count", "index")

ROWS = []


def row(name, covers, make, call, outputs, ranges=None, csr=()):
    ROWS.append(Row(name, covers, functools.lru_cache(maxsize=None)(make), call, tuple(outputs), dict(ranges or {}), tuple(csr)))


def rng(seed, salt):
    return np.random.RandomState(7919 * seed + salt)


# ------------------------------------------------------------------------------------------------------------ host recipes

def cloud(seed, n=N, salt=0, b=B):
    return rng(seed, salt).uniform(0.0, 1.0, (b, 3, n)).astype(F32)


def rows4(x):
    """native.to_rows4 on the host: [B,3,n] -> [B,n,4] rows (x, y, z, |p|^2)."""
    p = np.transpose(x, (0, 2, 1))
    return np.ascontiguousarray(np.concatenate([p, (p * p).sum(-1, keepdims=True)], -1), F32)


def unit(seed, n=N, salt=1, b=B):
    v = rng(seed, salt).normal(size=(b, 3, n))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def d2_matrix(x, q):
    d = q[:, :, :, None].astype(F64) - x[:, :, None, :].astype(F64)
    return (d * d).sum(1).astype(F32)                       # [B, queries, points]


def knn_lists(x, k=K):
    """The k nearest other points of every point, brute force: int32 [B,n,k]."""
    d = d2_matrix(x, x)
    d[:, np.arange(x.shape[2]), np.arange(x.shape[2])] = np.inf
    return np.ascontiguousarray(np.argsort(d, axis=2, kind="stable")[:, :, :k], I32)


def csr_rows(x, radius=RADIUS, queries=None, cap=CAP):
    """The radius rows of x about its own points (a point is not in its own row) or about `queries`, ascending in (d2, j):
    idx int32 [B,cap] (0 behind the total), row_start int64 [B,n+1], total int64 [B], d2 float32 [B,cap] (+inf behind)."""
    q = x if queries is None else queries
    d = d2_matrix(x, q)
    b, m, n = d.shape
    idx, d2 = np.zeros((b, cap), I32), np.full((b, cap), np.inf, F32)
    row_start, total = np.zeros((b, m + 1), I64), np.zeros(b, I64)
    for c in range(b):
        at = 0
        for i in range(m):
            hit = d[c, i] <= F32(radius) * F32(radius)
            if queries is None:
                hit[i] = False
            j = np.nonzero(hit)[0]
            j = j[np.argsort(d[c, i, j], kind="stable")]
            assert at + len(j) <= cap, "the recipe's rows must fit its capacity"
            idx[c, at:at + len(j)], d2[c, at:at + len(j)] = j, d[c, i, j]
            at += len(j)
            row_start[c, i + 1] = at
        total[c] = at
    return idx, row_start, total, d2


@functools.lru_cache(maxsize=None)
def _cloud_rows(seed):
    x = cloud(seed)
    return (x,) + csr_rows(x)


def cloud_rows(seed, want_d2=False):
    x, idx, row_start, total, d2 = _cloud_rows(seed)
    o = dict(idx=idx, row_start=row_start, total=total)
    if want_d2:
        o["d2"] = d2
    return x, o


def flags(seed, shape, salt=2, hi=2):
    return rng(seed, salt).randint(0, hi, shape).astype(I32)


def histograms(seed, n, salt=3):
    """SPFH words as the rows' kernels write them: int32 [B,n,3,12], eleven bin counts and their sum."""
    h = rng(seed, salt).randint(0, 4, (B, n, 3, 12)).astype(I32)
    h[..., 11] = h[..., :11].sum(-1)
    return h


def rotations(seed, b, degrees=4.0, salt=4):
    rs = rng(seed, salt)
    return np.stack([rr.rotation(rs.normal(size=3), degrees) for _ in range(b)])


def queries(seed):
    return rng(seed, 5).uniform(-0.05, 1.05, (B, 3, M)).astype(F32)


@functools.lru_cache(maxsize=None)
def _support(seed):
    return support_case_of(seed)


def support_case(seed):
    x, q, o = _support(seed)
    return x, q, dict(o)


def support_case_of(seed):
    """A support cloud, M centres (the first half the support's own points), the rows over the centres."""
    x, q = cloud(seed), queries(seed)
    self_index = np.full((B, M), -1, I32)
    for c in range(B):
        own = rng(seed, 6 + c).permutation(N)[:M // 2]
        q[c, :, :M // 2] = x[c][:, own]
        self_index[c, :M // 2] = own
    idx, row_start, total, _ = csr_rows(x, queries=q)
    return x, q, dict(xyz4=rows4(x), c4=rows4(q), idx=idx, row_start=row_start, total=total, self_index=self_index)


@functools.lru_cache(maxsize=None)
def pair(seed):
    """Two clouds of colored_restated's bowl: source, target, the target's normals, gradients and intensities, the start."""
    c = cr.batch("bowl", 40 + seed, NT, NS, B=B)
    return dict(src=np.array(c["src"], F32), tgt=np.array(c["tgt"], F32), R=np.array(c["R0"], F32), t=np.array(c["t0"], F32),
                tgt_normals=np.array(c["nrm_t"], F32), tgt_gradient=np.array(c["grad_t"], F32),
                src_intensity=np.array(c["I_s"], F32), tgt_intensity=np.array(c["I_t"], F32))


def pair_args(seed, *names, **scalars):
    p = pair(seed)
    return dict({n: p[n] for n in ("src", "tgt", "R", "t") + names}, max_dist=MAX_DIST, **scalars)


def matched(seed):
    return dict(_matched(seed))


@functools.lru_cache(maxsize=None)
def _matched(seed):
    """A source, a moved and permuted copy as the target, and corr: the true partner, a fifth of them wrong."""
    rs = rng(seed, 7)
    src = cloud(seed, NS, salt=8)
    R, t = rotations(seed, B, 30.0), rs.uniform(-0.3, 0.3, (B, 3, 1))
    tgt, corr = np.empty((B, 3, NT), F32), np.empty((B, NS), I32)
    for c in range(B):
        extra = rs.uniform(0.0, 1.0, (3, NT - NS))
        perm = rs.permutation(NT)
        full = np.concatenate([R[c] @ src[c].astype(F64) + t[c], extra], 1)
        tgt[c] = full[:, perm]
        where = np.empty(NT, I64)
        where[perm] = np.arange(NT)
        corr[c] = where[:NS]
        wrong = rs.permutation(NS)[:NS // 5]
        corr[c, wrong] = rs.randint(0, NT, len(wrong))
    return dict(src=src, tgt=tgt, corr=corr)


def randn(seed, salt, *shape, scale=1.0):
    return (rng(seed, salt).standard_normal(shape) * scale).astype(F32)


def gather_idx(seed, m, k, n, salt=9):
    return rng(seed, salt).randint(0, n, (m, k)).astype(I32)


# --------------------------------------------------------------------------------------------------------------- adapters

def mod(name):
    import importlib
    import vcrnet_amd  # noqa: F401
    return importlib.import_module("vcrnet_amd." + name)


def named(names, values):
    return {n: v for n, v in zip(names, values) if v is not None}


def pick(names, d):
    return {n: d[n] for n in names}


def fn(path):
    m, f = path.split(".")
    return getattr(mod(m), f)


def dict_call(path, outputs, **fixed):
    """The wrapper returns a dict: keep the declared outputs."""
    return lambda **kw: pick(outputs, fn(path)(**kw, **fixed))


def tuple_call(path, outputs, **fixed):
    """The wrapper returns a tensor or a tuple: name its elements."""
    def call(**kw):
        r = fn(path)(**kw, **fixed)
        return named(outputs, r if isinstance(r, tuple) else (r,))
    return call


# =================================================================================================== the learned path (native)

LIN_M, LIN_N, LIN_K = 300, 192, 64
E = 512                                                     # the embedding's width
NB, H, NQ = 2, 4, 100                                       # attention: batches, heads, queries = keys


def weights(seed, salt, o, i):
    return randn(seed, salt, o, i, scale=1.0 / math.sqrt(i))


row("pointwise", "native.pointwise",
    lambda s: dict(x_cf=cloud(s), w1=weights(s, 10, 64, 3), b1=randn(s, 11, 64), w2=weights(s, 12, 64, 64), b2=randn(s, 13, 64),
                   pq_w=weights(s, 14, 256, 64), pq_b=randn(s, 15, 256)),
    tuple_call("native.pointwise", ("xyz4", "feat64", "sq64", "pq")), ("xyz4", "feat64", "sq64", "pq"))


def feature_rows(s):
    f = randn(s, 16, B, N, 64)
    return dict(feat=f, sq=(f.astype(F64) ** 2).sum(-1).astype(F32), xyz4=rows4(cloud(s)))


row("knn[xyz4]", "native.knn", lambda s: dict(x=rows4(cloud(s)), k=20),
    lambda x, k: {"idx": fn("native.knn")(x, None, k)}, ("idx",))
row("knn[feat64]", "native.knn", lambda s: dict(pick(("feat", "sq"), feature_rows(s)), k=20),
    lambda feat, sq, k: {"idx": fn("native.knn")(feat, sq, k)}, ("idx",))
row("knn_pair", "native.knn_pair", lambda s: dict(feature_rows(s), k=20),
    tuple_call("native.knn_pair", ("idx_feat", "idx_xyz")), ("idx_feat", "idx_xyz"))
row("knn_pair_deferred", "native.knn_pair_deferred", lambda s: dict(feature_rows(s), k=20),
    lambda feat, sq, xyz4, k: named(("idx_xyz", "idx_feat"), fn("native.knn_pair_deferred")(xyz4, None, feat, sq, k)),
    ("idx_xyz", "idx_feat"))
ORDER_OUT = ("perm", "xyz4_p", "cen4", "cen4_rad", "cen4_sqmax", "feat_p", "sq_p", "cen64", "cen64_sq", "cen64_rad", "cen64_sqmax")
row("knn_order", "native.knn_order", lambda s: feature_rows(s),
    lambda feat, sq, xyz4: pick(ORDER_OUT, fn("native.knn_order")(xyz4, feat, sq)), ORDER_OUT)
row("linear", "native.linear",
    lambda s: dict(x=randn(s, 17, LIN_M, LIN_K), w=weights(s, 18, LIN_N, LIN_K), bias=randn(s, 19, LIN_N),
                   residual=randn(s, 20, LIN_M, LIN_N), relu=True, want_stats=True),
    tuple_call("native.linear", ("y", "stats")), ("y", "stats"))
row("fold_layernorm", "native.fold_layernorm",
    lambda s: dict(w=weights(s, 21, LIN_N, E), bias=randn(s, 22, LIN_N), ln_a=randn(s, 23, E), ln_b=randn(s, 24, E)),
    tuple_call("native.fold_layernorm", ("w", "colsum", "bias")), ("w", "colsum", "bias"))
row("split_bf16x3", "native.split_bf16x3", lambda s: dict(w=weights(s, 25, LIN_N, LIN_K)),
    tuple_call("native.split_bf16x3", ("planes",)), ("planes",))


def planes_of(w):
    """native.split_bf16x3 on the host: int16 [3, numel], hi + mid + lo == w exactly."""
    out, rest = [], w.astype(F32).ravel()
    for _ in range(3):
        piece = (rest.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)            # truncation: every remainder is exact
        out.append((piece.view(np.uint32) >> np.uint32(16)).astype(np.uint16).view(np.int16))
        rest = (rest - piece).astype(F32)
    return np.stack(out)


row("linear_bf16x3", "native.linear_bf16x3",
    lambda s: dict(x=randn(s, 26, LIN_M, LIN_K), w_planes=planes_of(weights(s, 27, LIN_N, LIN_K)), n_out=LIN_N,
                   bias=randn(s, 28, LIN_N), relu=True),
    tuple_call("native.linear_bf16x3", ("y",)), ("y",))
row("layernorm", "native.layernorm",
    lambda s: dict(x=randn(s, 29, LIN_M, E), a=randn(s, 30, E), b=randn(s, 31, E), residual=randn(s, 32, LIN_M, E),
                   xyz4=randn(s, 33, LIN_M, 4)),
    tuple_call("native.layernorm", ("y", "side4")), ("y", "side4"))
row("rowside", "native.rowside", lambda s: dict(x=randn(s, 34, LIN_M, E), xyz4=randn(s, 35, LIN_M, 4), scale=0.5),
    tuple_call("native.rowside", ("y", "side4")), ("y", "side4"))


def edge_case(s, width, k=20):
    return dict(pq=randn(s, 36, B * N, width), idx=gather_idx(s, B * N, k, N), n_per_cloud=N)


for _name, _fixed in (("edgeconv", {}), ("edgeconv[bf16x3]", {"bf16x3": True})):
    row(_name, "native.edgeconv",
        lambda s: dict(edge_case(s, 256), w2=weights(s, 37, 128, 128), b2=randn(s, 38, 128, scale=0.3)),
        tuple_call("native.edgeconv", ("x1", "x2"), **_fixed), ("x1", "x2"), {"idx": (0, N)})
for _name, _variant in (("gathermax", 0), ("gathermax[l2]", 1), ("gathermax[lds]", 32)):
    row(_name, "native.gathermax", lambda s: dict(edge_case(s, 512), Cc=256),
        tuple_call("native.gathermax", ("y",), variant=_variant), ("y",), {"idx": (0, N)})
row("edgerows", "native.edgerows", lambda s: dict(edge_case(s, 128), Cc=64),
    tuple_call("native.edgerows", ("h",)), ("h",), {"idx": (0, N)})
row("edgechain", "native.edgechain",
    lambda s: dict(edge_case(s, 128), w2=weights(s, 39, 64, 64), b2=randn(s, 40, 64, scale=0.3), w3=weights(s, 41, 128, 64),
                   b3=randn(s, 42, 128, scale=0.3), w4=weights(s, 43, 256, 128), b4=randn(s, 44, 256, scale=0.3)),
    tuple_call("native.edgechain", ("out",)), ("out",), {"idx": (0, N)})
row("segmax", "native.segmax", lambda s: dict(x=randn(s, 45, 129 * 7, 64), M=129, k=7),
    tuple_call("native.segmax", ("y",)), ("y",))


def qkv(s):
    return dict(q=randn(s, 46, NB * NQ, H * 128), k=randn(s, 47, NB * NQ, H * 128), v=randn(s, 48, NB * NQ, H * 128),
                nbatch=NB, heads=H, nq=NQ, nk=NQ, scale=1.0 / math.sqrt(128), kv_batch_shift=1)


row("sdpa", "native.sdpa", qkv, tuple_call("native.sdpa", ("out",)), ("out",))
row("sdpa[bf16x3]", "native.sdpa", qkv, tuple_call("native.sdpa", ("out",), bf16x3=True), ("out",))
row("sdpa[rowstat+split]", "native.sdpa", qkv,
    lambda v, **kw: {"rowstat": fn("native.sdpa")(v=None, pv=False, want_rowstat=True, split=True, **kw)[1]}, ("rowstat",))
LD = 128
row("keymass", "native.keymass",
    lambda s: dict(score=randn(s, 49, NB, H, NQ, LD),
                   rowstat=np.stack([randn(s, 50, NB, H, NQ) + 4.0, rng(s, 51).uniform(1.0, 50.0, (NB, H, NQ)).astype(F32)], -1),
                   nk=NQ, q_batch_shift=1),
    tuple_call("native.keymass", ("mass",)), ("mass",))


def sides(s, salt, rows_, e):
    return np.concatenate([rng(s, salt).uniform(0, 1, (rows_, 3)).astype(F32), (e.astype(F64) ** 2).sum(1, keepdims=True).astype(F32)], 1)


def embeddings(s, n_own=N, n_str=N):
    q, k = randn(s, 52, B * n_own, E, scale=0.3), randn(s, 53, B * n_str, E, scale=0.3)
    return q, k, sides(s, 54, B * n_own, q), sides(s, 55, B * n_str, k)


def softcorr_case(s):
    q, k, qs, ks = embeddings(s)
    return dict(q=q, k=k, qside4=qs, kside4=ks, nbatch=B, nq=N, nk=N, mode=0, scale=1.0 / math.sqrt(E))


row("softcorr", "native.softcorr", softcorr_case, tuple_call("native.softcorr", ("corr4",)), ("corr4",))
row("softcorr[split]", "native.softcorr", softcorr_case, tuple_call("native.softcorr", ("corr4",), split=True), ("corr4",))
row("rigid_svd", "native.rigid_svd", lambda s: dict(src=randn(s, 56, B, N, 3), corr=randn(s, 57, B, N, 3), want_h=True),
    tuple_call("native.rigid_svd", ("R", "t", "R_ba", "t_ba", "H")), ("R", "t", "R_ba", "t_ba", "H"))
N_OWN, N_STR = 200, 330


def pairscore_case(s, **kw):
    own, strm, os4, ss4 = embeddings(s, N_OWN, N_STR)
    return dict(own=own, strm=strm, nbatch=B, n_own=N_OWN, n_str=N_STR, own_side4=os4, str_side4=ss4, **kw)


row("pairscore[corr]", "native.pairscore", lambda s: pairscore_case(s, op=0, score=0),
    tuple_call("native.pairscore", ("corr4",)), ("corr4",))
row("pairscore[stat]", "native.pairscore", lambda s: pairscore_case(s, op=1, score=0, want_argmax=True),
    tuple_call("native.pairscore", ("stat2", "argmax")), ("stat2", "argmax"))
row("pairscore[stat+split]", "native.pairscore", lambda s: pairscore_case(s, op=1, score=0, split=True),
    tuple_call("native.pairscore", ("stat2",)), ("stat2",))
row("pairscore[mass]", "native.pairscore",
    lambda s: pairscore_case(s, op=2, score=0, str_stat2=np.stack([randn(s, 58, B * N_STR) - 1.0,
                                                                    rng(s, 59).uniform(1.0, 50.0, B * N_STR).astype(F32)], -1)),
    tuple_call("native.pairscore", ("mass",)), ("mass",))
row("scoremass", "native.scoremass",
    lambda s: dict(score=randn(s, 60, B, N_OWN, 352) - 2.0, n_cols=N_STR,
                   row_stat2=np.stack([randn(s, 61, B * N_OWN), rng(s, 62).uniform(1.0, 50.0, B * N_OWN).astype(F32)], -1)),
    tuple_call("native.scoremass", ("col_stat2", "col_mass", "row_mass")), ("col_stat2", "col_mass", "row_mass"))
P_BASE, KEEP = 500, 200


def make_pairs_case(s):
    rs = rng(s, 63)
    perm = lambda n, m: np.stack([rs.permutation(n)[:m] for _ in range(B)]).astype(I32)
    return dict(cloud=np.ascontiguousarray(np.transpose(cloud(s, P_BASE, salt=64), (0, 2, 1))), R_ab=rotations(s, B, 30.0),
                t_ab=rs.uniform(-0.5, 0.5, (B, 3)), pick=perm(P_BASE, N), perm_src=perm(N, N), perm_tgt=perm(N, N), keep=KEEP)


row("make_pairs", "native.make_pairs", make_pairs_case, tuple_call("native.make_pairs", ("src", "tgt")), ("src", "tgt"),
    {"pick": (0, P_BASE), "perm_src": (0, N), "perm_tgt": (0, N)})
for _name, _variant in (("fps[resident]", 1), ("fps[streaming]", 2)):
    row(_name, "native.fps", lambda s: dict(xyz=cloud(s, 1000, salt=65), npoint=64),
        tuple_call("native.fps", ("idx", "points"), variant=_variant), ("idx", "points"))
row("fps[start]", "native.fps", lambda s: dict(xyz=cloud(s, 1000, salt=65), npoint=64, start=flags(s, (B,), 66, 1000)),
    tuple_call("native.fps", ("idx", "points")), ("idx", "points"), {"start": (0, 1000)})
row("farthest_point_sample", "native.farthest_point_sample", lambda s: dict(xyz=cloud(s, 1000, salt=65), npoint=64),
    tuple_call("native.farthest_point_sample", ("idx",)), ("idx",))
row("to_rows4", "native.to_rows4", lambda s: dict(x_cf=cloud(s)), tuple_call("native.to_rows4", ("rows",)), ("rows",))
row("rows4_pq", "native.rows4_pq", lambda s: dict(x_cf=cloud(s), wpq=randn(s, 67, 128, 32), bpq=randn(s, 68, 128)),
    tuple_call("native.rows4_pq", ("rows", "pq")), ("rows", "pq"))
row("icp", "native.icp", lambda s: dict(pick(("src", "tgt"), matched(s)), max_iterations=4, tolerance=0.0),
    lambda src, tgt, **kw: named(("final", "R", "t", "R_ba", "t_ba", "iters"), fn("native.icp")(src, tgt, **kw)),
    ("final", "R", "t", "R_ba", "t_ba", "iters"))
row("pose_step", "native.pose_step",
    lambda s: dict(R_i=rotations(s, B).astype(F32), t_i=randn(s, 69, B, 3, scale=0.1), cloud=cloud(s),
                   R_f=rotations(s, B, 9.0, salt=70).astype(F32), t_f=randn(s, 71, B, 3, scale=0.1)),
    tuple_call("native.pose_step", ("moved", "R_f", "t_f", "R_ba", "t_ba")), ("moved", "R_f", "t_f", "R_ba", "t_ba"))


def rank_values(s):
    v = randn(s, 72, 5, 700)
    v[3] = np.arange(700) % 7                              # a hundred copies of every value: the ties' order
    return v


row("rankselect", "native.rankselect", lambda s: dict(values=rank_values(s), K=123, want_mask=True),
    tuple_call("native.rankselect", ("order", "mask")), ("order", "mask"))
row("gather_rows", "native.gather_rows",
    lambda s: dict(x=randn(s, 73, 5 * 700, 64), idx=gather_idx(s, 5, 123, 700), nbatch=5, n_in=700,
                   via=np.stack([rng(s, 74 + c).permutation(700) for c in range(5)]).astype(I32)),
    tuple_call("native.gather_rows", ("out",)), ("out",), {"idx": (0, 700), "via": (0, 700)})


# =========================================================================================================== one cloud at a time

def knn_case(s, *extra):
    x = cloud(s)
    o = dict(xyz4=rows4(x), idx=knn_lists(x))
    if "normals" in extra:
        o["normals"] = unit(s)
    if "xyz" in extra:
        o["xyz"] = x
        del o["xyz4"]
    return o


LIST = {"idx": (0, N)}
row("grid_knn", "grid.grid_knn", lambda s: dict(xyz=cloud(s), k=K), dict_call("grid.grid_knn", ("idx", "d2")), ("idx", "d2"))
for _name, _order in (("grid_knn[cell order]", 1), ("grid_knn[index order]", 2)):
    row(_name, "grid.grid_knn", lambda s: dict(xyz=cloud(s), k=K), dict_call("grid.grid_knn", ("idx", "d2"), variant=_order), ("idx", "d2"))
row("plane.normals", "plane.normals", lambda s: dict(knn_case(s), viewpoint=randn(s, 75, B, 3) + 0.5),
    tuple_call("plane.normals", ("normals", "curvature")), ("normals", "curvature"), LIST)
row("fpfh.spfh", "fpfh.spfh", lambda s: knn_case(s, "normals"), tuple_call("fpfh.spfh", ("spfh",)), ("spfh",), LIST)


def spfh_bytes(s):
    h = np.zeros((B, N, 3, 16), np.uint8)
    h[..., :12] = histograms(s, N)
    return h.reshape(B, N, 48)


row("fpfh.fpfh", "fpfh.fpfh", lambda s: dict(knn_case(s), spfh=spfh_bytes(s)), tuple_call("fpfh.fpfh", ("fpfh",)), ("fpfh",), LIST)
row("color_gradient", "colored.color_gradient", lambda s: dict(knn_case(s, "normals"), inten=rng(s, 76).uniform(0, 1, (B, N)).astype(F32)),
    tuple_call("colored.color_gradient", ("gradient",)), ("gradient",), LIST)
row("stat_filter", "outlier.stat_filter", lambda s: dict(knn_case(s), std_ratio=1.0),
    dict_call("outlier.stat_filter", FILTER_OUT + ("mean_dist", "valid", "stats")), FILTER_OUT + ("mean_dist", "valid", "stats"), LIST)
row("radius_filter", "outlier.radius_filter", lambda s: dict(xyz=cloud(s), radius=RADIUS, nb_points=6),
    dict_call("outlier.radius_filter", FILTER_OUT + ("neighbours",)), FILTER_OUT + ("neighbours",))
row("radius_filter_grid", "radius.radius_filter_grid", lambda s: dict(xyz=cloud(s), radius=RADIUS, nb_points=6),
    dict_call("radius.radius_filter_grid", FILTER_OUT + ("neighbours",)), FILTER_OUT + ("neighbours",))
for _name, _order in (("radius_filter_grid[cell order]", 1), ("radius_filter_grid[index order]", 2)):
    row(_name, "radius.radius_filter_grid", lambda s: dict(xyz=cloud(s), radius=RADIUS, nb_points=6),
        dict_call("radius.radius_filter_grid", FILTER_OUT + ("neighbours",), order=_order), FILTER_OUT + ("neighbours",))
row("orient_tangent", "orient.orient_tangent", lambda s: knn_case(s, "normals", "xyz"),
    dict_call("orient.orient_tangent", ("oriented", "flip", "ref", "n_trees"), want_flip=True, want_ref=True, want_trees=True),
    ("oriented", "flip", "ref", "n_trees"), LIST)
VOXEL_OUT = ("points", "count", "point_voxel", "voxel_points")
row("voxel[scan]", "voxel.voxel_grid", lambda s: dict(xyz=cloud(s), voxel_size=0.2), dict_call("voxel.voxel_grid", VOXEL_OUT), VOXEL_OUT)
for _bits in (0, 4):
    row(f"voxel[sort,digit_bits={_bits}]", "voxel_sort.voxel_grid_sort", lambda s: dict(xyz=cloud(s), voxel_size=0.2),
        dict_call("voxel_sort.voxel_grid_sort", VOXEL_OUT + ("members", "voxel_start"), want_members=True, digit_bits=_bits),
        VOXEL_OUT + ("members", "voxel_start"))
RANSAC_OUT = ("plane", "inlier", "count", "point", "best_trial", "candidates", "refit_sums",
              "trial_status", "trial_picks", "trial_plane", "trial_count")
for _form in ("trial", "point"):
    row(f"plane_ransac[{_form}]", "segment.plane_ransac",
        lambda s: dict(xyz=cloud(s), distance_threshold=0.05, num_iterations=300, seed=5, mask=flags(s, (B, N), 77, 4).clip(0, 1)),
        dict_call("segment.plane_ransac", RANSAC_OUT, want_trials=True, variant=_form), RANSAC_OUT)
SPLIT_OUT = tuple(side + part for side in ("plane", "rest") for part in ("_points", "_count", "_index"))
row("split_rows", "segment.split_rows", lambda s: dict(xyz=cloud(s), inlier=flags(s, (B, N))),
    dict_call("segment.split_rows", SPLIT_OUT), SPLIT_OUT)
row("iss.select", "iss.select", lambda s: dict(xyz=cloud(s), keypoint=flags(s, (B, N))), dict_call("iss.select", FILTER_OUT), FILTER_OUT)


def labelled(s):
    labels = rng(s, 78).randint(-1, 9, (B, N)).astype(I32)
    sizes = np.zeros((B, N), I32)
    for c in range(B):
        sizes[c, :9] = np.bincount(labels[c][labels[c] >= 0], minlength=9)
    return dict(xyz=cloud(s), labels=labels, sizes=sizes)


row("largest_rows", "dbscan.largest_rows", labelled, dict_call("dbscan.largest_rows", FILTER_OUT), FILTER_OUT, {"labels": (-1, N)})

# ----------------------------------------------------------------------------------------------------------- the radius rows
SEARCH_OUT = ("count", "row_start", "total", "idx", "d2")
row("grid_radius", "radius.grid_radius", lambda s: dict(xyz=cloud(s), radius=RADIUS, capacity=CAP),
    dict_call("radius.grid_radius", SEARCH_OUT), SEARCH_OUT)
for _name, _form in (("grid_radius[wave]", 1), ("grid_radius[lane]", 2)):     # the ordering's two launch chains (bits 4-7)
    row(_name, "radius.grid_radius", lambda s: dict(xyz=cloud(s), radius=RADIUS, capacity=CAP),
        dict_call("radius.grid_radius", SEARCH_OUT, variant=_form << 4), SEARCH_OUT)
for _name, _order in (("grid_radius[cell order]", 1), ("grid_radius[index order]", 2)):
    row(_name, "radius.grid_radius", lambda s: dict(xyz=cloud(s), radius=RADIUS, capacity=CAP),
        dict_call("radius.grid_radius", SEARCH_OUT, variant=_order), SEARCH_OUT)
row("grid_radius[count]", "radius.grid_radius", lambda s: dict(xyz=cloud(s), radius=RADIUS),
    dict_call("radius.grid_radius", SEARCH_OUT[:3], want_idx=False), SEARCH_OUT[:3])
for _name, _variant in (("query.grid_knn[cell order]", 1), ("query.grid_knn[index order]", 2)):
    row(_name, "query.grid_knn", lambda s: dict(xyz=cloud(s), queries=queries(s), k=K),
        dict_call("query.grid_knn", ("idx", "d2"), variant=_variant), ("idx", "d2"))
for _name, _variant in (("query.grid_radius[cell order]", 1), ("query.grid_radius[index order]", 2)):
    row(_name, "query.grid_radius", lambda s: dict(xyz=cloud(s), queries=queries(s), radius=RADIUS, capacity=CAP),
        dict_call("query.grid_radius", SEARCH_OUT, variant=_variant), SEARCH_OUT)

CSR = (("idx", "row_start", "total"),)


def over_rows(s, *extra, want_d2=False):
    x, o = cloud_rows(s, want_d2)
    if "xyz4" in extra:
        o["xyz4"] = rows4(x)
    if "xyz" in extra:
        o["xyz"] = x
    if "normals" in extra:
        o["normals"] = unit(s)
    return o


row("rows.normals", "rows.normals", lambda s: dict(over_rows(s, "xyz4"), viewpoint=randn(s, 75, B, 3) + 0.5),
    tuple_call("rows.normals", ("normals", "curvature")), ("normals", "curvature"), LIST, CSR)
for _form in ("lane", "wave"):
    row(f"rows.spfh[{_form}]", "rows.spfh", lambda s: over_rows(s, "xyz4", "normals"),
        tuple_call("rows.spfh", ("spfh",), variant=_form), ("spfh",), LIST, CSR)
    row(f"rows.fpfh[{_form}]", "rows.fpfh", lambda s: dict(over_rows(s, "xyz4"), spfh=histograms(s, N)),
        tuple_call("rows.fpfh", ("fpfh",), variant=_form), ("fpfh",), LIST, CSR)
    row(f"cluster_rows[{_form}]", "dbscan.cluster_rows", lambda s: dict(over_rows(s, "xyz"), N=N, min_points=5),
        dict_call("dbscan.cluster_rows", ("labels", "n_clusters", "core", "sizes"), want_core=True, want_sizes=True, variant=_form),
        ("labels", "n_clusters", "core", "sizes"), LIST, CSR)
    row(f"iss.nms_rows[{_form}]", "iss.nms_rows",
        lambda s: dict(over_rows(s, want_d2=True), saliency=rng(s, 79).uniform(0.0, 1.0, (B, N)) * flags(s, (B, N), 80, 4).clip(0, 1),
                       min_neighbors=3, r2_nm=0.02),
        dict_call("iss.nms_rows", ("keypoint",), variant=_form), ("keypoint",), LIST, CSR)
    row(f"border.gap_rows[{_form}]", "border.gap_rows",
        lambda s: dict(pick(("row_start", "total"), over_rows(s)), angle=rng(s, 81).uniform(-math.pi, math.pi, (B, CAP)),
                       frame=flags(s, (B, N), 82, 4).clip(0, 1), min_neighbors=3),
        dict_call("border.gap_rows", ("gap", "flag"), variant=_form), ("gap", "flag"), None, (("angle", "row_start", "total"),))
row("iss.saliency_rows", "iss.saliency_rows", lambda s: dict(over_rows(s, "xyz4"), min_neighbors=4),
    dict_call("iss.saliency_rows", ("saliency", "eigen"), want_eigen=True), ("saliency", "eigen"), LIST, CSR)
row("border.angles_rows", "border.angles_rows", lambda s: dict(over_rows(s, "xyz4", "normals", want_d2=True), r2=0.02),
    dict_call("border.angles_rows", ("angle", "frame"), want_frame=True), ("angle", "frame"), LIST, CSR)
row("border.near_rows", "border.near_rows", lambda s: dict(over_rows(s), flag=flags(s, (B, N), 83, 8).clip(0, 1)),
    dict_call("border.near_rows", ("near",)), ("near",), LIST, CSR)
row("border.boundary_rows", "border.boundary_rows",
    lambda s: dict(over_rows(s, "xyz4", "normals"), min_neighbors=3, threshold=math.pi / 2),
    tuple_call("border.boundary_rows", ("flag", "gap")), ("flag", "gap"), LIST, CSR)
H2 = RADIUS * RADIUS
row("mls.weights_rows", "mls.weights_rows", lambda s: dict(over_rows(s, "xyz4", "normals"), sqr_gauss_param=H2),
    dict_call("mls.weights_rows", ("weight", "origin", "w_self", "frame")), ("weight", "origin", "w_self", "frame"), LIST, CSR)
FIT_OUT = ("points", "fit", "normals", "coeffs")
for _form in ("plain", "transpose"):
    row(f"mls.fit_rows[{_form}]", "mls.fit_rows",
        lambda s: dict(over_rows(s, "xyz4", "normals"), weight=rng(s, 84).uniform(0.05, 1.0, (B, CAP)),
                       origin=rng(s, 85).normal(size=(B, N, 3)) * 0.01, w_self=rng(s, 86).uniform(0.5, 1.0, (B, N)),
                       frame=flags(s, (B, N), 87, 8).clip(0, 1)),
        dict_call("mls.fit_rows", FIT_OUT, variant=_form), FIT_OUT, LIST, CSR)
row("mls.smooth_rows", "mls.smooth_rows", lambda s: dict(over_rows(s, "xyz4", "normals"), sqr_gauss_param=H2),
    dict_call("mls.smooth_rows", FIT_OUT), FIT_OUT, LIST, CSR)

# ------------------------------------------------------------------------------------------- features at positions (support)
OVER = {"idx": (0, N), "self_index": (-1, N)}
row("support.normals", "support.normals", lambda s: dict(support_case(s)[2], viewpoint=randn(s, 75, B, 3) + 0.5),
    tuple_call("support.normals", ("normals", "curvature")), ("normals", "curvature"), OVER, CSR)
for _form in ("lane", "wave"):
    row(f"support.spfh[{_form}]", "support.spfh",
        lambda s: dict(support_case(s)[2], normals=unit(s), centre_normals=unit(s, M, salt=88)),
        tuple_call("support.spfh", ("spfh",), variant=_form), ("spfh",), OVER, CSR)
row("support.needed", "support.needed", lambda s: support_case(s)[2],
    dict_call("support.needed", FILTER_OUT + ("slot",)), FILTER_OUT + ("slot",), OVER, CSR)
row("support.fpfh", "support.fpfh",
    lambda s: dict(support_case(s)[2], support_spfh=histograms(s, N), centre_spfh=histograms(s, M, salt=89),
                   slot=np.stack([rng(s, 90 + c).permutation(N) for c in range(B)]).astype(I32)),
    tuple_call("support.fpfh", ("fpfh",)), ("fpfh",), dict(OVER, slot=(0, N)), CSR)

# ================================================================================================================ two clouds
LOOP = dict(max_iterations=4, rel_fitness=0.0, rel_rmse=0.0)
for _search in ("scan", "grid"):
    _kw = {"search": _search}
    row(f"nn_score[{_search}]", "score.nn_score", lambda s: pair_args(s),
        dict_call("score.nn_score", ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse"), **_kw),
        ("nn_idx", "nn_d2", "inliers", "sum_d2", "fitness", "rmse"))
    row(f"refine[{_search}]", "refine.refine", lambda s: pair_args(s, **LOOP), dict_call("refine.refine", POSE_OUT, **_kw), POSE_OUT)
    row(f"refine_plane[{_search}]", "plane.refine_plane", lambda s: pair_args(s, "tgt_normals", **LOOP),
        dict_call("plane.refine_plane", POSE_OUT, **_kw), POSE_OUT)
    row(f"refine_gicp[{_search}]", "gicp.refine_gicp",
        lambda s: dict(pair_args(s, "tgt_normals", **LOOP), src_normals=unit(s, NS, salt=91)),
        dict_call("gicp.refine_gicp", POSE_OUT, **_kw), POSE_OUT)
    row(f"refine_colored[{_search}]", "colored.refine_colored",
        lambda s: pair_args(s, "src_intensity", "tgt_intensity", "tgt_normals", "tgt_gradient", **LOOP),
        dict_call("colored.refine_colored", POSE_OUT, **_kw), POSE_OUT)
    row(f"refine_robust[{_search}]", "robust.refine_robust", lambda s: pair_args(s, "tgt_normals", loss="tukey", k=0.05, **LOOP),
        dict_call("robust.refine_robust", POSE_OUT, **_kw), POSE_OUT)
    row(f"information[{_search}]", "robust.information", lambda s: pair_args(s),
        dict_call("robust.information", POSE_OUT + ("information",), **_kw), POSE_OUT + ("information",))
row("feat_nn", "match.feat_nn", lambda s: dict(a=np.abs(randn(s, 92, B, 33, NS)), b=np.abs(randn(s, 93, B, 33, NT))),
    dict_call("match.feat_nn", ("nn_idx", "nn_d2", "rev_idx"), mutual=True, want_rev=True), ("nn_idx", "nn_d2", "rev_idx"))
CORR = {"corr": (0, NT)}
row("ransac", "match.ransac", lambda s: dict(matched(s), max_dist=0.05, trials=512, seed=3),
    dict_call("match.ransac", ("R", "t", "best_trial", "inliers", "pairs", "trial_status", "trial_picks", "trial_pose", "trial_inliers"),
              want_trials=True),
    ("R", "t", "best_trial", "inliers", "pairs", "trial_status", "trial_picks", "trial_pose", "trial_inliers"), CORR)
FGR_OUT = ("R", "t", "pairs", "tuples", "used", "status", "tuple_list", "norm", "pose64", "sums", "mu")
row("fgr", "fgr.fgr", lambda s: dict(matched(s), max_tuples=200, iterations=6, tuple_trials=4000, seed=3),
    dict_call("fgr.fgr", FGR_OUT, want_stages=True), FGR_OUT, CORR)

# ============================================================================================================ the pose graph
GRAPH_OUT = ("R", "t", "weight", "kept", "residual", "iterations", "converged")
RING_K = 8


def graphs(s):
    """Two rings of posegraph_restated (its recipe at two seeds a table seed): the same nodes and edge lists, other poses."""
    rc = [pgr.ring(seed=10 * s + g) for g in range(2)]
    st = lambda f, dt: np.stack([np.asarray(f(r), dt) for r in rc])
    return dict(R=st(lambda r: r["R0"], F64), t=st(lambda r: r["t0"], F64), src=st(lambda r: r["graph"].src, I32),
                dst=st(lambda r: r["graph"].dst, I32), R_edge=st(lambda r: r["graph"].Re, F64), t_edge=st(lambda r: r["graph"].te, F64),
                information=st(lambda r: r["graph"].info, F64), uncertain=st(lambda r: r["graph"].unc, I32),
                max_correspondence_distance=pgr.MCD)


for _name, _form in (("posegraph[lds]", "FORM_LDS"), ("posegraph[global]", "FORM_GLOBAL")):
    row(_name, "posegraph.optimize", graphs,
        (lambda form: lambda **kw: pick(GRAPH_OUT, fn("posegraph.optimize")(
            criteria=dict(max_iteration=4), variant=getattr(mod("posegraph"), form), **kw)))(_form),
        GRAPH_OUT, {"src": (0, RING_K), "dst": (0, RING_K)})


# ====================================================================================== what synchronises, and the coverage
# name -> (file of vcr-net_amd, the source line that documents the host read).  Nothing here is a staged call: each is a
# composite in front of staged calls that reads one number back, and says so.
SYNCHRONISES = {
    "radius.search_radius": ("radius.py", 'capacity = int(counted["total"].max())             # the ONE host synchronisation'),
    "radius._hybrid": ("radius.py", "capacity = int(total.max())                        # the ONE host synchronisation"),
    "iss.compute_iss_keypoints": ("iss.py", "res = model_resolution(xyz).cpu()                   # the host synchronisation of the default radii"),
    "voxel.unpad": ("voxel.py", "counts = count.tolist()"),
    "posegraph.check_edges": ("posegraph.py", "bad = ((s >= 0) & ((s >= K) | (d < 0) | (d >= K) | (s == d))).nonzero()[0].tolist()"),
    "module.register_sampled": ("module.py", "counts = torch.cat(counts).cpu()                                           # the one synchronisation"),
    # (the fused forward is staged and capturable in steady state -- tests/test_hip_forward.py holds that:
    # test_runs_on_the_callers_stream, test_forward_captures_into_a_hip_graph; it is listed for _pack's drain of the device when
    # the weights CHANGED, and has no row here because those two tests are its row)
    "module.VCRNet._forward_fused": ("module.py", "torch.cuda.synchronize(dev)"),
}

# The functions without the _guarded decorator that reach native.call, extension.call_with_workspace or an entry point of the
# library themselves, or chain staged calls without anything else: found by reading.
UNDECORATED = ("native.knn_order", "native.farthest_point_sample", "mls.smooth_rows", "border.boundary_rows", "plane.refine_plane",
               "gicp.refine_gicp", "module.VCRNet._forward_fused")


def by_name():
    return {r.name: r for r in ROWS}


# ============================================================================================== the public composite calls
# (name, make, call): the functions of vcrnet_amd.__all__ -- staged calls with torch plumbing between them, some documented to
# synchronise once.  call returns whatever the function returns; the test compares every tensor in it.
Composite = namedtuple("Composite", "name make call")
COMPOSITES = []


def composite(name, make, call):
    COMPOSITES.append(Composite(name, functools.lru_cache(maxsize=None)(make), call))


def public(name, **fixed):
    def call(**kw):
        import vcrnet_amd
        return getattr(vcrnet_amd, name)(**kw, **fixed)
    return call


def one_cloud(s, **kw):
    return dict(xyz=cloud(s), **kw)


def overlapping(s, k=3):
    """k views of one cloud of N points, each under a pose of a few degrees and with its own noise."""
    base = cloud(s)[0].astype(F64)
    R, rs = rotations(s, k, 3.0, salt=94), rng(s, 95)
    views = [R[i] @ base + rs.uniform(-0.02, 0.02, (3, 1)) + rs.normal(0, 0.002, base.shape) for i in range(k)]
    return dict(clouds=np.stack(views).astype(F32))


@functools.lru_cache(maxsize=None)
def forward_net():
    import test_hip_forward
    return test_hip_forward.build_net()[0]


for _cap in (CAP, None):
    _tag = "capacity" if _cap else "counted"
    composite(f"search_radius[{_tag}]", lambda s: one_cloud(s, radius=RADIUS), public("search_radius", capacity=_cap, want_d2=True))
    composite(f"cluster_dbscan[{_tag}]", lambda s: one_cloud(s, eps=RADIUS, min_points=5),
              public("cluster_dbscan", capacity=_cap, want_core=True, want_sizes=True))
    composite(f"compute_iss_keypoints[{_tag}]", lambda s: one_cloud(s, salient_radius=RADIUS, non_max_radius=0.8 * RADIUS),
              public("compute_iss_keypoints", capacity=_cap, want_flag=True, want_saliency=True))
    composite(f"smooth_mls[{_tag}]", lambda s: one_cloud(s, radius=RADIUS), public("smooth_mls", capacity=_cap, want_normals=True))
    composite(f"compute_boundary_points[{_tag}]", lambda s: one_cloud(s, radius=RADIUS),
              public("compute_boundary_points", capacity=_cap, want_flag=True, want_gap=True))
composite("search_radius[max_nn]", lambda s: one_cloud(s, radius=RADIUS), public("search_radius", capacity=CAP, max_nn=K))
composite("search_radius[queries]", lambda s: one_cloud(s, radius=RADIUS, queries=queries(s)), public("search_radius", capacity=CAP))
composite("compute_iss_keypoints[default radii]", one_cloud, public("compute_iss_keypoints", capacity=CAP))
composite("search_knn", lambda s: one_cloud(s, k=K), public("search_knn", want_d2=True))
composite("search_knn[queries]", lambda s: one_cloud(s, k=K, queries=queries(s)), public("search_knn", want_d2=True))
for _search in ("knn", "grid"):
    composite(f"estimate_normals[{_search}]", lambda s: one_cloud(s, k=K),
              public("estimate_normals", want_curvature=True, want_idx=True, search=_search))
    composite(f"compute_fpfh_feature[{_search}]", lambda s: one_cloud(s, k=K), public("compute_fpfh_feature", want_normals=True, search=_search))
    composite(f"remove_statistical_outlier[{_search}]", lambda s: one_cloud(s, nb_neighbors=K, std_ratio=1.0),
              public("remove_statistical_outlier", search=_search))
for _search in ("scan", "grid"):
    composite(f"remove_radius_outlier[{_search}]", lambda s: one_cloud(s, nb_points=6, radius=RADIUS),
              public("remove_radius_outlier", search=_search))
    composite(f"voxel_down_sample[{'scan' if _search == 'scan' else 'sort'}]", lambda s: one_cloud(s, voxel_size=0.2),
              public("voxel_down_sample", method="scan" if _search == "scan" else "sort"))
    composite(f"score_registration[{_search}]", lambda s: pair_args(s), public("score_registration", symmetric=True, want_nn=True, search=_search))
    for _method in ("point_to_point", "point_to_plane", "generalized"):
        composite(f"refine_registration[{_method},{_search}]", lambda s: pair_args(s, **LOOP),
                  public("refine_registration", method=_method, normal_k=K, search=_search))
    composite(f"refine_registration_colored[{_search}]",
              lambda s: dict(pair_args(s, **LOOP), src_colors=pair(s)["src_intensity"], tgt_colors=pair(s)["tgt_intensity"]),
              public("refine_registration_colored", normal_k=K, gradient_k=K, search=_search))
    composite(f"refine_registration_robust[{_search}]", lambda s: pair_args(s, **LOOP),
              public("refine_registration_robust", loss="huber", k=0.05, normal_k=K, search=_search))
    composite(f"information_matrix[{_search}]", lambda s: pair_args(s), public("information_matrix", want_score=True, search=_search))
composite("estimate_normals[radius]", lambda s: one_cloud(s, radius=RADIUS), public("estimate_normals", search="radius", capacity=CAP))
composite("compute_fpfh_feature[radius]", lambda s: one_cloud(s, radius=RADIUS), public("compute_fpfh_feature", search="radius", capacity=CAP))
composite("compute_fpfh_feature[queries]", lambda s: one_cloud(s, radius=RADIUS, queries=queries(s)),
          public("compute_fpfh_feature", search="radius", capacity=CAP))
composite("largest_cluster", labelled, public("largest_cluster"))
composite("segment_plane", lambda s: one_cloud(s, distance_threshold=0.05), public("segment_plane", num_iterations=300, seed=5))
composite("split_by_plane", lambda s: one_cloud(s, inlier=flags(s, (B, N))), public("split_by_plane"))
composite("segment_planes", lambda s: one_cloud(s, distance_threshold=0.05),
          public("segment_planes", max_planes=3, min_inliers=10, num_iterations=200, seed=5))
composite("orient_normals_consistent_tangent_plane", lambda s: one_cloud(s, normals=unit(s)),
          public("orient_normals_consistent_tangent_plane", k=K, want_flip=True, want_ref=True, want_trees=True))
composite("model_resolution", one_cloud, public("model_resolution"))
composite("centred", one_cloud, public("centred"))
composite("uncentred_pose",
          lambda s: dict(R=rotations(s, B).astype(F32), t=randn(s, 69, B, 3), c_src=randn(s, 96, B, 3), c_tgt=randn(s, 97, B, 3)),
          public("uncentred_pose"))
composite("compute_point_cloud_distance", lambda s: pick(("src", "tgt"), pair(s)), public("compute_point_cloud_distance", want_index=True))
composite("compute_color_gradient", lambda s: one_cloud(s, normals=unit(s), colors=rng(s, 76).uniform(0, 1, (B, 3, N)).astype(F32)),
          public("compute_color_gradient", k=K))
composite("farthest_point_sample", lambda s: dict(xyz=cloud(s, 1000, salt=65)), public("farthest_point_sample", npoint=64))
composite("match_features", lambda s: dict(src_feat=np.abs(randn(s, 92, B, 33, NS)), tgt_feat=np.abs(randn(s, 93, B, 33, NT))),
          public("match_features", mutual=True, want_d2=True))
composite("ransac_correspondences", lambda s: dict(matched(s), max_dist=0.05), public("ransac_correspondences", trials=512, seed=3))
composite("fast_global_registration", matched, public("fast_global_registration", max_tuples=200, iterations=6, tuple_trials=4000, seed=3))
for _method in ("ransac", "fgr"):
    composite(f"register_features[{_method}]", lambda s: dict(pick(("src", "tgt"), matched(s)), max_dist=0.05),
              public("register_features", k=K, trials=512, seed=3, method=_method, refine=0.05))
composite("optimize_pose_graph", graphs, public("optimize_pose_graph", criteria=dict(max_iteration=4)))
composite("pose_graph_from_clouds", overlapping, public("pose_graph_from_clouds", max_dist_coarse=0.15, max_dist_fine=0.07, max_iterations=4, normal_k=K))
composite("register_multiway", overlapping,
          public("register_multiway", max_dist_coarse=0.15, max_dist_fine=0.07, max_iterations=4, normal_k=K, criteria=dict(max_iteration=4)))
def sampled(**kw):
    import torch
    with torch.no_grad():
        return mod("module").register_sampled(forward_net(), npoint=128, iter=2, score=0.05, refine=0.05, voxel=0.02, **kw)


composite("register_sampled", lambda s: pick(("src", "tgt"), matched(s)), sampled)
