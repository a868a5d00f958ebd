"""vcr_grid_knn_f32 on the GPU: the exact kNN on a uniform grid (include/vcr_hip_grid.h).

The result is defined bit for bit, so every comparison here is exact and on int32 views: idx, and d2's bits, against the numpy
brute force (tests/grid_restated.py: ``knn`` is the definition).  Every output buffer, and the workspace, is prefilled with a
garbage byte and carries a guard band: every slot must have been written, and nothing behind it.  Every forced cell, every
variant, every batch and every run must return the same bits."""
import functools

import numpy as np
import pytest
import torch

import fpfh_restated as fr
import grid_restated as gr
import outlier_restated as orr
import plane_restated as pr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import fpfh, grid, native, outlier, plane
    return grid, native, plane, fpfh, outlier


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run(xyz, k, cell=0.0, variant=0, want_d2=True):
    """numpy [B,3,N] (or [3,N]) in -> (idx [B,N,k], d2 bits [B,N,k] or None); all of every output must have been overwritten, none
    of the band behind it."""
    grid = mods()[0]
    xyz = xyz[None] if xyz.ndim == 2 else xyz
    o = grid.grid_knn(dev(xyz), k, cell, want_d2=want_d2, variant=variant, guard=GUARD, prefill=SENTINEL_BYTE)
    torch.cuda.synchronize()
    for name in ("idx", "d2") if want_d2 else ("idx",):
        raw, n = o["_raw"][name], o[name].numel()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * 4 and (band == SENTINEL_BYTE).all(), (name, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, 4)
        assert not (body == SENTINEL_BYTE).all(axis=1).any(), (name, "element left unwritten")
    return o["idx"].cpu().numpy(), bits(o["d2"].cpu().numpy()) if want_d2 else None


@functools.lru_cache(maxsize=None)
def case(name, N, k, seed=0):
    """(xyz [3,N], the definition's idx and d2 bits): computed once, shared, never written to."""
    xyz = gr.RECIPES[name](N, seed)
    want = gr.knn(xyz, k)
    for a in (xyz,) + want:
        a.setflags(write=False)
    return xyz, want[0], want[1]


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "idx", np.argwhere(got[0] != want[0])[:5])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "d2", np.argwhere(got[1] != want[1])[:5])


@pytest.mark.parametrize("N,k", [(1, 1), (1, 20), (2, 1), (21, 20), (31, 30), (63, 62), (255, 20), (256, 30), (257, 1), (257, 62),
                                 (1025, 20), (2049, 30), (5, 20)])
def test_sizes_against_the_definition(N, k):
    """One point; N = k + 1; a workgroup's edge (255 / 256 / 257); 1 025 and 2 049 points; k + 1 > N (short rows)."""
    xyz, idx, d2 = case("random", N, k)
    got = run(xyz, k)
    assert got[0].min() >= 0 and got[0].max() < N
    assert_same((got[0][0], got[1][0]), (idx, d2), (N, k))
    if k + 1 > N:
        own = np.arange(N)[:, None]
        assert (got[0][0][:, N - 1:] == own).all() and (got[1][0][:, N - 1:] == gr.INF_BITS).all()


@pytest.mark.parametrize("name", sorted(gr.RECIPES))
@pytest.mark.parametrize("N,k", [(300, 20), (4096, 30)])
def test_content_against_the_definition(name, N, k):
    """The CPU recipes: lattice ties and points ON faces, flat, collinear, all points equal, copies, NaN / inf at point 0 and
    elsewhere, a far outlier (nearly every point in one cell: the brute force for that cloud), a tiny and a clustered cloud."""
    xyz, idx, d2 = case(name, N, k)
    got = run(xyz, k)
    assert_same((got[0][0], got[1][0]), (idx, d2), (name, N, k))
    if name.startswith("nonfinite"):
        bad = np.flatnonzero(~gr.finite(xyz))
        assert len(bad) >= 2 and (got[0][0][bad] == bad[:, None]).all() and not np.isin(got[0][0][gr.finite(xyz)], bad).any()


@pytest.mark.parametrize("name", ["random", "lattice", "copies", "nonfinite", "outlier"])
def test_every_cell_and_every_variant_returns_the_same_bits(name):
    """Every forced edge from "every point its own cell" (widened to the budget) to "one cell", the lattice's own 1 and 2, both
    query orders; and without d2 the same idx."""
    N, k = 1025, 20
    xyz, idx, d2 = case(name, N, k)
    grid = mods()[0]
    for cell in [0.0] + gr.forced_cells(xyz):
        for variant in (0, grid.variant(1), grid.variant(2)):
            got = run(xyz, k, cell, variant)
            assert_same((got[0][0], got[1][0]), (idx, d2), (name, cell, variant))
    alone = run(xyz, k, want_d2=False)
    assert alone[1] is None and np.array_equal(alone[0][0], idx)


def test_a_batch_is_its_clouds_alone_and_a_call_repeats_itself():
    """B = 3, three different clouds (uniform, lattice, one with non-finite points)."""
    N, k = 777, 20
    clouds = [case(n, N, k) for n in ("random", "lattice", "nonfinite")]
    xyz = np.stack([c[0] for c in clouds])
    first = run(xyz, k)
    again = run(xyz, k)
    assert_same(again, first, "the same call twice")
    for b, (x, idx, d2) in enumerate(clouds):
        assert_same((first[0][b], first[1][b]), (idx, d2), ("in the batch", b))
        assert_same(run(x, k), (idx[None], d2[None]), ("alone", b))


def test_a_translation_that_is_exact_returns_the_same_bits():
    """A cloud on a 1/1024 lattice moved by (1024, -512, 256): every coordinate and every difference stays exact in fp32."""
    N, k = 2000, 20
    rs = np.random.RandomState(9)
    x = (rs.randint(0, 1024, (3, N)) / 1024.0).astype(np.float32)
    far = (x + np.asarray([[1024.0], [-512.0], [256.0]], np.float32)).astype(np.float32)
    assert np.array_equal((far - np.asarray([[1024.0], [-512.0], [256.0]], np.float32)), x)
    want = gr.knn(x, k)
    assert_same(tuple(a[0] for a in run(x, k)), want, "at the origin")
    assert_same(tuple(a[0] for a in run(far, k)), want, "moved")
    native = mods()[1]
    old = native.knn(native.to_rows4(dev(far[None])), None, k).cpu().numpy()[0]      # (the expansion does cancel there)
    assert (np.sort(old, 1) != np.sort(want[0], 1)).any()


@pytest.mark.parametrize("N,shape", [(70001, "uniform"), (131072, "uniform"), (70001, "sphere"), (131072, "sphere")])
def test_large_clouds(N, shape):
    """70 001 and 131 072 points, uniform in a cube and on a sphere's surface: 256 sampled rows against the brute force."""
    k = 20
    xyz = gr.random_cloud(N, 11) if shape == "uniform" else gr.sphere(N, 12)
    rows = np.random.RandomState(13).choice(N, 256, replace=False)
    want = gr.knn(xyz, k, rows)
    got = run(xyz, k)
    assert got[0].min() >= 0 and got[0].max() < N
    assert_same((got[0][0][rows], got[1][0][rows]), want, (N, shape))
    assert not (got[0][0] == np.arange(N)[:, None]).any()


# ------------------------------------------------------------------------------------------------------------- the consumers

def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_estimate_normals_on_the_grid():
    """search="grid": the neighbours are the definition's, the normals those of plane_restated on that idx, at the tolerances
    tests/test_hip_normals.py holds the kernel to; search="knn" is the old path bit for bit."""
    import vcrnet_amd
    grid, native, plane, _, _ = mods()
    B, N, k = 2, 1000, 20
    x = np.stack([pr.jittered_torus(100 * N + b, N) for b in range(B)])
    xd = dev(x)
    nrm, cur, idx = vcrnet_amd.estimate_normals(xd, k, want_curvature=True, want_idx=True, search="grid")
    assert _eq(idx, vcrnet_amd.search_knn(xd, k))
    idx, n, c = idx.cpu().numpy(), nrm.cpu().numpy(), cur.cpu().numpy()
    for b in range(B):
        assert np.array_equal(idx[b], gr.knn(x[b], k)[0])
        C = pr.covariances(x[b], idx[b])
        lam, V = np.linalg.eigh(C)
        nd = n[b].astype(np.float64).T
        norm = np.abs(np.sqrt((nd * nd).sum(1)) - 1).max()
        rq = np.einsum("ni,nij,nj->n", nd, C, nd) / (nd * nd).sum(1) - lam[:, 0]
        apart = lam[:, 1] - lam[:, 0] >= 2.0 ** -10 * lam[:, 2]
        ref = np.stack([pr.orient(V[i, :, 0].astype(np.float32)) for i in range(N)])
        dn = np.abs(n[b].T - ref)[apart].max()
        c_ref = lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        dc = np.abs(c[b].astype(np.float64) - c_ref) - 2.0 ** -22 * c_ref
        print(f"grid normals cloud {b}: ||n|-1| {norm:.2e}  rq / l2 {(rq / lam[:, 2]).max():.2e}  |n - n_ref| {dn:.2e}  dc {dc.max():.2e}")
        assert norm <= 2.0 ** -22 and (rq <= 2.0 ** -40 * lam[:, 2]).all() and 1 - apart.mean() <= 0.01
        assert dn <= 2.0 ** -22 and (dc <= 2.0 ** -40).all()
    xyz4 = native.to_rows4(xd)
    old_idx = native.knn(xyz4, None, k)
    old_n, old_c = plane.normals(xyz4, old_idx, want_curvature=True)
    for got in (vcrnet_amd.estimate_normals(xd, k, want_curvature=True, want_idx=True, search="knn"),
                vcrnet_amd.estimate_normals(xd, k, want_curvature=True, want_idx=True)):
        assert _eq(got[0], old_n) and _eq(got[1], old_c) and _eq(got[2], old_idx)


def test_compute_fpfh_feature_on_the_grid():
    """search="grid": one search serves the normals and the features; the histograms are fpfh_restated's on that idx, as
    tests/test_hip_fpfh.py holds the kernels to it (the first group up to its excluded pairs, the second pass bit for bit);
    search="knn" is the old path bit for bit."""
    import vcrnet_amd
    grid, native, plane, fpfh, _ = mods()
    B, N, k = 2, 1000, 30
    x = fr.cloud(B, N)
    xd = dev(x)
    feat, nrm, idx = vcrnet_amd.compute_fpfh_feature(xd, None, k, want_normals=True, want_idx=True, search="grid")
    assert _eq(idx, vcrnet_amd.search_knn(xd, k))
    xyz4 = native.to_rows4(xd)
    assert _eq(nrm, plane.normals(xyz4, idx, want_curvature=False)[0])
    sp = fpfh.spfh(xyz4, nrm, idx)
    assert _eq(feat, fpfh.fpfh(xyz4, idx, sp))
    given = vcrnet_amd.compute_fpfh_feature(xd, nrm, k, search="grid")               # with the normals given: its own search
    assert _eq(given, feat)
    idx, nrm, sp, feat = (t.cpu().numpy() for t in (idx, nrm, sp, feat))
    e = n = 0
    for b in range(B):
        assert np.array_equal(idx[b], gr.knn(x[b], k)[0])
        p = fr.pairs(x[b], nrm[b], idx[b])
        ref = fr.pack(p).reshape(-1, 3, 16).astype(np.int64)
        got = sp[b].reshape(-1, 3, 16).astype(np.int64)
        ex = fr.excluded(p).sum(1)
        assert np.array_equal(got[ex == 0], ref[ex == 0]) and np.array_equal(got[:, 1:], ref[:, 1:])
        assert np.array_equal(got[:, 0, fr.BINS:], ref[:, 0, fr.BINS:])
        assert (np.abs(got[:, 0, :fr.BINS] - ref[:, 0, :fr.BINS]).max(1) <= ex).all()
        assert (got[:, 0, :fr.BINS].sum(1) == ref[:, 0, :fr.BINS].sum(1)).all()
        e, n = e + int(ex.sum()), n + int(p["counted"].sum())
        assert np.array_equal(bits(feat[b]), bits(fr.fpfh(x[b], idx[b], sp[b])))
    assert n == B * N * k and e <= 0.001 * n
    old_idx = native.knn(xyz4, None, k)
    old_n = plane.normals(xyz4, old_idx, want_curvature=False)[0]
    old = fpfh.fpfh(xyz4, old_idx, fpfh.spfh(xyz4, old_n, old_idx))
    for got in (vcrnet_amd.compute_fpfh_feature(xd, None, k, want_normals=True, want_idx=True, search="knn"),
                vcrnet_amd.compute_fpfh_feature(xd, None, k, want_normals=True, want_idx=True)):
        assert _eq(got[0], old) and _eq(got[1], old_n) and _eq(got[2], old_idx)


def _ulps(a, b):
    return np.abs(orr.bits(np.asarray(a)).astype(np.int64) - orr.bits(np.asarray(b)).astype(np.int64))


def test_remove_statistical_outlier_on_the_grid():
    """search="grid": the filter on the definition's nb_neighbors - 1 other points, stage by stage as tests/test_hip_outlier.py
    holds the kernel to outlier_restated (mean distance within 1 ulp, mu exact, sigma and thr within 2 ulps, the kept set from
    the device's own mean distances and threshold); search="knn" is the old path bit for bit."""
    import vcrnet_amd
    grid, native, _, _, outlier = mods()
    B, N, nb, ratio = 2, 2000, 20, 1.5
    x = np.stack([orr.blob_far(31 + b, N)[0][0] for b in range(B)])
    xd = dev(x)
    points, count, index = vcrnet_amd.remove_statistical_outlier(xd, nb, ratio, search="grid")
    idx = vcrnet_amd.search_knn(xd, nb - 1)
    xyz4 = native.to_rows4(xd)
    o = outlier.stat_filter(xyz4, idx, ratio, want_trace=True)
    assert _eq(points, o["points"]) and _eq(count, o["count"]) and _eq(index, o["index"])
    got = {name: o[name].cpu().numpy() for name in ("points", "count", "index", "mean_dist", "valid", "stats")}
    idx = idx.cpu().numpy()
    for b in range(B):
        assert np.array_equal(idx[b], gr.knn(x[b], nb - 1)[0])
        md, want_md = got["mean_dist"][b], orr.mean_dist_fast(x[b], idx[b])
        assert np.isfinite(md).all() and np.isfinite(want_md).all() and (_ulps(md, want_md) <= 1).all()
        d = orr.decide(md, ratio)
        mu, sigma, thr = got["stats"][b]
        assert got["valid"][b] == d["valid"] and _ulps(mu, d["mu"]) == 0
        assert _ulps(sigma, d["sigma"]) <= 2 and _ulps(thr, d["thr"]) <= 2
        want = orr.compact(x[b], md.astype(np.float64) <= thr)
        assert 0 < want["count"] < N
        for name in want:
            assert np.array_equal(orr.bits(got[name][b]), orr.bits(want[name])), (name, b)
    old = outlier.stat_filter(xyz4, native.knn(xyz4, None, nb - 1), ratio, want_trace=False)
    for res in (vcrnet_amd.remove_statistical_outlier(xd, nb, ratio, search="knn"), vcrnet_amd.remove_statistical_outlier(xd, nb, ratio)):
        assert _eq(res[0], old["points"]) and _eq(res[1], old["count"]) and _eq(res[2], old["index"])


def test_register_features_hands_the_search_to_both_feature_calls():
    """search="grid" through register_features, RANSAC and FGR: the correspondences are those of the two grid-searched feature
    sets; the default's are those of search="knn"."""
    import vcrnet_amd
    x = fr.cloud(2, 600)
    src = dev(x)
    tgt = dev(np.ascontiguousarray(x[:, :, ::-1][:, :, :500]) + np.float32(0.125))
    want = {s: vcrnet_amd.match_features(vcrnet_amd.compute_fpfh_feature(src, None, k=20, search=s),
                                         vcrnet_amd.compute_fpfh_feature(tgt, None, k=20, search=s), mutual=True) for s in ("knn", "grid")}
    for kw in (dict(method="ransac", trials=2000), dict(method="fgr")):
        got = vcrnet_amd.register_features(src, tgt, 0.05, k=20, search="grid", **kw)
        assert torch.equal(got["corr"], want["grid"]) and (got["corr"] >= 0).any()
        assert torch.equal(vcrnet_amd.register_features(src, tgt, 0.05, k=20, **kw)["corr"], want["knn"])
    far = vcrnet_amd.register_features(src, tgt, 0.05, k=20, search="grid", centre=True, trials=2000)
    assert far["corr"].shape == want["grid"].shape
