"""vcr_query_knn_f32 and vcr_query_radius_f32 on the GPU: the k nearest points and all points within a radius of ANY query
positions, searched on the points' uniform grid (include/query/vcr_hip_query.h).

The result is defined bit for bit, so every comparison here is exact and on int32 / int64 views: idx and d2's bits, count,
row_start and total against the numpy brute force (tests/query_restated.py: ``knn`` and ``radius_rows`` are the definition), and
against the searches that existed before on the same device.  Every output buffer, and the workspace, is prefilled with the byte
0x5A and carries a guard band of 64 elements: every slot must have been written, and nothing behind it.  Every forced cell, both
query orders, every batch and every run must return the same bits."""
import functools

import numpy as np
import pytest
import torch

import grid_restated as gr
import outlier_restated as orr
import query_restated as qr
import radius_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
K = 20
KNN_OUT = ("idx", "d2")
RADIUS_OUT = ("count", "row_start", "total", "idx", "d2")


def mod():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import query
    return query


def dev(x):
    x = np.asarray(x)
    return torch.from_numpy(np.array(x[None] if x.ndim == 2 else x, order="C")).cuda()      # (a copy: the shared cases are read-only)


def fetch(o, names):
    """dict of torch -> dict of numpy; all of every output must have been overwritten, none of the band behind it."""
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in names}
    for k in names:
        raw, n = o["_raw"][k], o[k].numel()
        size = raw.element_size()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * size and (band == SENTINEL_BYTE).all(), (k, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
        assert not (body == SENTINEL_BYTE).all(axis=1).any(), (k, "element left unwritten")
    return out


def run_knn(xyz, queries, k=K, cell=0.0, variant=0, want_d2=True):
    """numpy [B,3,N] / [B,3,M] (or one cloud each) in -> (idx int32 [B,M,k], d2 bits int32 [B,M,k] or None)."""
    names = KNN_OUT if want_d2 else ("idx",)
    o = fetch(mod().grid_knn(dev(xyz), dev(queries), k, cell=cell, want_d2=want_d2, variant=variant, guard=GUARD,
                             prefill=SENTINEL_BYTE), names)
    assert o["idx"].dtype == np.int32
    return o["idx"], (np.ascontiguousarray(o["d2"]).view(np.int32) if want_d2 else None)


def run_radius(xyz, queries, radius, capacity, cell=0.0, variant=0, want_d2=True, want_idx=True):
    """-> dict of count [B,M], row_start [B,M+1], total [B], idx [B,capacity], bits [B,capacity]."""
    names = tuple(k for k in RADIUS_OUT if (want_idx or k not in ("idx", "d2")) and (want_d2 or k != "d2"))
    o = fetch(mod().grid_radius(dev(xyz), dev(queries), radius, capacity, want_idx=want_idx, want_d2=want_d2, cell=cell,
                                variant=variant, guard=GUARD, prefill=SENTINEL_BYTE), names)
    assert o["count"].dtype == np.int32 and o["row_start"].dtype == np.int64 and o["total"].dtype == np.int64
    if "d2" in o:
        o["bits"] = np.ascontiguousarray(o.pop("d2")).view(np.int32)
    return o


def assert_knn(got, b, want, what):
    idx, bits = got
    assert np.array_equal(idx[b], want[0]), (what, "idx", np.argwhere(idx[b] != want[0])[:5])
    if bits is not None:
        assert np.array_equal(bits[b], want[1]), (what, "d2", np.argwhere(bits[b] != want[1])[:5])


def assert_rows(got, b, want, capacity, what):
    """Cloud b of a call's outputs against the definition's result `want` for that cloud, at this capacity."""
    assert np.array_equal(got["count"][b], want["count"]), (what, "count", np.flatnonzero(got["count"][b] != want["count"])[:5])
    assert np.array_equal(got["row_start"][b], want["row_start"]), (what, "row_start")
    assert int(got["total"][b]) == want["total"], (what, "total")
    idx, bits = rr.padded(want, capacity)
    if "idx" in got:
        assert got["idx"].shape[1] == capacity
        assert np.array_equal(got["idx"][b], idx), (what, "idx", np.flatnonzero(got["idx"][b] != idx)[:5])
    if "bits" in got:
        assert np.array_equal(got["bits"][b], bits), (what, "d2", np.flatnonzero(got["bits"][b] != bits)[:5])


@functools.lru_cache(maxsize=None)
def case(name, queries, N, M, k=K, seed=0):
    """(points [3,N], queries [3,M], radius, the definition's kNN rows, the definition's radius rows): computed once, shared,
    never written to."""
    xyz = gr.RECIPES[name](N, seed)
    q = qr.QUERIES[queries](xyz, M, seed + 1)
    radius = orr.radius_for(N, 12)
    D = qr.d2_matrix(xyz, q)
    knn = qr.knn(xyz, q, k, D)
    rows = qr.radius_rows(xyz, q, radius, D)
    for a in [xyz, q, *knn] + [v for v in rows.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return xyz, q, radius, knn, rows


@pytest.mark.parametrize("M,N", [(1, 1), (1, 300), (300, 1), (255, 257), (256, 256), (257, 255), (1025, 300), (300, 4096),
                                 (4096, 300), (4096, 4096)])
def test_sizes_against_the_definition(M, N):
    """One query, one point (k > N: the row is padded); a workgroup's edge in the queries and in the points; more queries than
    points and the reverse; 4 096 of both."""
    xyz, q, radius, knn, rows = case("random", "jitter", N, M)
    assert_knn(run_knn(xyz, q), 0, knn, (M, N))
    assert ((knn[0] >= 0).sum(1) == min(K, N)).all() and knn[0].max() < N
    assert_rows(run_radius(xyz, q, radius, rows["total"]), 0, rows, rows["total"], (M, N))


@pytest.mark.parametrize("k", [1, 62])
def test_the_smallest_and_the_largest_k(k):
    xyz, q, _, knn, _ = case("random", "jitter", 300, 300, k)
    assert knn[0].shape == (300, k) and (knn[0] >= 0).all()
    assert_knn(run_knn(xyz, q, k), 0, knn, k)
    assert_knn(run_knn(xyz, q, k, want_d2=False), 0, knn, (k, "without d2"))


@pytest.mark.parametrize("queries", sorted(qr.QUERIES))
@pytest.mark.parametrize("name", sorted(gr.RECIPES))
def test_content_against_the_definition(name, queries):
    """Every points recipe (lattice ties and points ON faces, flat, collinear, all points equal, copies, NaN / inf, a far outlier,
    a tiny cloud, clusters) x every query recipe (the points themselves, jittered, beyond every face, edge and corner of the box,
    exactly ON lo, hi and the faces, 1e6 and 3e19 away, NaN / inf, all equal) at N = M = 300."""
    xyz, q, radius, knn, rows = case(name, queries, 300, 300)
    assert_knn(run_knn(xyz, q), 0, knn, (name, queries))
    assert_rows(run_radius(xyz, q, radius, rows["total"]), 0, rows, rows["total"], (name, queries))
    bad = np.flatnonzero(~gr.finite(xyz))
    assert not np.isin(knn[0], bad).any() and not np.isin(rows["idx"], bad).any()
    assert (knn[0][~gr.finite(q)] == -1).all() and (rows["count"][~gr.finite(q)] == 0).all()
    if queries == "far":
        assert (knn[0][150:] == -1).all() and (knn[1][150:] == qr.INF_BITS).all()           # every d2 overflows: an empty row
    if queries == "same" and not name.startswith("nonfinite"):
        assert (knn[1][:, 0] == 0).all() and (rows["count"] >= 1).all()                    # nothing is excluded


def test_queries_outside_a_large_cloud():
    xyz, q, radius, knn, rows = case("random", "outside", 4096, 4096)
    assert_knn(run_knn(xyz, q), 0, knn, "outside")
    assert 0 < rows["total"] and (rows["count"] == 0).sum() > 2048                          # most queries lie beyond the box
    assert_rows(run_radius(xyz, q, radius, rows["total"]), 0, rows, rows["total"], "outside")


@pytest.mark.parametrize("queries", ["jitter", "outside", "nonfinite"])
@pytest.mark.parametrize("name", ["random", "lattice", "copies", "nonfinite", "outlier"])
def test_every_form_returns_the_same_bits(name, queries):
    """Every forced edge from "every point its own cell" (widened to the budget) to "one cell", the lattice's own 1 and 2, both
    query orders and the plan's; a second run; and without d2 the same idx."""
    xyz, q, radius, knn, rows = case(name, queries, 300, 300)
    cap = rows["total"] + 3
    for cell in [0.0] + gr.forced_cells(xyz):
        for order in (0, 1, 2):
            assert_knn(run_knn(xyz, q, cell=cell, variant=order), 0, knn, (name, queries, cell, order))
            assert_rows(run_radius(xyz, q, radius, cap, cell, order), 0, rows, cap, (name, queries, cell, order))
    for order in (1, 2):
        assert_knn(run_knn(xyz, q, variant=order), 0, knn, (name, queries, "again", order))
        alone = run_radius(xyz, q, radius, cap, variant=order, want_d2=False)
        assert "bits" not in alone
        assert_rows(alone, 0, rows, cap, (name, queries, "without d2", order))


def test_capacity_decides_what_is_written():
    """capacity == total fits; total - 1 does not: idx all -1, d2 all +inf, count / row_start / total right; total + 70 pads;
    the count-only call; capacity 0 with nothing to write."""
    xyz, q, radius, _, rows = case("random", "jitter", 4096, 1025)
    total = rows["total"]
    assert total > 1025
    for capacity in (total, total - 1, total + 70, 1, 0):
        got = run_radius(xyz, q, radius, capacity)
        assert_rows(got, 0, rows, capacity, capacity)
        if capacity < total:
            assert (got["idx"] == -1).all() and (got["bits"] == rr.INF_BITS).all()
    counted = run_radius(xyz, q, radius, 0, want_idx=False)
    assert set(counted) == {"count", "row_start", "total"}
    assert_rows(counted, 0, rows, 0, "count only")


def test_a_batch_is_its_clouds_alone_and_a_call_repeats_itself():
    """B = 3, three different (points, queries) pairs at one radius, the capacity between their totals: exactly one does not fit
    -- all -1 / +inf with its true row_start and total -- and the other two are written as if alone."""
    N, M = 777, 600
    cases = [case(n, qn, N, M) for n, qn in (("random", "jitter"), ("copies", "outside"), ("nonfinite", "nonfinite"))]
    pairs, radius = [c[:2] for c in cases], cases[0][2]
    knns, wants = [c[3] for c in cases], [c[4] for c in cases]
    totals = sorted(w["total"] for w in wants)
    assert totals[0] < totals[1] < totals[2]
    xyz, qs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    both = run_knn(xyz, qs)
    again = run_knn(xyz, qs)
    assert np.array_equal(both[0], again[0]) and np.array_equal(both[1], again[1])
    for b, (x, q) in enumerate(pairs):
        assert_knn(both, b, knns[b], ("in the batch", b))
        assert_knn(run_knn(x, q), 0, knns[b], ("alone", b))
    for capacity in (totals[2], totals[2] - 1):              # all three fit; exactly one does not
        first = run_radius(xyz, qs, radius, capacity)
        again = run_radius(xyz, qs, radius, capacity)
        for k in first:
            assert np.array_equal(first[k], again[k]), ("the same call twice", k)
        assert sum(w["total"] > capacity for w in wants) == (0 if capacity == totals[2] else 1)
        for b, ((x, q), w) in enumerate(zip(pairs, wants)):
            assert_rows(first, b, w, capacity, ("in the batch", b, capacity))
            assert_rows(run_radius(x, q, radius, capacity), 0, w, capacity, ("alone", b, capacity))
            if w["total"] > capacity:
                assert (first["idx"][b] == -1).all() and (first["bits"][b] == rr.INF_BITS).all()


# ----------------------------------------------------------------------------------------- relations to the searches that exist

@pytest.mark.parametrize("name", ["random", "copies", "nonfinite"])
def test_a_cloud_searched_in_itself_is_the_self_search_plus_the_point(name):
    """Independent kernels on the same device.  kNN: the cross rows at k + 1 with the entry j == i removed, cut to k, are
    search_knn's rows wherever those are full.  Radius: the cross rows minus j == i are search_radius' rows, and count = n_i + 1
    for a finite point."""
    import vcrnet_amd
    N, k = 1025, 16
    xyz = gr.RECIPES[name](N, 0)
    xd = dev(xyz)
    me = np.arange(N)[:, None]
    self_idx, self_d2 = (t[0].cpu().numpy() for t in vcrnet_amd.search_knn(xd, k, want_d2=True))
    cross_idx, cross_d2 = (t[0].cpu().numpy() for t in vcrnet_amd.search_knn(xd, k + 1, want_d2=True, queries=xd))
    order = np.argsort(cross_idx == me, axis=1, kind="stable")[:, :k]       # the entry j == i (at most one) goes last
    cut_idx, cut_d2 = np.take_along_axis(cross_idx, order, 1), np.take_along_axis(cross_d2, order, 1)
    full = np.isfinite(self_d2[:, k - 1])
    assert full.sum() >= N - 8 and ((cross_idx == me).sum(1) == gr.finite(xyz)).all()
    assert np.array_equal(cut_idx[full], self_idx[full]) and np.array_equal(cut_d2[full].view(np.int32), self_d2[full].view(np.int32))

    radius = orr.radius_for(N, 12)
    s_idx, s_start, s_total, s_d2 = (t[0].cpu().numpy() for t in vcrnet_amd.search_radius(xd, radius, want_d2=True))
    c_idx, c_start, c_total, c_d2 = (t[0].cpu().numpy() for t in vcrnet_amd.search_radius(xd, radius, want_d2=True, queries=xd))
    ok = gr.finite(xyz)
    assert np.array_equal(np.diff(c_start), np.where(ok, np.diff(s_start) + 1, 0)) and c_total == s_total + ok.sum()
    owner = np.repeat(np.arange(N), np.diff(c_start))
    keep = c_idx[:c_total] != owner
    assert np.array_equal(c_idx[:c_total][keep], s_idx[:s_total])
    assert np.array_equal(c_d2[:c_total][keep].view(np.int32), s_d2[:s_total].view(np.int32))


def test_the_nearest_point_is_the_scans():
    """On finite clouds the k = 1 rows are nn_scan_kernel's neighbours (score.nn_score, search="scan"), bit for bit."""
    from vcrnet_amd import score
    for name, queries in (("random", "outside"), ("lattice", "faces"), ("copies", "same"), ("clustered", "jitter")):
        xyz, q = case(name, queries, 300, 300)[:2]
        xd, qd = dev(xyz), dev(q)
        scan = score.nn_score(qd, xd, None, None, search="scan")
        o = mod().grid_knn(xd, qd, 1)
        assert torch.equal(o["idx"][:, :, 0], scan["nn_idx"]), (name, queries)
        assert torch.equal(o["d2"][:, :, 0].contiguous().view(torch.int32), scan["nn_d2"].view(torch.int32)), (name, queries)


@pytest.mark.parametrize("m", [1, 20, 62])
def test_the_hybrid_search_is_the_prefix_of_the_pure_rows(m):
    """search_radius(max_nn=m, queries=): every row's first min(n_i, m) entries, bit for bit; with capacity=None (one
    synchronisation) and with a capacity given (fits, and one short)."""
    import vcrnet_amd
    xyz, q = case("random", "jitter", 1025, 700)[:2]
    radius = orr.radius_for(1025, 70)
    full = qr.radius_rows(xyz, q, radius)
    assert full["count"].max() > 62 > full["count"].min()
    want = rr.cut(full, m)
    xd, qd = dev(xyz), dev(q)
    for capacity in (None, want["total"] + 5, want["total"] - 1):
        idx, row_start, total, d2 = vcrnet_amd.search_radius(xd, radius, max_nn=m, want_d2=True, capacity=capacity, queries=qd)
        cap = want["total"] if capacity is None else capacity
        got = {"count": np.diff(row_start.cpu().numpy(), axis=1).astype(np.int32), "row_start": row_start.cpu().numpy(),
               "total": total.cpu().numpy(), "idx": idx.cpu().numpy(), "bits": d2.cpu().numpy().view(np.int32)}
        assert idx.dtype == torch.int32 and row_start.dtype == total.dtype == torch.int64 and d2.dtype == torch.float32
        assert tuple(row_start.shape) == (1, 701)
        assert_rows(got, 0, want, cap, (m, capacity))
        alone = vcrnet_amd.search_radius(xd, radius, max_nn=m, capacity=capacity, queries=qd)
        assert len(alone) == 3 and torch.equal(alone[0], idx)


def test_the_public_searches_with_queries():
    """search_knn / search_radius with queries=: the shapes with M for N; capacity=None takes the batch's largest total;
    capacity=int is one call and whatever fits."""
    import vcrnet_amd
    pairs = [case("random", "jitter", 777, 600), case("copies", "outside", 777, 600)]
    xd, qd = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs]))
    radius = pairs[0][2]
    idx = vcrnet_amd.search_knn(xd, K, queries=qd)
    both = vcrnet_amd.search_knn(xd, K, want_d2=True, cell=0.2, queries=qd)
    assert tuple(idx.shape) == (2, 600, K) and idx.dtype == torch.int32 and torch.equal(idx, both[0])
    for b, p in enumerate(pairs):
        assert_knn((both[0].cpu().numpy(), both[1].cpu().numpy().view(np.int32)), b, p[3], ("search_knn", b))
    wants = [p[4] for p in pairs]
    idx, row_start, total, d2 = vcrnet_amd.search_radius(xd, radius, want_d2=True, queries=qd)
    cap = max(w["total"] for w in wants)
    assert tuple(idx.shape) == tuple(d2.shape) == (2, cap) and tuple(row_start.shape) == (2, 601)
    got = {"count": np.diff(row_start.cpu().numpy(), axis=1).astype(np.int32), "row_start": row_start.cpu().numpy(),
           "total": total.cpu().numpy(), "idx": idx.cpu().numpy(), "bits": d2.cpu().numpy().view(np.int32)}
    for b, w in enumerate(wants):
        assert_rows(got, b, w, cap, ("capacity=None", b))
    short = vcrnet_amd.search_radius(xd, radius, capacity=cap - 1, cell=0.3, queries=qd)
    assert len(short) == 3 and short[2].tolist() == total.tolist() and [w["total"] <= cap - 1 for w in wants].count(False) == 1
    for b, w in enumerate(wants):
        assert np.array_equal(short[0][b].cpu().numpy(), rr.padded(w, cap - 1)[0])


def test_a_translation_that_is_exact_returns_the_same_bits():
    """Points and queries on a 1/1024 lattice, BOTH moved by (1024, -512, 256): every coordinate and every difference stays
    exact in fp32, so every d2 keeps its bits."""
    N, M = 2000, 1500
    rs = np.random.RandomState(9)
    x = (rs.randint(0, 1024, (3, N)) / 1024.0).astype(np.float32)
    q = (rs.randint(-256, 1280, (3, M)) / 1024.0).astype(np.float32)                        # some beyond the box
    fx, fq = (x + rr.FAR).astype(np.float32), (q + rr.FAR).astype(np.float32)
    assert np.array_equal(fx - rr.FAR, x) and np.array_equal(fq - rr.FAR, q) and np.abs(fx).max() <= 1025
    radius = orr.radius_for(N, 12, extent=1.0)
    D = qr.d2_matrix(x, q)
    knn, rows = qr.knn(x, q, K, D), qr.radius_rows(x, q, radius, D)
    assert rows["total"] > M and (rows["count"] == 0).any()
    for cloud, queries, what in ((x, q, "at the origin"), (fx, fq, "moved")):
        assert_knn(run_knn(cloud, queries), 0, knn, what)
        assert_rows(run_radius(cloud, queries, radius, rows["total"]), 0, rows, rows["total"], what)


def test_compute_point_cloud_distance():
    """Open3D's call: sqrt of the k = 1 d2 (fp32 sqrt is correctly rounded, so the comparison with numpy's is exact); +inf and
    -1 for a source point that is not finite, and everywhere where the target has no finite point."""
    import vcrnet_amd
    tgt, src, _, _, _ = case("random", "nonfinite", 300, 300)
    other, src2 = case("clustered", "outside", 300, 300)[:2]
    none = np.full((3, 300), np.nan, np.float32)
    td, sd = dev(np.stack([tgt, other, none])), dev(np.stack([src, src2, src2]))
    dist, idx = vcrnet_amd.compute_point_cloud_distance(sd, td, want_index=True)
    alone = vcrnet_amd.compute_point_cloud_distance(sd, td)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(dist.shape) == tuple(idx.shape) == (3, 300)
    assert torch.equal(alone.view(torch.int32), dist.view(torch.int32))
    for b, (t, s) in enumerate(((tgt, src), (other, src2), (none, src2))):
        want_idx, want_bits = qr.knn(t, s, 1)
        want = np.sqrt(want_bits[:, 0].view(np.float32))
        assert np.array_equal(dist[b].cpu().numpy().view(np.int32), want.view(np.int32)), b
        assert np.array_equal(idx[b].cpu().numpy(), want_idx[:, 0]), b
    bad = ~gr.finite(src)
    assert bad.sum() >= 4 and torch.isinf(dist[0][torch.from_numpy(bad)]).all() and (idx[0][torch.from_numpy(bad)] == -1).all()
    assert torch.isfinite(dist[1]).all() and torch.isinf(dist[2]).all() and (idx[2] == -1).all()


def test_labels_travel_from_a_down_sampled_cloud_to_the_full_one():
    """The recipe of the README: voxel_down_sample -> cluster_dbscan -> search_knn(down, 1, queries=full) -> gather.  Two blobs
    far apart: every point of the full cloud gets the label of its blob."""
    import vcrnet_amd
    rs = np.random.RandomState(4)
    blob = rs.uniform(0, 1, (3, 1000)).astype(np.float32)
    full = np.concatenate([blob, blob + np.float32(5.0)], 1)[:, rs.permutation(2000)]
    fd = dev(full)
    down, count, _ = vcrnet_amd.voxel_down_sample(fd, 0.1)
    labels, n_clusters = vcrnet_amd.cluster_dbscan(down, 0.3, 4)[:2]
    assert int(n_clusters[0]) == 2 and 0 < int(count[0]) < 2000
    nearest = vcrnet_amd.search_knn(down, 1, queries=fd)[:, :, 0]
    assert int(nearest.min()) >= 0 and int(nearest.max()) < int(count[0])                  # (the NaN padding is in nobody's row)
    carried = torch.where(nearest >= 0, labels.gather(1, nearest.clamp(min=0).long()), -1)[0].cpu().numpy()
    side = full[0] > 3.0
    assert len(set(carried[side])) == 1 and len(set(carried[~side])) == 1 and carried[side][0] != carried[~side][0]
    assert set(carried) == {0, 1}
