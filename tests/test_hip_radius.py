"""vcr_grid_radius_f32 and vcr_outlier_radius_grid_f32 on the GPU: all points within a radius on the cloud's uniform grid, rows of
varying length (include/vcr_hip_radius.h).

The result is defined bit for bit, so every comparison here is exact and on int32 / int64 views: count, row_start, total, idx and
d2's bits against the numpy brute force (tests/radius_restated.py: ``radius_rows`` is the definition); the filter's four outputs
against tests/outlier_restated.py and against the scan entry point on the same device.  Every output buffer, and the workspace,
is prefilled with the byte 0x5A and carries a guard band of 64 elements: every slot must have been written, and nothing behind
it.  Every forced cell, both query orders, both ordering forms, every batch and every run must return the same bits."""
import functools

import numpy as np
import pytest
import torch

import grid_restated as gr
import outlier_restated as orr
import radius_restated as rr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
CHUNK = 128                                                # VCR_RADIUS_CHUNK: the keys the wave-per-row ordering stages at a time
SEARCH_OUT = ("count", "row_start", "total", "idx", "d2")
FILTER_OUT = ("points", "count", "index", "neighbours")


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import outlier, radius
    return radius, outlier


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


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


def run(xyz, radius, capacity, cell=0.0, variant=0, want_d2=True, want_idx=True):
    """numpy [B,3,N] (or [3,N]) in -> dict of count [B,N], row_start [B,N+1], total [B], idx [B,capacity], bits [B,capacity]."""
    radius_mod = mods()[0]
    xyz = xyz[None] if xyz.ndim == 2 else xyz
    names = tuple(k for k in SEARCH_OUT if (want_idx or k not in ("idx", "d2")) and (want_d2 or k != "d2"))
    o = fetch(radius_mod.grid_radius(dev(xyz), radius, capacity, want_idx=want_idx, want_d2=want_d2, cell=cell, variant=variant,
                                     guard=GUARD, prefill=SENTINEL_BYTE), names)
    assert o["count"].dtype == np.int32 and o["row_start"].dtype == np.int64 and o["total"].dtype == np.int64
    if "d2" in o:
        o["bits"] = np.ascontiguousarray(o.pop("d2")).view(np.int32)
    return o


def assert_cloud(got, b, want, capacity, what):
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
def case(name, N, inside=12, seed=0):
    """(xyz [3,N], radius, the definition's result): computed once, shared, never written to."""
    xyz = gr.RECIPES[name](N, seed)
    radius = orr.radius_for(N, inside)
    want = rr.radius_rows(xyz, radius)
    for a in [xyz] + [v for v in want.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return xyz, radius, want


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1025, 4096])
def test_sizes_against_the_definition(N):
    """One point (an empty row); two; a workgroup's edge (255 / 256 / 257); 1 025 and 4 096 points."""
    xyz, radius, want = case("random", N)
    got = run(xyz, radius, want["total"])
    assert_cloud(got, 0, want, want["total"], N)
    if N > 2:
        assert want["total"] > 0 and got["idx"].min() >= 0 and got["idx"].max() < N


@pytest.mark.parametrize("name", sorted(gr.RECIPES))
@pytest.mark.parametrize("N", [300, 4096])
def test_content_against_the_definition(name, N):
    """The CPU recipes: lattice ties and points ON faces, flat, collinear, all points equal (rows of N - 1 copies at d2 = 0, in
    index order), copies, NaN / inf at point 0 and elsewhere (empty rows, in nobody's row), a far outlier (nearly every point
    in few cells), a tiny cloud (the radius spans it) and a clustered one."""
    xyz, radius, want = case(name, N)
    got = run(xyz, radius, want["total"])
    assert_cloud(got, 0, want, want["total"], (name, N))
    if name == "equal":
        me = np.arange(N)
        rows = got["idx"][0].reshape(N, N - 1)
        assert (got["count"][0] == N - 1).all() and (got["bits"][0] == 0).all()
        assert all(np.array_equal(rows[i], me[me != i]) for i in (0, 1, N // 2, N - 1))
    if name.startswith("nonfinite"):
        bad = np.flatnonzero(~gr.finite(xyz))
        assert len(bad) >= 2 and (got["count"][0][bad] == 0).all() and not np.isin(got["idx"][0], bad).any()
        assert got["count"][0].max() > 0


@functools.lru_cache(maxsize=None)
def edge_cloud():
    xyz = gr.random_cloud(1025, 3)
    d2 = rr.d2_all(xyz)
    for a in (xyz, d2):
        a.setflags(write=False)
    return xyz, d2


@pytest.mark.parametrize("longest", [63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_row_lengths_at_the_ordering_kernels_edges(longest):
    """The longest row one below, exactly at and one above a wave's 64 elements, and the same around the LDS chunk of
    VCR_RADIUS_CHUNK = 128 keys: the radius is chosen on the CPU from the definition.  The plan's form and both forced ones."""
    radius_mod = mods()[0]
    xyz, d2 = edge_cloud()
    found = rr.radius_with_longest_row(xyz, longest, d2)
    assert found is not None, longest
    radius, want = found
    assert int(want["count"].max()) == longest and radius_mod.CHUNK == CHUNK
    for form in (0, 1, 2):
        got = run(xyz, radius, want["total"], variant=radius_mod.variant(0, form))
        assert_cloud(got, 0, want, want["total"], (longest, form))


@pytest.mark.parametrize("name", ["random", "lattice", "copies", "nonfinite", "outlier"])
def test_every_form_returns_the_same_bits(name):
    """Every forced edge from "every point its own cell" (widened to the budget) to "one cell", the lattice's own 1 and 2, both
    query orders and the plan's, both ordering forms and the plan's; and without d2 the same idx."""
    radius_mod = mods()[0]
    xyz, radius, want = case(name, 1025)
    cap = want["total"] + 3
    for cell in [0.0] + gr.forced_cells(xyz):
        for order in (0, 1, 2):
            for form in (0, 1, 2):
                got = run(xyz, radius, cap, cell, radius_mod.variant(order, form))
                assert_cloud(got, 0, want, cap, (name, cell, order, form))
    for form in (1, 2):
        alone = run(xyz, radius, cap, variant=radius_mod.variant(0, form), want_d2=False)
        assert "bits" not in alone
        assert_cloud(alone, 0, want, cap, (name, "without d2", form))


def test_capacity_decides_what_is_written():
    """capacity == total fits; total - 1 does not: idx all -1, d2 all +inf, count / row_start / total right; total + 70 pads;
    the count-only call; capacity 0 with nothing to write."""
    xyz, radius, want = case("random", 1025)
    total = want["total"]
    for capacity in (total, total - 1, total + 70, 1, 0):
        got = run(xyz, radius, capacity)
        assert_cloud(got, 0, want, capacity, capacity)
        if capacity < total:
            assert (got["idx"] == -1).all() and (got["bits"] == rr.INF_BITS).all()
    counted = run(xyz, radius, 0, want_idx=False)
    assert set(counted) == {"count", "row_start", "total"}
    assert_cloud(counted, 0, want, 0, "count only")


def test_a_batch_is_its_clouds_alone_and_a_call_repeats_itself():
    """B = 3, three different clouds (uniform, lattice, one with non-finite points) at one radius, the capacity between their
    totals: exactly one does not fit, and the other two are written as if alone."""
    N = 777
    clouds = [gr.RECIPES[n](N, 0) for n in ("random", "copies", "nonfinite")]
    radius = orr.radius_for(N, 12)
    wants = [rr.radius_rows(x, radius) for x in clouds]
    totals = sorted(w["total"] for w in wants)
    assert totals[1] < totals[2]
    xyz = np.stack(clouds)
    for capacity in (totals[2], totals[1]):                  # all three fit; exactly one does not
        first = run(xyz, radius, capacity)
        again = run(xyz, radius, capacity)
        for k in first:
            assert np.array_equal(first[k], again[k]), ("the same call twice", k)
        assert sum(w["total"] > capacity for w in wants) == (0 if capacity == totals[2] else 1)
        for b, (x, w) in enumerate(zip(clouds, wants)):
            assert_cloud(first, b, w, capacity, ("in the batch", b, capacity))
            assert_cloud(run(x, radius, capacity), 0, w, capacity, ("alone", b, capacity))


@pytest.mark.parametrize("m", [1, 20, 62])
def test_the_hybrid_search_is_the_prefix_of_the_pure_rows(m):
    """search_radius(max_nn=m): every row's first min(n_i, m) entries, bit for bit; with capacity=None (one synchronisation) and
    with a capacity given (fits, and one short)."""
    import vcrnet_amd
    xyz, radius, full = case("random", 1025)
    assert full["count"].max() > 62 > full["count"].min()
    want = rr.cut(full, m)
    xd = dev(xyz[None])
    for capacity in (None, want["total"] + 5, want["total"] - 1):
        idx, row_start, total, d2 = vcrnet_amd.search_radius(xd, radius, max_nn=m, want_d2=True, capacity=capacity)
        cap = want["total"] if capacity is None else capacity
        got = {"count": np.diff(row_start.cpu().numpy(), axis=1).astype(np.int32), "row_start": row_start.cpu().numpy(),
               "total": total.cpu().numpy(), "idx": idx.cpu().numpy(), "bits": d2.cpu().numpy().view(np.int32)}
        assert idx.dtype == torch.int32 and row_start.dtype == total.dtype == torch.int64 and d2.dtype == torch.float32
        assert_cloud(got, 0, want, cap, (m, capacity))
        alone = vcrnet_amd.search_radius(xd, radius, max_nn=m, capacity=capacity)
        assert len(alone) == 3 and torch.equal(alone[0], idx)


def test_search_radius_counts_then_searches():
    """capacity=None: the width of idx is the largest total of the batch; capacity=int: one call, whatever fits."""
    import vcrnet_amd
    clouds = [case("random", 1025)[0], case("copies", 1025)[0]]
    radius = case("random", 1025)[1]
    wants = [case("random", 1025)[2], case("copies", 1025)[2]]
    xd = dev(np.stack(clouds))
    idx, row_start, total, d2 = vcrnet_amd.search_radius(xd, radius, want_d2=True)
    cap = max(w["total"] for w in wants)
    assert tuple(idx.shape) == tuple(d2.shape) == (2, cap) and total.tolist() == [w["total"] for w in wants]
    got = {"count": np.diff(row_start.cpu().numpy(), axis=1).astype(np.int32), "row_start": row_start.cpu().numpy(),
           "total": total.cpu().numpy(), "idx": idx.cpu().numpy(), "bits": d2.cpu().numpy().view(np.int32)}
    for b, w in enumerate(wants):
        assert_cloud(got, b, w, cap, ("capacity=None", b))
    short = vcrnet_amd.search_radius(xd, radius, capacity=cap - 1, cell=0.3)
    assert len(short) == 3 and short[2].tolist() == total.tolist()
    fits = [w["total"] <= cap - 1 for w in wants]
    assert fits.count(False) == 1
    for b, w in enumerate(wants):
        assert np.array_equal(short[0][b].cpu().numpy(), rr.padded(w, cap - 1)[0])


# ------------------------------------------------------------------------------------------------------------------ the filter

def run_filter(xyz, radius, nb_points, cell=0.0, order=0):
    radius_mod = mods()[0]
    return fetch(radius_mod.radius_filter_grid(dev(xyz), radius, nb_points, cell=cell, order=order, guard=GUARD,
                                               prefill=SENTINEL_BYTE), FILTER_OUT)


def run_scan(xyz, radius, nb_points):
    outlier = mods()[1]
    return fetch(outlier.radius_filter(dev(xyz), radius, nb_points, guard=GUARD, prefill=SENTINEL_BYTE), FILTER_OUT)


def assert_filter(got, want, names, what):
    for k in names:
        assert np.array_equal(orr.bits(got[k]), orr.bits(want[k])), (what, k)


@pytest.mark.parametrize("name", list(orr.RADIUS_RECIPES))
def test_the_filter_on_the_grid_is_the_scan_filter(name):
    """Every radius case of the scan filter's tests, the two large ones on sampled rows as there: the four outputs against the
    restatement and, bit for bit, against vcr_outlier_radius_f32 on the same device; both query orders and a forced edge."""
    xyz, radius, nb = orr.RADIUS_RECIPES[name]()
    got = run_filter(xyz, radius, nb)
    if name in orr.LARGE:
        rows = orr.rows_of(name, xyz.shape[2])
        assert np.array_equal(got["neighbours"][0][rows], orr.radius_counts(xyz[0], radius, rows))
        want = orr.compact(xyz[0], got["neighbours"][0] > nb)
        assert 0 < want["count"] < xyz.shape[2]
        assert_filter({k: got[k][0] for k in want}, want, tuple(want), name)
    else:
        assert_filter(got, orr.batch(orr.radius_fast, xyz, radius, nb), FILTER_OUT, name)
    assert_filter(got, run_scan(xyz, radius, nb), FILTER_OUT, (name, "against the scan"))
    if name not in orr.LARGE:
        for cell, order in ((0.0, 1), (0.0, 2), (3.0 * radius, 0), (0.4 * radius, 2)):
            assert_filter(run_filter(xyz, radius, nb, cell, order), got, FILTER_OUT, (name, cell, order))


def test_remove_radius_outlier_on_the_grid():
    """search="grid" and filter_by's fourth element return what search="scan", the default and three elements return."""
    import vcrnet_amd
    outlier = mods()[1]
    xyz, radius, nb = orr.RADIUS_RECIPES["three_clouds"]()
    xd = dev(xyz)
    scan = vcrnet_amd.remove_radius_outlier(xd, nb, radius)
    assert 0 < int(scan[1].min()) and int(scan[1].max()) < xyz.shape[2]
    for got in (vcrnet_amd.remove_radius_outlier(xd, nb, radius, search="grid"), outlier.filter_by(("radius", nb, radius, "grid"), xd),
                vcrnet_amd.remove_radius_outlier(xd, nb, radius, search="scan"), outlier.filter_by(("radius", nb, radius), xd)):
        assert len(got) == 3
        for a, b in zip(got, scan):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_translation_that_is_exact_returns_the_same_rows():
    """A cloud on a 1/1024 lattice moved by (1024, -512, 256): every coordinate and every difference stays exact in fp32."""
    N = 2000
    rs = np.random.RandomState(9)
    x = (rs.randint(0, 1024, (3, N)) / 1024.0).astype(np.float32)
    far = (x + rr.FAR).astype(np.float32)
    assert np.array_equal(far - rr.FAR, x)
    radius = orr.radius_for(N, 12, extent=1.0)
    want = rr.radius_rows(x, radius)
    assert want["total"] > 5 * N
    assert_cloud(run(x, radius, want["total"]), 0, want, want["total"], "at the origin")
    assert_cloud(run(far, radius, want["total"]), 0, want, want["total"], "moved")
    for cloud in (x, far):
        assert_filter(run_filter(cloud[None], radius, 9), orr.batch(orr.radius_fast, x[None], radius, 9),
                      ("count", "index", "neighbours"), "the filter, moved")
