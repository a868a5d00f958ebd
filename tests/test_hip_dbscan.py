"""vcr_rows_dbscan_f32, vcr_cluster_largest_f32, ``cluster_dbscan`` and ``largest_cluster`` on the GPU (include/cluster/
vcr_hip_dbscan.h).

Every comparison is bit-equal on labels, n_clusters, core and sizes: with the numpy restatement (tests/dbscan_restated.py) fed the
DEVICE'S OWN rows, and for ``cluster_dbscan`` also with the restatement on the definition's rows (radius_restated.radius_rows).
Every raw call runs with its outputs and its workspace prefilled with the byte 0xA5 and 64 elements of guard behind the outputs,
and everything that has two launch forms runs in both and in the plan's."""
import functools

import numpy as np
import pytest
import torch

import dbscan_restated as dr
import fpfh_restated as fr
import grid_restated as gr
import outlier_restated as orr
import radius_restated as rr
import rows_restated as wr

pytestmark = pytest.mark.gpu

BYTE = 0xA5
GUARD = 64
FORMS = (0, "lane", "wave")
MIN_POINTS = (1, 4, 6)
KEYS = ("labels", "core", "sizes")


def mods():
    import vcrnet_amd
    from vcrnet_amd import dbscan
    return vcrnet_amd, dbscan


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def checked(out, raw, name):
    """The output as numpy; all of it must have been overwritten, none of the band behind it."""
    buf, n = raw[name], out.numel()
    size = buf.element_size()
    band = buf[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * size and (band == BYTE).all(), (name, "guard band written")
    body = buf[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
    assert not (body == BYTE).all(axis=1).any(), (name, "element left unwritten")
    return out.cpu().numpy()


def run(csr, N, mp, xyz=None, variant=0):
    """The raw call with everything asked for -> dict of numpy [B, ...]."""
    _, dbscan = mods()
    o = dbscan.cluster_rows(*csr, N, mp, xyz=xyz, want_core=True, want_sizes=True, variant=variant, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    return {k: checked(o[k], o["_raw"], k) for k in KEYS + ("n_clusters",)}


def cloud_of(o, b):
    return {"labels": o["labels"][b], "core": o["core"][b], "sizes": o["sizes"][b], "n_clusters": int(o["n_clusters"][b])}


def host(csr):
    return [t.cpu().numpy() for t in csr]


def restated(csr_np, b, N, mp, x=None, form=dr.sequential):
    """Cloud b by the restatement on the rows as the device holds them."""
    idx, row_start, total = csr_np
    if not dr.served(row_start[b], int(total[b]), idx.shape[1]):
        return dr.not_served(N)
    return form(idx[b], row_start[b], N, mp, None if x is None else gr.finite(x[b]))


def agree(got, want, what):
    assert got["n_clusters"] == want["n_clusters"], (what, got["n_clusters"], want["n_clusters"])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def all_forms_against_the_restatement(x, radius, min_points=MIN_POINTS, form=dr.sequential, definition=True):
    """x [B,3,N] at one radius: search_radius' rows, the raw call in every form against the restatement on those rows, and (where
    definition) cluster_dbscan against the restatement on the definition's rows.  -> the plan's results per min_points."""
    vcrnet_amd, _ = mods()
    B, _, N = x.shape
    xyz = dev(x)
    csr = vcrnet_amd.search_radius(xyz, radius)
    csr_np = host(csr)
    out = {}
    for mp in min_points:
        want = [restated(csr_np, b, N, mp, x, form) for b in range(B)]
        for variant in FORMS:
            o = run(csr, N, mp, xyz, variant)
            for b in range(B):
                agree(cloud_of(o, b), want[b], (radius, mp, variant, b))
            if variant == 0:
                out[mp] = o
        if definition:
            labels, n, core, sizes = vcrnet_amd.cluster_dbscan(xyz, radius, mp, want_core=True, want_sizes=True)
            o = {"labels": labels.cpu().numpy(), "core": core.cpu().numpy(), "sizes": sizes.cpu().numpy(), "n_clusters": n.cpu().numpy()}
            for b in range(B):
                agree(cloud_of(o, b), dr.of_cloud(x[b], radius, mp)[0], ("cluster_dbscan", radius, mp, b))
            two = vcrnet_amd.cluster_dbscan(xyz, radius, mp)
            assert len(two) == 2 and torch.equal(two[0], labels) and torch.equal(two[1], n)
    return out


# ----------------------------------------------------------------------------------------------- the restatement on real rows

def test_the_cloud_worked_by_hand():
    x = dr.hand_cloud()[None]
    N = x.shape[2]
    got = all_forms_against_the_restatement(x, dr.HAND_EPS, tuple(dr.HAND_WANT))
    for mp, want in dr.HAND_WANT.items():
        o = cloud_of(got[mp], 0)
        assert o["labels"].tolist() == want["labels"] and o["core"].tolist() == want["core"] and o["n_clusters"] == want["n_clusters"]
        assert o["sizes"][:len(want["sizes"])].tolist() == want["sizes"] and not o["sizes"][len(want["sizes"]):].any()
    assert N == 12


@pytest.mark.parametrize("N", [60, 1000])
def test_the_recipes_three_to_a_batch(N):
    radius = orr.radius_for(N, 12)
    for names in (("random", "copies", "nonfinite"), ("flat", "lattice", "random")):
        x = np.stack([gr.RECIPES[name](N, seed=N) for name in names])
        all_forms_against_the_restatement(x, radius)
    # the lattice at a radius that reaches its neighbours (its spacing is 1)
    all_forms_against_the_restatement(gr.RECIPES["lattice"](N, seed=N)[None], 1.5)


@pytest.mark.parametrize("radius", wr.RAGGED_RADII)
def test_the_ragged_recipe(radius):
    """fpfh_restated.cloud(2, 300): rows of 0, 1, 63, 64, 65 and more than 255 entries over the four radii; three clusters,
    contested border points and noise at the first; one cluster of N at the last (tests/test_dbscan_cpu.py asserts the recipe)."""
    B, N = wr.RAGGED
    got = all_forms_against_the_restatement(fr.cloud(B, N), radius)
    if radius == wr.RAGGED_RADII[-1]:
        for mp in MIN_POINTS:
            assert (got[mp]["n_clusters"] == 1).all() and (got[mp]["labels"] == 0).all() and (got[mp]["sizes"][:, 0] == N).all()
    if radius == wr.RAGGED_RADII[0]:
        assert got[6]["n_clusters"].max() >= 3 and (got[6]["labels"] == -1).any()


def test_a_path_is_one_cluster_and_a_cut_path_is_numbered_by_lowest_index():
    """The union-find's worst case: 4 096 points in a line, 1 apart, indices scrambled -- one component as long as the cloud --
    and the same line cut in seven places.  A wrong hook direction, a lost CAS or a shallow flatten shows here."""
    n = 4096
    whole, perm = dr.path(n)
    cut, perm2 = dr.path(n, dr.PATH_CUTS)
    assert np.array_equal(perm, perm2)
    got = all_forms_against_the_restatement(np.stack([whole, cut]), 1.0, (2,), definition=False)[2]
    assert got["n_clusters"].tolist() == [1, 8] and not got["labels"][0].any() and got["core"].all()
    assert np.array_equal(got["labels"][1], dr.path_want(n, perm, dr.PATH_CUTS))
    assert got["sizes"][0, 0] == n and got["sizes"][1, :8].sum() == n


def test_twenty_thousand_uniform_points():
    """About 12 entries a row: indices past 16 bits and many workgroups.  min_points = 6 leaves one large cluster, 16 sits near
    the percolation threshold of the core graph: hundreds of clusters of every size."""
    N = 20000
    x = dr.uniform(N, seed=7)[None]
    got = all_forms_against_the_restatement(x, orr.radius_for(N, 13), (6, 16), form=dr.vectorised, definition=False)
    assert got[6]["n_clusters"][0] >= 1 and got[16]["n_clusters"][0] >= 50
    print("clusters", got[6]["n_clusters"], got[16]["n_clusters"])


def test_the_largest_cloud():
    """One cloud of 131 072 points with its capacity given (no host synchronisation): against the vectorised restatement, and
    n_clusters and 4 096 sampled labels through the sequential definition run on those points' components."""
    vcrnet_amd, _ = mods()
    N, mp = 131072, 14
    x = dr.uniform(N, seed=3)[None]
    xyz = dev(x)
    radius = orr.radius_for(N, 13)
    csr = vcrnet_amd.search_radius(xyz, radius, capacity=16 * N)
    csr_np = host(csr)
    assert 0 < int(csr_np[2][0]) <= 16 * N
    want = restated(csr_np, 0, N, mp, x, dr.vectorised)
    for variant in FORMS:
        agree(cloud_of(run(csr, N, mp, xyz, variant), 0), want, variant)
    assert want["n_clusters"] >= 2
    # the sampled points' components, cut out of the cloud with their indices kept in order: the sequential definition on them
    # must number them in the same order, and count as many as the sample touches
    rs = np.random.RandomState(5)
    sample = rs.permutation(N)[:4096]
    touched = np.unique(want["labels"][sample][want["labels"][sample] >= 0])
    member = np.isin(want["labels"], touched)
    keep = np.flatnonzero(member)
    new = np.full(N, -1, np.int64)
    new[keep] = np.arange(len(keep))
    idx, row_start = csr_np[0][0], csr_np[1][0]
    src, dst = dr.entries(idx, row_start, N)
    inside = member[src]
    sub_start = np.zeros(len(keep) + 1, np.int64)
    np.cumsum(np.bincount(new[src[inside]], minlength=len(keep)), out=sub_start[1:])
    sub_idx = new[dst[inside]]                               # (an entry outside the components becomes -1: ignored, so ...)
    sub = dr.sequential(sub_idx, sub_start, len(keep), 1, want["core"][keep].astype(bool))     # ... core is given, not recounted
    assert sub["n_clusters"] == len(touched)
    rank = np.full(want["n_clusters"], -1)
    rank[touched] = np.arange(len(touched))
    on_core = want["core"][keep] == 1
    assert np.array_equal(sub["labels"][on_core], rank[want["labels"][keep]][on_core])


# ------------------------------------------------------------------------------------------------------------------ invariances

@functools.lru_cache(maxsize=None)
def mixed():
    """Three clouds of 300 points that differ: the torus, blobs with clutter, the non-finite recipe."""
    x = np.stack([fr.cloud(1, 300)[0], dr.blobs(300, k=4, seed=2, spread=0.08), gr.RECIPES["nonfinite"](300, seed=300)])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("variant", FORMS)
def test_a_cloud_alone_returns_the_bits_it_returns_in_the_batch_and_twice_the_same(variant):
    vcrnet_amd, _ = mods()
    x = mixed()
    B, _, N = x.shape
    xyz = dev(x)
    radius, mp = 0.2, 5
    csr = vcrnet_amd.search_radius(xyz, radius)
    o = run(csr, N, mp, xyz, variant)
    again = run(csr, N, mp, xyz, variant)
    assert o["n_clusters"].max() >= 2
    for b in range(B):
        agree(cloud_of(again, b), cloud_of(o, b), ("twice", b))
        one = vcrnet_amd.search_radius(xyz[b:b + 1], radius)
        agree(cloud_of(run(one, N, mp, xyz[b:b + 1], variant), 0), cloud_of(o, b), ("alone", b))
        agree(cloud_of(o, b), dr.of_cloud(x[b], radius, mp)[0], ("definition", b))


@pytest.mark.parametrize("variant", FORMS)
def test_a_cloud_that_is_not_served_comes_back_minus_two_and_leaves_the_others_alone(variant):
    """total[b] > capacity (search_radius' "does not fit": every idx -1), and a row_start that does not ascend from 0 to total."""
    vcrnet_amd, _ = mods()
    x = mixed()
    B, _, N = x.shape
    radius, mp = 0.2, 5
    totals = [rr.radius_rows(x[b], radius)["total"] for b in range(B)]
    big = int(np.argmax(totals))
    cap = int(max(t for t in totals if t != totals[big]))
    assert cap < totals[big]
    xyz = dev(x)
    fits = vcrnet_amd.search_radius(xyz, radius)
    whole = run(fits, N, mp, xyz, variant)
    csr = vcrnet_amd.search_radius(xyz, radius, capacity=cap)
    assert int(csr[2][big]) == totals[big] > cap and (csr[0][big] == -1).all()
    o = run(csr, N, mp, xyz, variant)
    for b in range(B):
        agree(cloud_of(o, b), dr.not_served(N) if b == big else cloud_of(whole, b), ("does not fit", b))
    labels, n = vcrnet_amd.cluster_dbscan(xyz, radius, mp, capacity=cap)                 # (it does not raise)
    assert np.array_equal(labels.cpu().numpy(), o["labels"]) and np.array_equal(n.cpu().numpy(), o["n_clusters"])
    assert n.cpu().numpy()[big] == -1 and (labels[big] == -2).all()
    for what, edit in (("descends", lambda rs, tot: rs.__setitem__((1, 150), rs[1, 149] - 1)),
                       ("does not start at 0", lambda rs, tot: rs.__setitem__((1, 0), 1)),
                       ("does not end at total", lambda rs, tot: tot.__setitem__(1, tot[1] + 1)),
                       ("negative", lambda rs, tot: rs.__setitem__((1, 0), -4)),
                       ("total above capacity", lambda rs, tot: tot.__setitem__(1, fits[0].shape[1] + 1))):
        rs, tot = fits[1].clone(), fits[2].clone()
        edit(rs, tot)
        o = run((fits[0], rs, tot), N, mp, xyz, variant)
        for b in range(B):
            agree(cloud_of(o, b), dr.not_served(N) if b == 1 else cloud_of(whole, b), (what, b))


@pytest.mark.parametrize("variant", FORMS)
def test_caller_built_rows(variant):
    """Asymmetric rows give the closure; -1, an index past N and the row's own index neither count nor link; an empty row; a
    border point is labelled from its own row.  No xyz: every point is finite.  The two clouds of tests/test_dbscan_cpu.py."""
    N = 7
    first = [[1], [], [1], [-1, 3, 99, N], [], [6, 6], []]
    second = [[1, 2, 3], [0], [], [0, 4, 5], [3, 5, 6], [3, 4], [4]]
    cap = max(sum(len(r) for r in rows) for rows in (first, second)) + 2
    idx = np.full((2, cap), 12345, np.int32)                # (slots behind total: never read)
    row_start = np.zeros((2, N + 1), np.int64)
    for b, rows in enumerate((first, second)):
        flat = [e for r in rows for e in r]
        idx[b, :len(flat)] = flat
        row_start[b] = np.cumsum([0] + [len(r) for r in rows])
    csr = (dev(idx), dev(row_start), dev(row_start[:, N].copy()))
    for mp, labels in ((1, ([0, 0, 0, 1, 2, 3, 3], None)), (2, ([0, -1, 1, -1, -1, 2, -1], None)), (4, (None, [0, 0, -1, 0, 0, 0, 0]))):
        o = run(csr, N, mp, None, variant)
        for b in range(2):
            agree(cloud_of(o, b), dr.sequential(idx[b], row_start[b], N, mp), (mp, b))
            if labels[b] is not None:
                assert o["labels"][b].tolist() == labels[b], (mp, b)
    # capacity 0: no idx at all, every row empty -- every point its own cluster at min_points = 1, noise above
    empty = (torch.zeros(2, 0, dtype=torch.int32, device="cuda"), dev(np.zeros((2, N + 1), np.int64)), dev(np.zeros(2, np.int64)))
    o = run(empty, N, 1, None, variant)
    assert o["labels"].tolist() == [list(range(N))] * 2 and o["n_clusters"].tolist() == [N, N] and (o["sizes"] == 1).all()
    o = run(empty, N, 2, None, variant)
    assert (o["labels"] == -1).all() and not o["n_clusters"].any() and not o["core"].any() and not o["sizes"].any()


def test_a_translation_does_not_change_the_labels():
    vcrnet_amd, _ = mods()
    x = mixed()
    radius, mp = 0.2, 5
    here = vcrnet_amd.cluster_dbscan(dev(x), radius, mp, want_core=True, want_sizes=True)
    # on the 2^-6 lattice a move by FAR is exact; elsewhere the labels are those of the MOVED cloud's own distances
    e = wr.exact_cloud(3, 300)
    a = vcrnet_amd.cluster_dbscan(dev(e), 1.0, 4, want_core=True, want_sizes=True)
    b = vcrnet_amd.cluster_dbscan(dev(e + rr.FAR[None]), 1.0, 4, want_core=True, want_sizes=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert int(a[1].min()) >= 1 and int((a[0] == -1).sum()) >= 1
    moved = (x + rr.FAR[None]).astype(np.float32)
    there = vcrnet_amd.cluster_dbscan(dev(moved), radius, mp, want_core=True, want_sizes=True)
    for b_ in range(x.shape[0]):
        want = dr.of_cloud(moved[b_], radius, mp)[0]
        got = {"labels": there[0][b_].cpu().numpy(), "n_clusters": int(there[1][b_]), "core": there[2][b_].cpu().numpy(),
               "sizes": there[3][b_].cpu().numpy()}
        agree(got, want, ("moved", b_))
    assert here[0].shape == there[0].shape


# -------------------------------------------------------------------------------------------------------------- largest_cluster

def test_largest_cluster_against_numpy():
    """The hand cloud's two clusters of five (the lower label wins), a cloud with no cluster, a cloud that was not served, and
    the mixed batch; the raw call's outputs and workspace prefilled, guard bands behind them."""
    vcrnet_amd, dbscan = mods()
    x = dr.hand_cloud()[None]
    xyz = dev(x)
    for mp, count, index in ((dr.HAND_MIN_POINTS, 5, [2, 3, 4, 6, 7]), (13, 0, []), (1, 10, [0, 2, 3, 4, 5, 6, 7, 8, 9, 10])):
        labels, n, sizes = vcrnet_amd.cluster_dbscan(xyz, dr.HAND_EPS, mp, want_sizes=True)
        points, cnt, idx = vcrnet_amd.largest_cluster(xyz, labels, sizes)
        assert int(cnt[0]) == count and idx[0, :count].tolist() == index and (idx[0, count:] == -1).all()
        assert np.array_equal(points[0, :, :count].cpu().numpy(), x[0][:, index]) and torch.isnan(points[0, :, count:]).all()
    x = mixed()
    B, _, N = x.shape
    xyz = dev(x)
    labels, n, sizes = vcrnet_amd.cluster_dbscan(xyz, 0.2, 5, want_sizes=True)
    labels[2] = -2                                          # as a cloud that was not served comes back
    sizes[2] = 0
    o = dbscan.largest_rows(xyz, labels, sizes, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    got = {k: checked(o[k], o["_raw"], k) for k in ("points", "count", "index")}
    for b in range(B):
        res = {"labels": labels[b].cpu().numpy(), "sizes": sizes[b].cpu().numpy()}
        points, count, index = dr.largest(x[b], res)
        assert got["count"][b] == count and np.array_equal(got["index"][b], index), b
        assert np.array_equal(got["points"][b].view(np.int32), points.view(np.int32)), b
    assert got["count"][0] > 0 and got["count"][2] == 0
