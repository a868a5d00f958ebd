"""vcr_outlier_radius_f32 and vcr_outlier_stat_f32 on the GPU (include/vcr_hip_outlier.h).

The radius filter is defined bit for bit and compared so: the int32 views of every output against the numpy restatement
(tests/outlier_restated.py, whose two routes tests/test_outlier_cpu.py holds to each other).  The statistical filter is checked
stage by stage: mean_dist within one fp32 ulp of the restatement fed the device's neighbours (the device's fp64 square root may
be an ulp off, which can only move a final fp32 rounding that sits on a boundary), valid and mu bit-equal to the restatement
fed the DEVICE's mean_dist, sigma and thr within 2 fp64 ulps of it (var is not an output: it is held through sigma), the
decision and the compaction exact given the device's own mean_dist and thr -- and, from the coordinates alone, the kept set
equal to the restatement's on the reference neighbours, the recipes keeping clear of their thresholds (the CPU test).
Every output buffer, and the workspace, is prefilled with a garbage byte and carries a guard band."""
import functools

import numpy as np
import pytest
import torch

import outlier_restated as orr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
RADIUS_OUT = ("points", "count", "index", "neighbours")
STAT_OUT = ("points", "count", "index", "mean_dist", "valid", "stats")


def outlier():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import outlier
    return outlier


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def fetch(o, names):
    """dict of torch -> dict of numpy; all of every output must have been overwritten, none of the band behind it."""
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in names}
    for k in names:
        raw = o["_raw"][k]
        n = o[k].numel()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * raw.element_size() and (band == SENTINEL_BYTE).all(), (k, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
        assert not (body == SENTINEL_BYTE).all(axis=1).any(), (k, "element left unwritten")
    return out


def run_radius(xyz, radius, nb_points, variant=0):
    return fetch(outlier().radius_filter(dev(xyz), radius, nb_points, variant=variant, guard=GUARD, prefill=SENTINEL_BYTE),
                 RADIUS_OUT)


def knn(xyz, k):
    """The device's neighbours of xyz [B,3,N]: (rows [B,N,4], idx int32 [B,N,k]) on the device."""
    from vcrnet_amd import native
    rows = native.to_rows4(dev(xyz))
    return rows, native.knn(rows, None, k)


def run_stat(rows, idx, ratio):
    return fetch(outlier().stat_filter(rows, idx, ratio, guard=GUARD, prefill=SENTINEL_BYTE), STAT_OUT)


def assert_same(got, want, names, what):
    for k in names:
        assert np.array_equal(orr.bits(got[k]), orr.bits(want[k])), (what, k)


@functools.lru_cache(maxsize=None)
def radius_case(name):
    """(xyz [B,3,N], radius, nb_points, the restatement's result; None for the LARGE ones): computed once, never written to."""
    xyz, r, nb = orr.RADIUS_RECIPES[name]()
    want = None if name in orr.LARGE else orr.batch(orr.radius_fast, xyz, r, nb)
    for a in [xyz] + list((want or {}).values()):
        a.setflags(write=False)
    return xyz, r, nb, want


@functools.lru_cache(maxsize=None)
def stat_case(name):
    """(xyz [B,3,N], k, std_ratio, the restatement's result on the reference neighbours): computed once."""
    xyz, k, ratio = orr.STAT_RECIPES[name]()
    want = orr.batch(orr.stat, xyz, np.stack([orr.neighbours(c, k) for c in xyz]), ratio)
    for a in [xyz] + list(want.values()):
        a.setflags(write=False)
    return xyz, k, ratio, want


# ---------------------------------------------------------------- the radius filter: no tolerance anywhere

@pytest.mark.parametrize("name", ["n1_nb0", "n1_nb1", "n255", "n256", "n257", "n1023", "n1024", "n1025", "all_kept", "none_kept",
                                  "blob_far", "copies", "lattice", "non_finite", "far_instead"])
def test_radius_against_the_restatement(name):
    """One point (nb_points 0 keeps it, 1 drops it); the block (255 / 256 / 257) and tile (1023 / 1024 / 1025) edges; a radius
    that keeps all; nb_points >= N keeps none; a blob and 5 % far points: exactly those go; duplicated points; a lattice whose
    neighbours lie ON the sphere (every d2 exact); a NaN point at index 0 and an inf point in the middle -- dropped, counted by
    nobody, the rest as in the cloud with them moved far away.  The plan's form and a forced split of two."""
    xyz, r, nb, want = radius_case(name)
    for v in (0, outlier().variant(2)):
        assert_same(run_radius(xyz, r, nb, v), want, RADIUS_OUT, (name, v))
    if name == "blob_far":
        assert np.array_equal(want["index"][0, :want["count"][0]], np.setdiff1d(np.arange(2000), orr.blob_far(12, 2000)[1]))
    if name == "non_finite":
        far = radius_case("far_instead")[3]
        assert_same(want, far, ("points", "count", "index"), name)
        rest = np.setdiff1d(np.arange(900), [0, 450])
        assert np.array_equal(want["neighbours"][0, rest], far["neighbours"][0, rest]) and not want["neighbours"][0, [0, 450]].any()


def test_radius_every_form_returns_the_same_bits():
    """N = 2049 (two tiles and a point) with the scan cut into 1, 2, 3, 8, 9, 128 segments and the plan's own number."""
    xyz, r, nb, want = radius_case("n2049")
    ol = outlier()
    assert ol.radius_form(1, 2049, cu_count=0)[1] not in (1, 2, 3)
    for s in (0, 1, 2, 3, 8, 9, 128):
        assert_same(run_radius(xyz, r, nb, ol.variant(s)), want, RADIUS_OUT, s)


def test_radius_a_batch_is_its_clouds_alone():
    xyz, r, nb, want = radius_case("three_clouds")
    got = run_radius(xyz, r, nb)
    assert_same(got, want, RADIUS_OUT, "batch")
    assert len(set(want["count"].tolist())) == 3
    for b in range(3):
        assert_same(run_radius(xyz[b:b + 1], r, nb), {k: got[k][b:b + 1] for k in RADIUS_OUT}, RADIUS_OUT, b)


@pytest.mark.parametrize("name", orr.LARGE)
def test_radius_large_clouds(name):
    """70 001 and 131 072 points: a sample of rows against the restatement's counts, and the whole of index / points / count
    against the compaction of the device's own counts."""
    xyz, r, nb, _ = radius_case(name)
    got = run_radius(xyz, r, nb)
    rows = orr.rows_of(name, xyz.shape[2])
    assert np.array_equal(got["neighbours"][0][rows], orr.radius_counts(xyz[0], r, rows))
    want = orr.compact(xyz[0], got["neighbours"][0] > nb)
    assert 0 < want["count"] < xyz.shape[2]
    assert_same({k: got[k][0] for k in want}, want, tuple(want), name)


# ---------------------------------------------------------------- the statistical filter, stage by stage

def ulps(a, b):
    """The distance of two floats of one width in units of the last place; NaN matches NaN only."""
    a, b = np.asarray(a), np.asarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(orr.bits(a).astype(np.int64) - orr.bits(b).astype(np.int64))       # (the values at hand are >= 0 or NaN)
    return np.where(both_nan, 0, np.where(np.isnan(a) | np.isnan(b), 1 << 40, d))


def check_stat(xyz, idx, ratio, got, what):
    """The stages of the docstring on the device's outputs `got` for the clouds xyz [B,3,N] and the neighbours idx [B,N,k]."""
    for b, cloud in enumerate(xyz):
        md = got["mean_dist"][b]
        want_md = orr.mean_dist_fast(cloud, idx[b])
        assert np.array_equal(np.isfinite(md), np.isfinite(want_md)), (what, b)
        fin = np.isfinite(md)
        assert (ulps(md[fin], want_md[fin]) <= 1).all(), (what, b, "mean_dist")
        d = orr.decide(md, ratio)                                                 # ... from here on, on the DEVICE's mean_dist
        mu, sigma, thr = got["stats"][b]
        assert got["valid"][b] == d["valid"] and ulps(mu, d["mu"]) == 0, (what, b, "valid, mu")
        assert ulps(sigma, d["sigma"]) <= 2 and ulps(thr, d["thr"]) <= 2, (what, b, "sigma, thr", sigma, d["sigma"], thr, d["thr"])
        with np.errstate(invalid="ignore"):
            keep = fin & (md.astype(np.float64) <= thr)                           # ... and on its own thr
        want = orr.compact(cloud, keep)
        assert_same({k: got[k][b] for k in want}, want, tuple(want), (what, b))


@pytest.mark.parametrize("name", ["n2_k1", "n255", "n256", "n257", "n1023", "n1024", "n1025", "all_kept", "ratio0", "blob_far",
                                  "copies", "non_finite", "all_nan", "k62", "n20000"])
def test_stat_against_the_restatement(name):
    """Two points, k = 1; the block and tile edges; a huge std_ratio keeps all; std_ratio 0; a blob and 5 % far points: exactly
    those go; points among their own copies (a mean distance of 0) are kept; a NaN and an inf point: dropped, valid two lower;
    nothing valid: NaN statistics, nothing kept; k = 62; 20 000 points.  Stage by stage on the device's neighbours, then the kept set from the coordinates alone."""
    xyz, k, ratio, want = stat_case(name)
    rows, idx = knn(xyz, k)
    got = run_stat(rows, idx, ratio)
    check_stat(xyz, idx.cpu().numpy(), ratio, got, name)
    assert_same(got, want, ("count", "index", "valid"), (name, "from the coordinates"))
    assert np.array_equal(orr.bits(got["points"]), orr.bits(want["points"])), name
    if name == "blob_far":
        assert np.array_equal(got["index"][0, :1900], np.setdiff1d(np.arange(2000), orr.blob_far(31, 2000)[1]))
    if name == "copies":
        zero = got["mean_dist"][0] == 0.0
        assert zero.sum() == 600 and np.isin(np.flatnonzero(zero), got["index"][0, :got["count"][0]]).all()
    if name == "non_finite":
        assert got["valid"][0] == 898 and not np.isin([0, 450], got["index"][0]).any()
    if name == "n2_k1":
        assert got["count"][0] == 2 and got["stats"][0, 1] == 0.0
    if name == "all_nan":
        assert got["count"][0] == 0 and got["valid"][0] == 0 and np.isnan(got["stats"][0, [0, 2]]).all()


def test_stat_a_batch_is_its_clouds_alone():
    xyz, k, ratio, want = stat_case("three_clouds")
    rows, idx = knn(xyz, k)
    got = run_stat(rows, idx, ratio)
    check_stat(xyz, idx.cpu().numpy(), ratio, got, "batch")
    assert_same(got, want, ("count", "index", "valid"), "from the coordinates")
    assert len(set(want["count"].tolist())) == 3
    for b in range(3):
        alone = run_stat(rows[b:b + 1].contiguous(), idx[b:b + 1].contiguous(), ratio)
        assert_same(alone, {n: got[n][b:b + 1] for n in STAT_OUT}, STAT_OUT, b)


def test_stat_idx_entries_outside_the_cloud_read_as_the_point_itself():
    xyz, k, ratio, _ = stat_case("n1025")
    rows, idx = knn(xyz, k)
    idx = idx.clone()
    N = xyz.shape[2]
    idx[0, ::7, 0] = -1
    idx[0, 1::11, 3] = N
    idx[0, 2::13, k - 1] = 2 ** 31 - 1
    idx[0, 5] = -2 ** 31
    idx[0, N - 1, :] = N + 5
    got = run_stat(rows, idx, ratio)
    host = idx.cpu().numpy()
    check_stat(xyz, host, ratio, got, "outside")
    assert got["mean_dist"][0, 5] == 0.0 and got["mean_dist"][0, N - 1] == 0.0
    inside = np.where((host >= 0) & (host < N), host, np.arange(N, dtype=np.int32)[None, :, None])
    assert_same(run_stat(rows, dev(inside), ratio), got, STAT_OUT, "the same list with the point itself written out")


# ---------------------------------------------------------------- the Python layer

def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_remove_statistical_outlier_is_the_composition_of_its_three_calls():
    import vcrnet_amd
    from vcrnet_amd import native, voxel
    xyz, k, ratio, want = stat_case("three_clouds")
    x = dev(xyz)
    points, count, index = vcrnet_amd.remove_statistical_outlier(x, nb_neighbors=k + 1, std_ratio=ratio)
    rows = native.to_rows4(x)
    o = outlier().stat_filter(rows, native.knn(rows, None, k), ratio)
    assert _eq(points, o["points"]) and _eq(count, o["count"]) and _eq(index, o["index"])
    assert points.dtype == torch.float32 and count.dtype == torch.int32 and index.dtype == torch.int32
    assert np.array_equal(index.cpu().numpy(), want["index"])
    clouds = voxel.unpad(points, count)
    assert [tuple(c.shape) for c in clouds] == [(3, int(m)) for m in want["count"]]


def test_remove_radius_outlier_and_unpad():
    import vcrnet_amd
    from vcrnet_amd import voxel
    xyz, r, nb, want = radius_case("three_clouds")
    points, count, index = vcrnet_amd.remove_radius_outlier(dev(xyz), nb, r)
    for got, name in ((points, "points"), (count, "count"), (index, "index")):
        assert np.array_equal(orr.bits(got.cpu().numpy()), orr.bits(want[name])), name
    for b, c in enumerate(voxel.unpad(points, count)):
        assert np.array_equal(orr.bits(c.cpu().numpy()), orr.bits(want["points"][b][:, :want["count"][b]]))


def test_python_refusals_come_before_any_launch():
    import vcrnet_amd
    from vcrnet_amd.native import VcrHipError
    x = torch.zeros(2, 3, 40, device="cuda")
    for bad in (1, 64, 41, 2.5, None):
        with pytest.raises(VcrHipError, match="nb_neighbors"):
            vcrnet_amd.remove_statistical_outlier(x, nb_neighbors=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(VcrHipError, match="std_ratio"):
            vcrnet_amd.remove_statistical_outlier(x, 8, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(VcrHipError, match="radius"):
            vcrnet_amd.remove_radius_outlier(x, 4, bad)
    for bad in (-1, 2.5, None):
        with pytest.raises(VcrHipError, match="nb_points"):
            vcrnet_amd.remove_radius_outlier(x, bad, 0.1)
    with pytest.raises(VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.remove_radius_outlier(x.transpose(1, 2), 4, 0.1)
    with pytest.raises(VcrHipError, match="no CPU fallback"):
        vcrnet_amd.remove_radius_outlier(x.cpu(), 4, 0.1)
    with pytest.raises(VcrHipError, match="rc=-1"):                               # the library's own check, behind Python's
        outlier().radius_filter(x, 0.1, 4, variant=2)


@pytest.mark.parametrize("spec", [("radius", 3, None), ("statistical", 12, 1.5)])
def test_register_sampled_on_filtered_clouds(spec):
    """outlier=spec, with and without voxel=: elements 0-7 are the steps done by hand (the grid, the filter on every cloud ALONE,
    the sampling cloud by cloud, vcrnetIter on the stacked samples), the indices refer to the filtered clouds, which come back
    last; too few points left raises and names the cloud; outlier=None is the call without the keyword."""
    import vcrnet_amd
    from vcrnet_amd import native, voxel
    from vcrnet_amd.module import vcrnetIter
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    npoint = 768
    h = float(np.ptp(src, axis=2).max()) / 16.0
    if spec[0] == "radius":
        spec = ("radius", 3, 1.5 * h)
    with torch.no_grad():
        for vox in (None, h):
            out = vcrnet_amd.register_sampled(net, s, t, npoint, voxel=vox, outlier=spec)
            clouds = [[c.unsqueeze(0).contiguous() for c in x] if vox is None else
                      [c.unsqueeze(0).contiguous() for c in voxel.unpad(*vcrnet_amd.voxel_down_sample(x, h)[:2])] for x in (s, t)]
            down = [[voxel.unpad(*outlier().filter_by(spec, c)[:2])[0] for c in side] for side in clouds]
            sizes = [[c.shape[1] for c in side] for side in down]
            assert all(npoint <= m < c.shape[2] for ms, side in zip(sizes, clouds) for m, c in zip(ms, side)), sizes
            picked = [[native.fps(c.unsqueeze(0).contiguous(), npoint) for c in side] for side in down]
            idx = [torch.cat([i for i, _ in p]) for p in picked]
            pts = [torch.cat([q for _, q in p]) for p in picked]
            manual = tuple(vcrnetIter(net, pts[0], pts[1], 1)) + (idx[0].long(), idx[1].long())
            assert len(out) == 9
            for a, b in zip(out[:8], manual):
                assert _eq(a, b)
            for got, want in zip(out[8], down):
                assert len(got) == 2 and all(_eq(a, b) for a, b in zip(got, want))
        both = vcrnet_amd.register_sampled(net, s, t, npoint, voxel=h, score=0.1, outlier=spec)
        assert len(both) == 10 and all(_eq(a, b) for a, b in zip(both[:8], out[:8])) and len(both[8]) == 2
        direct = vcrnet_amd.score_registration(down[0][1].unsqueeze(0), down[1][1].unsqueeze(0), out[2][1:2], out[3][1:2], max_dist=0.1)
        assert all(_eq(both[8][1][k], direct[k]) for k in direct)
        with pytest.raises(native.VcrHipError, match=r"src cloud 0 has \d+ points behind the \w+ outlier filter, fewer than npoint = 2900"):
            vcrnet_amd.register_sampled(net, s, t, 2900, outlier=("radius", 5000, spec[2]) if spec[0] == "radius" else ("statistical", 12, 0.0))
        plain = vcrnet_amd.register_sampled(net, s, t, 1024)
        none = vcrnet_amd.register_sampled(net, s, t, 1024, outlier=None)
        assert len(plain) == len(none) == 8 and all(_eq(a, b) for a, b in zip(plain, none))
