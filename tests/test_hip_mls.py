"""vcr_mls_weights_f32, vcr_mls_fit_f32 and ``smooth_mls`` on the GPU (include/smooth/vcr_hip_mls.h).

The fit of GIVEN weights -- coefficients, fit codes, points and normals -- is compared bit for bit with the numpy restatement
(tests/mls_restated.py), in every launch form; the weights, whose one library call is exp, are held to numpy's within
WEIGHT_ALLOWANCE units in the last place; the public call, which chains the two, is held to the restatement within one fp32 unit
in the last place of every coordinate.  Every raw call runs with its outputs prefilled with the byte 0xA5 and 64 elements of guard
behind them."""
import functools

import numpy as np
import pytest
import torch

import border_restated as br
import iss_restated as ir
import mls_restated as ml
import radius_restated as rr

pytestmark = pytest.mark.gpu

BYTE = 0xA5
GUARD = 64
VARIANTS = (0, "plain", "transpose")
F32, F64 = np.float32, np.float64
# What a device weight may differ from numpy's exp of the SAME argument by, in units in the last place.  The ROCm tree documents no
# bound for the device library's double exp, so the allowance is measured: the worst difference over the three noisy spheres'
# 100 036 weights and own weights (radius 0.3, all rows) on the device was one unit; the test allows 4 times that and never less
# than one unit.  profiles/mls_ledger.txt records both numbers.
WORST_MEASURED = 1.0
WEIGHT_ALLOWANCE = max(4 * WORST_MEASURED, 1.0)
H2 = 0.5                                                    # the hand-built rows' sqr_gauss_param


def mods():
    import vcrnet_amd
    from vcrnet_amd import mls
    return vcrnet_amd, mls


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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    """The same bits, a NaN against a NaN of any payload included."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def same_outputs(got, want, names=("points", "fit", "normals", "coeffs")):
    return all(same(got[k], want[k]) for k in names)


@functools.lru_cache(maxsize=None)
def hand_case():
    """Two hand-built clouds as one batch with three slots of slack -> (clouds, xyz4, normals, idx, row_start, total) on the host."""
    clouds = [ml.hand_cloud(seed) for seed in (0, 1)]
    idx, row_start, total = ir.batch([(c[2], c[3]) for c in clouds], slack=3)
    x = np.stack([c[0] for c in clouds])
    xyz4 = np.concatenate([x.transpose(0, 2, 1), np.full((2, ml.HAND_N, 1), 7.0, F32)], axis=2)
    nrm = np.stack([c[1] for c in clouds])
    for a in (xyz4, nrm, idx, row_start, total):
        a.setflags(write=False)
    return clouds, xyz4, nrm, idx, row_start, total


def stage_a(case, h2=H2):
    _, mls = mods()
    _, xyz4, nrm, idx, row_start, total = case
    o = mls.weights_rows(dev(xyz4), dev(nrm), dev(idx), dev(row_start), dev(total), h2, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    return {k: checked(o[k], o["_raw"], k) for k in ("weight", "origin", "w_self", "frame")}


def stage_b(case, given, variant=0, row_start=None, total=None, **kw):
    _, mls = mods()
    _, xyz4, nrm, idx, rs, tot = case
    o = mls.fit_rows(dev(xyz4), dev(nrm), dev(idx), dev(rs if row_start is None else row_start), dev(tot if total is None else total),
                     dev(given["weight"]), dev(given["origin"]), dev(given["w_self"]), dev(given["frame"]), variant=variant,
                     guard=GUARD, prefill=BYTE, **kw)
    torch.cuda.synchronize()
    return {k: checked(o[k], o["_raw"], k) for k in ("points", "fit", "normals", "coeffs")}


def restated_b(case, given, b, **kw):
    x, nrm, idx, row_start = case[0][b]
    got = ml.fit(x, nrm, idx, row_start, given["weight"][b], given["origin"][b], given["w_self"][b], given["frame"][b], **kw)
    return dict(got, coeffs=got["coeffs"])


def weight_ulps(got, want):
    """The largest difference of the device's weights to numpy's in units in the last place; the zeros and the NaNs must agree."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    zero = (want == 0) & ~nan
    assert np.array_equal((got == 0) & ~nan, zero)
    rest = ~nan & ~zero
    return ml.ulps(got[rest], want[rest])


# ------------------------------------------------------------------------------------------------------------------- stage A

def test_stage_a_on_hand_built_rows():
    """B = 2, N = 200, rows of 0, 1, 2, 4, 5, 6, 63, 64, 65, 128 and 129 entries with entries outside [0, N), the point itself, a
    copy of it, a NaN point inside rows, a NaN point that owns a row and a zero normal: origin and frame bit for bit, the weights
    within the allowance, NaN behind total.  The frame is the boundary pass's: the same flags from the same normals on the device,
    and the device's angles are numpy's atan2 in THIS restatement's nh, u and nh x u."""
    _, mls = mods()
    from vcrnet_amd import border
    case = hand_case()
    clouds, xyz4, nrm, idx, row_start, total = case
    got = stage_a(case)
    cap = idx.shape[1]
    worst = 0.0
    for b, (x, n, ix, rs) in enumerate(clouds):
        want = ml.weights(x, n, ix, rs, H2, cap)
        assert same(got["origin"][b], want[1]) and np.array_equal(got["frame"][b], want[3]), b
        assert np.isnan(got["weight"][b, total[b]:]).all() and total[b] + 3 == cap
        worst = max(worst, weight_ulps(got["weight"][b], want[0]), weight_ulps(got["w_self"][b], want[2]))
        assert got["frame"][b].tolist().count(0) == 3 and (want[0] == 0).sum() > 10
    print("hand-built rows: worst weight deviation", worst, "units in the last place; allowance", WEIGHT_ALLOWANCE)
    assert worst <= WEIGHT_ALLOWANCE
    o = border.angles_rows(dev(xyz4), dev(nrm), dev(idx), dev(row_start), dev(total), want_frame=True)
    assert np.array_equal(o["frame"].cpu().numpy(), got["frame"])
    ang = o["angle"].cpu().numpy()
    for b, (x, n, ix, rs) in enumerate(clouds):
        for i in (0, 7, 30, 63, 199):
            fm = ml.frame(x[:, i], n[:, i])
            h, u = fm[0], fm[1]
            v = np.asarray([h[1] * u[2] - h[2] * u[1], h[2] * u[0] - h[0] * u[2], h[0] * u[1] - h[1] * u[0]])
            d, _ = ml.differences(x, i, ix[rs[i]:rs[i + 1]])
            pu, pv = (u[0] * d[0] + u[1] * d[1]) + u[2] * d[2], (v[0] * d[0] + v[1] * d[1]) + v[2] * d[2]
            mine = ang[b, rs[i]:rs[i + 1]]
            ok = ~np.isnan(mine)
            assert np.abs(mine[ok] - np.arctan2(pv, pu)[ok]).max(initial=0.0) <= 4 * 4.440892098500626e-16, (b, i)
            assert np.array_equal(ok, ~np.isnan(br.angles(x, n, ix, rs)[0][rs[i]:rs[i + 1]]))


# ------------------------------------------------------------------------------------------------------------------- stage B

def random_given(case, seed=5):
    """(weight, origin, w_self, frame) that no stage A wrote: uniform weights with exact zeros, small origins, a tenth of the
    frames 0."""
    rs = np.random.RandomState(seed)
    _, xyz4, _, idx, _, _ = case
    B, N, cap = xyz4.shape[0], xyz4.shape[1], idx.shape[1]
    w = rs.uniform(0, 1, (B, cap))
    w[rs.uniform(size=w.shape) < 0.05] = 0.0
    return {"weight": w, "origin": 0.05 * rs.normal(size=(B, N, 3)), "w_self": rs.uniform(0.2, 1, (B, N)),
            "frame": (rs.uniform(size=(B, N)) > 0.1).astype(np.int32)}


@pytest.mark.parametrize("given", ["stage A's", "random"])
def test_stage_b_from_given_inputs_is_the_restatement_bit_for_bit(given):
    """Every row length of the hand-built case, the collinear row and the row of equal points (their pivot fails: the plane alone),
    with order 1 and with a larger min_neighbors; in every launch form."""
    case = hand_case()
    g = stage_a(case) if given == "stage A's" else random_given(case)
    if given == "stage A's":
        g = {k: np.nan_to_num(v, nan=0.25) if k != "frame" else v for k, v in g.items()}     # (a NaN is not a given weight)
    seen = set()
    for kw in (dict(), dict(order=1), dict(min_neighbors=6)):
        got = [stage_b(case, g, variant, **kw) for variant in VARIANTS]
        for other in got[1:]:
            assert same_outputs(other, got[0]), kw
        for b in range(2):
            want = restated_b(case, g, b, **kw)
            for k in ("fit", "coeffs", "points", "normals"):
                assert same(got[0][k][b], want[k]), (given, kw, b, k)
            seen |= set(want["fit"].tolist())
            if not kw and given == "stage A's":
                assert want["fit"][ml.COLLINEAR] == 1 and want["fit"][ml.EQUAL] == 1 and (want["fit"] == 2).sum() > 80
    assert seen == {0, 1, 2}


def test_a_cloud_that_is_not_served_is_voided_alone_and_nothing_is_written_past_the_end():
    case = hand_case()
    clouds, xyz4, nrm, idx, row_start, total = case
    g = random_given(case)
    whole = stage_b(case, g)
    wa = stage_a(case)
    _, mls = mods()
    for what, edit in (("descends", lambda rs, tot: rs.__setitem__((1, 100), rs[1, 99] - 1)),
                       ("does not start at 0", lambda rs, tot: rs.__setitem__((1, 0), 1)),
                       ("does not end at total", lambda rs, tot: tot.__setitem__(1, tot[1] - 1)),
                       ("exceeds the capacity", lambda rs, tot: (tot.__setitem__(1, idx.shape[1] + 1),
                                                                 rs.__setitem__((1, ml.HAND_N), idx.shape[1] + 1)))):
        rs, tot = row_start.copy(), total.copy()
        edit(rs, tot)
        for variant in VARIANTS[1:]:
            got = stage_b(case, g, variant, row_start=rs, total=tot)
            assert np.isnan(got["points"][1]).all() and np.isnan(got["normals"][1]).all() and np.isnan(got["coeffs"][1]).all(), what
            assert (got["fit"][1] == -2).all(), what
            assert all(same(got[k][0], whole[k][0]) for k in whole), what
        o = mls.weights_rows(dev(xyz4), dev(nrm), dev(idx), dev(rs), dev(tot), H2, guard=GUARD, prefill=BYTE)
        torch.cuda.synchronize()
        a = {k: checked(o[k], o["_raw"], k) for k in ("weight", "origin", "w_self", "frame")}
        assert np.isnan(a["weight"][1]).all() and np.isnan(a["origin"][1]).all() and np.isnan(a["w_self"][1]).all(), what
        assert (a["frame"][1] == -2).all() and all(same(a[k][0], wa[k][0]) for k in wa), what


# --------------------------------------------------------------------------------------------------------------- the public call

@functools.lru_cache(maxsize=None)
def spheres():
    x = np.stack([ml.noisy_sphere(seed) for seed in ml.SEEDS])
    x.setflags(write=False)
    return x


def rows_and_normals(x, radius, max_nn=None):
    """The device's rows of a batch and the normals it estimates on them, turned outward -> (idx, row_start, total, normals) as
    numpy."""
    vcrnet_amd, _ = mods()
    from vcrnet_amd import native, rows
    xyz = dev(x)
    csr = vcrnet_amd.search_radius(xyz, radius, max_nn=max_nn)
    nrm = rows.normals(native.to_rows4(xyz), *csr, want_curvature=False)[0].cpu().numpy()
    return [t.cpu().numpy() for t in csr] + [np.stack([ml.outward(x[b], nrm[b]) for b in range(x.shape[0])])]


def run_public(x, radius, nrm, **kw):
    vcrnet_amd, _ = mods()
    got = vcrnet_amd.smooth_mls(dev(x), radius, None if nrm is None else dev(nrm), want_normals=True, want_coeffs=True, **kw)
    torch.cuda.synchronize()
    return dict(zip(("points", "fit", "normals", "coeffs"), [g.cpu().numpy() for g in got]))


def test_the_weights_allowance_on_the_three_spheres():
    """THE measurement the allowance rests on: stage A on the three noisy spheres (radius 0.3, every row) against numpy's exp of the
    restatement's argument, which is the device's to the bit (the origins are compared bit for bit)."""
    _, mls = mods()
    from vcrnet_amd import native
    x = spheres()
    idx, row_start, total, nrm = rows_and_normals(x, ml.SPHERE_RADIUS)
    h2 = ml.SPHERE_RADIUS * ml.SPHERE_RADIUS
    o = mls.weights_rows(native.to_rows4(dev(x)), dev(nrm), dev(idx), dev(row_start), dev(total), h2)
    worst = 0.0
    for b in range(3):
        want = ml.weights(x[b], nrm[b], idx[b], row_start[b], h2, idx.shape[1])
        assert same(o["origin"][b].cpu().numpy(), want[1]) and (want[3] == 1).all()
        worst = max(worst, weight_ulps(o["weight"][b].cpu().numpy(), want[0]), weight_ulps(o["w_self"][b].cpu().numpy(), want[2]))
    print("three spheres: worst weight deviation", worst, "units in the last place over", int(total.sum()) + 3 * ml.SPHERE_N,
          "weights; allowance", WEIGHT_ALLOWANCE)
    assert worst <= WEIGHT_ALLOWANCE


@pytest.mark.parametrize("radius,max_nn", [(ml.SPHERE_RADIUS, None), (0.7, None), (ml.SPHERE_RADIUS, 30)])
def test_smooth_mls_on_the_noisy_spheres(radius, max_nn):
    """The three seeds as one batch: every coordinate of every point and normal within ONE fp32 unit in the last place of the
    restatement's (the one difference is exp's last places, about 1e-16 relative: orders below fp32's 6e-8 through a 6 x 6 solve,
    so a coordinate differs only where the fp64 value lies at a rounding boundary), every fit code equal; at radius 0.3 the
    smoothing condition of the CPU suite on the DEVICE's output."""
    x = spheres()
    idx, row_start, total, nrm = rows_and_normals(x, radius, max_nn)
    got = run_public(x, radius, nrm, max_nn=max_nn)
    n = np.diff(row_start, axis=1)
    print("rows of", int(n.min()), "to", int(n.max()), "entries")
    assert (n.max() > 128) == (radius == 0.7) and (max_nn is None or n.max() == max_nn)
    for b in range(3):
        want = ml.definition(x[b], nrm[b], (idx[b], row_start[b], int(total[b])), radius * radius, capacity=idx.shape[1])
        assert np.array_equal(got["fit"][b], want["fit"]) and (want["fit"] == 2).all(), b
        up, un = ml.ulps32(got["points"][b], want["points"]), ml.ulps32(got["normals"][b], want["normals"])
        print("cloud", b, "coordinates off by one unit:", int((up == 1).sum()), "of points,", int((un == 1).sum()), "of normals")
        assert up.max() <= 1 and un.max() <= 1, b
        assert np.allclose(got["coeffs"][b], want["coeffs"], rtol=1e-9, atol=1e-12)
        if radius == ml.SPHERE_RADIUS and max_nn is None:
            rms_in, rms_out, ang_in, ang_out = ml.smoothing(x[b], nrm[b], {"points": got["points"][b], "normals": got["normals"][b]})
            one = run_public(x[b:b + 1], radius, nrm[b:b + 1], order=1)
            rms_one = ml.radial_rms(one["points"][0])
            print("cloud", b, "rms in", rms_in, "order 2", rms_out, "order 1", rms_one, "angle in", ang_in, "out", ang_out)
            assert rms_out <= 0.5 * rms_in and rms_one >= rms_in and ang_out < ang_in and (one["fit"] == 1).all()
            assert ml.ulps32(one["points"][0], ml.definition(x[b], nrm[b], (idx[b], row_start[b]), radius * radius, order=1)["points"]).max() <= 1


def test_batching_capacity_and_estimated_normals():
    """A cloud alone and as the second of three returns the same bits; with a capacity too small for one cloud that cloud is NaN / -2
    and the others return the bits they return alone; normals=None is the estimate on the same rows."""
    vcrnet_amd, _ = mods()
    from vcrnet_amd import native, rows
    x = spheres().copy()
    x[1] *= F32(0.8)                                         # the middle cloud is denser: longer rows
    _, _, total, nrm = rows_and_normals(x, ml.SPHERE_RADIUS)
    assert total[1] > total[0] and total[1] > total[2]
    whole = run_public(x, ml.SPHERE_RADIUS, nrm)
    for b in (0, 1):
        alone = run_public(x[b:b + 1], ml.SPHERE_RADIUS, nrm[b:b + 1])
        assert all(same(alone[k][0], whole[k][b]) for k in whole), b
    got = run_public(x, ml.SPHERE_RADIUS, nrm, capacity=int(max(total[0], total[2])))
    assert np.isnan(got["points"][1]).all() and np.isnan(got["normals"][1]).all() and np.isnan(got["coeffs"][1]).all()
    assert (got["fit"][1] == -2).all()
    for b in (0, 2):
        assert all(same(got[k][b], whole[k][b]) for k in whole), b
    xyz = dev(x)
    csr = vcrnet_amd.search_radius(xyz, ml.SPHERE_RADIUS)
    est = rows.normals(native.to_rows4(xyz), *csr, want_curvature=False)[0].cpu().numpy()
    none, given = run_public(x, ml.SPHERE_RADIUS, None), run_public(x, ml.SPHERE_RADIUS, est)
    assert all(same(none[k], given[k]) for k in none) and (none["fit"] == 2).all()
    two = vcrnet_amd.smooth_mls(xyz, ml.SPHERE_RADIUS)
    assert len(two) == 2 and same(two[0].cpu().numpy(), none["points"]) and two[1].dtype == torch.int32


def test_a_translated_cloud_returns_the_same_coefficients():
    """Coordinates on a grid of 2^-12: adding 1024, -512, 256 is exact in fp32 and every difference keeps its bits; the fit reads
    differences alone."""
    x = spheres()[:2]
    q = (np.round(x * 4096.0) / 4096.0).astype(F32)
    far = (q + rr.FAR[None]).astype(F32)
    assert np.array_equal((far - rr.FAR[None]).astype(F32), q) and np.abs(far).max() > 1024
    nrm = rows_and_normals(q, ml.SPHERE_RADIUS)[3]
    near_, far_ = run_public(q, ml.SPHERE_RADIUS, nrm), run_public(far, ml.SPHERE_RADIUS, nrm)
    assert same(near_["coeffs"], far_["coeffs"]) and np.array_equal(near_["fit"], far_["fit"]) and same(near_["normals"], far_["normals"])
    assert (near_["fit"] == 2).all() and np.abs(far_["points"] - rr.FAR[None] - near_["points"]).max() < 2e-4


def test_the_lattice_in_a_plane_comes_back_with_its_bits():
    x, nrm = ml.plane_lattice()
    got = run_public(x[None], 4.0, nrm[None])
    assert (got["fit"] == 2).all() and same(got["points"][0], x) and (got["coeffs"] == 0).all() and same(got["normals"][0], nrm)


def test_one_point_copies_of_a_point_and_min_neighbors_above_every_row():
    one = np.asarray([[[0.5], [-0.25], [2.0]]], F32)
    up = np.asarray([[[0.0], [0.0], [1.0]]], F32)
    for nrm in (up, None):
        got = run_public(one, 0.1, nrm)
        assert same(got["points"], one) and got["fit"].tolist() == [[0]] and (got["coeffs"] == 0).all()
    assert same(run_public(one, 0.1, up)["normals"], up)
    copies = np.repeat(one, 40, axis=2)
    nrm = np.repeat(up, 40, axis=2)
    got = run_public(copies, 0.1, nrm)
    rows = ml.hybrid_rows(copies[0], 0.1)
    want = ml.of_cloud(copies[0], nrm[0], 0.1, rows=rows)
    assert (np.diff(rows["row_start"]) == 39).all() and (want["fit"] == 1).all()
    assert np.array_equal(got["fit"][0], want["fit"]) and same(got["points"][0], copies[0]) and same(got["normals"][0], nrm[0])
    x = spheres()[:1]
    nrm = rows_and_normals(x, ml.SPHERE_RADIUS)[3]
    got = run_public(x, ml.SPHERE_RADIUS, nrm, min_neighbors=1000)
    assert (got["fit"] == 0).all() and same(got["points"], x) and (got["coeffs"] == 0).all()
    assert ml.ulps32(got["normals"][0], (nrm[0].astype(F64) / np.sqrt((nrm[0].astype(F64) ** 2).sum(0))).astype(F32)).max() <= 1
