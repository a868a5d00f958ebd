"""vcr_border_angles_f32, vcr_border_gap_f32, vcr_border_near_f32, ``compute_boundary_points`` and the border rule of
``compute_iss_keypoints`` on the GPU (include/border/vcr_hip_border.h).

The gap, the flags and the spreading are compared bit for bit with the numpy restatement (tests/border_restated.py); the angles,
whose one library call is atan2, are held to numpy's within ANGLE_ALLOWANCE, and the device's own angles fed to the numpy gap
stage reproduce the device's gap to the bit.  Every raw call runs with its outputs prefilled with the byte 0xA5 and 64 elements of
guard behind them; the gap runs in the plan's form, as a lane a row and as a wave a row, and the three must agree."""
import functools
import math

import numpy as np
import pytest
import torch

import border_restated as br
import iss_restated as ir
import radius_restated as rr

pytestmark = pytest.mark.gpu

BYTE = 0xA5
GUARD = 64
FORMS = (0, "lane", "wave")
F32 = np.float32
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 129, br.CHUNK + 1)
# What a device angle may differ from numpy's by.  The ROCm tree documents no bound for the device library's double atan2, so the
# allowance is measured: the worst difference over this file's four recipes on the device was 4.440892098500626e-16 (one unit in
# the last place of pi) in each of them; 4 times that, which is far below the cap of 1e-12.  profiles/border_ledger.txt records
# both numbers.
WORST_MEASURED = 4.440892098500626e-16
ANGLE_ALLOWANCE = min(4 * WORST_MEASURED, 1e-12)


def mods():
    import vcrnet_amd
    from vcrnet_amd import border
    return vcrnet_amd, border


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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def gap_in_every_form(angle, row_start, total, min_neighbors=3, threshold=math.pi / 2, frame=None, d2=None, r2=None):
    """gap_rows on device tensors in the three forms, which must agree -> (gap, flag) as numpy."""
    _, border = mods()
    got = []
    for variant in FORMS:
        o = border.gap_rows(angle, row_start, total, min_neighbors, threshold, frame=frame, d2=d2, r2=r2, variant=variant,
                            guard=GUARD, prefill=BYTE)
        torch.cuda.synchronize()
        got.append((checked(o["gap"], o["_raw"], "gap"), checked(o["flag"], o["_raw"], "flag")))
        assert same_bits(got[-1][0], got[0][0]) and np.array_equal(got[-1][1], got[0][1]), variant
    return got[0]


# ------------------------------------------------------------------------------------------------------- the gap of given angles

def angle_batch(per_cloud, capacity):
    """[(angle, row_start)] -> (angle [B,capacity] with 7.0 behind each total, row_start [B,N+1], total [B])."""
    ang = np.full((len(per_cloud), capacity), 7.0)
    for b, (a, _) in enumerate(per_cloud):
        ang[b, :min(len(a), capacity)] = a[:capacity]
    row_start = np.stack([rs for _, rs in per_cloud])
    return ang, row_start, row_start[:, -1].copy()


@pytest.mark.parametrize("min_neighbors", [1, 3])
@pytest.mark.parametrize("B,N", [(1, 1), (1, 2), (3, 700)])
def test_the_gap_of_given_angles_is_the_restatement_bit_for_bit(B, N, min_neighbors):
    """Rows of 0, 1, 2, 3, 63, 64, 65, 129 and a chunk + 1 slots, a tenth of the slots NaN, rows of NaN alone, copies of angles.
    With B = 3 the middle cloud's rows are twice as long: it does not fit the capacity and nothing of it may be read."""
    lengths = [LENGTHS[(i + N) % len(LENGTHS)] for i in range(N)]
    clouds = [br.rows_of_angles(lengths if b != 1 else [2 * v for v in lengths], seed=10 * N + b, nan_rows=(1, 5, 8, 13))
              for b in range(B)]
    capacity = max(int(c[1][-1]) for b, c in enumerate(clouds) if b != 1) + 3
    ang, row_start, total = angle_batch(clouds, capacity)
    assert B == 1 or total[1] > capacity
    for thr in (math.pi / 2, 0.3):
        gap, flag = gap_in_every_form(dev(ang), dev(row_start), dev(total), min_neighbors, thr)
        for b in range(B):
            if b == 1:
                assert np.isnan(gap[b]).all() and (flag[b] == -2).all()
                continue
            want = br.gaps(clouds[b][0], clouds[b][1], min_neighbors, thr)
            assert same_bits(gap[b], want[0]) and np.array_equal(flag[b], want[1]), (b, thr)
        if N == 700:
            assert 0 < (flag[0] > 0).sum() < N and (gap[0] == 0).any()
    # a frame: gap NaN and flag 0 where it is 0, the other rows as they were
    frame = (np.arange(B * N).reshape(B, N) % 7 != 0).astype(np.int32)
    g2, f2 = gap_in_every_form(dev(ang), dev(row_start), dev(total), min_neighbors, 0.3, frame=dev(frame))
    for b in range(B):
        if b != 1:
            want = br.gaps(clouds[b][0], clouds[b][1], min_neighbors, 0.3, frame[b])
            assert same_bits(g2[b], want[0]) and np.array_equal(f2[b], want[1]) and np.isnan(g2[b][frame[b] == 0]).all()


def test_a_row_start_that_descends_voids_its_cloud_alone():
    N = 700
    lengths = [LENGTHS[i % len(LENGTHS)] for i in range(N)]
    clouds = [br.rows_of_angles(lengths, seed=40 + b) for b in range(3)]
    ang, row_start, total = angle_batch(clouds, int(clouds[0][1][-1]) + 5)
    whole = gap_in_every_form(dev(ang), dev(row_start), dev(total))
    for what, edit in (("descends", lambda rs, tot: rs.__setitem__((1, 350), rs[1, 349] - 1)),
                       ("does not start at 0", lambda rs, tot: rs.__setitem__((1, 0), 1)),
                       ("does not end at total", lambda rs, tot: tot.__setitem__(1, tot[1] - 1)),
                       ("negative", lambda rs, tot: rs.__setitem__((1, 0), -4))):
        rs, tot = row_start.copy(), total.copy()
        edit(rs, tot)
        gap, flag = gap_in_every_form(dev(ang), dev(rs), dev(tot))
        assert np.isnan(gap[1]).all() and (flag[1] == -2).all(), what
        for b in (0, 2):
            assert same_bits(gap[b], whole[0][b]) and np.array_equal(flag[b], whole[1][b]), (what, b)


# ------------------------------------------------------------------------------------------------------------------- the angles

@functools.lru_cache(maxsize=None)
def recipe(name):
    make, radius = br.RECIPES[name]
    x, nrm = make()
    x.setflags(write=False)
    nrm.setflags(write=False)
    return x, nrm, radius


@pytest.mark.parametrize("name", ["lattice", "sphere", "capped", "degenerate"])
def test_the_angles_against_the_restatement(name):
    """On search_radius' hybrid rows with two slots of slack: the skipped slots are the restatement's, the slots behind the rows
    are NaN, every counted angle is within ANGLE_ALLOWANCE of numpy's, and numpy's gap stage on the DEVICE'S angles returns the
    device's gap and flags bit for bit."""
    vcrnet_amd, border = mods()
    from vcrnet_amd import native
    x, nrm, radius = recipe(name)
    xyz = dev(x[None])
    total = int(vcrnet_amd.search_radius(xyz, radius, max_nn=30)[2][0])
    idx, row_start, tot = vcrnet_amd.search_radius(xyz, radius, max_nn=30, capacity=total + 2)
    o = border.angles_rows(native.to_rows4(xyz), dev(nrm[None]), idx, row_start, tot, want_frame=True, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    ang, frame = checked(o["angle"], o["_raw"], "angle")[0], checked(o["frame"], o["_raw"], "frame")[0]
    want, wframe, skipped = br.angles(x, nrm, idx[0].cpu().numpy(), row_start[0].cpu().numpy(), capacity=total + 2)
    assert np.array_equal(frame, wframe) and np.array_equal(np.isnan(ang), skipped) and skipped[total:].all()
    worst = float(np.abs(ang - want)[~skipped].max())
    print("angles", name, "counted", int((~skipped).sum()), "skipped in rows", int(skipped[:total].sum()),
          "worst |device - numpy|", worst)
    assert worst <= ANGLE_ALLOWANCE
    assert (np.abs(ang[~skipped]) <= math.pi).all()
    if name == "degenerate":
        assert frame.tolist().count(0) == 3 and skipped[:total].sum() > 8
    thr = br.radians(90.0)
    gap, flag = gap_in_every_form(o["angle"], row_start, tot, 3, thr, frame=o["frame"])
    wgap, wflag = br.gaps(ang, row_start[0].cpu().numpy(), 3, thr, frame)
    assert same_bits(gap[0], wgap) and np.array_equal(flag[0], wflag)
    # ... and on numpy's own angles the same flags: no gap lies at the threshold (tests/test_border_cpu.py)
    ngap, nflag = br.gaps(want, row_start[0].cpu().numpy(), 3, thr, wframe)
    ok = ~np.isnan(ngap)
    assert np.array_equal(flag[0], nflag) and np.abs(gap[0] - ngap)[ok].max() <= 2 * ANGLE_ALLOWANCE
    assert np.array_equal(np.isnan(gap[0]), ~ok)


def test_the_prefix_of_a_larger_search_is_the_smaller_search():
    """The three passes on the rows of a search at 0.6 cut by d2 <= fp32(0.35^2) against the rows of a search at 0.35."""
    vcrnet_amd, border = mods()
    from vcrnet_amd import native
    x, nrm = br.sphere(300)
    xyz, normals = dev(x[None]), dev(nrm[None])
    xyz4 = native.to_rows4(xyz)
    idx, row_start, total, d2 = vcrnet_amd.search_radius(xyz, 0.6, want_d2=True)
    small = vcrnet_amd.search_radius(xyz, 0.35)
    r2 = float(rr.r2_of(0.35))
    thr = br.radians(60.0)
    a1 = border.angles_rows(xyz4, normals, idx, row_start, total, d2=d2, r2=r2, want_frame=True)
    a2 = border.angles_rows(xyz4, normals, *small, want_frame=True)
    g1 = gap_in_every_form(a1["angle"], row_start, total, 3, thr, frame=a1["frame"], d2=d2, r2=r2)
    g2 = gap_in_every_form(a2["angle"], small[1], small[2], 3, thr, frame=a2["frame"])
    assert same_bits(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])
    want = br.definition(x, nrm, (idx[0].cpu().numpy(), row_start[0].cpu().numpy()), 3, thr, d2=d2[0].cpu().numpy(), r2=r2)
    assert np.array_equal(np.isnan(a1["angle"][0].cpu().numpy()), np.isnan(want["angle"]))
    flag = dev(g1[1])
    n1 = border.near_rows(flag, idx, row_start, total, d2=d2, r2=r2)["near"]
    n2 = border.near_rows(flag, *small)["near"]
    assert torch.equal(n1, n2)


# --------------------------------------------------------------------------------------------------------------- the public call

def run_public(x, nrm, radius, **kw):
    vcrnet_amd, _ = mods()
    got = vcrnet_amd.compute_boundary_points(dev(x), None if nrm is None else dev(nrm), radius, want_flag=True, want_gap=True, **kw)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def selected(points, count, index, x, flag):
    """(points, count, index) are the flagged points in index order, NaN / -1 behind them."""
    for b in range(x.shape[0]):
        at = np.flatnonzero(flag[b] > 0)
        assert count[b] == len(at) and np.array_equal(index[b][:len(at)], at) and (index[b][len(at):] == -1).all()
        assert same_bits(points[b][:, :len(at)], x[b][:, at]) and np.isnan(points[b][:, len(at):]).all()


@pytest.mark.parametrize("name", ["lattice", "sphere", "capped"])
def test_compute_boundary_points_on_surfaces_whose_rim_is_known(name):
    x, nrm, radius = recipe(name)
    points, count, index, flag, gap = run_public(x[None], nrm[None], radius)
    want = br.of_cloud(x, nrm, radius)
    assert np.array_equal(flag[0], want["flag"]) and np.array_equal(index[0], want["index"]) and count[0] == want["count"]
    assert same_bits(points[0], want["points"]) and np.abs(gap[0] - want["gap"]).max() <= 2 * ANGLE_ALLOWANCE
    selected(points, count, index, x[None], flag)
    if name == "lattice":
        assert np.array_equal(flag[0] > 0, br.lattice()[2]) and count[0] == 60
    elif name == "sphere":
        assert count[0] == 0 and not flag.any() and np.isnan(points).all()
    else:
        touched = br.touched()
        t = np.arcsin(np.float64(br.CUT)) - np.arcsin(np.clip(x[2].astype(np.float64), -1, 1))
        assert not (flag[0] > 0)[~touched].any() and (flag[0] > 0)[t <= 0.4 * br.SPHERE_RADIUS].all() and count[0] >= 20
    vcrnet_amd, _ = mods()
    three = vcrnet_amd.compute_boundary_points(dev(x[None]), dev(nrm[None]), radius)
    assert len(three) == 3 and np.array_equal(three[1].cpu().numpy(), count) and np.array_equal(three[2].cpu().numpy(), index)
    # all the points within the radius (no row reaches the cap of 30), and the angle in degrees
    every = run_public(x[None], nrm[None], radius, max_nn=None)
    assert np.array_equal(every[3], flag) and same_bits(every[4], gap)
    low = run_public(x[None], nrm[None], radius, angle_threshold=40.0)
    assert same_bits(low[4], gap) and np.array_equal(low[3][0], (gap[0] > br.radians(40.0)).astype(np.int32))


def lattices():
    xs, ns = zip(*(br.lattice(seed=s)[:2] for s in (11, 12, 13)))
    return np.stack(xs), np.stack(ns)


def test_a_batch_of_three_equals_its_clouds_alone_and_a_translated_cloud_returns_the_same_bits():
    x, nrm = lattices()
    whole = run_public(x, nrm, 1.6)
    for b in range(3):
        one = run_public(x[b:b + 1], nrm[b:b + 1], 1.6)
        want = br.of_cloud(x[b], nrm[b], 1.6)
        assert np.array_equal(one[3][0], want["flag"])
        for u, v in zip(whole, one):
            assert same_bits(u[b], v[0]), b
    # coordinates on a grid of 2^-12: adding 1024, -512, 256 is exact in fp32, every difference keeps its bits
    q = (np.round(x * 4096.0) / 4096.0).astype(F32)
    far = (q + rr.FAR[None]).astype(F32)
    assert np.array_equal((far - rr.FAR[None]).astype(F32), q)
    near_, far_ = run_public(q, nrm, 1.6), run_public(far, nrm, 1.6)
    for k in (1, 2, 3, 4):
        assert same_bits(near_[k], far_[k]), k
    assert same_bits(far_[0][:, :, :60], (near_[0] + rr.FAR[None])[:, :, :60].astype(F32)) and (near_[1] == 60).all()


def test_estimated_normals_are_those_of_the_same_rows():
    vcrnet_amd, _ = mods()
    from vcrnet_amd import native, rows
    x, _, radius = recipe("capped")
    xyz = dev(x[None])
    csr = vcrnet_amd.search_radius(xyz, radius, max_nn=30)
    nrm = rows.normals(native.to_rows4(xyz), *csr)[0]
    got = vcrnet_amd.compute_boundary_points(xyz, None, radius, want_flag=True, want_gap=True)
    given = vcrnet_amd.compute_boundary_points(xyz, nrm, radius, want_flag=True, want_gap=True)
    for u, v in zip(got, given):
        assert same_bits(u.cpu().numpy(), v.cpu().numpy())
    flagged = got[3][0].cpu().numpy() > 0
    assert flagged.sum() >= 20 and not flagged[~br.touched()].any()
    # fewer points than max_nn + 1: the cap is no cap
    tiny = run_public(x[None, :, :20], None, radius)
    assert tiny[3].shape == (1, 20) and (tiny[3] >= 0).all()


def test_a_cloud_that_does_not_fit_the_capacity_comes_back_empty():
    vcrnet_amd, _ = mods()
    x, nrm = lattices()
    x = x.copy()
    x[1] *= F32(0.75)                                        # the middle cloud is denser: longer rows
    totals = vcrnet_amd.search_radius(dev(x), 1.6, max_nn=30)[2].cpu().numpy()
    assert totals[1] > totals[0] == totals[2]
    fits = run_public(x, nrm, 1.6)
    got = run_public(x, nrm, 1.6, capacity=int(totals[0]))
    assert got[1][1] == 0 and (got[3][1] == -2).all() and np.isnan(got[4][1]).all() and np.isnan(got[0][1]).all()
    assert (got[2][1] == -1).all()
    for b in (0, 2):
        for u, v in zip(got, fits):
            assert same_bits(u[b], v[b]), b
    assert fits[1][1] > 0


# ---------------------------------------------------------------------------------------------------------------- the spreading

@pytest.mark.parametrize("prefix", [False, True])
def test_near_rows_against_numpy(prefix):
    vcrnet_amd, border = mods()
    x = np.stack([br.sphere(700)[0], ir.bumpy(700), ir.cube(700, 3)])
    idx, row_start, total, d2 = vcrnet_amd.search_radius(dev(x), 0.3, want_d2=True)
    flag = (np.random.RandomState(3).uniform(size=(3, 700)) < 0.03).astype(np.int32)
    flag[0, ::50] = -1                                      # (a flag below 0 that is not -2 is no flag and voids nothing)
    r2 = float(rr.r2_of(0.17)) if prefix else None
    kw = dict(d2=d2, r2=r2) if prefix else {}
    o = border.near_rows(dev(flag), idx, row_start, total, guard=GUARD, prefill=BYTE, **kw)
    torch.cuda.synchronize()
    near = checked(o["near"], o["_raw"], "near")
    h = [t.cpu().numpy() for t in (idx, row_start, d2)]
    for b in range(3):
        want = br.near(flag[b], h[0][b], h[1][b], h[2][b] if prefix else None, r2)
        assert np.array_equal(near[b], want), b
        assert (flag[b] > 0).sum() < (near[b] > 0).sum() < 700
    if prefix:
        whole = border.near_rows(dev(flag), idx, row_start, total)["near"].cpu().numpy()
        assert ((near > 0) <= (whole > 0)).all() and (near > 0).sum() < (whole > 0).sum()
    # the flags of a cloud that was not served, and rows that are not: that cloud alone is -2
    flag[1, 17] = -2
    got = border.near_rows(dev(flag), idx, row_start, total, **kw)["near"].cpu().numpy()
    assert (got[1] == -2).all() and np.array_equal(got[0], near[0]) and np.array_equal(got[2], near[2])
    flag[1, 17] = 0
    rs = row_start.clone()
    rs[2, 300] = rs[2, 299] - 1
    got = border.near_rows(dev(flag), idx, rs, total, **kw)["near"].cpu().numpy()
    assert (got[2] == -2).all() and np.array_equal(got[0], near[0]) and (got[1] >= 0).all()


# ---------------------------------------------------------------------------------------------------------- the keypoints' rule

ISS = dict(salient_radius=0.3, non_max_radius=0.2, gamma_21=0.99, gamma_32=0.99, min_neighbors=5)
BORDER_RADIUS = 0.25


def test_the_keypoints_without_a_border_radius_are_the_bits_they_were():
    vcrnet_amd, _ = mods()
    x, _, _ = recipe("capped")
    xyz = dev(x[None])
    plain = vcrnet_amd.compute_iss_keypoints(xyz, want_flag=True, want_saliency=True, **ISS)
    none = vcrnet_amd.compute_iss_keypoints(xyz, want_flag=True, want_saliency=True, border_radius=None, normal_radius=None,
                                            border_angle=90.0, normals=None, **ISS)
    want = ir.of_cloud(x, ISS["salient_radius"], ISS["non_max_radius"], gamma_21=0.99, gamma_32=0.99, min_neighbors=5)
    assert len(plain) == len(none) == 5
    for u, v in zip(plain, none):
        assert u.dtype == v.dtype and same_bits(u.cpu().numpy(), v.cpu().numpy())
    assert np.array_equal(plain[3][0].cpu().numpy(), want["keypoint"]) and same_bits(plain[4][0].cpu().numpy(), want["saliency"])


@pytest.mark.parametrize("normals", ["given", "estimated", "given, a radius above the searched"])
def test_no_keypoint_lies_within_the_border_radius_of_the_boundary(normals):
    vcrnet_amd, border = mods()
    from vcrnet_amd import iss, native
    x, nrm, _ = recipe("capped")
    xyz = dev(x[None])
    radius = 0.35 if "above" in normals else BORDER_RADIUS
    given = None if normals == "estimated" else dev(nrm[None])
    plain = vcrnet_amd.compute_iss_keypoints(xyz, want_flag=True, want_saliency=True, **ISS)
    got = vcrnet_amd.compute_iss_keypoints(xyz, want_flag=True, want_saliency=True, border_radius=radius, normals=given, **ISS)
    rim = vcrnet_amd.compute_boundary_points(xyz, given, radius, max_nn=None, want_flag=True)[3][0].cpu().numpy() > 0
    d2 = rr.d2_all(x)
    close = (d2[:, rim] <= rr.r2_of(radius)).any(1) | rim   # a boundary point within the radius, itself included
    key, was = got[3][0].cpu().numpy() > 0, plain[3][0].cpu().numpy() > 0
    sal, sal_was = got[4][0].cpu().numpy(), plain[4][0].cpu().numpy()
    print("border rule,", normals, ": boundary points", int(rim.sum()), "close", int(close.sum()), "keypoints", int(was.sum()), "->",
          int(key.sum()), "of them close before", int((was & close).sum()))
    assert rim.sum() >= 20 and not (key & close).any()
    assert not sal[close].any() and same_bits(sal[~close], sal_was[~close])
    # away from the rim -- no neighbour of the suppression is close -- a point is what it was
    apart = ~(d2[:, close] <= rr.r2_of(ISS["non_max_radius"])).any(1) & ~close
    assert np.array_equal(key[apart], was[apart]) and apart.sum() >= 100
    selected(got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), x[None], got[3].cpu().numpy())
    if normals == "given":
        # the prefix of the rows searched already against a search of its own, composed by hand
        xyz4 = native.to_rows4(xyz)
        csr = vcrnet_amd.search_radius(xyz, radius)
        flag, _ = border.boundary_rows(xyz4, given, *csr, 3, border.radians(90.0))
        near = border.near_rows(flag, *csr)["near"]
        assert np.array_equal(near[0].cpu().numpy() > 0, close)
        big = vcrnet_amd.search_radius(xyz, ISS["salient_radius"], want_d2=True)
        s = iss.saliency_rows(xyz4, *big[:3], 0.99, 0.99, 5)["saliency"]
        s = torch.where(near > 0, torch.zeros_like(s), s)
        k = iss.nms_rows(*big[:3], s, 5, d2=big[3], r2_nm=float(rr.r2_of(ISS["non_max_radius"])))["keypoint"]
        assert torch.equal(k, got[3]) and same_bits(s.cpu().numpy(), got[4].cpu().numpy())


def test_register_features_forwards_the_border_rule():
    """keypoints="iss" with a border_radius (and the default radii: the path that runs a batch cloud by cloud): corr is
    match_features' with -1 wherever compute_iss_keypoints with the same keywords has no keypoint."""
    import match_restated as mr
    vcrnet_amd, _ = mods()
    c = mr.surface(600)
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    opts = dict(gamma_21=0.8, gamma_32=0.8, min_neighbors=4, border_radius=0.12, border_angle=100.0)
    res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=20, mutual=False, keypoints="iss", iss=opts, trials=1024, seed=mr.SEED)
    flag = vcrnet_amd.compute_iss_keypoints(src, want_flag=True, **opts)[3]
    plain = vcrnet_amd.compute_iss_keypoints(src, want_flag=True, gamma_21=0.8, gamma_32=0.8, min_neighbors=4)[3]
    every = vcrnet_amd.match_features(vcrnet_amd.compute_fpfh_feature(src, None, k=20), vcrnet_amd.compute_fpfh_feature(tgt, None, k=20),
                                      mutual=False)
    assert torch.equal(res["corr"], torch.where(flag > 0, every, torch.full_like(every, -1)))
    rim = vcrnet_amd.compute_boundary_points(src, None, 0.12, max_nn=None, angle_threshold=100.0, want_flag=True)[3]
    print("register_features: keypoints", int((plain > 0).sum()), "->", int((flag > 0).sum()), "boundary points", int((rim > 0).sum()))
    assert int((rim > 0).sum()) > 0 and not ((flag > 0) & (rim > 0)).any() and not torch.equal(flag, plain)
    assert int((flag > 0).sum()) >= 2
