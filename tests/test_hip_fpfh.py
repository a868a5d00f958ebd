"""vcr_spfh_f32 and vcr_fpfh_f32 on the GPU (include/vcr_hip_fpfh.h) against the numpy restatement
(tests/fpfh_restated.py), on the device's own neighbours and the device's own normals.

The first pass is held to the restatement byte for byte, except where the last bit of an arc tangent could decide a bin: a pair
whose f0 coordinate lies within 2^-30 of an integer is excluded (at most 0.1 % of a case; tests/test_fpfh_cpu.py holds the
recipes to that on the CPU), and a point with e excluded pairs may differ by at most e per count, in the f0 group only.  The
second pass has a defined order and no such step: fed the device's SPFH bytes, the restatement's fp32 result is the device's,
bit for bit.  Every call runs with guard bands behind prefilled outputs: all of the output written, none of the band."""
import functools

import numpy as np
import pytest
import torch

import fpfh_restated as fr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A                                        # no count (<= 62) and no byte of a feature's fp32 pattern below
GUARD = 64


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import fpfh, native, plane
    return native, plane, fpfh


def dev(x):
    return None if x is None else torch.tensor(np.array(x)).cuda()                  # (a copy: the cached cases are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def checked(out, raw, name, guard, byte):
    """The output's buffer: nothing behind it written, nothing of it left as prefilled."""
    n = out.numel()
    width = out.element_size()
    band = raw[name][n:].view(torch.uint8).cpu().numpy()
    assert band.size == guard * width and (band == byte).all(), (name, "guard band written")
    body = raw[name][:n].view(torch.uint8).cpu().numpy()
    if width == 1:
        assert not (body == byte).any(), (name, "byte left unwritten")
    else:
        assert not (body.reshape(n, width) == byte).all(axis=1).any(), (name, "element left unwritten")


def run_spfh(xyz4, nrm, idx, radius=0.0, guard=GUARD, byte=SENTINEL_BYTE):
    """-> uint8 [B,N,48] numpy."""
    _, _, fpfh = mods()
    sp, raw = fpfh.spfh(xyz4, nrm, idx, radius, guard=guard, prefill=byte)
    torch.cuda.synchronize()
    checked(sp, raw, "spfh", guard, byte)
    return sp


def run_fpfh(xyz4, idx, sp, radius=0.0, guard=GUARD, byte=SENTINEL_BYTE):
    """-> float32 [B,33,N] device tensor."""
    _, _, fpfh = mods()
    feat, raw = fpfh.fpfh(xyz4, idx, sp, radius, guard=guard, prefill=byte)
    torch.cuda.synchronize()
    checked(feat, raw, "fpfh", guard, byte)
    return feat


def inputs(x, k):
    """x [B,3,N] numpy -> (xyz4, idx int32 [B,N,k], normals [B,3,N]), all the device's own."""
    native, plane, _ = mods()
    xyz4 = native.to_rows4(dev(x))
    idx = native.knn(xyz4, None, k)
    nrm, _ = plane.normals(xyz4, idx, want_curvature=False)
    return xyz4, idx, nrm


@functools.lru_cache(maxsize=None)
def case(B, N, k):
    """One shape's device run and its inputs on the host, computed once: (x, idx, nrm, spfh, fpfh) numpy."""
    x = fr.cloud(B, N)
    xyz4, idx, nrm = inputs(x, k)
    sp = run_spfh(xyz4, nrm, idx)
    feat = run_fpfh(xyz4, idx, sp)
    out = tuple(t.cpu().numpy() for t in (idx, nrm, sp, feat))
    for a in out:
        a.setflags(write=False)
    return (x,) + out


def held_to_the_restatement(sp, p, label):
    """The device's bytes sp [N,48] against the pairs p of the restatement; returns (excluded, counted)."""
    ref = fr.pack(p).reshape(-1, 3, 16).astype(np.int64)
    got = np.asarray(sp).reshape(-1, 3, 16).astype(np.int64)
    ex = fr.excluded(p).sum(1)
    clean = ex == 0
    assert np.array_equal(got[clean], ref[clean]), (label, "a point without an excluded pair differs")
    assert np.array_equal(got[:, 1:], ref[:, 1:]), (label, "the f1 / f2 groups and their c differ")
    assert np.array_equal(got[:, 0, fr.BINS:], ref[:, 0, fr.BINS:]), label
    assert (np.abs(got[:, 0, :fr.BINS] - ref[:, 0, :fr.BINS]).max(1) <= ex).all(), label
    assert (got[:, 0, :fr.BINS].sum(1) == ref[:, 0, :fr.BINS].sum(1)).all(), label
    return int(ex.sum()), int(p["counted"].sum())


@pytest.mark.parametrize("B,N,k", fr.SHAPES)
def test_spfh_against_the_restatement(B, N, k):
    x, idx, nrm, sp, _ = case(B, N, k)
    assert idx.min() >= 0 and idx.max() < N and not (idx == np.arange(N)[None, :, None]).any()
    e = n = 0
    for b in range(B):
        p = fr.pairs(x[b], nrm[b], idx[b])
        eb, nb = held_to_the_restatement(sp[b], p, (B, N, k, b))
        e, n = e + eb, n + nb
        counts, c = fr.group_bins(sp[b])
        assert (c == k).all() and (counts.reshape(N, 3, 11).sum(2) == k).all()
    print(f"spfh B {B} N {N} k {k}: {e} of {n} pairs excluded ({e / n:.2e})")
    assert n == B * N * k and e <= 0.001 * n


@pytest.mark.parametrize("B,N,k", fr.SHAPES)
def test_fpfh_is_the_restatement_bit_for_bit(B, N, k):
    x, idx, _, sp, feat = case(B, N, k)
    for b in range(B):
        want = fr.fpfh(x[b], idx[b], sp[b])
        assert np.array_equal(bits(feat[b]), bits(want)), (B, N, k, b, np.abs(feat[b] - want).max())
        assert np.abs(feat[b].astype(np.float64).reshape(3, 11, N).sum(1) - 200).max() <= 11 * 2.0 ** -24 * 200


def test_an_exact_plane():
    """z = 0.25 and normals (0, 0, 1): every pair has f = (0, 0, 0) exactly, so every histogram has one bin a group and every
    feature is 0 or 200."""
    native, _, _ = mods()
    x, nrm = fr.plane_cloud()
    xyz4 = native.to_rows4(dev(x[None]))
    idx = native.knn(xyz4, None, 10)
    sp = run_spfh(xyz4, dev(nrm[None]), idx)
    counts, c = fr.group_bins(sp.cpu().numpy()[0])
    want = np.zeros(33, np.int64)
    want[[5, 16, 27]] = 10
    assert (counts == want).all() and (c == 10).all()
    feat = run_fpfh(xyz4, idx, sp).cpu().numpy()[0]
    assert np.array_equal(feat, np.tile(np.where(want > 0, np.float32(200), np.float32(0))[:, None], (1, 200)))


def test_a_cloud_of_copies():
    """Every d2 is 0: every pair is counted with f = (0, 0, 0), and the second pass skips every neighbour -- the feature is the
    point's own term alone."""
    native, _, _ = mods()
    B, N, k = 2, 64, 8
    x = np.tile(np.asarray([0.3, -0.7, 1.1], np.float32)[None, :, None], (B, 1, N))
    nrm = np.tile(np.asarray([0.6, 0.0, 0.8], np.float32)[None, :, None], (B, 1, N))
    idx = np.tile(np.arange(k, dtype=np.int32), (B, N, 1))                       # (any rows: they are all equal)
    xyz4 = native.to_rows4(dev(x))
    sp = run_spfh(xyz4, dev(nrm), dev(idx))
    counts, c = fr.group_bins(sp.cpu().numpy())
    want = np.zeros(33, np.int64)
    want[[5, 16, 27]] = k
    assert (counts == want).all() and (c == k).all()
    feat = run_fpfh(xyz4, dev(idx), sp).cpu().numpy()
    own = np.float32(np.float64(k) * (100.0 / np.float64(k)))
    assert np.array_equal(feat, np.tile(np.where(want > 0, own, np.float32(0))[None, :, None], (B, 1, N)))


def test_a_nan_point_an_inf_point_and_a_nan_normal():
    B, N, k = 2, 1000, 8
    x = fr.cloud(B, N)
    xyz4, idx, nrm = inputs(x, k)
    clean_sp = run_spfh(xyz4, nrm, idx)
    clean = run_fpfh(xyz4, idx, clean_sp).cpu().numpy()
    clean_sp = clean_sp.cpu().numpy()
    bad_x, bad_n = x.copy(), nrm.cpu().numpy().copy()
    bad_x[0, 1, 17] = np.nan
    bad_x[0, 2, 123] = np.inf
    bad_n[0, 0, 200] = np.nan
    rows = [17, 123, 200]
    native, _, _ = mods()
    bad4 = native.to_rows4(dev(bad_x))
    sp_t = run_spfh(bad4, dev(bad_n), idx)                                        # (the clean cloud's neighbours)
    feat = run_fpfh(bad4, idx, sp_t).cpu().numpy()
    sp = sp_t.cpu().numpy()
    idx = idx.cpu().numpy()
    among = np.isin(idx[0], rows)
    counts, c = fr.group_bins(sp)
    want_c = k - among.sum(1)
    want_c[rows] = 0
    assert np.array_equal(c[0], want_c) and (c[0][among.any(1)] < k).all()       # the affected pairs are not counted
    assert counts.max() <= k and (counts.reshape(B, N, 3, 11).sum(3) == c[:, :, None]).all()
    hit = among.any(1)
    hit[rows] = True
    assert 3 < hit.sum() < 100
    assert np.array_equal(sp[0][~hit], clean_sp[0][~hit])
    # the second pass reads a point's neighbours' histograms: a point is untouched if neither it nor a neighbour was hit
    far = hit | hit[idx[0]].any(1)
    assert hit.sum() < far.sum() < N // 2
    assert np.array_equal(bits(feat[0][:, ~far]), bits(clean[0][:, ~far]))
    assert np.isfinite(feat).all() and not feat[0][:, [17, 123]].any() and feat[0][:, 200].any()
    assert np.array_equal(sp[1], clean_sp[1]) and np.array_equal(bits(feat[1]), bits(clean[1]))   # the other cloud
    held_to_the_restatement(sp[0], fr.pairs(bad_x[0], bad_n[0], idx[0]), "non-finite")
    assert np.array_equal(bits(feat[0]), bits(fr.fpfh(bad_x[0], idx[0], sp[0])))


def test_idx_entries_outside_the_cloud_read_as_the_row_itself():
    """... with 4096 elements of guard behind outputs prefilled with NaN bytes: nothing outside them is written."""
    B, N, k = 2, 257, 20
    x, idx, nrm, _, _ = case(B, N, k)
    native, _, _ = mods()
    xyz4, nrm = native.to_rows4(dev(x)), dev(nrm)
    rs = np.random.RandomState(10)
    own = np.broadcast_to(np.arange(N)[None, :, None], idx.shape)
    where = rs.uniform(size=idx.shape) < 0.1
    out = np.where(where, rs.choice([-1, N, 2 ** 30], size=idx.shape), idx).astype(np.int32)
    same = np.where(where, own, idx).astype(np.int32)
    got_sp = run_spfh(xyz4, nrm, dev(out), guard=4096, byte=0xFF)
    want_sp = run_spfh(xyz4, nrm, dev(same), guard=4096, byte=0xFF)
    assert torch.equal(got_sp, want_sp)
    got = run_fpfh(xyz4, dev(out), got_sp, guard=4096, byte=0xFF)
    want = run_fpfh(xyz4, dev(same), want_sp, guard=4096, byte=0xFF)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    for b in range(B):                                      # the row itself: counted in bins 5 / 16 / 27, skipped by the sum
        p = fr.pairs(x[b], nrm[b].cpu().numpy(), out[b])
        assert (p["bins"][where[b]] == 5).all() and p["counted"].all()
        held_to_the_restatement(got_sp[b].cpu().numpy(), p, ("outside", b))
        assert np.array_equal(bits(got[b].cpu().numpy()), bits(fr.fpfh(x[b], out[b], got_sp[b].cpu().numpy())))
    assert not torch.equal(got_sp, dev(case(B, N, k)[3]))                         # (the entries mattered)


def test_a_radius_drops_the_same_pairs_in_both_passes():
    B, N, k = fr.SHAPES[1]
    x, idx, nrm, sp0, feat0 = case(B, N, k)
    native, _, _ = mods()
    xyz4, idx_d, nrm_d = native.to_rows4(dev(x)), dev(idx), dev(nrm)
    # above every neighbour distance: radius = 0's bits
    sp = run_spfh(xyz4, nrm_d, idx_d, 10.0)
    assert np.array_equal(sp.cpu().numpy(), sp0)
    assert np.array_equal(bits(run_fpfh(xyz4, idx_d, sp, 10.0).cpu().numpy()), bits(feat0))
    # between the fifth and the sixth neighbour distance
    d2 = np.stack([fr.geometry(x[b], idx[b])[2] for b in range(B)])
    radius = fr.radius_between(np.sqrt(d2[0]), 5)
    inside = d2 <= fr.r2_of(radius)
    assert 0 < inside.sum() < inside.size
    sp = run_spfh(xyz4, nrm_d, idx_d, float(radius))
    feat = run_fpfh(xyz4, idx_d, sp, float(radius))
    masked = dev(np.where(inside, idx, -1).astype(np.int32))                      # the dropped entries read as the row: skipped
    assert torch.equal(run_fpfh(xyz4, masked, sp, float(radius)).view(torch.int32), feat.view(torch.int32))
    assert not torch.equal(run_fpfh(xyz4, idx_d, sp, 0.0).view(torch.int32), feat.view(torch.int32))
    sp, feat = sp.cpu().numpy(), feat.cpu().numpy()
    for b in range(B):
        p = fr.pairs(x[b], nrm[b], idx[b], radius)
        assert np.array_equal(p["counted"], inside[b])
        assert np.array_equal(fr.group_bins(sp[b])[1], inside[b].sum(1))          # the restatement's c_i
        held_to_the_restatement(sp[b], p, ("radius", b))
        assert np.array_equal(bits(feat[b]), bits(fr.fpfh(x[b], idx[b], sp[b], radius)))


def test_a_cloud_does_not_depend_on_its_batch():
    B, N, k = fr.SHAPES[2]
    x, idx, nrm, sp, feat = case(B, N, k)
    native, _, _ = mods()
    for b in range(B):
        xyz4 = native.to_rows4(dev(x[b:b + 1]))
        alone_sp = run_spfh(xyz4, dev(nrm[b:b + 1]), dev(idx[b:b + 1]))
        alone = run_fpfh(xyz4, dev(idx[b:b + 1]), alone_sp)
        assert np.array_equal(alone_sp.cpu().numpy()[0], sp[b])
        assert np.array_equal(bits(alone.cpu().numpy()[0]), bits(feat[b]))


def test_compute_fpfh_feature_is_the_composition_of_its_calls(monkeypatch):
    import vcrnet_amd
    native, plane, fpfh = mods()
    x = dev(fr.cloud(2, 1000))
    feat, nrm, idx = vcrnet_amd.compute_fpfh_feature(x, k=20, want_normals=True, want_idx=True)
    xyz4 = native.to_rows4(x)
    idx2 = native.knn(xyz4, None, 20)
    nrm2, _ = plane.normals(xyz4, idx2, want_curvature=False)
    feat2 = fpfh.fpfh(xyz4, idx2, fpfh.spfh(xyz4, nrm2, idx2))
    assert idx.dtype == torch.int32 and idx.shape == (2, 1000, 20) and torch.equal(idx, idx2)
    assert nrm.shape == (2, 3, 1000) and torch.equal(nrm.view(torch.int32), nrm2.view(torch.int32))
    assert feat.dtype == torch.float32 and feat.shape == (2, 33, 1000) and torch.equal(feat.view(torch.int32), feat2.view(torch.int32))
    only = vcrnet_amd.compute_fpfh_feature(x, k=20)
    assert torch.is_tensor(only) and torch.equal(only.view(torch.int32), feat.view(torch.int32))
    assert len(vcrnet_amd.compute_fpfh_feature(x, k=20, want_idx=True)) == 2
    # a radius goes to both passes
    r = 0.05
    assert torch.equal(vcrnet_amd.compute_fpfh_feature(x, k=20, radius=r).view(torch.int32),
                       fpfh.fpfh(xyz4, idx2, fpfh.spfh(xyz4, nrm2, idx2, r), r).view(torch.int32))
    # given normals: no normals launch, the composition on those normals
    given = torch.roll(nrm2, 1, dims=1).contiguous()

    def no_launch(*a, **kw):
        raise AssertionError("a normals launch with normals given")
    monkeypatch.setattr(plane, "normals", no_launch)
    monkeypatch.setattr(plane, "estimate_normals", no_launch)
    got, used = vcrnet_amd.compute_fpfh_feature(x, normals=given, k=20, want_normals=True)
    assert torch.equal(used.view(torch.int32), given.view(torch.int32))
    assert torch.equal(got.view(torch.int32), fpfh.fpfh(xyz4, idx2, fpfh.spfh(xyz4, given, idx2)).view(torch.int32))
    assert not torch.equal(got.view(torch.int32), feat.view(torch.int32))


def test_python_entry_points_refuse_before_any_launch():
    import vcrnet_amd
    native, _, fpfh = mods()
    x = dev(fr.cloud(1, 64))
    with pytest.raises(native.VcrHipError, match=r"k \+ 1 = 31"):
        vcrnet_amd.compute_fpfh_feature(x[:, :, :30])
    with pytest.raises(native.VcrHipError, match=r"k must be in \[1, 62\]"):
        vcrnet_amd.compute_fpfh_feature(dev(fr.cloud(1, 257)), k=63)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.compute_fpfh_feature(x, normals=x.cpu())
    with pytest.raises(native.VcrHipError, match="radius must be positive and finite"):
        vcrnet_amd.compute_fpfh_feature(x, radius=0.0)
    xyz4 = native.to_rows4(x)
    idx63 = torch.zeros(1, 64, 63, dtype=torch.int32, device="cuda")
    with pytest.raises(native.VcrHipError, match="vcr_spfh_f32"):
        fpfh.spfh(xyz4, x, idx63)
    with pytest.raises(native.VcrHipError, match="vcr_fpfh_f32"):
        fpfh.fpfh(xyz4, idx63, torch.zeros(1, 64, 48, dtype=torch.uint8, device="cuda"))
    with pytest.raises(native.VcrHipError, match="vcr_spfh_f32"):
        fpfh.spfh(xyz4, x, idx63[:, :, :8], radius=-1.0)
