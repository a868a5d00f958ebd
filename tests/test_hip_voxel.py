"""vcr_voxel_f32 on the GPU: down-sampling on a voxel grid (include/vcr_hip_voxel.h).

The result is defined bit for bit, so every comparison here is exact: the int32 views of every output against the numpy
restatement (tests/voxel_restated.py, whose two routes tests/test_voxel_cpu.py holds to each other), NaN padding and -0.0
included.  Every output buffer, and the workspace, is prefilled with a garbage byte and carries a guard band: every slot must
have been written, and nothing behind it.  Every launch form and every batch must return the same bits."""
import functools

import numpy as np
import pytest
import torch

import voxel_restated as vr

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
OUTPUTS = ("points", "count", "point_voxel", "voxel_points")


def voxel():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import voxel
    return voxel


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz [B,3,N], h, the restatement's result): computed once, shared, never written to."""
    xyz, h = vr.RECIPES[name]()
    want = vr.batch(xyz, h)
    for a in [xyz] + list(want.values()):
        a.setflags(write=False)
    return xyz, h, want


def run(xyz, h, variant=0):
    """numpy in, dict of numpy out; all of every output must have been overwritten, none of the band behind it."""
    o = voxel().voxel_grid(dev(xyz), h, variant=variant, guard=GUARD, prefill=SENTINEL_BYTE)
    torch.cuda.synchronize()
    out = {k: o[k].cpu().numpy() for k in OUTPUTS}
    for k in OUTPUTS:
        raw = o["_raw"][k]
        n = o[k].numel()
        band = raw[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * raw.element_size() and (band == SENTINEL_BYTE).all(), (k, "guard band written")
        body = raw[:n].view(torch.uint8).cpu().numpy().reshape(n, -1)
        assert not (body == SENTINEL_BYTE).all(axis=1).any(), (k, "element left unwritten")
    return out


def assert_same(got, want, what):
    for k in OUTPUTS:
        assert np.array_equal(vr.bits(got[k]), vr.bits(want[k])), (what, k)


@pytest.mark.parametrize("name", ["n1", "n5_one_voxel", "n256", "n257", "n1024", "n1025", "lattice_faces", "duplicates",
                                  "own_voxel", "one_voxel_1025", "non_finite", "all_nan"])
def test_against_the_restatement(name):
    """One point; one voxel; a block edge (256 / 257) and a tile edge (1024 / 1025); points ON cell faces; duplicated points;
    every point its own voxel (the output IS the input, a -0.0 among it); one voxel across a tile edge (the sum's order);
    NaN / inf points, at point 0 and as a voxel's would-be representative; a cloud of nothing finite.  The plan's form and a
    forced split of two."""
    xyz, h, want = case(name)
    for v in (0, voxel().variant(2)):
        assert_same(run(xyz, h, v), want, (name, v))
    if name == "own_voxel":
        assert want["count"][0] == xyz.shape[2] and np.array_equal(vr.bits(want["points"]), vr.bits(xyz))
    if name == "all_nan":
        assert want["count"][0] == 0


def test_every_form_returns_the_same_bits():
    """N = 2049 (two tiles and a point) with the scan cut into 1, 2, 3, 8 segments and the plan's own number."""
    xyz, h, want = case("n2049")
    vx = voxel()
    plan = vx.voxel_form(1, 2049, cu_count=0)[1]
    assert plan not in (1, 2, 3)
    for s in (0, 1, 2, 3, 8):
        assert_same(run(xyz, h, vx.variant(s)), want, s)


def test_a_batch_is_its_clouds_alone():
    """B = 3, three different clouds (uniform, lattice, one with non-finite points): the restatement's, and each cloud's own
    run."""
    xyz, h, want = case("three_clouds")
    got = run(xyz, h)
    assert_same(got, want, "batch")
    assert len(set(want["count"].tolist())) == 3
    for b in range(3):
        alone = run(xyz[b:b + 1], h)
        assert_same(alone, {k: got[k][b:b + 1] for k in OUTPUTS}, b)


def test_a_grid_too_fine_is_refused_for_its_cloud_alone():
    """extent / h one cell over 2^21 on x, just under on y and z: count -1 and the stated fills; its neighbours -- one of them
    just under the limit on all three axes -- are served, bit-identical to their runs alone."""
    xyz, h, want = case("fine_batch")
    assert want["count"][1] == -1 and want["count"][0] > 0 and want["count"][2] > 0
    for v in (0, voxel().variant(3)):
        got = run(xyz, h, v)
        assert_same(got, want, v)
        assert (got["point_voxel"][1] == -1).all() and (got["voxel_points"][1] == 0).all()
        assert (vr.bits(got["points"][1]) == vr.NAN_BITS).all()
    for b in (0, 2):
        assert_same(run(xyz[b:b + 1], h), {k: got[k][b:b + 1] for k in OUTPUTS}, b)


@pytest.mark.parametrize("name", ["n70001", "n131072"])
def test_large_clouds(name):
    """A uniform cube at about 8 points a voxel, against the vectorised restatement."""
    xyz, h, want = case(name)
    assert_same(run(xyz, h), want, name)


# ---------------------------------------------------------------- the Python layer

def test_voxel_down_sample_and_unpad():
    import vcrnet_amd
    from vcrnet_amd.native import VcrHipError
    vx = voxel()
    xyz, h, want = case("three_clouds")
    points, count, point_voxel = vcrnet_amd.voxel_down_sample(dev(xyz), h)
    assert points.dtype == torch.float32 and count.dtype == torch.int32 and point_voxel.dtype == torch.int32
    assert np.array_equal(vr.bits(points.cpu().numpy()), vr.bits(want["points"]))
    assert np.array_equal(count.cpu().numpy(), want["count"]) and np.array_equal(point_voxel.cpu().numpy(), want["point_voxel"])
    clouds = vx.unpad(points, count)
    assert [tuple(c.shape) for c in clouds] == [(3, int(m)) for m in want["count"]]
    for b, c in enumerate(clouds):
        assert np.array_equal(vr.bits(c.cpu().numpy()), vr.bits(want["points"][b][:, :want["count"][b]]))
    xyz, h, want = case("fine_batch")
    points, count, _ = vcrnet_amd.voxel_down_sample(dev(xyz), h)
    with pytest.raises(VcrHipError, match="cloud 1"):
        vx.unpad(points, count)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_register_sampled_on_voxelised_clouds():
    """voxel=h: elements 0-7 are the steps done by hand (voxel_down_sample, unpad, the sampling cloud by cloud, vcrnetIter on
    the stacked samples), the indices refer to the down-sampled clouds, score / refine come back cloud by cloud, the clouds
    themselves last; too few voxels raises; voxel=None is the call without the keyword."""
    import vcrnet_amd
    from vcrnet_amd import native
    from vcrnet_amd.module import vcrnetIter
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    vx = voxel()
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    npoint = 768
    h = float(np.ptp(src, axis=2).max()) / 16.0
    with torch.no_grad():
        out = vcrnet_amd.register_sampled(net, s, t, npoint, voxel=h)
        down = [vx.unpad(*vcrnet_amd.voxel_down_sample(x, h)[:2]) for x in (s, t)]
        sizes = [[c.shape[1] for c in clouds] for clouds in down]
        assert len(set(sizes[0])) == 2 and min(sizes[0] + sizes[1]) >= npoint and max(sizes[0]) < 3000    # different sizes
        picked = [[native.fps(c.unsqueeze(0).contiguous(), npoint) for c in clouds] for clouds in down]
        idx = [torch.cat([i for i, _ in p]) for p in picked]
        pts = [torch.cat([q for _, q in p]) for p in picked]
        manual = tuple(vcrnetIter(net, pts[0], pts[1], 1)) + (idx[0].long(), idx[1].long())
        assert len(out) == 9
        for a, b in zip(out[:8], manual):
            assert _eq(a, b)
        for got, want in zip(out[8], down):
            assert len(got) == 2 and all(_eq(a, b) for a, b in zip(got, want))
        for b in range(2):                                                        # the indices refer to the down-sampled clouds
            assert _eq(out[8][0][b][:, out[6][b]], pts[0][b]) and _eq(out[8][1][b][:, out[7][b]], pts[1][b])
        both = vcrnet_amd.register_sampled(net, s, t, npoint, voxel=h, score=0.1, refine=0.1)
        assert len(both) == 11 and all(_eq(a, b) for a, b in zip(both[:8], out[:8]))
        assert isinstance(both[8], list) and isinstance(both[9], list) and len(both[8]) == len(both[9]) == 2
        for b in range(2):
            sb, tb = down[0][b].unsqueeze(0), down[1][b].unsqueeze(0)
            direct = vcrnet_amd.score_registration(sb, tb, out[2][b:b + 1], out[3][b:b + 1], max_dist=0.1)
            assert sorted(both[8][b]) == sorted(direct) and all(_eq(both[8][b][k], direct[k]) for k in direct)
            direct = vcrnet_amd.refine_registration(sb, tb, out[2][b:b + 1], out[3][b:b + 1], max_dist=0.1)
            assert sorted(both[9][b]) == sorted(direct)
            assert all(_eq(both[9][b][k], direct[k]) for k in direct if torch.is_tensor(direct[k]))
        assert all(_eq(a, b) for a, b in zip(both[10][0] + both[10][1], down[0] + down[1]))
        with pytest.raises(native.VcrHipError, match=r"src cloud 0 has \d+ voxels.*fewer than npoint = 768"):
            vcrnet_amd.register_sampled(net, s, t, npoint, voxel=h * 8.0)
        plain = vcrnet_amd.register_sampled(net, s, t, 1024)
        none = vcrnet_amd.register_sampled(net, s, t, 1024, voxel=None)
        assert len(plain) == len(none) == 8 and all(_eq(a, b) for a, b in zip(plain, none))
