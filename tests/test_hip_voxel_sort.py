"""vcr_voxel_sort_f32 on the GPU: the voxel grid by a stable radix sort, with member lists (include/vcr_hip_voxel_sort.h,
DESIGN.md section 4.21).

The result is vcr_voxel_f32's, defined bit for bit, so every comparison is exact: the int32 views of every output against the
numpy restatement of the definition (tests/voxel_restated.py) with the member lists by their definition
(tests/voxel_sort_restated.py), NaN padding and -0.0 included.  Every output buffer, and the workspace, is prefilled with a
garbage byte and carries a guard band: every slot must have been written, and nothing behind it.  Every digit width, the scan
form and every batch must return the same bits."""
import functools

import numpy as np
import pytest
import torch

import voxel_restated as vr
import voxel_sort_restated as vs

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64
OUTPUTS = vs.OUTPUTS
WIDTHS = (4, 8, 11)
TILE = {4: 1024, 8: 1024, 11: 2048}                        # the elements of one workgroup of the sort


def mod():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import voxel_sort
    return voxel_sort


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()              # (a copy: the shared cases are read-only)


def expect(xyz, h):
    want = vs.with_member_lists(vr.batch(xyz, h))
    for a in want.values():
        a.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz [B,3,N], h, the definition's result): computed once, shared, never written to."""
    xyz, h = vr.RECIPES[name]()
    xyz.setflags(write=False)
    return xyz, h, expect(xyz, h)


def run(xyz, h, bits=0):
    """numpy in, dict of numpy out; all of every output must have been overwritten, none of the band behind it."""
    o = mod().voxel_grid_sort(dev(xyz), h, digit_bits=bits, want_members=True, guard=GUARD, prefill=SENTINEL_BYTE)
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


def assert_same(got, want, what, outputs=OUTPUTS):
    for k in outputs:
        assert np.array_equal(vr.bits(got[k]), vr.bits(want[k])), (what, k)


def assert_members_ascend(got):
    for b in range(len(got["count"])):
        M, mem, start = int(got["count"][b]), got["members"][b], got["voxel_start"][b]
        for v in range(max(M, 0)):
            seg = mem[start[v]:start[v] + got["voxel_points"][b][v]]
            assert len(seg) >= 1 and (np.diff(seg) > 0).all() and (got["point_voxel"][b][seg] == v).all(), (b, v)


@pytest.mark.parametrize("name", ["n1", "n5_one_voxel", "n256", "n257", "n1024", "n1025", "n2049", "three_clouds", "lattice_faces",
                                  "duplicates", "own_voxel", "one_voxel_1025", "non_finite", "all_nan", "fine_batch", "n70001",
                                  "n131072"])
def test_against_the_restatement(name):
    """Every recipe tests/test_hip_voxel.py runs, the large clouds included: the four outputs against the definition, the member
    lists against theirs."""
    xyz, h, want = case(name)
    assert_same(run(xyz, h), want, name)
    if name == "own_voxel":
        assert want["count"][0] == xyz.shape[2] and np.array_equal(vr.bits(want["points"]), vr.bits(xyz))
        assert np.array_equal(want["members"][0], np.arange(xyz.shape[2]))
    if name == "all_nan":
        assert want["count"][0] == 0 and (want["members"] == -1).all() and (want["voxel_start"] == 0).all()
    if name == "fine_batch":
        assert want["count"][1] == -1 and (want["members"][1] == -1).all() and (want["voxel_start"][1] == 0).all()


@pytest.mark.parametrize("name", ["three_clouds", "non_finite", "n2049"])
def test_the_scan_form_returns_the_same_bits(name):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import voxel
    xyz, h, _ = case(name)
    scan = voxel.voxel_grid(dev(xyz), h)
    sort = mod().voxel_grid_sort(dev(xyz), h)
    for k in ("points", "count", "point_voxel", "voxel_points"):
        assert torch.equal(scan[k].view(torch.int32), sort[k].view(torch.int32)), (name, k)


@pytest.mark.parametrize("bits", WIDTHS)
def test_every_digit_width_returns_the_same_bits(bits):
    """Two blocks of the widest form and one element; and fine_batch, whose clouds need one to three passes, none (too fine) and
    every pass: the buffer a cloud's order ends in differs from cloud to cloud."""
    m = mod()
    assert m.voxel_sort_form(1, 1000, digit_bits=bits)[0] == bits and tuple(m.DIGIT_BITS) == WIDTHS
    N = 2 * max(TILE.values()) + 1
    xyz = vr.uniform(21, 1, N)
    h = vr.edge_for(N)
    assert_same(run(xyz, h, bits), expect(xyz, h), (bits, N))
    xyz, h, want = case("fine_batch")
    passes = [None if w is None else vs.passes_needed(sum(w), bits) for w in (vs.widths(c, h)[2] for c in xyz)]
    assert passes == [{4: 3, 8: 2, 11: 1}[bits], None, -(-64 // bits)]       # (cloud 0: W = 9; an odd number at 4 and 11)
    assert_same(run(xyz, h, bits), want, (bits, "fine_batch"))


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097])
def test_block_and_tile_edges(N):
    """One point; two points in one voxel; one element below, at and above one block and two blocks of the sort, at 8 bits (blocks
    of 1 024) and at 11, the plan's (of 2 048) -- a cloud of a few hundred voxels and the same points in one voxel."""
    assert TILE[mod().voxel_sort_form(1, N)[0]] == 2048 and TILE[8] == 1024
    xyz = vr.uniform(30 + N, 1, N)
    for h in (vr.edge_for(max(N, 8)), 10.0):
        want = expect(xyz, h)
        assert h != 10.0 or want["count"][0] == 1
        for bits in (0, 8):
            assert_same(run(xyz, h, bits), want, (N, h, bits))


@pytest.mark.parametrize("N,seed", [(1000, 4), (3000, 5), (5000, 12)])
def test_sums_whose_order_shows(N, seed):
    """One block, three blocks of 1 024 and three blocks of 2 048 of the sort.  One voxel of edge 2^63 whose members cancel: its mean depends on the order of
    the additions (tests/test_voxel_sort_cpu.py shows a shuffled window changes it), and the same cloud as two voxels
    interleaved across every block.  Every width; the members of every voxel ascend."""
    for xyz, voxels in ((vs.cancelling(seed, N), 1), (vs.interleaved(seed, N), 2)):
        want = expect(xyz, vs.CANCEL_H)
        assert want["count"][0] == voxels
        for bits in (0,) + WIDTHS:
            got = run(xyz, vs.CANCEL_H, bits)
            assert_same(got, want, (N, voxels, bits))
            assert_members_ascend(got)


def test_non_finite_points_at_the_ends():
    """A cloud whose only finite point is its last; NaN at point 0 alone; (non_finite and all_nan run with the recipes)."""
    xyz = np.full((1, 3, 1500), np.nan, np.float32)
    xyz[0, :, -1] = (1.0, -2.0, 3.0)
    want = expect(xyz, 0.5)
    assert want["count"][0] == 1 and want["point_voxel"][0, -1] == 0 and want["members"][0, 0] == 1499
    assert_same(run(xyz, 0.5), want, "last")
    xyz = np.array(vr.uniform(40, 1, 1500))
    xyz[0, 1, 0] = np.nan
    want = expect(xyz, vr.edge_for(1500))
    assert want["point_voxel"][0, 0] == -1 and want["point_voxel"][0, 1] == 0
    got = run(xyz, vr.edge_for(1500))
    assert_same(got, want, "first")
    assert_members_ascend(got)


def test_a_batch_is_its_clouds_alone():
    xyz, h, want = case("three_clouds")
    got = run(xyz, h)
    assert_same(got, want, "batch")
    for b in range(3):
        assert_same(run(xyz[b:b + 1], h), {k: got[k][b:b + 1] for k in OUTPUTS}, b)
    assert_members_ascend(got)


# ---------------------------------------------------------------- the Python layer

def test_voxel_down_sample_method_sort_and_the_trace():
    import vcrnet_amd
    from vcrnet_amd import voxel
    from vcrnet_amd.native import VcrHipError
    xyz, h, want = case("three_clouds")
    points, count, point_voxel = vcrnet_amd.voxel_down_sample(dev(xyz), h, method="sort")
    assert points.dtype == torch.float32 and count.dtype == torch.int32 and point_voxel.dtype == torch.int32
    assert np.array_equal(vr.bits(points.cpu().numpy()), vr.bits(want["points"]))
    assert np.array_equal(count.cpu().numpy(), want["count"]) and np.array_equal(point_voxel.cpu().numpy(), want["point_voxel"])
    out = mod().voxel_down_sample_and_trace(dev(xyz), h)
    assert len(out) == 5 and all(o.dtype == torch.int32 for o in out[1:])
    for got, k in zip(out, ("points", "count", "point_voxel", "members", "voxel_start")):
        assert np.array_equal(vr.bits(got.cpu().numpy()), vr.bits(want[k])), k
    clouds = voxel.unpad(out[0], out[1])
    assert [tuple(c.shape) for c in clouds] == [(3, int(m)) for m in want["count"]]
    xyz, h, want = case("fine_batch")
    points, count, _ = vcrnet_amd.voxel_down_sample(dev(xyz), h, method="sort")
    with pytest.raises(VcrHipError, match="cloud 1"):
        voxel.unpad(points, count)
    with pytest.raises(VcrHipError, match='method must be "scan" or "sort"'):
        vcrnet_amd.voxel_down_sample(dev(xyz), h, method="grid")


def test_register_sampled_takes_the_method():
    """voxel_method="sort" returns what "scan" returns, bit for bit, down to the down-sampled clouds."""
    import vcrnet_amd
    from test_hip_forward import build_net
    from test_hip_fps import _pair
    from test_hip_voxel import _eq
    net, _ = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = dev(src), dev(tgt)
    h = float(np.ptp(src, axis=2).max()) / 16.0
    with torch.no_grad():
        scan = vcrnet_amd.register_sampled(net, s, t, 768, voxel=h, voxel_method="scan")
        sort = vcrnet_amd.register_sampled(net, s, t, 768, voxel=h, voxel_method="sort")
    assert len(scan) == len(sort) == 9 and all(_eq(a, b) for a, b in zip(scan[:8], sort[:8]))
    for a, b in zip(scan[8], sort[8]):
        assert len(a) == len(b) == 2 and all(_eq(p, q) for p, q in zip(a, b))
