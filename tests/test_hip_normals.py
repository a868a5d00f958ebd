"""vcr_normals_f32 on the GPU: a normal per point from given neighbours (include/vcr_hip_plane.h).

The neighbours are native.knn's on the same rows; the covariance, its eigenvalues and the reference normal are the restatement's
(tests/plane_restated.py: the header's sums, numpy.linalg.eigh) on the SAME idx.  For every point:
  * | |n| - 1 | <= 2^-22;
  * n^T C n / n^T n - lambda0 <= 2^-40 lambda2, degenerate points included.  (The Rayleigh quotient: for a unit n it is
    n^T C n, and it is what the fp32 rounding of n moves by about 2^-44 lambda2 only -- second order.  Without the division the
    rounding of n enters in first order, 2^-24 lambda0, and numpy.linalg.eigh's own vector misses the bound once rounded.)
  * where lambda1 - lambda0 >= 2^-10 lambda2: max |n - n_ref| <= 2^-22, the sign rule applied to both; at most 1 % of a case is
    left out (tests/test_plane_cpu.py checks the recipe for that on the CPU);
  * |c - c_ref| <= 2^-22 c_ref + 2^-40 for the curvature.
Every call runs with guard bands behind prefilled outputs: all of the output written, none of the band."""
import numpy as np
import pytest
import torch

import plane_restated as pr
from test_plane_cpu import NORMALS_SHAPES

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x5A
GUARD = 64


def mods():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native, plane
    return native, plane


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def neighbours(x, k):
    """x [B,3,N] numpy -> (xyz4 device, idx device int32 [B,N,k]) by the library's kNN."""
    native, _ = mods()
    xyz4 = native.to_rows4(dev(x))
    return xyz4, native.knn(xyz4, None, k)


def run(x, idx, viewpoint=None):
    """x [B,3,N] numpy, idx device or numpy [B,N,k] -> (normals [B,3,N], curvature [B,N]) numpy."""
    native, plane = mods()
    xyz4 = native.to_rows4(dev(x))
    if not torch.is_tensor(idx):
        idx = dev(np.asarray(idx, np.int32))
    nrm, cur, raw = plane.normals(xyz4, idx, dev(viewpoint), guard=GUARD, prefill=SENTINEL_BYTE)
    torch.cuda.synchronize()
    for name, o in (("normals", nrm), ("curvature", cur)):
        n = o.numel()
        band = raw[name][n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * 4 and (band == SENTINEL_BYTE).all(), (name, "guard band written")
        body = raw[name][:n].view(torch.uint8).cpu().numpy().reshape(n, 4)
        assert not (body == SENTINEL_BYTE).all(axis=1).any(), (name, "element left unwritten")
    only, _ = plane.normals(xyz4, idx, dev(viewpoint), want_curvature=False)       # the curvature is optional
    assert torch.equal(only.view(torch.int32), nrm.view(torch.int32))
    return nrm.cpu().numpy(), cur.cpu().numpy()


def cloud(B, N):
    return np.stack([pr.jittered_torus(100 * N + b, N) for b in range(B)])


@pytest.mark.parametrize("B,N,k", NORMALS_SHAPES)
def test_normals_against_the_restatement(B, N, k):
    x = cloud(B, N)
    _, idx = neighbours(x, k)
    n, c = run(x, idx)
    idx = idx.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < N
    for b in range(B):
        C = pr.covariances(x[b], idx[b])
        lam, V = np.linalg.eigh(C)
        nd = n[b].astype(np.float64).T                                            # [N,3]
        norm = np.abs(np.sqrt((nd * nd).sum(1)) - 1).max()
        rq = np.einsum("ni,nij,nj->n", nd, C, nd) / (nd * nd).sum(1) - lam[:, 0]
        apart = lam[:, 1] - lam[:, 0] >= 2.0 ** -10 * lam[:, 2]
        ref = np.stack([pr.orient(V[i, :, 0].astype(np.float32)) for i in range(N)])
        dn = np.abs(n[b].T - ref)[apart].max()
        c_ref = lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        dc = np.abs(c[b].astype(np.float64) - c_ref) - 2.0 ** -22 * c_ref
        print(f"normals B {B} N {N} k {k} cloud {b}: ||n|-1| {norm:.2e}  (n^T C n / n^T n - l0) / l2 {(rq / lam[:, 2]).max():.2e}  "
              f"|n - n_ref| {dn:.2e} over {apart.mean():.3f} of the points  |c - c_ref| - 2^-22 c_ref {dc.max():.2e}")
        assert norm <= 2.0 ** -22
        assert (rq <= 2.0 ** -40 * lam[:, 2]).all(), (rq / lam[:, 2]).max()
        assert 1 - apart.mean() <= 0.01
        assert dn <= 2.0 ** -22
        assert (dc <= 2.0 ** -40).all()
        big = np.abs(n[b]).argmax(0)                                              # the sign rule, on the output itself
        assert (n[b][big, np.arange(N)] > 0).all()


def test_an_exact_plane():
    """z = 0.25 x + 0.5 y on a jittered grid whose x and y are multiples of 2^-12: every coordinate, and every difference, is
    exact in fp32, so C has rank two up to the fp64 additions."""
    rs = np.random.RandomState(7)
    g = (np.stack(np.meshgrid(np.arange(20), np.arange(20)), 0).reshape(2, -1) + 0.5) / 20 + rs.uniform(-0.02, 0.02, (2, 400))
    xy = np.round(g * 4096) / 4096
    x = np.stack([xy[0], xy[1], 0.25 * xy[0] + 0.5 * xy[1]]).astype(np.float32)[None]
    assert np.array_equal(x[0, 2].astype(np.float64), 0.25 * xy[0] + 0.5 * xy[1])
    _, idx = neighbours(x, 12)
    n, c = run(x, idx)
    want = np.asarray([-0.25, -0.5, 1.0]) / np.linalg.norm([-0.25, -0.5, 1.0])
    assert np.abs(n[0].T.astype(np.float64) - want).max() <= 2.0 ** -20
    assert np.abs(c).max() <= 2.0 ** -30


def test_collinear_rows_and_a_cloud_of_copies():
    rs = np.random.RandomState(8)
    step = np.asarray([1.0, 2.0, -2.0]) / 1024                                    # (exact in fp32, with every multiple below)
    m = rs.permutation(200)[:40]
    x = (np.asarray([0.25, 0.5, 0.75])[:, None] + step[:, None] * m[None, :]).astype(np.float32)[None]
    _, idx = neighbours(x, 8)
    n, c = run(x, idx)
    nd = n[0].astype(np.float64)
    assert np.abs(np.sqrt((nd * nd).sum(0)) - 1).max() <= 2.0 ** -22
    assert np.abs(nd.T @ (step / np.linalg.norm(step))).max() <= 2.0 ** -20
    assert np.isfinite(c).all() and np.abs(c).max() <= 2.0 ** -30
    same = np.tile(np.asarray([0.3, -0.7, 1.1], np.float32)[None, :, None], (2, 1, 64))
    idx = np.tile(np.arange(8, dtype=np.int32), (2, 64, 1))                       # (any rows: they are all equal)
    n, c = run(same, idx)
    assert np.array_equal(n, np.tile(np.asarray([0, 0, 1], np.float32)[None, :, None], (2, 1, 64))) and not c.any()


def test_a_viewpoint_inside_and_outside_a_sphere():
    rs = np.random.RandomState(9)
    p = rs.normal(size=(3, 500))
    centre = np.asarray([0.2, -0.1, 0.3])
    x = (centre[:, None] + p / np.linalg.norm(p, axis=0)).astype(np.float32)[None]
    _, idx = neighbours(x, 10)
    free, _ = run(x, idx)
    for view in (centre, centre + [10.0, 0, 0], centre + [0, 0, -3.0]):
        v32 = np.asarray(view, np.float32)[None]
        n, _ = run(x, idx, viewpoint=v32)
        w = v32[0].astype(np.float64)[:, None] - x[0].astype(np.float64)
        nd = n[0].astype(np.float64)
        dot = (nd[0] * w[0] + nd[1] * w[1]) + nd[2] * w[2]
        assert (dot >= 0).all() and (dot > 0).mean() > 0.99
        assert np.array_equal(np.abs(n), np.abs(free))                            # the sign alone differs
    inward, _ = run(x, idx, viewpoint=np.asarray(centre, np.float32)[None])
    assert ((inward[0].astype(np.float64) * (x[0].astype(np.float64) - centre[:, None])).sum(0) < 0).all()


def test_a_nan_and_an_inf_point_stay_in_their_sets():
    x = cloud(1, 300)
    _, idx = neighbours(x, 20)
    clean_n, clean_c = run(x, idx)
    bad = x.copy()
    bad[0, 1, 17] = np.nan
    bad[0, 2, 123] = np.inf
    n, c = run(bad, idx)                                                          # (the clean cloud's neighbours)
    idx = idx.cpu().numpy()[0]
    hit = (idx == 17).any(1) | (idx == 123).any(1)
    hit[[17, 123]] = True
    assert 2 < hit.sum() < 150
    assert np.array_equal(n[0][:, hit], np.tile(np.asarray([[0], [0], [1]], np.float32), (1, hit.sum()))) and np.isnan(c[0][hit]).all()
    assert np.array_equal(bits(n[0][:, ~hit]), bits(clean_n[0][:, ~hit])) and np.array_equal(bits(c[0][~hit]), bits(clean_c[0][~hit]))


def test_idx_entries_outside_the_cloud_read_as_the_row_itself():
    B, N, k = 2, 257, 20
    x = cloud(B, N)
    _, idx = neighbours(x, k)
    idx = idx.cpu().numpy()
    rs = np.random.RandomState(10)
    own = np.broadcast_to(np.arange(N)[None, :, None], idx.shape)
    where = rs.uniform(size=idx.shape) < 0.1
    out = np.where(where, rs.choice([-1, N, N + 5, -2 ** 31, 2 ** 31 - 1], size=idx.shape), idx).astype(np.int32)
    got = run(x, out)
    want = run(x, np.where(where, own, idx))
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert not np.array_equal(bits(got[0]), bits(run(x, idx)[0]))                 # (the entries mattered)


def test_a_cloud_does_not_depend_on_its_batch():
    x = cloud(3, 257)
    _, idx = neighbours(x, 20)
    view = np.asarray([[0.5, 0.5, 3.0], [0.5, 0.5, -3.0], [3.0, 0.5, 0.5]], np.float32)
    for v in (None, view):
        whole = run(x, idx, viewpoint=v)
        for b in range(3):
            alone = run(x[b:b + 1], idx[b:b + 1], viewpoint=None if v is None else v[b:b + 1])
            assert np.array_equal(bits(alone[0]), bits(whole[0][b:b + 1])) and np.array_equal(bits(alone[1]), bits(whole[1][b:b + 1]))


def test_estimate_normals_is_the_composition_of_its_three_calls():
    import vcrnet_amd
    native, plane = mods()
    x = dev(cloud(2, 1000))
    view = dev(np.asarray([[0.5, 0.5, 3.0], [0.5, 0.5, -3.0]], np.float32))
    for k, v in ((20, None), (40, view)):
        n, c, idx = vcrnet_amd.estimate_normals(x, k, viewpoint=v, want_curvature=True, want_idx=True)
        xyz4 = native.to_rows4(x)
        idx2 = native.knn(xyz4, None, k)
        n2, c2 = plane.normals(xyz4, idx2, v)
        assert idx.dtype == torch.int32 and idx.shape == (2, 1000, k) and torch.equal(idx, idx2)
        assert torch.equal(n.view(torch.int32), n2.view(torch.int32)) and torch.equal(c.view(torch.int32), c2.view(torch.int32))
        only = vcrnet_amd.estimate_normals(x, k, viewpoint=v)
        assert torch.is_tensor(only) and only.shape == (2, 3, 1000) and torch.equal(only.view(torch.int32), n.view(torch.int32))
        assert len(vcrnet_amd.estimate_normals(x, k, viewpoint=v, want_idx=True)) == 2


def test_python_entry_points_refuse_before_any_launch():
    import vcrnet_amd
    native, plane = mods()
    x = dev(cloud(1, 64))
    with pytest.raises(native.VcrHipError, match=r"k \+ 1 = 21"):
        vcrnet_amd.estimate_normals(x[:, :, :20], 20)
    with pytest.raises(native.VcrHipError, match=r"k must be in \[1, 62\]"):
        vcrnet_amd.estimate_normals(dev(cloud(1, 257)), 63)
    with pytest.raises(native.VcrHipError, match=r"k must be in \[1, 62\]"):
        vcrnet_amd.estimate_normals(x, 0)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.estimate_normals(x.cpu())
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.estimate_normals(x.transpose(1, 2))
    with pytest.raises(native.VcrHipError, match=r"viewpoint must be a device tensor \[B, 3\]"):
        vcrnet_amd.estimate_normals(x, 20, viewpoint=torch.zeros(2, 3, device="cuda"))
    xyz4 = native.to_rows4(x)
    with pytest.raises(native.VcrHipError, match="idx must be int32"):
        plane.normals(xyz4, torch.zeros(1, 64, 20, dtype=torch.int64, device="cuda"))
    with pytest.raises(native.VcrHipError, match="vcr_normals_f32"):
        plane.normals(xyz4, torch.zeros(1, 64, 63, dtype=torch.int32, device="cuda"))
