"""The conditions tests/test_hip_far.py relies on, held on the CPU restatements alone -- so that a failure on the GPU can only be
the device's: the exactness of the grid recipes, cond(A) at the moderate offset, the restatements' inliers and at-cloud errors at
every offset, the float64 agreement of the neighbours, the RANSAC's 77 of 77, the pose-map algebra -- and one test that records
why refine_registration and register_features have a `centre` option.  No GPU."""
import functools

import numpy as np
import pytest

import far_cases as fc
import fpfh_restated as fr
import gicp_restated as gr
import match_restated as mr
import nnscore_restated as nr
import outlier_restated as orr
import plane_restated as pr
import refine_restated as rr
import voxel_restated as vr

F32, F64 = np.float32, np.float64
NB, NS = rr.SHAPES[0]


@functools.lru_cache(maxsize=None)
def torus():
    """gicp_restated.batch at the smallest shape: the recipe of every refinement test here."""
    return gr.batch(10 + NS, NB, NS)


def one(c, b):
    return {k: v[b] for k, v in c.items()}


def grid_clouds():
    """name -> [.., 3, N] fp32: every cloud the exact-translation tests of the GPU file run."""
    c, p, s = fc.gridded(torus()), fc.gridded(mr.planted(*mr.RANSAC_SHAPES[1][:2])), fc.gridded(mr.surface(600))
    out = {"torus src": c["src"], "torus tgt": c["tgt"], "planted src": p["src"], "planted tgt": p["tgt"],
           "surface src": s["src"], "surface tgt": s["tgt"]}
    for B, N, _ in fr.SHAPES[1:3]:
        out[f"fpfh cloud {N}"] = fc.on_grid(fr.cloud(B, N))
    for name in ("n257", "three_clouds"):
        out[f"voxel {name}"] = fc.on_grid(vr.RECIPES[name]()[0])
        out[f"radius {name}"] = fc.on_grid(orr.RADIUS_RECIPES[name]()[0])
        out[f"stat {name}"] = fc.on_grid(orr.STAT_RECIPES[name]()[0])
    out["fps uniform 700"] = fc.on_grid(np.random.RandomState(5).uniform(-1.0, 1.0, size=(2, 3, 700)).astype(F32))   # test_hip_fps.uniform(5, 2, 700)
    return out


def test_the_offsets_and_the_grid_recipes_are_exact():
    """fp32(x + c) is x + c and fp32((x + c) - c) is x for every cloud and offset the GPU file translates -- asserted, not
    assumed -- and is_exact does tell: off the grid it fails."""
    for c in fc.OFFSETS:
        assert all(float(v / fc.GRID).is_integer() for v in c)
    clouds = grid_clouds()
    assert len(clouds) == 15
    for name, x in clouds.items():
        assert np.isfinite(x).any() and x.dtype == F32
        for c in fc.OFFSETS:
            assert fc.is_exact(x, c), (name, c)
    assert not fc.is_exact(torus()["src"], fc.FAR_OFFSETS[0])              # the recipe as it is: not on the grid
    assert not fc.is_exact(fc.on_grid(torus()["src"]), (4096.0, 0.0, 0.0))  # past 2048
    g = fc.gridded(torus())
    assert np.abs(g["src"].astype(F64) - torus()["src"]).max() <= fc.GRID / 2


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS)
def test_the_restatements_do_not_change_under_an_exact_translation(offset):
    """The premise of the GPU file's exact-translation tests, on the definitions themselves: nnscore_restated.score without a
    pose, the radius filter, the voxel grid, FPS with a given start, the normals' covariances and the SPFH / FPFH restatements
    fed the near neighbours return the same bits on the grid recipes before and after the translation.  And the test tells: the
    kNN's fp32 expansion does NOT -- its neighbours change."""
    import fps_restated
    near, far = fc.gridded(torus()), fc.translated(fc.gridded(torus()), offset)
    a, b = nr.score(near["src"], near["tgt"], None, None, 0.25), nr.score(far["src"], far["tgt"], None, None, 0.25)
    assert (0 < a["inliers"]).all() and (a["inliers"] < NS + rr.FAR).all()
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    xyz, r, nb = orr.RADIUS_RECIPES["n257"]()
    xyz = fc.on_grid(xyz)
    ra, rb = orr.batch(orr.radius_fast, xyz, r, nb), orr.batch(orr.radius_fast, fc.moved_cloud(xyz, offset), r, nb)
    assert all(np.array_equal(ra[k], rb[k]) for k in ("count", "index", "neighbours")) and 0 < ra["count"][0] < 257
    xyz, h = vr.RECIPES["n257"]()
    xyz = fc.on_grid(xyz)
    va, vb = vr.batch(xyz, h), vr.batch(fc.moved_cloud(xyz, offset), h)
    assert all(np.array_equal(va[k], vb[k]) for k in ("count", "point_voxel", "voxel_points")) and 1 < va["count"][0] < 257
    ok = np.isfinite(va["points"])
    assert np.abs(vb["points"].astype(F64) - (va["points"].astype(F64) + np.asarray(offset)[:, None]))[ok].max() <= 2.0 ** -14
    x = grid_clouds()["fps uniform 700"]
    assert np.array_equal(fps_restated.fps(x, 64, [3, 400]), fps_restated.fps(fc.moved_cloud(x, offset), 64, [3, 400]))
    B, N, k = fr.SHAPES[1]
    x = fc.on_grid(fr.cloud(B, N))[0]
    xf = fc.moved_cloud(x, offset)
    idx = fr.neighbours(x, k)
    assert np.array_equal(pr.covariances(x, idx), pr.covariances(xf, idx))
    nrm = fr.normals(x, idx)
    sa, sb = fr.spfh(x, nrm, idx), fr.spfh(xf, nrm, idx)
    assert np.array_equal(sa, sb) and sa.max() > 0
    assert np.array_equal(fr.fpfh(x, idx, sa).view(np.int32), fr.fpfh(xf, idx, sb).view(np.int32))
    assert not np.array_equal(fc.knn_expansion_f32(x, k + 1), fc.knn_expansion_f32(xf, k + 1))


@pytest.mark.parametrize("offset", ((0.0, 0.0, 0.0),) + fc.FAR_OFFSETS)
def test_the_fgr_restatement_far_from_the_origin(offset):
    """FGR centres and scales itself: on the translated RANSAC recipe it recovers the planted rotation within tests/test_fgr_cpu.py's
    0.1 degree at every offset, and at the cloud its pose is within 1e-3 of the planted one."""
    import fgr_restated as fg
    M, share, _ = mr.RANSAC_SHAPES[1]
    c = fc.translated(mr.planted(M, share, extra=5), offset)
    r = fg.fgr(c["src"], c["tgt"], c["corr"])
    R, t = r["pose64"][:9].reshape(3, 3), r["pose64"][9:]
    deg, e = fg.rotation_error_deg(R, c["R"]), fc.at_cloud_error(R, t, c["R"], c["t"], c["src"][:, c["good"]])
    print(f"far cpu: fgr offset {offset[0]:g}: rotation error {deg:.3e} deg, at-cloud error {e:.2e}, {r['tuples']} tuples")
    assert r["status"] == 0 and r["pairs"] == 257 and deg <= 0.1 and e <= 1e-3


def test_translated_maps_clouds_and_poses():
    c = torus()
    off = np.asarray(fc.FAR_OFFSETS[1])
    f = fc.translated(c, off)
    assert f["nrm_t"] is c["nrm_t"] and f["nrm_s"] is c["nrm_s"] and f["twin"] is c["twin"] and f["R"] is c["R"]
    assert f["src"].dtype == F32 and f["t0"].dtype == F32 and f["t"].dtype == F64
    for b in range(3):
        p = c["src"][b][:, :NS].astype(F64)
        want = c["R"][b] @ p + c["t"][b][:, None] + off[:, None]
        got = f["R"][b] @ (p + off[:, None]) + f["t"][b][:, None]
        assert np.abs(got - want).max() <= 1e-12 * 2048
        assert np.abs(f["t0"][b] - (c["t0"][b].astype(F64) + off - c["R0"][b].astype(F64) @ off)).max() <= np.spacing(F32(2048)) / 2
        # measured at the cloud the translated start is as far off as the recipe's; at the origin it is not
        near = fc.at_cloud_error(c["R0"][b], c["t0"][b], c["R"][b], c["t"][b], c["src"][b][:, :NS])
        far = fc.at_cloud_error(f["R0"][b], f["t0"][b], f["R"][b], f["t"][b], f["src"][b][:, :NS])
        assert abs(far - near) <= 2e-4 and pr.pose_error(f["R0"][b], f["t0"][b], f["R"][b], f["t"][b])[1] > 50 * near
    m = fc.translated(mr.planted(40, 0.5), off)
    assert "t0" not in m and m["corr"].dtype == np.int32


def test_the_pose_maps_round_trip():
    """centred_pose and uncentred_pose are inverses: t + R c_s - c_t - R c_s + c_t returns to t within one fp32 ulp at the
    largest term; and a pose carried to the centred frames moves the centred source onto the centred target."""
    c = fc.translated(torus(), fc.FAR_OFFSETS[1])
    for b in range(3):
        cs, ct = fc.centre_of(c["src"][b]), fc.centre_of(c["tgt"][b])
        R, t = c["R0"][b], c["t0"][b]
        _, tc = fc.centred_pose(R, t, cs, ct)
        tc32 = tc.astype(F32)                                   # (what the device hands the kernels)
        _, back = fc.uncentred_pose(R, tc32, cs, ct)
        assert np.abs(back - t.astype(F64)).max() <= np.spacing(F32(np.abs(t).max()))
        p = c["src"][b].astype(F64)
        direct = R.astype(F64) @ p + t.astype(F64)[:, None] - ct.astype(F64)[:, None]
        through = R.astype(F64) @ (p - cs.astype(F64)[:, None]) + tc[:, None]
        assert np.abs(direct - through).max() <= 1e-9
        assert np.abs(tc).max() < 4.0                          # the centred pose is small again


@functools.lru_cache(maxsize=None)
def step_conditions():
    """cond(A) of the first update at the moderate offset, uncentred: (plane, gicp) per cloud."""
    f = fc.translated(torus(), fc.MODERATE)
    out = []
    for b in range(3):
        k = one(f, b)
        ev = rr.evaluate(k["src"], k["tgt"], k["R0"], k["t0"], rr.MAX_DIST)
        p = pr.plane_step(k["src"], k["tgt"], k["nrm_t"], k["R0"], k["t0"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
        g = gr.gicp_step(k["src"], k["tgt"], k["nrm_s"], k["nrm_t"], k["R0"], k["t0"], ev["nn_idx"], ev["nn_d2"], rr.MAX_DIST)
        out.append((p["cond"], g["cond"]))
    return out


def test_the_condition_at_the_moderate_offset():
    """Above anything the near-origin suite reaches (1e6), below 1e8: the one-update bound 2^-22 + 64 cond(A) 2^-53 stays under
    2^-20 there."""
    for b, (cp, cg) in enumerate(step_conditions()):
        print(f"far cpu: moderate offset cloud {b}: cond(A) plane {cp:.3e} gicp {cg:.3e}")
        assert 1e6 < cp < 1e8 and 1e6 < cg < 1e8


def _loops(c, b, centre):
    """(point, plane, gicp) restated loops of ten updates on cloud b of c; centre: about each cloud's own centre, the pose
    carried back in float64."""
    k = one(c, b)
    src, tgt, R0, t0 = k["src"], k["tgt"], k["R0"], k["t0"]
    cs = ct = np.zeros(3, F32)
    if centre:
        cs, ct = fc.centre_of(src), fc.centre_of(tgt)
        src, tgt = src - cs[:, None], tgt - ct[:, None]
        t0 = fc.centred_pose(R0, t0, cs, ct)[1].astype(F32)
    kw = dict(max_dist=rr.MAX_DIST, max_iterations=10, rel_fitness=0.0, rel_rmse=0.0)
    runs = (rr.icp(src, tgt, R0, t0, **kw), pr.plane_icp(src, tgt, k["nrm_t"], R0, t0, **kw),
            gr.gicp_icp(src, tgt, k["nrm_s"], k["nrm_t"], R0, t0, **kw))
    out = []
    for r in runs:
        R, t = fc.uncentred_pose(r["R"], r["t"], cs, ct)
        out.append((r["inliers"], r["iterations"], fc.at_cloud_error(R, t, k["R"], k["t"], k["src"][:, :NS])))
    return out


@functools.lru_cache(maxsize=None)
def loops(offset, centre, b=0):
    return _loops(fc.translated(torus(), offset) if offset else torus(), b, centre)


def test_why_the_centre_option_exists():
    """At (128, -64, 32), from a start 6 degrees off: uncentred, the point-to-plane and the plane-to-plane loops lose EVERY
    inlier within a few updates -- a step linearised about the origin, applied exactly, overshoots by about a^2 r / 2 -- while
    the point-to-point loop keeps them all; about the clouds' own centres all three keep them all.  And the kNN's fp32 expansion
    keeps under 95 % of the true neighbours there, all of them after centring."""
    point, plane, gicp = loops(fc.FAR_OFFSETS[0], False)
    print(f"far cpu: offset 128 uncentred: inliers point {point[0]} plane {plane[0]} (after {plane[1]}) gicp {gicp[0]} (after {gicp[1]})")
    assert point[0] == NS and point[1] == 10
    assert plane[0] == 0 and plane[1] < 10 and gicp[0] == 0 and gicp[1] < 10
    assert plane[2] > rr.MAX_DIST and gicp[2] > rr.MAX_DIST
    for r in loops(fc.FAR_OFFSETS[0], True):
        assert r[0] == NS and r[1] == 10 and r[2] <= 1e-5
    x = pr.jittered_torus(3, 1000)
    far = fc.moved_cloud(x, fc.FAR_OFFSETS[0])
    kept_far, kept_near = fc.kept_neighbours(far, 20), fc.kept_neighbours(far - fc.centre_of(far)[:, None], 20)
    print(f"far cpu: kNN expansion in fp32, 1000 points, k 20: kept {kept_far:.3f} at offset 128, {kept_near:.3f} centred")
    assert kept_far < 0.95 and kept_near == 1.0


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS)
def test_the_restatements_far_from_the_origin(offset):
    """What the GPU file's margins are set against: the point-to-point loop uncentred, the two six-unknown loops centred, keep
    every clean source point at both far offsets, and their at-cloud errors stay at the fp32 grid of the inputs."""
    ulp = fc.ulp_at(np.asarray(offset, F32) + 1)
    for b in range(3):
        point = loops(offset, False, b)[0]
        _, plane, gicp = loops(offset, True, b)
        print(f"far cpu: offset {offset[0]:g} cloud {b}: at-cloud error point {point[2]:.2e} plane (centred) {plane[2]:.2e} gicp "
              f"(centred) {gicp[2]:.2e}, one ulp {ulp:.2e}")
        for r in (point, plane, gicp):
            assert r[0] == NS and r[1] == 10 and r[2] <= 2 * ulp


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS)
def test_the_fp32_neighbours_are_the_float64_ones(offset):
    """nnscore_restated.score under the start pose, far away: no neighbour differs from the float64 arg-min of the same fp32
    moved points (3 x 337 = 1011 source points)."""
    f = fc.translated(torus(), offset)
    got = nr.score(f["src"], f["tgt"], f["R0"], f["t0"], rr.MAX_DIST)
    differ = 0
    for b in range(3):
        moved = nr.moved(f["src"][b], f["R0"][b], f["t0"][b])
        idx64 = nr.nearest_f64(moved, f["tgt"][b])[0]
        differ += int((np.asarray(idx64) != got["nn_idx"][b]).sum())
    assert got["nn_idx"].size == 1011 and differ == 0
    assert (got["inliers"] > 0.9 * NS).all() and (got["inliers"] <= NS).all()


@pytest.mark.parametrize("offset", ((0.0, 0.0, 0.0),) + fc.FAR_OFFSETS)
def test_the_ransac_holds_the_77_planted_pairs(offset):
    M, share, T = mr.RANSAC_SHAPES[1]
    c = fc.translated(mr.planted(M, share), offset)
    r = mr.ransac(c["src"], c["tgt"], c["corr"], mr.MAX_DIST, mr.SIMILARITY, T, mr.SEED)
    good = np.nonzero(c["good"])[0]
    assert len(good) == 77 and r["inliers"] == 77 and c["good"][r["picks"][r["best_trial"]]].all()
    moved = r["R"].astype(F64) @ c["src"][:, good].astype(F64) + r["t"].astype(F64)[:, None]
    assert np.sqrt(((moved - c["tgt"][:, c["corr"][good]].astype(F64)) ** 2).sum(0)).max() <= mr.MAX_DIST


def test_the_documents_name_the_helper():
    import os
    import vcrnet_amd
    from vcrnet_amd import centre, fpfh, match, outlier, plane, refine
    assert vcrnet_amd.centred is centre.centred and vcrnet_amd.uncentred_pose is centre.uncentred_pose
    assert {"centred", "uncentred_pose"} <= set(vcrnet_amd.__all__)
    for fn in (plane.estimate_normals, fpfh.compute_fpfh_feature, outlier.remove_statistical_outlier):
        assert "Centre such a cloud first" in fn.__doc__ and "centred" in fn.__doc__, fn.__name__
    for fn in (refine.refine_registration, match.register_features):
        assert "centre" in fn.__doc__ and "uncentred_pose" in fn.__doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "### 4.18" in open(os.path.join(root, "DESIGN.md")).read()
    assert "centre=True" in open(os.path.join(root, "INTEGRATION.md")).read()


def test_the_centre_option_refuses_what_it_cannot_read():
    import torch
    import vcrnet_amd
    from vcrnet_amd.native import VcrHipError
    a = torch.zeros(1, 3, 8)
    with pytest.raises(VcrHipError, match="HIP path only"):
        vcrnet_amd.refine_registration(a, a, max_dist=0.1, centre=True)
    with pytest.raises(VcrHipError, match="method must be one of"):
        vcrnet_amd.refine_registration(a, a, max_dist=0.1, method="plane", centre=True)
    x, c = vcrnet_amd.centred(torch.tensor([[[1.0, 3.0, float("nan")], [2.0, 2.0, 2.0], [float("inf"), 0.0, 4.0]]]))
    assert c.tolist() == [[2.0, 2.0, 2.0]] and x[0, 0, :2].tolist() == [-1.0, 1.0] and x.dtype == torch.float32
    with pytest.raises(VcrHipError, match=r"\[B, 3\]"):
        vcrnet_amd.centred(a, torch.zeros(3))
    with pytest.raises(VcrHipError, match="centre must be False, True or a pair"):
        from vcrnet_amd import centre as cm
        cm.take_centres("refine_registration", "yes", a, a)
    R, t = torch.eye(3)[None], torch.tensor([[1.0, 2.0, 3.0]])
    cs, ct = torch.tensor([[100.0, 0.0, 0.0]]), torch.tensor([[0.0, 50.0, 0.0]])
    _, tc = cm.centred_pose(R, t, cs, ct)
    assert tc.tolist() == [[101.0, -48.0, 3.0]] and vcrnet_amd.uncentred_pose(R, tc, cs, ct)[1].tolist() == t.tolist()
    assert cm.centred_pose(None, None, cs, ct)[1].tolist() == [[100.0, -50.0, 0.0]]
