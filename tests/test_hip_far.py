"""The registration stack on clouds far from the origin relative to their extent: the recipes of the
other GPU files moved by tests/far_cases.py's offsets.  tests/test_far_cpu.py holds every condition used here on the CPU
restatements alone.  Three kinds of check:

  * EXACT TRANSLATIONS.  On coordinates of the 2^-12 grid a translation is exact in fp32, so every kernel that works from
    coordinate differences must return the same bits before and after it -- no reference, no tolerance.  A kernel that slipped
    in an expansion, an absolute coordinate or an fp32 accumulation of positions fails.  (native.knn is not among them: its
    limit is documented.)  The runs go through the other files' `run` helpers: the guard bands and prefills are checked.
  * FAR CLOUDS WITH A POSE against the restatements on the same fp32 inputs: nn_score bit for bit, the point-to-point loop by
    its at-cloud error, one update of the two six-unknown fits at the moderate offset by the files' own bound (cond(A) 4e6 to
    7e6: above anything the near-origin suite reaches), the RANSAC by test_hip_match's stages, FGR as test_hip_fgr holds it.
  * THE `centre` OPTION of refine_registration and register_features.

Every margin is set against the restatement or the number format, never against the device's own output.  The measured values
are printed and go to far_ledger.txt under VCR_LEDGER_DIR."""
import functools
import os

import numpy as np
import pytest
import torch

import far_cases as fc
import fgr_restated as fg
import fpfh_restated as fr
import fps_restated
import gicp_restated as gr
import match_restated as mr
import nnscore_restated as nr
import outlier_restated as orr
import plane_restated as pr
import refine_restated as rr
import voxel_restated as vr

import test_hip_fgr as t_fgr
import test_hip_fpfh as t_fpfh
import test_hip_fps as t_fps
import test_hip_gicp as t_gicp
import test_hip_match as t_match
import test_hip_nnscore as t_nn
import test_hip_normals as t_normals
import test_hip_outlier as t_outlier
import test_hip_plane as t_plane
import test_hip_refine as t_refine
import test_hip_voxel as t_voxel

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NB, NS = rr.SHAPES[0]
FAR = rr.FAR
EVAL = t_refine.EVAL
TEN = dict(max_iterations=10, rel_fitness=0.0, rel_rmse=0.0)
LEDGER = []


def _emit(line):
    print(line)
    LEDGER.append(line)
    out = os.environ.get("VCR_LEDGER_DIR", "")
    if os.path.isdir(out):
        path = os.path.join(out, "far_ledger.txt")
        if len(LEDGER) == 1:                                 # a new table: which kernel sources it measures
            import vcrnet_amd  # noqa: F401
            from vcrnet_amd import build as vb
            with open(path, "w") as f:
                f.write(f"# kernel_sources_sha16={vb.sources_sha16()}\n")
        with open(path, "a") as f:
            f.write(line + "\n")


def dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x)).cuda()         # (a copy: the recipes are read-only)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(t):
    return t.cpu().numpy()


def tag(offset):
    return f"offset {offset[0]:g}"


@functools.lru_cache(maxsize=None)
def torus():
    return gr.batch(10 + NS, NB, NS)


@functools.lru_cache(maxsize=None)
def grid_torus():
    return fc.gridded(torus())


@functools.lru_cache(maxsize=None)
def far_torus(offset, grid=False):
    return fc.translated(grid_torus() if grid else torus(), offset)


def one(c, b):
    return {k: v[b] for k, v in c.items()}


def moved_exactly(far, near, c):
    """far == near + c in every finite coordinate, bit for bit; NaN where near is NaN."""
    want = fc.moved_cloud(near, c)
    ok = np.isfinite(near)
    return far.shape == near.shape and np.array_equal(np.isnan(far), np.isnan(near)) and np.array_equal(bits(far)[ok], bits(want)[ok])


# =========================================================================================== exact translations: the same bits

@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
def test_nn_score_without_a_pose_does_not_change_under_an_exact_translation(offset):
    from vcrnet_amd import score
    near, far = grid_torus(), far_torus(offset, True)
    assert fc.is_exact(near["src"], offset) and fc.is_exact(near["tgt"], offset)
    max_dist = 0.25                                          # (no pose: the clouds are 40 degrees apart; some pairs are within, most not)
    for v in (0, score.variant(2, 3)):
        a = t_nn.run(np.array(near["src"]), np.array(near["tgt"]), max_dist=max_dist, variant=v)     # (copies: the recipes are read-only)
        b = t_nn.run(np.array(far["src"]), np.array(far["tgt"]), max_dist=max_dist, variant=v)
        assert (0 < a["inliers"]).all() and (a["inliers"] < NS + FAR).all()
        t_nn.assert_same_bits(b, a, (offset, v))
        t_nn.assert_same_bits(a, nr.score(near["src"], near["tgt"], None, None, max_dist), "the restatement")


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
@pytest.mark.parametrize("name", ["n257", "three_clouds"])
def test_the_radius_filter_does_not_change_under_an_exact_translation(name, offset):
    xyz, r, nb = orr.RADIUS_RECIPES[name]()
    xyz = fc.on_grid(xyz)
    assert fc.is_exact(xyz, offset)
    a, b = t_outlier.run_radius(xyz, r, nb), t_outlier.run_radius(fc.moved_cloud(xyz, offset), r, nb)
    assert (0 < a["count"]).all() and (a["count"] < xyz.shape[2]).all()
    for k in ("count", "index", "neighbours"):
        assert same(a[k], b[k]), k
    assert moved_exactly(b["points"], a["points"], offset)


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
@pytest.mark.parametrize("name", ["n257", "three_clouds"])
def test_the_voxel_grid_does_not_change_under_an_exact_translation(name, offset):
    xyz, h = vr.RECIPES[name]()
    xyz = fc.on_grid(xyz)
    assert fc.is_exact(xyz, offset)
    far = fc.moved_cloud(xyz, offset)
    a, b = t_voxel.run(xyz, h), t_voxel.run(far, h)
    assert (1 < a["count"]).all() and (a["count"] < xyz.shape[2]).all()
    for k in ("count", "point_voxel", "voxel_points"):
        assert same(a[k], b[k]), k
    t_voxel.assert_same(b, vr.batch(far, h), "the restatement on the translated input")
    ok = np.isfinite(a["points"])
    assert np.array_equal(np.isnan(a["points"]), np.isnan(b["points"]))
    gap = np.abs(b["points"].astype(F64) - (a["points"].astype(F64) + np.asarray(offset)[:, None]))[ok].max()
    assert gap <= 2.0 ** -14, gap                            # a mean rounded to fp32 below 2048: half an ulp there


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
def test_fps_with_a_given_start_does_not_change_under_an_exact_translation(offset):
    x = fc.on_grid(t_fps.uniform(5, 2, 700))
    assert fc.is_exact(x, offset)
    for v in t_fps.forms_for(700):
        a, b = t_fps.run(x, 64, start=[3, 400], variant=v), t_fps.run(fc.moved_cloud(x, offset), 64, start=[3, 400], variant=v)
        assert np.array_equal(a, b) and a[:, 0].tolist() == [3, 400] and len(set(a[0].tolist())) == 64
    assert np.array_equal(a, fps_restated.fps(x, 64, [3, 400]))


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
@pytest.mark.parametrize("B,N,k", fr.SHAPES[1:3])
def test_the_second_stages_fed_the_near_neighbours_do_not_change(B, N, k, offset):
    """plane.normals, fpfh.spfh and fpfh.fpfh on the translated rows with the UNTRANSLATED run's idx (and, for the features, its
    normals): the same normals, curvature, bytes and features."""
    from vcrnet_amd import native
    x = fc.on_grid(fr.cloud(B, N))
    assert fc.is_exact(x, offset)
    far = fc.moved_cloud(x, offset)
    near4, idx = t_normals.neighbours(x, k)
    far4 = native.to_rows4(dev(far))
    n_a, c_a = t_normals.run(x, idx)
    n_b, c_b = t_normals.run(far, idx)
    assert same(n_a, n_b) and same(c_a, c_b)
    assert np.abs(np.linalg.norm(n_a.astype(F64), axis=1) - 1).max() <= 1e-6
    nrm = dev(n_a)
    sp_a, sp_b = t_fpfh.run_spfh(near4, nrm, idx), t_fpfh.run_spfh(far4, nrm, idx)
    assert torch.equal(sp_a, sp_b) and int(sp_a.max()) > 0
    f_a, f_b = t_fpfh.run_fpfh(near4, idx, sp_a), t_fpfh.run_fpfh(far4, idx, sp_b)
    assert same(host(f_a), host(f_b)) and float(f_a.max()) > 0


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
@pytest.mark.parametrize("name", ["n257", "three_clouds"])
def test_the_statistical_filter_fed_the_near_neighbours_does_not_change(name, offset):
    xyz, k, ratio = orr.STAT_RECIPES[name]()
    xyz = fc.on_grid(xyz)
    assert fc.is_exact(xyz, offset)
    from vcrnet_amd import native
    rows, idx = t_outlier.knn(xyz, k)
    far_rows = native.to_rows4(dev(fc.moved_cloud(xyz, offset)))
    a, b = t_outlier.run_stat(rows, idx, ratio), t_outlier.run_stat(far_rows, idx, ratio)
    assert (0 < a["count"]).all() and (a["count"] < xyz.shape[2]).all()
    for key in ("count", "index", "mean_dist", "valid", "stats"):
        assert same(a[key], b[key]), key
    assert moved_exactly(b["points"], a["points"], offset)


# ================================================================================ far clouds with a pose, against the restatements

@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
def test_nn_score_with_the_start_pose_is_the_restatement_bit_for_bit(offset):
    from vcrnet_amd import score
    f = far_torus(offset)
    want = nr.score(f["src"], f["tgt"], f["R0"], f["t0"], rr.MAX_DIST)
    assert (want["inliers"] > 0.9 * NS).all() and (want["inliers"] <= NS).all()
    for v in (0, score.variant(4, 2)):
        got = t_nn.run(*(np.array(f[k]) for k in ("src", "tgt", "R0", "t0")), rr.MAX_DIST, variant=v)   # (copies: read-only recipes)
        assert np.array_equal(got["nn_idx"], want["nn_idx"]), v
        t_nn.assert_same_bits(got, want, (offset, v))


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
def test_the_point_to_point_loop_far_from_the_origin(offset):
    """Ten updates, uncentred: the device's at-cloud error is at most twice refine_restated.icp's plus one fp32 ulp at the
    largest |coordinate| -- the files' rule 2 x restated + 2^-20 with the margin on the grid the inputs live on.  The closing
    invariant is test_hip_refine.run's."""
    f = far_torus(offset)
    o = t_refine.run(f["src"], f["tgt"], f["R0"], f["t0"], **TEN)
    assert o["iterations"].tolist() == [10, 10, 10]
    ulp = fc.ulp_at(f["src"][:, :, :NS], f["tgt"])
    for b in range(3):
        k = one(f, b)
        ref = rr.icp(k["src"], k["tgt"], k["R0"], k["t0"], rr.MAX_DIST, 10, 0.0, 0.0)
        e_dev = fc.at_cloud_error(o["R"][b], o["t"][b], k["R"], k["t"], k["src"][:, :NS])
        e_ref = fc.at_cloud_error(ref["R"], ref["t"], k["R"], k["t"], k["src"][:, :NS])
        _emit(f"far point_to_point {tag(offset)} cloud {b}: at-cloud error device {e_dev:.3e} restated {e_ref:.3e} ulp {ulp:.3e} "
              f"inliers device {o['inliers'][b]} restated {ref['inliers']}")
        assert ref["inliers"] == NS and ref["iterations"] == 10
        assert e_dev <= 2 * e_ref + ulp, (e_dev, e_ref, ulp)
        assert o["inliers"][b] == NS


@pytest.mark.parametrize("method", ["point_to_plane", "generalized"])
def test_one_update_of_the_six_unknown_fits_at_the_moderate_offset(method):
    """Uncentred at (16, -8, 4), against plane_step / gicp_step on the device's own iteration-0 neighbours: |dR| <= bound and
    |dt| <= bound max(1, |t|) with the files' bound 2^-22 + 64 cond(A) 2^-53 -- both of its terms are relative errors, and t is
    about 20 here.  Pins the fp64 sums and the Cholesky solve at cond(A) of 4e6 to 7e6."""
    f = far_torus(fc.MODERATE)
    if method == "point_to_plane":
        go = lambda **kw: t_plane.run(f["src"], f["tgt"], f["nrm_t"], f["R0"], f["t0"], **kw)                       # noqa: E731
        step = lambda k, z: pr.plane_step(k["src"], k["tgt"], k["nrm_t"], k["R0"], k["t0"], z[0], z[1], rr.MAX_DIST)  # noqa: E731
    else:
        go = lambda **kw: t_gicp.run(f["src"], f["tgt"], f["nrm_s"], f["nrm_t"], f["R0"], f["t0"], **kw)            # noqa: E731
        step = lambda k, z: gr.gicp_step(k["src"], k["tgt"], k["nrm_s"], k["nrm_t"], k["R0"], k["t0"], z[0], z[1], rr.MAX_DIST)  # noqa: E731
    zero = go(max_iterations=0)
    one_up = go(max_iterations=1, rel_fitness=0.0, rel_rmse=0.0)
    assert zero["iterations"].tolist() == [0] * 3 and one_up["iterations"].tolist() == [1] * 3
    for b in range(3):
        k = one(f, b)
        up = step(k, (zero["nn_idx"][b], zero["nn_d2"][b]))
        assert up is not None and up["n"] == zero["inliers"][b] >= 6
        R0, t0 = k["R0"].astype(F64), k["t0"].astype(F64)
        t_want = up["R"] @ t0 + up["t"]
        dR = np.abs(one_up["R"][b] - up["R"] @ R0).max()
        dt = np.abs(one_up["t"][b] - t_want).max()
        bound = 2.0 ** -22 + 64 * up["cond"] * 2.0 ** -53
        scale = max(1.0, float(np.abs(t_want).max()))
        _emit(f"far {method} step offset 16 cloud {b}: n {up['n']} cond(A) {up['cond']:.3e} |dR| {dR:.2e} |dt| {dt:.2e} "
              f"bound {bound:.2e} |t| {scale:.1f}")
        assert 1e6 < up["cond"] < 1e8
        assert dR <= bound and dt <= bound * scale, (dR, dt, bound, scale)
        assert 0 < np.abs(one_up["R"][b] - k["R0"]).max()        # (a step was taken)


@functools.lru_cache(maxsize=None)
def far_planted(offset, extra=0):
    M, share, _ = mr.RANSAC_SHAPES[1]
    return fc.translated(mr.planted(M, share, extra=extra), offset)


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
def test_the_ransac_far_from_the_origin_by_its_stages(offset):
    """test_hip_match.staged on the translated recipe: the draws and early tests exact, the solve by its properties, the
    distance check and the count exact from the device's own poses, the winner by the arg-max rule -- and the winner holds all
    77 planted pairs, as the restatement's does at every offset."""
    M, share, T = mr.RANSAC_SHAPES[1]
    c = far_planted(offset)
    o = t_match.run_ransac(c["src"][None], c["tgt"][None], c["corr"][None], T)
    valid = t_match.staged(o, 0, c["src"], c["tgt"], c["corr"], T)
    _emit(f"far ransac {tag(offset)}: {valid} valid trials, best {o['best_trial'][0]} with {o['inliers'][0]} of {int(c['good'].sum())}")
    assert valid >= 1 and int(c["good"].sum()) == 77
    t_match.planted_recovered(o, 0, c)


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
def test_fgr_far_from_the_origin_is_the_restatement(offset):
    """As test_hip_fgr holds it: pairs, the tuple list, the normalisation, the first iteration's sums and mu are the
    restatement's bits; the final pose within that file's allowance, computed from the restatement alone (64 x the spread of a
    one-ulp nudge of every Ri)."""
    c = far_planted(offset, extra=5)
    want1 = fg.fgr(c["src"], c["tgt"], c["corr"], iterations=1)
    o1 = t_fgr.one(c, iterations=1)
    assert (o1["pairs"][0], o1["tuples"][0], o1["used"][0], o1["status"][0]) == (257, want1["tuples"], want1["used"], 0)
    assert np.array_equal(o1["tuple_list"][0, :want1["used"]], want1["list"]) and want1["used"] >= 30
    assert t_fgr.same(o1["norm"][0], want1["norm"]) and t_fgr.same(o1["sums"][0], want1["sums"]) and t_fgr.same(o1["mu"], [want1["mu"]])
    want = fg.fgr(c["src"], c["tgt"], c["corr"])
    spread = max(float(np.abs(fg.fgr(c["src"], c["tgt"], c["corr"], nudge=lambda it, Ri, way=way: np.nextafter(Ri, way))["pose64"]
                              - want["pose64"]).max()) for way in (np.inf, -np.inf))
    o = t_fgr.one(c)
    diff = float(np.abs(o["pose64"][0] - want["pose64"]).max())
    e_dev = fc.at_cloud_error(o["R"][0], o["t"][0], c["R"], c["t"], c["src"][:, c["good"]])
    e_ref = fc.at_cloud_error(want["pose64"][:9].reshape(3, 3), want["pose64"][9:], c["R"], c["t"], c["src"][:, c["good"]])
    _emit(f"far fgr {tag(offset)}: device - restatement {diff:.3g} allowance {64 * spread:.3g}; at-cloud error device {e_dev:.3e} "
          f"restated {e_ref:.3e}; rotation error restated {fg.rotation_error_deg(want['pose64'][:9].reshape(3, 3), c['R']):.3e} deg")
    assert 0 < spread and diff <= 64 * spread, (diff, spread)
    assert t_fgr.same(o["mu"], [want["mu"]]) and o["status"][0] == 0


# ============================================================================================================ the centre option

PUBLIC = t_gicp.PUBLIC
METHODS = {"point_to_plane": lambda c: dict(tgt_normals=dev(c["nrm_t"])),
           "generalized": lambda c: dict(src_normals=dev(c["nrm_s"]), tgt_normals=dev(c["nrm_t"]))}


def restated_centred(method, k, cs, ct):
    """plane_icp / gicp_icp on cloud k centred at cs, ct (the device's own centres), ten updates; the pose carried back in
    float64."""
    src, tgt = k["src"] - cs[:, None], k["tgt"] - ct[:, None]
    t0 = fc.centred_pose(k["R0"], k["t0"], cs, ct)[1].astype(F32)
    if method == "point_to_plane":
        r = pr.plane_icp(src, tgt, k["nrm_t"], k["R0"], t0, rr.MAX_DIST, 10, 0.0, 0.0)
    else:
        r = gr.gicp_icp(src, tgt, k["nrm_s"], k["nrm_t"], k["R0"], t0, rr.MAX_DIST, 10, 0.0, 0.0)
    R, t = fc.uncentred_pose(r["R"], r["t"], cs, ct)
    return r, R, t


@pytest.mark.parametrize("offset", fc.FAR_OFFSETS, ids=tag)
@pytest.mark.parametrize("method", sorted(METHODS))
def test_centre_true_keeps_the_six_unknown_fits_far_from_the_origin(method, offset):
    """Where the uncentred fit loses every inlier (tests/test_far_cpu.py): with centre=True every cloud makes its ten updates,
    keeps at least 0.99 Ns inliers (a cap: the centred restatement keeps all Ns), ends within twice the centred restatement's
    at-cloud error plus one fp32 ulp at the largest |coordinate|, and returns exactly score_registration's evaluation of the
    returned pose on the caller's clouds."""
    import vcrnet_amd
    f = far_torus(offset)
    s, q, R0, t0 = dev(f["src"]), dev(f["tgt"]), dev(f["R0"]), dev(f["t0"])
    res = vcrnet_amd.refine_registration(s, q, R0, t0, max_dist=rr.MAX_DIST, method=method, want_nn=True, centre=True,
                                         **TEN, **METHODS[method](f))
    assert sorted(res) == sorted([a for a, _ in PUBLIC] + ["nn_idx", "nn_d2"])
    closing = vcrnet_amd.score_registration(s, q, res["R"], res["t"], max_dist=rr.MAX_DIST, want_nn=True)
    for key in ("fitness", "inlier_rmse", "inliers", "nn_idx", "nn_d2"):
        assert res[key].dtype == closing[key].dtype and torch.equal(res[key], closing[key]), key
    cs, ct = host(vcrnet_amd.centred(s)[1]), host(vcrnet_amd.centred(q)[1])
    for got, x in ((cs, f["src"]), (ct, f["tgt"])):             # (the mean of the finite coordinates; the sums' order is the device's)
        assert np.abs(got - fc.centre_of(x)).max() <= np.spacing(F32(np.abs(offset).max()))
    o = {k: host(v) for k, v in res.items()}
    assert o["iterations"].tolist() == [10, 10, 10]
    assert np.array_equal(bits(o["R_ba"]), bits(o["R"].transpose(0, 2, 1)))
    ulp = fc.ulp_at(f["src"][:, :, :NS], f["tgt"])
    for b in range(3):
        k = one(f, b)
        ref, R, t = restated_centred(method, k, cs[b], ct[b])
        e_dev = fc.at_cloud_error(o["R"][b], o["t"][b], k["R"], k["t"], k["src"][:, :NS])
        e_ref = fc.at_cloud_error(R, t, k["R"], k["t"], k["src"][:, :NS])
        back = np.abs(o["t_ba"][b] + o["R"][b].astype(F64).T @ o["t"][b].astype(F64)).max()
        _emit(f"far centred {method} {tag(offset)} cloud {b}: at-cloud error device {e_dev:.3e} restated {e_ref:.3e} ulp {ulp:.3e} "
              f"inliers device {o['inliers'][b]} restated {ref['inliers']} |t_ba + R^T t| {back:.2e}")
        assert ref["inliers"] == NS and ref["iterations"] == 10
        assert e_dev <= 2 * e_ref + ulp, (e_dev, e_ref, ulp)
        assert o["inliers"][b] >= 0.99 * NS
        # the inverse is carried back on its own: t and t_ba each round once (half an ulp, the first turned by R^T: sqrt(3)
        # of it), and R^T R - I of an fp32 rotation (2^-23) meets |c| (an ulp): under three ulps, held to four
        assert back <= 4 * ulp


def test_given_centres_on_the_grid_return_the_near_origin_run():
    """The exact-grid recipe at (1024, -512, 256 + 5 2^-12) with centre=(c, c): the centred clouds ARE the near-origin ones, so
    iterations, converged and R are the near-origin run's bits, and t is t_near + c - R c within 2 fp32 ulp at |c|.  The start:
    the far start carried to the centred frame rounds once more (an ulp at |c|), so the near-origin run starts from THAT pose
    -- centred_pose of the same inputs --, within an ulp at |c| of the recipe's; from the identity (c - c = 0 exactly) nothing
    needs carrying."""
    import vcrnet_amd
    from vcrnet_amd import centre
    offset = fc.FAR_OFFSETS[1]
    near, far = grid_torus(), far_torus(offset, True)
    c = dev(np.tile(np.asarray(offset, F32), (3, 1)))
    sn, qn, sf, qf = dev(near["src"]), dev(near["tgt"]), dev(far["src"]), dev(far["tgt"])
    xc, cc = vcrnet_amd.centred(sf, c)
    assert torch.equal(xc.view(torch.int32), sn.view(torch.int32)) and torch.equal(cc, c)
    R0, t0 = dev(far["R0"]), dev(far["t0"])
    t0_near = centre.centred_pose(R0, t0, c, c)[1]
    assert np.abs(host(t0_near) - near["t0"]).max() <= np.spacing(F32(1024))
    ulp = float(np.spacing(F32(np.abs(offset).max())))
    for method, start in (("point_to_plane", True), ("generalized", True), ("point_to_point", True), ("generalized", False)):
        kw = METHODS[method](near) if method in METHODS else {}
        a = vcrnet_amd.refine_registration(sn, qn, R0 if start else None, t0_near if start else None, max_dist=rr.MAX_DIST, method=method, **kw)
        b = vcrnet_amd.refine_registration(sf, qf, R0 if start else None, t0 if start else None, max_dist=rr.MAX_DIST, method=method,
                                           centre=(c, c), **kw)
        for key in ("iterations", "converged", "R", "R_ba"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (method, start, key)
        if start:
            assert (host(a["iterations"]) >= 1).all()
        R, co = host(b["R"]).astype(F64), np.asarray(offset, F64)
        want = host(a["t"]).astype(F64) + co - R @ co
        gap = np.abs(host(b["t"]) - want).max()
        _emit(f"far given centres {method} start {start}: iterations {host(b['iterations']).tolist()} |t - (t_near + c - R c)| {gap:.2e} "
              f"(2 ulp {2 * ulp:.2e}) inliers near {host(a['inliers']).tolist()} far {host(b['inliers']).tolist()}")
        assert gap <= 2 * ulp


def test_centre_true_with_normals_estimated_inside():
    """tgt_normals=None: the normals come from the kNN, which keeps a tenth of the true neighbours at this offset and all of
    them about the cloud's centre -- centre=True centres before it estimates."""
    import vcrnet_amd
    f = far_torus(fc.FAR_OFFSETS[1])
    res = vcrnet_amd.refine_registration(dev(f["src"]), dev(f["tgt"]), dev(f["R0"]), dev(f["t0"]), max_dist=rr.MAX_DIST,
                                         method="point_to_plane", centre=True)
    fit = host(res["fitness"])
    _emit(f"far centred point_to_plane, normals estimated inside, offset 1024: fitness {fit.tolist()} iterations "
          f"{host(res['iterations']).tolist()} converged {host(res['converged']).tolist()}")
    assert host(res["converged"]).tolist() == [1, 1, 1]
    assert (fit >= F32(0.99 * NS / (NS + FAR))).all()


@functools.lru_cache(maxsize=None)
def surface_case():
    """match_restated.surface(600) on the grid, its normals (the device's, estimated near the origin) oriented alike, and the
    near-origin run of register_features."""
    import vcrnet_amd
    c = fc.gridded(mr.surface(600))
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    ns, nt = (dev(mr.orient(host(vcrnet_amd.estimate_normals(x, 20)[0]), up)[None]) for x, up in zip((src, tgt), mr.surface_up(c)))
    kw = dict(k=20, trials=4096, seed=mr.SEED, refine=mr.MAX_DIST, src_normals=ns, tgt_normals=nt)
    near = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, **kw)
    return c, kw, near


def _moved_pose(t_near, R, c_s, c_t):
    """The near-origin pose between clouds moved by c_s and c_t: t - R c_s + c_t in float64."""
    return t_near.astype(F64) - R.astype(F64) @ np.asarray(c_s, F64) + np.asarray(c_t, F64)


def test_register_features_with_given_centres_returns_the_near_origin_run():
    """The source moved by one far offset, the target by the other, centre=(c_s, c_t): corr, best_trial and R (the RANSAC's and
    the refined) are the near-origin run's bits; every t is the near-origin one carried over, within 2 fp32 ulp at |c|; the
    scores are score_registration's on the caller's clouds."""
    import vcrnet_amd
    c, kw, near = surface_case()
    o_s, o_t = fc.FAR_OFFSETS[1], fc.FAR_OFFSETS[0]
    assert fc.is_exact(c["src"], o_s) and fc.is_exact(c["tgt"], o_t)
    src, tgt = dev(fc.moved_cloud(c["src"], o_s)[None]), dev(fc.moved_cloud(c["tgt"], o_t)[None])
    far = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, centre=(dev(np.asarray([o_s], F32)), dev(np.asarray([o_t], F32))), **kw)
    assert sorted(far) == sorted(near) and sorted(far["refined"]) == sorted(near["refined"])
    for key in ("corr", "best_trial", "pairs", "ransac_inliers", "R"):
        assert torch.equal(far[key].view(torch.int32), near[key].view(torch.int32)), key
    for key in ("R", "R_ba", "iterations", "converged"):
        assert torch.equal(far["refined"][key].view(torch.int32), near["refined"][key].view(torch.int32)), key
    ulp = float(np.spacing(F32(1024)))
    for what, a, b in (("ransac", near, far), ("refined", near["refined"], far["refined"])):
        gap = np.abs(host(b["t"])[0] - _moved_pose(host(a["t"])[0], host(a["R"])[0], o_s, o_t)).max()
        _emit(f"far register_features given centres, {what}: |t - carried t_near| {gap:.2e} (2 ulp {2 * ulp:.2e}) fitness near "
              f"{float(a['fitness'][0]):.4f} far {float(b['fitness'][0]):.4f}")
        assert gap <= 2 * ulp
        sc = vcrnet_amd.score_registration(src, tgt, b["R"], b["t"], mr.MAX_DIST)
        for key in ("fitness", "inlier_rmse", "inliers"):
            assert torch.equal(b[key], sc[key]), (what, key)


def test_register_features_with_centre_true_far_from_the_origin():
    """Both clouds at (1024, -512, 256 + 5 2^-12), centres of their own: the fitness is the near-origin run's within
    match_restated.SHARE_SLACK, for the RANSAC and for FGR."""
    import vcrnet_amd
    c, kw, near = surface_case()
    o = fc.FAR_OFFSETS[1]
    f = fc.translated(c, o)
    src, tgt = dev(f["src"][None]), dev(f["tgt"][None])
    for method in ("ransac", "fgr"):
        extra = dict(kw, method=method)
        if method == "fgr":
            extra = {k: v for k, v in extra.items() if k not in ("trials", "seed")}
            base = vcrnet_amd.register_features(dev(c["src"][None]), dev(c["tgt"][None]), mr.MAX_DIST, **extra)
        else:
            base = near
        far = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, centre=True, **extra)
        e = fc.at_cloud_error(host(far["refined"]["R"])[0], host(far["refined"]["t"])[0], f["R"], f["t"], f["src"])
        _emit(f"far register_features centre=True {method} offset 1024: fitness {float(far['fitness'][0]):.4f} (near {float(base['fitness'][0]):.4f}) "
              f"refined fitness {float(far['refined']['fitness'][0]):.4f} (near {float(base['refined']['fitness'][0]):.4f}) at-cloud error {e:.2e}")
        assert float(far["fitness"][0]) >= float(base["fitness"][0]) - mr.SHARE_SLACK
        assert float(far["refined"]["fitness"][0]) >= float(base["refined"]["fitness"][0]) - mr.SHARE_SLACK
        sc = vcrnet_amd.score_registration(src, tgt, far["R"], far["t"], mr.MAX_DIST)
        assert torch.equal(far["fitness"], sc["fitness"]) and torch.equal(far["inliers"], sc["inliers"])
