"""vcr_orient_tangent_f32 and orient_normals_consistent_tangent_plane on the device, and
register_features(orient="tangent").

Every comparison is bit-equal on oriented, flip, ref and n_trees with the numpy restatement of the DEFINITION
(tests/orient_restated.py: Kruskal's algorithm on the sorted keys and a walk from every reference point), fed the normals and the
neighbour rows the device itself was given or computed.  Every raw call runs with its outputs and its workspace prefilled with
the byte 0xA5 and 64 elements of guard behind the outputs, in the plan's form and in every built one."""
import functools

import numpy as np
import pytest
import torch

import match_restated as mr
import orient_restated as ot

pytestmark = pytest.mark.gpu

GUARD = 64
BYTE = 0xA5
F32 = np.float32
KEYS = ("oriented", "flip", "ref", "n_trees")


def mods():
    import vcrnet_amd
    from vcrnet_amd import orient
    return vcrnet_amd, orient


def dev(x):
    return torch.tensor(np.array(x)).cuda()                  # (a copy: the cached cases are read-only)


def checked(out, raw, name):
    """The output as numpy; nothing behind it was written and no element of it was left as prefilled."""
    buf, n = raw[name], out.numel()
    size = buf.element_size()
    band = buf[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * size and (band == BYTE).all(), (name, "guard band written")
    body = buf[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
    assert not (body == BYTE).all(axis=1).any(), (name, "element left unwritten")
    return out.cpu().numpy()


def run(xyz, nrm, idx, variant=0):
    """The raw call on device tensors [B, ...] with everything asked for -> dict of numpy [B, ...]."""
    _, orient = mods()
    o = orient.orient_tangent(xyz, nrm, idx, want_flip=True, want_ref=True, want_trees=True, variant=variant, guard=GUARD,
                              prefill=BYTE)
    torch.cuda.synchronize()
    return {k: checked(o[k], o["_raw"], k) for k in KEYS}


def forms():
    _, orient = mods()
    return (0,) + tuple(orient.BUILT)


def compare(got, b, xyz, nrm, idx, name):
    """Cloud b of a device result against the definition on the same inputs (numpy, one cloud)."""
    want = ot.definition(xyz, nrm, idx)
    assert got["n_trees"][b] == want["n_trees"], (name, got["n_trees"][b], want["n_trees"])
    assert np.array_equal(got["ref"][b], want["ref"]), name
    assert np.array_equal(got["flip"][b], want["flip"]), name
    assert np.array_equal(got["oriented"][b].view(np.uint32), want["oriented"].view(np.uint32)), name
    return want


def run_and_compare(xyz, nrm, idx, name):
    """One cloud (numpy) in every form."""
    for v in forms():
        got = run(dev(xyz[None]), dev(nrm[None]), dev(idx[None]), v)
        want = compare(got, 0, xyz, nrm, idx, (name, v))
    return want


@functools.lru_cache(maxsize=None)
def recipes():
    return ot.small_recipes()


# ------------------------------------------------------------------------------------------------------------ the raw call

@pytest.mark.parametrize("name", sorted(ot.small_recipes()))
def test_the_small_recipes_are_the_definition_bit_for_bit(name):
    """N = 1, N = 2 with k = 1, N = 65 with k = 3 (crosses a wave), rows with self entries, out-of-range entries and duplicates,
    an edge listed only by its far end, all weights tied, two and five blobs, equal z at the top (also as -0.0 and 0.0), NaN,
    infinite and zero normals, non-finite z."""
    x, nrm, idx = recipes()[name]
    want = run_and_compare(x, nrm, idx, name)
    if name.startswith("blobs"):
        assert want["n_trees"] == int(name.split("-")[1])
    if name == "far-end":
        assert want["n_trees"] == 1


def test_a_batch_is_its_clouds_alone():
    """B = 3 clouds of different content (one of them two trees): the same bits as each cloud alone, in every form."""
    clouds = [ot.random_rows(300, 5, seed=s) for s in (0, 1)]
    x, nrm, idx = ot.random_rows(300, 5, seed=2)
    idx = idx.copy()
    idx[:150][(idx[:150] >= 150)] = -1                      # two halves that do not name each other
    idx[150:][(idx[150:] < 150)] = -1
    clouds.append((x, nrm, idx))
    X, Nn, I = (np.stack([c[j] for c in clouds]) for j in range(3))
    for v in forms():
        got = run(dev(X), dev(Nn), dev(I), v)
        for b, (x, nrm, idx) in enumerate(clouds):
            compare(got, b, x, nrm, idx, ("batch", b, v))
            alone = run(dev(x[None]), dev(nrm[None]), dev(idx[None]), v)
            for k in KEYS:
                assert np.array_equal(np.ascontiguousarray(alone[k][0]).view(np.uint8), np.ascontiguousarray(got[k][b]).view(np.uint8)), (k, b, v)
    assert got["n_trees"][2] >= 2


@pytest.mark.parametrize("scrambled", [False, True])
def test_all_weights_tied_on_a_path_of_4096(scrambled):
    """All normals equal: the order is (lo, hi) alone.  In index order every vertex hooks under its predecessor in round one
    -- a chain of depth N - 1 for the flatten --, scrambled the rounds are Boruvka's usual few."""
    x, nrm, idx = ot.path(4096, scrambled)
    want = run_and_compare(x, nrm, idx, ("path", scrambled))
    assert want["n_trees"] == 1 and want["flip"].all()


def test_the_in_order_path_at_the_largest_cloud():
    """N = 131 072 in index order: the flatten's worst case at the size limit (a plain walk up the chain would take
    N^2 / 2 = 8.6e9 dependent loads)."""
    x, nrm, idx = ot.path(ot.MAX_N)
    got = run(dev(x[None]), dev(nrm[None]), dev(idx[None]))
    want = compare(got, 0, x, nrm, idx, "path-131072")
    assert want["n_trees"] == 1 and (want["ref"] == ot.MAX_N - 1).all()


def test_a_random_surface_of_20000_points():
    """The device's own normals (estimate_normals on the grid search) and rows (search_knn, k = 12) on the test surface's
    function at N = 20 000; the public call with idx=None is the raw call on search_knn's rows."""
    vcrnet_amd, _ = mods()
    N, k = 20000, 12
    x = dev(mr.surface(N)["tgt"][None])
    nrm = vcrnet_amd.estimate_normals(x, k, search="grid")
    idx = vcrnet_amd.search_knn(x, k)
    got = run(x, nrm, idx)
    want = compare(got, 0, x[0].cpu().numpy(), nrm[0].cpu().numpy(), idx[0].cpu().numpy(), "surface-20000")
    print("surface 20000: trees", want["n_trees"], "flipped", int(want["flip"].sum()))
    o, flip, ref, trees = vcrnet_amd.orient_normals_consistent_tangent_plane(x, nrm, k=k, want_flip=True, want_ref=True, want_trees=True)
    assert np.array_equal(o.cpu().numpy().view(np.uint32), got["oriented"].view(np.uint32))
    assert np.array_equal(flip.cpu().numpy(), got["flip"]) and np.array_equal(ref.cpu().numpy(), got["ref"])
    assert np.array_equal(trees.cpu().numpy(), got["n_trees"])
    only = vcrnet_amd.orient_normals_consistent_tangent_plane(x, nrm, idx=idx)
    assert torch.is_tensor(only) and torch.equal(only.view(torch.int32), o.view(torch.int32))
    # on this surface the top point looks up and so does everything else: the sensor's orientation, exactly
    assert want["n_trees"] == 1 and (got["oriented"][0, 2] > 0).all()


def test_the_public_call_at_its_edges():
    """N = 1 needs no search; k is cut to N - 1; the one-launch form is not built and says so."""
    vcrnet_amd, orient = mods()
    x, nrm = dev(np.asarray([[[1], [2], [3]]], F32)), dev(np.asarray([[[0], [0], [-1]]], F32))
    o, flip, ref, trees = vcrnet_amd.orient_normals_consistent_tangent_plane(x, nrm, want_flip=True, want_ref=True, want_trees=True)
    assert o.cpu().tolist() == [[[0.0], [0.0], [1.0]]] and flip.tolist() == [[1]] and ref.tolist() == [[0]] and trees.tolist() == [1]
    c, _ = ot.sphere(9)
    x = dev(c[None])
    nrm = vcrnet_amd.estimate_normals(x, 5)
    a = vcrnet_amd.orient_normals_consistent_tangent_plane(x, nrm, k=12)
    b = vcrnet_amd.orient_normals_consistent_tangent_plane(x, nrm, idx=vcrnet_amd.search_knn(x, 8))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(orient.VcrHipError, match="rc=-3"):
        orient.orient_tangent(x, nrm, vcrnet_amd.search_knn(x, 8), variant="one_launch")


# ------------------------------------------------------------------------------------------------------------------ end to end

def end_to_end(c, up_src, k, method):
    """register_features(orient="tangent") on the surface case c against the steps called one by one -> the result."""
    vcrnet_amd, _ = mods()
    N = c["src"].shape[1]
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    T = 4096
    kw = dict(trials=T, seed=mr.SEED) if method == "ransac" else dict(method="fgr")
    res = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, k=k, mutual=False, refine=mr.MAX_DIST, orient="tangent", **kw)
    # the steps, one by one
    est = [vcrnet_amd.estimate_normals(x, k) for x in (src, tgt)]
    ns, nt = (vcrnet_amd.orient_normals_consistent_tangent_plane(x, n, k=12) for x, n in zip((src, tgt), est))
    ft = vcrnet_amd.compute_fpfh_feature(tgt, nt, k=k)
    runs = []
    for n in (ns, -ns):
        corr = vcrnet_amd.match_features(vcrnet_amd.compute_fpfh_feature(src, n, k=k), ft, mutual=False)
        if method == "ransac":
            r = vcrnet_amd.ransac_correspondences(src, tgt, corr, mr.MAX_DIST, T, seed=mr.SEED)
            r = dict(R=r["R"], t=r["t"], best_trial=r["best_trial"], pairs=r["pairs"], ransac_inliers=r["inliers"])
        else:
            r = vcrnet_amd.fast_global_registration(src, tgt, corr)
            r = {key: r[key] for key in ("R", "t", "pairs", "tuples", "used", "status")}
        r.update(vcrnet_amd.score_registration(src, tgt, r["R"], r["t"], mr.MAX_DIST), corr=corr)
        runs.append(r)
    f, e = [float(r["fitness"][0]) for r in runs], [float(r["inlier_rmse"][0]) for r in runs]
    flipped = f[1] > f[0] or (f[1] == f[0] and e[1] < e[0])  # the higher fitness, then the lower rmse, then the first
    for i, r in enumerate(runs):
        got = r["corr"][0].cpu().numpy()
        print(f"  run {i}: fitness {float(r['fitness'][0]):.6f} rmse {float(r['inlier_rmse'][0]):.3e} share {float((got == c['twin']).mean()):.4f} "
              + (f"ransac inliers {int(r['ransac_inliers'][0])}" if method == "ransac" else f"tuples {int(r['tuples'][0])}"))
    kept = runs[int(flipped)]
    assert res["flipped"].dtype == torch.bool and res["flipped"].tolist() == [flipped]
    assert set(res) == set(kept) | {"flipped", "refined"}
    for key, want in kept.items():
        assert torch.equal(res[key].view(torch.int32) if res[key].dtype == torch.float32 else res[key],
                           want.view(torch.int32) if want.dtype == torch.float32 else want), key
    rf = vcrnet_amd.refine_registration(src, tgt, kept["R"], kept["t"], mr.MAX_DIST)
    assert set(res["refined"]) == set(rf)
    for key in rf:
        assert torch.equal(res["refined"][key].view(torch.int32), rf[key].view(torch.int32)), key
    # which run is the right one: the one in which the two clouds' normals look alike -- both towards the sensor or both away
    toward = []
    for n, e, up in zip((ns, nt), est, (up_src, mr.surface_up(c)[1])):
        share = float(((n[0].cpu().numpy().astype(np.float64) * mr.orient(e[0].cpu().numpy(), up)).sum(0) > 0).mean())
        assert share in (0.0, 1.0), share                   # one global sign is all that is left
        toward.append(share == 1.0)
    assert flipped == (toward[0] != toward[1])
    corr = res["corr"][0].cpu().numpy()
    paired = corr >= 0
    correct = int((corr[paired] == c["twin"][paired]).sum())
    share = correct / max(1, int(paired.sum()))
    fit = float(res["fitness"][0])
    Rr, tr = res["refined"]["R"][0].cpu().numpy().astype(np.float64), res["refined"]["t"][0].cpu().numpy().astype(np.float64)
    dR, dt = np.abs(Rr - c["R"]).max(), np.abs(tr - c["t"]).max()
    print(f"register_features orient=tangent {method} N {N} k {k}: flipped {flipped}, fitness of the two runs "
          f"{float(runs[0]['fitness'][0]):.4f} / {float(runs[1]['fitness'][0]):.4f}, {correct} of {int(paired.sum())} pairs correct "
          f"({share:.4f}; CPU oriented {mr.SURFACE_SHARES[(N, k, True, False)]}), fitness {fit:.4f}, refined |dR| {dR:.2e} |dt| {dt:.2e}")
    assert paired.all()
    assert share >= mr.SURFACE_SHARES[(N, k, True, False)] - mr.SHARE_SLACK
    if method == "ransac":                                  # what tests/test_hip_match.py asks of its oriented-normals case
        assert int(res["pairs"][0]) == int(paired.sum()) and int(res["ransac_inliers"][0]) >= correct
    assert fit >= F32(correct) / F32(N)
    assert dR <= 1e-5 and dt <= 1e-5, (dR, dt)
    return res


def upside_down(c):
    """The surface case with its source turned by 180 degrees about x: (case, the source's `towards the sensor`)."""
    D = np.diag([1.0, -1.0, -1.0])
    d = dict(c, src=np.ascontiguousarray((c["src"] * np.asarray([[1], [-1], [-1]], F32)).astype(F32)), R=c["R"] @ D)
    return d, D @ mr.surface_up(c)[0]


@pytest.mark.parametrize("method", ["ransac", "fgr"])
def test_register_features_with_tangent_orientation_on_the_surface(method):
    """surface(600) at k = 20 with nothing but the points: the one-way share of correct matches reaches the CPU chain's with
    oriented normals (0.997 against 0.183 with estimated ones), the RANSAC's inliers and the closing fitness reach what the
    oriented-normals case of tests/test_hip_match.py requires, the refinement recovers the pose, and the call is the composition
    of its steps bit for bit -- the second run included.  With the source turned upside down its top point is another one and
    its normals come out opposite: `flipped` says so, and the same bounds hold."""
    c = mr.surface(600)
    res = end_to_end(c, mr.surface_up(c)[0], 20, method)
    d, up = upside_down(c)
    turned = end_to_end(d, up, 20, method)
    assert res["flipped"].tolist() == [False] and turned["flipped"].tolist() == [True]


def test_register_features_orients_only_what_it_estimated():
    """Given normals are used as they are: with both given nothing is oriented, one chain runs and flipped is False -- the
    result is orient=None's; with one side given the chain runs twice.  The centred call carries the keyword through."""
    vcrnet_amd, _ = mods()
    c = mr.surface(600)
    k = 20
    src, tgt = dev(c["src"][None]), dev(c["tgt"][None])
    ups = mr.surface_up(c)
    ns, nt = (dev(mr.orient(vcrnet_amd.estimate_normals(x, k)[0].cpu().numpy(), up)[None]) for x, up in zip((src, tgt), ups))
    kw = dict(k=k, mutual=False, trials=4096, seed=mr.SEED)
    plain = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, src_normals=ns, tgt_normals=nt, **kw)
    both = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, src_normals=ns, tgt_normals=nt, orient="tangent", **kw)
    assert set(both) == set(plain) | {"flipped"} and both["flipped"].tolist() == [False]
    for key in plain:
        assert torch.equal(both[key], plain[key]), key
    # the source's given normals look AWAY from the sensor: the target's, estimated and oriented, look up -- the second run wins
    one = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, src_normals=-ns, orient="tangent", **kw)
    assert one["flipped"].tolist() == [True]
    for key in plain:                                       # (the tangent orientation of the target IS the sensor's here)
        assert torch.equal(one[key], plain[key]), key
    cen = vcrnet_amd.register_features(src, tgt, mr.MAX_DIST, orient="tangent", centre=True, **kw)
    corr = cen["corr"][0].cpu().numpy()
    assert cen["flipped"].tolist() == [False]
    assert float((corr == c["twin"]).mean()) >= mr.SURFACE_SHARES[(600, k, True, False)] - mr.SHARE_SLACK
