"""vcr_plane_ransac_f32, vcr_plane_split_f32, ``segment_plane``, ``split_by_plane`` and ``segment_planes`` on the GPU
(include/segment/vcr_hip_segment.h).

Every comparison with the numpy restatement (tests/segment_restated.py) is bit-equal -- the trials' status, picks, planes and
counts, the winner, the inlier flags, the refit's nine sums, the point -- except the refit's normal, which the same Jacobi as
the normals' computes and which is held the way tests/test_hip_normals.py holds normals against numpy.linalg.eigh on the same
sums: | |n| - 1 | <= 2^-22, the Rayleigh quotient within 2^-40 lambda2 of lambda0, and max |n - n_ref| <= 2^-22 where
lambda1 - lambda0 >= 2^-10 lambda2; d is then the header's function of the device's own normal, bit for bit.  Every raw call
runs with its outputs and its workspace prefilled with the byte 0xA5 and 64 elements of guard behind the outputs."""
import functools

import numpy as np
import pytest
import torch

import segment_restated as sr

pytestmark = pytest.mark.gpu

BYTE = 0xA5
GUARD = 64
TRIAL_KEYS = ("trial_status", "trial_picks", "trial_plane", "trial_count")
KEYS = ("plane", "inlier", "count", "point", "best_trial", "candidates", "refit_sums")
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
TRIALS = (1, 63, 64, 65, 256, 257, 1000)
THR, SEED = 0.02, 11


def mods():
    import vcrnet_amd
    from vcrnet_amd import segment
    return vcrnet_amd, segment


def dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def checked(out, raw, name):
    """The output as numpy; all of it must have been overwritten, none of the band behind it."""
    buf, n = raw[name], out.numel()
    size = buf.element_size()
    band = buf[n:].view(torch.uint8).cpu().numpy()
    assert band.size == GUARD * size and (band == BYTE).all(), (name, "guard band written")
    body = buf[:n].view(torch.uint8).cpu().numpy().reshape(n, size)
    assert not (body == BYTE).all(axis=1).any(), (name, "element left unwritten")
    return out.cpu().numpy()


def run(x, thr=THR, T=256, seed=SEED, mask=None, variant=0, trials=True, prefill=BYTE):
    """The raw call on x [B,3,N] numpy with everything asked for -> dict of numpy [B, ...]."""
    _, segment = mods()
    guard = GUARD if prefill is not None else 0
    o = segment.plane_ransac(dev(x), thr, 3, T, seed, dev(mask), want_trials=trials, variant=variant, guard=guard, prefill=prefill)
    torch.cuda.synchronize()
    keys = KEYS + (TRIAL_KEYS if trials else ())
    if prefill != BYTE:                                     # (another filling: the bands are checked under BYTE)
        return {k: o[k].cpu().numpy() for k in keys}
    return {k: checked(o[k], o["_raw"], k) for k in keys}


def same_bits(a, b, what, keys=None):
    for k in keys or a:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, int((bits(a[k]) != bits(b[k])).sum()))


def normal_held(n, want, what):
    """The device's fp32 normal against numpy.linalg.eigh on the restated sums: tests/test_hip_normals.py's three allowances."""
    m, C = sr.covariance(want["sums"], want["best_count"])
    lam = want["lam"]
    nd = n.astype(np.float64)
    norm = abs(np.sqrt(nd @ nd) - 1)
    rq = nd @ C @ nd / (nd @ nd) - lam[0]
    apart = lam[1] - lam[0] >= 2.0 ** -10 * lam[2]
    dn = np.abs(n - want["normal"]).max()
    print(what, f"||n|-1| {norm:.2e}  (rq - l0) / l2 {rq / lam[2]:.2e}  |n - n_ref| {dn:.2e} apart {apart}")
    assert norm <= 2.0 ** -22, what
    assert rq <= 2.0 ** -40 * lam[2], (what, rq / lam[2])
    if apart:
        assert dn <= 2.0 ** -22, (what, dn)


def agree(got, b, want, x, what):
    """Cloud b of a device result against the restatement's finished dict."""
    T = len(want["status"])
    assert np.array_equal(got["trial_status"][b], want["status"]), (what, "status")
    assert np.array_equal(got["trial_picks"][b], want["picks"]), (what, "picks")
    assert np.array_equal(bits(got["trial_plane"][b]), bits(want["plane"])), (what, "trial_plane")
    assert np.array_equal(got["trial_count"][b], want["count"]), (what, "count", T)
    assert got["candidates"][b] == want["M"] and got["best_trial"][b] == want["best_trial"], (what, "best_trial")
    assert got["count"][b] == want["best_count"] and np.array_equal(got["inlier"][b], want["inlier"]), (what, "inlier")
    assert np.array_equal(bits(got["refit_sums"][b]), bits(want["sums"])), (what, "sums")
    assert np.array_equal(bits(got["point"][b]), bits(want["point"])), (what, "point")
    if want["best_trial"] < 0:
        assert np.isnan(got["plane"][b]).all(), (what, "plane")
        return
    n = got["plane"][b][:3]
    if want["normal"] is None:                              # the trial's own plane
        assert np.array_equal(bits(got["plane"][b]), bits(want["fit"])), (what, "fallback")
    else:
        normal_held(n, want, what)
        t = got["trial_plane"][b][want["best_trial"]][:3]
        assert n.astype(np.float64) @ t.astype(np.float64) >= 0, (what, "sign")
        plane, _ = sr.outputs(got["trial_plane"][b][want["best_trial"]], want["sums"], want["best_count"], n)
        assert np.array_equal(bits(got["plane"][b]), bits(plane)), (what, "d")


@functools.lru_cache(maxsize=None)
def restated(N, b, T=max(TRIALS)):
    """Cloud b of size N with all TRIALS' trials, computed once and read-only: a trial does not depend on the trial count."""
    x = sr.cloud(N, seed=b)
    o = sr.trials_vector(x, THR, T, SEED)
    x.setflags(write=False)
    return x, o


# ------------------------------------------------------------------------------------------------------------------- parity

@pytest.mark.parametrize("N", SIZES)
def test_parity_with_the_restatement(N):
    """N x every T of TRIALS x B in {1, 3}, the plan's form: every per-trial array, the winner, the flags, the sums and the
    outputs."""
    clouds = [restated(N, b) for b in range(3)]
    seen = set()
    for B in (1, 3):
        x = np.stack([c[0] for c in clouds[:B]])
        for T in TRIALS:
            got = run(x, T=T)
            for b in range(B):
                want = sr.finish(clouds[b][0], THR, sr.head(clouds[b][1], T))
                agree(got, b, want, clouds[b][0], (N, T, B, b))
                seen |= set(want["status"].tolist())
    assert 1 in seen and (N < 3 or 0 in seen)


@pytest.mark.parametrize("B,N,T", [(3, 1000, 257), (1, 5000, 300), (2, 9000, 70)])
def test_both_forms_and_every_split_return_the_same_bits(B, N, T):
    """The TRIAL and the POINT form with 1, 2, 3 and 7 splits, the forms with the plan's splits, and the plan: one result.
    (9 000 points a cloud: the plan itself takes the POINT form there, and a POINT workgroup walks several tiles of 1 024.)"""
    x = np.stack([sr.cloud(N, seed=b) for b in range(B)])
    mask = (np.random.RandomState(N).uniform(size=(B, N)) < 0.9).astype(np.int32)
    ref = run(x, T=T, mask=mask)
    want = sr.segment_plane(x[0], THR, T, SEED, mask[0])
    agree(ref, 0, want, x[0], (B, N, T))
    for form in ("trial", "point"):
        for splits in (0, 1, 2, 3, 7):
            same_bits(ref, run(x, T=T, mask=mask, variant=(form, splits)), (form, splits))
    assert (ref["trial_count"].max(1) > 3).all()


def test_a_cloud_in_a_batch_is_the_cloud_alone():
    N, T = 777, 300
    x = np.stack([sr.cloud(N, seed=b) for b in range(3)])
    x[1, 0, 5] = np.nan
    mask = (np.random.RandomState(3).uniform(size=(3, N)) < 0.8).astype(np.int32)
    batch = run(x, T=T, mask=mask)
    for b in range(3):
        alone = run(x[b:b + 1], T=T, mask=mask[b:b + 1])
        same_bits({k: v[b:b + 1] for k, v in batch.items()}, alone, b)


# ------------------------------------------------------------------------------------------------------------------ the refit

def test_the_refit_on_a_slab_and_its_fallback():
    """A thick slab (the refit has something to do: the normal moves away from the trial's), the sign rule, and count < 3
    (threshold 0 on a cloud in general position: the winner counts its own p0 and little else), which returns the trial's own
    plane and p0."""
    c = sr.planted(3000, 0.7, 0.05, seed=4)
    got = run(c["x"][None], thr=0.05, T=200)
    want = sr.segment_plane(c["x"], 0.05, 200, SEED)
    agree(got, 0, want, c["x"], "slab")
    trial = got["trial_plane"][0][want["best_trial"]][:3]
    n = got["plane"][0][:3]
    assert want["normal"] is not None and not np.array_equal(bits(n), bits(trial))
    assert sr.angle(n, c["normal"]) < sr.angle(trial, c["normal"])             # the least-squares plane is the better one
    assert n.astype(np.float64) @ trial.astype(np.float64) > 0
    # the mirrored cloud: the same plane, and the sign still follows the trial's normal
    flipped = (c["x"] * np.asarray([[1], [1], [-1]], np.float32)).astype(np.float32)
    g2 = run(flipped[None], thr=0.05, T=200)
    assert g2["best_trial"][0] == got["best_trial"][0] and g2["count"][0] == got["count"][0]
    t2 = g2["trial_plane"][0][g2["best_trial"][0]][:3]
    assert g2["plane"][0][:3].astype(np.float64) @ t2.astype(np.float64) > 0
    # threshold 0
    x = sr.cloud(400, seed=9)
    got = run(x[None], thr=0.0, T=64)
    want = sr.segment_plane(x, 0.0, 64, SEED)
    agree(got, 0, want, x, "threshold 0")
    assert 1 <= want["best_count"] < 3 and want["normal"] is None
    row = got["trial_plane"][0][want["best_trial"]]
    assert np.array_equal(bits(got["plane"][0][:3]), bits(row[:3])) and np.array_equal(bits(got["point"][0]), bits(row[4:7]))


# ------------------------------------------------------------------------------------------------------------------ the edges

def test_nonfinite_points_and_masked_points_are_neither_drawn_nor_counted():
    N, T = 600, 257
    rs = np.random.RandomState(8)
    x = np.stack([sr.cloud(N, seed=b) for b in range(2)])
    bad = rs.permutation(N)[:90]
    x[0, rs.randint(0, 3, 90), bad] = np.asarray([np.nan, np.inf, -np.inf] * 30, np.float32)
    mask = np.ones((2, N), np.int32)
    gone = rs.permutation(N)[:200]
    mask[1, gone] = 0
    got = run(x, T=T, mask=mask)
    for b in range(2):
        agree(got, b, sr.segment_plane(x[b], THR, T, SEED, mask[b]), x[b], ("excluded", b))
    assert not np.isin(got["trial_picks"][0], bad).any() and not got["inlier"][0][bad].any() and got["candidates"][0] == N - 90
    assert not np.isin(got["trial_picks"][1], gone).any() and not got["inlier"][1][gone].any() and got["candidates"][1] == N - 200
    # any mask value other than 0 admits a point
    other = mask.copy()
    other[other != 0] = -7
    same_bits(got, run(x, T=T, mask=other), "mask values")


def test_clouds_without_a_plane():
    """M < 3 (by size, by mask, by NaN), a cloud on a line and a cloud of copies of one point: best_trial -1, NaN plane and
    point, no inlier, count 0; bitwise copies of one point among the picks are status 2."""
    N, T = 70, 65
    line = np.arange(N, dtype=np.float32) / 64
    x = np.stack([sr.cloud(N, 1), np.stack([line, 2 * line, -line]), np.repeat(sr.cloud(1, 2), N, axis=1), sr.cloud(N, 3),
                  np.repeat(sr.cloud(7, 5), 10, axis=1)])
    mask = np.ones((5, N), np.int32)
    mask[0, 2:] = 0                                         # two candidates
    x[3, :, 1:] = np.nan                                    # one
    got = run(x, T=T, mask=mask)
    for b in range(5):
        agree(got, b, sr.segment_plane(x[b], THR, T, SEED, mask[b]), x[b], ("no plane", b))
    assert (got["best_trial"][:4] == -1).all() and np.isnan(got["plane"][:4]).all() and np.isnan(got["point"][:4]).all()
    assert not got["inlier"][:4].any() and not got["count"][:4].any() and not got["refit_sums"][:4].any()
    assert (got["trial_status"][[0, 3]] == 1).all() and set(got["trial_status"][1].tolist()) <= {1, 2}
    assert (got["trial_count"][:4] == -1).all() and not got["trial_plane"][:4].any()
    assert got["candidates"].tolist() == [2, N, N, 1, N]
    assert got["best_trial"][4] >= 0 and 2 in got["trial_status"][4]            # copies among the picks: collinear
    picks = got["trial_picks"][4][got["trial_status"][4] == 2]
    by_index, by_point = np.sort(picks, 1), np.sort(picks // 10, 1)                     # different indices, the same point
    assert (np.diff(by_index, axis=1) > 0).all() and (np.diff(by_point, axis=1) == 0).any(1).all()
    for N1 in (1, 2):
        g = run(sr.cloud(N1)[None], T=9)
        assert g["best_trial"][0] == -1 and (g["trial_status"] == 1).all() and (g["trial_picks"] >= 0).all()
    g = run(np.full((1, 3, 4), np.nan, np.float32), T=9)
    assert g["candidates"][0] == 0 and (g["trial_picks"] == -1).all() and g["best_trial"][0] == -1


def test_ties_between_trials_go_to_the_lower_trial():
    """Every point on one lattice plane: z = 0.5 x at a threshold above the rounding of n32, and z = 0.25, where n32 is
    (0, 0, +-1) and every distance exactly 0, at threshold 0.  Every valid trial counts all N, and the winner is the first."""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(15)), 0).reshape(2, -1).astype(np.float32) / 32
    N = g.shape[1]
    for x, thr in ((np.stack([g[0], g[1], 0.5 * g[0]]), 0.01), (np.stack([g[0], g[1], np.full(N, 0.25)]), 0.0)):
        x = x.astype(np.float32)
        got = run(x[None], thr=thr, T=100)
        valid = np.nonzero(got["trial_status"][0] == 0)[0]
        assert len(valid) > 50 and (got["trial_count"][0][valid] == N).all()
        assert got["best_trial"][0] == valid[0] and got["count"][0] == N and got["inlier"][0].all()
        agree(got, 0, sr.segment_plane(x, thr, 100, SEED), x, ("ties", thr))
    # a tie among fewer: the first of the trials with the highest count, whatever it is
    x = sr.cloud(300, 4)
    got = run(x[None], T=1000)
    top = np.nonzero(got["trial_count"][0] == got["trial_count"][0].max())[0]
    assert got["best_trial"][0] == top[0]


def test_the_workspace_contents_have_no_influence():
    x = np.stack([sr.cloud(900, seed=b) for b in range(2)])
    ref = run(x, T=130)
    same_bits(ref, run(x, T=130, prefill=0x00), "prefill 0")
    same_bits(ref, run(x, T=130, prefill=0xFF), "prefill ff")
    same_bits(ref, run(x, T=130, prefill=None), "no prefill")
    short = run(x, T=130, trials=False)                      # the per-trial arrays in the workspace
    same_bits({k: ref[k] for k in KEYS}, short, "trials in the workspace")
    vcrnet_amd, _ = mods()
    plane, inlier, count = vcrnet_amd.segment_plane(dev(x), THR, num_iterations=130, seed=SEED)
    same_bits({"plane": ref["plane"], "inlier": ref["inlier"], "count": ref["count"]},
              {"plane": plane.cpu().numpy(), "inlier": inlier.cpu().numpy(), "count": count.cpu().numpy()}, "segment_plane")


def test_far_from_the_origin():
    """Coordinates on a 2^-10 grid, moved by 512 along every axis: the move is exact in fp32 and so is every difference, so
    the trials, the winner, the flags, the sums and the normal are the same bits; the point moves by 512 and d by -512 (n.x +
    n.y + n.z), each within an ulp of its own size."""
    x = (np.round(sr.cloud(2000, 6) * 1024) / 1024).astype(np.float32)
    far = (x + np.float32(512)).astype(np.float32)
    assert np.array_equal((far - np.float32(512)).astype(np.float32), x)
    a, b = run(x[None], T=300), run(far[None], T=300)
    same_bits(a, b, "moved", ("inlier", "count", "best_trial", "refit_sums", "trial_status", "trial_picks", "trial_count"))
    assert np.array_equal(bits(a["plane"][0][:3]), bits(b["plane"][0][:3])) and a["count"][0] > 100
    assert np.array_equal(bits(a["trial_plane"][..., :4]), bits(b["trial_plane"][..., :4]))
    assert np.abs(b["point"][0].astype(np.float64) - (a["point"][0].astype(np.float64) + 512)).max() <= 2.0 ** -14
    n = a["plane"][0][:3].astype(np.float64)
    assert abs(b["plane"][0][3] - (a["plane"][0][3] - 512 * n.sum())) <= 2.0 ** -14
    agree(b, 0, sr.segment_plane(far, THR, 300, SEED), far, "far")


# -------------------------------------------------------------------------------------------------------------------- at size

def torch_fma32(a, b, c):
    """match_restated.fma32 on the device: the exact product and TwoSum in float64, the one rounding to fp32 last."""
    p, cd = a.double() * b.double(), c.double()
    s0 = p + cd
    bb = s0 - p
    err = (p - (s0 - bb)) + (cd - bb)
    halfway = (s0.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
    fix = halfway & torch.isfinite(s0) & torch.isfinite(err) & (err != 0)
    inf = torch.full_like(s0, float("inf"))
    return torch.where(fix, torch.nextafter(s0, torch.where(err > 0, inf, -inf)), s0).float()


def test_a_planted_plane_at_size():
    """One cloud of 131 072 points, T = 256: every trial's count equals a chunked torch count from the device's own
    trial_plane rows (the header's distance, fmaf restated exactly), the flags are the winner's, and the planted normal comes
    back within the angle the restatement reaches at N = 2 000 plus tests/test_segment_cpu.py's bound."""
    _, segment = mods()
    P = sr.PLANTED
    N, T = 131072, P["T"]
    c = sr.planted(N, P["share"], P["thr"], P["seed"])
    xyz = dev(c["x"][None])
    o = segment.plane_ransac(xyz, P["thr"], 3, T, P["seed"], want_trials=True)
    rows, status = o["trial_plane"][0], o["trial_status"][0]
    pts = xyz[0].t().contiguous()                           # [N,3]
    thr = torch.tensor(P["thr"], dtype=torch.float32, device="cuda")
    count = torch.full((T,), -1, dtype=torch.int32, device="cuda")
    for lo in range(0, T, 16):
        n, p0 = rows[lo:lo + 16, None, 0:3], rows[lo:lo + 16, None, 4:7]
        r = pts[None] - p0
        d = torch_fma32(n[..., 2], r[..., 2], torch_fma32(n[..., 1], r[..., 1], n[..., 0] * r[..., 0]))
        count[lo:lo + 16] = (d.abs() <= thr).sum(1).to(torch.int32)
    count = torch.where(status == 0, count, torch.full_like(count, -1))
    assert torch.equal(count, o["trial_count"][0]) and int((status == 0).sum()) > T // 2
    bt = int(o["best_trial"][0])
    assert bt == int(torch.argmax(count)) and int(o["count"][0]) == int(count[bt]) == int(o["inlier"][0].sum())
    small = sr.planted(P["N"], P["share"], P["thr"], P["seed"])
    reached = sr.angle(sr.segment_plane(small["x"], P["thr"], T, P["seed"])["fit"][:3], small["normal"])
    ang = sr.angle(o["plane"][0, :3].cpu().numpy(), c["normal"])
    print("angle at size", ang, "the restatement's at 2 000", reached, "bound", sr.angle_bound(P["thr"]))
    assert ang <= reached + sr.angle_bound(P["thr"])


# ------------------------------------------------------------------------------------------------------------------ the split

def test_split_by_plane_compacts_both_sides_in_index_order():
    vcrnet_amd, segment = mods()
    for B, N in ((1, 1), (3, 257), (2, 1000)):
        rs = np.random.RandomState(N)
        x = np.stack([sr.cloud(N, seed=b) for b in range(B)])
        if N > 1:
            x[0, 1, 0] = np.nan                             # a point that is nobody's inlier goes to the rest
        inl = (rs.uniform(size=(B, N)) < 0.4).astype(np.int32) * rs.randint(1, 4, (B, N)).astype(np.int32)
        if B > 1:
            inl[1] = 0                                      # an empty side
        o = segment.split_rows(dev(x), dev(inl), guard=GUARD, prefill=BYTE)
        torch.cuda.synchronize()
        got = {k: checked(o[k], o["_raw"], k) for k in o if k != "_raw"}
        for b in range(B):
            for side, keep in (("plane", inl[b] > 0), ("rest", ~(inl[b] > 0))):
                idx = np.nonzero(keep)[0]
                k = len(idx)
                assert got[side + "_count"][b] == k, (N, b, side)
                assert np.array_equal(got[side + "_index"][b][:k], idx) and (got[side + "_index"][b][k:] == -1).all()
                assert np.array_equal(bits(got[side + "_points"][b][:, :k]), bits(x[b][:, idx]))
                assert np.isnan(got[side + "_points"][b][:, k:]).all()
            assert got["plane_count"][b] + got["rest_count"][b] == N
        (pp, pc, pi), (rp, rc, ri) = vcrnet_amd.split_by_plane(dev(x), dev(inl))
        for k, t in (("plane_points", pp), ("plane_count", pc), ("plane_index", pi), ("rest_points", rp), ("rest_count", rc),
                     ("rest_index", ri)):
            assert np.array_equal(bits(t.cpu().numpy()), bits(got[k])), k
        both = segment.split_rows(dev(x), dev(inl), want_index=False)
        assert "plane_index" not in both and torch.equal(both["rest_count"], rc)


# ---------------------------------------------------------------------------------------------------------------- the peeling

def three_planes(seed, sizes=(900, 500, 250), noise=150, thr=0.01):
    """Three planted planes of different sizes, far from parallel, in the unit cube, plus uniform noise; shuffled."""
    rs = np.random.RandomState(600 + seed)
    normals = np.eye(3)[rs.permutation(3)] + rs.uniform(-0.1, 0.1, (3, 3))
    parts, owner = [], []
    for k, (n, size) in enumerate(zip(normals, sizes)):
        n = n / np.linalg.norm(n)
        u = np.cross(n, [0.3, 0.5, 0.8])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        ab = rs.uniform(-0.45, 0.45, (2, size))
        centre = np.full(3, 0.5) + n * (0.12 * (k - 1))
        parts.append(centre[:, None] + u[:, None] * ab[0] + v[:, None] * ab[1] + n[:, None] * rs.uniform(-0.2 * thr, 0.2 * thr, size))
        owner += [k] * size
    parts.append(rs.uniform(0, 1, (3, noise)))
    owner += [-1] * noise
    perm = rs.permutation(len(owner))
    return np.concatenate(parts, 1)[:, perm].astype(np.float32), np.asarray(owner)[perm], normals


def test_segment_planes_peels_in_order_of_size_and_stops_a_cloud_on_its_own():
    vcrnet_amd, _ = mods()
    thr, T, K = 0.01, 200, 4
    x0, own0, normals0 = three_planes(0)
    x1, own1, _ = three_planes(1)
    x2 = x1.copy()
    x2[:, own1 != 0] = np.random.RandomState(2).uniform(0, 1, (3, int((own1 != 0).sum()))).astype(np.float32)   # one plane only
    x = np.stack([x0, x1, x2])
    labels, planes, counts = (t.cpu().numpy() for t in vcrnet_amd.segment_planes(dev(x), thr, K, 200, num_iterations=T, seed=5))
    assert labels.shape == (3, x.shape[2]) and planes.shape == (3, K, 4) and counts.shape == (3, K)
    for b in range(3):
        want = sr.segment_planes(x[b], thr, K, 200, T, 5)
        assert np.array_equal(labels[b], want[0]) and np.array_equal(counts[b], want[1]), b
        found = int((want[1] > 0).sum())
        assert np.isnan(planes[b, found:]).all() and not np.isnan(planes[b, :found]).any()
        assert np.abs(planes[b, :found, :3] - want[2][:found, :3]).max() <= 2.0 ** -20
    for b, own in ((0, own0), (1, own1)):                   # three planes, the largest first, then nothing of 200 points
        assert (counts[b, :3] > 0).all() and counts[b, 3] == 0 and (np.diff(counts[b, :3]) < 0).all()
        for k in range(3):
            assert (labels[b][own == k] == k).mean() >= 0.9, (b, k)       # (the rest lies within thr of an earlier plane)
    assert sr.angle(planes[0, 0, :3], normals0[0]) < 0.02
    assert counts[2, 0] > 0 and (counts[2, 1:] == 0).all() and (labels[2] <= 0).all()       # stopped on its own ...
    alone = [t.cpu().numpy() for t in vcrnet_amd.segment_planes(dev(x[:2]), thr, K, 200, num_iterations=T, seed=5)]
    assert np.array_equal(alone[0], labels[:2]) and np.array_equal(alone[2], counts[:2])    # ... the others unaffected
    assert np.array_equal(bits(alone[1]), bits(planes[:2]))


def test_the_pipeline_takes_the_table_away_before_clustering():
    """A table with two blobs standing on it: clustered as it is, the table joins everything into one cluster; after
    segment_plane and split_by_plane the rest clusters into the two blobs, 0 and 1 in index order."""
    vcrnet_amd, _ = mods()
    rs = np.random.RandomState(12)

    def ball(centre, n):
        v = rs.normal(size=(3, n))
        return np.asarray(centre)[:, None] + v / np.linalg.norm(v, axis=0) * 0.05 * rs.uniform(0, 1, n) ** (1 / 3)
    g = (np.stack(np.meshgrid(np.arange(60), np.arange(50)), 0).reshape(2, -1) + rs.uniform(-0.3, 0.3, (2, 3000))) / 60
    table = np.stack([g[0], g[1], rs.uniform(-0.001, 0.001, 3000)])
    a, b = ball((0.3, 0.3, 0.06), 250), ball((0.7, 0.5, 0.06), 250)
    x = np.concatenate([a, table, b], 1).astype(np.float32)[None]
    xyz = dev(x)
    eps, mp = 0.04, 5
    labels, n = vcrnet_amd.cluster_dbscan(xyz, eps, mp)
    assert int(n[0]) == 1 and bool((labels[0] == 0).all())
    plane, inlier, count = vcrnet_amd.segment_plane(xyz, 0.015, num_iterations=200, seed=1)
    assert abs(float(plane[0, 2])) > 0.999 and int(count[0]) >= 3000
    (_, tc, _), (rest, rc, index) = vcrnet_amd.split_by_plane(xyz, inlier)
    assert int(tc[0]) == int(count[0]) and int(tc[0]) + int(rc[0]) == x.shape[2]
    labels, n = vcrnet_amd.cluster_dbscan(rest, eps, mp)
    k = int(rc[0])
    index, labels = index[0, :k].cpu().numpy(), labels[0].cpu().numpy()
    assert int(n[0]) == 2 and (labels[k:] == -1).all()
    assert (labels[:k][index < 250] == 0).all() and (labels[:k][index >= 3250] == 1).all()
    assert (index < 250).sum() > 150 and (index >= 3250).sum() > 150
