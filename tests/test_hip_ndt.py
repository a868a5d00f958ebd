"""include/ndt/vcr_hip_ndt.h on the GPU against the numpy restatement (tests/ndt_restated.py): the map
byte for byte; the voxels a point reads and the hits exactly; f, g and H within a measured multiple of 2^-52 times the sums of
the absolute terms -- the one exp per (point, voxel) is the device library's -- and byte for byte once the restatement is fed the
device's e; the loop by its closing invariant, its trace, its stops and the recovery recipe.  Every call runs with 4096 elements of
guard behind outputs prefilled with 0xFF, the workspace prefilled likewise."""
import functools
import math

import numpy as np
import pytest
import torch

import ndt_restated as nd
import voxel_restated as vr

pytestmark = pytest.mark.gpu

GUARD = 4096
BYTE = 0xFF
F32 = np.float32
MAP_KEYS = ("mean", "inv_cov", "valid", "count", "voxel_points", "origin")
MAP_SIZES = (1, 5, 6, 7, 63, 64, 65, 257, 1000, 5000)
SCAN_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
VARIANTS = (0, 1)
# What a device sum may differ from the restatement's by, in units of 2^-52 times the sum of the absolute terms.  Every term is
# linear in e = exp(.), the one value the header leaves to the device's math library (the ROCm tree documents no bound for
# its double exp), so the allowance is measured: the largest ratio over every case of
# test_derivatives_match_the_restatement on the device was K_MEASURED; the test allows four times that.
# profiles/ndt_ledger.txt records it.
K_MEASURED = 1.139
K_ALLOWED = 4 * K_MEASURED
RECOVERY_FACTOR = 1.5                                        # the GPU loop's allowance over the restated loop's error (ledger)


def mods():
    import vcrnet_amd
    from vcrnet_amd import ndt
    return vcrnet_amd, ndt


def dev(x):
    return torch.tensor(np.array(x)).cuda()


def guards_untouched(raw, outs):
    for name, buf in raw.items():
        n = outs[name].numel()
        band = buf[n:].view(torch.uint8).cpu().numpy()
        assert band.size == GUARD * buf.element_size() and (band == BYTE).all(), (name, "guard band written")


def build_map(tgt, h, min_points=6, min_eig_ratio=0.01):
    """tgt [B,3,Nt] numpy -> (the NdtMap, its tensors as numpy)."""
    _, ndt = mods()
    m = ndt.ndt_map(dev(tgt), h, min_points, min_eig_ratio, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    guards_untouched(m._raw, {k: getattr(m, k) for k in ndt.NdtMap.FIELDS})
    return m, {k: getattr(m, k).cpu().numpy() for k in ndt.NdtMap.FIELDS}


def map_is_the_restatement(got, tgt, h, min_points=6, min_eig_ratio=0.01):
    want = nd.map_batch(tgt, h, min_points, min_eig_ratio)
    for b, w in enumerate(want):
        for k in MAP_KEYS:
            assert nd.same_bits(got[k][b], np.asarray(w[k])), (b, k)
        table_is_the_lookup(got, b, w)
    return want


def table_is_the_lookup(got, b, w):
    """The table's first T slots hold every voxel's key once with its number, and nothing else."""
    _, ndt = mods()
    V = max(int(w["count"]), 0)
    T = 1 << math.ceil(math.log2(2 * V + 2))
    keys, vals = got["table_keys"][b], got["table_vals"][b]
    full = keys != -1
    assert not full[T:].any() and (vals[~full] == -1).all() and int(full.sum()) == V <= T // 2
    have = {int(k): int(v) for k, v in zip(keys[full], vals[full])}
    assert have == {c[0] | c[1] << 21 | c[2] << 42: v for c, v in w["lookup"].items()}


def derive(src, m, R=None, t=None, neighbors=7, variant=0):
    _, ndt = mods()
    o = ndt.ndt_derivatives(dev(src), m, None if R is None else dev(R), None if t is None else dev(t), neighbors,
                            want_stages=True, variant=variant, guard=GUARD, prefill=BYTE)
    torch.cuda.synchronize()
    guards_untouched(o["_raw"], o)
    return {k: o[k].cpu().numpy() for k in ("score", "hits", "g", "H", "e", "voxel")}


def refine(src, tgt, R=None, t=None, h=None, **kw):
    _, ndt = mods()
    o = ndt.refine_registration_ndt(dev(src), None if tgt is None else dev(tgt), None if R is None else dev(R),
                                    None if t is None else dev(t), h, want_trace=True, guard=GUARD, prefill=BYTE, **kw)
    torch.cuda.synchronize()
    guards_untouched(o["_raw"], o)
    return {k: v.cpu().numpy() for k, v in o.items() if k != "_raw"}


# ----------------------------------------------------------------------------------------------------------------------- the map

@pytest.mark.parametrize("Nt", MAP_SIZES)
def test_the_map_is_the_restatement_byte_for_byte(Nt):
    h = max(vr.edge_for(Nt, 12.0), 0.3)
    tgt = vr.uniform(20 + Nt % 7, 1, Nt)
    _, got = build_map(tgt, h)
    want = map_is_the_restatement(got, tgt, h)
    if Nt >= 257:
        assert want[0]["valid"].sum() > 3


def test_a_batch_with_a_too_fine_an_all_nan_and_a_one_voxel_cloud():
    N = 500
    tgt = vr.uniform(31, 3, N)
    tgt[0, :, 1] = 5000.0                                    # at h = 2^-9 its cell would be past 2^21: too fine
    tgt[1] = np.nan
    tgt[2] = tgt[2] * F32(2.0 ** -12)                        # the whole cloud in one voxel
    tgt[2, 0, 7] = np.inf
    h = float(F32(2.0 ** -9))
    _, got = build_map(tgt, h)
    want = map_is_the_restatement(got, tgt, h)
    assert [int(w["count"]) for w in want] == [-1, 0, 1] and want[2]["valid"][0] == 1 and want[2]["voxel_points"][0] == N - 1
    assert np.isnan(got["origin"][1]).all() and np.isfinite(got["origin"][0]).all()
    for b, cloud in enumerate(tgt):                          # a cloud's map does not depend on its batch
        _, alone = build_map(cloud[None], h)
        for k in MAP_KEYS:
            assert nd.same_bits(alone[k][0], got[k][b]), (b, k)


def test_copies_a_planar_voxel_and_a_lattice_of_five_and_six():
    rs = np.random.RandomState(4)
    x = np.concatenate([np.repeat(rs.uniform(0, 0.1, (3, 1)), 8, axis=1),             # copies of a point: C all zero
                        np.stack([rs.uniform(1.0, 1.2, 9), rs.uniform(1.0, 1.2, 9), np.full(9, 1.1)]),      # planar: the floor acts
                        rs.uniform(2.0, 2.2, (3, 5)), rs.uniform(3.0, 3.2, (3, 6))], axis=1).astype(F32)
    _, got = build_map(x[None], 0.5)
    want = map_is_the_restatement(got, x[None], 0.5)
    assert list(want[0]["valid"][:4]) == [0, 1, 0, 1]
    # a lattice: voxels of exactly five and exactly six points, interleaved in index order
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij")).reshape(3, -1)
    pts = []
    for j in range(cells.shape[1]):
        n = 5 + j % 2
        pts.append(cells[:, j:j + 1] + rs.uniform(0.05, 0.95, (3, n)))
    lat = np.concatenate(pts, axis=1)
    lat = np.concatenate([np.zeros((3, 1)), lat[:, rs.permutation(lat.shape[1])]], axis=1).astype(F32)   # (min 0: origin -0.5)
    lat[:, 1:] += F32(0.5)
    _, got = build_map(lat[None], 1.0)
    want = map_is_the_restatement(got, lat[None], 1.0)[0]
    M = int(want["count"])
    vp, ok = want["voxel_points"][:M], want["valid"][:M]
    assert set(vp[1:]) == {5, 6} and (ok[vp == 5] == 0).all() and (ok[vp == 6] == 1).all()
    _, got5 = build_map(lat[None], 1.0, min_points=5, min_eig_ratio=0.2)
    want5 = map_is_the_restatement(got5, lat[None], 1.0, 5, 0.2)[0]
    assert (want5["valid"][:M][vp >= 5] == 1).all()


# -------------------------------------------------------------------------------------------------------------------- the lookup

def test_the_table_at_its_designed_load_faces_the_box_and_the_last_cell():
    """Every point in a voxel of its own fills the table to V / T = Nt / 2^ceil(log2(2 Nt + 2)); moved points exactly on a cell
    face, outside the box on every side, and in the cells 2^21 - 1."""
    rs = np.random.RandomState(9)
    N = 1023                                                 # 2 N + 2 = 2048 = T: the fullest a table gets
    cells = np.concatenate([[0], 1 + rs.permutation(16 * 16 * 16 - 1)[:N - 1]])      # cell 0 first: origin = 0.5 - 0.5 = 0 exactly
    own = np.stack([cells % 16, cells // 16 % 16, cells // 256]).astype(np.float64) + 0.5
    dense = own[:, :40, None] + rs.uniform(0.0, 0.45, (3, 40, 8))                   # forty of them get eight more points
    tgt = np.concatenate([own, dense.reshape(3, -1)], axis=1).astype(F32)
    m, got = build_map(tgt[None], 1.0, min_points=6)
    want = map_is_the_restatement(got, tgt[None], 1.0)[0]
    assert got["origin"][0].tolist() == [0.0, 0.0, 0.0]
    V = int(want["count"])
    assert V == N and int(want["valid"].sum()) == 40
    m1, got1 = build_map(own.astype(F32)[None], 1.0)
    assert int(got1["count"][0]) == N and int((got1["table_keys"][0] != -1).sum()) == N and got1["table_keys"].shape[1] == 2 * N + 2
    map_is_the_restatement(got1, own.astype(F32)[None], 1.0)
    # scan points: on faces (integers), outside on every side, in valid voxels
    centre = own[:, :40]
    src = np.concatenate([np.floor(centre) + np.array([[1.0], [0.25], [0.5]]), np.floor(centre) + np.array([[0.5], [0.0], [0.5]]),
                          centre, np.array([[-0.25, 16.5, 3, 3, 3, 3, -40, 1e30], [3, 3, -0.25, 16.5, 3, 3, -40, 3], [3, 3, 3, 3, -0.25, 16.5, -40, 3]]),
                          np.array([[np.nan, 3, np.inf], [3, np.nan, 3], [3, 3, 3]])], axis=1).astype(F32)
    o = derive(src[None], m)
    w = nd.derivatives(src, want)
    assert np.array_equal(o["voxel"][0], w["voxel"]) and int(o["hits"][0]) == w["hits"] and w["hits"] >= 80
    for i in (0, 2, 4, 6, 7, 8, 9, 10):                      # below cell 0, far outside, or not finite: nothing is read
        assert (w["voxel"][len(w["voxel"]) - 11 + i] == -1).all(), i
    fed = nd.derivatives(src, want, e=o["e"][0])
    assert nd.same_bits(np.concatenate([o["score"], o["hits"].astype(np.float64), o["g"][0], o["H"][0]]), fed["values"])


def test_cells_at_the_last_index_are_served():
    """h = 2^-10 and an extent of 2^21 - 1 cells on every axis: the voxels at cell 2^21 - 1 are found, their +1 neighbours skipped."""
    rs = np.random.RandomState(10)
    top = vr.FINE_UNDER
    lo = rs.uniform(0.0, 0.0009, (3, 10))
    lo[:, 0] = 0.0
    hi = top - rs.uniform(0.0, 0.0004, (3, 10))
    hi[:, 0] = top
    tgt = np.concatenate([lo, hi], axis=1).astype(F32)
    m, got = build_map(tgt[None], vr.FINE_H)
    want = map_is_the_restatement(got, tgt[None], vr.FINE_H)[0]
    assert int(want["count"]) >= 2 and max(max(c) for c in want["lookup"]) == (1 << 21) - 1
    src = np.concatenate([hi[:, :6], lo[:, :6]], axis=1).astype(F32)
    o = derive(src[None], m)
    w = nd.derivatives(src, want)
    assert np.array_equal(o["voxel"][0], w["voxel"]) and int(o["hits"][0]) == w["hits"]


# --------------------------------------------------------------------------------------------------------------- the derivatives

@functools.lru_cache(maxsize=None)
def scene():
    """One target of 3000 surface points in two clouds and its restated maps, shared (and left unchanged) by the tests below."""
    tgt = np.stack([nd.torus(41, 3000, noise=0.01), nd.torus(42, 3000, noise=0.02)])
    return tgt, 0.3, nd.map_batch(tgt, 0.3)


@functools.lru_cache(maxsize=None)
def scene_map():
    tgt, h, _ = scene()
    return build_map(tgt, h)[0]


def poses(kind):
    """all / some / none of the source inside the map."""
    R = np.stack([nd.pose(0.05, 0.0, 1)[0], nd.pose(0.1, 0.0, 2)[0]]).astype(F32)
    t = {"all": np.array([[0.01, -0.02, 0.01], [0.0, 0.02, 0.0]]), "some": np.array([[1.2, 0.0, 0.0], [0.0, 0.9, 0.1]]),
         "none": np.array([[9.0, 0.0, 0.0], [0.0, -7.0, 5.0]])}[kind].astype(F32)
    return R, t


def ratios(o, w, b):
    """|device - restated| in units of 2^-52 times the sum of the absolute terms, over the 28 sums."""
    got = np.concatenate([o["score"][b:b + 1], o["g"][b], o["H"][b]])
    want = np.concatenate([w["values"][:1], w["values"][2:]])
    scale = np.concatenate([w["abs"][:1], w["abs"][2:]]) * 2.0 ** -52
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(scale > 0, np.abs(got - want) / scale, np.where(got == want, 0.0, np.inf))
    return float(r.max())


@pytest.mark.parametrize("kind", ("all", "some", "none"))
@pytest.mark.parametrize("Ns", SCAN_SIZES)
def test_derivatives_match_the_restatement(Ns, kind):
    tgt, h, maps = scene()
    m = scene_map()
    src = np.stack([nd.torus(50 + Ns, Ns, noise=0.01), nd.torus(51 + Ns, Ns, noise=0.01)])
    R, t = poses(kind)
    worst = 0.0
    for variant in VARIANTS:
        o = derive(src, m, R, t, variant=variant)
        for b in range(2):
            w = nd.derivatives(src[b], maps[b], R[b], t[b])
            assert np.array_equal(o["voxel"][b], w["voxel"]) and int(o["hits"][b]) == w["hits"], (variant, b)
            assert np.array_equal(np.isnan(o["e"][b]), w["voxel"] < 0)
            worst = max(worst, ratios(o, w, b))
            fed = nd.derivatives(src[b], maps[b], R[b], t[b], e=o["e"][b])               # the stage test: the device's e
            dev_values = np.concatenate([o["score"][b:b + 1], [float(o["hits"][b])], o["g"][b], o["H"][b]])
            assert nd.same_bits(dev_values, fed["values"]), (variant, b)
            if kind == "none":
                assert w["hits"] == 0 and not dev_values.any()
            if kind == "all" and Ns >= 63:
                assert w["hits"] > Ns // 2
    print("Ns %d %s: largest |difference| / (2^-52 sum |term|) = %.3f" % (Ns, kind, worst))
    assert worst <= K_ALLOWED


def test_one_neighbour_reads_the_own_cell_alone_and_the_identity_is_the_default():
    tgt, h, maps = scene()
    m = scene_map()
    src = np.stack([nd.torus(61, 300, noise=0.01), nd.torus(62, 300, noise=0.01)])
    one = derive(src, m, neighbors=1)
    for b in range(2):
        w = nd.derivatives(src[b], maps[b], neighbors=1)
        assert np.array_equal(one["voxel"][b], w["voxel"]) and (w["voxel"][:, 1:] == -1).all() and int(one["hits"][b]) == w["hits"] > 100
        assert nd.same_bits(np.concatenate([one["score"][b:b + 1], [float(one["hits"][b])], one["g"][b], one["H"][b]]),
                            nd.derivatives(src[b], maps[b], neighbors=1, e=one["e"][b])["values"])
    eye = derive(src, m, np.stack([np.eye(3, dtype=F32)] * 2), np.zeros((2, 3), F32), neighbors=1)
    for k in one:
        assert nd.same_bits(one[k], eye[k]), k


# ------------------------------------------------------------------------------------------------------------------------ the loop

@functools.lru_cache(maxsize=None)
def recovery(i):
    src, tgt, R0, t0, Rg, tg = nd.recovery_case(i)
    return src, tgt, R0, t0, Rg, tg, refine(src[None], tgt[None], R0[None], t0[None], nd.RECOVERY_H)


def ledger_figures():
    import test_ndt_cpu
    return test_ndt_cpu.ledger_figures()


@pytest.mark.parametrize("i", (0, 1))
def test_the_loop_recovers_the_pose_within_the_ledgers_allowance(i):
    """The recovery recipe of tests/test_ndt_cpu.py: the GPU loop may end RECOVERY_FACTOR times as far from the truth as the
    restated loop did (profiles/ndt_ledger.txt): the decisions are discrete and one unit of an exp may flip one."""
    src, tgt, R0, t0, Rg, tg, o = recovery(i)
    ea, es = nd.pose_error(o["R"][0], o["t"][0], Rg, tg)
    want = ledger_figures()[i]
    print("device recovery %d: iterations %d trials %d status %s angle %.6e shift %.6e (restated %.6e %.6e)"
          % (i, o["iterations"][0], o["trials"][0], nd.STATUS[o["status"][0]], ea, es, want[0], want[1]))
    assert ea <= RECOVERY_FACTOR * want[0] and es <= RECOVERY_FACTOR * want[1]
    assert 1 <= o["iterations"][0] <= 30 and o["iterations"][0] <= o["trials"][0] <= 120


@pytest.mark.parametrize("i", (0, 1))
def test_the_closing_invariant_and_the_trace(i):
    """score, hits, g and H are the derivative call's at (R_out, t_out), bit for bit; the accepted scores fall strictly; R_ba, t_ba
    are the refinements' inverse; probability is the header's expression."""
    _, ndt = mods()
    src, tgt, R0, t0, Rg, tg, o = recovery(i)
    m, _ = build_map(tgt[None], nd.RECOVERY_H)
    d = derive(src[None], m, o["R"], o["t"])
    for k in ("score", "hits", "g", "H"):
        assert nd.same_bits(d[k], o[k]), k
    acc = o["trace"][0][np.isfinite(o["trace"][0])]
    assert len(acc) == o["iterations"][0] + 1 and (np.diff(acc) < 0).all() and acc[-1] == o["score"][0]
    assert np.isnan(o["trace"][0][o["trials"][0] + 1:]).all()
    d1, _ = ndt.constants(0.55, nd.RECOVERY_H)
    assert o["probability"][0] == ((-d1) * (-o["score"][0])) / 500.0
    assert np.array_equal(o["R_ba"][0], o["R"][0].T)
    assert np.allclose(o["t_ba"][0], -(o["R"][0].astype(np.float64).T @ o["t"][0].astype(np.float64)), rtol=0, atol=1e-6)


def test_no_iterations_return_the_start_pose_and_its_derivatives():
    src, tgt, R0, t0, Rg, tg, _ = recovery(1)
    R, t = nd.pose(0.02, 0.01, 5)
    R, t = R.astype(F32)[None], t.astype(F32)[None]
    o = refine(src[None], tgt[None], R, t, nd.RECOVERY_H, max_iterations=0)
    m, _ = build_map(tgt[None], nd.RECOVERY_H)
    d = derive(src[None], m, R, t)
    assert nd.same_bits(o["R"], R) and nd.same_bits(o["t"], t)
    for k in ("score", "hits", "g", "H"):
        assert nd.same_bits(d[k], o[k]), k
    assert (o["iterations"][0], o["trials"][0], o["converged"][0], nd.STATUS[o["status"][0]]) == (0, 0, 0, "max iterations")
    assert o["trace"].shape == (1, 1) and o["trace"][0, 0] == o["score"][0]
    one = refine(src[None], tgt[None], R, t, nd.RECOVERY_H, max_iterations=5, max_trials=1)
    assert one["trials"][0] == 1 and one["iterations"][0] <= 1 and nd.STATUS[one["status"][0]] in ("max trials", "converged")


def test_a_batch_is_its_clouds_alone_in_every_variant_and_with_a_reused_map():
    """Three clouds -- the two recovery cases and a source wholly outside the map -- against each alone; the forced variant and a
    map built once and passed as map= return the same bytes."""
    _, ndt = mods()
    cases = [recovery(0), recovery(1)]
    src = np.stack([cases[0][0], cases[1][0], cases[0][0] + F32(50.0)])
    tgt = np.stack([cases[0][1], cases[1][1], cases[0][1]])
    R0 = np.stack([np.eye(3, dtype=F32)] * 3)
    t0 = np.zeros((3, 3), F32)
    o = refine(src, tgt, R0, t0, nd.RECOVERY_H)
    keys = ("R", "t", "R_ba", "t_ba", "score", "probability", "hits", "g", "H", "iterations", "trials", "converged", "status", "trace")
    for b in range(2):
        for k in keys:
            assert nd.same_bits(o[k][b], cases[b][6][k][0]), (b, k)
    assert nd.STATUS[o["status"][2]] == "no hits" and o["hits"][2] == 0 and o["converged"][2] == 0 and o["trials"][2] == 0
    assert nd.same_bits(o["R"][2], R0[2]) and nd.same_bits(o["t"][2], t0[2]) and o["score"][2] == 0.0
    forced = refine(src, tgt, R0, t0, nd.RECOVERY_H, variant=1)
    m, _ = build_map(tgt, nd.RECOVERY_H)
    reused = refine(src, None, R0, t0, None, map=m)
    again = refine(src, None, R0, t0, None, map=m)
    for k in keys:
        assert nd.same_bits(forced[k], o[k]) and nd.same_bits(reused[k], o[k]) and nd.same_bits(again[k], o[k]), k


# ------------------------------------------------------------------------------------------------- streams and graph capture

STREAM_KEYS = ("R", "t", "score", "hits", "g", "H", "iterations", "trials", "status", "d_score", "d_g", "count", "valid")


def stream_call(src, tgt):
    """The three calls in a row: the map, the derivatives at the identity and the loop on the map."""
    _, ndt = mods()
    m = ndt.ndt_map(tgt, nd.RECOVERY_H)
    d = ndt.ndt_derivatives(src, m)
    o = ndt.refine_registration_ndt(src, None, map=m, max_iterations=3)
    out = {k: o[k] for k in STREAM_KEYS[:9]}
    out.update(d_score=d["score"], d_g=d["g"], count=m.count, valid=m.valid)
    return out


def stream_data(i):
    src, tgt = nd.recovery_case(i)[:2]
    return {"src": src[None], "tgt": tgt[None] if i == 0 else (tgt[None] * F32(1.01))}


def test_the_calls_are_ordered_on_a_side_stream_and_replay_from_a_graph():
    """tests/test_hip_streams.py's checks (a) and (b) with its harness: behind a delayed overwrite of its inputs on a side stream
    the calls return while the stream is busy and their outputs are the eager calls' on the new data, byte for byte; captured
    once, their replays follow the buffers' contents."""
    import test_hip_streams as hs
    a, b = stream_data(0), stream_data(1)
    on_a, on_b = hs.eager(stream_call, a), hs.eager(stream_call, b)
    assert set(on_b) == set(STREAM_KEYS) and hs.wrong(on_a, on_b)
    busy, out = hs.side_stream(stream_call, a, b, delay_ms=25.0)  # (some sixty launches are enqueued behind the delay)
    assert busy, "the side stream was idle when the call returned: the delay is too short, or the call waits"
    assert not hs.wrong(out, on_b)
    first, again, back = hs.captured(stream_call, a, b)
    bad = hs.wrong(first, on_b), hs.wrong(again, on_b), hs.wrong(back, on_a)
    assert not any(bad), f"replays on (B, B again, A) differ from the eager calls in {bad}"
