"""vcr_fps_f32 on the GPU: farthest-point sampling, index for index.

The result is discrete, so EVERY comparison here is exact (torch.equal / array_equal): against the reference's recorded
indices (tests/golden/fps_*.npz) and, at sizes too large to commit, against the CPU restatement (tests/fps_restated.py) that
tests/test_fps_cpu.py holds to those same fixtures."""
import glob
import os
import threading

import numpy as np
import pytest
import torch

import fps_restated as fr
import oracle
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "fps_*.npz")))
SENTINEL = -0x5A5A5A5A
RESIDENT, STREAMING = 1, 2


def native():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native as n
    return n


def uniform(seed, B, N, scale=1.0):
    return (np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, 3, N)) * scale).astype(np.float32)


def lattice(seed, N):
    rs = np.random.RandomState(seed)
    grid = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), 0).reshape(3, -1).astype(np.float32) * 0.25
    return grid[:, rs.randint(0, grid.shape[1], size=N)]


def run(x, npoint, start=None, variant=0, want_points=False, prefill=None):
    """numpy [B,3,N] -> int64 numpy [B,npoint] (and the sampled clouds as a tensor)."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    st = None if start is None else torch.as_tensor(np.asarray(start), dtype=torch.int32).cuda()
    idx, pts = native().fps(xt, npoint, start=st, variant=variant, want_points=want_points, prefill=prefill)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy().astype(np.int64)
    return (idx, pts) if want_points else idx


def forms_for(N):
    return (0, RESIDENT, STREAMING) if N <= 20480 else (0, STREAMING)


def test_fixture_list_is_complete():
    assert len(FIXTURES) == 13, FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_index_for_index(name):
    """Every recorded case of the reference, explicit start and (where the fixture allows) the barycentre rule, through
    native.fps in every form and through farthest_point_sample."""
    import vcrnet_amd
    z = np.load(os.path.join(GOLDEN, f"fps_{name}.npz"))
    npoint = int(z["npoint"])
    for k, s in enumerate(z["scales"]):
        x = z["xyz"] * np.float32(s)
        ref = z[f"idx_s{k}"].astype(np.int64)
        for v in forms_for(x.shape[2]):
            assert np.array_equal(run(x, npoint, start=ref[:, 0], variant=v), ref), (name, s, v, "start")
            if not int(z["use_start"]):
                assert np.array_equal(run(x, npoint, variant=v), ref), (name, s, v, "barycentre")
        if not int(z["use_start"]):
            got = vcrnet_amd.farthest_point_sample(torch.from_numpy(x).cuda(), npoint)
            assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == ref.shape
            assert torch.equal(got.cpu(), torch.from_numpy(ref)), (name, s)


# one below, at and one above the capacity of every instantiation (resident: 1, 4, 8, 16, 20 points per thread of 1024;
# streaming: 32, 64, 128), N not a multiple of the block, N = 1
BOUNDARY_N = [1, 2, 63, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 20479, 20480, 20481,
              32767, 32768, 32769, 65535, 65536, 65537]


@pytest.mark.parametrize("N", BOUNDARY_N)
def test_every_form_gives_the_same_indices(N):
    n = native()
    x = uniform(1000 + N, 2, N)
    want = fr.fps(x, 24)
    form, ppt = n.fps_form(N)
    assert form == (RESIDENT if N <= 20480 else STREAMING) and ppt * 1024 >= N
    for v in forms_for(N):
        assert np.array_equal(run(x, 24, variant=v), want), (N, v)
    start = [N - 1, N // 2]
    want = fr.fps(x, 7, start=start)
    for v in forms_for(N):
        assert np.array_equal(run(x, 7, start=start, variant=v), want), (N, v, "start")


@pytest.mark.parametrize("N,npoint", [(1, 1), (1, 9), (5, 1), (100, 150), (1500, 1), (3000, 3100)])
def test_degenerate_sizes_in_every_form(N, npoint):
    x = uniform(77 + N, 3, N)
    want = fr.fps(x, npoint)
    for v in forms_for(N):
        assert np.array_equal(run(x, npoint, variant=v), want), (N, npoint, v)


@pytest.mark.parametrize("B,N,npoint,variants", [(4, 16384, 1024, (0, STREAMING)), (2, 65536, 4096, (0,)), (1, 131072, 2048, (0,))])
def test_large_seeded_clouds_against_the_restatement(B, N, npoint, variants):
    x = uniform(N + B, B, N, scale=3.0)
    for b in range(B):
        assert fr.margin(x[b]) >= 1e-4
    want = fr.fps(x, npoint)
    for v in variants:
        assert np.array_equal(run(x, npoint, variant=v), want), (N, v)


def test_clouds_of_a_batch_are_independent():
    """A lattice (ties everywhere), a cloud of one repeated point and a uniform cloud in one batch: each equals its B = 1 run
    and the restatement (explicit starts: the tie clouds' barycentre start is a rounding decision)."""
    N = 2000
    rep = np.repeat(uniform(5, 1, 1)[0], N, axis=1)
    x = np.stack([lattice(3, N), rep, uniform(6, 1, N)[0]])
    start = [17, 1999, 3]
    want = fr.fps(x, 300, start=start)
    for v in forms_for(N):
        got = run(x, 300, start=start, variant=v)
        assert np.array_equal(got, want), v
        for b in range(3):
            assert np.array_equal(run(x[b:b + 1], 300, start=start[b:b + 1], variant=v), got[b:b + 1]), (v, b)
        bary = run(x, 300, variant=v)                        # the barycentre rule: batch == single, whatever the rounding decides
        for b in range(3):
            assert np.array_equal(run(x[b:b + 1], 300, variant=v), bary[b:b + 1]), (v, b)


@pytest.mark.parametrize("N,npoint", [(3000, 512), (40000, 300)])
@pytest.mark.parametrize("pad", [0, 37])
def test_sampled_clouds_equal_the_gather_bit_for_bit(N, npoint, pad):
    """out_cf, written by the launch as each point is chosen, is xyz gathered at idx -- with and without a cloud stride above 3 N."""
    n = native()
    B = 3
    x = torch.from_numpy(uniform(N + pad, B, N)).cuda()
    if pad:
        buf = torch.full((B, 3 * N + pad), float("nan"), device="cuda")
        view = buf.as_strided((B, 3, N), (3 * N + pad, N, 1))
        view.copy_(x)
        assert view.data_ptr() == buf.data_ptr() and view.stride(0) == 3 * N + pad
    else:
        view = x
    for v in forms_for(N):
        idx, pts = n.fps(view, npoint, variant=v)
        assert pts.shape == (B, 3, npoint) and idx.dtype == torch.int32
        gathered = torch.gather(x, 2, idx.long().unsqueeze(1).expand(B, 3, npoint))
        assert torch.equal(pts.view(torch.int32), gathered.view(torch.int32)), v
        assert np.array_equal(idx.cpu().numpy(), fr.fps(x.cpu().numpy(), npoint)), v
    idx_only, none = n.fps(view, npoint, want_points=False)
    assert none is None and torch.equal(idx_only, idx)


@pytest.mark.parametrize("N", [700, 30000])
def test_non_finite_coordinates(N):
    """NaN / +-inf coordinates: the restatement's indices (= the reference's rule: such a point is chosen second and then for
    ever), every index written in [0, N), the finite clouds of the batch untouched."""
    clean = uniform(N, 4, N)
    x = clean.copy()
    x[0, 1, 7] = np.nan
    x[1, 0, N - 1] = np.inf
    x[2, 2, 5] = -np.inf
    x[2, 0, 6] = np.nan
    want = fr.fps(x, 40)
    assert (want[0, 1:] == 7).all() and want[0, 0] == 0          # NaN cloud: start 0 (every distance NaN), then the NaN point
    assert want[1, 0] == N - 1 and (want[1, 2:] == N - 1).all()  # +inf: that point's barycentre distance is the only NaN
    for v in forms_for(N):
        got = run(x, 40, variant=v, prefill=SENTINEL)
        assert got.min() >= 0 and got.max() < N
        assert np.array_equal(got, want), v
        assert np.array_equal(got[3], run(clean, 40, variant=v)[3])
        idx, pts = run(x, 40, variant=v, want_points=True)
        gathered = torch.gather(torch.from_numpy(x).cuda(), 2, torch.from_numpy(idx).cuda().unsqueeze(1).expand(4, 3, 40))
        assert torch.equal(pts.view(torch.int32), gathered.view(torch.int32))


@pytest.mark.parametrize("N", [700, 30000])
def test_out_of_range_start_is_clamped(N):
    x = uniform(N + 1, 4, N)
    start = np.asarray([-5, N, N + 100, 2 ** 31 - 1], dtype=np.int64)
    want = fr.fps(x, 20, start=np.clip(start, 0, N - 1))
    for v in forms_for(N):
        got = run(x, 20, start=start.astype(np.int32), variant=v, prefill=SENTINEL)
        assert got.min() >= 0 and got.max() < N
        assert np.array_equal(got, want), v


def test_two_streams_and_two_threads():
    """Concurrent calls (two host threads, each on its own stream) give the single-call results: the entry point keeps no state."""
    n = native()
    jobs = [(uniform(31, 3, 9000), 700), (uniform(32, 2, 40000), 500)]
    single = [run(x, p) for x, p in jobs]
    dev = [torch.from_numpy(x).cuda() for x, _ in jobs]
    out, err = [None, None], []

    def work(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                res = [n.fps(dev[i], jobs[i][1])[0] for _ in range(4)]
            st.synchronize()
            out[i] = [r.cpu().numpy() for r in res]
        except Exception as e:                                # noqa: BLE001
            err.append(e)
    torch.cuda.synchronize()
    ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not err, err
    for i in range(2):
        for r in out[i]:
            assert np.array_equal(r, single[i])


def test_argument_errors_on_device_tensors():
    n = native()
    x = torch.zeros(2, 3, 100, device="cuda")
    with pytest.raises(n.VcrHipError):
        n.fps(x, 0)
    with pytest.raises(n.VcrHipError):
        n.fps(x, 10, variant=3)
    with pytest.raises(n.VcrHipError):
        n.fps(torch.zeros(1, 3, 30000, device="cuda"), 10, variant=RESIDENT)
    with pytest.raises(n.VcrHipError):
        n.fps(torch.zeros(2, 4, 100, device="cuda"), 10)
    with pytest.raises(n.VcrHipError):
        n.fps(x, 10, start=torch.zeros(3, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------- register_sampled

def _pair(Ns, Nt, B=2, first=500):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import synth
    src, tgt, _, _, _ = synth.make_batch(first, B, max(Ns, Nt), kind="uniform")
    return np.ascontiguousarray(src[:, :, :Ns]), np.ascontiguousarray(tgt[:, :, :Nt])


@pytest.mark.parametrize("iters", [1, 2])
def test_register_sampled_whole(iters):
    """Ns = 3000, Nt = 4100 sampled to 1024: bit-identical to the manual composition fps -> vcrnetIter, the indices are the
    restatement's, and the pose is the oracle's on those sampled clouds at BASELINE's tolerance."""
    import vcrnet_amd
    from vcrnet_amd.module import vcrnetIter
    from test_hip_forward import build_net, R_TOL, T_TOL
    n = native()
    net, w = build_net()
    src, tgt = _pair(3000, 4100)
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    with torch.no_grad():
        out = vcrnet_amd.register_sampled(net, s, t, 1024, iter=iters)
        idx_s, src_s = n.fps(s, 1024)
        idx_t, tgt_s = n.fps(t, 1024)
        manual = vcrnetIter(net, src_s, tgt_s, iter=iters)
    assert len(out) == 8
    for a, b in zip(out[:6], manual):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert out[6].dtype == torch.int64 and torch.equal(out[6], idx_s.long()) and torch.equal(out[7], idx_t.long())
    assert np.array_equal(out[6].cpu().numpy(), fr.fps(src, 1024)) and np.array_equal(out[7].cpu().numpy(), fr.fps(tgt, 1024))
    ref = oracle.vcrnet_iter(w, src_s.cpu(), tgt_s.cpu(), oracle.OracleConfig(), iters=iters)
    dR = float((out[2].cpu() - ref[2]).abs().max())
    dt = float((out[3].cpu() - ref[3]).abs().max())
    print(f"register_sampled iter={iters}: max|dR|={dR:.3e} max|dt|={dt:.3e}")
    assert dR <= R_TOL and dt <= T_TOL, (dR, dt)


def test_register_sampled_explicit_start_and_partial():
    """partial=True, both clouds sampled to 768: the bit-identity with the manual composition only (the free-running partial
    selections have their own envelope tests); explicit starts travel through."""
    import vcrnet_amd
    from vcrnet_amd.module import vcrnetIter
    from test_hip_forward import build_net
    n = native()
    net, _ = build_net(partial=True)
    src, tgt = _pair(3000, 4100, first=510)
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    st = (torch.tensor([5, 2999], dtype=torch.int32).cuda(), torch.tensor([0, 4099], dtype=torch.int32).cuda())
    with torch.no_grad():
        for start in (None, st):
            out = vcrnet_amd.register_sampled(net, s, t, 768, start=start)
            idx_s, src_s = n.fps(s, 768, start=None if start is None else start[0])
            idx_t, tgt_s = n.fps(t, 768, start=None if start is None else start[1])
            manual = vcrnetIter(net, src_s, tgt_s, iter=1)
            for a, b in zip(out[:6], manual):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert torch.equal(out[6], idx_s.long()) and torch.equal(out[7], idx_t.long())
            if start is not None:
                assert out[6][:, 0].tolist() == [5, 2999] and out[7][:, 0].tolist() == [0, 4099]


def test_register_sampled_refuses_bad_input():
    import vcrnet_amd
    from test_hip_forward import build_net
    n = native()
    net, _ = build_net()
    a, b = torch.zeros(2, 3, 3000, device="cuda"), torch.zeros(3, 3, 4100, device="cuda")
    with torch.no_grad():
        with pytest.raises(n.VcrHipError, match="same number of clouds"):
            vcrnet_amd.register_sampled(net, a, b, 1024)
        with pytest.raises(n.VcrHipError, match=r"\[B, 3, N\]"):
            vcrnet_amd.register_sampled(net, a.transpose(1, 2), b[:2], 1024)
        with pytest.raises(n.VcrHipError):                   # the forward itself still refuses unequal sizes
            net(a, torch.zeros(2, 3, 4100, device="cuda"))
