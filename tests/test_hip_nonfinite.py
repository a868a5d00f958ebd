"""Non-finite and mis-shaped input (-m gpu).  The contract (include/vcr_hip.h): every index a kernel writes is
in range whatever the input values; rankselect and the pair-score arg-max order values the way torch does (NaN above +inf);
a pair whose non-finite coordinate reaches the rigid solve comes back with an all-NaN pose, and every other pair of its batch
stays bit-identical;
a tgt that is not shaped like src is refused before anything is launched.

The kernel-level tests fill every index output with a sentinel before the launch and check every index on the host; nothing
here reads an index on the device that the host has not checked."""
import numpy as np
import pytest
import torch

from test_hip_kernels import dev, knn_sets_ok

pytestmark = pytest.mark.gpu

SENT = -7


@pytest.fixture(scope="module")
def nat():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native
    native.lib()
    return native


def bits(t):
    """Bit pattern of a tensor: NaN compares equal to the same NaN."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ---------------------------------------------------------------- kNN

def _poison(x, kind, k, rs):
    """x [N, C] float32 numpy (one cloud; C = 3 coordinates or 64 features) -> poisoned copy."""
    x = x.copy()
    N, C = x.shape
    if kind == "nan1":
        x[rs.randint(N), rs.randint(C)] = np.nan
    elif kind == "infpm":
        p = rs.choice(N, 2, replace=False)
        x[p[0], rs.randint(C)] = np.inf
        x[p[1], rs.randint(C)] = -np.inf
    elif kind == "allnan":
        x[:] = np.nan
    elif kind == "kfinite":                                # only k finite points: their queries get short lists too
        x[rs.permutation(N)[k:], rs.randint(C)] = np.nan
    return x


def _check_knn(idx_p, idx_c, x_cf, fin, k, poisoned=1):
    """idx_p / idx_c [B,N,k] of the poisoned / clean batch; x_cf [C,N] cpu of the poisoned cloud, fin [N] its finite points."""
    got = idx_p.cpu().numpy()
    N = got.shape[1]
    assert not (got == SENT).any(), "an index slot was left unwritten"
    assert (got >= 0).all() and (got < N).all(), "index out of range"
    ref = idx_c.cpu().numpy()
    for b in range(got.shape[0]):
        if b != poisoned:
            assert np.array_equal(got[b], ref[b]), f"unpoisoned cloud {b} changed"
    row = got[poisoned]
    nf = int(fin.sum())
    fidx = np.flatnonzero(fin)
    for q in np.flatnonzero(~fin):                         # no finite score: the whole row is the query itself
        assert (row[q] == q).all(), (q, row[q])
    if nf >= k + 1:
        pos = np.full(N, -1)
        pos[fidx] = np.arange(nf)
        sub = row[fidx]
        assert fin[sub].all(), "a finite query got a non-finite neighbour although it had k + 1 finite candidates"
        nbad = knn_sets_ok(x_cf[None, :, fidx], torch.from_numpy(pos[sub]), k)
        assert nbad <= max(2, nf // 100), nbad
    else:                                                  # short lists: the nf - 1 others, then the query's own index
        for q in fidx:
            assert set(row[q].tolist()) == set(fidx.tolist()), (q, row[q])
            assert (row[q][max(nf - 1, 0):] == q).all(), (q, row[q])


def _clouds(N, k, kind, seed, B=3):
    rs = np.random.RandomState(seed)
    xyz = (rs.rand(B, N, 3) - 0.5).astype(np.float32)
    feat = rs.randn(B, N, 64).astype(np.float32)
    xyz_p, feat_p = xyz.copy(), feat.copy()
    xyz_p[1] = _poison(xyz[1], kind, k, np.random.RandomState(seed + 1))
    feat_p[1] = _poison(feat[1], kind, k, np.random.RandomState(seed + 2))

    def dev_set(xyz_, feat_):
        x4 = dev(torch.from_numpy(np.concatenate((xyz_, (xyz_ ** 2).sum(-1, keepdims=True)), -1)))
        f = dev(torch.from_numpy(feat_))
        sq = (f ** 2).sum(-1).contiguous()
        ft = f.view(B, N, 4, 4, 4).transpose(3, 4).reshape(B, N, 64).contiguous()
        return x4, f, sq, ft

    return dev_set(xyz_p, feat_p), dev_set(xyz, feat), xyz_p[1], feat_p[1]


KNN_SHAPES = [(21, 20), (21, 5), (100, 20), (100, 62), (1024, 5), (1024, 20), (1024, 40), (1343, 20), (1343, 62),
              (2048, 20), (4096, 40)]


@pytest.mark.parametrize("kind", ["nan1", "infpm", "allnan", "kfinite"])
@pytest.mark.parametrize("N,k", KNN_SHAPES)
def test_knn_nonfinite_indices_in_range(nat, N, k, kind):
    """Every kNN launch form -- Cartesian with 1 / 2 / 4 waves per query group, feature space, the fused pair, in-launch slot
    replay, the deferred replay of two launches, and the ordered search from N = 2048 -- on a batch whose cloud 1 holds a
    NaN, a +inf and a -inf, nothing but NaN, or only k finite points: no slot unwritten, every index a row of its cloud,
    a short list padded with the query's own index, the finite queries' sets those of the reference over the finite points,
    and clouds 0 and 2 bit-identical to the clean batch's."""
    seed = N * 7 + k
    (x4, f, sq, ft), (x4c, fc, sqc, ftc), xyz1, feat1 = _clouds(N, k, kind, seed)
    fin3 = np.isfinite(xyz1).all(1)
    fin64 = np.isfinite(feat1).all(1)
    x3_cf, x64_cf = torch.from_numpy(np.ascontiguousarray(xyz1.T)), torch.from_numpy(np.ascontiguousarray(feat1.T))

    def both(run):
        return run(x4, f, sq, ft), run(x4c, fc, sqc, ftc)

    for waves in (0, 1, 2, 4):
        p, c = both(lambda x4_, f_, sq_, ft_: nat.knn(x4_, None, k, waves=waves, prefill=SENT))
        _check_knn(p, c, x3_cf, fin3, k)
    p, c = both(lambda x4_, f_, sq_, ft_: nat.knn(f_, sq_, k, prefill=SENT))
    _check_knn(p, c, x64_cf, fin64, k)
    forms = [dict(), dict(tie_slots=True)]
    for kw in forms:
        p, c = both(lambda x4_, f_, sq_, ft_: nat.knn_pair(f_, sq_, x4_, k, xt=ft_, prefill=SENT, **kw))
        _check_knn(p[0], c[0], x64_cf, fin64, k)
        _check_knn(p[1], c[1], x3_cf, fin3, k)
    p, c = both(lambda x4_, f_, sq_, ft_: nat.knn_pair_deferred(x4_, None, f_, sq_, k, prefill=SENT))
    _check_knn(p[0], c[0], x3_cf, fin3, k)
    _check_knn(p[1], c[1], x64_cf, fin64, k)
    if N >= 2048:
        order = nat.knn_order(x4, ft, sq)
        perm = order["perm"].long().cpu()
        for b in range(perm.shape[0]):                     # a permutation by construction, non-finite coordinates or not
            assert torch.equal(torch.sort(perm[b]).values, torch.arange(N)), b
        order_c = nat.knn_order(x4c, ftc, sqc)
        for kw in forms:
            p = nat.knn_pair(f, sq, x4, k, xt=ft, order=order, prefill=SENT, **kw)
            c = nat.knn_pair(fc, sqc, x4c, k, xt=ftc, order=order_c, prefill=SENT, **kw)
            _check_knn(p[0], c[0], x64_cf, fin64, k)
            _check_knn(p[1], c[1], x3_cf, fin3, k)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- rankselect

def _rank_rows(n, rs):
    rows = []
    base = lambda: rs.randn(n).astype(np.float32)
    r = base(); r[rs.rand(n) < 0.05] = np.nan; rows.append(r)                                   # scattered NaNs
    rows.append(np.full(n, np.nan, np.float32))                                                 # all NaN
    r = base(); r[50:min(140, n)] = np.nan; rows.append(r)                                      # a run across 64-wide windows
    r = base(); r[max(n - 40, 0):] = np.nan; rows.append(r)                                     # a run at the ragged tail
    r = base(); r[rs.rand(n) < 0.1] = np.inf; r[rs.rand(n) < 0.1] = -np.inf; rows.append(r)     # +-inf
    r = rs.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), n); rows.append(r)              # +-0 (and other ties)
    r = rs.choice(np.array([-0.0, 0.0, np.nan, np.inf, -np.inf], np.float32), n); rows.append(r)
    r = base(); r[::7] = np.nan; r[3::11] = -0.0; r[5::13] = np.inf; rows.append(r)
    rows.append(base())                                                                         # clean
    return np.stack(rows)


@pytest.mark.parametrize("n", [700, 64, 130, 5])
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("strided", [False, True])
def test_rankselect_nonfinite_follows_torch_sort(nat, n, largest, strided):
    """order and mask against torch.sort(v, descending=largest, stable=True)[1][:, :K] on the CPU, exactly: NaN above +inf,
    -0 == +0, equal keys in index order; every order slot written once, the mask 0 / 1."""
    rs = np.random.RandomState(n + 3 * largest + strided)
    v = torch.from_numpy(_rank_rows(n, rs))
    want = torch.sort(v, dim=1, descending=largest, stable=True)[1]
    if strided:                                            # one column of a [nb, n, 2] record: element stride 2
        rec = torch.stack((v, torch.full_like(v, 123.0)), -1).cuda()
        vd = rec[:, :, 0]
    else:
        vd = dev(v)
    for K in sorted({n, max(1, n // 2), 1}):
        order, mask = nat.rankselect(vd, K, want_order=True, want_mask=True, largest=largest, prefill=SENT)
        o, m = order.cpu().long(), mask.cpu().long()
        assert not (o == SENT).any(), "an order slot was left unwritten"
        assert ((o >= 0) & (o < n)).all()
        assert all(len(set(r.tolist())) == K for r in o), "ranks collide"
        assert torch.equal(o, want[:, :K]), (K, (o != want[:, :K]).nonzero()[:4])
        wm = torch.zeros(v.shape, dtype=torch.long).scatter_(1, want[:, :K], 1)
        assert torch.equal(m, wm), K


# ---------------------------------------------------------------- pair-score arg-max

@pytest.mark.parametrize("E", [128, 512])
def test_pairscore_argmax_nonfinite_follows_torch(nat, E):
    """op 1's arg-max against torch.argmax of the float64 score matrix: a NaN column (every row: its index), two NaN columns
    (the first), an all-NaN row (0), an all -inf row (0), NaN in streamed tiles that other waves own, split scratch given."""
    rs = np.random.RandomState(E)
    nb, n_own, n_str, scale = 4, 200, 300, 0.05
    own = rs.randn(nb, n_own, E).astype(np.float32)
    st = rs.randn(nb, n_str, E).astype(np.float32)
    st[1, 211, 7] = np.nan                                 # one NaN column
    st[3, 97, 0] = np.nan                                  # two: the first wins
    st[3, 211, 3] = np.nan
    own[2, 5, :] = np.nan                                  # all-NaN row
    st[2, :, 0] = np.abs(st[2, :, 0]) + 0.5
    own[2, 9, 0] = -np.inf                                 # all -inf row
    own[0, 17, 1] = np.nan                                 # an all-NaN row in an otherwise clean sample
    s64 = torch.matmul(torch.from_numpy(own).double(), torch.from_numpy(st).double().transpose(1, 2)) * scale
    want = torch.argmax(s64, dim=-1)
    assert want[2, 9] == 0 and torch.isinf(s64[2, 9]).all()
    for split in (False, True):
        _, amax = nat.pairscore(dev(torch.from_numpy(own).view(-1, E)), dev(torch.from_numpy(st).view(-1, E)), nb, n_own,
                                n_str, op=1, score=1, scale=scale, want_argmax=True, split=split, prefill=SENT)
        got = amax.cpu().long().view(nb, n_own)
        assert not (got == 0x7fffffff).any() and not (got == SENT).any()
        assert ((got >= 0) & (got < n_str)).all()
        special = torch.isnan(s64).any(-1) | torch.isinf(s64).all(-1)
        assert torch.equal(got[special], want[special])
        # clean rows: the fp32 scores may order a near-tie differently; the two picks' float64 scores must then agree closely
        sv = torch.gather(s64, 2, got[..., None])[..., 0]
        wv = torch.gather(s64, 2, want[..., None])[..., 0]
        ok = (got == want) | ((wv - sv).abs() <= 1e-5 * s64.abs().nan_to_num(0, 0, 0).amax())
        assert ok.all(), (~ok).nonzero()[:4]


# ---------------------------------------------------------------- rigid SVD

def test_rigid_svd_nonfinite_pair_is_nan(nat):
    """A pair with a NaN point or an Inf correspondence: R, t, R_ba, t_ba all NaN; the other pairs bit-identical to the clean
    batch (test_rigid_svd's inputs)."""
    rs = np.random.RandomState(0)
    B, K = 6, 300
    src = torch.from_numpy(rs.uniform(-1, 1, (B, 3, K)).astype(np.float32))
    corr = torch.from_numpy(rs.uniform(-1, 1, (B, 3, K)).astype(np.float32)) * 0.3
    ang = rs.uniform(0, 1, B)
    for i in range(B):
        c, s = np.cos(ang[i]), np.sin(ang[i])
        Rz = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float32)
        corr[i] = 0.05 * corr[i] + Rz @ src[i] + torch.tensor([0.1, 0.2, -0.3]).view(3, 1)
    corr[4] = torch.diag(torch.tensor([1.0, 1.0, -1.0])) @ src[4]
    clean = nat.rigid_svd(dev(src.transpose(1, 2)), dev(corr.transpose(1, 2)))
    sp, cp = src.clone(), corr.clone()
    sp[1, 2, 17] = float("nan")
    cp[3, 0, 250] = float("inf")
    sp[5, 1, 0] = float("-inf")
    got = nat.rigid_svd(dev(sp.transpose(1, 2)), dev(cp.transpose(1, 2)))
    torch.cuda.synchronize()
    for g, c in zip(got, clean):
        g, c = g.cpu(), c.cpu()
        for b in range(B):
            if b in (1, 3, 5):
                assert torch.isnan(g[b]).all(), b
            else:
                assert torch.equal(bits(g[b]), bits(c[b])), b


# ---------------------------------------------------------------- the whole forward

def _net(**kw):
    from test_hip_forward import build_net
    mode = kw.pop("_mode", "fp32")
    k = kw.pop("_k", None)
    net, _ = build_net(**kw)
    net.linear_mode = mode
    if k is not None:
        net.emb_nn.k = k
    return net


def _poisoned(src, tgt):
    s, t = src.clone(), tgt.clone()
    s[1, 0, 5] = float("nan")
    t[2, 2, 11] = float("inf")
    return s, t


POSE = (2, 3, 4, 5)


def _compare_pairs(got, ref, bad=(1, 2), B=None, nan=(1, 2)):
    """Per-pair comparison of the forward's outputs (tensors with the pair as the leading dimension; emb: [2, B, ...]): the
    pairs `nan` have all-NaN poses, the other poisoned pairs all-NaN or all-finite ones, the rest equal `ref` bit for bit."""
    for i in POSE:
        for b in bad:
            x = got[i][b]
            assert torch.isnan(x).all() or (b not in nan and torch.isfinite(x).all()), (i, b, x)
    for i, (g, r) in enumerate(zip(got, ref)):
        if not torch.is_tensor(g):
            continue
        if i == 6:                                         # emb [2B*N, E]: src clouds, then tgt clouds
            g, r = g.reshape(2, B, -1).transpose(0, 1), r.reshape(2, B, -1).transpose(0, 1)
        for b in range(B):
            if b not in bad:
                assert torch.equal(bits(g[b]), bits(r[b])), (i, b)


FORWARD_CASES = [
    ("whole1024", dict(), dict(B=4, N=1024)),
    ("whole2048", dict(), dict(B=3, N=2048)),
    ("whole4096k40", dict(_k=40), dict(B=3, N=4096)),
    ("dgcnn", dict(emb_nn="dgcnn"), dict(B=3, N=512)),
    ("bf16x3", dict(_mode="bf16x3+sdpa"), dict(B=3, N=1024)),
]


@pytest.mark.parametrize("name,kw,shape", FORWARD_CASES, ids=[c[0] for c in FORWARD_CASES])
def test_forward_poisoned_pairs_are_nan_and_isolated(name, kw, shape):
    """Whole mode: a NaN in src of pair 1 and an +inf in tgt of pair 2 -- the call returns, the device is healthy, both poses
    are all NaN, and every other pair's outputs (embeddings included) are bit-identical to the clean batch's.  The pooled
    workspace pre-filled with NaN or with zeros gives the same bits."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import synth
    net = _net(**kw)
    B, N = shape["B"], shape["N"]
    src, tgt, _, _, _ = synth.make_batch(610, B, N, kind="uniform" if N > 2048 else "object")
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    sp, tp = _poisoned(s, t)
    with torch.no_grad():
        ref = [o.clone() for o in net._forward_fused(s, t, want_emb=True)]
        torch.cuda.synchronize()
        outs = []
        for fill in (0xFF, 0x00):
            for ws in [b["ws"] for idle in net._shared.pool.values() for b in idle]:
                ws.fill_(fill)
            outs.append([o.clone() for o in net._forward_fused(sp, tp, want_emb=True)])
            torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    _compare_pairs(outs[0], ref, B=B)
    with torch.no_grad():
        out = net(sp, tp)                                  # the nn.Module entry point
    torch.cuda.synchronize()
    for i in POSE:
        assert torch.equal(bits(out[i]), bits(outs[0][i]))


@pytest.mark.parametrize("mode", ["fp32", "bf16x3+sdpa"])
def test_partial_poisoned_pairs_are_nan_and_selections_in_range(mode):
    """Partial mode, N = 768, three device-side iterations: the NaN-poisoned pose NaN, the other pairs bit-identical, every reported
    selection in range (keys / overlap sets: points of the cloud; arg-max / pairs: positions in the overlap sets)."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import synth
    o2 = synth.OVERLAP2_0575
    net = _net(partial=True, overlap2=o2, _mode=mode)
    B, N, iters = 3, 768, 3
    src, tgt, _, _, _ = synth.make_batch(620, B, N, partial=True)
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    N = s.shape[2]
    sp, tp = _poisoned(s, t)
    sizes = net.selection_sizes(N)
    with torch.no_grad():
        ref = net._forward_fused(s, t, iters=iters, want_selections=True)
        torch.cuda.synchronize()
        outs = []
        for fill in (0xFF, 0x00):
            for ws in [b["ws"] for idle in net._shared.pool.values() for b in idle]:
                ws.fill_(fill)
            outs.append(net._forward_fused(sp, tp, iters=iters, want_selections=True))
            torch.cuda.synchronize()
    got = outs[0]
    for a, b in zip(outs[0][:6], outs[1][:6]):
        assert torch.equal(bits(a), bits(b))
    sel = got[6]
    bound = {"keys": N, "sel_src": N, "sel_tgt": N, "argmax": sizes["argmax"], "pairs": sizes["argmax"]}
    for name, x in sel.items():
        x = x.cpu()
        assert ((x >= 0) & (x < bound[name])).all(), (name, x.min().item(), x.max().item())
        assert torch.equal(x, outs[1][6][name].cpu()), name
        r = ref[6][name].cpu()
        rows = [b for b in range(B) if b not in (1, 2)]
        if name == "keys":                                 # [iters, 2B, nkeep]: src clouds, then tgt clouds
            rows = rows + [B + b for b in rows]
        for b in rows:
            assert torch.equal(x[:, b], r[:, b]), (name, b)
    # (the +inf of tgt pair 2 may be pruned before the solve -- DESIGN section 7 --: that pose is then finite, not NaN)
    _compare_pairs(list(got[:6]), list(ref[:6]), B=B, nan=(1,))


@pytest.mark.parametrize("reuse", [False, True])
def test_iter_poisoned_pairs_are_nan(reuse):
    """forward_iter with two passes and vcrnetIter (target reuse on and off): the composed poses of the poisoned pairs are
    NaN, the other pairs bit-identical to the clean batch."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import synth
    from vcrnet_amd.module import vcrnetIter
    net = _net()
    net.iter_reuse = reuse
    B, N = 3, 512
    src, tgt, _, _, _ = synth.make_batch(630, B, N)
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    sp, tp = _poisoned(s, t)
    with torch.no_grad():
        for run in (lambda a, b: net.forward_iter(a, b, 2), lambda a, b: vcrnetIter(net, a, b, iter=3)):
            ref = [o.clone() for o in run(s, t)]
            got = run(sp, tp)
            torch.cuda.synchronize()
            _compare_pairs(list(got), ref, B=B)


# ---------------------------------------------------------------- the module boundary

def _boundary_nets():
    from test_hip_forward import make_args
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd.module import DCP, VCRNet
    nets = {"vcrnet": VCRNet(make_args()), "dcp": DCP(make_args(head="svd")),
            "composed": VCRNet(make_args(n_blocks=2))}
    return {k: v.cuda().eval() for k, v in nets.items()}


BAD_TGT = {
    "n_minus_1": lambda B, N: (B, 3, N - 1),
    "n_plus_1": lambda B, N: (B, 3, N + 1),
    "b_minus_1": lambda B, N: (B - 1, 3, N),
    "rows_tgt": lambda B, N: (B, N, 3),
}


@pytest.mark.parametrize("entry", ["vcrnet", "forward_iter", "dcp", "composed"])
def test_mismatched_clouds_are_refused(entry):
    """tgt with N - 1 / N + 1 points or B - 1 pairs, a [B, N, 3] tensor for either cloud, a 2-D tensor: VcrHipError with a
    message about the shapes, raised before anything is launched."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native
    nets = _boundary_nets()
    net = nets["vcrnet" if entry == "forward_iter" else entry]
    B, N = 2, 64
    src = torch.rand(B, 3, N, device="cuda")
    call = (lambda a, b: net.forward_iter(a, b, 2)) if entry == "forward_iter" else net
    cases = [(src, torch.rand(*f(B, N), device="cuda")) for f in BAD_TGT.values()]
    cases += [(torch.rand(B, N, 3, device="cuda"), src.clone()), (src[0], src[0].clone()), (src, src[0].clone())]
    for a, b in cases:
        with torch.no_grad(), pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]|same B and N"):
            call(a, b)
