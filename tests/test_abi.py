"""CPU-side checks of the drop-in boundary: libvcr_hip.so loads and exports every entry point
include/vcr_hip.h declares; argument validation returns error codes without touching a GPU;
the ctypes structs match the C layout the header implies."""
import ctypes
import os
import re

import pytest

from boundary import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcr_hip.h")
INTERNAL_HEADER = os.path.join(ROOT, "vcr-net_amd", "csrc", "vcr_internal.h")


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, native
    build.build()
    return native.lib()


def declared_symbols(header=None):
    src = open(header or HEADER).read()
    return sorted(set(re.findall(r"\b(vcr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/vcr_hip.h but not exported"


def test_version_and_strerror(lib):
    from vcrnet_amd import native
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27
    assert lib.vcr_strerror(0) == b"ok"
    assert b"invalid" in lib.vcr_strerror(-1)
    assert b"workspace" in lib.vcr_strerror(-2)


def test_ctypes_structs_match_the_c_layout(tmp_path):
    """sizeof + the offset of every field of each args struct, as gcc lays out include/vcr_hip.h, against the ctypes
    mirrors in vcrnet_amd/native.py (a field added on one side only would silently shift everything after it)."""
    import subprocess
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native
    pairs = native.STRUCTS
    # every mirror native.py defines is in the map, or is a member (by value) of a mirror that is
    mirrors = {c for c in vars(native).values() if isinstance(c, type) and issubclass(c, ctypes.Structure)
               and c.__module__ == native.__name__ and not c.__name__.startswith("_")}
    nested = {t for ct in pairs.values() for _, t in ct._fields_ if isinstance(t, type) and issubclass(t, ctypes.Structure)}
    assert mirrors == set(pairs.values()) | nested, sorted(c.__name__ for c in mirrors ^ (set(pairs.values()) | nested))
    hdr = open(HEADER).read()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    expect = []
    for cname, ct in pairs.items():
        body = re.search(r"typedef struct[^{]*\{((?:[^{}]|\{[^{}]*\})*)\}\s*%s;" % cname, hdr)
        assert body, cname
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        expect.append((cname, "sizeof", ctypes.sizeof(ct)))
        for fname, _ in ct._fields_:
            cfield = "in" if fname == "in_" else fname
            lines.append(f'printf("%zu\\n", offsetof({cname}, {cfield}));')
            expect.append((cname, fname, getattr(ct, fname).offset))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(expect)
    bad = [(c, f, e, g) for (c, f, e), g in zip(expect, got) if e != g]
    assert not bad, bad


def test_ctypes_signatures_match_the_header(lib):
    """native.SIGNATURES against the prototypes: PUBLIC names exactly what include/vcr_hip.h declares, INTERNAL what
    csrc/vcr_internal.h declares; per prototype the arity, the return type, every scalar exactly, every struct pointer as
    POINTER of the mirror native.STRUCTS names, every other pointer (and vcr_stream_t) as some pointer-typed parameter.  And
    lib() has applied the table: a restype nobody set would truncate a size_t, a parameter added to the header would go
    unnoticed until a GPU run went wrong."""
    from vcrnet_amd import native
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "float": ctypes.c_float}
    returns = dict(scalars, **{"char*": ctypes.c_char_p})
    pointer_like = lambda t: t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)  # noqa: E731
    assert set(native.SIGNATURES) == set(native.PUBLIC) | set(native.INTERNAL) and not set(native.PUBLIC) & set(native.INTERNAL)
    for header, table in ((HEADER, native.PUBLIC), (INTERNAL_HEADER, native.INTERNAL)):
        protos = prototypes(header)
        assert set(protos) == set(table) == set(declared_symbols(header)), \
            sorted(set(protos) ^ set(table)) + sorted(set(protos) ^ set(declared_symbols(header)))
        for name, (ret, params) in protos.items():
            res, args = table[name]
            assert res is returns[ret], (name, ret, res)
            assert len(args) == len(params), (name, params, args)
            for i, (c, t) in enumerate(zip(params, args)):
                if c in scalars:
                    assert t is scalars[c], (name, i, c, t)
                elif c.startswith("vcr_") and c != "vcr_stream_t":
                    assert c.endswith("*") and not c.endswith("**"), (name, i, c)
                    assert t is ctypes.POINTER(native.STRUCTS[c[:-1]]), (name, i, c, t)
                else:
                    assert c == "vcr_stream_t" or c.endswith("*"), (name, i, c)       # no scalar type this test does not know
                    assert pointer_like(t), (name, i, c, t)
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes or []) == list(args), name
    assert len(native.PUBLIC) == 51 and len(native.INTERNAL) == 6


def test_argument_errors_do_not_need_a_gpu(lib):
    from vcrnet_amd import native
    a = native.LinearArgs()          # all NULL
    assert lib.vcr_linear_f32(ctypes.byref(a), None) == -1
    k = native.KnnArgs()
    assert lib.vcr_knn_f32(ctypes.byref(k), None) == -1
    assert lib.vcr_linear_f32(None, None) == -1
    w = native.VcrnetWeights()
    w.E, w.F, w.heads, w.k = 512, 1024, 4, 20
    n1 = lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 1, 1024)
    n16 = lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 16, 1024)
    assert 0 < n1 < n16 < (4 << 30)
    assert lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 0, 1024) == 0
    # vcrnetIter's bookkeeping step: NULL poses, a cloud without its output, a composition without its destination
    assert lib.vcr_pose_step_f32(None, None) == -1
    ps = native.PoseStepArgs()
    assert lib.vcr_pose_step_f32(ctypes.byref(ps), None) == -1
    ps.R_i, ps.t_i, ps.B, ps.N = 0x1000, 0x2000, 2, 64
    assert lib.vcr_pose_step_f32(ctypes.byref(ps), None) == 0          # nothing asked for: no launch
    ps.in_cf = 0x3000
    assert lib.vcr_pose_step_f32(ctypes.byref(ps), None) == -1
    ps.in_cf, ps.compose = None, 1
    assert lib.vcr_pose_step_f32(ctypes.byref(ps), None) == -1
    ps.compose = 3
    assert lib.vcr_pose_step_f32(ctypes.byref(ps), None) == -1
    # the ordered search's ranking entry point: NULL / missing outputs, then a cloud beyond its 8192 points
    assert lib.vcr_knn_order_f32(None, None) == -1
    o = native.KnnOrderArgs()
    assert lib.vcr_knn_order_f32(ctypes.byref(o), None) == -1
    for f in ("xyz4", "perm", "xyz4_p", "cen4", "cen4_rad", "cen4_sqmax"):
        setattr(o, f, 0x1000)                                # (never dereferenced: the size check comes first)
    o.B, o.N = 2, 9000
    assert lib.vcr_knn_order_f32(ctypes.byref(o), None) == -3 and b"unsupported" in lib.vcr_strerror(-3)
    o.feat_t = 0x2000                                        # features without their norms / outputs
    assert lib.vcr_knn_order_f32(ctypes.byref(o), None) == -1


def test_sized_structs_refuse_what_they_cannot_read(lib):
    """ABI 27: vcr_knn_args / vcr_vcrnet_weights state their size.  Zero (a caller that never heard of the field), less than
    the mandatory part, or more than the library knows is an argument error; a SHORTER struct from an older header is served,
    its missing tail read as zeros -- the library never reads past what the caller said it passed."""
    from vcrnet_amd import native
    w = native.VcrnetWeights()
    assert w.struct_bytes == ctypes.sizeof(native.VcrnetWeights)
    w.E, w.F, w.heads, w.k, w.has_pointer = 512, 1024, 4, 20, 1
    full = lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 4, 1024)
    assert full > 0 and lib.vcr_vcrnet_pairs(ctypes.byref(w), 1024) == 1024
    mandatory = native.VcrnetWeights.fold_encdec_qkv.offset
    w.partial = 1                                            # lives BEHIND the mandatory part ...
    w.overlap2 = 0.75
    assert lib.vcr_vcrnet_pairs(ctypes.byref(w), 1024) < 1024
    w.struct_bytes = mandatory                               # ... so a struct that ends before it is a whole-mode request
    assert lib.vcr_vcrnet_pairs(ctypes.byref(w), 1024) == 1024
    assert lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 4, 1024) == full
    for bad in (0, mandatory - 8, ctypes.sizeof(native.VcrnetWeights) + 8):
        w.struct_bytes = bad
        assert lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 4, 1024) == 0
        assert lib.vcr_vcrnet_pairs(ctypes.byref(w), 1024) == 0
        assert lib.vcr_vcrnet_forward_f32(ctypes.byref(w), None, None, 0, None) == -1
        assert lib.vcr_vcrnet_iter_f32(ctypes.byref(w), None, 1, None, 0, None, None) == -1
    a = native.KnnArgs(0x1000, 4, None, 64, 1024, 4, 20, 0x2000, 0x3000, 64 * 1024)
    assert a.struct_bytes == ctypes.sizeof(native.KnnArgs) and a.N == 1024
    assert lib.vcr_knn_ties_inline(ctypes.byref(a)) == 1
    a.struct_bytes = native.KnnArgs.waves.offset             # the mandatory part alone
    assert lib.vcr_knn_ties_inline(ctypes.byref(a)) == 1
    for bad in (0, native.KnnArgs.waves.offset - 4, ctypes.sizeof(native.KnnArgs) + 8):
        a.struct_bytes = bad
        assert lib.vcr_knn_ties_inline(ctypes.byref(a)) == 0
        assert lib.vcr_knn_f32(ctypes.byref(a), None) == -1
        assert lib.vcr_knn_pair_f32(ctypes.byref(a), ctypes.byref(a), None) == -1
        assert lib.vcr_knn_ties_f32(ctypes.byref(a), None, None) == -1


def test_iter_workspace_adds_the_target_cache_where_it_applies(lib):
    """vcr_vcrnet_iter_workspace_bytes: the forward's workspace + 2 B N x 2560 floats (the four buffers whose target rows persist) for a vcrnetIter loop of more
    than one pass (every embedding and pointer); nothing for one pass or with iter_reuse = 1."""
    from vcrnet_amd import native
    w = native.VcrnetWeights()
    w.E, w.F, w.heads, w.k, w.has_pointer = 512, 1024, 4, 20, 1
    base = lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 24, 768)
    it = lambda n: lib.vcr_vcrnet_iter_workspace_bytes(ctypes.byref(w), 24, 768, n)
    assert it(1) == base and it(2) == it(3) == base + 2 * 24 * 768 * 2560 * 4
    w.iter_reuse = 1
    assert it(3) == base
    w.iter_reuse, w.emb_kind = 0, 1
    assert it(3) == lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 24, 768) + 2 * 24 * 768 * 2560 * 4
    w.emb_kind, w.has_pointer = 0, 2
    assert it(3) == lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), 24, 768) + 2 * 24 * 768 * 2560 * 4
    assert lib.vcr_vcrnet_iter_workspace_bytes(ctypes.byref(w), 24, 768, 0) == 0


def test_workspace_plan_sizes_of_the_baseline_configs(lib):
    """The forward's workspace is laid out by buffer liveness (forward.hip: Plan): pure host arithmetic, so the
    sizes of the BASELINE configs are pinned here -- a buffer registered with too long a life, or the bump allocator coming
    back, shows up as a size regression without a GPU.  (Round 4's bump layout: 1.5 GB at configs[1], ~12 GB at configs[4].)"""
    from vcrnet_amd import native

    def gib(B, N, k=20, merged=True, **kw):
        w = native.VcrnetWeights()
        w.E, w.F, w.heads, w.k, w.has_pointer = 512, 1024, 4, k, 1
        if merged:                                           # (the merged enc + dec first sublayers: never dereferenced here)
            w.fold_encdec_qkv.w = w.fold_encdec_qkv.colsum = w.fold_encdec_qkv.bias = 0x1000
        for f, v in kw.items():
            setattr(w, f, v)
        return lib.vcr_vcrnet_workspace_bytes(ctypes.byref(w), B, N) / 2.0 ** 30

    c1, c1u = gib(16, 1024), gib(16, 1024, merged=False)
    assert 0.5 < c1 < 0.6 and 0.5 < c1u < 0.6, (c1, c1u)     # GiB: nine [M, 512] buffers live at the peak (+ the small ones)
    assert 0.9 < gib(24, 768, partial=1, overlap2=0.75) < 1.25
    assert 1.0 < gib(16, 2048) < 1.35                        # twice configs[1]'s rows
    assert 4.0 < gib(32, 4096, k=40) < 5.3
    sizes = [gib(B, 1024) for B in (1, 2, 4, 8, 16)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] / sizes[0] < 16.5                       # linear in the batch, no per-call constant of note


def test_host_side_dispatch_logic_without_a_gpu(lib):
    """Pure host logic of the round-3 entry points: which kNN calls replay their ties inside the launch, how much
    scratch the replay of long rows needs, the limits that are refused rather than degraded, argument errors of the
    paired linear and the grouped / indexed attention."""
    from vcrnet_amd import native

    def knn_args(B, N, Cc, k, ties=True, waves=0):
        a = native.KnnArgs()
        a.x, a.idx, a.sq = 0x1000, 0x2000, 0x3000            # (never dereferenced on the host)
        a.ldx, a.B, a.N, a.C, a.k, a.waves = Cc, B, N, Cc, k, waves
        if ties:
            a.tie_scratch, a.tie_cap = 0x4000, B * N
        return a
    inline = lambda *a, **k: lib.vcr_knn_ties_inline(ctypes.byref(knn_args(*a, **k)))
    assert inline(32, 1024, 64, 20) == 1 and inline(32, 1024, 4, 20) == 1      # BASELINE configs[1]: both searches
    assert inline(48, 768, 64, 20) == 1 and inline(32, 2048, 64, 20) == 1
    assert inline(64, 4096, 64, 40) == 0 and inline(64, 4096, 4, 40) == 0      # the row image does not fit the workgroup's LDS
    assert inline(2, 1024, 64, 20) == 0                                        # small grid: 32-query kernel, separate replay
    assert inline(32, 1024, 64, 20, waves=1) == 0 and inline(2, 1024, 64, 20, waves=8) == 1
    assert inline(32, 1024, 64, 20, ties=False) == 0
    assert lib.vcr_knn_tie_work_bytes(1024) == 0 and lib.vcr_knn_tie_work_bytes(10091) == 0
    assert lib.vcr_knn_tie_work_bytes(12000) == 64 * 16 * 12000
    a = knn_args(1, 12000, 4, 20)                          # long rows, replay owed, no scratch: refused, not skipped
    assert lib.vcr_knn_f32(ctypes.byref(a), None) == -3
    assert lib.vcr_knn_f32(ctypes.byref(knn_args(4, 1024, 4, 63)), None) == -3 # library limit k <= 62
    assert lib.vcr_knn_f32(ctypes.byref(knn_args(4, 1024, 4, 20, waves=3)), None) == -1
    la = native.LinearArgs()
    assert lib.vcr_linear_pair_f32(ctypes.byref(la), ctypes.byref(la), None) == -1
    la.x, la.w, la.y, la.ldx, la.ldy, la.M, la.N, la.K = 0x1000, 0x2000, 0x3000, 64, 64, 128, 64, 64
    la.variant = 32                                        # a retired selector
    assert lib.vcr_linear_f32(ctypes.byref(la), None) == -1
    sa = native.SdpaArgs()
    sa.q, sa.k, sa.v, sa.out = 0x1000, 0x2000, 0x3000, 0x4000
    sa.ldq = sa.ldk = sa.ldv = sa.ldo = 512
    sa.nbatch, sa.heads, sa.nq, sa.nk, sa.scale = 2, 4, 64, 64, 0.1
    sa.ngroups, sa.rowstat = 2, 0x5000                     # grouped launches: attention-output form only
    assert lib.vcr_sdpa_f32(ctypes.byref(sa), None) == -1
    sa.ngroups, sa.rowstat, sa.key_index, sa.nk_src = 0, None, 0x6000, 0
    assert lib.vcr_sdpa_f32(ctypes.byref(sa), None) == -1  # indexed keys need nk_src


def test_linear_launch_choice_against_the_recorded_sweep(lib):
    """vcr_linear_config (host-only): the kernel configuration per launch.  The BASELINE shapes take what DESIGN says
    (128-row tiles at configs[1]; 96-row tiles for the residual launches of configs[2]; 32-row tiles and the 16x16x4 shape
    for one pair per call), and replayed against the sweep recorded on the GPU (profiles/rounds1-3/r3z_sweep_bm_after.txt: both
    forced heights timed at 56 shapes) the automatic height never loses more than 6 % to the better one."""
    import os
    import re
    from vcrnet_amd import native

    def cfg(M, N, K, residual, variant=0):
        a = native.LinearArgs()
        a.x, a.w, a.y, a.bias = 0x1000, 0x2000, 0x3000, 0x4000            # (never dereferenced on the host)
        a.ldx, a.ldy, a.M, a.N, a.K, a.variant = K, N, M, N, K, variant
        if residual:
            a.residual, a.ldr, a.stats_out = 0x5000, N, 0x6000
        c = lib.vcr_linear_config(ctypes.byref(a))
        assert c > 0, c
        return c & 0xFF, (c >> 8) & 0xFF, bool(c & (1 << 16))
    assert cfg(32768, 512, 512, True) == (128, 32, True) and cfg(32768, 1536, 512, False) == (128, 16, False)     # configs[1]
    assert cfg(36864, 512, 512, True) == (96, 32, True) and cfg(36864, 512, 1024, True) == (96, 32, True)          # configs[2]
    assert cfg(36864, 1024, 512, False) == (128, 16, False)                                                          # (BK 16: no)
    assert cfg(2048, 512, 512, True) == (32, 32, True) and cfg(2048, 512, 512, False) == (32, 32, True)            # one pair
    assert cfg(2048, 3072, 512, False)[0] in (64, 128) and cfg(2048, 3072, 512, False)[2]
    assert cfg(8192, 512, 512, True) == (128, 32, True)               # 256 tiles: exactly one per CU (the first model took 96: -34 %)
    assert cfg(32768, 512, 512, True, variant=2048)[0] == 96 and cfg(2048, 512, 512, True, variant=4096 | 16)[0] == 128
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rounds1-3", "r3z_sweep_bm_after.txt")
    worst, n = 0.0, 0
    for line in open(path):
        m = re.match(r"K=(\d+) M=\s*(\d+) tiles128=\s*\d+: auto\s+[\d.]+\s+bm128\s+([\d.]+)\s+bm96\s+([\d.]+)", line)
        if not m:
            continue
        K, M, t128, t96 = int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4))
        if M < 16384:
            continue                                              # (small problems may take 64 / 32 rows: not in this sweep)
        rows = cfg(M, 512, K, True)[0]
        assert rows in (96, 128)
        worst, n = max(worst, (t96 if rows == 96 else t128) / min(t96, t128) - 1), n + 1
    assert n >= 30 and worst <= 0.06, (n, worst)


def test_sdpa_launch_form_of_the_quoted_shapes(lib):
    """vcr_sdpa_forms_ (host-only, library-internal): what sdpa_plan makes of the attention launches DESIGN and the tests quote,
    on 256 CUs -- MI355X's count, and the one the library assumes without a GPU."""
    from vcrnet_amd import native

    def form(nb, nq, nk, out=True, groups=1, split_floats=0, key_index=False):
        a = native.SdpaArgs()
        a.q, a.k, a.v = 0x1000, 0x2000, 0x3000                # (never dereferenced on the host)
        a.ldq = a.ldk = a.ldv = a.ldo = 512
        a.nbatch, a.heads, a.nq, a.nk, a.scale = nb, 4, nq, nk, 128 ** -0.5
        if out:
            a.out = 0x4000
        else:                                                # statistics pass: (max, sum) rows and the kept scores
            a.rowstat, a.score_out, a.ld_score = 0x5000, 0x6000, (nk + 31) & ~31
        if groups > 1:
            a.ngroups, a.q_group_stride = groups, 1536
            a.k_group_stride = a.v_group_stride = a.out_group_stride = 1536
        if split_floats:
            a.split_work, a.split_work_floats = 0x7000, split_floats
        if key_index:
            a.key_index, a.nk_src = 0x8000, nk
        nsplit, persist = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.vcr_sdpa_forms_(ctypes.byref(a), ctypes.byref(nsplit), ctypes.byref(persist))
        return rc, nsplit.value, persist.value
    # configs[2] cross-attention statistics pass, 48 x 4 heads x 768: 1152 workgroups on 512 slots -> four key runs each
    assert form(48, 768, 768, out=False, split_floats=4 * 48 * 4 * 768 * 2) == (0, 4, 0)
    # configs[1] grouped self-attention, 2 groups x 32 x 1024: 2048 items, the persistent kernel, no split
    assert form(32, 1024, 1024, groups=2) == (0, 1, 1)
    # an attention-output launch of 2 x 1024 (64 workgroups) with planes for every split: split
    assert form(2, 1024, 1024, split_floats=4 * (2 * 1024 * 512 + 2 * 4 * 1024 * 2)) == (0, 4, 0)
    # the key-index form holds its list in LDS: 16 384 kept keys at most
    assert form(2, 1024, 16384, key_index=True) == (0, 1, 0)
    assert form(2, 1024, 16385, key_index=True)[0] == -1


def test_linear_pair_launch_form_of_the_quoted_shapes(lib):
    """vcr_linear_forms_ (host-only, library-internal): what linear_plan makes of the paired linear launches DESIGN and the
    tests quote, on 256 CUs -- whether the two halves are one launch, and per half (LDS-DMA family, tile rows, k-slab, MFMA
    shape, grid[, dynamic LDS bytes]).  K = 512; "res" = a residual and stats_out on that half."""
    from vcrnet_amd import native

    def half(M, N, res=False, stats=None, variant=0):
        a = native.LinearArgs()
        a.x, a.w, a.y, a.bias = 0x1000, 0x2000, 0x3000, 0x4000            # (never dereferenced on the host)
        a.ldx, a.ldy, a.M, a.N, a.K, a.variant = 512, N, M, N, 512, variant
        if res:
            a.residual, a.ldr = 0x5000, N
        if res if stats is None else stats:
            a.stats_out = 0x6000
        return a

    def forms(a, b=None, lds=True):
        one, fa, fb = ctypes.c_int(-1), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
        assert lib.vcr_linear_forms_(ctypes.byref(a), ctypes.byref(b) if b is not None else None, ctypes.byref(one), fa, fb) == 0

        def short(f):                                            # (family, rows, k-slab, shape, grid[, LDS])
            return (f[0], f[1], f[2], f[3], f[4] * f[5]) + ((f[6],) if lds else ())
        return (one.value, short(fa), short(fb)) if b is not None else short(fa)
    res = lambda M, N=512, **kw: half(M, N, res=True, **kw)      # noqa: E731
    # configs[1] / configs[2]: the encoder's and the decoder's output projections side by side
    assert forms(res(32768), res(32768)) == (1, (1, 128, 32, 16, 1024, 65536), (1, 128, 32, 16, 1024, 65536))
    assert forms(res(36864), res(36864)) == (1, (1, 96, 32, 16, 1536, 57344), (1, 96, 32, 16, 1536, 57344))
    # configs[1] ffn1 | cross.q: one launch on the BK 16 kernel ... whose second half, alone, takes the one-round rule
    assert forms(half(32768, 1024), half(16384, 512)) == (1, (1, 128, 16, 32, 2048, 34816), (1, 128, 16, 32, 512, 34816))
    assert forms(half(16384, 512), lds=False) == (1, 128, 32, 16, 512)
    # a residual beside none: two launches, the second as it goes alone (the one-round rule)
    assert forms(res(32768), half(32768, 512), lds=False) == (0, (1, 128, 32, 16, 1024), (1, 128, 32, 16, 1024))
    # one pair per call: heights from the combined grid
    assert forms(res(2048), res(2048)) == (1, (1, 64, 32, 16, 128, 49152), (1, 64, 32, 16, 128, 49152))
    assert forms(half(2048, 1024), half(1024, 512), lds=False) == (1, (1, 128, 16, 16, 128), (1, 128, 16, 16, 32))
    assert forms(res(2048), res(32768), lds=False) == (1, (1, 96, 32, 16, 88), (1, 96, 32, 16, 1368))
    assert forms(res(14336), res(14336), lds=False) == (1, (1, 96, 32, 16, 600), (1, 96, 32, 16, 600))
    assert forms(res(16384), res(16384), lds=False) == (1, (1, 128, 32, 16, 512), (1, 128, 32, 16, 512))
    # N = 510: the register-staged fallback (2 x TileT<32> of LDS) beside an LDS-DMA launch -- two launches
    assert forms(half(3000, 510), half(3000, 512)) == (0, (0, 128, 32, 32, 96, 73728), (1, 64, 32, 16, 188, 49152))
    # forced heights hold for the pair
    assert forms(res(3000, variant=2048), res(3077, 256, variant=2048), lds=False) == (1, (1, 96, 32, 16, 128), (1, 96, 32, 16, 66))
    assert forms(res(3000, variant=8192), half(3077, 256, stats=True, variant=8192), lds=False) == \
        (1, (1, 64, 32, 16, 188), (1, 64, 32, 16, 98))


def test_edgeconv_launch_form_of_the_quoted_shapes(lib):
    """vcr_edgeconv_forms_ (host-only, library-internal): what edgeconv_check / edgeconv_plan make of the EdgeConv launches
    DESIGN and the tests quote, on 256 CUs: (code, form, grid) with form 0 = padded, 1 = packed, 2 = the hand-scheduled packed
    kernel, 3 = bf16x3."""
    from vcrnet_amd import native

    def form(M, N, k, bf16x3=False, pq=0x10000, b2=0x40000, x2=0x60000, ldx2=128):
        a = native.EdgeconvArgs(pq, 256, 0x20000, k, M, N, 0x30000, b2, 0x50000, 128, x2, ldx2)   # (never dereferenced on the host)
        f, g = ctypes.c_int(-1), ctypes.c_int(-1)
        return lib.vcr_edgeconv_forms_(ctypes.byref(a), int(bf16x3), ctypes.byref(f), ctypes.byref(g)), f.value, g.value
    PADDED, PACKED, PIPE, BF16X3 = 0, 1, 2, 3
    assert form(32768, 1024, 20) == (0, PIPE, 512)           # configs[1]: 4096 groups on 2 x 256 slots
    assert form(8192, 4096, 40) == (0, PIPE, 512)            # configs[4]: 2048 groups
    assert form(74, 37, 20) == (0, PIPE, 10) and form(74, 37, 40) == (0, PIPE, 19)      # fewer groups than slots: one each
    assert form(74, 37, 20, x2=0x60004) == (0, PACKED, 10) and form(74, 37, 20, ldx2=130) == (0, PACKED, 10)
    assert form(74, 37, 20, b2=0x40004) == (0, PACKED, 10)
    assert form(192, 96, 7) == (0, PADDED, 192) and form(140, 70, 33) == (0, PADDED, 140)   # min(M, 2048)
    assert form(4096, 1024, 7) == (0, PADDED, 2048) and form(4096, 1024, 33) == (0, PADDED, 2048)
    assert form(4096, 1024, 65) == (-1, -1, -1)
    assert form(32768, 1024, 20, bf16x3=True) == (0, BF16X3, 1024) and form(600, 300, 20, bf16x3=True) == (0, BF16X3, 75)
    assert form(406, 203, 7, bf16x3=True) == (-3, -1, -1)    # no static row -> point map: VCR_EUNSUPPORTED
    assert form(600, 300, 20, bf16x3=True, pq=0x10004) == (-1, -1, -1)
    assert lib.vcr_edgeconv_forms_(None, 0, None, None) == -1


def test_gathermax_launch_form_of_the_quoted_shapes(lib):
    """vcr_gathermax_forms_ (host-only, library-internal): what gathermax_check / gathermax_plan make of the shapes of
    test_gathermax_lds_and_l2_paths_are_exact and of the limits DESIGN quotes: (code, form, channel slice, grid, LDS bytes)
    with form 0 = gathers through L2 (one wave per point), 1 = out of LDS (one workgroup per cloud and slice, N x (slice + 4)
    floats)."""
    from vcrnet_amd import native

    def form(B, N, k=20, C=256, variant=0, idx=0x20000):
        a = native.GathermaxArgs(0x10000, 2 * C, C, idx, k, B * N, N, 0x30000, C, variant, None)
        o = [ctypes.c_int(-1) for _ in range(4)]
        return (lib.vcr_gathermax_forms_(ctypes.byref(a), *[ctypes.byref(x) for x in o]),) + tuple(x.value for x in o)
    L2, LDS, REFUSED, INVALID = 0, 1, (-3, -1, -1, -1, -1), (-1, -1, -1, -1, -1)
    assert form(32, 1024) == (0, LDS, 32, 256, 147456) and form(48, 768) == (0, LDS, 32, 384, 110592)
    assert form(24, 1000, k=40) == (0, LDS, 32, 192, 144000)          # 192 workgroups exactly
    assert form(32, 1066) == (0, LDS, 32, 256, 153504)                # the last N whose 32-channel slice fits 150 KB
    assert form(32, 1067) == (0, LDS, 16, 512, 85360)
    assert form(4, 1024) == (0, L2, 0, 1024, 0)                       # 32 workgroups: the L2 gathers, four points each
    assert form(64, 333, C=96) == (0, LDS, 32, 192, 47952) and form(200, 64, C=32) == (0, LDS, 32, 200, 9216)
    assert form(32, 2048) == (0, LDS, 16, 512, 163840)                # the last N whose 16-channel slice fits a CU's 160 KB
    assert form(32, 2049) == (0, L2, 0, 16392, 0)
    # forced forms: any grid size; refused when the slice of one cloud does not fit, unknown values are argument errors
    assert form(32, 1024, variant=32) == (0, LDS, 32, 256, 147456) and form(4, 1024, variant=32) == (0, LDS, 32, 32, 147456)
    assert form(32, 1067, variant=32) == (0, LDS, 32, 256, 153648) and form(32, 2049, variant=32) == REFUSED
    assert form(32, 1024, variant=16) == (0, LDS, 16, 512, 81920) and form(32, 2049, variant=16) == REFUSED
    assert form(32, 1024, variant=8) == (0, LDS, 8, 1024, 49152) and form(32, 2049, variant=8) == (0, LDS, 8, 1024, 98352)
    assert form(32, 1024, variant=1) == (0, L2, 0, 8192, 0) and form(32, 2049, variant=1) == (0, L2, 0, 16392, 0)
    assert form(32, 1024, variant=5) == INVALID and form(4, 1024, variant=5) == INVALID
    # the LDS form's 16-B index loads need an aligned list, and a k of 20 / 40
    assert form(32, 1024, idx=0x20004) == (0, L2, 0, 8192, 0) and form(32, 1024, idx=0x20004, variant=32) == REFUSED
    assert form(32, 1024, k=7) == (0, L2, 0, 8192, 0) and form(32, 1024, k=7, variant=16) == REFUSED
    assert lib.vcr_gathermax_forms_(None, None, None, None, None) == -1


def test_module_contract_on_cpu():
    """Constructor / state-dict contract of the reference module without a GPU."""
    from types import SimpleNamespace
    import torch
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import weights
    from vcrnet_amd.module import VCRNet
    args = SimpleNamespace(emb_dims=512, cycle=False, emb_nn="lpdnet", pointer="transformer", vcp_nn="topK",
                           partial=False, overlap2=0.75, t3d=False, tfea=False, n_blocks=1, dropout=0.0,
                           ff_dims=1024, n_heads=4)
    net = VCRNet(args)
    keys = set(net.state_dict().keys())
    assert keys == set(weights.param_shapes().keys())
    assert len(keys) == 59 and sum(p.numel() for p in net.parameters()) == 5625161
    w = weights.generate_weights(1234, lpd=weights.load_lpd_fixture())
    net.load_state_dict({"module." + k: v for k, v in w.items()}, strict=True)   # DataParallel-saved checkpoint
    assert torch.equal(net.emb_nn.conv3_lpd.weight, w["emb_nn.conv3_lpd.weight"])
    # attributes util/initPara.py:38-65 touches
    assert hasattr(net.emb_nn, "convDG1") and net.emb_nn.negative_slope == 0.0
    assert any(isinstance(m, torch.nn.Conv2d) for m in net.emb_nn.modules())
    assert not hasattr(net.head, "linears_emb")
    assert net._get_name() == "VCRNet"
    with pytest.raises(Exception):
        VCRNet(SimpleNamespace(**{**vars(args), "emb_nn": "nope"}))
    with pytest.raises(Exception):
        VCRNet(SimpleNamespace(**{**vars(args), "vcp_nn": "nope"}))
    net.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):   # no CPU fallback by design
        net(torch.zeros(1, 3, 64), torch.zeros(1, 3, 64))


def test_cpp_host_example_builds_and_refuses_a_foreign_file(lib, tmp_path):
    """examples/host_cpp/forward_host.cpp (the C-ABI from C++ without Python) compiles against the header and links the library;
    without a GPU it can still be asked to read a file that is not a model blob."""
    import subprocess
    from vcrnet_amd import build
    exe = build.build_host_example()
    bad = tmp_path / "not_a_blob.bin"
    bad.write_bytes(b"\0" * 256)
    r = subprocess.run([exe, str(bad), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 2 and "not a VCRB blob" in r.stderr
    assert subprocess.run([exe], capture_output=True, text=True).returncode == 2      # usage
