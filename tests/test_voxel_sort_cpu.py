"""The voxel grid by a radix sort, without a GPU: the boundary of include/vcr_hip_voxel_sort.h (prototypes against
vcrnet_amd.voxel_sort.SIGNATURES, vcr_voxel_sort_args against gcc's layout, the exported symbols, the other headers where they
were), the argument errors, the form and the workspace against the header's formula, the resource remarks of voxel_sort.hip, and
the numpy restatement of the ROUTE (tests/voxel_sort_restated.py: packed widths, stable digit passes, heads, ranks of the
representatives, ordered sums, member lists) against the definition (tests/voxel_restated.py), bit for bit -- also on clouds
whose sums depend on their order, which a sort that is not stable would get wrong."""
import ctypes
import inspect
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import boundary
import voxel_restated as vr
import voxel_sort_restated as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_voxel_sort.h")
OTHERS = ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h", "vcr_hip_voxel.h", "vcr_hip_outlier.h",
          "vcr_hip_gicp.h", "vcr_hip_fpfh.h", "vcr_hip_match.h", "vcr_hip_fgr.h", "vcr_hip_grid.h", "vcr_hip_gridnn.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_voxel_sort_workspace_bytes", "vcr_voxel_sort_f32", "vcr_voxel_sort_form"}
PER_LANE = {4: 4, 8: 4, 11: 8}                              # digit width -> elements per lane
PLAN_BITS = 11


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, voxel_sort
    build.build()
    return voxel_sort.lib()


# ---------------------------------------------------------------------------------------------------------------- the boundary

def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import voxel_sort
    boundary.check_signatures(HEADER, voxel_sort, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import voxel, voxel_sort
    assert set(voxel_sort.NEW_STRUCTS) == {"vcr_voxel_sort_args"}
    boundary.check_layout(HEADER, types.SimpleNamespace(STRUCTS=voxel_sort.NEW_STRUCTS), tmp_path)
    assert ctypes.sizeof(voxel_sort.VoxelSortArgs) == 24
    assert voxel_sort.STRUCTS["vcr_voxel_args"] is voxel.VoxelArgs           # (the scan form's own mirror, unchanged)
    boundary.check_layout(os.path.join(INCLUDE, "vcr_hip_voxel.h"), voxel, tmp_path)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The calls live beside the twelve headers, not in them: none mentions them, ABI 27, the same 51 prototypes; the new header
    is taken into the digests through a list of its own."""
    from vcrnet_amd import build, fgr, fpfh, gicp, grid, gridnn, match, native, outlier, plane, refine, score, voxel, voxel_sort
    for h in OTHERS:
        assert "voxel_sort" not in open(os.path.join(INCLUDE, h)).read(), h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    for other in (native, score, refine, plane, voxel, outlier, gicp, fpfh, match, fgr, grid, gridnn):
        assert not set(voxel_sort.SIGNATURES) & set(other.SIGNATURES)
        assert not set(voxel_sort.NEW_STRUCTS) & set(other.STRUCTS)
    assert not set(voxel_sort.SIGNATURES) & set(native.PUBLIC)
    assert build.VOXEL_SORT_HEADERS == [HEADER] and build.GRIDNN_HEADERS == [os.path.join(INCLUDE, "vcr_hip_gridnn.h")]
    full = build.sources_sha16()
    monkeypatch.setattr(build, "VOXEL_SORT_HEADERS", [])
    assert build.sources_sha16() != full


# ---------------------------------------------------------------------------------------------------------------- refusals

def _args(B=2, N=1000, h=0.1, variant=0):
    from vcrnet_amd import voxel
    a = voxel.VoxelArgs()
    a.xyz, a.points, a.count = 0x1000, 0x2000, 0x3000      # (never dereferenced on the host)
    a.B, a.N, a.voxel_size, a.variant = B, N, h, variant
    return a


def _s(bits=0):
    from vcrnet_amd import voxel_sort
    return voxel_sort.VoxelSortArgs(bits, None, None)


def _codes(lib, a, s, ws=0x10000, n=1 << 40):
    """The three entry points agree on a refusal: its code, its code, 0 bytes."""
    aa, ss = None if a is None else ctypes.byref(a), None if s is None else ctypes.byref(s)
    rc = lib.vcr_voxel_sort_f32(aa, ss, ws, n, None)
    assert lib.vcr_voxel_sort_workspace_bytes(aa, ss, 256) == 0
    assert lib.vcr_voxel_sort_form(aa, ss, 256, None, None, None) == rc
    return rc


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import voxel, voxel_sort
    assert _codes(lib, None, _s()) == EINVAL and _codes(lib, _args(), None) == EINVAL
    assert lib.vcr_voxel_sort_form(ctypes.byref(_args()), ctypes.byref(_s()), 256, None, None, None) == 0
    for field in ("xyz", "points", "count"):
        a = _args()
        setattr(a, field, None)
        assert _codes(lib, a, _s()) == EINVAL, field
    for variant in (1, 2, voxel.variant(2), 1 | voxel.variant(128), -1):              # the scan's forms do not apply
        assert _codes(lib, _args(variant=variant), _s()) == EINVAL, variant
    for bits in (1, 2, 3, 5, 7, 9, 10, 12, 16, -8, 0x108):                               # an unknown digit width
        assert _codes(lib, _args(), _s(bits)) == EINVAL, bits
    for kw in (dict(B=0), dict(B=-2), dict(h=0.0), dict(h=-0.5), dict(h=float("nan")), dict(h=float("inf")), dict(h=-float("inf"))):
        assert _codes(lib, _args(**kw), _s()) == EINVAL, kw
    for kw in (dict(N=0), dict(N=-4), dict(N=131073), dict(N=131072, B=16384)):
        assert _codes(lib, _args(**kw), _s()) == EUNSUPPORTED, kw
    assert lib.vcr_voxel_sort_form(ctypes.byref(_args(N=131072, B=16383)), ctypes.byref(_s()), 256, None, None, None) == 0
    assert lib.vcr_voxel_sort_form(ctypes.byref(_args()), ctypes.byref(_s()), -1, None, None, None) == EINVAL
    # struct_bytes of either struct: unsized, short of its mandatory part, longer than the library knows
    for bad in (0, voxel.VoxelArgs.point_voxel.offset - 4, ctypes.sizeof(voxel.VoxelArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert _codes(lib, a, _s()) == EINVAL, bad
    size = ctypes.sizeof(voxel_sort.VoxelSortArgs)
    for bad in (0, 4, size + 8):
        s = _s()
        s.struct_bytes = bad
        assert _codes(lib, _args(), s) == EINVAL, bad
    s = _s(11)
    s.struct_bytes = voxel_sort.VoxelSortArgs.members.offset                             # the mandatory part alone is served
    bits = ctypes.c_int(0)
    assert lib.vcr_voxel_sort_form(ctypes.byref(_args()), ctypes.byref(s), 256, ctypes.byref(bits), None, None) == 0
    assert bits.value == 11
    # the workspace: missing, misaligned, one byte short
    a, s = _args(), _s()
    need = lib.vcr_voxel_sort_workspace_bytes(ctypes.byref(a), ctypes.byref(s), 0)
    assert need == lib.vcr_voxel_sort_workspace_bytes(ctypes.byref(a), ctypes.byref(s), 256) > 0
    f32 = lambda ws, n: lib.vcr_voxel_sort_f32(ctypes.byref(a), ctypes.byref(s), ws, n, None)      # noqa: E731
    assert f32(None, 1 << 40) == EINVAL and f32(0x10004, 1 << 40) == EINVAL and f32(0x10008, 1 << 40) == EINVAL
    assert f32(0x10000, need - 1) == EWORKSPACE and f32(0x10000, 0) == EWORKSPACE


# ---------------------------------------------------------------------------------------------------------------- plan, remarks

def workspace_formula(B, N, d, e):
    """The header's: up(64 B) + up(4 B) + up(24 B nt) + 2 up(8 B N) + 2 up(4 B N) + up(4 B R nt) + up(4 B R) + 5 up(4 B N)
    + 2 up(4 B nb)."""
    up = lambda v: (v + 255) // 256 * 256                                          # noqa: E731
    R, nt, nb = 1 << d, -(-N // (256 * e)), -(-N // 256)
    return (up(64 * B) + up(4 * B) + up(24 * B * nt) + 2 * up(8 * B * N) + 2 * up(4 * B * N) + up(4 * B * R * nt) + up(4 * B * R)
            + 5 * up(4 * B * N) + 2 * up(4 * B * nb))


def test_the_form_and_the_workspace_are_the_headers(lib):
    from vcrnet_amd import voxel_sort
    assert voxel_sort.DIGIT_BITS == tuple(PER_LANE)
    for B, N in [(1, 1), (1, 5), (1, 257), (16, 1024), (16, 16384), (1, 70001), (1, 131072), (3, 700), (256, 16384)]:
        for force in (0,) + voxel_sort.DIGIT_BITS:
            for cu in (256, 1, 0):
                d, passes, e, ws = voxel_sort.voxel_sort_form(B, N, digit_bits=force, cu_count=cu)
                assert d == (force or PLAN_BITS) and e == PER_LANE[d] and passes == -(-64 // d), (B, N, force)
                assert ws == workspace_formula(B, N, d, e), (B, N, force)
    for B, N in ((1, 0), (1, 131073), (16384, 131072)):
        with pytest.raises(Exception):
            voxel_sort.voxel_sort_form(B, N)


def test_the_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """hipcc's remarks for voxel_sort.hip: no scratch, no spill anywhere; the scatter of the plan's width (11 bits: four counters
    of 2 048 digits, 32 KB of LDS) and the means kernel (its wave stage) at four waves a SIMD or more, the 8-bit scatter within
    64 VGPRs and a few KB of LDS at eight."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: res[n]
            for n, d in zip(names, dem) if res[n]["file"] == "voxel_sort.hip"}
    assert set(mine) == {
        "vs_bounds_kernel<4>", "vs_bounds_kernel<8>", "vs_fold_kernel", "vs_keys_kernel", "vs_heads_kernel", "vs_count_kernel",
        "vs_offsets_kernel", "vs_rank_kernel", "vs_means_kernel", "vs_mstart_kernel", "vs_members_kernel",
        "rs_hist_kernel<4, 4>", "rs_hist_kernel<8, 4>", "rs_hist_kernel<11, 8>", "rs_scan_kernel<4>", "rs_scan_kernel<8>",
        "rs_scan_kernel<11>", "rs_scatter_kernel<4, 4>", "rs_scatter_kernel<8, 4>", "rs_scatter_kernel<11, 8>"}
    for d, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
    plan, narrow = mine["rs_scatter_kernel<11, 8>"], mine["rs_scatter_kernel<8, 4>"]
    assert plan["occupancy"] >= 4 and plan["vgprs"] <= 96 and plan["lds"] <= 33 * 1024, plan
    assert narrow["occupancy"] == 8 and narrow["vgprs"] <= 64 and narrow["lds"] <= 4 * 1024 + 64, narrow
    assert mine["vs_means_kernel"]["occupancy"] >= 4 and mine["vs_means_kernel"]["lds"] <= 8 * 1024, mine["vs_means_kernel"]
    for d in ("rs_hist_kernel<8, 4>", "rs_hist_kernel<11, 8>", "rs_scan_kernel<11>", "vs_keys_kernel", "vs_heads_kernel", "vs_members_kernel"):
        assert mine[d]["occupancy"] == 8, (d, mine[d])
    text = open(os.path.join(ROOT, "vcr-net_amd", "csrc", "radix_sort.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert code.count("atomicAdd") == 1 and "atomicAdd(&h[" in code           # the histogram's LDS count, and no other atomic
    assert "while" not in code                                                  # no wait of any kind


# ---------------------------------------------------------------------------------------------------------------- the route

@pytest.fixture(scope="module")
def cases():
    """name -> (xyz, h, the definition's result with the member lists by their definition), every recipe below 70 001 points."""
    out = {}
    for name, make in vr.RECIPES.items():
        xyz, h = make()
        if xyz.shape[2] < 70001:
            out[name] = (xyz, h, vs.with_member_lists(vr.batch(xyz, h)))
    return out


@pytest.mark.parametrize("bits", [4, 8, 11])
def test_the_route_returns_the_definitions_bits(cases, bits):
    assert len(cases) == len(vr.RECIPES) - 2
    for name, (xyz, h, want) in cases.items():
        assert vs.same(vs.batch(xyz, h, bits), want), name


def test_the_recipes_span_the_key_widths(cases):
    """W = 0, a few bits, 54 and the full 63; a cloud too fine beside them."""
    def W(name, b=0):
        w = vs.widths(cases[name][0][b], cases[name][1])[2]
        return None if w is None else sum(w)
    assert W("n1") == 0 and W("one_voxel_1025") == 0 and 6 <= W("n256") <= 12 and 6 <= W("three_clouds") <= 12
    assert W("own_voxel") == 54 and W("fine_batch", 2) == 63 and W("fine_batch", 1) is None and W("all_nan") is None
    assert [vs.passes_needed(63, d) for d in (4, 8, 11)] == [16, 8, 6] and vs.passes_needed(0, 8) == 1


def test_the_member_lists_are_their_definition(cases):
    """voxel v's members are the points with point_voxel == v, ascending; the voxels follow each other; -1 / the number of
    finite points behind them; -1 and 0 throughout for a cloud too fine or without a finite point."""
    for name, (xyz, h, want) in cases.items():
        got = vs.batch(xyz, h, 8)
        for b in range(len(xyz)):
            M, pv, mem, start = int(got["count"][b]), got["point_voxel"][b], got["members"][b], got["voxel_start"][b]
            if M <= 0:
                assert (mem == -1).all() and (start == 0).all(), name
                continue
            nf = int((pv >= 0).sum())
            assert (mem[nf:] == -1).all() and (start[M:] == nf).all(), name
            ends = np.concatenate([start[1:M], [nf]])
            for v in (0, M // 2, M - 1):
                assert np.array_equal(mem[start[v]:ends[v]], np.flatnonzero(pv == v)), (name, v)
            assert np.array_equal(ends - start[:M], got["voxel_points"][b][:M]), name


# (N, seed) at which shuffling the window of 64 sorted slots at N / 2 - 32 changes the voxel's bits -- found by trying seeds
ORDER_CASES = [(513, 0), (1000, 4), (3000, 5), (5000, 12)]


@pytest.mark.parametrize("N,seed", ORDER_CASES)
def test_a_sum_whose_order_shows(N, seed):
    """One voxel of edge 2^63 whose members cancel: a window of the sorted order shuffled -- what a pass that is not stable
    would leave -- changes the mean's bits; the route returns the definition's.  The same cloud as two interleaved voxels."""
    xyz = vs.cancelling(seed, N)
    want = vs.with_member_lists(vr.batch(xyz, vs.CANCEL_H, vr.voxel_loop))
    assert want["count"][0] == 1 and want["voxel_points"][0, 0] == N
    for bits in (4, 8, 11):
        assert vs.same(vs.batch(xyz, vs.CANCEL_H, bits), want), bits
    shuffled = vs.voxel_sort(xyz[0], vs.CANCEL_H, disturb=vs.shuffle_window(1, N // 2 - 32))
    assert not np.array_equal(vr.bits(shuffled["points"]), vr.bits(want["points"][0]))
    assert np.array_equal(shuffled["point_voxel"], want["point_voxel"][0])
    xyz = vs.interleaved(seed, N)
    want = vs.with_member_lists(vr.batch(xyz, vs.CANCEL_H, vr.voxel_loop))
    assert want["count"][0] == 2 and (want["point_voxel"][0] == np.arange(N) % 2).all()
    for bits in (4, 8, 11):
        assert vs.same(vs.batch(xyz, vs.CANCEL_H, bits), want), bits


# ---------------------------------------------------------------------------------------------------------------- Python

def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import module, native, voxel, voxel_sort
    a = torch.zeros(2, 3, 300)
    assert inspect.signature(voxel.voxel_down_sample).parameters["method"].default == "scan"
    assert inspect.signature(module.register_sampled).parameters["voxel_method"].default == "scan"
    with pytest.raises(native.VcrHipError, match='method must be "scan" or "sort"'):
        vcrnet_amd.voxel_down_sample(a, 0.1, method="hash")
    with pytest.raises(native.VcrHipError, match='voxel_method must be "scan" or "sort"'):
        module.register_sampled(None, a, a, 64, voxel=0.1, voxel_method="hash")
    for call in (lambda: vcrnet_amd.voxel_down_sample(a, 0.1, method="sort"), lambda: voxel_sort.voxel_down_sample_and_trace(a, 0.1)):
        with pytest.raises(native.VcrHipError, match="no CPU fallback"):
            call()
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        voxel_sort.voxel_down_sample_and_trace(torch.zeros(3, 300), 0.1)
