"""Down-sampling on a voxel grid, without a GPU: the boundary of include/vcr_hip_voxel.h (prototypes against
vcrnet_amd.voxel.SIGNATURES, the struct against gcc's layout, the exported symbols), the argument errors, the form and the
workspace voxel_plan answers, the new kernels' register remarks, and the two numpy restatements of the definition
(tests/voxel_restated.py) against each other and against the definition's structure."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import boundary
import voxel_restated as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "vcr_hip_voxel.h")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
ENTRY_POINTS = {"vcr_voxel_workspace_bytes", "vcr_voxel_f32", "vcr_voxel_form"}


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, voxel
    build.build()
    return voxel.lib()


def test_signatures_match_the_header_and_the_library_exports_them(lib):
    from vcrnet_amd import voxel
    boundary.check_signatures(HEADER, voxel, lib, ENTRY_POINTS)


def test_args_match_the_c_layout(tmp_path):
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import voxel
    boundary.check_layout(HEADER, voxel, tmp_path)
    assert voxel.VoxelArgs().struct_bytes == ctypes.sizeof(voxel.VoxelArgs)


def test_the_other_boundaries_are_where_they_were(lib, monkeypatch):
    """The feature lives beside the four headers, not in them: none mentions it, ABI 27, the same 51 prototypes; the new header
    is taken into the digests through a list of its own."""
    from vcrnet_amd import build, native, voxel
    for h in ("vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h", "vcr_hip_plane.h"):
        assert "vcr_voxel" not in open(os.path.join(INCLUDE, h)).read(), h
    assert len(native.PUBLIC) == 51 and lib.vcr_abi_version() == native.ABI_VERSION == 27
    assert not set(voxel.SIGNATURES) & set(native.SIGNATURES) and not set(voxel.STRUCTS) & set(native.STRUCTS)
    assert voxel.VoxelArgs.__module__ == voxel.__name__
    assert [os.path.basename(h) for h in build.PUBLIC_HEADERS] == ["vcr_hip.h", "vcr_hip_score.h", "vcr_hip_refine.h",
                                                                   "vcr_hip_plane.h"]
    assert [os.path.basename(h) for h in build.LATER_HEADERS] == ["vcr_hip_voxel.h"]
    full = build.sources_sha16()
    monkeypatch.setattr(build, "LATER_HEADERS", [])
    assert build.sources_sha16() != full


def _args(B=2, N=1000, h=0.1, variant=0):
    from vcrnet_amd import voxel
    a = voxel.VoxelArgs()
    a.xyz, a.points, a.count = 0x1000, 0x2000, 0x3000      # (never dereferenced on the host)
    a.B, a.N, a.voxel_size, a.variant = B, N, h, variant
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import voxel
    f32 = lambda a, ws=0x10000, n=1 << 40: lib.vcr_voxel_f32(ctypes.byref(a), ws, n, None)      # noqa: E731
    form = lambda a: lib.vcr_voxel_form(ctypes.byref(a), 256, None, None)                        # noqa: E731
    size = lambda a: lib.vcr_voxel_workspace_bytes(ctypes.byref(a), 256)                         # noqa: E731
    assert lib.vcr_voxel_f32(None, 0x10000, 1 << 40, None) == EINVAL
    assert lib.vcr_voxel_form(None, 256, None, None) == EINVAL and lib.vcr_voxel_workspace_bytes(None, 256) == 0
    assert form(_args()) == 0 and size(_args()) > 0
    for field in ("xyz", "points", "count"):
        a = _args()
        setattr(a, field, None)
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, field
    a = _args()
    a.point_voxel, a.voxel_points = 0x4000, 0x5000         # the optional outputs change nothing here
    assert form(a) == 0 and size(a) == size(_args())
    for kw in (dict(B=0), dict(B=-2), dict(h=0.0), dict(h=-0.5), dict(h=float("nan")), dict(h=float("inf")),
               dict(h=-float("inf")), dict(variant=2), dict(variant=4), dict(variant=-1), dict(variant=voxel.variant(129)),
               dict(variant=1 << 16), dict(variant=1 << 4)):
        assert f32(_args(**kw)) == EINVAL and form(_args(**kw)) == EINVAL and size(_args(**kw)) == 0, kw
    assert form(_args(h=1e-45)) == 0 and form(_args(variant=1)) == 0 and form(_args(variant=1 | voxel.variant(128))) == 0
    for kw in (dict(N=0), dict(N=-4), dict(N=131073), dict(N=131072, B=16384)):
        assert f32(_args(**kw)) == EUNSUPPORTED and form(_args(**kw)) == EUNSUPPORTED and size(_args(**kw)) == 0, kw
    assert form(_args(N=131072, B=16383)) == 0
    assert lib.vcr_voxel_form(ctypes.byref(_args()), -1, None, None) == EINVAL
    # struct_bytes: unsized, short of count, longer than the library knows; the mandatory part alone is served
    for bad in (0, voxel.VoxelArgs.point_voxel.offset - 4, ctypes.sizeof(voxel.VoxelArgs) + 8):
        a = _args()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and form(a) == EINVAL and size(a) == 0, bad
    a = _args(variant=voxel.variant(2))
    q, s = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.vcr_voxel_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) == (1, 2)
    a.struct_bytes = voxel.VoxelArgs.point_voxel.offset                           # ... and its variant reads as 0
    assert lib.vcr_voxel_form(ctypes.byref(a), 256, ctypes.byref(q), ctypes.byref(s)) == 0 and (q.value, s.value) == (1, 3)
    # the workspace: missing, misaligned, short (the size is asked for the device at hand -- without one, 256 CUs)
    a = _args()
    need = lib.vcr_voxel_workspace_bytes(ctypes.byref(a), 0)
    assert need == size(a) > 0
    assert f32(a, ws=None) == EINVAL and f32(a, ws=0x10004) == EINVAL and f32(a, ws=0x10008) == EINVAL
    assert f32(a, n=need - 1) == EWORKSPACE and f32(a, n=0) == EWORKSPACE


def workspace_formula(B, N, S):
    """The header's: up(32 B) + up(8 B N) + 2 up(4 S B N) + 4 up(4 B N) + up(4 B nblk)."""
    up = lambda v: (v + 255) // 256 * 256                                          # noqa: E731
    return up(32 * B) + up(8 * B * N) + 2 * up(4 * S * B * N) + 4 * up(4 * B * N) + up(4 * B * ((N + 255) // 256))


def test_the_form_is_the_score_plans_and_the_workspace_the_headers(lib):
    from vcrnet_amd import score, voxel
    shapes = [(1, 1), (1, 5), (1, 257), (16, 1024), (16, 16384), (1, 70001), (1, 131072), (64, 16384), (256, 16384), (3, 700)]
    for B, N in shapes:
        for cu in (256, 1, 304):
            for force in (0, 1, 2, 3, 8, 128):
                q, s, ws = voxel.voxel_form(B, N, cu_count=cu, variant=voxel.variant(force))
                assert (q, s) == (1, score.nn_score_form(B, N, N, cu_count=cu, variant=score.variant(0, force))[1]), (B, N, cu, force)
                assert force == 0 or s == force
                assert ws == workspace_formula(B, N, s), (B, N, cu, force)
    assert voxel.voxel_form(1, 131072)[1] == 32 and voxel.voxel_form(256, 16384)[1] == 1
    assert voxel.voxel_form(1, 2049, variant=1)[:2] == voxel.voxel_form(1, 2049)[:2]          # "one point per lane" is the form
    for B, N in ((1, 0), (1, 131073), (16384, 131072)):
        with pytest.raises(Exception):
            voxel.voxel_form(B, N)


def test_the_new_kernels_use_no_scratch():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build
    build.build()
    res = build.kernel_resources()
    names = list(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    mine = {d.replace("(anonymous namespace)::", ""): res[n] for n, d in zip(names, dem) if res[n]["file"] == "voxel.hip" and "voxel_" in d}
    assert {d.split("(")[0] for d in mine} == {
        "voxel_bounds_kernel", "voxel_keys_kernel", "voxel_scan_kernel", "voxel_merge_kernel", "voxel_offsets_kernel",
        "voxel_rank_kernel", "voxel_means_kernel"}
    for d, v in mine.items():
        assert v.get("scratch", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, (d, v)
        assert v["lds"] <= 21 * 1024, (d, v)
    scan = [v for d, v in mine.items() if d.startswith("voxel_scan_kernel")][0]
    assert scan["occupancy"] >= 8 and scan["vgprs"] <= 64, scan             # the hot loop: nn_scan_kernel<1>'s residency


@pytest.fixture(scope="module")
def cases():
    """name -> (xyz, h, the loop's result, the vectorised route's), computed once."""
    out = {}
    for name, make in vr.RECIPES.items():
        xyz, h = make()
        out[name] = (xyz, h, vr.batch(xyz, h, vr.voxel_loop), vr.batch(xyz, h, vr.voxel_fast))
    return out


def test_the_two_restatements_agree_bit_for_bit(cases):
    for name, (xyz, h, slow, fast) in cases.items():
        assert vr.same(slow, fast), name
        assert slow["points"].dtype == np.float32 and slow["point_voxel"].dtype == np.int32


def test_the_definitions_structure_holds_on_every_recipe(cases):
    for name, (xyz, h, r, _) in cases.items():
        for b, cloud in enumerate(xyz):
            finite, cells = vr._cells(cloud, h)
            M, pv, vp, pts = int(r["count"][b]), r["point_voxel"][b], r["voxel_points"][b], r["points"][b]
            if M == -1:
                assert (pv == -1).all() and (vp == 0).all() and (vr.bits(pts) == vr.NAN_BITS).all(), name
                assert (cells[:, finite] >= vr.MAX_CELLS).any(), name
                continue
            assert (pv[~finite] == -1).all() and (pv[finite] >= 0).all(), name
            assert vp[:M].sum() == finite.sum() and (vp[:M] >= 1).all() and (vp[M:] == 0).all(), name
            assert (vr.bits(pts[:, M:]) == vr.NAN_BITS).all() and np.isfinite(pts[:, :M]).all(), name
            assert M == (len(np.unique(cells[:, finite].T, axis=0)) if finite.any() else 0), name
            if M == 0:
                continue
            assert (cells[:, finite] >= 0).all() and (cells[:, finite] < vr.MAX_CELLS).all(), name
            reps = np.asarray([np.flatnonzero(pv == v)[0] for v in range(M)])    # the lowest member of every voxel
            assert (np.diff(reps) > 0).all(), name                                # ... ascends with the voxel's number
            assert np.array_equal(cells[:, finite], cells[:, reps[pv[finite]]]), name   # every member's cell is its voxel's
            assert np.array_equal(np.bincount(pv[finite], minlength=M), vp[:M]), name


def test_the_recipes_meet_the_edges_they_are_named_for(cases):
    r = cases["n5_one_voxel"][2]
    assert r["count"][0] == 1 and r["voxel_points"][0, 0] == 5
    xyz, h, r, _ = cases["own_voxel"]
    assert r["count"][0] == xyz.shape[2] and np.array_equal(vr.bits(r["points"]), vr.bits(xyz))
    assert vr.bits(xyz)[0, 1, 5] == np.int32(-2 ** 31)                            # the -0.0 came through
    xyz, h, r, _ = cases["one_voxel_1025"]
    assert r["count"][0] == 1 and r["voxel_points"][0, 0] == 1025
    want = xyz[0].astype(np.float64)[:, 0]
    for i in range(1, 1025):
        want = want + xyz[0].astype(np.float64)[:, i]
    assert np.array_equal(r["points"][0, :, 0], (want / 1025.0).astype(np.float32))
    xyz, h, r, _ = cases["lattice_faces"]
    finite, cells = vr._cells(xyz[0], h)
    exact = (xyz[0].astype(np.float64) - (xyz[0].min(axis=1).astype(np.float64) - 0.125)[:, None]) / 0.25
    assert (exact == np.floor(exact)).mean() > 0.3 and r["voxel_points"][0].max() > 1   # many points ON a face
    r = cases["duplicates"][2]
    assert (r["voxel_points"][0, :r["count"][0]] >= 2).all()
    xyz, h, r, _ = cases["non_finite"]
    pv = r["point_voxel"][0]
    assert pv[0] == -1 and pv[1] == -1 and pv[17] == -1 and pv[300] == -1 and pv[50] == pv[51] >= 0
    assert np.flatnonzero(pv == pv[50])[0] == 50                                  # the would-be representative 1 is not finite
    assert cases["all_nan"][2]["count"][0] == 0
    r = cases["fine_batch"][2]
    assert list(r["count"] > 0) == [True, False, True] and r["count"][1] == -1
    for name in ("n70001", "n131072"):
        xyz, h, r, _ = cases[name]
        assert 6.0 < xyz.shape[2] / r["count"][0] < 10.0                          # about 8 points a voxel


def test_python_entry_points_refuse_what_they_cannot_run():
    import vcrnet_amd
    from vcrnet_amd import native, voxel
    assert vcrnet_amd.voxel_down_sample is voxel.voxel_down_sample and "voxel_down_sample" in vcrnet_amd.__all__
    a = torch.zeros(2, 3, 300)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        vcrnet_amd.voxel_down_sample(a, 0.1)
    with pytest.raises(native.VcrHipError, match=r"xyz must be a \[B, 3, N\]"):
        vcrnet_amd.voxel_down_sample(a.transpose(1, 2), 0.1)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        vcrnet_amd.voxel_down_sample(torch.zeros(3, 300), 0.1)
    with pytest.raises(native.VcrHipError, match="cloud 1"):
        voxel.unpad(torch.zeros(2, 3, 4), torch.tensor([2, -1]))
    assert [tuple(p.shape) for p in voxel.unpad(torch.zeros(2, 3, 4), torch.tensor([2, 0]))] == [(3, 2), (3, 0)]
    import inspect
    from vcrnet_amd import module
    assert inspect.signature(module.register_sampled).parameters["voxel"].default is None
