"""Farthest-point sampling without a GPU: the CPU restatement (tests/fps_restated.py) against the reference's recorded indices,
and everything of vcr_fps_f32 / vcr_fps_form that is host logic -- the exported symbols, the struct layout, the argument
errors, the form the plan picks."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fps_restated as fr
from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcr_hip.h")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "fps_*.npz")))
MIN_MARGIN = 1e-4


@pytest.fixture(scope="module")
def lib():
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import build, native
    build.build()
    return native.lib()


def test_the_fixtures_the_issue_lists_are_there():
    names = {os.path.basename(p)[4:-4] for p in FIXTURES}
    assert {"uniform_b3_n1000_p64", "uniform_b2_n5000_p512", "uniform_b2_n20000_p1024", "uniform_b1_n70001_p2048",
            "lattice_b2_n257_p257", "uniform_b2_n100_p150", "nan_b2_n300_p32", "inf_b2_n300_p32"} <= names
    for p in FIXTURES:
        assert os.path.getsize(p) < (1 << 20), p
    for n in ("uniform_b3_n1000_p64", "uniform_b2_n5000_p512", "uniform_b2_n20000_p1024", "uniform_b1_n70001_p2048"):
        z = np.load(os.path.join(GOLDEN, f"fps_{n}.npz"))
        assert [float(s) for s in z["scales"]] == [float(np.float32(v)) for v in (1e-3, 1.0, 30.0)]


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[4:-4])
def test_restatement_reproduces_the_reference_index_for_index(path):
    """What lets the GPU tests use the restatement at sizes too large to commit.  Explicit start on every fixture; the
    barycentre rule on every fixture recorded for it, whose finite clouds must be clear decisions of the reference
    (margin >= 1e-4 on the reference's side and on the restatement's)."""
    z = np.load(path)
    npoint = int(z["npoint"])
    assert np.abs(z["xyz"][np.isfinite(z["xyz"])]).max() * float(z["scales"].max()) <= 1e3
    for k, s in enumerate(z["scales"]):
        x = z["xyz"] * np.float32(s)
        assert x.dtype == np.float32
        ref = z[f"idx_s{k}"].astype(np.int64)
        assert ref.shape == (x.shape[0], npoint) and ref.min() >= 0 and ref.max() < x.shape[2]
        assert np.array_equal(fr.fps(x, npoint, start=ref[:, 0]), ref)
        if int(z["use_start"]):
            continue
        recorded = z[f"margin_s{k}"]
        for b in range(x.shape[0]):
            if np.isfinite(x[b]).all():
                assert recorded[b] >= MIN_MARGIN and fr.margin(x[b]) >= MIN_MARGIN, (b, recorded[b], fr.margin(x[b]))
            else:
                assert np.isnan(recorded[b])
        assert np.array_equal(fr.fps(x, npoint), ref)


def test_restatement_non_finite_rules():
    x = np.random.RandomState(0).uniform(-1, 1, (3, 50)).astype(np.float32)
    x[1, 7] = np.nan
    assert fr.fps_one(x, 6).tolist() == [0, 7, 7, 7, 7, 7]                    # the issue's example
    y = np.random.RandomState(1).uniform(-1, 1, (3, 50)).astype(np.float32)
    y[0, 30] = np.inf
    assert fr.barycentre_start(y) == 30                                       # its own distance is the only NaN
    assert fr.fps_one(y, 5, start=99).tolist()[0] == 49 and fr.fps_one(y, 5, start=-3).tolist()[0] == 0   # clamped


def test_header_declares_and_library_exports_the_entry_points(lib):
    hdr = open(HEADER).read()
    assert re.search(r"int\s+vcr_fps_f32\s*\(\s*const\s+vcr_fps_args\s*\*\s*,\s*vcr_stream_t\s*\)\s*;", hdr)
    assert re.search(r"int\s+vcr_fps_form\s*\(\s*const\s+vcr_fps_args\s*\*\s*,\s*int\s*\*\s*form\s*,\s*int\s*\*\s*points_per_thread\s*\)\s*;", hdr)
    assert hasattr(lib, "vcr_fps_f32") and hasattr(lib, "vcr_fps_form")
    from vcrnet_amd import native
    assert lib.vcr_abi_version() == native.ABI_VERSION == 27                  # purely additive: the version stays


def test_fps_args_match_the_c_layout(tmp_path):
    """Same method as test_abi.py::test_ctypes_structs_match_the_c_layout, for vcr_fps_args / native.FpsArgs."""
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
             'printf("%zu\\n", sizeof(vcr_fps_args));']
    expect = [("sizeof", ctypes.sizeof(native.FpsArgs))]
    for fname, _ in native.FpsArgs._fields_:
        lines.append(f'printf("%zu\\n", offsetof(vcr_fps_args, {fname}));')
        expect.append((fname, getattr(native.FpsArgs, fname).offset))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [e for _, e in expect], list(zip(expect, got))
    assert native.FpsArgs().struct_bytes == ctypes.sizeof(native.FpsArgs)


def _args(N=4096, npoint=64, B=2, variant=0, stride=None):
    from vcrnet_amd import native
    a = native.FpsArgs()
    a.xyz_cf, a.idx = 0x1000, 0x2000                                          # (never dereferenced on the host)
    a.cloud_stride, a.B, a.N, a.npoint, a.variant = (3 * N if stride is None else stride), B, N, npoint, variant
    return a


def test_argument_errors_return_their_codes_without_a_gpu(lib):
    from vcrnet_amd import native
    EINVAL, EUNSUPPORTED = -1, -3
    f32 = lambda a: lib.vcr_fps_f32(ctypes.byref(a), None)
    form = lambda a: lib.vcr_fps_form(ctypes.byref(a), None, None)
    assert lib.vcr_fps_f32(None, None) == EINVAL and lib.vcr_fps_form(None, None, None) == EINVAL
    assert form(_args()) == 0
    for field in ("xyz_cf", "idx"):
        a = _args()
        setattr(a, field, None)
        assert f32(a) == EINVAL and form(a) == EINVAL, field
    for bad in (0, native.FpsArgs.out_cf.offset - 4, ctypes.sizeof(native.FpsArgs) + 8):   # unsized, short of idx, too long
        a = _args()
        a.struct_bytes = bad
        assert f32(a) == EINVAL and form(a) == EINVAL, bad
    a = _args()
    a.struct_bytes = native.FpsArgs.out_cf.offset                                       # the mandatory part alone is served
    assert form(a) == 0
    for kw in (dict(N=0), dict(npoint=0), dict(B=0), dict(N=-4), dict(stride=3 * 4096 - 1), dict(variant=3), dict(variant=-1)):
        assert f32(_args(**kw)) == EINVAL and form(_args(**kw)) == EINVAL, kw
    assert f32(_args(N=131073)) == EUNSUPPORTED and form(_args(N=131073)) == EUNSUPPORTED
    assert form(_args(N=131072, B=16384)) == EUNSUPPORTED                              # B * N = 2^31
    assert form(_args(N=100, npoint=1 << 20, B=2048)) == EUNSUPPORTED                  # B * npoint = 2^31
    assert form(_args(N=131072, B=16383)) == 0
    assert form(_args(N=20481, variant=1)) == EUNSUPPORTED                             # the resident form ends at 20 480 points
    assert b"unsupported" in lib.vcr_strerror(EUNSUPPORTED)


def test_the_plan_picks_the_forms_design_quotes(lib):
    """vcr_fps_form: resident (coordinates and distances in registers) through 20 480 points, streaming beyond; the points each
    of the 1024 threads holds -- DESIGN.md section 4.7's table."""
    from vcrnet_amd import native
    RES, STR = 1, 2
    assert native.fps_form(4096) == (RES, 4) and native.fps_form(16384) == (RES, 16) and native.fps_form(131072) == (STR, 128)
    table = {1: (RES, 1), 1024: (RES, 1), 1025: (RES, 4), 4097: (RES, 8), 8192: (RES, 8), 8193: (RES, 16), 16385: (RES, 20),
             20480: (RES, 20), 20481: (STR, 32), 32768: (STR, 32), 32769: (STR, 64), 65536: (STR, 64), 65537: (STR, 128),
             70001: (STR, 128)}
    for N, want in table.items():
        assert native.fps_form(N) == want, N
    assert native.fps_form(4096, variant=STR) == (STR, 32) and native.fps_form(20480, variant=RES) == (RES, 20)
    assert native.fps_form(4096, npoint=5000, B=32) == (RES, 4)                         # neither npoint nor B moves the form
    with pytest.raises(native.VcrHipError):
        native.fps_form(131073)


def test_python_entry_points_refuse_cpu_tensors():
    """No CPU fallback, as everywhere: farthest_point_sample / native.fps / register_sampled on CPU tensors raise VcrHipError;
    register_sampled names what is wrong with mis-shaped input before anything is launched."""
    import vcrnet_amd
    from vcrnet_amd import native
    from vcrnet_amd.module import register_sampled
    assert vcrnet_amd.register_sampled is register_sampled and vcrnet_amd.farthest_point_sample is native.farthest_point_sample
    x = torch.zeros(2, 3, 100)
    with pytest.raises(native.VcrHipError):
        vcrnet_amd.farthest_point_sample(x, 10)
    with pytest.raises(native.VcrHipError):
        native.fps(x, 10)
    with pytest.raises(native.VcrHipError, match="no CPU fallback"):
        register_sampled(None, torch.zeros(2, 3, 3000), torch.zeros(2, 3, 4100), 1024)
    with pytest.raises(native.VcrHipError, match="same number of clouds"):
        register_sampled(None, torch.zeros(2, 3, 3000), torch.zeros(3, 3, 4100), 1024)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        register_sampled(None, torch.zeros(2, 3000, 3), torch.zeros(2, 3, 4100), 1024)
    with pytest.raises(native.VcrHipError, match=r"\[B, 3, N\]"):
        register_sampled(None, torch.zeros(3, 3000), torch.zeros(2, 3, 4100), 1024)
