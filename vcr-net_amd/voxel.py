"""ctypes binding of include/vcr_hip_voxel.h and the Python API on top of it: down-sampling a cloud on a voxel grid (DESIGN.md
section 4.11) -- the points of one cell of a grid of edge voxel_size replaced by their mean (Open3D's voxel_down_sample), the
voxels in order of first appearance -- by vcr_voxel_f32.

The header extends include/vcr_hip.h without touching it, and so does this module for ``native``: its own STRUCTS / SIGNATURES
maps, in the same shape, applied once to ``native.lib()`` on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native
from .native import VcrHipError, f32p, ptr
from .score import i32p

MAX_N = 131072
MAX_SPLITS = 128
MAX_CELLS = 1 << 21                                        # cells per axis: three of them pack into one 64-bit key


class VoxelArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("xyz", f32p), ("B", C.c_int), ("N", C.c_int), ("voxel_size", C.c_float),
                ("points", f32p), ("count", i32p), ("point_voxel", i32p), ("voxel_points", i32p), ("variant", C.c_int)]


STRUCTS = {"vcr_voxel_args": VoxelArgs}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_voxel.h (tests/test_voxel_cpu.py holds them to it)
SIGNATURES = extension.workspace_signatures("vcr_voxel", VoxelArgs)

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def variant(splits: int = 0) -> int:
    """vcr_voxel_args.variant that forces the scan's number of segments (VCR_NN_SCORE_VARIANT's encoding): 0 = the plan's."""
    return int(splits) << 8


def voxel_form(B, N, cu_count=256, variant=0):
    """vcr_voxel_form (host only with an explicit cu_count): (points per lane, segments of the scan, workspace bytes)
    vcr_voxel_f32 would run [B,3,N] with on a device of cu_count compute units."""
    a = VoxelArgs(0x1000, B, N, 1.0, 0x2000, 0x3000, None, None, variant)       # (never dereferenced on the host)
    return extension.form(lib(), "vcr_voxel", a, cu_count)


@native._guarded
def voxel_grid(xyz, voxel_size, variant=0, want_trace=True, guard=0, prefill=None):
    """vcr_voxel_f32 on xyz [B,3,N] (device, fp32) -> dict of points float32 [B,3,N] (the voxels' means in order of first
    appearance, NaN behind them), count int32 [B] (-1: the grid is too fine for that cloud) and, with want_trace, point_voxel
    int32 [B,N] (-1: the point is not finite) and voxel_points int32 [B,N] (0 behind the voxels).
    guard / prefill (tests): every output is a view of a buffer with `guard` more elements behind it, all of it -- and the
    workspace -- filled with the byte `prefill` before the launch; the buffers come back under "_raw"."""
    extension.check_cloud("voxel_down_sample", "xyz", xyz)
    if not xyz.is_cuda:
        raise VcrHipError("voxel_down_sample runs on the MI355X HIP path only; move the cloud to cuda "
                          "(there is no CPU fallback by design)")
    voxel_size = float(voxel_size)
    if not (math.isfinite(voxel_size) and voxel_size > 0.0):
        raise VcrHipError(f"voxel_down_sample: voxel_size must be finite and > 0, got {voxel_size}")
    dev = xyz.device
    B, _, N = xyz.shape
    xyz = xyz.contiguous().float()
    out, raw = extension.outputs(dev, guard, prefill)
    o = {"points": out("points", B * 3 * N, torch.float32).view(B, 3, N), "count": out("count", B, torch.int32)}
    if want_trace:
        o["point_voxel"] = out("point_voxel", B * N, torch.int32).view(B, N)
        o["voxel_points"] = out("voxel_points", B * N, torch.int32).view(B, N)
    a = VoxelArgs(ptr(xyz), B, N, voxel_size, ptr(o["points"]), ptr(o["count"]), ptr(o.get("point_voxel")),
                  ptr(o.get("voxel_points")), int(variant))
    extension.call_with_workspace(lib(), "vcr_voxel", a, dev, prefill)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def voxel_down_sample(xyz, voxel_size, method="scan"):
    """xyz [B,3,N] (device tensor, up to 131 072 points a cloud) on a grid of edge voxel_size: every occupied cell gives one
    point, the mean of the points inside it (Open3D's voxel_down_sample; its grid starts at the finite points' minimum minus
    voxel_size / 2).  Returns (points, count, point_voxel) without a host synchronisation:
      points       float32 [B,3,N]  cloud b's count[b] voxels in order of first appearance, NaN behind them
      count        int32 [B]        -1 where the grid is too fine for the cloud (more than 2^21 cells along an axis)
      point_voxel  int32 [B,N]      the voxel every point went to, -1 for a point with a NaN or infinite coordinate
    ``unpad(points, count)`` cuts the clouds to their sizes.
    ``method``: "scan" (the default: every point against every point, vcr_voxel_f32) or "sort" (a stable device radix sort of
    the points' cells, vcr_voxel_sort_f32) -- the same bits either way; anything else raises.
    Measured (profiles/voxel_sort_bench.txt, ~8 points a voxel): "sort" is worth taking from about 4 096 points a cloud (x1.5 for
    one cloud, x1.9 for sixteen; x39 at 131 072 points), is a draw at 2 048 and loses at 1 024 (x0.78), where its fixed 28
    launches cost more than the scan."""
    if method == "sort":
        from . import voxel_sort
        o = voxel_sort.voxel_grid_sort(xyz, voxel_size, want_trace=True)
    elif method == "scan":
        o = voxel_grid(xyz, voxel_size, want_trace=True)
    else:
        raise VcrHipError(f'voxel_down_sample: method must be "scan" or "sort", got {method!r}')
    return o["points"], o["count"], o["point_voxel"]


def unpad(points, count):
    """(points [B,3,N], count [B]) of voxel_down_sample -> a list of B tensors [3, count[b]] (views).  One synchronisation (the
    counts travel to the host; none if they are there already); a cloud whose grid was too fine (count -1) raises."""
    counts = count.tolist()
    for b, m in enumerate(counts):
        if m < 0:
            raise VcrHipError(f"voxel_down_sample: the grid is too fine for cloud {b} (more than {MAX_CELLS} cells along an "
                              "axis); use a larger voxel_size")
    return [points[b, :, :m] for b, m in enumerate(counts)]
