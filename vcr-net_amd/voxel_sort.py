"""ctypes binding of include/vcr_hip_voxel_sort.h: the voxel grid of ``voxel`` by a stable device radix
sort -- the same definition and the same bits in passes linear in the cloud's size -- and the voxels' member lists.
``voxel.voxel_down_sample(..., method="sort")`` calls it.

The entry points take ``voxel.VoxelArgs`` and a ``VoxelSortArgs`` behind it.  Like the other bindings the header extends
include/vcr_hip.h without touching it and this module keeps its own STRUCTS / SIGNATURES maps, applied once to ``native.lib()``
on first use.  No CPU fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math
import torch

from . import extension, native, voxel
from .native import VcrHipError, ptr
from .score import i32p

DIGIT_BITS = (4, 8, 11)                                    # the digit widths vcr_voxel_sort_args.variant forces; 0 = the plan's
METHODS = ("scan", "sort")                                 # what ``method=`` / ``voxel_method=`` take


class VoxelSortArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("variant", C.c_int), ("members", i32p), ("voxel_start", i32p)]


NEW_STRUCTS = {"vcr_voxel_sort_args": VoxelSortArgs}       # what the header itself defines
STRUCTS = {**NEW_STRUCTS, **voxel.STRUCTS}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_voxel_sort.h (tests/test_voxel_sort_cpu.py holds them to it)
SIGNATURES = extension.workspace_signatures2("vcr_voxel_sort", voxel.VoxelArgs, VoxelSortArgs)

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def check_method(api, method, name="method"):
    if method not in METHODS:
        raise VcrHipError(f'{api}: {name} must be "scan" or "sort", got {method!r}')


def voxel_sort_form(B, N, digit_bits=0, cu_count=256):
    """vcr_voxel_sort_form (host only): (digit width, passes launched, elements per lane, workspace bytes) vcr_voxel_sort_f32
    would run [B,3,N] with; digit_bits forces the width (0 = the plan's)."""
    a = voxel.VoxelArgs(0x1000, B, N, 1.0, 0x2000, 0x3000, None, None, 0)      # (never dereferenced on the host)
    s = VoxelSortArgs(int(digit_bits), None, None)
    L = lib()
    bits, passes, per_lane = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(L.vcr_voxel_sort_form(C.byref(a), C.byref(s), cu_count, C.byref(bits), C.byref(passes), C.byref(per_lane)),
                 "vcr_voxel_sort_form")
    return bits.value, passes.value, per_lane.value, L.vcr_voxel_sort_workspace_bytes(C.byref(a), C.byref(s), cu_count)


@native._guarded
def voxel_grid_sort(xyz, voxel_size, digit_bits=0, want_trace=True, want_members=False, guard=0, prefill=None):
    """vcr_voxel_sort_f32 on xyz [B,3,N] (device, fp32) -> ``voxel.voxel_grid``'s dict, bit for bit, and with want_members
    members int32 [B,N] (the finite points' indices voxel by voxel, -1 behind them) and voxel_start int32 [B,N] (where voxel v's
    members begin; the number of finite points behind the voxels).  digit_bits forces the sort's digit width (tests,
    benchmarks).  guard / prefill (tests): as ``voxel.voxel_grid``'s."""
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
    if want_members:
        o["members"] = out("members", B * N, torch.int32).view(B, N)
        o["voxel_start"] = out("voxel_start", B * N, torch.int32).view(B, N)
    a = voxel.VoxelArgs(ptr(xyz), B, N, voxel_size, ptr(o["points"]), ptr(o["count"]), ptr(o.get("point_voxel")),
                        ptr(o.get("voxel_points")), 0)
    s = VoxelSortArgs(int(digit_bits), ptr(o.get("members")), ptr(o.get("voxel_start")))
    extension.call_with_workspace(lib(), "vcr_voxel_sort", a, dev, prefill, second=s)
    if guard or prefill is not None:
        o["_raw"] = raw
    return o


def voxel_down_sample_and_trace(xyz, voxel_size):
    """``voxel.voxel_down_sample(xyz, voxel_size, method="sort")`` with the voxels' member lists (Open3D's
    voxel_down_sample_and_trace).  Returns (points, count, point_voxel, members, voxel_start) without a host synchronisation:
      members      int32 [B,N]  the indices of the finite points, voxel 0's first, then voxel 1's, ...; ascending inside every
                                voxel; -1 behind the finite points
      voxel_start  int32 [B,N]  the slot of ``members`` where voxel v begins, for v < count[b]; the number of finite points
                                beyond.  A voxel's end is the next one's start
    A cloud whose grid is too fine (count -1) reads -1 and 0 throughout."""
    o = voxel_grid_sort(xyz, voxel_size, want_trace=True, want_members=True)
    return o["points"], o["count"], o["point_voxel"], o["members"], o["voxel_start"]
