"""ctypes binding of include/vcr_hip_gridnn.h: the grid siblings of vcr_nn_score_f32 and of the three
refinements -- the same merge, fits, solves and stop test behind a nearest-neighbour search that walks the TARGET's uniform grid
and stops at max_dist.  ``score.nn_score`` and ``refine.refine`` call them for ``search="grid"``.

Every entry point takes its scan sibling's args struct (``score.NnScoreArgs``, ``refine.RefineArgs``, ``plane.RefinePlaneArgs``,
``gicp.RefineGicpArgs``) and a ``GridNnArgs`` behind it.  Like the other bindings the header extends include/vcr_hip.h without
touching it and this module keeps its own STRUCTS / SIGNATURES maps, applied once to ``native.lib()`` on first use.  No CPU
fallback, as everywhere."""
from __future__ import annotations

import ctypes as C
import math

from . import extension, gicp, grid, native, plane, refine, score
from .native import VcrHipError

SEARCHES = ("scan", "grid")                                # what ``search=`` / ``nn_search=`` of the scoring and refining calls take
ORDERS = (0, 1, 2)                                         # the plan's, the source's cell order, index order
QUERIES = grid.QUERIES


class GridNnArgs(native._Sized):
    _fields_ = [("struct_bytes", C.c_uint32), ("cell", C.c_float), ("order", C.c_int)]


FAMILIES = {"vcr_nn_score_grid": score.NnScoreArgs, "vcr_refine_grid": refine.RefineArgs,
            "vcr_refine_plane_grid": plane.RefinePlaneArgs, "vcr_refine_gicp_grid": gicp.RefineGicpArgs}

NEW_STRUCTS = {"vcr_grid_nn_args": GridNnArgs}             # what the header itself defines
STRUCTS = {**NEW_STRUCTS, **score.STRUCTS, **refine.STRUCTS, "vcr_refine_plane_args": plane.RefinePlaneArgs, **gicp.STRUCTS}

# name -> (restype, [argtypes]): the prototypes of include/vcr_hip_gridnn.h (tests/test_gridnn_cpu.py holds them to it)
SIGNATURES = {}
for _entry, _Args in FAMILIES.items():
    SIGNATURES.update(extension.workspace_signatures2(_entry, _Args, GridNnArgs))

lib = extension.typed_lib(SIGNATURES)                      # native.lib() with this module's entry points typed (once)


def check_search(api, search, name="search"):
    if search not in SEARCHES:
        raise VcrHipError(f'{api}: {name} must be "scan" or "grid", got {search!r}')


def check_cell(api, cell):
    """cell=None (the target's automatic edge) or a finite edge > 0 -> the float vcr_grid_nn_args.cell takes."""
    if cell is None:
        return 0.0
    try:
        c = float(cell)
    except (TypeError, ValueError):
        c = float("nan")
    if not (math.isfinite(c) and c > 0.0):
        raise VcrHipError(f"{api}: cell must be None (the automatic grid) or finite and > 0, got {cell!r}")
    return c


def grid_args(cell=0.0, order=0):
    return GridNnArgs(float(cell), int(order))


def entry_of(scan_entry):
    """The grid sibling's name: vcr_refine_plane -> vcr_refine_plane_grid."""
    return scan_entry + "_grid"


def form(entry, a, g, cu_count=256):
    """`entry`_form and _workspace_bytes (host only): (cells per cloud, order taken, queries per workgroup, workspace bytes)."""
    L = lib()
    cells, order, queries = C.c_int(0), C.c_int(0), C.c_int(0)
    native.check(getattr(L, entry + "_form")(C.byref(a), C.byref(g), cu_count, C.byref(cells), C.byref(order), C.byref(queries)),
                 entry + "_form")
    return cells.value, order.value, queries.value, getattr(L, entry + "_workspace_bytes")(C.byref(a), C.byref(g), cu_count)


def nn_score_grid_form(B, Ns, Nt, order=0, cell=0.0, cu_count=256):
    a = score.NnScoreArgs(0x1000, 0x2000, B, Ns, Nt, None, None, 0.0, None, None, None, None, 0x3000, 0x4000, 0)
    return form("vcr_nn_score_grid", a, grid_args(cell, order), cu_count)


def refine_grid_form(B, Ns, Nt, order=0, cell=0.0, cu_count=256, method="point_to_point", max_iterations=30):
    """The three refinements' grid forms (method as refine_registration's)."""
    kw = dict(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=max_iterations, R_out=0x3000, t_out=0x4000,
              fitness=0x5000, rmse=0x6000, variant=0)      # (never dereferenced on the host)
    if method == "point_to_point":
        return form("vcr_refine_grid", refine.RefineArgs(**kw), grid_args(cell, order), cu_count)
    if method == "point_to_plane":
        return form("vcr_refine_plane_grid", plane.RefinePlaneArgs(tgt_normals=0x7000, **kw), grid_args(cell, order), cu_count)
    return form("vcr_refine_gicp_grid", gicp.RefineGicpArgs(tgt_normals=0x7000, src_normals=0x8000, epsilon=gicp.EPSILON, **kw),
                grid_args(cell, order), cu_count)
