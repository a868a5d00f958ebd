#!/usr/bin/env python
"""Record how the five entry points that cut a brute-force scan into segments answer over a grid of shapes, CU counts and
forced forms, so that the split policy (csrc/seg_scan.h and its callers' limits) is pinned to the commit this script was run
at instead of to the code under test: tests/test_scan_forms.py asserts that the library reproduces the file exactly.

Host only: every call names its cu_count, so no device is asked.  Run at the commit whose answers are to be kept:

  python tests/golden/gen_scan_forms.py      ->  tests/golden/scan_forms.json

The file: the grid's axes, and per entry point its answers in the order `points()` walks them -- one row
(return code of *_form, Q, S, *_workspace_bytes) per grid point, Q = S = 0 where the form was refused -- as int64,
little-endian, zlib-compressed, base64: 225 000 rows in plain JSON would be several times the size a committed file may have.
`decode()` gives the rows back; `ENTRIES[name].axes` names the grid point of a row.
"""
import base64
import ctypes as C
import itertools
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "scan_forms.json")

GRID = {
    "B": [1, 3, 16, 256, 16384],
    "N": [1, 63, 64, 255, 256, 257, 1024, 2049, 16384, 70001, 131072, 131073],
    "cu": [1, 256, 304],
    "Q": [0, 1, 2, 4, 3],                                   # forced; 3 is no form
    "S": [0, 1, 3, 128, 129],                               # forced; 129 is past the limit
    "mutual": [0, 1],
}


class Entry:
    """One entry point: its module, the args for a shape (as the module's *_form helper fills them) and the grid's axes."""

    def __init__(self, module, prefix, args, axes):
        self.module, self.prefix, self.args, self.axes = module, prefix, args, axes

    def points(self):
        return itertools.product(*(GRID["N" if a in ("Ns", "Nt") else a] for a in self.axes))


ENTRIES = {                                                 # (the pointers are never dereferenced on the host)
    "vcr_nn_score": Entry("score", "vcr_nn_score",
                          lambda m, B, Ns, Nt, **_: m.NnScoreArgs(0x1000, 0x2000, B, Ns, Nt, None, None, 0.0, None, None, None,
                                                                  None, 0x3000, 0x4000, 0),
                          ("cu", "B", "Ns", "Nt", "Q", "S")),
    "vcr_refine": Entry("refine", "vcr_refine",
                        lambda m, B, Ns, Nt, **_: m.RefineArgs(src=0x1000, tgt=0x2000, B=B, Ns=Ns, Nt=Nt, max_iterations=30,
                                                               R_out=0x3000, t_out=0x4000, fitness=0x5000, rmse=0x6000),
                        ("cu", "B", "Ns", "Nt", "Q", "S")),
    "vcr_voxel": Entry("voxel", "vcr_voxel", lambda m, B, N, **_: m.VoxelArgs(0x1000, B, N, 1.0, 0x2000, 0x3000, None, None, 0),
                       ("cu", "B", "N", "Q", "S")),
    "vcr_outlier_radius": Entry("outlier", "vcr_outlier_radius",
                                lambda m, B, N, **_: m.RadiusArgs(0x1000, B, N, 1.0, 0, 0x2000, 0x3000, None, None, 0),
                                ("cu", "B", "N", "Q", "S")),
    "vcr_feat_nn": Entry("match", "vcr_feat_nn",
                         lambda m, B, Ns, Nt, mutual, **_: m.FeatNnArgs(0x1000, 0x2000, B, m.FEAT_C, Ns, Nt, 0x3000, None, mutual,
                                                                        None, 0),
                         ("mutual", "cu", "B", "Ns", "Nt", "Q", "S")),
}


def answers(name):
    """The library's rows for one entry point: int64 [points, 4] = (rc, Q, S, workspace bytes)."""
    sys.path.insert(0, ROOT)
    import importlib
    import vcrnet_amd  # noqa: F401
    e = ENTRIES[name]
    mod = importlib.import_module("vcrnet_amd." + e.module)
    L = mod.lib()
    form, size = getattr(L, e.prefix + "_form"), getattr(L, e.prefix + "_workspace_bytes")
    q, s = C.c_int(0), C.c_int(0)
    pq, ps = C.byref(q), C.byref(s)
    rows, shape, a = [], None, None
    for point in e.points():
        kw = dict(zip(e.axes, point))
        cu, fq, fs = kw.pop("cu"), kw.pop("Q"), kw.pop("S")
        if kw != shape:
            shape, a = kw, e.args(mod, **kw)
        a.variant = fq | fs << 8
        q.value = s.value = 0
        rc = form(C.byref(a), cu, pq, ps)
        rows.append((rc, q.value if rc == 0 else 0, s.value if rc == 0 else 0, size(C.byref(a), cu)))
    return np.asarray(rows, dtype="<i8")


def encode(rows):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(rows, dtype="<i8").tobytes(), 9)).decode("ascii")


def decode(text):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype="<i8").reshape(-1, 4)


if __name__ == "__main__":
    out = {"grid": GRID, "row": ["rc", "Q", "S", "workspace_bytes"], "entries": {}}
    for name, e in ENTRIES.items():
        rows = answers(name)
        out["entries"][name] = {"axes": list(e.axes), "rows": len(rows), "data": encode(rows)}
        ok = rows[:, 0] == 0
        print(name, len(rows), "rows,", int(ok.sum()), "served,", {int(c): int((rows[:, 0] == c).sum()) for c in set(rows[~ok, 0])})
    with open(PATH, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(PATH, f"{os.path.getsize(PATH) / 1024:.0f} KiB")
