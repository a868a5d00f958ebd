#!/usr/bin/env python
"""Record what the REFERENCE's farthest_point_sample (util/util.py:107-140) returns, so that the CPU restatement
(tests/fps_restated.py) and through it the device kernels (vcr_fps_f32) are pinned to the reference instead of to themselves.

Runs only in the build container (needs /root/reference); the GPU box never sees the reference, only the .npz files this
script writes.  util/util.py calls NVML at import (absent on AMD): a MagicMock stands in for pynvml; farthest_point_sample
itself runs unmodified, on the CPU.

  python tests/golden/gen_fps_golden.py      ->  tests/golden/fps_*.npz

Every file: xyz [B,3,N] fp32, npoint, and per entry of `scales` the reference's indices idx_s<k> [B,npoint] (int32) for the
input xyz * fp32(scale) -- an fp32 product, so a test rebuilds the input bit for bit.  use_start = 1: the clouds have exact
ties / copies, where the reference's fp32 barycentre start is a rounding decision: tests hand the reference's first index to
the kernel as `start`.  use_start = 0: the barycentre rule is tested too, and this script ASSERTS that the reference's own
decision is not marginal there (relative gap between its largest and second-largest |p - c|^2 of at least 1e-4; no cloud
is skipped -- pick another seed instead); the gaps are recorded as margin_s<k> [B].  A non-finite cloud is exempt (NaN in
margin_s<k>): its start is decided by torch.max's NaN rule, not by rounding.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.modules["pynvml"] = MagicMock()
sys.path.insert(0, REF)

from util.util import farthest_point_sample               # noqa: E402

MIN_MARGIN = 1e-4


def reference_margin(xyz):
    """The reference's own start decision (util.py:125-130, its tensors, its summation order): relative gap of the two
    largest distances from its barycentre, per cloud."""
    p = torch.from_numpy(xyz).transpose(2, 1)
    c = (torch.sum(p, 1) / p.shape[1]).view(-1, 1, 3)
    d = torch.sum((p - c) ** 2, -1).double()
    top = torch.topk(d, 2, dim=1)[0]
    m = ((top[:, 0] - top[:, 1]) / top[:, 0]).numpy()
    m[~np.isfinite(xyz).all(axis=(1, 2))] = np.nan
    return m


def uniform(seed, B, N):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(B, 3, N)).astype(np.float32)


def lattice(seed, B, N):
    """N points drawn with replacement from a 5 x 5 x 4 lattice: ~95 distinct points, exact ties and copies everywhere."""
    rs = np.random.RandomState(seed)
    grid = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), 0).reshape(3, -1).astype(np.float32) * 0.25
    return np.stack([grid[:, rs.randint(0, grid.shape[1], size=N)] for _ in range(B)])


def poked(seed, B, N, pokes):
    """uniform clouds with cloud 0 made non-finite: pokes = [(point, coordinate, value)]; the other clouds stay finite."""
    x = uniform(seed, B, N)
    for n, c, v in pokes:
        x[0, c, n] = v
    return x


CASES = {  # name: (xyz, npoint, scales, use_start)
    "uniform_b3_n1000_p64": (uniform(11, 3, 1000), 64, (1e-3, 1.0, 30.0), 0),
    "uniform_b2_n5000_p512": (uniform(12, 2, 5000), 512, (1e-3, 1.0, 30.0), 0),
    "uniform_b2_n20000_p1024": (uniform(13, 2, 20000), 1024, (1e-3, 1.0, 30.0), 0),
    "uniform_b1_n70001_p2048": (uniform(14, 1, 70001), 2048, (1e-3, 1.0, 30.0), 0),
    "lattice_b2_n257_p257": (lattice(15, 2, 257), 257, (1.0,), 1),
    "uniform_b2_n100_p150": (uniform(16, 2, 100), 150, (1.0,), 0),              # npoint > N: points repeat
    "nan_b2_n300_p32": (poked(17, 2, 300, [(7, 1, np.nan)]), 32, (1.0,), 0),
    "inf_b2_n300_p32": (poked(18, 2, 300, [(41, 0, np.inf)]), 32, (1.0,), 0),
    "neginf_b2_n300_p32": (poked(19, 2, 300, [(5, 2, -np.inf)]), 32, (1.0,), 0),
    "naninf_b2_n300_p32": (poked(20, 2, 300, [(9, 0, np.nan), (200, 1, np.inf), (201, 1, -np.inf)]), 32, (1.0,), 0),
    "repeated_b2_n64_p16": (np.repeat(uniform(21, 2, 1), 64, axis=2), 16, (1.0,), 1),
    "single_b2_n1_p5": (uniform(22, 2, 1), 5, (1.0,), 1),
    "uniform_b2_n500_p1": (uniform(23, 2, 500), 1, (1.0,), 0),
}

if __name__ == "__main__":
    for name, (xyz, npoint, scales, use_start) in CASES.items():
        out = {"xyz": xyz, "npoint": np.int32(npoint), "scales": np.asarray(scales, np.float32), "use_start": np.int32(use_start)}
        for k, s in enumerate(scales):
            x = xyz * np.float32(s)
            assert x.dtype == np.float32
            with torch.no_grad():
                idx = farthest_point_sample(torch.from_numpy(x), npoint).numpy()
            assert idx.shape == (xyz.shape[0], npoint) and idx.min() >= 0 and idx.max() < xyz.shape[2]
            out[f"idx_s{k}"] = idx.astype(np.int32)
            if not use_start:
                m = reference_margin(x)
                assert (np.isnan(m) | (m >= MIN_MARGIN)).all(), (name, s, m)        # the reference's start is not a rounding decision here
                out[f"margin_s{k}"] = m
        path = os.path.join(HERE, f"fps_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, xyz.shape, npoint, f"{os.path.getsize(path) / 1024:.0f} KiB")
