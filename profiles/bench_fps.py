#!/usr/bin/env python
"""Farthest-point sampling (vcr_fps_f32) against the reference's algorithm itself: the loop of farthest_point_sample
(util/util.py:107-140) restated with torch device ops, on the same GPU, the same inputs, in the same process, alternated with
the kernel.  There is no parent-commit time to compare with: the library had no such function.

Shapes: B = 32 clouds (configs[1]'s two times sixteen) and B = 2 (one pair) sampled 4096 -> 1024, 16 384 -> 1024,
65 536 -> 2048, 131 072 -> 4096.  Per shape and contender: ms per call (device events around `--calls` calls after a warm-up,
taken in two alternated halves), us per round, the ratio to the kernel's automatic form; every form is forced where more than
one applies.  The kernel's indices are compared index for index with the CPU restatement (tests/fps_restated.py) on the
first two clouds of every shape, and with the torch loop's on all of them.  Last, once: what register_sampled costs end to end
at 16 384 -> 1024, B = 16, next to the forward it feeds.

  python profiles/bench_fps.py [--calls 20] [--kernel-only] [--quick]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vcrnet_amd  # noqa: E402,F401
import fps_restated as fr  # noqa: E402
from vcrnet_amd import build, native  # noqa: E402

SHAPES = ((4096, 1024), (16384, 1024), (65536, 2048), (131072, 4096))
FORM_NAMES = {0: "auto", 1: "resident", 2: "streaming"}


def torch_loop(xyz, npoint):
    """The reference's loop, operation for operation, on channels-first device tensors: at least eight launches a round."""
    B, _, N = xyz.shape
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    dist = torch.ones(B, N, device=xyz.device) * 1e10
    rows = torch.arange(B, dtype=torch.long, device=xyz.device)
    c = torch.sum(xyz, 2) / N
    d = (x - c[:, 0:1]) ** 2 + (y - c[:, 1:2]) ** 2 + (z - c[:, 2:3]) ** 2
    far = torch.max(d, 1)[1]
    for i in range(npoint):
        out[:, i] = far
        p = xyz[rows, :, far]
        d = (x - p[:, 0:1]) ** 2 + (y - p[:, 1:2]) ** 2 + (z - p[:, 2:3]) ** 2
        dist = torch.where(d < dist, d, dist)
        far = torch.max(dist, -1)[1]
    return out


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def clouds(B, N):
    """uniform in [-1, 1]^3, cloud b from seed 9000 + b whatever B is: the first two clouds of B = 32 are the clouds of B = 2."""
    return np.stack([np.random.RandomState(9000 + b).uniform(-1, 1, (3, N)).astype(np.float32) for b in range(B)])


def bench_shape(B, N, npoint, calls, kernel_only):
    x_np = clouds(B, N)
    x = torch.from_numpy(x_np).cuda()
    auto_form, ppt = native.fps_form(N, npoint, B)
    forms = [0] + ([1, 2] if auto_form == 1 else [])
    res = {}
    contenders = [(FORM_NAMES[v] if v else f"auto={FORM_NAMES[auto_form]}/{ppt}", (lambda v=v: res.__setitem__(v, native.fps(x, npoint, variant=v)[0])), calls)
                  for v in forms]
    if not kernel_only:
        contenders.append(("torch loop", lambda: res.__setitem__("torch", torch_loop(x, npoint)), None))
    times = {}
    for name, fn, c in contenders:                            # warm every contender; size the slow one's call count
        fn()
        torch.cuda.synchronize()
        one = timed(fn, 1)
        times[name] = [max(2, (calls if one < 250.0 else 4) // 2) if c is None else max(1, c // 2)]
    for half in range(2):                                     # two alternated halves
        for name, fn, _ in contenders:
            times[name].append(timed(fn, times[name][0]))
    want = fr.fps(x_np[:2], npoint)
    ok_cpu = all(np.array_equal(res[v][:2].cpu().numpy(), want) for v in forms)
    ok_all = all(torch.equal(res[v], res[0]) for v in forms)
    ok_torch = None if kernel_only else bool(torch.equal(res["torch"].int(), res[0]))
    base = None
    for name, _, _ in contenders:
        n, t1, t2 = times[name]
        ms = 0.5 * (t1 + t2)
        base = ms if base is None else base
        print(f"B={B:2d} {N:6d} -> {npoint:4d}  {name:22s} {ms:10.3f} ms/call  {ms * 1e3 / npoint:8.2f} us/round  "
              f"x{ms / base:7.2f} of auto   ({2 * n} calls; halves {t1:.3f} / {t2:.3f})", flush=True)
    print(f"B={B:2d} {N:6d} -> {npoint:4d}  indices: restatement (clouds 0-1) {ok_cpu}, forms agree {ok_all}, torch loop (all clouds) {ok_torch}",
          flush=True)
    assert ok_cpu and ok_all, "the kernel's indices differ from the restatement's"


def bench_register(calls):
    from types import SimpleNamespace
    from vcrnet_amd import weights
    from vcrnet_amd.module import VCRNet, register_sampled, vcrnetIter
    args = SimpleNamespace(emb_dims=512, cycle=False, emb_nn="lpdnet", pointer="transformer", vcp_nn="topK", partial=False,
                           overlap2=0.75, t3d=False, tfea=False, n_blocks=1, dropout=0.0, ff_dims=1024, n_heads=4)
    net = VCRNet(args)
    net.load_state_dict(weights.generate_weights(1234, lpd=weights.load_lpd_fixture()))
    net = net.cuda().eval()
    B, N, npoint = 16, 16384, 1024
    src = torch.from_numpy(clouds(B, N)).cuda()
    tgt = torch.from_numpy(clouds(2 * B, N)[B:]).cuda()
    with torch.no_grad():
        _, s = native.fps(src, npoint)
        _, t = native.fps(tgt, npoint)
        full = lambda: register_sampled(net, src, tgt, npoint)
        fwd = lambda: vcrnetIter(net, s, t, 1)
        two = lambda: (native.fps(src, npoint), native.fps(tgt, npoint))
        for f in (full, fwd, two):
            f()
        torch.cuda.synchronize()
        for name, f in (("register_sampled 16384 -> 1024, B=16", full), ("  vcrnetIter on the sampled clouds", fwd), ("  the two fps launches", two)):
            t1, t2 = timed(f, calls), timed(f, calls)
            print(f"{name:40s} {0.5 * (t1 + t2):8.3f} ms/call  ({2 * calls} calls; halves {t1:.3f} / {t2:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="no torch loop (the run under rocprofv3 --kernel-trace)")
    ap.add_argument("--quick", action="store_true", help="the two small shapes only")
    a = ap.parse_args()
    print(f"kernel sources {build.sources_sha16()}  device {torch.cuda.get_device_name(0)}  calls {a.calls}", flush=True)
    for B in (32, 2):
        for N, npoint in (SHAPES[:2] if a.quick else SHAPES):
            bench_shape(B, N, npoint, a.calls, a.kernel_only)
    if not a.kernel_only:
        bench_register(a.calls)


if __name__ == "__main__":
    main()
