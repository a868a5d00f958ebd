"""CPU restatement of the ROUTE vcr_voxel_sort_f32 takes (include/vcr_hip_voxel_sort.h) in numpy: the
axes' bit widths from the largest cell, the packed keys, stable least-significant-digit passes of (key, index), the heads of the
sorted order, the voxel numbers as the ranks of the representatives in index order, the fp64 sums in segment order and the member
lists.  tests/test_voxel_sort_cpu.py holds it to tests/voxel_restated.py -- the definition -- bit for bit; the GPU tests compare
the kernels with both.  Also the definition of the member lists in one line each, and the recipes in which the order of a sum
shows."""
import numpy as np

import voxel_restated as vr

F32 = np.float32
OUTPUTS = ("points", "count", "point_voxel", "voxel_points", "members", "voxel_start")


def _empty(N, count):
    out = vr._empty(N, count)
    out["members"] = np.full(N, -1, np.int32)
    out["voxel_start"] = np.zeros(N, np.int32)
    return out


def widths(xyz, h):
    """xyz [3, N] -> (finite [N], cells [3, N] float64, (w_x, w_y, w_z)) or (finite, None, None) for a cloud without a finite
    point or too fine: the width of an axis is the bit length of its largest cell, the cell of the fp32 maximum."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    finite, cells = vr._cells(xyz, h)
    if cells is None:
        return finite, None, None
    hi = xyz[:, finite].max(axis=1)
    lo = xyz[:, finite].min(axis=1)
    hd = np.float64(F32(h))
    with np.errstate(over="ignore", invalid="ignore"):
        top = np.floor((hi.astype(np.float64) - (lo.astype(np.float64) - 0.5 * hd)) / hd)
    if not (top < vr.MAX_CELLS).all():
        return finite, cells, None
    return finite, cells, tuple(int(t).bit_length() for t in top)


def passes_needed(W, bits):
    return (W + 1 + bits - 1) // bits


def stable_pass(keys, idx, shift, bits):
    """One pass: every element goes to [elements of a lower digit] + [elements of its digit in front of it]."""
    digit = ((keys >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    counts = np.bincount(digit, minlength=1 << bits)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    in_front = np.empty(len(keys), np.int64)                                     # of the same digit
    by_digit = np.argsort(digit, kind="stable")
    in_front[by_digit] = np.arange(len(keys)) - start[digit[by_digit]]
    to = start[digit] + in_front
    k2, i2 = np.empty_like(keys), np.empty_like(idx)
    k2[to], i2[to] = keys, idx
    return k2, i2


def ordered_sums(x64, order, first, members):
    """Per voxel the fp64 sum of x64[:, order[first : first + members]], starting AS the first and in that order."""
    sums = x64[:, order[first]].copy()
    for k in range(1, int(members.max())):
        has = np.flatnonzero(members > k)
        sums[:, has] = sums[:, has] + x64[:, order[first[has] + k]]
    return sums


def voxel_sort(xyz, h, bits=8, disturb=None):
    """xyz [3, N] fp32, h, the digit width -> voxel_restated's dict with members and voxel_start.  disturb(idx sorted) -> idx:
    a hook for the tests to break the order inside the sorted list (what a sort that is not stable would do)."""
    xyz = np.ascontiguousarray(xyz, dtype=F32)
    N = xyz.shape[1]
    finite, cells, w = widths(xyz, h)
    if cells is None:
        return _empty(N, 0)
    if w is None:
        return _empty(N, -1)
    W = sum(w)
    assert W <= 63 and max(w) <= 21
    c = np.where(finite, cells, 0.0).astype(np.uint64)
    keys = c[0] | c[1] << np.uint64(w[0]) | c[2] << np.uint64(w[0] + w[1])
    assert (keys[finite] >> np.uint64(W) == 0).all() if W < 64 else True
    keys = np.where(finite, keys, np.uint64(1) << np.uint64(W))                  # the bit above: behind every voxel
    idx = np.arange(N, dtype=np.int64)
    for p in range(passes_needed(W, bits)):
        keys, idx = stable_pass(keys, idx, p * bits, bits)
    if disturb is not None:
        idx = disturb(idx)
    voxel = (keys >> np.uint64(W)) == 0
    head = voxel & np.concatenate([[True], keys[1:] != keys[:-1]])
    is_rep = np.zeros(N, bool)
    is_rep[idx[head]] = True                                                      # a head's index is the lowest of its voxel
    number = np.cumsum(is_rep) - 1                                                # the rank among the representatives, by index
    head_slot = np.flatnonzero(head)
    M = len(head_slot)
    v_of_head = number[idx[head_slot]]
    first = np.empty(M, np.int64)
    first[v_of_head] = head_slot                                                  # per voxel its first sorted slot
    ends = np.concatenate([head_slot[1:], [int(voxel.sum())]])
    members = np.empty(M, np.int64)
    members[v_of_head] = ends - head_slot
    out = _empty(N, M)
    if M == 0:
        return out
    sums = ordered_sums(xyz.astype(np.float64), idx, first, members)
    out["points"][:, :M] = (sums / members.astype(np.float64)).astype(F32)
    out["voxel_points"][:M] = members
    seg = np.cumsum(head) - 1                                                     # per sorted slot its head
    out["point_voxel"][idx[voxel]] = v_of_head[seg[voxel]]
    start = np.concatenate([[0], np.cumsum(members)[:-1]])
    out["voxel_start"][:] = int(voxel.sum())
    out["voxel_start"][:M] = start
    slots = np.flatnonzero(voxel)
    v = v_of_head[seg[slots]]
    out["members"][start[v] + slots - first[v]] = idx[slots]
    return out


def batch(xyz, h, bits=8):
    res = [voxel_sort(c, h, bits) for c in xyz]
    return {k: np.stack([r[k] for r in res]) for k in res[0]}


def member_lists(point_voxel, count):
    """The definition of (members, voxel_start) from one cloud's point_voxel [N] and count: the finite points by a stable argsort
    of their voxel numbers; where voxel v begins."""
    N = len(point_voxel)
    members, start = np.full(N, -1, np.int32), np.zeros(N, np.int32)
    if count <= 0:
        return members, start
    at = np.flatnonzero(point_voxel >= 0)
    members[:len(at)] = at[np.argsort(point_voxel[at], kind="stable")]
    start[:] = len(at)
    start[:count] = np.concatenate([[0], np.cumsum(np.bincount(point_voxel[at], minlength=count))[:-1]])
    return members, start


def with_member_lists(want):
    """voxel_restated.batch's dict with the member lists by their definition."""
    lists = [member_lists(pv, int(c)) for pv, c in zip(want["point_voxel"], want["count"])]
    return dict(want, members=np.stack([m for m, _ in lists]), voxel_start=np.stack([s for _, s in lists]))


def same(a, b, outputs=OUTPUTS):
    return all(np.array_equal(vr.bits(a[k]), vr.bits(b[k])) for k in outputs)


# ---- recipes in which the ORDER of a sum shows (an ordinary cloud's fp64 sums are exact in any order) ----

CANCEL_H = float(2.0 ** 63)


def cancelling(seed, N):
    """[1, 3, N] in ONE voxel of edge 2^63: per coordinate a quarter of the values +2^k, a quarter -2^k (k from 20 ... 56, the
    same k's, so that they cancel over the voxel), the rest in [0.5, 1.5); all permuted."""
    rs = np.random.RandomState(seed)
    x = np.empty((1, 3, N), F32)
    q = N // 4
    for c in range(3):
        k = rs.randint(20, 57, size=q)
        v = np.concatenate([2.0 ** k, -(2.0 ** k), rs.uniform(0.5, 1.5, size=N - 2 * q)])
        x[0, c] = v[rs.permutation(N)].astype(F32)
    return x


def interleaved(seed, N):
    """cancelling() with x of every odd point moved by 2^64: two voxels interleaved across every block."""
    x = cancelling(seed, N)
    x[0, 0, 1::2] = (x[0, 0, 1::2].astype(np.float64) + 2.0 ** 64).astype(F32)
    return x


def shuffle_window(seed, lo, n=64):
    """disturb= hook: the sorted slots [lo, lo + n) permuted."""
    def disturb(idx):
        idx = idx.copy()
        idx[lo:lo + n] = idx[lo:lo + n][np.random.RandomState(seed).permutation(n)]
        return idx
    return disturb
