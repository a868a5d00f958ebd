"""Centring a cloud that lies far from the origin relative to its extent, and carrying a pose between the caller's frame and
the centred one.  Plain torch on the clouds' device -- a subtraction and a 3 x 3 product per cloud, no
kernel of its own and no host synchronisation.

Why: the six-unknown fits (point to plane, plane to plane) linearise a rotation about the frame's ORIGIN and apply it exactly,
so a residual rotation a at distance r from the origin overshoots by about a^2 r / 2; cond(A) of their normal equations grows
with r^2; and the kNN behind estimate_normals, compute_fpfh_feature and remove_statistical_outlier cancels in fp32 far from
the origin.  All three go away when each cloud is moved to its own centre first."""
from __future__ import annotations

import torch

from . import extension
from .native import VcrHipError


def _centre(api, name, c, B, dev):
    if not (torch.is_tensor(c) and tuple(c.shape) == (B, 3)):
        raise VcrHipError(f"{api}: {name} must be a [B, 3] = [{B}, 3] tensor, got "
                          f"{tuple(c.shape) if torch.is_tensor(c) else type(c).__name__}")
    if c.device != dev:
        raise VcrHipError(f"{api}: {name} must be on the device of the clouds ({dev}), got {c.device}")
    return c.contiguous().float()


def centred(xyz, centre=None, api="centred", name="centre"):
    """xyz [B,3,N] (a device tensor) -> (xyz_c float32 [B,3,N], c float32 [B,3]) with xyz_c = xyz - c, subtracted in fp32.
    centre None: per cloud and axis the mean of the FINITE coordinates (summed in float64, rounded once; 0 where there is
    none), computed on the device without a host synchronisation.  A given centre [B,3] is used as it is: with a c on the grid of
    the coordinates the subtraction is exact."""
    extension.check_cloud(api, "xyz", xyz)
    x = xyz.contiguous().float()
    if centre is None:
        ok = torch.isfinite(x)
        total = torch.where(ok, x, torch.zeros((), dtype=x.dtype, device=x.device)).double().sum(dim=2)
        c = (total / ok.sum(dim=2).clamp(min=1).double()).float()
    else:
        c = _centre(api, name, centre, x.shape[0], x.device)
    return x - c[:, :, None], c


def _shift(R, c_from, c_to):
    """R c_from - c_to in float64: what the centred frame adds to t."""
    return torch.einsum("bij,bj->bi", R.double(), c_from.double()) - c_to.double()


def centred_pose(R, t, c_src, c_tgt):
    """The pose (R [B,3,3], t [B,3]; src -> tgt in the caller's frame; both None = the identity) in the frames centred at
    c_src, c_tgt [B,3]: (R, t + R c_src - c_tgt), in float64 on the device, rounded once."""
    if R is None:
        R = torch.eye(3, dtype=torch.float32, device=c_src.device).expand(c_src.shape[0], 3, 3).contiguous()
        t = torch.zeros_like(c_src)
    return R, (t.double() + _shift(R, c_src, c_tgt)).float()


def uncentred_pose(R, t, c_src, c_tgt):
    """The inverse of ``centred_pose``: a pose found between clouds centred at c_src, c_tgt [B,3] in the caller's frame,
    (R, t - R c_src + c_tgt), in float64 on the device, rounded once."""
    return R, (t.double() - _shift(R, c_src, c_tgt)).float()


def take_centres(api, centre, src, tgt):
    """centre=True or a pair of [B,3] tensors -> (src_c, c_src, tgt_c, c_tgt): each cloud about its own centre."""
    if centre is True:
        given = (None, None)
    elif isinstance(centre, (tuple, list)) and len(centre) == 2:
        given = tuple(centre)
    else:
        raise VcrHipError(f"{api}: centre must be False, True or a pair (c_src, c_tgt) of [B, 3] tensors, got "
                          f"{type(centre).__name__}")
    src_c, c_src = centred(src, given[0], api, "centre[0]")
    tgt_c, c_tgt = centred(tgt, given[1], api, "centre[1]")
    return src_c, c_src, tgt_c, c_tgt
