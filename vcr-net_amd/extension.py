"""What the bindings of the headers beside include/vcr_hip.h repeat (``score``, ``refine``, ``plane``): the library with a
module's SIGNATURES applied, the prototypes of an entry point that takes a workspace, the checks of a cloud pair and its pose,
the guarded output buffers of the tests, and the call that sizes, allocates and passes the workspace.  `api` is the public
function's name, as the error messages carry it."""
from __future__ import annotations

import ctypes as C
import torch

from . import native
from .native import VcrHipError

_int, _size, _vp = C.c_int, C.c_size_t, C.c_void_p
_intp = C.POINTER(C.c_int)


def workspace_signatures(entry, Args):
    """name -> (restype, [argtypes]) of the three entry points `entry`_workspace_bytes / _f32 / _form over the struct Args."""
    return {entry + "_workspace_bytes": (_size, [C.POINTER(Args), _int]),
            entry + "_f32": (_int, [C.POINTER(Args), _vp, _size, _vp]),
            entry + "_form": (_int, [C.POINTER(Args), _int, _intp, _intp])}


def workspace_signatures2(entry, Args, Second):
    """As workspace_signatures, for entry points that take a second struct behind the first (include/vcr_hip_gridnn.h); their
    _form reports three ints."""
    return {entry + "_workspace_bytes": (_size, [C.POINTER(Args), C.POINTER(Second), _int]),
            entry + "_f32": (_int, [C.POINTER(Args), C.POINTER(Second), _vp, _size, _vp]),
            entry + "_form": (_int, [C.POINTER(Args), C.POINTER(Second), _int, _intp, _intp, _intp])}


def typed_lib(signatures):
    """-> lib(): native.lib() with `signatures` applied to it (once)."""
    typed = []

    def lib() -> C.CDLL:
        L = native.lib()
        if not typed:
            for name, (res, args) in signatures.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
            typed.append(True)
        return L
    return lib


def form(L, entry, a, cu_count):
    """`entry`_form and _workspace_bytes on the args a: (source points per lane, target splits, workspace bytes)."""
    q, s = C.c_int(0), C.c_int(0)
    native.check(getattr(L, entry + "_form")(C.byref(a), cu_count, C.byref(q), C.byref(s)), entry + "_form")
    return q.value, s.value, getattr(L, entry + "_workspace_bytes")(C.byref(a), cu_count)


def call_with_workspace(L, entry, a, dev, prefill=None, second=None):
    """`entry`_f32 on the args a with the workspace `entry`_workspace_bytes asks for, 256-aligned (filled with the byte
    `prefill` first).  second: the struct an entry point of workspace_signatures2 takes behind a."""
    f32, workspace_bytes = getattr(L, entry + "_f32"), getattr(L, entry + "_workspace_bytes")
    structs = (C.byref(a),) if second is None else (C.byref(a), C.byref(second))
    need = workspace_bytes(*structs, 0)
    if need == 0:                                            # refused: let the entry point say why
        native.check(f32(*structs, None, 0, native.stream_ptr()), entry + "_f32")
        raise VcrHipError(f"{entry}_workspace_bytes: 0 for arguments {entry}_f32 accepts")
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    if prefill is not None:
        ws.fill_(prefill)
    off = (-ws.data_ptr()) % 256
    native.check(f32(*structs, ws.data_ptr() + off, need, native.stream_ptr()), entry + "_f32")


def outputs(dev, guard=0, prefill=None):
    """-> (out, raw): out(name, n, dtype) is a view of n elements of a buffer with `guard` more behind it, all of it filled
    with the byte `prefill`; the buffers gather in raw under their names."""
    raw = {}

    def out(name, n, dtype):
        buf = torch.empty(n + guard, dtype=dtype, device=dev)
        if prefill is not None:
            buf.view(torch.uint8).fill_(prefill)
        raw[name] = buf
        return buf[:n]
    return out, raw


def check_cloud(api, name, x):
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != 3:
        raise VcrHipError(f"{api}: {name} must be a [B, 3, N] point cloud, got "
                          f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")


def check_pair(api, src, tgt, R, t):
    """What can be said of src [B,3,Ns], tgt [B,3,Nt] and the pose before any other argument is looked at."""
    check_cloud(api, "src", src)
    check_cloud(api, "tgt", tgt)
    if src.shape[0] != tgt.shape[0]:
        raise VcrHipError(f"{api}: src and tgt must hold the same number of clouds, got {src.shape[0]} "
                          f"and {tgt.shape[0]}")
    if not (src.is_cuda and tgt.is_cuda):
        raise VcrHipError(f"{api} runs on the MI355X HIP path only; move the clouds to cuda "
                          "(there is no CPU fallback by design)")
    if (R is None) != (t is None):
        raise VcrHipError(f"{api}: give both R and t, or neither (the identity)")


def take_pair(api, src, tgt, R, t):
    """-> (device, B, Ns, Nt, src, tgt, R, t): the checked pair on one device, contiguous fp32, the pose R [B,3,3], t [B,3]."""
    dev = native.same_device(src, tgt, R, t)
    B, _, Ns = src.shape
    Nt = tgt.shape[2]
    src, tgt = src.contiguous().float(), tgt.contiguous().float()
    if R is not None:
        if tuple(R.shape) != (B, 3, 3) or tuple(t.shape) != (B, 3):
            raise VcrHipError(f"{api}: R must be [B, 3, 3] and t [B, 3] with B = {B}, got {tuple(R.shape)} "
                              f"and {tuple(t.shape)}")
        R, t = R.contiguous().float(), t.contiguous().float()
    return dev, B, Ns, Nt, src, tgt, R, t
