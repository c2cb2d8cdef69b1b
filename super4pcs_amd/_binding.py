"""What every ctypes binding of this package needs (icp, posegraph, normals and the modules on its library), stated once: the
signature table and its declaration, the loader's error, and the helpers for clouds and results that are numpy arrays or GPU
torch tensors.  capi.py, the binding the benchmark drives, stands on its own.

A signature table is a dict with one entry per C function, next to the Structure classes it refers to:

    SIGNATURES = {
        "s4p_x_create": [C.c_int32, C.POINTER(C.c_void_p)],          # name: argtypes; the restype is c_int32
        "s4p_x_destroy": (None, [C.c_void_p]),                        # name: (restype, argtypes)
        "s4p_x_run" + TWIN: [C.c_void_p, C.c_int64],                  # s4p_x_run and s4p_x_run_device, one signature
    }

names(SIGNATURES) is the module's symbol list, so the list and the argtypes are one statement.

Synchronisation: torch's copies and allocations run on torch's stream, the libraries work on their own.  cols() synchronises
after its column copies; a wrapper that allocates results for a _device entry point calls sync(like) immediately before the
library call, and nowhere else.
"""
import ctypes as C
import os

import numpy as np

TWIN = "[_device]"            # at the end of a table's key: the function and its _device form, with the same signature


def names(signatures):
    """The C names of a table in its order, each twin entry as the host form and then the _device form."""
    out = []
    for key in signatures:
        out += [key[:-len(TWIN)], key[:-len(TWIN)] + "_device"] if key.endswith(TWIN) else [key]
    return out


def declare(L, signatures, error=None):
    """restype and argtypes of every function of the table on the library L.  With error (an exception class taking (code,
    text) and naming its build step as error.REBUILD) a function L lacks raises it with code -7 before anything is declared;
    without, such a function is skipped (another build of the library, opened by a tool)."""
    missing = [s for s in names(signatures) if not hasattr(L, s)]
    if missing and error is not None:
        raise error(-7, "%s lacks %s: rebuild it (%s)" % (os.path.basename(getattr(L, "_name", "the library")), ", ".join(missing),
                                                          error.REBUILD))
    for key, sig in signatures.items():
        restype, argtypes = sig if isinstance(sig, tuple) else (C.c_int32, sig)
        for name in names([key]):
            if name not in missing:
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes


def open_library(path, error, what):
    """ctypes.CDLL(path); error with code -7 when `what` (the library's file name) is not there."""
    if not os.path.exists(path):
        raise error(-7, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % what)
    return C.CDLL(path)


def load(cache, path, tables, error, what):
    """The library at path, opened once per cache (a binding module's dict: path -> (library, the tables declared on it)),
    with every table of `tables` declared on it, each once.  A second path binds a second copy in the same process."""
    path = os.fspath(path)
    if path not in cache:
        cache[path] = (open_library(path, error, what), [])
    L, done = cache[path]
    for table in tables:
        if not any(table is d for d in done):
            declare(L, table, error)
            done.append(table)
    return L


def is_torch(t):
    return type(t).__module__.startswith("torch")


def cols(X):
    """(device?, three column pointers, n, keep-alive) of a numpy array or a GPU torch tensor."""
    if is_torch(X):
        import torch
        if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] == 3):
            raise ValueError("torch input must be a (N, 3) float32 tensor on the GPU")
        keep = [X[:, k].contiguous() for k in range(3)]
        torch.cuda.synchronize(X.device)              # the copies run on torch's stream; the library reads on its own
        return True, [c.data_ptr() for c in keep], int(X.shape[0]), keep
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("clouds are (N, 3)")
    keep = [np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(3)]
    return False, [c.ctypes.data for c in keep], int(X.shape[0]), keep


def empty(like, shape, np_dtype):
    """(array, pointer): a torch tensor on like's device when like is a tensor, else (like None) a numpy array."""
    if like is not None:
        import torch
        t = torch.empty(shape, dtype=getattr(torch, np.dtype(np_dtype).name), device=like.device)
        return t, t.data_ptr()
    a = np.empty(shape, np_dtype)
    return a, a.ctypes.data


def sync(like):
    """Waits for like's device (torch's allocations and copies before a library writes on its own stream); nothing for None."""
    if like is not None:
        import torch
        torch.cuda.synchronize(like.device)
