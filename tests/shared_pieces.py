"""Loader of tests/native/libbsr_shared_pieces.so (tests/native/shared_pieces.hip: the product's wg_scan.h, grid_sum.h and
mlp_wgrad.* behind test-only entry points) and the few idioms its three GPU test modules share."""
import ctypes as C
import functools
import os

import numpy as np
import torch

DEV = "cuda:0"
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libbsr_shared_pieces.so")


@functools.lru_cache(maxsize=None)
def lib():
    assert os.path.exists(PATH), f"{PATH} missing: run __graft_entry__.build()"
    L = C.CDLL(PATH)
    L.pt_mlp_wgrad_layout.restype = None
    L.pt_mlp_wgrad_layout.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_size_t)]
    return L


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def u32(a):
    """numpy uint32 -> a device tensor of the same bits (torch has no arithmetic on uint32: int32 carries them)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)
