"""What csrc/wg_scan.h computes, in numpy: unsigned 32-bit sums, that is numpy.cumsum in uint64 reduced mod 2^32 (an
element count far below 2^32 keeps the uint64 sum itself exact)."""
import numpy as np

MASK = np.uint64(0xFFFFFFFF)


def exclusive_scan(v):
    """v [..., n] uint32 -> (the exclusive prefix sums along the last axis, the totals), mod 2^32"""
    v = np.asarray(v, dtype=np.uint32)
    incl = np.cumsum(v.astype(np.uint64), axis=-1, dtype=np.uint64)
    excl = (incl - v.astype(np.uint64)) & MASK
    total = (incl[..., -1] & MASK) if v.shape[-1] else np.zeros(v.shape[:-1], dtype=np.uint64)
    return excl.astype(np.uint32), total.astype(np.uint32)


def exclusive_scan_valid(v, valid):
    """the scan of v with the elements where `valid` is False counted as 0 (whatever bits they hold)"""
    return exclusive_scan(np.where(valid, np.asarray(v, dtype=np.uint32), np.uint32(0)))
