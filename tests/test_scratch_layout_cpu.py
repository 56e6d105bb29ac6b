"""The layout of the three caller-owned scratch buffers (bloomscene_amd/csrc/scratch.h), held against its two other
statements: the sizes the product library reports (bsr_geometry_bytes / bsr_binning_bytes / bsr_image_bytes) and the
Python mirror the GPU suite decodes the buffers with (helpers.scratch_offsets).

scratch.h is compiled into tests/native/libbsr_pure_functions.so (pt_scratch_layout: host code, no GPU), which carves
every state from an aligned base and hands back the section offsets.  Every byte of device memory the library touches
lies in one of these sections, so what is pinned here is that they do not overlap (except the radix ping-pong pair
with the backward's slab, which are the same bytes on purpose), that they end inside the size the caller was told, and
that the backward's carve of a buffer -- point_list[R], then R slab rows -- ends before the histogram section."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = ("rec", "inst_offset", "wg_kept", "wg_area", "hist1", "kept_mask", "rect", "clamped", "depth")
BIN = ("point_list", "elems_a", "elems_b", "slab", "hist")
IMG = ("final_T", "n_contrib", "tile_range", "flags", "big_tiles")
N_OUT = 3 + len(GEOM) + len(BIN) + len(IMG) + 2


def _load(path, what):
    if not os.path.exists(path):
        pytest.skip(f"{what} not built (run __graft_entry__.build())")
    try:
        return C.CDLL(path)
    except OSError as e:                 # (no HIP runtime on this host)
        pytest.skip(str(e))


@pytest.fixture(scope="module")
def libs():
    pure = _load(os.path.join(ROOT, "tests", "native", "libbsr_pure_functions.so"), "tests/native/libbsr_pure_functions.so")
    prod = _load(os.path.join(ROOT, "bloomscene_amd", "libbloomscene_rast.so"), "bloomscene_amd/libbloomscene_rast.so")
    pure.pt_scratch_layout.argtypes = [C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    pure.pt_scratch_layout.restype = None
    for name, args in (("bsr_geometry_bytes", [C.c_int]), ("bsr_binning_bytes", [C.c_int]), ("bsr_image_bytes", [C.c_int, C.c_int])):
        getattr(prod, name).argtypes = args
        getattr(prod, name).restype = C.c_size_t
    return pure, prod


def _layout(pure, P=0, R=0, with_slab=True, W=1, H=1):
    """(totals, geometry offsets, binning offsets, image offsets, slab row bytes, slab tail bytes) as scratch.h has them"""
    out = np.zeros(N_OUT, dtype=np.uint64)
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    pure.pt_scratch_layout(P, R, int(with_slab), N, T, out.ctypes.data)
    v = [int(x) for x in out]
    g = dict(zip(GEOM, v[3:]))
    b = dict(zip(BIN, v[3 + len(GEOM):]))
    i = dict(zip(IMG, v[3 + len(GEOM) + len(BIN):]))
    return SimpleNamespace(geom=v[0], bin=v[1], img=v[2]), g, b, i, v[-2], v[-1]


def _check_sections(offsets, payload, total, same_bytes=()):
    """offsets / payload: section -> offset / bytes the section must hold, in layout order.  Aligned, inside the total
    less the 256 bytes of alignment slack, and disjoint except for the pairs named in same_bytes."""
    names = list(offsets)
    for n in names:
        assert offsets[n] % 256 == 0, (n, offsets[n])
        assert offsets[n] + payload[n] <= total - 256, (n, offsets[n], payload[n], total)
    for k, a in enumerate(names):
        for b in names[k + 1:]:
            if (a, b) in same_bytes:
                continue
            a0, a1, b0, b1 = offsets[a], offsets[a] + payload[a], offsets[b], offsets[b] + payload[b]
            assert a1 <= b0 or b1 <= a0, (a, b, a0, a1, b0, b1)


def _counts():
    """0, 1, the 256 boundaries, 5000 consecutive values, and sizes up to a few million around powers of two and at
    random"""
    rng = np.random.default_rng(0)
    s = set(range(0, 5000)) | {255, 256, 257}
    for k in range(12, 22):
        s |= {(1 << k) - 1, 1 << k, (1 << k) + 1, (1 << k) + 255, (1 << k) + 257}
    s |= {2_999_999, 3_000_000}
    s |= {int(x) for x in rng.integers(5000, 3_000_000, 400)}
    return sorted(s)


SIDES = (1, 2, 15, 16, 17, 31, 33, 100, 255, 257, 270, 480, 800, 1080, 1920, 4095, 4096)


def test_geometry_layout_equals_the_library_and_the_python_mirror(libs):
    pure, prod = libs
    for P in _counts():
        tot, g, _, _, _, _ = _layout(pure, P=P)
        assert tot.geom == prod.bsr_geometry_bytes(P), P
        mirror, _ = Hh.scratch_offsets(P, 16, 16)
        for name, off in vars(mirror).items():
            assert g[name] == off, (P, name)
        n_wg = (P + 255) // 256
        payload = dict(rec=P * 64, inst_offset=P * 4, wg_kept=n_wg * 4, wg_area=n_wg * 4,
                       hist1=(256 * 8 * ((n_wg + 7) // 8) + 512) * 4, kept_mask=P * 8, rect=P * 8, clamped=P, depth=P * 4)
        _check_sections(g, payload, tot.geom)


def test_image_layout_equals_the_library_and_the_python_mirror(libs):
    pure, prod = libs
    for W in SIDES:
        for H in SIDES:
            tot, _, _, i, _, _ = _layout(pure, W=W, H=H)
            assert tot.img == prod.bsr_image_bytes(W, H), (W, H)
            _, mirror = Hh.scratch_offsets(0, W, H)
            for name, off in vars(mirror).items():
                assert i[name] == off, (W, H, name)
            N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
            payload = dict(final_T=N * 4, n_contrib=N * 4, tile_range=T * 8, flags=512, big_tiles=3 * T * 4)
            _check_sections(i, payload, tot.img)


def test_binning_layout_equals_the_library_and_holds_the_backwards_slab(libs):
    pure, prod = libs
    for R in _counts():
        for with_slab in (True, False):
            tot, _, b, _, row, tail = _layout(pure, R=R, with_slab=with_slab)
            assert (row, tail) == (40, 16)
            if with_slab:
                assert tot.bin == prod.bsr_binning_bytes(R), R
            slab = R * row + tail if with_slab else 0
            payload = dict(point_list=R * 4, elems_a=R * 12, elems_b=R * 12, slab=slab, hist=256 * (2048 + 1) * 4)
            _check_sections(b, payload, tot.bin, same_bytes={("elems_a", "slab"), ("elems_b", "slab")})
            assert b["slab"] == b["elems_a"], R
            if with_slab:
                # what the backward relies on: point_list[R], then R slab rows and the reader's tail, end before hist
                assert b["slab"] == (R * 4 + 255) // 256 * 256, R
                assert b["slab"] + R * row + tail <= b["hist"], R
