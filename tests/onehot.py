"""One-hot upstreams: summation order taken out of the nine pair sums of the render backward.

With dL/dcolour kept at ONE pixel and zero elsewhere every per-pair term at every other pixel is exactly +-0; a Gaussian
occurs at most once in a tile's list and a pixel belongs to one tile, so each of the 9 P sums has at most one nonzero
term and is that term, in any order and any precision.  tests/test_onehot_oracle_cpu.py holds these premises on the CPU
oracle, tests/test_strict_backward_gpu.py uses them; this module is the one statement of the hot-pixel rule and of the
one-hot upstream that both share.  (A module of its own, not part of helpers.py: no file the existing tests import
changes with it.)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

import helpers as Hh

# the new dense ragged case of the one-hot tests: 3 x 2 tiles (the right column 8 pixels wide, the lower row 8 high),
# SH colour, a strongly non-default background
DENSE_RAGGED = dict(P=3000, W=40, H=24, deg=1, seed=31, scale_mul=10.0, bg=(1.0, 0.5, 0.0))

# local (x, y) offsets inside the 16 x 16 tile: every local column and every local row once, all four 8 x 8 quadrants
HOT_OFFSETS = tuple((i, (5 * i + 3) % 16) for i in range(16))


def hottest_tile(n_contrib, W, H):
    """(tx, ty) of the tile whose largest n_contrib is largest (the first one in row-major order on a tie)."""
    nc = np.asarray(n_contrib).reshape(H, W)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    best = [int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max()) for ty in range(gy) for tx in range(gx)]
    ty, tx = divmod(int(np.argmax(best)), gx)
    return tx, ty


def hot_pixels(n_contrib, W, H):
    """The hot pixels of a case, from the ORACLE's n_contrib [H * W]: HOT_OFFSETS inside the hottest tile, clipped to the
    image (a coordinate past the edge moves onto the edge) and deduplicated, plus the image's last pixel.  Sorted
    (x, y) pairs."""
    tx, ty = hottest_tile(n_contrib, W, H)
    pix = {(min(tx * 16 + ox, W - 1), min(ty * 16 + oy, H - 1)) for ox, oy in HOT_OFFSETS}
    pix.add((W - 1, H - 1))
    return sorted(pix)


def onehot_upstream(gC, x, y):
    """gC [3, H, W] kept at pixel (x, y), exact zeros everywhere else."""
    out = torch.zeros_like(gC)
    out[:, y, x] = gC[:, y, x]
    return out


def nine_sums(g):
    """[P, 9] view of an oracle gradient namespace in the order of its abs_sums: mean2D.x,y conic.x,y,w opacity
    colour r,g,b."""
    con = g.dL_dconic.reshape(-1, 4)
    return np.stack([g.dL_dmeans2D[:, 0], g.dL_dmeans2D[:, 1], con[:, 0], con[:, 1], con[:, 3], g.dL_dopacity[:, 0],
                     g.dL_dcolors[:, 0], g.dL_dcolors[:, 1], g.dL_dcolors[:, 2]], axis=1)


def nine_sums_hip(out):
    """The same [P, 9] from the dict test_parity_gpu._raw_backward returns."""
    return np.stack([out["mean2D"][:, 0], out["mean2D"][:, 1], out["conic"][:, 0], out["conic"][:, 1], out["conic"][:, 3],
                     out["opacity"][:, 0], out["color"][:, 0], out["color"][:, 1], out["color"][:, 2]], axis=1)


def contracted_oracle_nine_sums(c, upstreams):
    """The nine pair sums [P, 9] (order of nine_sums) of the contracted oracle build (oracle/libbsr_oracle_fma.so: see
    helpers.contracted_oracle_grads, which this follows) for each dL/dcolour of `upstreams` on ONE forward of case `c`.
    One child process for all of them (one process loads one oracle build); None if the build is unavailable or the
    child failed."""
    import pickle
    import subprocess
    import tempfile
    lib = os.path.join(Hh.ROOT, "oracle", "libbsr_oracle_fma.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(Hh.ROOT, "oracle"), "fma"], capture_output=True)
    if not os.path.exists(lib):
        return None
    c = SimpleNamespace(**vars(c))
    c.upstreams = list(upstreams)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "case.pkl"), "wb") as f:
            pickle.dump(c, f)
        code = ("import pickle, sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import helpers as H; "
                "import onehot; c = pickle.load(open(sys.argv[1], 'rb')); st = H.run_oracle(c, backward=False)[0]; "
                "np.savez(sys.argv[2], **{'n%%d' %% i: onehot.nine_sums(H.O.backward(st, u, c.gD)) "
                "for i, u in enumerate(c.upstreams)})" % (Hh.ROOT, os.path.join(Hh.ROOT, "tests")))
        r = subprocess.run([sys.executable, "-c", code, os.path.join(d, "case.pkl"), os.path.join(d, "g.npz")],
                           env=dict(os.environ, BSR_ORACLE_LIB=lib), capture_output=True, text=True)
        if r.returncode != 0:
            return None
        with np.load(os.path.join(d, "g.npz")) as z:
            return [z["n%d" % i] for i in range(len(c.upstreams))]
