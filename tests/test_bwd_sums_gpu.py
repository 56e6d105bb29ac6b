"""The backward walks' cross-lane sum networks (csrc/bwd_sums.h), each on its own: hand-scheduled DPP / permlane
sequences whose lane contracts were until now checked only by calibrate_components at run time and by the whole-frame
parity tests.  tests/native/libbsr_pure_functions.so runs each network, nine and ten values, for one wave on the inputs
given here; the inputs are small integers, so every order of addition gives the same float and `==` is the check."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_parity_gpu import _dev

pytestmark = pytest.mark.gpu

WAVE_SUMS_MASKED, ROW8_SUMS, ROW4_SUMS = 0, 1, 2


def _run(network, ten, x):
    """x[v][lane] (10 x 64) -> (out[v][lane], aux[2][lane]) of pt_bwd_sums."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libbsr_pure_functions.so")
    assert os.path.exists(path), f"{path} missing: run __graft_entry__.build()"
    L = C.CDLL(path)
    dev = _dev()
    assert x.shape == (10, 64)
    tin = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    tout = torch.full((10, 64), float("nan"), dtype=torch.float32, device=dev)
    taux = torch.full((2, 64), -1, dtype=torch.int32, device=dev)
    rc = L.pt_bwd_sums(network, int(ten), C.c_void_p(tin.data_ptr()), C.c_void_p(tout.data_ptr()), C.c_void_p(taux.data_ptr()),
                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    return tout.cpu().numpy(), taux.cpu().numpy()


def _inputs(seed):
    """Different data in every lane and register: integers of up to 5 bits (a 64-lane total stays far below 2^24)."""
    return np.random.default_rng(seed).integers(-31, 32, size=(10, 64)).astype(np.float32)


@pytest.mark.parametrize("ten", [False, True])
def test_wave_sums_masked_leaves_every_component_total_in_exactly_one_storing_lane(ten):
    nv = 10 if ten else 9
    x = _inputs(1 + ten)
    out, aux = _run(WAVE_SUMS_MASKED, ten, x)
    comp, stores = aux[0], aux[1].astype(bool)
    total = x.sum(axis=1, dtype=np.float64)
    print("component of lane:", comp.tolist(), "storing lanes:", np.flatnonzero(stores).tolist())
    assert stores.sum() == nv
    for c in range(nv):
        lanes = np.flatnonzero(stores & (comp == c))
        assert len(lanes) == 1, (c, lanes)
        assert out[0][lanes[0]] == total[c], (c, lanes[0], out[0][lanes[0]], total[c])


@pytest.mark.parametrize("ten", [False, True])
def test_row8_sums_lane_contract(ten):
    """Over the 8 lanes sharing lane >> 3: lanes with bit 2 clear hold the totals of inputs 0..3 (0..4) in x0..x3 (x4)
    -- and, of nine values, that of input 8 in x8 --; lanes with bit 2 set hold those of inputs 4..7 (5..9)."""
    half = 5 if ten else 4
    x = _inputs(3 + ten)
    out, _ = _run(ROW8_SUMS, ten, x)
    group_total = x.reshape(10, 8, 8).sum(axis=2, dtype=np.float64)   # [v][group]
    for lane in range(64):
        g, upper = lane >> 3, bool(lane & 4)
        for m in range(half):
            assert out[m][lane] == group_total[(half if upper else 0) + m][g], (lane, m)
        if not ten and not upper:
            assert out[8][lane] == group_total[8][g], lane


@pytest.mark.parametrize("ten", [False, True])
def test_row4_sums_every_lane_holds_its_quads_totals(ten):
    nv = 10 if ten else 9
    x = _inputs(5 + ten)
    out, _ = _run(ROW4_SUMS, ten, x)
    quad_total = x.reshape(10, 16, 4).sum(axis=2, dtype=np.float64)   # [v][quad]
    for lane in range(64):
        for v in range(nv):
            assert out[v][lane] == quad_total[v][lane >> 2], (lane, v)
