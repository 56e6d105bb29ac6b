"""csrc/grid_sum.h on its own: grid_sum<N, 256> for the three N the losses instantiate (1: the entropy backward, 2: the
photometric, entropy and depth-prior sums, 5: the depth prior's BSR_DEPTH_NSUM) and grid_last_ticket, run by
tests/native/libbsr_shared_pieces.so.  The N totals must equal grid_sum_reference.grid_sum -- the header's four steps in
numpy float64 -- BIT FOR BIT on inputs that show a wrong order in every sum (tests/test_grid_sum_cpu.py checks that they
do, without a GPU), exactly one thread of the grid is told it holds the totals, and a second launch on a re-zeroed
ticket gives the same bits.

Grids: 1 and 2 (no partial stride to speak of), 255, 256, 257 (a full round of partials less one, exact, plus one: the
second partial of thread 0), 513, 1536 (six partials on every thread) and 16384 (64 on every thread)."""
import numpy as np
import pytest
import torch

import grid_sum_reference as GR
import shared_pieces as SP
from test_grid_sum_cpu import GRIDS, NS

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _launch(N, G, x):
    ticket = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=SP.DEV)       # (the entry point zeroes it)
    psum = torch.full((N * G,), float("nan"), dtype=torch.float64, device=SP.DEV)
    out = torch.full((N,), float("nan"), dtype=torch.float64, device=SP.DEV)
    winners = torch.zeros(1, dtype=torch.int32, device=SP.DEV)
    rc = SP.lib().pt_grid_sum(N, G, SP.ptr(x), SP.ptr(ticket), SP.ptr(psum), SP.ptr(out), SP.ptr(winners), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert int(ticket.item()) == G
    return out.cpu().numpy(), int(winners.item()), psum.cpu().numpy().reshape(G, N)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("G", GRIDS)
def test_totals_bit_equal_to_the_headers_order(G, N):
    host = GR.cancelling_grid(G, N)
    partials = GR.workgroup_partials(host)
    want = GR.last_workgroup(partials)
    x = torch.from_numpy(host).to(SP.DEV)
    got, winners, psum = _launch(N, G, x)
    print(f"[grid sum] G={G} N={N} totals {got.tolist()} want {want.tolist()}")
    assert winners == 1, "exactly one thread of the grid holds the totals"
    assert (_bits(psum) == _bits(partials)).all(), "the workgroups' partials (steps 1 to 3)"
    assert (_bits(got) == _bits(want)).all()
    again, winners, _ = _launch(N, G, x)
    assert winners == 1 and (_bits(again) == _bits(got)).all(), "a second launch on a re-zeroed ticket"


@pytest.mark.parametrize("G", GRIDS)
def test_two_tickets_in_a_row_each_pick_one_last_workgroup(G):
    tickets = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device=SP.DEV)      # (the entry point zeroes them)
    words = torch.full((2, G), -1, dtype=torch.int32, device=SP.DEV)
    out = torch.tensor([0, -1, 0, 0, -1, 0], dtype=torch.int32, device=SP.DEV)
    rc = SP.lib().pt_grid_tickets(G, SP.ptr(tickets), SP.ptr(words), SP.ptr(out), SP.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert tickets.tolist() == [G, G]
    assert (words.cpu().numpy() == np.arange(1, G + 1)[None, :]).all()
    out = out.cpu().numpy().reshape(2, 3)
    for c in range(2):
        total, index, count = (int(v) for v in out[c])
        assert count == 1, (c, "workgroups that were told they are the last", count)
        assert 0 <= index < G
        assert total == G * (G + 1) // 2, (c, "a word of another workgroup was not visible to the last one")
