"""mean_dist3 / simple_knn on the GPU (include/bloomscene_knn.h): every output bit-equal to the restatement
(tests/knn_reference.py) on awkward inputs and on 10^6-point clouds, invariance under permutation, strides, streams and a
graph replay, BloomScene's call pattern through the shim, the early exit on identical points, and no device memory
outside torch's pool."""
import time

import numpy as np
import pytest
import torch

import knn_reference as KR

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
KINDS = ["uniform", "planar", "collinear", "identical", "duplicates", "clusters", "offset", "nonfinite"]


def _mean_dist3(x):
    from bloomscene_amd.knn import mean_dist3
    return mean_dist3(x)


def _bits_equal(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 7, 64, 1000, 20000])
@pytest.mark.parametrize("kind", KINDS)
def test_bit_equal_to_restatement(kind, P):
    x = KR.make_cloud(kind, P, seed=P + len(kind))
    xt = torch.from_numpy(x).to(DEV)
    got = _mean_dist3(xt)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (P,)
    ref = KR.mean_dist3_torch(xt, chunk=1024)
    assert _bits_equal(got, ref), (kind, P)
    if P <= 1000:
        assert _bits_equal(got, KR.mean_dist3_numpy(x)), (kind, P)


@pytest.mark.parametrize("kind", ["uniform", "surface"])
def test_bit_equal_at_1m(kind):
    P = 1_000_000
    x = KR.make_cloud(kind, P, seed=1)
    xt = torch.from_numpy(x).to(DEV)
    got = _mean_dist3(xt)
    ref = KR.mean_dist3_torch(xt, chunk=1024)
    torch.cuda.synchronize()
    g, r = got.cpu().numpy(), ref.cpu().numpy()
    bad = np.flatnonzero(g.view(np.uint32) != r.view(np.uint32))
    assert bad.size == 0, (kind, bad.size, bad[:5], g[bad[:5]], r[bad[:5]])
    if kind == "surface":
        assert np.unique(x, axis=0).shape[0] < 0.96 * P   # the exact duplicates are there


def test_bit_equal_at_257_sort_tiles():
    """One point more than 256 sort tiles of 4096: the row scan of the sort's histogram (256 columns a step) takes a
    second step, which is a single column and needs the carry of the first."""
    P = 256 * 4096 + 1
    xt = torch.from_numpy(KR.make_cloud("uniform", P, seed=1)).to(DEV)
    got = _mean_dist3(xt)
    ref = KR.mean_dist3_torch(xt, chunk=1024)
    torch.cuda.synchronize()
    g, r = got.cpu().numpy(), ref.cpu().numpy()
    bad = np.flatnonzero(g.view(np.uint32) != r.view(np.uint32))
    assert bad.size == 0, (bad.size, bad[:5], g[bad[:5]], r[bad[:5]])


def test_permutation_strides_and_streams():
    P = 50_000
    x = torch.from_numpy(KR.make_cloud("surface", P, seed=4)).to(DEV)
    base = _mean_dist3(x)
    perm = torch.randperm(P, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    assert torch.equal(_mean_dist3(x[perm]), base[perm])
    wide = torch.cat([x, torch.full((P, 1), 7.0, device=DEV)], 1)
    view = wide[:, :3]
    assert not view.is_contiguous()
    assert torch.equal(_mean_dist3(view), base)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        on_s = _mean_dist3(x)
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert torch.equal(on_s, base)
    # and again: nothing is kept between calls
    assert torch.equal(_mean_dist3(x), base)


def test_graph_capture_and_replay():
    P = 30_000
    x = torch.from_numpy(KR.make_cloud("clusters", P, seed=8)).to(DEV)
    eager = _mean_dist3(x)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        _mean_dist3(x)   # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _mean_dist3(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(torch.from_numpy(KR.make_cloud("uniform", P, seed=9)).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _mean_dist3(x))


def test_shim_on_bloomscene_call_pattern():
    """scene/gaussian_model.py:464-465: dist2 = clamp_min(distCUDA2(pts).float().cuda(), 1e-7); log(sqrt(dist2))."""
    from simple_knn._C import distCUDA2
    P = 100_000
    x = KR.make_cloud("surface", P, seed=2)
    pts = torch.from_numpy(x).float().cuda()
    dist2 = torch.clamp_min(distCUDA2(pts).float().cuda(), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 6)
    assert tuple(scales.shape) == (P, 6) and torch.isfinite(scales).all()
    ref = torch.clamp_min(KR.mean_dist3_torch(pts, chunk=1024), 0.0000001)
    assert torch.equal(dist2, ref)
    med = torch.kthvalue(dist2.cpu(), P // 2).values
    ref_med = np.partition(ref.cpu().numpy(), P // 2 - 1)[P // 2 - 1]
    assert float(med) == float(ref_med) and float(med) > 0


def test_zero_points_and_bad_shape():
    out = _mean_dist3(torch.empty(0, 3, device=DEV))
    assert tuple(out.shape) == (0,) and out.device.type == "cuda"
    with pytest.raises(ValueError):
        _mean_dist3(torch.zeros(5, 2, device=DEV))
    with pytest.raises(TypeError):
        _mean_dist3(torch.zeros(5, 3, device=DEV, dtype=torch.float16))


def test_identical_points_exit_early():
    P = 1_000_000
    x = torch.full((P, 3), 0.5, device=DEV)
    _mean_dist3(x[:1000])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _mean_dist3(x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert (out == 0).all()
    assert dt < 2.0, dt


def test_no_device_memory_outside_torch_at_1m():
    from bloomscene_amd import _capi
    P = 1_000_000
    x = torch.rand(P, 3, device=DEV)
    _mean_dist3(x[:1000])    # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, total = torch.cuda.mem_get_info()
    outside0 = total - free0 - torch.cuda.memory_reserved()
    alloc0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = _mean_dist3(x)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    outside1 = total - free1 - torch.cuda.memory_reserved()
    assert outside1 - outside0 < (8 << 20), (outside0, outside1)
    # the scratch is on torch's books
    assert torch.cuda.max_memory_allocated() - alloc0 >= _capi.lib().bsr_knn_scratch_bytes(P)
    assert torch.isfinite(out).all() and (out > 0).all()
