"""Time the hash-grid encoder on BloomScene's mix_3D2D_encoding shape (scene/gaussian_model.py:97-104): one 3D call
(12 levels, 2^19 hashmap) + three 2D calls (4 levels, 2^17), F = 2, forward + backward, against a pure-torch restatement
of the same math on the GPU (gather + autograd's index_add_ backward).

    python tools/bench_grid.py [--steps 20] [--warmup 5] [--sizes 100000,1000000]

Prints one JSON line: per (N, distribution) the microseconds of one mix_3D2D forward + backward (four calls) for the
HIP path and the torch baseline, the algorithmic bytes of the HIP path, and the max / median contributions per
touched table row of the 3D table's coarsest level and of the whole 3D table.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.grid_encoder import GridEncoder, grid_encode  # noqa: E402

RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
RES_2D = (130, 258, 514, 1026)
PRIMES = (1, 2654435761, 805459861)


def torch_rows(x, offs, res, l):
    """Per corner: (weight, included, absolute row) of every point at level l -- the header's rule in torch."""
    off, hs, r = int(offs[l]), int(offs[l + 1]) - int(offs[l]), int(res[l])
    N, D = x.shape
    pos = x * float(r - 2) + 0.5
    pg = torch.floor(pos)
    fr = pos - pg
    pg = pg.long()
    stride, d = 1, 0
    while d < D and stride <= hs:
        stride *= r
        d += 1
    hashed = stride > hs
    out = []
    for k in range(1 << D):
        w = torch.ones(N, device=x.device)
        idx = torch.zeros(N, dtype=torch.long, device=x.device)
        ok = torch.ones(N, dtype=torch.bool, device=x.device)
        for d in range(D):
            if (k >> d) & 1:
                w = w * fr[:, d]
                p = torch.clamp(pg[:, d] + 1, max=r - 1)
            else:
                w = w * (1 - fr[:, d])
                p = pg[:, d]
            ok &= (p != 0) & (p != r - 1)
            idx = idx ^ ((p * PRIMES[d]) & 0xFFFFFFFF) if hashed else idx + p * r ** d
        out.append((w, ok, off + idx % hs))
    return out


def torch_encode(x, emb, offs, res):
    """Baseline forward (differentiable in emb through the gather)."""
    inside = ((x >= 0) & (x <= 1)).all(dim=1, keepdim=True)
    outs = []
    for l in range(len(res)):
        corners = torch_rows(x, offs, res, l)
        wn = sum(torch.where(ok, w, torch.zeros_like(w)) for w, ok, _ in corners)
        wn = torch.where(wn == 0, torch.full_like(wn, 1e-9), wn)
        o = sum(torch.where(ok, w / wn, torch.zeros_like(w))[:, None] * emb[row] for w, ok, row in corners)
        outs.append(torch.where(inside, o, torch.zeros_like(o)))
    return torch.cat(outs, dim=1)


def contributions_per_row(x, offs, res, levels, n_rows):
    cnt = torch.zeros(n_rows, dtype=torch.long, device=x.device)
    for l in levels:
        for w, ok, row in torch_rows(x, offs, res, l):
            cnt += torch.bincount(row[ok], minlength=n_rows)
    t = cnt[cnt > 0]
    return int(t.max()), int(t.median())


def make_points(N, dist, gen):
    if dist == "uniform":
        return torch.rand(N, 3, device="cuda", generator=gen)
    centres = torch.rand(8, 3, device="cuda", generator=gen) * 0.6 + 0.2
    which = torch.randint(0, 8, (N,), device="cuda", generator=gen)
    x = centres[which] + 0.02 * torch.randn(N, 3, device="cuda", generator=gen)
    return x.clamp(0, 1)


def mix_inputs(x):
    return [x, x[:, [0, 1]].contiguous(), x[:, [0, 2]].contiguous(), x[:, [1, 2]].contiguous()]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    encs = [GridEncoder(3, 2, RES_3D, 19).cuda()] + [GridEncoder(2, 2, RES_2D, 17).cuda() for _ in range(3)]
    host_offs = [e.offsets_list.tolist() for e in encs]
    host_res = [e.resolutions_list.tolist() for e in encs]
    gen = torch.Generator("cuda").manual_seed(1)
    results = []
    for N in [int(s) for s in a.sizes.split(",")]:
        for dist in ("uniform", "clustered"):
            xs = mix_inputs(make_points(N, dist, gen))
            grads = [torch.randn(N, e.output_dim, device="cuda", generator=gen) for e in encs]

            def hip_step():
                for e, x, g in zip(encs, xs, grads):
                    e.params.grad = None
                    grid_encode(x, e.params, e.offsets_list, e.resolutions_list).backward(g)

            def torch_step():
                for e, x, g, o, r in zip(encs, xs, grads, host_offs, host_res):
                    e.params.grad = None
                    torch_encode(x, e.params, o, r).backward(g)

            us_hip = timed(hip_step, a.steps, a.warmup)
            us_torch = None if a.no_baseline else timed(torch_step, max(2, a.steps // 4), 1)
            nbytes = 0
            for e, x in zip(encs, xs):
                D, L, R = e.num_dim, e.n_levels, int(e.offsets_list[-1])
                fwd = N * D * 4 + L * N * (1 << D) * 2 * 4 + L * N * 2 * 4
                bwd = L * N * 2 * 4 * 2 + L * N * (1 << D) * 2 * 8 + R * 2 * (8 + 8 + 4) + N * D * 4
                nbytes += fwd + bwd
            mx0, med0 = contributions_per_row(xs[0], host_offs[0], host_res[0], [0], host_offs[0][-1])
            mx, med = contributions_per_row(xs[0], host_offs[0], host_res[0], range(12), host_offs[0][-1])
            results.append({"N": N, "dist": dist, "us_hip_fwd_bwd": round(us_hip, 1),
                            "us_torch_fwd_bwd": None if us_torch is None else round(us_torch, 1),
                            "speedup": None if us_torch is None else round(us_torch / us_hip, 2),
                            "algorithmic_bytes": nbytes, "GBps": round(nbytes / us_hip / 1e3, 1),
                            "contrib_per_row_3d_level0_max_median": [mx0, med0],
                            "contrib_per_row_3d_all_max_median": [mx, med]})
    print(json.dumps({"workload": "mix_3D2D_encoding fwd+bwd (1x3D + 3x2D, F=2)", "results": results}))


if __name__ == "__main__":
    main()
