#!/usr/bin/env python3
"""Records what the reference's OWN kernels compute (the strict builds of oracle/_ref, see oracle/reference_build.py) for
a handful of small cases, as tests/golden/reference/reference_knn.npz and reference_grid_d{1,2,3}.npz (a directory of their own: tests/golden/*.npz
are the rasterizer's vectors, which other tests enumerate).

Runs on a machine with an MI355X, after build() has produced oracle/_ref there or the binaries were carried over; reads
only oracle/_ref/ (through tests/reference_builds.py), never the reference tree.  The inputs are not stored: the CPU test
(tests/test_reference_goldens_cpu.py) regenerates them from the seeds of tests/reference_cases.py.

    python tests/golden/make_reference_goldens.py [--out DIR]        (default: tests/golden/reference)

knn:  out_{kind}_{P}  [P] fp32                         every kind, P <= 1000
grid: outputs_f{F} [L, N, F], dy_dx_f{F} [N, L, D, F], grad_inputs_f{F} [N, D]      every (D, F), N = 400, edge points in
(grad_embeddings is not recorded: the reference sums it with fp32 atomics, its bits are not a function of the input.)
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reference_builds as RB  # noqa: E402
import reference_cases as RC  # noqa: E402

DEV = "cuda:0"


def knn_records():
    out = {}
    for kind in RC.KNN_KINDS:
        for P in RC.KNN_GOLDEN_SIZES:
            xt = torch.from_numpy(RC.knn_cloud(kind, P)).to(DEV)
            out[f"out_{kind}_{P}"] = RB.ref_mean_dist3(xt, "strict").cpu().numpy()
    return out


def grid_records(D):
    out = {}
    for F in RC.GRID_FEATURES:
        offs, r, emb, x, g = RC.golden_grid_case(D, F)
        N, L = x.shape[0], len(r)
        xt, et, gt = (torch.from_numpy(a).to(DEV) for a in (x, emb, g))
        ot = torch.tensor(offs, dtype=torch.int32, device=DEV)
        rt = torch.tensor(r, dtype=torch.int32, device=DEV)
        outputs = torch.zeros(L, N, F, device=DEV)
        dy_dx = torch.zeros(N, L * D * F, device=DEV)
        RB.ref_grid_forward(xt, et, ot, rt, outputs, N, D, F, L, 0, 128, 0.0, dy_dx, None, None, build="strict")
        ge = torch.zeros_like(et)
        gi = torch.zeros(N, D, device=DEV)
        RB.ref_grid_backward(gt, xt, et, ot, rt, ge, N, D, F, L, 0, 128, dy_dx, gi, None, None, build="strict")
        out[f"outputs_f{F}"] = outputs.cpu().numpy()
        out[f"dy_dx_f{F}"] = dy_dx.view(N, L, D, F).cpu().numpy()
        out[f"grad_inputs_f{F}"] = gi.cpu().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "reference"))
    args = ap.parse_args()
    if RB.reference_missing():
        sys.exit("oracle/_ref/MANIFEST.json says reference_missing: nothing to record")
    os.makedirs(args.out, exist_ok=True)
    files = {"reference_knn.npz": knn_records()}
    for D in RC.GRID_DIMS:
        files[f"reference_grid_d{D}.npz"] = grid_records(D)
    for name, arrays in files.items():
        path = os.path.join(args.out, name)
        np.savez_compressed(path, **arrays)
        print(f"{name}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
