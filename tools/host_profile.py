#!/usr/bin/env python3
"""Host-side cost of one rasterizer step (python + ctypes + torch allocator + autograd), measured where the GPU is
not the limit: the C3 call shape on a SMALL scene (P = 20 000), so that every step's wall time is the host's.
    python3 tools/host_profile.py [--steps 300] [--profile] [--lib other_build.so] [--adam]
Prints ms per step of forward, backward and the whole step; --profile adds a cProfile table (top 35 by cumulative time);
--lib measures another build of the library (tools/build_base.sh).
--adam: the optimizer's step instead (bloomscene_amd.optim.Adam over BloomScene's 29 stepped tensors at --gaussians ANCHORS,
default form; tools/bench_adam.py has the shapes), where the host's walk over the live tensors is the whole cost."""
import argparse, cProfile, math, os, pstats, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bloomscene_amd import GaussianRasterizationSettings, GaussianRasterizer
from bloomscene_amd.synthetic import scene_a, upstream_grads
from bloomscene_amd.views import yawed_camera

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--gaussians", type=int, default=20000)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--lib", default=None)
ap.add_argument("--adam", action="store_true")
a = ap.parse_args()
if a.lib:
    from bloomscene_amd import _capi
    _capi.use_library(a.lib)
dev = torch.device("cuda", 0)
if a.adam:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_adam
    from bloomscene_amd.optim import Adam
    shapes = bench_adam.model_shapes(a.gaussians)
    flat = [s for _, shs, _ in shapes for s in shs]
    values = [torch.randn(s, device=dev) for s in flat]
    opt = bench_adam.make_side(shapes, values, [v * 1e-2 for v in values], Adam)[1]
    for _ in range(20):
        opt.step()
    torch.cuda.synchronize()
    pr = cProfile.Profile() if a.profile else None
    t0 = time.perf_counter()
    if pr:
        pr.enable()
    for _ in range(a.steps):
        opt.step()
    if pr:
        pr.disable()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    print(f"host time of an optimizer step ({a.gaussians} anchors, {sum(len(g['params']) for g in opt.param_groups)} tensors): "
          f"{dt / a.steps * 1e3:.4f} ms  ({os.cpu_count()} host threads)")
    if pr:
        pstats.Stats(pr).sort_stats("cumulative").print_stats(25)
    sys.exit(0)
W, H, deg = 1920, 1080, 3
sc = scene_a(a.gaussians, W, H, deg, seed=0)
leaves = {k: getattr(sc, k).to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
gC, gD = [t.to(dev) for t in upstream_grads(W, H, seed=1)]
cam = yawed_camera(W, H, math.radians(60.0), yaw_deg=0.0).to(dev)
st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                   bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                                   projmatrix=cam.full_proj_transform, sh_degree=deg, campos=cam.camera_center, prefiltered=False, debug=False)
rast = GaussianRasterizer(st)
t_f = t_b = 0.0

def step():
    global t_f, t_b
    t0 = time.perf_counter()
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, radii, depth = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                               scales=leaves["scales"], rotations=leaves["rotations"])
    t1 = time.perf_counter()
    for v in leaves.values():
        v.grad = None
    torch.autograd.backward((color, depth), (gC, gD))
    t2 = time.perf_counter()
    t_f += t1 - t0
    t_b += t2 - t1

for _ in range(20):
    step()
torch.cuda.synchronize()
t_f = t_b = 0.0
pr = cProfile.Profile() if a.profile else None
t0 = time.perf_counter()
if pr:
    pr.enable()
for _ in range(a.steps):
    step()
if pr:
    pr.disable()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"host-bound step (P={a.gaussians}): {dt / a.steps * 1e3:.4f} ms  forward call {t_f / a.steps * 1e3:.4f} ms  "
      f"backward call {t_b / a.steps * 1e3:.4f} ms  ({os.cpu_count()} host threads)")
if pr:
    pstats.Stats(pr).sort_stats("cumulative").print_stats(35)
