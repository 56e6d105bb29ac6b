"""GPU tests of the scene file (bloomscene_amd/scene_file.py) on a tiny model: ``load_scene(path)`` of what ``save_scene``
wrote gives back, from the path alone, the quantised anchors bit for bit (in key order), the masks, the tables' signs, the MLP
parameters, and the attributes the encoder side's own operands decode to; a render of the loaded scene is bit-identical
to the render of the source tensors pruned, permuted and quantised the same way; the section bytes add up to the file."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

import anchor_codec_reference as R
from bloomscene_amd import anchor_state as AS
from bloomscene_amd import codec, context, heads, synthetic, views
from bloomscene_amd import scene_file as SF
from bloomscene_amd.mix_encoding import MixEncoding

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, F, K, W, H = 300, 8, 4, 64, 64


def tiny_model(seed=0):
    torch.manual_seed(seed)
    s = synthetic.anchor_scene(N, K, W, H, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    mask = (torch.rand(N, K, 1, generator=g) < 0.6).float()
    mask[::9] = 0.0                                                  # every ninth anchor is pruned
    bmin, bmax = R.anchor_bounds(s.anchor.numpy())
    enc = MixEncoding(2, (8, 12, 18), 10, (16, 24), 9)
    D = enc.output_dim
    mlp_grid = nn.Sequential(nn.Linear(D, 32), nn.ReLU(True), nn.Linear(32, context.outputs(F, K)))
    mlps = OrderedDict([("mlp_opacity", nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, K), nn.Tanh())),
                        ("mlp_cov", nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, 7 * K))),
                        ("mlp_color", nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, 3 * K), nn.Sigmoid()))])
    t = lambda x: x.to(DEV)
    return dict(anchor=t(s.anchor), bound_min=t(torch.from_numpy(bmin)), bound_max=t(torch.from_numpy(bmax).reshape(1, 3)),
                anchor_feat=t(torch.randn(N, F, generator=g)), offset=t(s.grid_offsets), scaling=t(s.grid_scaling), mask=t(mask),
                encoding=enc.to(DEV), mlp_grid=mlp_grid.to(DEV), mlps=OrderedDict((k, m.to(DEV)) for k, m in mlps.items()),
                F=F, K=K), s.camera.to(DEV)


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    model, cam = tiny_model()
    path = str(tmp_path_factory.mktemp("scene") / "scene.bsrs")
    info = SF.save_scene(path, **model)
    return model, cam, path, info, SF.load_scene(path, DEV)


def encoder_side(model, info):
    """The source tensors pruned and permuted as the file has them, quantised and coded with the same calls."""
    z = lambda *s: torch.zeros(*s, device=DEV)
    lo, hi = model["bound_min"], model["bound_max"]
    anchor_q = AS.visible(torch.arange(N, device=DEV), model["anchor"], lo, hi, z(N, 1), z(N, 1, 3), z(N, 6), z(N, 1, 1))[0][info.perm]
    weights = context.grid_weights(model["mlp_grid"])
    with torch.no_grad():
        enc = model["encoding"](anchor_q, lo, hi)
        ctx, Q = context.context_head_maps(enc, weights, F, K)[:2]
        feat, scaling, offset = (model[k][info.perm] for k in ("anchor_feat", "scaling", "offset"))
        mask = model["mask"][info.perm]
        q = context.context_quantise_tensors(enc, weights, F, K, feat, scaling, offset, feat.mean(), scaling.mean(), offset.mean(),
                                             steps=True)
        assert torch.equal(q[3].view(torch.int32), Q.view(torch.int32))      # the quantiser's steps are the head's, bit for bit
        streams = codec.encode_attributes(ctx, Q, q[0], q[1], q[2] * mask, mask, F, K)
        decoded = codec.decode_attributes(streams, ctx, Q, mask, F, K)
    return anchor_q, mask, decoded


def bits(t):
    return t.contiguous().view(torch.int32)


def test_load_gives_back_what_the_encoder_coded(saved):
    model, cam, path, info, scene = saved
    anchor_q, mask, (feat, scaling, offset) = encoder_side(model, info)
    keep = model["mask"].reshape(N, K).any(dim=1)
    assert torch.equal(info.keep, keep) and 0 < info.n == int(keep.sum()) < N and scene.n == info.n
    assert torch.equal(torch.sort(info.perm)[0], torch.nonzero(keep).reshape(-1))
    assert (scene.F, scene.K) == (F, K)
    assert torch.equal(bits(scene.anchor), bits(anchor_q))
    assert torch.equal(scene.mask, mask) and scene.mask.shape == (info.n, K, 1)
    assert torch.equal(bits(scene.bound_min), bits(model["bound_min"])) and torch.equal(scene.bound_max, model["bound_max"].reshape(3))
    for name in MixEncoding.NAMES:
        src, got = getattr(model["encoding"], name), getattr(scene.encoding, name)
        assert torch.equal(got.params, torch.where(src.params >= 0, 1.0, -1.0)) and bool((got.params == -1).any())
        assert torch.equal(got.offsets_list, src.offsets_list) and torch.equal(got.resolutions_list, src.resolutions_list)
    for name, src in [("mlp_grid", model["mlp_grid"])] + list(model["mlps"].items()):
        got = scene.mlp_grid if name == "mlp_grid" else scene.mlps[name]
        assert [type(l) for l in got] == [type(l) for l in src]
        for (k, a), (_, b) in zip(got.state_dict().items(), src.state_dict().items()):
            assert torch.equal(bits(a), bits(b)), (name, k)
    assert list(scene.mlps) == list(model["mlps"])
    for name, got, want in (("feat", scene.anchor_feat, feat), ("scaling", scene.scaling, scaling), ("offset", scene.offset, offset)):
        assert got.shape == want.shape and torch.equal(bits(got), bits(want)), name
    # the decoded attributes are the quantised ones: within half a step of the source (Q <= 2 * the base step)
    assert float((scene.anchor_feat - model["anchor_feat"][info.perm]).abs().max()) <= 0.25
    assert float((scene.offset - model["offset"][info.perm] * mask).abs().max()) <= 0.05


def test_render_of_the_loaded_scene_is_the_render_of_the_source_quantised(saved):
    model, cam, path, info, scene = saved
    anchor_q, mask, (feat, scaling, offset) = encoder_side(model, info)
    bg = torch.zeros(3, device=DEV)

    def render(anchor, feat, scaling, offset, mask, mlps):
        with torch.no_grad():
            op, color, sr = heads.anchor_heads(feat, anchor, cam.camera_center, mlps["mlp_opacity"], mlps["mlp_cov"],
                                               mlps["mlp_color"], offset_mask=mask)
            return views.render_neural(cam, anchor, scaling, offset, op, color, sr, bg)

    a = render(scene.anchor, scene.anchor_feat, scene.scaling, scene.offset, scene.mask, scene.mlps)
    b = render(anchor_q, feat, scaling, offset, mask, model["mlps"])
    assert a["render"].shape == (3, H, W) and bool(a["render"].any()) and int(a["radii"].numel()) > 0
    for k in ("render", "depth", "radii", "selection_mask"):
        assert torch.equal(a[k], b[k]), k


def test_section_bytes_add_up_to_the_file(saved):
    model, cam, path, info, scene = saved
    assert info.header_bytes + sum(info.sections.values()) == info.file_bytes == os.path.getsize(path)
    assert list(info.sections) == ["mlps", "table_0", "table_1", "table_2", "table_3", "anchors", "masks", "feat", "scaling",
                                   "offsets"]
    params = sum(p.numel() for m in [model["mlp_grid"]] + list(model["mlps"].values()) for p in m.parameters())
    assert info.sections["mlps"] == 4 * params + (-4 * params % 8)
    with open(path, "rb") as f:
        assert f.read(4) == b"BSRS"


def test_apply_to_replaces_the_models_parameters(saved):
    model, cam, path, info, scene = saved
    from types import SimpleNamespace
    fresh, _ = tiny_model(seed=5)
    pc = SimpleNamespace(encoding_xyz=fresh["encoding"], mlp_grid=fresh["mlp_grid"], decoded_version=False, **fresh["mlps"])
    scene.apply_to(pc)
    assert pc.decoded_version is True and torch.equal(pc._anchor, scene.anchor) and torch.equal(pc._mask, scene.mask)
    assert torch.equal(pc.encoding_xyz.encoding_xy.params, scene.encoding.encoding_xy.params)
    assert torch.equal(pc.mlp_cov[2].weight, model["mlps"]["mlp_cov"][2].weight) and pc.x_bound_min.shape == (1, 3)


def test_probabilities_of_zero_and_one(tmp_path):
    """Every mask entry 1 (p = 1, nothing pruned), a table of +1 alone (p = 1) and one of -1 alone (p = 0): the symbol
    without mass keeps the model's floor of two counts, and everything comes back."""
    model, _ = tiny_model(seed=3)
    model["mask"] = torch.ones_like(model["mask"])
    enc = model["encoding"]
    enc.encoding_xy.params.data = enc.encoding_xy.params.data.abs()
    enc.encoding_xz.params.data = -enc.encoding_xz.params.data.abs() - 1e-6
    path = str(tmp_path / "ones.bsrs")
    info = SF.save_scene(path, **model)
    scene = SF.load_scene(path, DEV)
    assert info.n == N and bool(info.keep.all()) and bool((scene.mask == 1).all()) and scene.mask.shape == (N, K, 1)
    assert bool((scene.encoding.encoding_xy.params == 1).all()) and bool((scene.encoding.encoding_xz.params == -1).all())
    anchor_q, mask, (feat, scaling, offset) = encoder_side(model, info)
    assert torch.equal(bits(scene.anchor), bits(anchor_q)) and torch.equal(bits(scene.anchor_feat), bits(feat))
    assert torch.equal(bits(scene.offset), bits(offset)) and torch.equal(bits(scene.scaling), bits(scaling))
    none = dict(model, mask=torch.zeros_like(model["mask"]))                 # p = 0 and n = 0: every anchor is pruned
    info = SF.save_scene(path, **none)
    scene = SF.load_scene(path, DEV)
    assert info.n == scene.n == 0 and scene.anchor.shape == (0, 3) and scene.mask.shape == (0, K, 1)
    assert scene.anchor_feat.shape == (0, F) and scene.offset.shape == (0, K, 3)


def test_a_corrupt_header_is_a_value_error_before_anything_is_allocated(saved, tmp_path):
    """load_scene allocates nothing from a number of the file that it has not bounded: each of these would otherwise ask for
    gigabytes (an nn.Linear, a table, an output) and end in a MemoryError."""
    import struct
    model, cam, path, info, scene = saved
    data = open(path, "rb").read()
    names = list(info.sections)
    start = lambda name: info.header_bytes + sum(info.sections[k] for k in names[:names.index(name)])
    mlp_grid_at = 4 + 16 + 20 + 4 * (3 + 2) + 4 + 4 + 8           # magic, four words, five words, the lists, count, "mlp_grid"
    assert struct.unpack_from("<3I", data, mlp_grid_at) == (18, 32, context.outputs(F, K))
    big = 0x7fffffff
    # the section count stands before the table of 10 x 20 bytes, which ends at the header's end or 4 bytes before it
    sections_at = next(at for at in (info.header_bytes - 204, info.header_bytes - 208) if struct.unpack_from("<I", data, at) == (10,))
    for what, at, value in (("n", 8, 1 << 27), ("n", 8, big), ("F", 12, big), ("K", 16, big), ("n_features", 20, big),
                            ("log2_hashmap_size", 24, 31), ("levels", 32, big), ("a resolution", 40, big),
                            ("hidden width", mlp_grid_at + 4, big), ("hidden width", mlp_grid_at + 4, 4096),
                            ("layer code", mlp_grid_at + 12, 7), ("sections", sections_at, 11),
                            ("mask count", start("masks") + 4, big), ("table count", start("table_1") + 4, big),
                            ("mask p", start("masks"), 0x7fc00000)):
        bad = bytearray(data)
        struct.pack_into("<I", bad, at, value)
        p = str(tmp_path / "bad.bsrs")
        with open(p, "wb") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            SF.load_scene(p, DEV)


def test_refusals_come_in_the_siblings_order(saved, tmp_path):
    model, cam, path, info, scene = saved
    out = str(tmp_path / "x.bsrs")
    bad = lambda **kw: SF.save_scene(out, **{**model, **kw})
    with pytest.raises(TypeError, match="anchor_feat must be float32"):          # a dtype before the layer, the shape, the device
        bad(anchor_feat=model["anchor_feat"].half().cpu()[:5], mlp_grid=nn.Linear(4, 4))
    with pytest.raises(NotImplementedError, match="mlp_grid must be an nn.Sequential"):
        bad(mlp_grid=nn.Linear(4, 4), offset=model["offset"][:5])
    with pytest.raises(NotImplementedError, match=r"mlp_cov\[1\] is a GELU"):
        bad(mlps=OrderedDict(model["mlps"], mlp_cov=nn.Sequential(nn.Linear(F + 4, F), nn.GELU(), nn.Linear(F, 7 * K))))
    with pytest.raises(NotImplementedError, match="MixEncoding"):
        bad(encoding=model["encoding"].encoding_xyz)
    with pytest.raises(ValueError, match=r"offset must be \[300, 4, 3\]"):       # a shape before the device
        bad(offset=model["offset"][:5].cpu())
    with pytest.raises(ValueError, match="scaling must be on the GPU"):
        bad(scaling=model["scaling"].cpu())
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="device must be a GPU"):
        SF.load_scene(path, "cpu")
    data = open(path, "rb").read()
    for name, blob, what in (("magic", b"XSRS" + data[4:], "not a scene file"), ("cut", data[:len(data) // 2], "truncated"),
                             ("head", data[:30], "truncated")):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(blob)
        with pytest.raises(ValueError, match=what):
            SF.load_scene(p, DEV)
