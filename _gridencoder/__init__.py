"""Import shim: BloomScene's ``utils/encodings.py:10`` does ``import _gridencoder as _backend`` (the CUDA extension of
``submodules/gridencoder``).  With this repository on ``sys.path`` that import resolves here, to the MI355X-native
encoder of ``bloomscene_amd.grid_encoder`` (C ABI ``include/bloomscene_grid.h``), so BloomScene's own
``_grid_encode`` autograd function runs unmodified.

Only the two functions BloomScene calls are implemented, with the extension's positional argument lists
(``gridencoder.cu:939-1000``).  They write into the tensors they are handed and accept sliced ``offsets_list`` /
``resolutions_list`` views (BloomScene's int ``min_level_id``).  ``grid_encode_backward`` OVERWRITES
``grad_embeddings`` where the extension adds into it; BloomScene hands it zeros (``encodings.py:301``), so the result is
the same.  ``binary_vxl`` and a tensor ``min_level_id`` raise NotImplementedError; the six other functions of the
extension exist and raise NotImplementedError.
"""
from bloomscene_amd import grid_encoder as _ge


def _n_levels_checked(who, offsets_list, resolutions_list, n_levels):
    if offsets_list.shape[0] < n_levels + 1 or resolutions_list.shape[0] < n_levels:
        raise ValueError(f"{who}: {n_levels} levels need {n_levels + 1} offsets and {n_levels} resolutions "
                         f"(got {offsets_list.shape[0]} and {resolutions_list.shape[0]})")


def grid_encode_forward(inputs, embeddings, offsets_list, resolutions_list, outputs, N, num_dim, n_features, n_levels,
                        max_level, Rb, PV, dy_dx, binary_vxl, min_level_id):
    """outputs [n_levels, N, F] (and dy_dx [N, n_levels * D * F] if given) of levels offsets_list[0 .. n_levels].
    max_level, Rb and PV are unused, as in the extension."""
    who = "_gridencoder.grid_encode_forward"
    _ge.check_call(who, num_dim, n_features,
                   float_tensors=(("inputs", inputs), ("embeddings", embeddings), ("outputs", outputs),
                                  ("dy_dx", dy_dx)),
                   int_tensors=(("offsets_list", offsets_list), ("resolutions_list", resolutions_list)),
                   binary_vxl=binary_vxl, min_level_id=min_level_id)
    if tuple(inputs.shape) != (N, num_dim) or embeddings.shape[1] != n_features or outputs.numel() != n_levels * N * n_features:
        raise ValueError(f"{who}: tensor shapes disagree with N={N}, num_dim={num_dim}, n_features={n_features}, "
                         f"n_levels={n_levels}")
    if dy_dx is not None and dy_dx.numel() != N * n_levels * num_dim * n_features:
        raise ValueError(f"{who}: dy_dx must hold N * n_levels * num_dim * n_features values")
    _n_levels_checked(who, offsets_list, resolutions_list, n_levels)
    _ge.forward_into(inputs, embeddings, offsets_list, resolutions_list, outputs, dy_dx, n_levels)


def grid_encode_backward(grad, inputs, embeddings, offsets_list, resolutions_list, grad_embeddings, N, num_dim,
                         n_features, n_levels, max_level, Rb, dy_dx, grad_inputs, binary_vxl, min_level_id):
    """grad_embeddings (fully overwritten) and, if dy_dx and grad_inputs are given, grad_inputs [N, D], from
    grad [n_levels, N, F].  embeddings, max_level and Rb are unused, as in the extension."""
    who = "_gridencoder.grid_encode_backward"
    _ge.check_call(who, num_dim, n_features,
                   float_tensors=(("grad", grad), ("inputs", inputs), ("embeddings", embeddings),
                                  ("grad_embeddings", grad_embeddings), ("dy_dx", dy_dx), ("grad_inputs", grad_inputs)),
                   int_tensors=(("offsets_list", offsets_list), ("resolutions_list", resolutions_list)),
                   binary_vxl=binary_vxl, min_level_id=min_level_id)
    if tuple(inputs.shape) != (N, num_dim) or grad_embeddings.shape[1] != n_features or grad.numel() != n_levels * N * n_features:
        raise ValueError(f"{who}: tensor shapes disagree with N={N}, num_dim={num_dim}, n_features={n_features}, "
                         f"n_levels={n_levels}")
    _n_levels_checked(who, offsets_list, resolutions_list, n_levels)
    if dy_dx is None:
        grad_inputs = None   # (the extension computes grad_inputs only with dy_dx, gridencoder.cu:917)
    _ge.backward_into(grad, inputs, offsets_list, resolutions_list, grad_embeddings, dy_dx, grad_inputs, n_levels)


def _unsupported(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"_gridencoder.{name} is not implemented on this backend (BloomScene does not call it)")
    fn.__name__ = name
    return fn


grid_encode_mix2D_forward = _unsupported("grid_encode_mix2D_forward")
grid_encode_mix2D_backward = _unsupported("grid_encode_mix2D_backward")
avg_2D_forward = _unsupported("avg_2D_forward")
avg_2D_backward = _unsupported("avg_2D_backward")
cnt_np_embed = _unsupported("cnt_np_embed")
cnt_np_embed_backward = _unsupported("cnt_np_embed_backward")
