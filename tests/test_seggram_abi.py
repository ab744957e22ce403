# coding=utf-8
"""include/tfgx_seggram.h (the segmented transposed product S_g^T Y_g of DiffPool / MinCutPool and its backward) without a GPU:
the exact list of its names and its own macros (the uniform header / table / version checks are tests/test_abi_registry.py's),
the host argument checks name the refused member before any device work, and zero sizes succeed."""
import pytest

from abi_header import declarations, macro, refused as _refused

HEADER = "tfgx_seggram.h"


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


def test_symbols_versions_and_signatures():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.SEGGRAM_SIGNATURES) == [
        "tfgx_seggram_block", "tfgx_seggram_version", "tfgx_segment_gram_backward_f32", "tfgx_segment_gram_f32",
        "tfgx_segment_gram_workspace_bytes"]
    assert L.SEGGRAM_MAX_K == macro(HEADER, "TFGX_SEGGRAM_MAX_K") == 64


FWD_OK = dict(seg_ptr=8, seg_node=None, G=3, N=200, S=8, lds=5, K=5, Y=8, ldy=20, W=20, out=8, ldo=20, flag=None, ws=8,
              ws_bytes=1 << 30, stream=None)
BWD_OK = dict(node_seg=8, N=200, G=3, S=8, lds=5, K=5, Y=8, ldy=20, W=20, dOut=8, ldo=20, dS=8, ldds=5, dY=8, lddy=20,
              flag=None, stream=None)


@pytest.mark.parametrize("change, word", [
    (dict(K=0), "TFGX_SEGGRAM_MAX_K"), (dict(K=65, lds=65), "TFGX_SEGGRAM_MAX_K"),
    (dict(N=-1), "negative"), (dict(G=-1), "negative"), (dict(W=-1), "negative"), (dict(N=1 << 31), "fit int32"),
    (dict(G=1 << 30), "fit int32"), (dict(W=(1 << 20) + 1, ldy=1 << 21, ldo=1 << 21), "2^20"),
    (dict(lds=4), "lds"), (dict(ldy=19), "ldy"), (dict(ldo=19), "ldo"),
    (dict(seg_ptr=None), "seg_ptr is null"), (dict(S=None), "S is null"), (dict(Y=None), "Y is null"),
    (dict(out=None), "out is null"), (dict(ws=None), "workspace is null"),
])
def test_forward_argument_checks_name_the_member(change, word):
    _refused("tfgx_segment_gram_f32", FWD_OK, change, word)


@pytest.mark.parametrize("change, word", [
    (dict(K=0), "TFGX_SEGGRAM_MAX_K"), (dict(K=65, lds=65, ldds=65), "TFGX_SEGGRAM_MAX_K"),
    (dict(N=-1), "negative"), (dict(G=-1), "negative"), (dict(W=-1), "negative"), (dict(N=1 << 31), "fit int32"),
    (dict(lds=4), "lds"), (dict(ldy=19), "ldy"), (dict(ldo=19), "ldo"), (dict(ldds=4), "ldds"), (dict(lddy=19), "lddy"),
    (dict(node_seg=None), "node_seg is null"), (dict(S=None), "S is null"), (dict(Y=None), "Y is null"),
    (dict(dOut=None), "dOut is null"),
])
def test_backward_argument_checks_name_the_member(change, word):
    _refused("tfgx_segment_gram_backward_f32", BWD_OK, change, word)


def test_workspace_too_small_is_its_own_code_and_the_size_query():
    lib = _lib()
    B = lib.tfgx_seggram_block()
    need = lib.tfgx_segment_gram_workspace_bytes(200, 3, 5, 20)
    assert need == ((200 + B - 1) // B) * 2 * 5 * 20 * 4          # two partial tiles per position block
    _refused("tfgx_segment_gram_f32", FWD_OK, dict(ws_bytes=need - 1), "workspace_bytes", code=3)
    assert lib.tfgx_segment_gram_workspace_bytes(B, 3, 5, 20) == 0          # one block: no segment crosses a boundary
    for bad in ((-1, 3, 5, 20), (200, 3, 0, 20), (200, 3, 65, 20), (1 << 31, 3, 5, 20)):
        assert lib.tfgx_segment_gram_workspace_bytes(*bad) == 0
    assert lib.tfgx_segment_gram_workspace_bytes(200, 0, 5, 20) == 0 and lib.tfgx_segment_gram_workspace_bytes(200, 3, 5, 0) == 0


def test_zero_sizes_succeed_without_device_work():
    lib = _lib()
    null = dict(seg_ptr=None, S=None, Y=None, out=None, ws=None, ws_bytes=0)
    assert lib.tfgx_segment_gram_f32(*dict(FWD_OK, **dict(null, N=0, G=0)).values()) == 0
    assert lib.tfgx_segment_gram_f32(*dict(FWD_OK, **dict(null, G=0)).values()) == 0
    assert lib.tfgx_segment_gram_f32(*dict(FWD_OK, **dict(null, N=0, W=0, ldy=0, ldo=0)).values()) == 0
    bnull = dict(node_seg=None, S=None, Y=None, dOut=None, dS=None, dY=None)
    assert lib.tfgx_segment_gram_backward_f32(*dict(BWD_OK, **dict(bnull, N=0)).values()) == 0
    assert lib.tfgx_segment_gram_backward_f32(*dict(BWD_OK, **dict(bnull, N=0, G=0)).values()) == 0
    assert lib.tfgx_segment_gram_backward_f32(*dict(BWD_OK, dS=None, dY=None).values()) == 0      # nothing is wanted


def test_public_names_and_constructors_fail_loudly_without_a_gpu():
    """The layers and functions import everywhere; without a GPU they raise TfgxError, as the other layers do."""
    import numpy as np
    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd._lib import TfgxError
    for name in ("diff_pool", "diff_pool_coarsen", "min_cut_pool", "min_cut_pool_coarsen", "min_cut_pool_compute_losses"):
        assert getattr(tfg.nn, name) is getattr(tfg.nn.pool, name) and callable(getattr(tfg.nn, name))
    assert tfg.layers.DiffPool is tfg.layers.pool.DiffPool and tfg.layers.MinCutPool is tfg.layers.pool.MinCutPool
    from tf_geometric_amd import autograd
    assert callable(autograd.segment_gram)
    from tf_geometric_amd.nn.pool.set2set import _graph_plan, CACHE_KEY_GRAPH_PLAN      # where the Set2Set tools import it from
    from tf_geometric_amd.nn.pool.common_pool import _graph_plan as shared
    assert _graph_plan is shared and CACHE_KEY_GRAPH_PLAN == "tfgx_set2set_graph_plan"
    with pytest.raises(Exception, match="\"units\" parameter is required"):
        tfg.layers.DiffPool(None, None, None, 3)
    with pytest.raises(ValueError, match="cannot be set to True at the same time"):
        tfg.nn.min_cut_pool(None, None, None, None, None, None, 3, return_loss_func=True, return_losses=True)
    if torch.cuda.is_available():
        return
    x, ei, gid = np.zeros((3, 2), np.float32), np.zeros((2, 0), np.int32), np.zeros(3, np.int32)
    with pytest.raises(TfgxError):
        tfg.layers.MinCutPool(None, None, 4, 3)
    with pytest.raises(TfgxError):
        tfg.nn.diff_pool_coarsen(x, ei, None, gid, np.ones((3, 2), np.float32))
    with pytest.raises(TfgxError):
        tfg.nn.min_cut_pool_compute_losses(ei, None, gid, np.ones((3, 2), np.float32))
