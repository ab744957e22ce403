# coding=utf-8
"""Host-side contract of the induced-subgraph / gather-scale entry points (no GPU needed): argument checks return
TFGX_ERR_INVALID_ARG before any device work, workspace queries grow with the plan."""
import ctypes


def test_subgraph_entry_points_check_arguments():
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    kept = ctypes.c_int64(0)
    assert lib.tfgx_induced_subgraph_workspace_bytes(-1, 10, 5, 0) == 0
    small = lib.tfgx_induced_subgraph_workspace_bytes(1000, 100000, 500, 0)
    assert small > 4 * (100000 // 2048) and lib.tfgx_induced_subgraph_workspace_bytes(1000, 100000, 500, 1) > small + 4 * 100000
    assert lib.tfgx_induced_subgraph_count(None, None, -1, 3, None, 0, None, ctypes.byref(kept), None, 0, None) == 1
    assert lib.tfgx_induced_subgraph_count(None, None, 0, 3, None, 0, None, None, None, 0, None) == 1
    assert b"n_kept" in lib.tfgx_last_error()
    assert lib.tfgx_induced_subgraph_emit(None, None, 10, 3, None, 0, None, 11, None, None, None, None, None, None, None,
                                          None, None, None, 0, None) == 1
    assert b"n_kept" in lib.tfgx_last_error()
    assert lib.tfgx_gather_i32(None, None, -2, None, None) == 1
    assert lib.tfgx_gather_scale_rows_f32(None, 4, None, None, 3, 8, None, 8, None) == 1    # ldx < F
    assert lib.tfgx_gather_scale_rows_backward_f32(None, 8, None, 3, None, 8, None, 8, None, 8, ctypes.c_void_p(16),
                                                   None) == 1                              # ds without x
    assert b"ds needs x" in lib.tfgx_last_error()


def test_pool_api_is_exported():
    import tf_geometric_amd as tfg
    for f in (tfg.nn.sag_pool, tfg.nn.sort_pool, tfg.utils.sample_new_graph_by_node_index,
              tfg.utils.compute_edge_mask_by_node_index):
        assert callable(f)
    layer = tfg.layers.SortPool(k=3)
    assert layer.k == 3 and layer.sort_index == -1
