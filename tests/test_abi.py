# coding=utf-8
"""The C-ABI library loads (no GPU needed) and exports every symbol include/tfgx.h declares; the ctypes structs
match the header's structs; host-side argument checks fire; the product path refuses to run without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_header
from conftest import ROOT


def test_library_exports_every_declared_symbol():
    """tfgx.h, by name (tests/test_abi_registry.py holds every header to its table type by type)."""
    from tf_geometric_amd import _lib
    assert set(abi_header.declarations("tfgx.h")) == set(_lib.SIGNATURES) <= abi_header.exported_symbols()


def test_structs_match_header_layout(tmp_path):
    """sizeof / offsetof of the two launch structs through gcc against the ctypes mirrors."""
    from tf_geometric_amd import _lib
    for c_struct in ("tfgx_reduce_args", "tfgx_gat_args"):
        abi_header.struct_layout("tfgx.h", c_struct, _lib.STRUCTS[c_struct], tmp_path)


def test_argument_validation_without_gpu():
    """Host-side checks return TFGX_ERR_INVALID_ARG before anything touches a device."""
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    assert lib.tfgx_segment_reduce_f32(None, None) == 1
    assert b"args is null" in lib.tfgx_last_error()
    a = _lib.ReduceArgs()
    a.n_dst, a.F, a.op = 4, 0, 0
    assert lib.tfgx_segment_reduce_f32(ctypes.byref(a), None) == 1
    a.F, a.op = 8, 7
    assert lib.tfgx_segment_reduce_f32(ctypes.byref(a), None) == 1 and b"bad op" in lib.tfgx_last_error()
    assert lib.tfgx_gemm_bias_act_f32(None, 4, None, 4, None, 0, None, 4, 2, 0, 4, None) == 1
    assert lib.tfgx_gcn_norm_edges_f32(None, None, None, 3, None, None, 9, 1.0, 1, 1, None, None, None) == 1
    assert lib.tfgx_csr_plan_workspace_bytes(10, 100) > 800
    assert lib.tfgx_build_csr_by_dst(None, None, -1, 3, 3, None, None, None, None, 0, None) == 1
    # entry points added later in the round: same contract (argument errors are reported before any device work)
    assert lib.tfgx_segment_topk(None, None, -1, 3, 1, 0.0, None, None, None, 0, None) == 1
    assert lib.tfgx_segment_topk(None, None, 5, 3, -1, -0.5, None, None, None, 0, None) == 1
    assert lib.tfgx_segment_topk(None, None, 5, 3, 1, 0.0, None, None, None, 0, None) == 1 and b"out_count" in lib.tfgx_last_error()
    assert lib.tfgx_segment_topk_workspace_bytes(1000, 10) > 1000 * 24 and lib.tfgx_segment_topk_workspace_bytes(-1, 1) == 0
    assert lib.tfgx_gemm_workspace_bytes(2708, 1433, 256) >= 2 * 4 * 2708 * 256      # small M, long K: split-K
    assert 0 < lib.tfgx_gemm_workspace_bytes(2400000, 100, 256) <= 4096               # plenty of tiles: no split, only the row kernel's tile counters
    assert lib.tfgx_gemm_workspace_bytes(170000, 128, 256) == 0                       # short launches keep the fixed tile map
    assert lib.tfgx_gemm_bias_act_cols_ws_f32(None, 4, None, 4, None, 0, 9, None, 4, 2, 4, 4, None, 0, None) == 1
    assert b"act_cols" in lib.tfgx_last_error()
    # tfgx_gemm_describe: host only, same argument checks as the launch, never writes past buf_bytes
    al = 1 << 20
    args = (al, 128, 2 * al, 256, None, 0, 0, 3 * al, 256, 1 << 18, 128, 256)
    big = ctypes.create_string_buffer(b"\xff" * 200, 200)
    assert lib.tfgx_gemm_describe(*args, None, 0, big, 200) == 0 and big.value == b"gemm_rows_kernel<8,bv4> fixed"
    assert lib.tfgx_gemm_describe(*args, 4 * al, 4096, big, 200) == 0 and big.value == b"gemm_rows_kernel<8,bv4> claimed"
    small = ctypes.create_string_buffer(b"\xff" * 16, 16)
    assert lib.tfgx_gemm_describe(*args, None, 0, small, 8) == 1 and b"buffer too small" in lib.tfgx_last_error()
    assert small.raw[0:1] == b"\x00" and small.raw[8:] == b"\xff" * 8             # empty string, nothing past buf_bytes
    assert lib.tfgx_gemm_describe(*args, None, 0, None, 200) == 1 and lib.tfgx_gemm_describe(*args, None, 0, big, 0) == 1
    assert lib.tfgx_gemm_describe(None, 128, 2 * al, 256, None, 0, 0, 3 * al, 256, 4, 128, 256, None, 0, big, 200) == 1
    assert b"null pointer" in lib.tfgx_last_error()
    assert lib.tfgx_gemm_describe(al, 128, 2 * al, 256, None, 0, 257, 3 * al, 256, 4, 128, 256, None, 0, big, 200) == 1
    assert b"act_cols" in lib.tfgx_last_error()
    assert lib.tfgx_gemm_describe(al, 127, 2 * al, 256, None, 0, 0, 3 * al, 256, 4, 128, 256, None, 0, big, 200) == 1
    assert b"leading dimension" in lib.tfgx_last_error()
    assert lib.tfgx_gemm_describe(None, 0, None, 0, None, 0, 0, None, 0, 0, 1, 1, None, 0, big, 200) == 0 and b"M = 0" in big.value
    assert lib.tfgx_segment_max_with_count_f32(None, None, None, 4, None, 2, 8, None, 8, None, 8, None) == 1
    assert lib.tfgx_segment_max_backward_w_f32(None, None, None, 4, None, 8, 8, None, 8, None, 4, None, None) == 1
    # phases outside {1, 2, 3}; and a fused aggregate -> GEMM shape that does not fit LDS is refused on the host
    assert lib.tfgx_segment_max_backward_mask_phases_f32(None, None, None, 4, 8, None, 8, 8, None, 8, None, 8, None, 8, None, 8,
                                                         None, None, None, None, 4, None, 8, None, 0, 0, None) == 1
    assert lib.tfgx_aggregate_gemm_fits(128, 256) == 1 and lib.tfgx_aggregate_gemm_fits(100, 256) == 1
    assert lib.tfgx_aggregate_gemm_fits(102, 16) == 0 and lib.tfgx_aggregate_gemm_fits(100, 257) == 0
    g = _lib.GatArgs()
    g.H, g.d, g.dv, g.n_dst, g.scale, g.drop_rate = 2, 4, 4, 3, 2.0, 1.5
    assert lib.tfgx_gat_fused_f32(ctypes.byref(g), None) == 1
    # GAT backward: bad head geometry / scale, and packed destination tables whose rows cannot hold what goes in them
    gb = _lib.GatBackwardArgs()
    gb.d, gb.dv, gb.n_dst, gb.n_src = 4, 8, 3, 3
    for fn in (lib.tfgx_gat_backward_dst_f32, lib.tfgx_gat_backward_src_f32):
        gb.H, gb.scale = 0, 2.0
        assert fn(ctypes.byref(gb), None) == 1 and b"bad H / d / dv / scale" in lib.tfgx_last_error()
        gb.H, gb.scale = 2, 0.0
        assert fn(ctypes.byref(gb), None) == 1 and b"bad H / d / dv / scale" in lib.tfgx_last_error()
    H, d, dv = 2, 4, 8                                     # W = 16, A = 8: [dO | Q | (m, l) | D] needs 30 floats a row
    assert lib.tfgx_gat_pack_dst_f32(None, 16, None, 16, None, 8, None, 5, H, d, dv, None, 29, None, None) == 1
    assert b"leading dimension too small" in lib.tfgx_last_error()
    assert lib.tfgx_gat_pack_dst_f32(None, 16, None, 16, None, 8, None, 5, H, d, dv, None, 30, None, None) == 1
    assert b"null pointer" in lib.tfgx_last_error()                                   # (30 is enough: the next check)
    # head blocks: roundup4(16) + 2 * roundup4(4 + 3) = 32 floats a row
    assert lib.tfgx_gat_pack_dst_heads_f32(None, 16, None, 16, None, 8, None, 5, H, d, dv, None, 31, None, None) == 1
    assert b"ld_pack >= roundup4(H * dv) + H * roundup4(d + 3)" in lib.tfgx_last_error()
    assert lib.tfgx_gat_pack_dst_heads_f32(None, 16, None, 16, None, 8, None, 5, H, d, dv, None, 32, None, None) == 1
    assert b"null pointer" in lib.tfgx_last_error()
    assert lib.tfgx_dropout_keep(7, 3, 0.0) == 1                                      # rate 0 keeps everything
    kept = sum(lib.tfgx_dropout_keep(0x1234567890, i, 0.25) for i in range(4000))
    assert 2850 < kept < 3150                                                         # ~75 %
    assert [lib.tfgx_dropout_keep(99, i, 0.5) for i in range(64)] == [lib.tfgx_dropout_keep(99, i, 0.5) for i in range(64)]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_product_path_fails_loudly_without_gpu():
    import tf_geometric_amd as tfg
    x = np.ones((4, 3), np.float32)
    ei = np.array([[0, 1], [1, 0]], np.int32)
    with pytest.raises(tfg._lib.TfgxError):
        tfg.nn.aggregate_neighbors(x, ei, None)
    with pytest.raises(tfg._lib.TfgxError):
        tfg.layers.GCN(4)([x, ei])
    with pytest.raises(tfg._lib.TfgxError):
        tfg.layers.GAT(4)([x, ei])
    with pytest.raises(tfg._lib.TfgxError):
        tfg.layers.MeanGraphSage(4)([x, ei])
    with pytest.raises(tfg._lib.TfgxError):
        tfg.SparseMatrix(ei, None, [4, 4]) @ x


def test_product_never_imports_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkg = os.path.join(ROOT, "tf_geometric_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if not fn.endswith((".py", ".hip", ".h")):
                continue
            for line in open(os.path.join(dirpath, fn)).read().splitlines():
                assert not re.match(r"\s*(from|import)\s+oracle", line), "{} imports oracle".format(fn)
                assert "libtfg_oracle" not in line and "tfg_oracle" not in line, "{} references the oracle".format(fn)


def test_activation_resolution_and_layer_contract():
    import tf_geometric_amd as tfg
    from tf_geometric_amd.activations import resolve
    assert resolve(None) == (0, None) and resolve("relu") == (1, None) and resolve(tfg.relu) == (1, None)
    assert resolve(torch.relu) == (1, None)
    code, post = resolve(torch.tanh)
    assert code == 0 and post is torch.tanh
    with pytest.raises(ValueError):
        resolve("gelu")
    with pytest.raises(Exception):
        tfg.layers.GCN(4, num_splits=2, num_or_size_splits=2)                 # layers/conv/gcn.py:82-83
    with pytest.raises(Exception):
        tfg.layers.MeanGraphSage(5, concat=True)                              # layers/conv/graph_sage.py:36-37
    from tf_geometric_amd.nn.conv.gcn import compute_cache_key
    assert compute_cache_key("both", True, True, True, False) == "gcn_normed_adj_both_True_True_True_False"


def test_synthetic_inputs_are_reproducible():
    from tf_geometric_amd import synthetic
    a = synthetic.synthetic_edges(1000, 5000, seed=0)
    b = synthetic.synthetic_edges(1000, 5000, seed=0)
    assert np.array_equal(a, b) and a.dtype == np.int32 and a.shape[0] == 2
    half = a.shape[1] // 2
    assert np.array_equal(a[0, :half], a[1, half:]) and np.array_equal(a[1, :half], a[0, half:])   # (a,b) then (b,a)
    assert (a[0] != a[1]).all()


def test_dist_library_exports_every_declared_symbol():
    """include/tfgx_dist.h (the halo-exchange C ABI: ncclComm_t + streams) vs lib/libtfgx_dist.so; host
    argument checks run without a GPU (no RCCL call is reached)."""
    from tf_geometric_amd import _build
    with open(os.path.join(ROOT, "include", "tfgx_dist.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tfgx_[a-z0-9_]+)\s*\(", src)))
    assert len(names) == 19, names          # 19 = + tfgx_dist_comm_abort (round 5)
    if not os.path.exists(_build.DIST_LIB):
        _build.build_dist(verbose=False)
    lib = ctypes.CDLL(_build.DIST_LIB)
    for name in names:
        assert hasattr(lib, name), "libtfgx_dist.so does not export {}".format(name)
    lib.tfgx_dist_last_error.restype = ctypes.c_char_p
    plan = ctypes.c_void_p()
    cnt = (ctypes.c_int64 * 4)(0, 3, 0, 2)
    assert lib.tfgx_halo_plan_create(2, 5, 2, cnt, cnt, None, None, ctypes.byref(plan)) == 1      # rank outside world
    assert b"bad world" in lib.tfgx_dist_last_error()
    assert lib.tfgx_halo_plan_create(2, 0, 2, cnt, cnt, None, None, ctypes.byref(plan)) == 1      # rows to pack, no index list
    dense = (ctypes.c_int64 * 4)(-1, 0, -1, 3)          # every non-empty (round, peer) entry is a contiguous block:
    rc = lib.tfgx_halo_plan_create(2, 0, 2, cnt, cnt, dense, None, ctypes.byref(plan))            # nothing to pack: the
    assert rc in (0, 4)           # arguments are accepted; without a GPU the plan's hipEventCreate then fails (TFGX_ERR_HIP)
    if rc == 0:
        lib.tfgx_halo_plan_rows_packed.restype = lib.tfgx_halo_plan_rows_sent.restype = ctypes.c_int64
        assert lib.tfgx_halo_plan_rows_packed(plan) == 0 and lib.tfgx_halo_plan_rows_sent(plan) == 5
        assert lib.tfgx_halo_plan_destroy(plan) == 0
    else:
        assert b"hipEventCreate" in lib.tfgx_dist_last_error()
    assert lib.tfgx_dist_comm_init(0, 0, None, None) == 1 and lib.tfgx_dist_unique_id(None) == 1
    assert lib.tfgx_dist_comm_info(None, None, None, None) == 1
    assert lib.tfgx_alltoallv(None, None, None, None, 4, 2, None, None) == 1
    assert lib.tfgx_halo_exchange_finish(None, 0, None) == 1
    assert lib.tfgx_halo_reverse_start(None, None, 4, None, 0, None, None, None) == 1
    assert lib.tfgx_halo_reverse_start_round(None, 0, None, 4, None, 0, None, None, None) == 1
    assert lib.tfgx_halo_reverse_finish(None, None, 4, 4, None, None) == 1


def test_tf_shim_compiles_against_mock_headers():
    """integration/tf_shim/tfgx_tf_ops.cc (the tf.load_op_library binding of INTEGRATION.md) type-checks against
    include/tfgx.h and a mock of the TensorFlow headers it uses: every C-ABI call in it has the declared argument
    types.  TensorFlow itself is not installable here — the shim is a sketch that has never been linked or run."""
    shim = os.path.join(ROOT, "integration", "tf_shim")
    res = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(shim, "mock"),
                          "-I", os.path.join(ROOT, "include"), os.path.join(shim, "tfgx_tf_ops.cc")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode()
    src = open(os.path.join(shim, "tfgx_tf_ops.cc")).read()
    ops = ("TfgxBuildCsrByDst", "TfgxSegmentReduce", "TfgxGatFused", "TfgxGcnNormEdges", "TfgxGemmBiasAct", "TfgxAggregateGemm",
           # round 3: the backward ops and the sharded path
           "TfgxSddmm", "TfgxPermuteRows", "TfgxGemmTn", "TfgxReluBackward", "TfgxHaloExchange", "TfgxHaloReverse",
           "TfgxAllReduceSum")
    for op in ops:
        assert 'REGISTER_OP("{}")'.format(op) in src and 'Name("{}")'.format(op) in src
    # the Python side (gradient registration, GCN layer over the ops): compiles, and names only ops the library registers
    import py_compile
    pyfile = os.path.join(shim, "tfgx_tf.py")
    py_compile.compile(pyfile, doraise=True)
    pysrc = open(pyfile).read()
    snake = {re.sub(r"(?<!^)(?=[A-Z])", "_", op).lower() for op in ops}
    used = set(re.findall(r"ops\.(tfgx_[a-z_]+)\(", pysrc))
    assert used and used <= snake, used - snake
    for grad in ("TfgxSegmentReduce", "TfgxGemmBiasAct", "TfgxHaloExchange"):
        assert '@tf.RegisterGradient("{}")'.format(grad) in pysrc


def test_host_code_under_address_sanitizer():
    """SURVEY.md §5 (memory-error detection): the host side of the C-ABI library built with AddressSanitizer
    (lib/asan/libtfgx.so, device code untouched) survives a sweep over its entry points' validation / query paths —
    including a deliberately short output buffer — without an ASAN report."""
    from tf_geometric_amd import _build
    rt = _build.asan_runtime()
    if rt is None:
        pytest.skip("clang's shared ASAN runtime is not in this ROCm image")
    lib = _build.build_asan(verbose=False)
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    res = subprocess.run([os.sys.executable, os.path.join(ROOT, "tools", "asan_host_check.py"), lib], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = res.stdout.decode()
    assert res.returncode == 0 and "ASAN_HOST_CHECK_OK" in text and "AddressSanitizer" not in text, text[-3000:]
