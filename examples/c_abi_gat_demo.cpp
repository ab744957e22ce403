// The fast GAT attention routes from a host that has only include/tfgx.h and libtfgx.so (no Python, no torch): what a
// tf.load_op_library op or a ctypes binding does to get the same launches the Python package makes.
//
//   c_abi_gat_demo DIR      reads   DIR/meta.bin  int64 {n, H, A, W}    (n nodes, H heads, A = H*d, W = H*dv)
//                                   DIR/row.bin, DIR/col.bin  int32 [E] (edge_index[0] = destination, [1] = source)
//                                   DIR/q.bin [n, A], DIR/k.bin [n, A], DIR/v.bin [n, W]  float32, row-major
//                           writes  DIR/out.bin  float32 [n, W]  (softmax attention with self-loops, no bias / activation)
//
// 1. the CSR plan (tfgx_build_csr_by_dst);
// 2. the library's policies and per-plan structures, built on the device: walk order (tfgx_plan_row_order), hub lists
//    (tfgx_hub_policy + tfgx_plan_hub_lists_count / _emit), hub_order_slot, and the number of source blocks
//    (tfgx_gat_source_block_count) with the partition they need (tfgx_plan_source_blocks);
// 3. the attention as tf_geometric_amd/nn/conv/gat.py:gat_attention launches it — on a dense, near-regular plan KB chained
//    tfgx_gat_fused_f32 launches over the source blocks (raw softmax state handed from launch to launch, double-buffered,
//    the last launch adding the self-loop and finishing the rows), otherwise one launch with the walk order and hub lists.
// Prints the route taken and the plan-structure build time (hipEvents; information only).
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/c_abi_gat_demo.cpp -L tf_geometric_amd/lib -ltfgx \
//         -Wl,-rpath,'$ORIGIN' -o tf_geometric_amd/lib/c_abi_gat_demo
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "tfgx.h"

#define HIP_OK(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));               \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)
#define TFGX_OK_OR_DIE(call)                                                              \
    do {                                                                                  \
        int rc_ = (call);                                                                 \
        if (rc_ != 0) {                                                                   \
            std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tfgx_last_error());        \
            return 3;                                                                     \
        }                                                                                 \
    } while (0)

template <typename T>
static bool read_file(const std::string& path, std::vector<T>& out)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (f == nullptr) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(size_t(bytes) / sizeof(T));
    const size_t got = out.empty() ? 0 : std::fread(out.data(), sizeof(T), out.size(), f);
    std::fclose(f);
    return got == out.size() && size_t(bytes) % sizeof(T) == 0;
}

// device buffers owned by the demo, freed at exit
static std::vector<void*> g_bufs;
static void* dev_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipMalloc(&p, bytes > 0 ? bytes : 1) != hipSuccess) return nullptr;
    g_bufs.push_back(p);
    return p;
}
template <typename T>
static T* to_device(const std::vector<T>& h)
{
    T* d = static_cast<T*>(dev_alloc(sizeof(T) * h.size()));
    if (d != nullptr && !h.empty() && hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) != hipSuccess)
        return nullptr;
    return d;
}
static void free_all()
{
    for (void* p : g_bufs) (void)hipFree(p);
    g_bufs.clear();
}

static int run(const std::string& dir)
{
    std::vector<int64_t> meta;
    std::vector<int32_t> row, col;
    std::vector<float> q, k, v;
    if (!read_file(dir + "/meta.bin", meta) || meta.size() != 4 || !read_file(dir + "/row.bin", row) ||
        !read_file(dir + "/col.bin", col) || !read_file(dir + "/q.bin", q) || !read_file(dir + "/k.bin", k) ||
        !read_file(dir + "/v.bin", v)) {
        std::fprintf(stderr, "cannot read the inputs in %s\n", dir.c_str());
        return 1;
    }
    const int64_t n = meta[0], H = meta[1], A = meta[2], W = meta[3], E = int64_t(row.size());
    if (n < 1 || H < 1 || A % H || W % H || int64_t(col.size()) != E || int64_t(q.size()) != n * A ||
        int64_t(k.size()) != n * A || int64_t(v.size()) != n * W) {
        std::fprintf(stderr, "inconsistent input sizes\n");
        return 1;
    }
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    int32_t *d_row = to_device(row), *d_col = to_device(col);
    float *d_q = to_device(q), *d_k = to_device(k), *d_v = to_device(v);
    float* d_out = static_cast<float*>(dev_alloc(sizeof(float) * size_t(n * W)));
    if (!d_row || !d_col || !d_q || !d_k || !d_v || !d_out) return 2;

    // 1. the plan
    int32_t* row_ptr = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n + 1)));
    int32_t* plan_col = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(E)));
    int32_t* perm = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(E)));
    const size_t ws_plan = tfgx_csr_plan_workspace_bytes(n, E);
    void* ws = dev_alloc(ws_plan);
    if (!row_ptr || !plan_col || !perm || !ws) return 2;
    TFGX_OK_OR_DIE(tfgx_build_csr_by_dst(d_row, d_col, E, n, n, row_ptr, plan_col, perm, ws, ws_plan, stream));

    // 2. the per-plan structures
    hipEvent_t t0, t1;
    HIP_OK(hipEventCreate(&t0));
    HIP_OK(hipEventCreate(&t1));
    HIP_OK(hipEventRecord(t0, stream));
    int32_t* order = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n)));
    const size_t ws_order = tfgx_plan_row_order_workspace_bytes(n);
    void* ws_o = dev_alloc(ws_order);
    if (!order || !ws_o) return 2;
    int32_t skewed = 0;
    TFGX_OK_OR_DIE(tfgx_plan_row_order(row_ptr, n, E, order, &skewed, ws_o, ws_order, stream));

    int32_t thr = 0, chunk = 0;
    TFGX_OK_OR_DIE(tfgx_hub_policy(E, n, &thr, &chunk));
    const size_t ws_hub = tfgx_plan_hub_lists_workspace_bytes(n);
    void* ws_h = dev_alloc(ws_hub);
    if (!ws_h) return 2;
    int64_t n_hub = 0, n_chunks = 0;
    TFGX_OK_OR_DIE(tfgx_plan_hub_lists_count(row_ptr, row_ptr + 1, 1, n, thr, chunk, &n_hub, &n_chunks, ws_h, ws_hub, stream));
    int32_t *hub_rows = nullptr, *chunk_ptr = nullptr, *chunk_begin = nullptr, *chunk_end = nullptr, *chunk_row = nullptr;
    if (n_hub > 0) {
        hub_rows = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n_hub)));
        chunk_ptr = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n_hub + 1)));
        chunk_begin = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n_chunks)));
        chunk_end = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n_chunks)));
        chunk_row = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n_chunks)));
        if (!hub_rows || !chunk_ptr || !chunk_begin || !chunk_end || !chunk_row) return 2;
        TFGX_OK_OR_DIE(tfgx_plan_hub_lists_emit(row_ptr, row_ptr + 1, 1, n, thr, chunk, n_hub, n_chunks, hub_rows, chunk_ptr,
                                                chunk_begin, chunk_end, chunk_row, ws_h, ws_hub, stream));
    }
    // nn/conv/gat.py: the source blocks only on near-regular plans (no walk order, no hub rows); the policy's defaults
    int32_t KB = 1;
    int32_t *rpk = nullptr, *col_k = nullptr;
    if (!skewed && n_hub == 0) {
        KB = tfgx_gat_source_block_count(n, n, E, A, W, 0, 0);
        if (KB < 1) {
            std::fprintf(stderr, "tfgx_gat_source_block_count: %s\n", tfgx_last_error());
            return 3;
        }
        if (KB >= 2) {
            rpk = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(n * KB + 1)));
            col_k = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * size_t(E)));
            if (!rpk || !col_k) return 2;
            TFGX_OK_OR_DIE(tfgx_plan_source_blocks(row_ptr, plan_col, n, n, E, KB, rpk, col_k, stream));
        }
    }
    HIP_OK(hipEventRecord(t1, stream));
    HIP_OK(hipEventSynchronize(t1));
    float build_ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&build_ms, t0, t1));

    // 3. the attention (the fields nn/conv/gat.py:gat_args fills)
    tfgx_gat_args base = {};
    base.n_dst = n;
    base.q = d_q, base.ldq = A;
    base.k = d_k, base.ldk = A;
    base.v = d_v, base.ldv = W;
    base.ldo = W > 0 ? W : 1;
    base.H = int32_t(H), base.d = int32_t(A / H), base.dv = int32_t(W / H);
    base.scale = float(std::sqrt(double(A / H)));
    base.act = TFGX_ACT_NONE;
    if (KB >= 2) {
        const int nb = KB > 2 ? 2 : 1;
        float* acc[2] = {nullptr, nullptr};
        float* ml[2] = {nullptr, nullptr};
        for (int i = 0; i < nb; ++i) {
            acc[i] = static_cast<float*>(dev_alloc(sizeof(float) * size_t(n * W)));
            ml[i] = static_cast<float*>(dev_alloc(sizeof(float) * size_t(n * 2 * H)));
            if (!acc[i] || !ml[i]) return 2;
        }
        const float *prev_acc = nullptr, *prev_ml = nullptr;
        for (int32_t b = 0; b < KB; ++b) {
            const bool last = b == KB - 1;
            tfgx_gat_args a = base;
            a.col = col_k;
            a.row_begin = rpk + b, a.row_end = rpk + b + 1, a.rp_stride = KB;
            a.add_self_loop = last ? 1 : 0;
            a.state_in_acc = prev_acc, a.state_in_ml = prev_ml;
            if (last) {
                a.out = d_out;
            } else {
                a.out = acc[b % nb];
                a.state_acc = acc[b % nb], a.state_ml = ml[b % nb];
                prev_acc = acc[b % nb], prev_ml = ml[b % nb];
            }
            TFGX_OK_OR_DIE(tfgx_gat_fused_f32(&a, stream));
        }
        std::printf("route=source_blocks KB=%d\n", KB);
    } else {
        tfgx_gat_args a = base;
        a.row_ptr = row_ptr, a.col = plan_col, a.out = d_out, a.add_self_loop = 1;
        if (skewed) a.row_order = order;
        if (n_hub > 0) {
            float* s_acc = static_cast<float*>(dev_alloc(sizeof(float) * size_t(n_chunks * W)));
            float* s_ml = static_cast<float*>(dev_alloc(sizeof(float) * size_t(n_chunks * 2 * H)));
            if (!s_acc || !s_ml) return 2;
            a.hub_threshold = thr;
            a.hub_rows = hub_rows, a.hub_chunk_ptr = chunk_ptr, a.hub_chunk_begin = chunk_begin, a.hub_chunk_end = chunk_end;
            a.hub_chunk_row = chunk_row, a.n_hub_rows = n_hub, a.n_hub_chunks = n_chunks;
            a.hub_scratch_acc = s_acc, a.hub_scratch_ml = s_ml;
        }
        TFGX_OK_OR_DIE(tfgx_gat_fused_f32(&a, stream));
        std::printf("route=one_pass KB=1 row_order=%d hub_rows=%lld hub_chunks=%lld\n", int(skewed), (long long)n_hub,
                    (long long)n_chunks);
    }
    HIP_OK(hipStreamSynchronize(stream));
    std::vector<float> out(size_t(n * W));
    HIP_OK(hipMemcpy(out.data(), d_out, sizeof(float) * out.size(), hipMemcpyDeviceToHost));
    FILE* f = std::fopen((dir + "/out.bin").c_str(), "wb");
    if (f == nullptr || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) {
        std::fprintf(stderr, "cannot write %s/out.bin\n", dir.c_str());
        if (f) std::fclose(f);
        return 1;
    }
    std::fclose(f);
    std::printf("plan_structures_ms=%.3f n=%lld E=%lld hub_threshold=%d\n", double(build_ms), (long long)n, (long long)E, thr);
    HIP_OK(hipEventDestroy(t0));
    HIP_OK(hipEventDestroy(t1));
    HIP_OK(hipStreamDestroy(stream));
    std::printf("C_ABI_GAT_DEMO_OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 1;
    }
    const int rc = run(argv[1]);
    free_all();
    return rc;
}
