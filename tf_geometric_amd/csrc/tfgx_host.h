// Host-side helpers of the entry points: the refusals that name their argument, and workspaces that are described once.
#pragma once
#include "tfgx_common.h"
#include <hipcub/hipcub.hpp>

namespace tfgx {

constexpr int64_t kMaxSize = (int64_t(1) << 31) - 1;      // sizes and ids are int32 on the device

// the refusals every entry point shares: a negative size, a size that does not fit int32 — with the argument named
inline int check_size(const char* fn, const char* name, int64_t v)
{
    if (v < 0) {
        set_error("%s: negative size (%s = %lld)", fn, name, (long long)v);
        return TFGX_ERR_INVALID_ARG;
    }
    if (v >= kMaxSize) {
        set_error("%s: %s = %lld does not fit int32", fn, name, (long long)v);
        return TFGX_ERR_INVALID_ARG;
    }
    return TFGX_OK;
}

struct NamedSize {
    const char* name;
    int64_t v;
};

// check_size over a list; the first size that is refused decides the message
template <size_t N>
int check_sizes(const char* fn, const NamedSize (&sizes)[N])
{
    for (const auto& s : sizes)
        if (int rc = check_size(fn, s.name, s.v)) return rc;
    return TFGX_OK;
}

// The refusals of a padded tail (fixed-shape batches: the last `sinks` rows hold the e_cap padded edges, sink_degree to a row).
// One helper per refusal: every entry point calls them in its own order, and the first that fires decides the message.
inline int check_sink_degree(const char* fn, int64_t sink_degree)
{
    if (sink_degree >= 1) return TFGX_OK;
    set_error("%s: sink_degree = %lld must be at least 1", fn, (long long)sink_degree);
    return TFGX_ERR_INVALID_ARG;
}

inline int check_sinks_within(const char* fn, int64_t sinks, const char* rows_name, int64_t rows)
{
    if (sinks <= rows) return TFGX_OK;
    set_error("%s: sinks = %lld is more than %s = %lld rows", fn, (long long)sinks, rows_name, (long long)rows);
    return TFGX_ERR_INVALID_ARG;
}

inline int check_sink_tail(const char* fn, int64_t sinks, int64_t sink_degree, int64_t e_cap)
{
    if (sinks * sink_degree >= e_cap) return TFGX_OK;      // both factors are below 2^31: no overflow
    set_error("%s: sinks = %lld of sink_degree = %lld cannot hold a tail of e_cap = %lld padded edges", fn, (long long)sinks,
              (long long)sink_degree, (long long)e_cap);
    return TFGX_ERR_INVALID_ARG;
}

inline int null_arg(const char* fn, const char* name)
{
    set_error("%s: %s is null", fn, name);
    return TFGX_ERR_INVALID_ARG;
}

inline int bad_arg(const char* fn, const char* what, long long v)
{
    set_error("%s: %s (got %lld)", fn, what, v);
    return TFGX_ERR_INVALID_ARG;
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// hipcub's scratch for one exclusive int32 sum over n items
inline size_t scan_bytes(int64_t n)
{
    size_t temp = 0;
    const int32_t* in = nullptr;
    int32_t* out = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, temp, in, out, static_cast<int>(n > 0 ? n : 1));
    return temp;
}

// radix-sort bits that tell n keys [0, n) apart
inline int key_bits(int64_t n)
{
    int b = 1;
    while (b < 31 && (int64_t(1) << b) < n) ++b;
    return b;
}

// A workspace, described ONCE by the byte counts of its pieces in order.  bytes() is what the *_workspace_bytes query returns:
// every piece rounded up to 256 bytes, plus 256 of slack for a caller's block that does not start on such a boundary;
// at(workspace, i) is piece i of that block, on a 256-byte boundary.
template <int N>
struct Workspace {
    size_t piece[N];

    size_t bytes() const
    {
        size_t b = 256;
        for (int i = 0; i < N; ++i) b += align256(piece[i]);
        return b;
    }

    template <class T = void>
    T* at(void* workspace, int i) const
    {
        char* p = reinterpret_cast<char*>(align256(reinterpret_cast<uintptr_t>(workspace)));
        for (int j = 0; j < i; ++j) p += align256(piece[j]);
        return reinterpret_cast<T*>(p);
    }
};

}  // namespace tfgx
