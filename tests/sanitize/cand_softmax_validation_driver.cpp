// ASan + UBSan run of the HOST half of nrx_cand_softmax_workspace, nrx_cand_softmax_fwd and nrx_cand_softmax_bwd (include/nrx_embed.h):
// their argument validation, status codes and error text, compiled from the library's own sources with host-side sanitizers (hipcc
// -fsanitize=address,undefined -fno-gpu-sanitize; the device code is not instrumented and never runs: every call below fails validation BEFORE any
// launch, or has nothing to do).  No GPU needed.  Built by tests/sanitize/cand_softmax.mk and run by tests/test_candidate_softmax.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nrx_embed.h"

static int failures = 0;
#define EXPECT_RC(call, rc_, word)                                                                        \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        const char* e__ = nrx_last_error();                                                               \
        if (rc__ != (rc_) || e__ == nullptr || std::strstr(e__, word) == nullptr) {                       \
            std::fprintf(stderr, "expected %d naming '%s' from %s, got %d (%s)\n", (rc_), word, #call, rc__, e__ ? e__ : "");           \
            ++failures;                                                                                   \
        }                                                                                                 \
    } while (0)
#define EXPECT_BAD(call, word) EXPECT_RC(call, NRX_ERR_BAD_ARG, word)
#define EXPECT_OK(call)                                                                                   \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        if (rc__ != 0) { std::fprintf(stderr, "%s returned %d (%s)\n", #call, rc__, nrx_last_error()); ++failures; } \
    } while (0)
#define EXPECT_TRUE(cond)                                                                                 \
    do {                                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "%s does not hold\n", #cond); ++failures; }                   \
    } while (0)

template <typename T>
static T* off(T* p, int bytes) { return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + bytes); }

int main() {
    // "device" buffers: never dereferenced by the host code under test
    float* u = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* v = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* gu = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* gv = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* loss = static_cast<float*>(std::aligned_alloc(64, 256));
    float* lse = static_cast<float*>(std::aligned_alloc(64, 256));
    float* g = static_cast<float*>(std::aligned_alloc(64, 256));
    float* bias = static_cast<float*>(std::aligned_alloc(64, 256));
    int64_t* ids = static_cast<int64_t*>(std::aligned_alloc(64, 256));
    void* ws = std::aligned_alloc(64, 4096);
    const float inf = std::strtof("inf", nullptr), nan = std::strtof("nan", nullptr);
    if (nrx_abi_version() != NRX_ABI_VERSION) ++failures;

    // the size call: -1 for anything the entry points refuse; a square set without a bias needs what the in-batch op needs
    EXPECT_TRUE(nrx_cand_softmax_workspace(8, 12, 16, 1) >= 4 * 3 * 8);
    EXPECT_TRUE(nrx_cand_softmax_workspace(8, 12, 16, 3) >= 4 * 3 * 12 * 16);
    EXPECT_TRUE(nrx_cand_softmax_workspace(0, 0, 16, 0) >= 0 && nrx_cand_softmax_workspace(0, 12, 16, 0) >= 0);
    for (int64_t b : {1LL, 33LL, 511LL, 512LL, 1000LL, 4096LL, 8191LL, 65536LL, 1000000LL})
        for (int32_t sp : {0, 1, 3, 64})
            EXPECT_TRUE(nrx_cand_softmax_workspace(b, b, 16, sp) == nrx_inbatch_softmax_workspace(b, 16, sp));
    // ... and never a [batch, n_cand] matrix
    EXPECT_TRUE(nrx_cand_softmax_workspace(4096, 8192, 16, 0) < 4096LL * 8192 * 4 / 8);
    EXPECT_TRUE(nrx_cand_softmax_workspace(-1, 12, 16, 0) == -1 && nrx_cand_softmax_workspace(8, 7, 16, 0) == -1);
    EXPECT_TRUE(nrx_cand_softmax_workspace(8, 0x7fffffffLL, 16, 0) == -1 && nrx_cand_softmax_workspace(8, INT64_MAX, 16, 0) == -1);
    EXPECT_TRUE(nrx_cand_softmax_workspace(8, 12, 0, 0) == -1 && nrx_cand_softmax_workspace(8, 12, 5, 0) == -1 && nrx_cand_softmax_workspace(8, 12, 132, 0) == -1);
    EXPECT_TRUE(nrx_cand_softmax_workspace(8, 12, 96, 0) == -1 && nrx_cand_softmax_workspace(8, 12, 16, -1) == -1 && nrx_cand_softmax_workspace(8, 12, 16, 65) == -1);
    EXPECT_TRUE(nrx_cand_softmax_workspace(0x7fffffffLL - 128, 0x7fffffffLL - 128, 64, 64) == -1);
    EXPECT_TRUE(nrx_cand_softmax_workspace(0x7fffffffLL - 129, 0x7fffffffLL - 129, 64, 64) > 0);       // the largest sizes: no overflow

#define FWD(u_, uld_, v_, vld_, b_, n_, d_, it_, ids_, bits_, bias_, sp_, lo_, ls_, ws_) \
    nrx_cand_softmax_fwd(u_, uld_, v_, vld_, b_, n_, d_, it_, ids_, bits_, bias_, sp_, lo_, ls_, ws_, nullptr)
#define BWD(u_, uld_, v_, vld_, b_, n_, d_, it_, ids_, bits_, bias_, sp_, ls_, g_, gu_, guld_, gv_, gvld_, ws_) \
    nrx_cand_softmax_bwd(u_, uld_, v_, vld_, b_, n_, d_, it_, ids_, bits_, bias_, sp_, ls_, g_, gu_, guld_, gv_, gvld_, ws_, nullptr)
    // forward: sizes
    EXPECT_BAD(FWD(u, 16, v, 16, -1, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "batch");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 7, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "n_cand");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, -3, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "n_cand");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 0x7fffffffLL, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "n_cand");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 1LL << 40, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "n_cand");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 0, 10.f, ids, 64, bias, 0, loss, lse, ws), "dim");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 5, 10.f, ids, 64, bias, 0, loss, lse, ws), "dim");
    EXPECT_BAD(FWD(u, 132, v, 132, 8, 12, 132, 10.f, ids, 64, bias, 0, loss, lse, ws), "dim");
    EXPECT_RC(FWD(u, 96, v, 96, 8, 12, 96, 10.f, ids, 64, bias, 0, loss, lse, ws), NRX_ERR_UNSUPPORTED, "dim");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, -1, loss, lse, ws), "col_splits");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 65, loss, lse, ws), "col_splits");
    EXPECT_BAD(FWD(u, 12, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "row stride");
    EXPECT_BAD(FWD(u, 16, v, 12, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "row stride");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 16, bias, 0, loss, lse, ws), "index_bits");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 0.f, ids, 64, bias, 0, loss, lse, ws), "inv_temperature");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, -1.f, ids, 64, bias, 0, loss, lse, ws), "inv_temperature");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, inf, ids, 64, bias, 0, loss, lse, ws), "inv_temperature");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, nan, ids, 64, bias, 0, loss, lse, ws), "inv_temperature");
    // ... null and misaligned buffers (ids and bias may be null: that is "none")
    EXPECT_BAD(FWD(nullptr, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "null buffer");
    EXPECT_BAD(FWD(u, 16, nullptr, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "null buffer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, nullptr, lse, ws), "null buffer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, nullptr, ws), "null buffer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, nullptr, 32, nullptr, 0, loss, lse, nullptr), "null buffer");
    EXPECT_BAD(FWD(off(u, 4), 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "misaligned rows");
    EXPECT_BAD(FWD(u, 16, off(v, 8), 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "misaligned rows");
    EXPECT_BAD(FWD(u, 18, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "misaligned rows");
    EXPECT_BAD(FWD(u, 16, v, 17, 8, 12, 16, 10.f, ids, 64, bias, 0, loss, lse, ws), "misaligned rows");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, off(ids, 4), 64, bias, 0, loss, lse, ws), "misaligned pointer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, off(ids, 2), 32, bias, 0, loss, lse, ws), "misaligned pointer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, off(bias, 2), 0, loss, lse, ws), "misaligned pointer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, off(bias, 1), 0, loss, lse, ws), "misaligned pointer");
    EXPECT_BAD(FWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, off(loss, 2), lse, ws), "misaligned pointer");
    // ... an empty batch has nothing to launch, whatever the pointers and however many candidates
    EXPECT_OK(FWD(nullptr, 16, nullptr, 16, 0, 0, 16, 10.f, nullptr, 32, nullptr, 0, nullptr, nullptr, nullptr));
    EXPECT_OK(FWD(u, 64, v, 64, 0, 12, 64, 10.f, ids, 64, bias, 3, loss, lse, ws));

    // backward
    EXPECT_BAD(BWD(u, 16, v, 16, -1, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "batch");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 7, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "n_cand");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 0x7fffffffLL, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "n_cand");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 0, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "dim");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 5, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "dim");
    EXPECT_BAD(BWD(u, 132, v, 132, 8, 12, 132, 10.f, ids, 64, bias, 0, lse, g, gu, 132, gv, 132, ws), "dim");
    EXPECT_RC(BWD(u, 128, v, 128, 8, 12, 128, 10.f, ids, 64, bias, 0, lse, g, gu, 128, gv, 128, ws), NRX_ERR_UNSUPPORTED, "dim");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 65, lse, g, gu, 16, gv, 16, ws), "col_splits");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, -1, lse, g, gu, 16, gv, 16, ws), "col_splits");
    EXPECT_BAD(BWD(u, 12, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "row stride");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 12, gv, 16, ws), "row stride");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 8, ws), "row stride");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 16, bias, 0, lse, g, gu, 16, gv, 16, ws), "index_bits");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 0.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "inv_temperature");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, nan, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "inv_temperature");
    EXPECT_BAD(BWD(nullptr, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "null buffer");
    EXPECT_BAD(BWD(u, 16, nullptr, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "null buffer");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, nullptr, g, gu, 16, gv, 16, ws), "null buffer");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, nullptr, gu, 16, gv, 16, ws), "null buffer");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, nullptr, 16, nullptr), "null buffer");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, off(gu, 4), 16, gv, 16, ws), "misaligned rows");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 18, ws), "misaligned rows");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, off(lse, 1), g, gu, 16, gv, 16, ws), "misaligned pointer");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, off(bias, 2), 0, lse, g, gu, 16, gv, 16, ws), "misaligned pointer");
    EXPECT_BAD(BWD(u, 16, v, 16, 8, 12, 16, 10.f, off(ids, 4), 64, bias, 0, lse, g, gu, 16, gv, 16, ws), "misaligned pointer");
    // ... nothing to do: an empty batch (g_v's rows stay the caller's), or neither gradient asked for
    EXPECT_OK(BWD(nullptr, 16, nullptr, 16, 0, 0, 16, 10.f, nullptr, 32, nullptr, 0, nullptr, nullptr, nullptr, 16, nullptr, 16, nullptr));
    EXPECT_OK(BWD(u, 16, v, 16, 0, 12, 16, 10.f, ids, 64, bias, 0, lse, g, gu, 16, gv, 16, ws));
    EXPECT_OK(BWD(u, 16, v, 16, 8, 12, 16, 10.f, ids, 64, bias, 0, lse, g, nullptr, 0, nullptr, 0, ws));

    std::free(u); std::free(v); std::free(gu); std::free(gv); std::free(loss); std::free(lse); std::free(g); std::free(bias); std::free(ids); std::free(ws);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("nrx_cand_softmax validation sanitize driver: OK");
    return 0;
}
