// ASan + UBSan run of the HOST half of nrx_sparse_adagrad_step (include/nrx_embed.h): its argument validation, status codes and error text,
// compiled from the library's own sources with host-side sanitizers (hipcc -fsanitize=address,undefined -fno-gpu-sanitize; the device code is
// not instrumented and never runs: every call below fails validation BEFORE any launch, or has nothing to do).  No GPU needed.  Built by
// tests/sanitize/adagrad.mk and run by tests/test_sparse_adagrad.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nrx_embed.h"

static int failures = 0;
#define EXPECT_BAD(call, word)                                                                            \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        const char* e__ = nrx_last_error();                                                               \
        if (rc__ != NRX_ERR_BAD_ARG || e__ == nullptr || std::strstr(e__, word) == nullptr) {             \
            std::fprintf(stderr, "expected a validation error naming '%s' from %s, got %d (%s)\n", word, #call, rc__, e__ ? e__ : "");           \
            ++failures;                                                                                   \
        }                                                                                                 \
    } while (0)
#define EXPECT_OK(call)                                                                                   \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        if (rc__ != 0) { std::fprintf(stderr, "%s returned %d (%s)\n", #call, rc__, nrx_last_error()); ++failures; } \
    } while (0)

int main() {
    // "device" buffers: never dereferenced by the host code under test
    float* w = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* s = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* g = static_cast<float*>(std::aligned_alloc(64, 4096));
    int64_t* keys = static_cast<int64_t*>(std::aligned_alloc(64, 4096));
    void* tabs[2] = {w, w + 512};
    float* st[2] = {s, s + 512};
    const int64_t mul[2] = {3, 1}, add[2] = {-2, 0};
    const uint32_t RW = NRX_ADAGRAD_ROWWISE, BF = NRX_ADAGRAD_TABLE_BF16;
    if (nrx_abi_version() != NRX_ABI_VERSION) ++failures;
    // counts, widths, flags
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 0, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "bad argument");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, NRX_MAX_FEATURES + 1, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "bad argument");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 0, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, 0, 0, 1, nullptr, nullptr, nullptr, nullptr), "bad argument");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, g, -1, nullptr, 0.1f, nullptr, 1e-10f, 0.f, 0, 0, 1, nullptr, nullptr, nullptr, nullptr), "bad argument");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, 4u, 0, 1, nullptr, nullptr, nullptr, nullptr), "flag");
    // row maps: both or neither, and only for bf16 tables
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW | BF, 0, 1, nullptr, mul, nullptr, nullptr), "row_mul");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, mul, add, nullptr), "bf16");
    // null buffers
    EXPECT_BAD(nrx_sparse_adagrad_step(nullptr, st, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "null buffer");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, nullptr, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "null buffer");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 16, nullptr, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, 0, 0, 1, nullptr, nullptr, nullptr, nullptr), "null buffer");
    EXPECT_BAD(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, nullptr, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, 0, 0, 1, nullptr, nullptr, nullptr, nullptr), "null buffer");
    {   // a formatted message with an integer argument: table 1 is null / misaligned
        void* bad[2] = {w, nullptr};
        EXPECT_BAD(nrx_sparse_adagrad_step(bad, st, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "table 1");
        float* bads[2] = {s, nullptr};
        EXPECT_BAD(nrx_sparse_adagrad_step(tabs, bads, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "table 1");
        void* odd[2] = {w, reinterpret_cast<char*>(w) + 2};      // a 2-byte aligned table is fine for bf16 rows, not for fp32 ones
        EXPECT_BAD(nrx_sparse_adagrad_step(odd, st, 2, 16, keys, g, 4, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr), "misaligned");
    }
    // an empty list has nothing to launch -- in every mode, with NRX_MAX_FEATURES tables' worth of maps read from the caller's arrays
    EXPECT_OK(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, g, 0, nullptr, 0.1f, nullptr, 1e-10f, 0.f, 0, 0, 1, nullptr, nullptr, nullptr, nullptr));
    EXPECT_OK(nrx_sparse_adagrad_step(tabs, st, 2, 16, keys, g, 0, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW | BF, 7, 1, nullptr, mul, add, nullptr));
    EXPECT_OK(nrx_sparse_adagrad_step(nullptr, nullptr, 1, 1, nullptr, nullptr, 0, nullptr, 0.1f, nullptr, 1e-10f, 0.f, RW, 0, 1, nullptr, nullptr, nullptr, nullptr));
    std::free(w); std::free(s); std::free(g); std::free(keys);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("nrx_sparse_adagrad_step validation sanitize driver: OK");
    return 0;
}
