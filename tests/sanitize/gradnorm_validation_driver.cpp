// ASan + UBSan run of the HOST half of nrx_rows_sqnorm, nrx_rows_sqnorm_finish and nrx_rows_scale (include/nrx_embed.h): their argument validation,
// status codes and error text, compiled from the library's own sources with host-side sanitizers (hipcc -fsanitize=address,undefined
// -fno-gpu-sanitize; the device code is not instrumented and never runs: every call below fails validation BEFORE any launch, or has nothing to
// do).  No GPU needed.  Built by tests/sanitize/gradnorm.mk and run by tests/test_grad_clip.py.
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
    float* g = static_cast<float*>(std::aligned_alloc(64, 4096));
    int64_t* keys = static_cast<int64_t*>(std::aligned_alloc(64, 4096));
    uint64_t* bins = static_cast<uint64_t*>(std::aligned_alloc(64, 4096));
    double* norm = static_cast<double*>(std::aligned_alloc(64, 64));
    float* coef = static_cast<float*>(std::aligned_alloc(64, 64));
    if (nrx_abi_version() != NRX_ABI_VERSION) ++failures;
    // nrx_rows_sqnorm: counts and widths
    EXPECT_BAD(nrx_rows_sqnorm(keys, g, 4, nullptr, 0, 16, 0, bins, nullptr), "bad argument");
    EXPECT_BAD(nrx_rows_sqnorm(keys, g, 4, nullptr, NRX_MAX_FEATURES + 1, 16, 0, bins, nullptr), "bad argument");
    EXPECT_BAD(nrx_rows_sqnorm(keys, g, 4, nullptr, 2, 0, 0, bins, nullptr), "bad argument");
    EXPECT_BAD(nrx_rows_sqnorm(keys, g, -1, nullptr, 2, 16, 0, bins, nullptr), "bad argument");
    // ... null and misaligned buffers
    EXPECT_BAD(nrx_rows_sqnorm(nullptr, g, 4, nullptr, 2, 16, 0, bins, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_sqnorm(keys, nullptr, 4, nullptr, 2, 16, 0, bins, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_sqnorm(keys, g, 4, nullptr, 2, 16, ~0ull, nullptr, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_sqnorm(keys, reinterpret_cast<float*>(reinterpret_cast<char*>(g) + 2), 4, nullptr, 2, 16, 0, bins, nullptr), "misaligned");
    EXPECT_BAD(nrx_rows_sqnorm(keys, g, 4, nullptr, 2, 16, 0, reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(bins) + 4), nullptr), "misaligned");
    // ... an empty list has nothing to launch
    EXPECT_OK(nrx_rows_sqnorm(keys, g, 0, nullptr, NRX_MAX_FEATURES, 1, ~0ull, bins, nullptr));
    EXPECT_OK(nrx_rows_sqnorm(nullptr, nullptr, 0, nullptr, 1, 320, 0, nullptr, nullptr));
    // nrx_rows_sqnorm_finish: the bound must be positive (a NaN is not), the three buffers present and aligned
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, nullptr, 0.0, norm, coef, 1, nullptr), "max_norm");
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, nullptr, -1.0, norm, coef, 1, nullptr), "max_norm");
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, nullptr, std::strtod("nan", nullptr), norm, coef, 0, nullptr), "max_norm");
    EXPECT_BAD(nrx_rows_sqnorm_finish(nullptr, nullptr, 1.0, norm, coef, 1, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, nullptr, 1.0, nullptr, coef, 1, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, nullptr, 1.0, norm, nullptr, 1, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, reinterpret_cast<double*>(reinterpret_cast<char*>(norm) + 4), 1.0, norm, coef, 1, nullptr), "misaligned");
    EXPECT_BAD(nrx_rows_sqnorm_finish(bins, nullptr, 1.0, reinterpret_cast<double*>(reinterpret_cast<char*>(norm) + 4), coef, 1, nullptr), "misaligned");
    // nrx_rows_scale
    EXPECT_BAD(nrx_rows_scale(g, 4, 0, coef, nullptr), "bad argument");
    EXPECT_BAD(nrx_rows_scale(g, -1, 16, coef, nullptr), "bad argument");
    EXPECT_BAD(nrx_rows_scale(nullptr, 4, 16, coef, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_scale(g, 4, 16, nullptr, nullptr), "null buffer");
    EXPECT_BAD(nrx_rows_scale(reinterpret_cast<float*>(reinterpret_cast<char*>(g) + 1), 4, 16, coef, nullptr), "misaligned");
    EXPECT_OK(nrx_rows_scale(g, 0, 16, coef, nullptr));
    EXPECT_OK(nrx_rows_scale(nullptr, 0, 1, nullptr, nullptr));
    std::free(g); std::free(keys); std::free(bins); std::free(norm); std::free(coef);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("nrx_rows_sqnorm validation sanitize driver: OK");
    return 0;
}
