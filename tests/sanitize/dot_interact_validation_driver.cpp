// ASan + UBSan run of the HOST half of nrx_dot_interact_fwd and nrx_dot_interact_bwd (include/nrx_embed.h): their argument validation, status
// codes and error text, compiled from the library's own sources with host-side sanitizers (hipcc -fsanitize=address,undefined
// -fno-gpu-sanitize; the device code is not instrumented and never runs: every call below fails validation BEFORE any launch, or has nothing to
// do).  The field offsets are the one HOST array the entry points read: the arrays below are exactly n_fields long, so a read past one is
// an ASan report.  No GPU needed.  Built by tests/sanitize/dot_interact.mk and run by tests/test_dot_interact_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nrx_embed.h"

static int failures = 0;
#define EXPECT_RC(call, want, fn, word)                                                                   \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        const char* e__ = nrx_last_error();                                                               \
        if (rc__ != (want) || e__ == nullptr || std::strstr(e__, fn) == nullptr || std::strstr(e__, word) == nullptr) { \
            std::fprintf(stderr, "expected %d naming '%s' and '%s' from %s, got %d (%s)\n", (want), fn, word, #call, rc__, e__ ? e__ : ""); \
            ++failures;                                                                                   \
        }                                                                                                 \
    } while (0)
#define EXPECT_BAD(call, fn, word) EXPECT_RC(call, NRX_ERR_BAD_ARG, fn, word)
#define EXPECT_UNSUPPORTED(call, fn) EXPECT_RC(call, NRX_ERR_UNSUPPORTED, fn, "supports")
#define EXPECT_OK(call)                                                                                   \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        if (rc__ != 0) { std::fprintf(stderr, "%s returned %d (%s)\n", #call, rc__, nrx_last_error()); ++failures; } \
    } while (0)

template <typename T>
static T* off(T* p, int bytes) { return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + bytes); }

// adjacent fields, the array exactly n long (heap: a read past it is caught)
static std::vector<int32_t> adjacent(int n, int dim) {
    std::vector<int32_t> o(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) o[i] = i * dim;
    return o;
}

int main() {
    // "device" buffers: never dereferenced by the host code under test
    float* x = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* z = static_cast<float*>(std::aligned_alloc(64, 4096));
    float* gx = static_cast<float*>(std::aligned_alloc(64, 4096));
    if (nrx_abi_version() != NRX_ABI_VERSION) ++failures;
    const char* FW = "nrx_dot_interact_fwd";
    const char* BW = "nrx_dot_interact_bwd";
    const std::vector<int32_t> o3 = adjacent(3, 16);                    // 3 fields of 16 in rows of 48: P = 3 (6 with the diagonal)

#define FWD(x_, ld_, fo_, nf_, dim_, b_, fl_, z_, zld_) nrx_dot_interact_fwd(x_, ld_, fo_, nf_, dim_, b_, fl_, z_, zld_, nullptr)
#define BWD(x_, ld_, fo_, nf_, dim_, b_, fl_, gz_, gzld_, gx_, gxld_, acc_) \
    nrx_dot_interact_bwd(x_, ld_, fo_, nf_, dim_, b_, fl_, gz_, gzld_, gx_, gxld_, acc_, nullptr)
    EXPECT_BAD(FWD(x, 48, o3.data(), 0, 16, 5, 0, z, 3), FW, "n_fields");
    EXPECT_BAD(FWD(x, 48, o3.data(), -2, 16, 5, 0, z, 3), FW, "n_fields");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 0, 5, 0, z, 3), FW, "dim");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, -1, 0, z, 3), FW, "batch");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, 5, 2, z, 3), FW, "flags");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, 5, -1, z, 3), FW, "flags");
    EXPECT_BAD(FWD(x, 48, nullptr, 3, 16, 5, 0, z, 3), FW, "field_off");
    EXPECT_BAD(FWD(x, 46, o3.data(), 3, 16, 5, 0, z, 3), FW, "ld");
    EXPECT_BAD(FWD(x, 12, o3.data(), 3, 16, 5, 0, z, 3), FW, "ld");
    EXPECT_BAD(FWD(x, 44, o3.data(), 3, 16, 5, 0, z, 3), FW, "field_off[2]");             // the last field leaves the row
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, 5, 0, z, 2), FW, "z_ld");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, 5, NRX_DOT_SELF, z, 5), FW, "z_ld");
    EXPECT_BAD(FWD(nullptr, 48, o3.data(), 3, 16, 5, 0, z, 3), FW, "null buffer");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, 5, 0, nullptr, 3), FW, "null buffer");
    EXPECT_BAD(FWD(off(x, 8), 48, o3.data(), 3, 16, 5, 0, z, 3), FW, "misaligned x");
    EXPECT_BAD(FWD(x, 48, o3.data(), 3, 16, 5, 0, off(z, 2), 3), FW, "misaligned z");
    {
        const std::vector<int32_t> o = {0, 18, 36};
        EXPECT_BAD(FWD(x, 64, o.data(), 3, 16, 5, 0, z, 3), FW, "field_off[1]");          // not a multiple of 4
    }
    {
        const std::vector<int32_t> o = {0, -4, 32};
        EXPECT_BAD(FWD(x, 64, o.data(), 3, 16, 5, 0, z, 3), FW, "field_off[1]");
    }
    {
        const std::vector<int32_t> o = {32, 0, 12};
        EXPECT_BAD(FWD(x, 64, o.data(), 3, 16, 5, 0, z, 3), FW, "overlap");
        EXPECT_BAD(BWD(x, 64, o.data(), 3, 16, 5, 0, z, 3, gx, 64, 0), BW, "overlap");
    }
    {
        const std::vector<int32_t> o = {16, 16};
        EXPECT_BAD(FWD(x, 64, o.data(), 2, 16, 5, 0, z, 1), FW, "overlap");
    }
    // z inside the rows of x (the in-place cat form): past the fields it is fine (nothing to launch at batch 0 -- the check needs batch > 0,
    // so the refusals are exercised and the accepted form is left to the GPU tests), on a field or leaving the row it is refused
    EXPECT_BAD(FWD(x, 52, o3.data(), 3, 16, 5, 0, x + 44, 52), FW, "overlaps field");
    EXPECT_BAD(FWD(x, 52, o3.data(), 3, 16, 5, 0, x + 50, 52), FW, "leaves");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, gx + 44, 52, gx, 52, 1), BW, "overlaps field");

    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, z, 3, gx, 48, 2), BW, "accumulate");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, z, 3, gx, 48, -1), BW, "accumulate");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, z, 2, gx, 48, 0), BW, "gz_ld");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, z, 3, gx, 47, 0), BW, "gx_ld");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, nullptr, 3, gx, 48, 0), BW, "null buffer");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, z, 3, nullptr, 48, 0), BW, "null buffer");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, off(z, 1), 3, gx, 48, 0), BW, "misaligned g_z");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 0, z, 3, off(gx, 2), 48, 0), BW, "misaligned g_x");
    EXPECT_BAD(BWD(x, 48, o3.data(), 3, 16, 5, 4, z, 3, gx, 48, 0), BW, "flags");
    EXPECT_BAD(BWD(x, 48, nullptr, 3, 16, 5, 0, z, 3, gx, 48, 0), BW, "field_off");

    // valid form, unsupported shape: 1 field, 65 fields, dim 6 / 2 / 68
    {
        const std::vector<int32_t> o1 = adjacent(1, 16), o65 = adjacent(65, 4), o6 = {0, 8}, o68 = adjacent(2, 68);
        EXPECT_UNSUPPORTED(FWD(x, 16, o1.data(), 1, 16, 5, 0, z, 0), FW);
        EXPECT_UNSUPPORTED(FWD(x, 260, o65.data(), 65, 4, 5, 0, z, 2080), FW);
        EXPECT_UNSUPPORTED(FWD(x, 16, o6.data(), 2, 6, 5, 0, z, 1), FW);
        EXPECT_UNSUPPORTED(FWD(x, 16, o6.data(), 2, 2, 5, 0, z, 1), FW);
        EXPECT_UNSUPPORTED(FWD(x, 136, o68.data(), 2, 68, 5, 0, z, 1), FW);
        EXPECT_UNSUPPORTED(BWD(x, 16, o1.data(), 1, 16, 5, 0, z, 0, gx, 16, 0), BW);
        EXPECT_UNSUPPORTED(BWD(x, 260, o65.data(), 65, 4, 5, 0, z, 2080, gx, 260, 1), BW);
        EXPECT_UNSUPPORTED(BWD(x, 136, o68.data(), 2, 68, 5, 0, z, 1, gx, 136, 0), BW);
    }
    // ... an empty batch has nothing to launch, whatever the pointers; the largest supported field count is read to its end and no further
    {
        const std::vector<int32_t> o64 = adjacent(64, 64);
        EXPECT_OK(FWD(nullptr, 4096, o64.data(), 64, 64, 0, NRX_DOT_SELF, nullptr, 2080));
        EXPECT_OK(BWD(nullptr, 4096, o64.data(), 64, 64, 0, NRX_DOT_SELF, nullptr, 2080, nullptr, 4096, 1));
        EXPECT_OK(FWD(nullptr, 48, o3.data(), 3, 16, 0, 0, nullptr, 3));
    }

    std::free(x); std::free(z); std::free(gx);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("nrx_dot_interact validation sanitize driver: OK");
    return 0;
}
