// ASan + UBSan run of the HOST half of nrx_itemcf_similarity, nrx_itemcf_recall_workspace and nrx_itemcf_recall (include/nrx_embed.h): their
// argument validation, status codes and error text, compiled from the library's own sources with host-side sanitizers (hipcc
// -fsanitize=address,undefined -fno-gpu-sanitize; the device code is not instrumented and never runs: every call below fails validation BEFORE any
// launch, or has nothing to do).  No GPU needed.  Built by tests/sanitize/itemcf.mk and run by tests/test_itemcf.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nrx_embed.h"

static int failures = 0;
#define EXPECT_BAD(call, fn, word)                                                                        \
    do {                                                                                                  \
        const int rc__ = (call);                                                                          \
        const char* e__ = nrx_last_error();                                                               \
        if (rc__ != NRX_ERR_BAD_ARG || e__ == nullptr || std::strstr(e__, fn) == nullptr || std::strstr(e__, word) == nullptr) { \
            std::fprintf(stderr, "expected -1 naming '%s' and '%s' from %s, got %d (%s)\n", fn, word, #call, rc__, e__ ? e__ : ""); \
            ++failures;                                                                                   \
        }                                                                                                 \
    } while (0)
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
    int64_t* uoff = static_cast<int64_t*>(std::aligned_alloc(64, 256));
    int64_t* ioff = static_cast<int64_t*>(std::aligned_alloc(64, 256));
    int64_t* items = static_cast<int64_t*>(std::aligned_alloc(64, 256));
    int64_t* users = static_cast<int64_t*>(std::aligned_alloc(64, 256));
    float* sim = static_cast<float*>(std::aligned_alloc(64, 4096));
    int32_t* co = static_cast<int32_t*>(std::aligned_alloc(64, 4096));
    int64_t* oidx = static_cast<int64_t*>(std::aligned_alloc(64, 4096));
    float* osc = static_cast<float*>(std::aligned_alloc(64, 4096));
    void* ws = std::aligned_alloc(64, 4096);
    if (nrx_abi_version() != NRX_ABI_VERSION) ++failures;

#define SIM(uo_, it_, nu_, io_, us_, ni_, bits_, tile_, sim_, co_) \
    nrx_itemcf_similarity(uo_, it_, nu_, io_, us_, ni_, bits_, tile_, sim_, co_, nullptr, nullptr)
    const char* S = "nrx_itemcf_similarity";
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 0, 64, 0, sim, co), S, "n_items");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, -5, 64, 0, sim, co), S, "n_items");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 0x7fffffffLL, 64, 0, sim, co), S, "n_items");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 1LL << 40, 64, 0, sim, co), S, "n_items");
    EXPECT_BAD(SIM(uoff, items, -1, ioff, users, 8, 64, 0, sim, co), S, "n_users");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 16, 0, sim, co), S, "index_bits");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 0, 0, sim, co), S, "index_bits");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 64, -1, sim, co), S, "col_tile");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 64, 16385, sim, co), S, "col_tile");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 0x7ffffff0LL, 64, 64, sim, co), S, "col_tile");          // more than 65535 tiles
    EXPECT_BAD(SIM(nullptr, items, 4, ioff, users, 8, 64, 0, sim, co), S, "null buffer");
    EXPECT_BAD(SIM(uoff, nullptr, 4, ioff, users, 8, 64, 0, sim, co), S, "null buffer");
    EXPECT_BAD(SIM(uoff, items, 4, nullptr, users, 8, 64, 0, sim, co), S, "null buffer");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, nullptr, 8, 64, 0, sim, co), S, "null buffer");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 64, 0, nullptr, co), S, "null buffer");
    EXPECT_BAD(SIM(off(uoff, 4), items, 4, ioff, users, 8, 64, 0, sim, co), S, "misaligned pointer");
    EXPECT_BAD(SIM(uoff, off(items, 4), 4, ioff, users, 8, 64, 0, sim, co), S, "misaligned pointer");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, off(users, 2), 8, 32, 0, sim, co), S, "misaligned pointer");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 64, 0, off(sim, 2), co), S, "misaligned pointer");
    EXPECT_BAD(SIM(uoff, items, 4, ioff, users, 8, 64, 0, sim, off(co, 1)), S, "misaligned pointer");

    // the size call: -1 for anything the entry point refuses; one K-entry list per (query, split); no overflow at the largest sizes
    EXPECT_TRUE(nrx_itemcf_recall_workspace(100, 7, 10, 3) >= 3 * 7 * 10 * 8);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(100, 7, 32, 1) >= 7 * 32 * 8);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(2, 7, 1, 3) >= 2 * 7 * 4 * 8);                               // never more splits than items
    EXPECT_TRUE(nrx_itemcf_recall_workspace(100, 0, 10, 0) >= 0);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(0, 7, 10, 0) == -1 && nrx_itemcf_recall_workspace(100, -1, 10, 0) == -1);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(100, 7, 0, 0) == -1 && nrx_itemcf_recall_workspace(100, 7, 33, 0) == -1);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(100, 7, 10, -1) == -1 && nrx_itemcf_recall_workspace(100, 7, 10, 1025) == -1);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(0x7fffffffLL, 7, 10, 0) == -1 && nrx_itemcf_recall_workspace(100, 0x7fffffffLL, 10, 0) == -1);
    EXPECT_TRUE(nrx_itemcf_recall_workspace(0x7ffffffeLL, 0x7ffffffeLL, 32, 1024) > 0);

#define REC(sim_, ni_, ho_, hi_, eo_, ei_, bits_, nq_, k_, sp_, oi_, os_, ws_) \
    nrx_itemcf_recall(sim_, ni_, ho_, hi_, eo_, ei_, bits_, nq_, k_, sp_, oi_, os_, ws_, nullptr)
    const char* R = "nrx_itemcf_recall";
    EXPECT_BAD(REC(sim, 0, uoff, items, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "n_items");
    EXPECT_BAD(REC(sim, 0x7fffffffLL, uoff, items, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "n_items");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, -1, 10, 0, oidx, osc, ws), R, "n_queries");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 0, 0, oidx, osc, ws), R, "k must");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, -3, 0, oidx, osc, ws), R, "k must");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 33, 0, oidx, osc, ws), R, "k must");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 8, 4, 10, 0, oidx, osc, ws), R, "index_bits");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, -1, oidx, osc, ws), R, "col_splits");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, 1025, oidx, osc, ws), R, "col_splits");
    EXPECT_BAD(REC(nullptr, 8, uoff, items, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, nullptr, items, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, uoff, nullptr, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, uoff, items, nullptr, users, 64, 4, 10, 0, oidx, osc, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, nullptr, 64, 4, 10, 0, oidx, osc, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, 0, nullptr, osc, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, 0, oidx, nullptr, ws), R, "null buffer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, 0, oidx, osc, nullptr), R, "null buffer");
    EXPECT_BAD(REC(off(sim, 2), 8, uoff, items, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "misaligned pointer");
    EXPECT_BAD(REC(sim, 8, off(uoff, 4), items, ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "misaligned pointer");
    EXPECT_BAD(REC(sim, 8, uoff, off(items, 4), ioff, users, 64, 4, 10, 0, oidx, osc, ws), R, "misaligned pointer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, off(users, 2), 32, 4, 10, 0, oidx, osc, ws), R, "misaligned pointer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, 0, off(oidx, 4), osc, ws), R, "misaligned pointer");
    EXPECT_BAD(REC(sim, 8, uoff, items, ioff, users, 64, 4, 10, 0, oidx, off(osc, 1), ws), R, "misaligned pointer");
    // ... no query has nothing to launch, whatever the pointers
    EXPECT_OK(REC(nullptr, 8, nullptr, nullptr, nullptr, nullptr, 32, 0, 10, 0, nullptr, nullptr, nullptr));
    EXPECT_OK(REC(sim, 8, uoff, items, ioff, users, 64, 0, 32, 3, oidx, osc, ws));

    std::free(uoff); std::free(ioff); std::free(items); std::free(users); std::free(sim); std::free(co); std::free(oidx); std::free(osc); std::free(ws);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("nrx_itemcf validation sanitize driver: OK");
    return 0;
}
