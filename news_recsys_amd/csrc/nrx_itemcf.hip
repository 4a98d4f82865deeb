// Item-based collaborative filtering (the reference's recall/ItemCF/itemCF_base.py): co-occurrence similarity and top-k recall.
// Reference: src/model/recall/ItemCF/itemCF_base.py:18-58 (dict-of-dict loops over every pair of items of every user's history).
//
// Similarity -- row owner, counts in LDS.  One workgroup owns (item i, column tile t), zeroes tile_len int32 counters in LDS, walks the
// users of i (from the CSC; a wave takes 64 users, finds each one's part of the tile by lower bounds with a lane per user, then goes
// through the parts with lanes over items), and for every item j of such a user that falls in the tile does one integer LDS atomic
// add.  Then the tile is normalised and the row segment stored with streaming stores (16 bytes per lane where the rows are aligned).
// Sum_u L_u^2 LDS adds, no global atomics, no I x I integer matrix unless the caller asks for the counts.  The counts are integers, so
// the result is the same bits whatever the order of users, lanes or workgroups:
//     n_i = item_off[i+1] - item_off[i];   c_ij = #users holding both (c_ii written as 0);
//     sim_ij = c_ij == 0 ? 0 : (float)((double)c_ij / sqrt((double)n_i * (double)n_j)).
//
// Recall -- grid over (query, column split); the threads of a block own columns, the L rows of the history are read coalesced:
//     s = 0; for i in hist (ascending): s = s + sim[i][j]           (plain fp32 adds in that order: no fma, nothing reassociated)
// candidates: s > 0 and j not in the exclusion list.  Every thread keeps a sorted top-k of its columns in registers, the block pops the k
// best heads one by one, and a second kernel merges the splits.  Order: (score desc, index asc), a total order, so the result does not
// depend on the split; missing slots are -1 / -FLT_MAX (as nrx_topk_ip).  No float atomics anywhere in this unit.
#include "nrx_common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int KMAX = 32;
constexpr int TILE_MAX = 16384;           // 64 KiB of int32 counters
constexpr int SIM_BLOCK = 1024;           // 16 waves walk the users of one item (with 64 KiB tiles two workgroups fill a CU's 32 wave slots)
constexpr int REC_WAVES = NRX_BLOCK / 64;
constexpr int MAX_SPLITS = 1024;

template <bool I64>
__device__ __forceinline__ int64_t load_id(const void* p, int64_t i) {
    return I64 ? reinterpret_cast<const int64_t*>(p)[i] : (int64_t)reinterpret_cast<const int32_t*>(p)[i];
}

// first position in [lo, hi) of the ascending list whose value is >= v
template <bool I64>
__device__ __forceinline__ int64_t lower_bound(const void* lst, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (load_id<I64>(lst, mid) < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), j);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// VEC: rows of the tile start 16-byte aligned in sim and co (n_items % 4 == 0, tile % 4 == 0, aligned bases): four columns per lane and store
template <bool I64, bool VEC>
__global__ __launch_bounds__(SIM_BLOCK) void itemcf_sim_kernel(const int64_t* __restrict__ user_off, const void* __restrict__ items, int64_t n_users,
                                                               const int64_t* __restrict__ item_off, const void* __restrict__ users, int64_t n_items,
                                                               int tile, float* __restrict__ sim, int32_t* __restrict__ co) {
    extern __shared__ __attribute__((aligned(16))) int cnt[];           // tile rounded up to 4 counters
    using i32x4 = __attribute__((ext_vector_type(4))) int;
    const int64_t i = blockIdx.x;
    const int64_t t0 = (int64_t)blockIdx.y * tile;
    const int len = (int)(n_items - t0 < tile ? n_items - t0 : tile);
    const int len4 = (len + 3) >> 2;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < len4; c += SIM_BLOCK) reinterpret_cast<i32x4*>(cnt)[c] = i32x4{0, 0, 0, 0};
    __syncthreads();
    // The users of item i, SIM_BLOCK at a time, dealt to the waves round-robin (a workgroup holds its LDS for as long as its walk's chain of
    // dependent loads lasts, so the few users of an ordinary item are spread over all the waves).  First every LANE takes one user and
    // finds the part [lo, lo + n) of that user's ascending list that falls in the tile; then the wave goes through its parts, lanes over
    // items, four users' loads in flight.
    constexpr int WAVES = SIM_BLOCK / 64;
    const int64_t p0 = item_off[i], p1 = item_off[i + 1];
    for (int64_t pb = p0; pb < p1; pb += SIM_BLOCK) {
        int64_t lo = 0;
        int n = 0;
        const int64_t p = pb + (int64_t)lane * WAVES + wid;
        if (p < p1) {
            const int64_t u = load_id<I64>(users, p);
            if (u >= 0 && u < n_users) {                          // (a malformed CSC: never an address)
                const int64_t a = user_off[u], b = user_off[u + 1];
                // (a list of at most 64 items is one load per lane either way: the tile test below filters it, no dependent searches)
                const bool whole = b - a <= 64;
                lo = t0 == 0 || whole ? a : lower_bound<I64>(items, a, b, t0);
                const int64_t hi = t0 + len >= n_items || whole ? b : lower_bound<I64>(items, lo, b, t0 + len);
                n = (int)(hi - lo);
            }
        }
        const int64_t mine = (p1 - pb - wid + WAVES - 1) / WAVES;   // lanes of this wave that hold a user (may be <= 0)
        const int nb = (int)(mine < 64 ? mine : 64);
        for (int j = 0; j < nb; j += 4) {                         // lanes past nb hold n = 0
            int64_t lo_j[4];
            int n_j[4];
            uint32_t c[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                lo_j[a] = readlane64(lo, j + a);
                n_j[a] = __builtin_amdgcn_readlane(n, j + a);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) c[a] = lane < n_j[a] ? (uint32_t)(load_id<I64>(items, lo_j[a] + lane) - t0) : 0xffffffffu;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (c[a] < (uint32_t)len) atomicAdd(&cnt[c[a]], 1);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                for (int q = 64 + lane; q < n_j[a]; q += 64) {    // the rest of a list longer than the wave
                    const uint32_t cc = (uint32_t)(load_id<I64>(items, lo_j[a] + q) - t0);
                    if (cc < (uint32_t)len) atomicAdd(&cnt[cc], 1);
                }
        }
    }
    __syncthreads();
    const double n_i = (double)(p1 - p0);
    float* const srow = sim + i * n_items + t0;
    int32_t* const crow = co ? co + i * n_items + t0 : nullptr;
    auto value = [&](int c, int cij) {
        if (cij == 0) return 0.f;
        const double n_j = (double)(item_off[t0 + c + 1] - item_off[t0 + c]);
        return (float)((double)cij / sqrt(n_i * n_j));
    };
    if (VEC) {
        for (int c4 = threadIdx.x; c4 < len4; c4 += SIM_BLOCK) {  // len % 4 == 0 here
            i32x4 k = reinterpret_cast<const i32x4*>(cnt)[c4];
            const int c = 4 * c4;
            if ((uint64_t)(i - t0 - c) < 4u) k[(int)(i - t0 - c)] = 0;
            nrx_f32x4 s;
            s.x = value(c, k.x); s.y = value(c + 1, k.y); s.z = value(c + 2, k.z); s.w = value(c + 3, k.w);
            __builtin_nontemporal_store(s, reinterpret_cast<nrx_f32x4*>(srow) + c4);
            if (crow) __builtin_nontemporal_store(k, reinterpret_cast<i32x4*>(crow) + c4);
        }
    } else {
        for (int c = threadIdx.x; c < len; c += SIM_BLOCK) {
            const int cij = t0 + c == i ? 0 : cnt[c];
            __builtin_nontemporal_store(value(c, cij), srow + c);
            if (crow) __builtin_nontemporal_store(cij, crow + c);
        }
    }
}

__device__ __forceinline__ bool before(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

// insert into a list sorted by (score desc, index asc), kept in registers (static indexing only)
template <int K>
__device__ __forceinline__ void topk_insert(float (&s)[K], int (&ix)[K], float score, int idx) {
    float cs = score;
    int ci = idx;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool take = before(cs, ci, s[j], ix[j]);
        const float ts = s[j];
        const int ti = ix[j];
        s[j] = take ? cs : ts;
        ix[j] = take ? ci : ti;
        cs = take ? ts : cs;
        ci = take ? ti : ci;
    }
}

template <int K, bool I64>
__global__ __launch_bounds__(NRX_BLOCK) void itemcf_recall_kernel(const float* __restrict__ sim, int64_t n_items, const int64_t* __restrict__ hist_off,
                                                                  const void* __restrict__ hist_items, const int64_t* __restrict__ excl_off,
                                                                  const void* __restrict__ excl_items, int k, int64_t per_split,
                                                                  float* __restrict__ p_score, int* __restrict__ p_idx) {
    constexpr int UN = 4, HU = 4;                              // columns per thread, history rows per step
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t begin = (int64_t)blockIdx.y * per_split;
    const int64_t end = begin + per_split < n_items ? begin + per_split : n_items;
    const int64_t h0 = hist_off[q], h1 = hist_off[q + 1];
    const int64_t e0 = excl_off[q], e1 = excl_off[q + 1];

    float bs[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bs[j] = -FLT_MAX; bi[j] = -1; }

    for (int64_t c0 = begin + threadIdx.x; c0 < end; c0 += (int64_t)UN * NRX_BLOCK) {
        float s[UN];
        int64_t col[UN];
#pragma unroll
        for (int r = 0; r < UN; ++r) {
            s[r] = 0.f;
            const int64_t c = c0 + (int64_t)r * NRX_BLOCK;
            col[r] = c < end ? c : end - 1;                    // clamped: a value that is dropped below
        }
        // HU rows of the history at a time: HU * UN independent loads in flight per thread, then the additions in the history's order.
        // An id outside the matrix (a malformed history) never becomes an address: it reads row 0 and adds +0, which changes nothing.
        for (int64_t h = h0; h < h1; h += HU) {
            float v[HU][UN];
#pragma unroll
            for (int a = 0; a < HU; ++a) {
                const int64_t it = h + a < h1 ? load_id<I64>(hist_items, h + a) : -1;
                const bool ok = it >= 0 && it < n_items;
                const float* row = sim + (ok ? it : 0) * n_items;
#pragma unroll
                for (int r = 0; r < UN; ++r) {
                    const float t = row[col[r]];
                    v[a][r] = ok ? t : 0.f;
                }
            }
#pragma unroll
            for (int a = 0; a < HU; ++a)
#pragma unroll
                for (int r = 0; r < UN; ++r) s[r] = s[r] + v[a][r];
        }
#pragma unroll
        for (int r = 0; r < UN; ++r) {
            const int64_t c = c0 + (int64_t)r * NRX_BLOCK;
            // a thread's columns ascend, so a later one of equal score never enters before an earlier one: strict '>'
            if (c < end && s[r] > 0.f && s[r] > bs[K - 1]) {
                const int64_t e = lower_bound<I64>(excl_items, e0, e1, c);
                if (!(e < e1 && load_id<I64>(excl_items, e) == c)) topk_insert<K>(bs, bi, s[r], (int)c);
            }
        }
    }

    // the block's k best: every round takes the best head of the 256 lists and pops it where it came from (column indices are unique)
    __shared__ float w_s[2][REC_WAVES];
    __shared__ int w_i[2][REC_WAVES];
    float* const ps = p_score + (q * gridDim.y + blockIdx.y) * (int64_t)K;
    int* const pi = p_idx + (q * gridDim.y + blockIdx.y) * (int64_t)K;
#pragma unroll 1
    for (int r = 0; r < k; ++r) {
        float hs = bs[0];
        int hi = bi[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(hs, off);
            const int oi = __shfl_xor(hi, off);
            if (before(os, oi, hs, hi)) { hs = os; hi = oi; }
        }
        const int buf = r & 1;
        if (lane == 0) { w_s[buf][wid] = hs; w_i[buf][wid] = hi; }
        __syncthreads();                                       // (two buffers: round r + 1 writes the other one, round r + 2 follows a barrier)
        hs = w_s[buf][0];
        hi = w_i[buf][0];
#pragma unroll
        for (int w = 1; w < REC_WAVES; ++w)
            if (before(w_s[buf][w], w_i[buf][w], hs, hi)) { hs = w_s[buf][w]; hi = w_i[buf][w]; }
        if (hi >= 0 && bi[0] == hi) {
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) { bs[j] = bs[j + 1]; bi[j] = bi[j + 1]; }
            bs[K - 1] = -FLT_MAX;
            bi[K - 1] = -1;
        }
        if (threadIdx.x == 0) { ps[r] = hi >= 0 ? hs : -FLT_MAX; pi[r] = hi; }
    }
}

// merge the n_lists partial lists of one query (each holds k entries sorted by (score desc, index asc), -1 behind the last candidate)
template <int K>
__global__ __launch_bounds__(NRX_BLOCK) void itemcf_merge_kernel(const float* __restrict__ p_score, const int* __restrict__ p_idx, int64_t n_queries,
                                                                 int n_lists, int k, int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const int64_t qi = (int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x;
    if (qi >= n_queries) return;
    float bs[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { bs[j] = -FLT_MAX; bi[j] = -1; }
    for (int s = 0; s < n_lists; ++s) {
        const float* ps = p_score + (qi * n_lists + s) * (int64_t)K;
        const int* pi = p_idx + (qi * n_lists + s) * (int64_t)K;
        for (int j = 0; j < k; ++j) {
            const float cs = ps[j];
            const int ci = pi[j];
            if (ci < 0 || !before(cs, ci, bs[K - 1], bi[K - 1])) break;     // sorted: nothing further can enter
            topk_insert<K>(bs, bi, cs, ci);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) {
            out_idx[qi * k + j] = (int64_t)bi[j];
            out_score[qi * k + j] = bs[j];
        }
    }
}

// list length instantiated for a requested k (10 is what the reference's hit_rate asks for)
int pick_k(int k) { return k <= 4 ? 4 : (k <= 10 ? 10 : (k <= 16 ? 16 : KMAX)); }

int choose_splits(int64_t n_items, int64_t n_queries, int col_splits) {
    int64_t s = col_splits;
    if (s == 0) {
        s = n_queries > 0 ? (1024 + n_queries - 1) / n_queries : 1;         // aim at >= 1024 blocks ...
        const int64_t max_s = (n_items + 2047) / 2048;                      // ... of >= 2048 columns: two trips of the block
        if (s > max_s) s = max_s;
        if (s > 64) s = 64;
    }
    if (s > n_items) s = n_items;
    if (s < 1) s = 1;
    return (int)s;
}

bool aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace

extern "C" int nrx_itemcf_similarity(const int64_t* user_off, const void* items, int64_t n_users, const int64_t* item_off, const void* users,
                                     int64_t n_items, int32_t index_bits, int32_t col_tile, float* sim, int32_t* co, void* workspace,
                                     void* stream) {
    NRX_TRACE();
    (void)workspace;
    NRX_REQUIRE(n_items >= 1 && n_items < 0x7fffffffLL, "nrx_itemcf_similarity: n_items must be in 1..2^31-2 (got %lld)", (long long)n_items);
    NRX_REQUIRE(n_users >= 0, "nrx_itemcf_similarity: n_users must be >= 0 (got %lld)", (long long)n_users);
    NRX_REQUIRE(index_bits == 32 || index_bits == 64, "nrx_itemcf_similarity: index_bits must be 32 or 64 (got %d)", index_bits);
    NRX_REQUIRE(col_tile >= 0 && col_tile <= TILE_MAX, "nrx_itemcf_similarity: col_tile must be in 0..%d, 0 = default (got %d)", TILE_MAX, col_tile);
    NRX_REQUIRE(user_off && items && item_off && users && sim, "nrx_itemcf_similarity: null buffer (user_off, items, item_off, users, sim)");
    NRX_REQUIRE(aligned(user_off, 8) && aligned(item_off, 8) && aligned(items, index_bits / 8) && aligned(users, index_bits / 8) &&
                aligned(sim, 4) && aligned(co, 4), "nrx_itemcf_similarity: misaligned pointer");
    const int tile = col_tile > 0 ? col_tile : (int)(n_items < TILE_MAX ? n_items : TILE_MAX);
    const int64_t n_tiles = (n_items + tile - 1) / tile;
    NRX_REQUIRE(n_tiles <= 65535, "nrx_itemcf_similarity: col_tile %d cuts %lld items into more than 65535 tiles", tile, (long long)n_items);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_items, (unsigned)n_tiles);
    const size_t lds = (size_t)((tile + 3) & ~3) * sizeof(int);
    const bool vec = (n_items & 3) == 0 && (tile & 3) == 0 && nrx_aligned16(sim) && nrx_aligned16(co);
#define NRX_SIM(I64_, VEC_) hipLaunchKernelGGL((itemcf_sim_kernel<I64_, VEC_>), grid, dim3(SIM_BLOCK), lds, st, user_off, items, \
                                               n_users, item_off, users, n_items, tile, sim, co)
    if (index_bits == 64) { if (vec) NRX_SIM(true, true); else NRX_SIM(true, false); }
    else { if (vec) NRX_SIM(false, true); else NRX_SIM(false, false); }
#undef NRX_SIM
    NRX_LAUNCH_CHECK("nrx_itemcf_similarity");
    return NRX_OK;
}

extern "C" int64_t nrx_itemcf_recall_workspace(int64_t n_items, int64_t n_queries, int32_t k, int32_t col_splits) {
    if (n_items < 1 || n_items >= 0x7fffffffLL || n_queries < 0 || n_queries >= 0x7fffffffLL || k < 1 || k > KMAX || col_splits < 0 || col_splits > MAX_SPLITS) return -1;
    return (int64_t)choose_splits(n_items, n_queries, col_splits) * n_queries * pick_k(k) * (int64_t)(sizeof(float) + sizeof(int)) + 256;
}

extern "C" int nrx_itemcf_recall(const float* sim, int64_t n_items, const int64_t* hist_off, const void* hist_items, const int64_t* excl_off,
                                 const void* excl_items, int32_t index_bits, int64_t n_queries, int32_t k, int32_t col_splits,
                                 int64_t* out_idx, float* out_score, void* workspace, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n_items >= 1 && n_items < 0x7fffffffLL, "nrx_itemcf_recall: n_items must be in 1..2^31-2 (got %lld)", (long long)n_items);
    NRX_REQUIRE(n_queries >= 0 && n_queries < 0x7fffffffLL, "nrx_itemcf_recall: n_queries must be in 0..2^31-2 (got %lld)", (long long)n_queries);
    NRX_REQUIRE(k >= 1 && k <= KMAX, "nrx_itemcf_recall: k must be in 1..%d per call (got %d)", KMAX, k);
    NRX_REQUIRE(index_bits == 32 || index_bits == 64, "nrx_itemcf_recall: index_bits must be 32 or 64 (got %d)", index_bits);
    NRX_REQUIRE(col_splits >= 0 && col_splits <= MAX_SPLITS, "nrx_itemcf_recall: col_splits must be in 0..%d, 0 = chosen (got %d)", MAX_SPLITS,
                col_splits);
    if (n_queries == 0) return NRX_OK;
    NRX_REQUIRE(sim && hist_off && hist_items && excl_off && excl_items && out_idx && out_score && workspace,
                "nrx_itemcf_recall: null buffer (sim, hist_off, hist_items, excl_off, excl_items, out_idx, out_score, workspace)");
    NRX_REQUIRE(aligned(sim, 4) && aligned(hist_off, 8) && aligned(excl_off, 8) && aligned(hist_items, index_bits / 8) &&
                aligned(excl_items, index_bits / 8) && aligned(out_idx, 8) && aligned(out_score, 4), "nrx_itemcf_recall: misaligned pointer");
    const int K = pick_k(k);
    const int S = choose_splits(n_items, n_queries, col_splits);
    const int64_t per_split = (n_items + S - 1) / S;
    char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    int* p_idx = reinterpret_cast<int*>(ws);
    float* p_score = reinterpret_cast<float*>(ws + (size_t)S * n_queries * K * sizeof(int));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_queries, (unsigned)S);
    const unsigned mg = (unsigned)((n_queries + NRX_BLOCK - 1) / NRX_BLOCK);
#define NRX_CF2(K_, I64_) hipLaunchKernelGGL((itemcf_recall_kernel<K_, I64_>), grid, dim3(NRX_BLOCK), 0, st, sim, n_items, hist_off, hist_items, \
                                             excl_off, excl_items, (int)k, per_split, p_score, p_idx)
#define NRX_CF(K_)                                                                                                                              \
    do {                                                                                                                                        \
        if (index_bits == 64) NRX_CF2(K_, true); else NRX_CF2(K_, false);                                                                       \
        hipLaunchKernelGGL(itemcf_merge_kernel<K_>, dim3(mg), dim3(NRX_BLOCK), 0, st, p_score, p_idx, n_queries, S, (int)k, out_idx, out_score); \
    } while (0)
    switch (K) {
        case 4: NRX_CF(4); break;
        case 10: NRX_CF(10); break;
        case 16: NRX_CF(16); break;
        default: NRX_CF(32); break;
    }
#undef NRX_CF
#undef NRX_CF2
    NRX_LAUNCH_CHECK("nrx_itemcf_recall");
    return NRX_OK;
}
