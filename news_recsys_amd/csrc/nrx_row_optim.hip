// The row-list kernels: each takes the (key, row) list the sorted backward produced -- key = (table << 40) | row, one per unique row, values
// [n, dim] -- and updates tables from it: the fused row-sparse Adam(W) and Adagrad steps (fp32 and bf16 tables), the dense gradient tables
// (nrx_rows_to_dense), the slot maps (nrx_rows_mark, nrx_rows_merge) and the exact dense AdamW that reads them (nrx_dense_adamw_rows).
// What they share is written once: the list walk (RowGroup), the weight load / store of either table format (row_load_w*, row_store_w*),
// the rounding hash of a row (sr_step_hash, sr_row_hash) and the launch shape (RowLaunch, dispatch_qlog2).
#include "nrx_common.h"
#include <cmath>
#include <cstring>
#include <type_traits>

namespace {

// ---- the list walk ---------------------------------------------------------------------------------
// The list's length: the host's bound, clamped by the count the planner left on the device (optional).
__device__ __forceinline__ int64_t row_list_len(int64_t max_n, const int64_t* n_dev) {
    int64_t n = max_n;
    if (n_dev != nullptr) {
        const int64_t nd = nrx_gconst<int64_t>(n_dev)[0];
        n = nd < n ? nd : n;
    }
    return n;
}

__device__ __forceinline__ void split_key(int64_t key, int64_t& t, int64_t& row) {
    t = key >> 40;
    row = key & ((1ll << 40) - 1);
}

// One lane group (Q = 2^QLOG2 lanes) walks R = 4 consecutive list entries: key loads, then 4 R independent row loads are in flight.
// Entry r is `on` unless its key is a filler (negative: the tail of the list, a pair nrx_rows_merge consumed), names a table the call
// does not have, or (SKIP_ROW0: the optimizers) names the padding row, which never trains.  An entry that is off reads table 0, row 0
// and the group's first value row -- valid addresses -- and writes nothing.
// A kernel calls begin(), then load_key(r) for every r, then entry(r) for every r, forming its own pointers from tc and rc.  (The two steps
// are per entry and the loops over r stay in the kernels: a walker step with a loop inside moves instructions of the pinned kernels.)
template <int QLOG2, bool SKIP_ROW0>
struct RowGroup {
    static constexpr int Q = 1 << QLOG2, TB = NRX_BLOCK / Q, R = 4;
    int64_t n, u0;              // the list's length, the group's first entry
    int64_t key[R];
    bool on[R];

    // false: the whole lane group lies behind the end of the list (and leaves)
    __device__ __forceinline__ bool begin(int64_t max_n, const int64_t* n_dev) {
        n = row_list_len(max_n, n_dev);
        u0 = ((int64_t)blockIdx.x * TB + (threadIdx.x >> QLOG2)) * R;
        return u0 < n;
    }
    __device__ __forceinline__ void load_key(int r, const int64_t* keys) { key[r] = u0 + r < n ? nrx_gconst<int64_t>(keys)[u0 + r] : -1; }
    // Sets on[r]; tc, rc: the table and the row of entry u0 + r ({0, 0} when it is off), from which the kernel forms its own pointers.
    // (n_tables points into the kernarg segment: it is read only for keys that are no fillers)
    __device__ __forceinline__ void entry(int r, const NRX_CONST int32_t* n_tables, int64_t& tc, int64_t& rc) {
        int64_t t, row;
        split_key(key[r], t, row);
        on[r] = key[r] >= 0 && (!SKIP_ROW0 || row != 0) && t < *n_tables;
        tc = on[r] ? t : 0;
        rc = on[r] ? row : 0;
    }
    __device__ __forceinline__ const float* values(const float* base, int r, int D) const { return base + (u0 + (on[r] ? r : 0)) * (int64_t)D; }
};

// ---- weights of fp32 and bf16 tables -----------------------------------------------------------------
// bf16 tables: the stored weight is widened, the update runs in fp32, and the new weight is rounded to bf16 stochastically with 16 bits
// of a stateless counter hash of (seed, step, table, row, column) -- the definition is in nrx_embed.h.  The row the hash sees is
// key row * row_mul[t] + row_add[t] where a call carries row maps: a row-sharded arena names a row by its local index, the rounding
// stream by the global one.
__device__ __forceinline__ uint64_t sr_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// The hash is a chain, each link mixing the next counter into the hash so far: seed -> step -> table -> row -> column.
__device__ __forceinline__ uint64_t sr_link(uint64_t h, uint64_t counter) { return sr_mix(h ^ counter); }
__device__ __forceinline__ uint64_t sr_step_hash(uint64_t seed, uint64_t step) { return sr_link(sr_mix(seed), step); }
__device__ __forceinline__ uint64_t sr_row_hash(uint64_t h_table, int64_t hashed_row) { return sr_link(h_table, (uint64_t)hashed_row); }
__device__ __forceinline__ uint16_t sr_bf16(float w, uint64_t h_row, int64_t col) {
    const uint32_t u = __builtin_bit_cast(uint32_t, w);
    if ((u & 0x7F800000u) == 0x7F800000u) return __builtin_bit_cast(uint16_t, static_cast<__bf16>(w));   // inf / NaN: plain cast
    const uint32_t r = (uint32_t)(sr_link(h_row, (uint64_t)col) >> 48);
    return (uint16_t)((u + r) >> 16);
}

// Columns k .. k + 3 (row_*_w4: k % 4 == 0; 16-byte aligned fp32 rows, 8-byte aligned bf16 ones) or column k of a row.
template <bool BF16>
__device__ __forceinline__ float4 row_load_w4(const void* row, int k) {
    if (BF16) {
        const uint2 wb = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(row) + k);
        return nrx_bf16x4_to_f32(wb.x, wb.y);
    }
    return nrx_ldg4(reinterpret_cast<const float*>(row) + k, 0);
}
// The same load for a kernel that keeps many rows in flight (Adam: four arrays of R): the four bf16 weights stay packed in their two
// dwords until row_widen_w4 at the point of use.
template <bool BF16>
using RowW4 = std::conditional_t<BF16, uint2, float4>;
template <bool BF16>
__device__ __forceinline__ void row_load_w4_packed(RowW4<BF16>& w, const void* row, int k) {
    if constexpr (BF16) w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(row) + k);
    else w = nrx_ldg4(reinterpret_cast<const float*>(row) + k, 0);
}
__device__ __forceinline__ float4 row_widen_w4(const uint2& w) { return nrx_bf16x4_to_f32(w.x, w.y); }
__device__ __forceinline__ const float4& row_widen_w4(const float4& w) { return w; }
template <bool BF16>
__device__ __forceinline__ void row_store_w4(void* row, int k, float4 o, uint64_t h) {
    if (BF16) {
        uint2 b;
        b.x = (uint32_t)sr_bf16(o.x, h, k) | ((uint32_t)sr_bf16(o.y, h, k + 1) << 16);
        b.y = (uint32_t)sr_bf16(o.z, h, k + 2) | ((uint32_t)sr_bf16(o.w, h, k + 3) << 16);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(row) + k) = b;
    } else {
        nrx_stg4(reinterpret_cast<float*>(row) + k, 0, o);
    }
}
template <bool BF16>
__device__ __forceinline__ float row_load_w(const void* row, int k) {
    if (BF16) return nrx_bf16_to_f32(reinterpret_cast<const uint16_t*>(row)[k]);
    return reinterpret_cast<const float*>(row)[k];
}
template <bool BF16>
__device__ __forceinline__ void row_store_w(void* row, int k, float o, uint64_t h) {
    if (BF16) reinterpret_cast<uint16_t*>(row)[k] = sr_bf16(o, h, k);
    else reinterpret_cast<float*>(row)[k] = o;
}

// ---- the launch shape ------------------------------------------------------------------------------
// Q lanes per row from dim, NRX_BLOCK / Q lane groups per block, 4 list entries per lane group.
struct RowLaunch {
    int ql;
    unsigned grid;
};
RowLaunch row_launch(int dim, int64_t n_unique) {
    const int ql = nrx_row_qlog2(dim);
    const int tb = NRX_BLOCK >> ql;
    const int64_t groups = (n_unique + 3) / 4;
    return {ql, (unsigned)((groups + tb - 1) / tb)};
}
// f(std::integral_constant<int, ql>) / f(std::bool_constant<b>): a run-time launch parameter becomes a template argument
template <typename F>
void dispatch_qlog2(int ql, F&& f) {
    switch (ql) {
        case 0: f(std::integral_constant<int, 0>()); break;
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        default: f(std::integral_constant<int, 6>()); break;
    }
}
template <typename F>
void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type());
    else f(std::false_type());
}
template <typename ARGS>
void launch_blocks(void (*kernel)(const ARGS), unsigned grid, hipStream_t st, const ARGS& a) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NRX_BLOCK), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------
// Fused row-sparse Adam(W) on the unique rows the sorted backward produced.
// Replaces, for the embedding tables only, the reference's dense AdamW over every row of every table
// (configure_optimizers, src/model/sort/deep/model.py:54-65).  Semantics = torch.optim.SparseAdam (moments and
// weights of a row move only in steps that looked the row up; bias correction from the global step) plus an
// optional decoupled weight decay applied to the touched rows; the padding row (row 0) never moves.
// ---------------------------------------------------------------------------------------------------
struct SparseAdamArgs {
    float* table[NRX_MAX_FEATURES];     // (bf16 tables: the uint16 tables)
    float* m[NRX_MAX_FEATURES];
    float* v[NRX_MAX_FEATURES];
    const int64_t* keys;        // (table << 40) | row, one per unique row
    const float* grads;         // [n, dim]
    const int64_t* n_dev;       // optional: actual count on the device
    int64_t max_n;
    int32_t n_tables;
    int32_t dim;
    int32_t mom_ld[NRX_MAX_FEATURES];   // per table: floats between consecutive rows of a moment array: dim, or 2 * dim when the row's two moments are adjacent
    float step_size, one_minus_b1, one_minus_b2, eps, decay;
    const float* step_size_dev;   // optional: step size read on the device (graph-captured training loops)
};
static_assert(sizeof(SparseAdamArgs) <= 3584, "kernarg budget");
// bf16 tables (nrx_sparse_adam_step_bf16) carry the rounding stream BEHIND the fp32 launch's arguments, and the MAP launches
// (nrx_sparse_adam_step_bf16_rows) the row maps behind those, each in a struct of its own: a launch without them keeps its shorter
// kernarg segment.
struct SparseAdamBf16Args {
    SparseAdamArgs base;
    uint64_t seed;
    int64_t step;
    const int64_t* step_dev;    // optional: step read on the device (captured loops)
};
static_assert(sizeof(SparseAdamBf16Args) <= 3584, "kernarg budget");
struct SparseAdamBf16MapArgs {
    SparseAdamBf16Args b;
    int64_t row_mul[NRX_MAX_FEATURES];
    int64_t row_add[NRX_MAX_FEATURES];
};
static_assert(sizeof(SparseAdamBf16MapArgs) <= 3584, "kernarg budget");

__device__ __forceinline__ float adam_elem(float g, float& m, float& v, float w, float step_size, const NRX_CONST SparseAdamArgs* a) {
    m = m + (g - m) * a->one_minus_b1;          // torch's update order
    v = v + (g * g - v) * a->one_minus_b2;
    w -= w * a->decay;
    return w - step_size * (m / (sqrtf(v) + a->eps));
}

// ARGS: SparseAdamArgs, or (BF16) SparseAdamBf16Args, or (BF16 and MAP) SparseAdamBf16MapArgs -- each begins with the one before.
// VEC: dim % 4 == 0 and aligned rows (16 bytes; 8 for bf16 weights) -> one float4 per lane per array; the update is a random 3-array
// read-modify-write, HBM-bound.
template <int QLOG2, bool VEC, bool BF16, bool MAP, typename ARGS>
__global__ __launch_bounds__(NRX_BLOCK) void sparse_adam_kernel(const ARGS args_in_kernarg) {
    const NRX_CONST SparseAdamArgs* a = nrx_kernarg<SparseAdamArgs>();
    using G = RowGroup<QLOG2, true>;
    using W = std::conditional_t<BF16, uint16_t, float>;
    constexpr int Q = G::Q, R = G::R;
    const int q = threadIdx.x & (Q - 1);
    const int D = a->dim;
    const float ss = a->step_size_dev != nullptr ? nrx_gconst<float>(a->step_size_dev)[0] : a->step_size;
    const NRX_CONST SparseAdamBf16Args* ab = nrx_kernarg<SparseAdamBf16Args>();       // (read only where BF16)
    uint64_t step = 0;
    if (BF16) step = ab->step_dev != nullptr ? (uint64_t)nrx_gconst<int64_t>(ab->step_dev)[0] : (uint64_t)ab->step;
    G grp;
    if (!grp.begin(a->max_n, a->n_dev)) return;
    const uint64_t h_step = BF16 ? sr_step_hash(ab->seed, step) : 0;
    W* p[R];
    float* pm[R];
    float* pv[R];
    uint64_t h[R];
#pragma unroll
    for (int r = 0; r < R; ++r) grp.load_key(r, a->keys);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t tc, rc;
        grp.entry(r, &a->n_tables, tc, rc);
        p[r] = reinterpret_cast<W*>(a->table[tc]) + rc * D;
        pm[r] = a->m[tc] + rc * a->mom_ld[tc];
        pv[r] = a->v[tc] + rc * a->mom_ld[tc];
        int64_t hashed = rc;
        if constexpr (MAP) {
            const NRX_CONST SparseAdamBf16MapArgs* am = nrx_kernarg<SparseAdamBf16MapArgs>();
            hashed = rc * am->row_mul[tc] + am->row_add[tc];
        }
        h[r] = BF16 ? sr_row_hash(sr_link(h_step, (uint64_t)tc), hashed) : 0;
    }
    if (VEC) {
        for (int k = q * 4; k < D; k += 4 * Q) {
            float4 g[R], m[R], v[R];
            RowW4<BF16> wp[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                g[r] = nrx_ldg4(grp.values(a->grads, r, D) + k, 0);
                row_load_w4_packed<BF16>(wp[r], p[r], k);
                m[r] = nrx_ldg4(pm[r] + k, 0);
                v[r] = nrx_ldg4(pv[r] + k, 0);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (grp.on[r]) {
                    const float4& w = row_widen_w4(wp[r]);
                    float4 o;
                    o.x = adam_elem(g[r].x, m[r].x, v[r].x, w.x, ss, a);
                    o.y = adam_elem(g[r].y, m[r].y, v[r].y, w.y, ss, a);
                    o.z = adam_elem(g[r].z, m[r].z, v[r].z, w.z, ss, a);
                    o.w = adam_elem(g[r].w, m[r].w, v[r].w, w.w, ss, a);
                    nrx_stg4(pm[r] + k, 0, m[r]);
                    nrx_stg4(pv[r] + k, 0, v[r]);
                    row_store_w4<BF16>(p[r], k, o, h[r]);
                }
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!grp.on[r]) continue;
            const float* g = a->grads + (grp.u0 + r) * (int64_t)D;
            for (int k = q; k < D; k += Q) {
                float m = pm[r][k], v = pv[r][k];
                const float o = adam_elem(g[k], m, v, row_load_w<BF16>(p[r], k), ss, a);
                pm[r][k] = m;
                pv[r][k] = v;
                row_store_w<BF16>(p[r], k, o, h[r]);
            }
        }
    }
}

// One launcher for the three Adam entry points (T: the table element, float or the uint16 bf16 pattern; the rounding stream and the
// optional row maps are read only for bf16 tables).
template <typename T>
int sparse_adam_launch(const char* who, T* const* tables, float* const* exp_avg, float* const* exp_avg_sq, int32_t n_tables, int32_t dim,
                       const int64_t* uniq_keys, const float* grads, int64_t n_unique, const int64_t* n_unique_dev, float step_size,
                       const float* step_size_dev, float beta1, float beta2, float eps, float lr_times_weight_decay, uint64_t sr_seed,
                       int64_t step, const int64_t* step_dev, const int64_t* row_mul, const int64_t* row_add, void* stream) {
    constexpr bool BF16 = std::is_same<T, uint16_t>::value;
    NRX_REQUIRE(n_tables >= 1 && n_tables <= NRX_MAX_FEATURES && dim >= 1 && n_unique >= 0, "%s: bad argument", who);
    if (n_unique == 0) return NRX_OK;
    NRX_REQUIRE(tables && exp_avg && exp_avg_sq && uniq_keys && grads, "%s: null buffer", who);
    SparseAdamBf16MapArgs am;
    SparseAdamBf16Args& ab = am.b;
    SparseAdamArgs& a = ab.base;
    // Interleaved moments: exp_avg_sq[t] == exp_avg[t] + dim means the two moments of a row of table t sit side by side
    // ([rows, 2, dim]: for dim = 16 ONE 128-byte line per row instead of two half-used ones -- the update is a random
    // read-modify-write and every 64-byte access costs a 128-byte fetch).  Separate arrays can never satisfy this by accident.
    // (The caller may list tables of other widths too -- the keys of this call never name them; their entry is unused.)
    for (int t = 0; t < n_tables; ++t) {
        NRX_REQUIRE(tables[t] && exp_avg[t] && exp_avg_sq[t], "%s: table %d: null pointer", who, t);
        a.table[t] = reinterpret_cast<float*>(tables[t]);
        a.m[t] = exp_avg[t];
        a.v[t] = exp_avg_sq[t];
        a.mom_ld[t] = exp_avg_sq[t] == exp_avg[t] + dim ? 2 * dim : dim;
    }
    a.keys = uniq_keys;
    a.grads = grads;
    a.n_dev = n_unique_dev;
    a.max_n = n_unique;
    a.n_tables = n_tables;
    a.dim = dim;
    a.step_size = step_size;
    a.step_size_dev = step_size_dev;
    a.one_minus_b1 = 1.0f - beta1;
    a.one_minus_b2 = 1.0f - beta2;
    a.eps = eps;
    a.decay = lr_times_weight_decay;
    ab.seed = sr_seed;
    ab.step = step;
    ab.step_dev = step_dev;
    const bool map = BF16 && row_mul != nullptr && row_add != nullptr;
    if (map) {
        memset(am.row_mul, 0, sizeof(am.row_mul));
        memset(am.row_add, 0, sizeof(am.row_add));
        for (int t = 0; t < n_tables; ++t) {
            am.row_mul[t] = row_mul[t];
            am.row_add[t] = row_add[t];
        }
    }
    bool vec = (dim & 3) == 0 && nrx_aligned16(grads);
    for (int t = 0; t < n_tables && vec; ++t)          // four weights: 16 bytes of fp32, 8 of bf16
        vec = (reinterpret_cast<uintptr_t>(tables[t]) & (4 * sizeof(T) - 1)) == 0 && nrx_aligned16(exp_avg[t]) && nrx_aligned16(exp_avg_sq[t]);
    const RowLaunch L = row_launch(dim, n_unique);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_qlog2(L.ql, [&](auto QL) {
        dispatch_bool(vec, [&](auto V) {
            constexpr int ql = decltype(QL)::value;
            constexpr bool v = decltype(V)::value;
            if constexpr (!BF16) launch_blocks(sparse_adam_kernel<ql, v, false, false, SparseAdamArgs>, L.grid, st, a);
            else if (map) launch_blocks(sparse_adam_kernel<ql, v, true, true, SparseAdamBf16MapArgs>, L.grid, st, am);
            else launch_blocks(sparse_adam_kernel<ql, v, true, false, SparseAdamBf16Args>, L.grid, st, ab);
        });
    });
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

}  // namespace

extern "C" int nrx_sparse_adam_step(float* const* tables, float* const* exp_avg, float* const* exp_avg_sq, int32_t n_tables,
                                    int32_t dim, const int64_t* uniq_keys, const float* grads, int64_t n_unique,
                                    const int64_t* n_unique_dev, float step_size, const float* step_size_dev, float beta1,
                                    float beta2, float eps, float lr_times_weight_decay, void* stream) {
    NRX_TRACE();
    return sparse_adam_launch("nrx_sparse_adam_step", tables, exp_avg, exp_avg_sq, n_tables, dim, uniq_keys, grads, n_unique, n_unique_dev,
                              step_size, step_size_dev, beta1, beta2, eps, lr_times_weight_decay, 0, 0, nullptr, nullptr, nullptr, stream);
}

extern "C" int nrx_sparse_adam_step_bf16(uint16_t* const* tables, float* const* exp_avg, float* const* exp_avg_sq, int32_t n_tables,
                                         int32_t dim, const int64_t* uniq_keys, const float* grads, int64_t n_unique,
                                         const int64_t* n_unique_dev, float step_size, const float* step_size_dev, float beta1,
                                         float beta2, float eps, float lr_times_weight_decay, uint64_t sr_seed, int64_t step,
                                         const int64_t* step_dev, void* stream) {
    NRX_TRACE();
    return sparse_adam_launch("nrx_sparse_adam_step_bf16", tables, exp_avg, exp_avg_sq, n_tables, dim, uniq_keys, grads, n_unique, n_unique_dev,
                              step_size, step_size_dev, beta1, beta2, eps, lr_times_weight_decay, sr_seed, step, step_dev, nullptr, nullptr, stream);
}

extern "C" int nrx_sparse_adam_step_bf16_rows(uint16_t* const* tables, float* const* exp_avg, float* const* exp_avg_sq, int32_t n_tables,
                                              int32_t dim, const int64_t* uniq_keys, const float* grads, int64_t n_unique,
                                              const int64_t* n_unique_dev, float step_size, const float* step_size_dev, float beta1,
                                              float beta2, float eps, float lr_times_weight_decay, uint64_t sr_seed, int64_t step,
                                              const int64_t* step_dev, const int64_t* row_mul, const int64_t* row_add, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE((row_mul == nullptr) == (row_add == nullptr), "nrx_sparse_adam_step_bf16_rows: row_mul and row_add come together (both null: identity)");
    return sparse_adam_launch("nrx_sparse_adam_step_bf16_rows", tables, exp_avg, exp_avg_sq, n_tables, dim, uniq_keys, grads, n_unique, n_unique_dev,
                              step_size, step_size_dev, beta1, beta2, eps, lr_times_weight_decay, sr_seed, step, step_dev, row_mul, row_add, stream);
}

// --------------------------------------------------------------------------------------------
// Unique-row gradients -> dense gradient tables (the DEFAULT backward of the gather: nn.Embedding(sparse=False)'s
// [rows, dim] .grad, formed from the deterministic sorted reduction instead of float atomics).
// One lane group per 4 unique rows: key loads, then 4 independent row loads, then the stores.  Row 0 is written like any other.
// --------------------------------------------------------------------------------------------
namespace {

struct RowsToDenseArgs {
    float* table[NRX_MAX_FEATURES];
    const int64_t* keys;        // (table << 40) | row, one per unique row
    const float* rows;          // [n, dim]
    const int64_t* n_dev;       // optional: actual count on the device
    int64_t max_n;
    int32_t n_tables;
    int32_t dim;
    int32_t accumulate;         // != 0: table row += (a table fed by more than one reduction); 0: plain store
};

template <int QLOG2, bool VEC, bool ACC>
__global__ __launch_bounds__(NRX_BLOCK) void rows_to_dense_kernel(const RowsToDenseArgs args_in_kernarg) {
    const NRX_CONST RowsToDenseArgs* a = nrx_kernarg<RowsToDenseArgs>();
    using G = RowGroup<QLOG2, false>;
    constexpr int Q = G::Q, R = G::R;
    const int q = threadIdx.x & (Q - 1);
    const int D = a->dim;
    G grp;
    if (!grp.begin(a->max_n, a->n_dev)) return;
    float* p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) grp.load_key(r, a->keys);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t tc, rc;
        grp.entry(r, &a->n_tables, tc, rc);
        p[r] = a->table[tc] + rc * D;
    }
    if (VEC) {
        for (int k = q * 4; k < D; k += 4 * Q) {
            float4 g[R], w[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                g[r] = nrx_ldg4(grp.values(a->rows, r, D) + k, 0);
                if (ACC) w[r] = nrx_ldg4(p[r] + k, 0);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (grp.on[r]) {
                    if (ACC) { g[r].x += w[r].x; g[r].y += w[r].y; g[r].z += w[r].z; g[r].w += w[r].w; }
                    nrx_stg4(p[r] + k, 0, g[r]);
                }
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!grp.on[r]) continue;
            const float* g = a->rows + (grp.u0 + r) * (int64_t)D;
            for (int k = q; k < D; k += Q) p[r][k] = ACC ? p[r][k] + g[k] : g[k];
        }
    }
}

}  // namespace

extern "C" int nrx_rows_to_dense(float* const* tables, int32_t n_tables, int32_t dim, const int64_t* uniq_keys, const float* rows,
                                 int64_t n_unique, const int64_t* n_unique_dev, int32_t accumulate, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n_tables >= 1 && n_tables <= NRX_MAX_FEATURES && dim >= 1 && n_unique >= 0, "nrx_rows_to_dense: bad argument");
    if (n_unique == 0) return NRX_OK;
    NRX_REQUIRE(tables && uniq_keys && rows, "nrx_rows_to_dense: null buffer");
    RowsToDenseArgs a;
    bool vec = (dim & 3) == 0 && nrx_aligned16(rows);
    for (int t = 0; t < n_tables; ++t) {         // (tables of another width may be listed: the keys of this call never name them)
        NRX_REQUIRE(tables[t] != nullptr, "nrx_rows_to_dense: table %d: null pointer", t);
        a.table[t] = tables[t];
        vec = vec && nrx_aligned16(tables[t]);
    }
    a.keys = uniq_keys;
    a.rows = rows;
    a.n_dev = n_unique_dev;
    a.max_n = n_unique;
    a.n_tables = n_tables;
    a.dim = dim;
    a.accumulate = accumulate;
    const RowLaunch L = row_launch(dim, n_unique);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_qlog2(L.ql, [&](auto QL) {
        dispatch_bool(vec, [&](auto V) {
            dispatch_bool(accumulate != 0, [&](auto ACC) {
                launch_blocks(rows_to_dense_kernel<decltype(QL)::value, decltype(V)::value, decltype(ACC)::value>, L.grid, st, a);
            });
        });
    });
    NRX_LAUNCH_CHECK("nrx_rows_to_dense");
    return NRX_OK;
}

// ---- exact dense AdamW from row-sparse gradients ("exact-dense mode"): the reference trains every table with one dense
// torch.optim.AdamW (sort/deep/model.py:55) -- EVERY row moves every step (weight decay, decaying moments), so the optimizer is a stream over the
// whole tables however few rows the batch looked up.  This form does that stream ONCE: (p, m, v) of every row read and written, the gradient taken
// from the backward's (key, row) pairs where there is one (a per-table slot map, -1 elsewhere, written by nrx_rows_mark and reset here) and zero
// otherwise -- no dense gradient tensor is formed, zero-filled or read.  torch's single-tensor AdamW arithmetic, fp32.  (It walks table rows, not
// a key list: the lane mapping is the row-list kernels', the walk its own.)
namespace {

struct DenseAdamWArgs {
    float* table[NRX_MAX_FEATURES];
    float* m[NRX_MAX_FEATURES];
    float* v[NRX_MAX_FEATURES];
    int32_t* map[NRX_MAX_FEATURES];         // [rows] slot of the row's gradient in `grads`, or -1
    int64_t rows[NRX_MAX_FEATURES];
    int32_t tile0[NRX_MAX_FEATURES + 1];    // first block of every table
    const float* grads;                     // [n, dim]
    int32_t n_tables, dim;
    float decay_keep, one_minus_b1, one_minus_b2, b2, step_size, inv_bc2_sqrt, eps;
    const float* hyper_dev;                 // optional {lr / bias_correction1, 1 / sqrt(bias_correction2)} on the device (captured training loops)
};
static_assert(sizeof(DenseAdamWArgs) <= 3840, "kernarg budget");

__device__ __forceinline__ float adamw_elem(float g, float& m, float& v, float w, const NRX_CONST DenseAdamWArgs* a, float step_size, float inv_bc2_sqrt) {
    w *= a->decay_keep;                                   // param.mul_(1 - lr * weight_decay)
    m = m + (g - m) * a->one_minus_b1;                    // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a->b2 + g * g * a->one_minus_b2;              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) * inv_bc2_sqrt + a->eps;
    return w - step_size * (m / denom);                  // param.addcdiv_(exp_avg, denom, value = -lr / bias_correction1)
}

template <int QLOG2, bool VEC>
__global__ __launch_bounds__(NRX_BLOCK) void dense_adamw_rows_kernel(const DenseAdamWArgs args_in_kernarg) {
    const NRX_CONST DenseAdamWArgs* a = nrx_kernarg<DenseAdamWArgs>();
    constexpr int Q = 1 << QLOG2, TB = NRX_BLOCK / Q, R = 4;
    const int q = threadIdx.x & (Q - 1), g = threadIdx.x >> QLOG2;
    int t = 0;                              // the block's table: tile0[t] <= blockIdx.x < tile0[t + 1] (uniform)
    while (t + 1 < a->n_tables && (int)blockIdx.x >= a->tile0[t + 1]) ++t;
    const int64_t nrows = a->rows[t];
    const int D = a->dim;
    const float ss = a->hyper_dev != nullptr ? nrx_gconst<float>(a->hyper_dev)[0] : a->step_size;
    const float ib = a->hyper_dev != nullptr ? nrx_gconst<float>(a->hyper_dev)[1] : a->inv_bc2_sqrt;
    float* tab = a->table[t];
    float* mt = a->m[t];
    float* vt = a->v[t];
    int32_t* map = a->map[t];
    const int64_t r0 = ((int64_t)((int)blockIdx.x - a->tile0[t]) * TB + g) * R;
    int slot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) slot[r] = r0 + r < nrows ? map[r0 + r] : -1;
    if (VEC) {
        for (int k = q * 4; k < D; k += 4 * Q) {
            float4 gr[R], w[R], m[R], v[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t row = r0 + r < nrows ? r0 + r : 0;
                gr[r] = slot[r] >= 0 ? nrx_ldg4(a->grads + (int64_t)slot[r] * D + k, 0) : make_float4(0.f, 0.f, 0.f, 0.f);
                w[r] = nrx_ldg4(tab + row * D + k, 0);
                m[r] = nrx_ldg4(mt + row * D + k, 0);
                v[r] = nrx_ldg4(vt + row * D + k, 0);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r0 + r >= nrows) continue;
                w[r].x = adamw_elem(gr[r].x, m[r].x, v[r].x, w[r].x, a, ss, ib);
                w[r].y = adamw_elem(gr[r].y, m[r].y, v[r].y, w[r].y, a, ss, ib);
                w[r].z = adamw_elem(gr[r].z, m[r].z, v[r].z, w[r].z, a, ss, ib);
                w[r].w = adamw_elem(gr[r].w, m[r].w, v[r].w, w[r].w, a, ss, ib);
                const int64_t row = r0 + r;
                nrx_stg4(tab + row * D + k, 0, w[r]);
                nrx_stg4(mt + row * D + k, 0, m[r]);
                nrx_stg4(vt + row * D + k, 0, v[r]);
            }
        }
    } else {
        for (int r = 0; r < R; ++r) {
            if (r0 + r >= nrows) continue;
            const int64_t row = r0 + r;
            for (int k = q; k < D; k += Q) {
                const float gk = slot[r] >= 0 ? a->grads[(int64_t)slot[r] * D + k] : 0.f;
                float mk = mt[row * D + k], vk = vt[row * D + k];
                tab[row * D + k] = adamw_elem(gk, mk, vk, tab[row * D + k], a, ss, ib);
                mt[row * D + k] = mk;
                vt[row * D + k] = vk;
            }
        }
    }
    if (q == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (slot[r] >= 0) map[r0 + r] = -1;       // the map is all -1 again when the launch ends
    }
}

struct RowsMarkArgs {
    int32_t* map[NRX_MAX_FEATURES];
    int64_t rows[NRX_MAX_FEATURES];
    const int64_t* keys;
    const int64_t* n_dev;
    int64_t max_n;
    int32_t n_tables;
    int32_t unmark;
};

__global__ __launch_bounds__(NRX_BLOCK) void rows_mark_kernel(const RowsMarkArgs args_in_kernarg) {
    const NRX_CONST RowsMarkArgs* a = nrx_kernarg<RowsMarkArgs>();
    const int64_t n = row_list_len(a->max_n, a->n_dev);
    const int64_t i = (int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t key = nrx_gconst<int64_t>(a->keys)[i];
    int64_t t, row;
    split_key(key, t, row);
    if (key < 0 || t >= a->n_tables || row == 0) return;         // filler keys; the padding row never trains
    if (row < a->rows[t]) a->map[t][row] = a->unmark ? -1 : (int32_t)i;
}

// Two unique-key lists that may name the same row (DSSM's towers share the news table: two backward launches, two sink entries): with list A
// marked in the slot maps, every pair of list B whose row A also has is ADDED to A's row and its key becomes the filler -1; the rest of B stays.
// A row has at most one pair in each list, so every sum is one addition: deterministic.  One lane group per pair of B.
struct RowsMergeArgs {
    int32_t* map[NRX_MAX_FEATURES];
    int64_t rows[NRX_MAX_FEATURES];
    int64_t* keys_b;
    const float* values_b;
    float* values_a;
    const int64_t* n_dev;
    int64_t max_n;
    int32_t n_tables, dim;
};

__global__ __launch_bounds__(NRX_BLOCK) void rows_merge_kernel(const RowsMergeArgs args_in_kernarg) {
    const NRX_CONST RowsMergeArgs* a = nrx_kernarg<RowsMergeArgs>();
    const int64_t n = row_list_len(a->max_n, a->n_dev);
    const int q = threadIdx.x & 15;                              // 16 lanes per pair
    const int64_t j = ((int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x) >> 4;
    if (j >= n) return;
    const int64_t key = a->keys_b[j];
    int64_t t, row;
    split_key(key, t, row);
    if (key < 0 || t >= a->n_tables || row == 0 || row >= a->rows[t]) return;
    const int32_t sa = a->map[t][row];
    if (sa < 0) return;
    const int D = a->dim;
    for (int k = q; k < D; k += 16) a->values_a[(int64_t)sa * D + k] += a->values_b[j * D + k];
    if (q == 0) a->keys_b[j] = -1;
}

}  // namespace

// slot_maps[t][row] = i for every key i = (t << 40 | row) of the list (negative keys and keys of tables >= n_tables are fillers; row 0 is the
// padding row): the per-table row -> gradient-slot maps nrx_dense_adamw_rows reads.  The maps must be all -1 before (they are again after
// nrx_dense_adamw_rows).  Keys must be unique.  unmark != 0: writes -1 instead (undoes a marking).
extern "C" int nrx_rows_mark(const int64_t* uniq_keys, int64_t n, const int64_t* n_dev, int32_t* const* slot_maps, const int64_t* rows,
                             int32_t n_tables, int32_t unmark, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n >= 0 && n <= 0x7fffffffll && n_tables >= 1 && n_tables <= NRX_MAX_FEATURES, "nrx_rows_mark: bad argument");
    if (n == 0) return NRX_OK;
    NRX_REQUIRE(uniq_keys && slot_maps && rows, "nrx_rows_mark: null buffer");
    RowsMarkArgs a;
    for (int t = 0; t < n_tables; ++t) {
        NRX_REQUIRE(slot_maps[t] != nullptr && rows[t] >= 1, "nrx_rows_mark: table %d: null map / no rows", t);
        a.map[t] = slot_maps[t];
        a.rows[t] = rows[t];
    }
    a.keys = uniq_keys; a.n_dev = n_dev; a.max_n = n; a.n_tables = n_tables; a.unmark = unmark != 0;
    launch_blocks(rows_mark_kernel, (unsigned)((n + NRX_BLOCK - 1) / NRX_BLOCK), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK("nrx_rows_mark");
    return NRX_OK;
}

// keys_b / values_b [n, dim] merged into the list marked in slot_maps (values_a: its [.., dim] rows): see rows_merge_kernel.
extern "C" int nrx_rows_merge(int64_t* keys_b, const float* values_b, int64_t n, const int64_t* n_dev, float* values_a, int32_t* const* slot_maps,
                              const int64_t* rows, int32_t n_tables, int32_t dim, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n >= 0 && n_tables >= 1 && n_tables <= NRX_MAX_FEATURES && dim >= 1, "nrx_rows_merge: bad argument");
    if (n == 0) return NRX_OK;
    NRX_REQUIRE(keys_b && values_b && values_a && slot_maps && rows, "nrx_rows_merge: null buffer");
    RowsMergeArgs a;
    for (int t = 0; t < n_tables; ++t) {
        NRX_REQUIRE(slot_maps[t] != nullptr && rows[t] >= 1, "nrx_rows_merge: table %d: null map / no rows", t);
        a.map[t] = slot_maps[t];
        a.rows[t] = rows[t];
    }
    a.keys_b = keys_b; a.values_b = values_b; a.values_a = values_a; a.n_dev = n_dev; a.max_n = n; a.n_tables = n_tables; a.dim = dim;
    launch_blocks(rows_merge_kernel, (unsigned)((n * 16 + NRX_BLOCK - 1) / NRX_BLOCK), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK("nrx_rows_merge");
    return NRX_OK;
}

// One AdamW step (torch.optim.AdamW's arithmetic: decoupled weight decay, bias corrections of step `step` >= 1) over EVERY row of the n_tables
// [rows[t], dim] tables: the gradient of row r of table t is grads[slot_maps[t][r]] where that slot is >= 0 (nrx_rows_mark), zero elsewhere;
// exp_avg / exp_avg_sq: [rows[t], dim] like the tables (torch's state layout).  Resets every slot it consumed to -1.  hyper_dev (optional, device):
// {lr / bias_correction1, 1 / sqrt(bias_correction2)} read by the kernel instead of the values computed from `step` -- a loop captured in a
// hipGraph advances them between replays.
extern "C" int nrx_dense_adamw_rows(float* const* tables, float* const* exp_avg, float* const* exp_avg_sq, int32_t* const* slot_maps,
                                    const int64_t* rows, int32_t n_tables, int32_t dim, const float* grads, int64_t step, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, const float* hyper_dev, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n_tables >= 1 && n_tables <= NRX_MAX_FEATURES && dim >= 1 && step >= 1, "nrx_dense_adamw_rows: bad argument");
    NRX_REQUIRE(tables && exp_avg && exp_avg_sq && slot_maps && rows, "nrx_dense_adamw_rows: null buffer");
    DenseAdamWArgs a;
    const int ql = nrx_row_qlog2(dim);
    const int tb = (NRX_BLOCK >> ql) * 4;                   // rows per block
    bool vec = (dim & 3) == 0 && (grads == nullptr || nrx_aligned16(grads));
    int64_t blocks = 0;
    for (int t = 0; t < n_tables; ++t) {
        NRX_REQUIRE(tables[t] && exp_avg[t] && exp_avg_sq[t] && slot_maps[t] && rows[t] >= 1, "nrx_dense_adamw_rows: table %d: null pointer / no rows", t);
        a.table[t] = tables[t]; a.m[t] = exp_avg[t]; a.v[t] = exp_avg_sq[t]; a.map[t] = slot_maps[t]; a.rows[t] = rows[t];
        a.tile0[t] = (int32_t)blocks;
        blocks += (rows[t] + tb - 1) / tb;
        vec = vec && nrx_aligned16(tables[t]) && nrx_aligned16(exp_avg[t]) && nrx_aligned16(exp_avg_sq[t]);
    }
    NRX_REQUIRE(blocks <= 0x7fffffffll, "nrx_dense_adamw_rows: too many rows for one launch");
    a.tile0[n_tables] = (int32_t)blocks;
    a.grads = grads;
    a.n_tables = n_tables;
    a.dim = dim;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    a.decay_keep = 1.0f - lr * weight_decay;
    a.one_minus_b1 = 1.0f - beta1;
    a.one_minus_b2 = 1.0f - beta2;
    a.b2 = beta2;
    a.step_size = (float)((double)lr / bc1);
    a.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    a.eps = eps;
    a.hyper_dev = hyper_dev;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_qlog2(ql, [&](auto QL) {
        dispatch_bool(vec, [&](auto V) { launch_blocks(dense_adamw_rows_kernel<decltype(QL)::value, decltype(V)::value>, (unsigned)blocks, st, a); });
    });
    NRX_LAUNCH_CHECK("nrx_dense_adamw_rows");
    return NRX_OK;
}

// ---------------------------------------------------------------------------------------------------
// Fused row-sparse Adagrad on the same unique-row lists (nrx_sparse_adagrad_step; the update rules and the summation order of the
// row-wise form are written down in nrx_embed.h).  One fp32 accumulator per ELEMENT (state [rows, dim]: torch.optim.Adagrad on sparse
// gradients) or one per ROW (state [rows]: the mean of the row's squared gradient) instead of Adam's two moments per element.
// Lane mapping = sparse_adam_kernel's: Q lanes per row chosen from dim, R = 4 rows in flight per lane group, a float4 per lane.  Lane l
// of a group owns the columns c with (c / 4) % Q == l in BOTH forms (VEC: one 16-byte access per four columns; otherwise element by
// element), so the row-wise sum of squares has one order per dim, whatever the alignment of the buffers.
// ---------------------------------------------------------------------------------------------------
namespace {

struct SparseAdagradArgs {
    void* table[NRX_MAX_FEATURES];      // fp32 [rows, dim], or (BF16) uint16 patterns
    float* state[NRX_MAX_FEATURES];     // [rows, dim], or (ROWWISE) [rows]
    int64_t row_mul[NRX_MAX_FEATURES];  // BF16: the rounding hash sees row * row_mul[t] + row_add[t] ({1, 0}: the key's row)
    int64_t row_add[NRX_MAX_FEATURES];
    const int64_t* keys;
    const float* grads;
    const int64_t* n_dev;
    int64_t max_n;
    int32_t n_tables;
    int32_t dim;
    float lr, eps, decay;
    const float* lr_dev;
    uint64_t seed;
    int64_t step;
    const int64_t* step_dev;
};
static_assert(sizeof(SparseAdagradArgs) <= 3584, "kernarg budget");

// (contraction off: the products and sums below round exactly as written, in every instantiation -- the bit-identity of the two forms,
// of sharded and unsharded runs and of bf16 against fp32 tables rests on it; the one fused operation is the explicit fmaf)
__device__ __forceinline__ float adagrad_sq(float g, float acc) {
    return fmaf(g, g, acc);
}
__device__ __forceinline__ float adagrad_denom(float s, float eps) {
#pragma clang fp contract(off)
    return sqrtf(s) + eps;
}
__device__ __forceinline__ float adagrad_w(float g, float w, float denom, float lr, float decay) {
#pragma clang fp contract(off)
    const float wd = w * decay;
    w = w - wd;
    const float num = lr * g;
    return w - num / denom;
}

// Sum over the Q = 2^QLOG2 lanes of a row's group (aligned, contiguous lanes of one wavefront), the result in every lane of the group.  The fixed tree:
// lane ^ 1, lane ^ 2 (quad permutes), the other quad of each 8 (row_half_mirror), the other half of each 16 (row_mirror), lane ^ 16, lane ^ 32.
// Every step adds two values that are equal across the lanes they came from, so all lanes of the group hold the same bits afterwards.
template <int QLOG2>
__device__ __forceinline__ float adagrad_group_sum(float v) {
    if (QLOG2 >= 1) v += nrx_dpp<0xB1>(v);
    if (QLOG2 >= 2) v += nrx_dpp<0x4E>(v);
    if (QLOG2 >= 3) v += nrx_dpp<0x141>(v);
    if (QLOG2 >= 4) v += nrx_dpp<0x140>(v);
    if (QLOG2 >= 5) v += __shfl_xor(v, 16, 64);
    if (QLOG2 >= 6) v += __shfl_xor(v, 32, 64);
    return v;
}

template <int QLOG2, bool VEC, bool ROWWISE, bool BF16>
__global__ __launch_bounds__(NRX_BLOCK) void sparse_adagrad_kernel(const SparseAdagradArgs args_in_kernarg) {
    const NRX_CONST SparseAdagradArgs* a = nrx_kernarg<SparseAdagradArgs>();
    using G = RowGroup<QLOG2, true>;
    constexpr int Q = G::Q, R = G::R;
    const int q = threadIdx.x & (Q - 1);
    const int D = a->dim;
    const float lr = a->lr_dev != nullptr ? nrx_gconst<float>(a->lr_dev)[0] : a->lr;
    const float eps = a->eps, decay = a->decay;
    G grp;              // (a whole lane group leaves: the cross-lane sums below never read outside their group)
    if (!grp.begin(a->max_n, a->n_dev)) return;
    uint64_t h_step = 0;
    if (BF16) {
        const uint64_t step = a->step_dev != nullptr ? (uint64_t)nrx_gconst<int64_t>(a->step_dev)[0] : (uint64_t)a->step;
        h_step = sr_step_hash(a->seed, step);
    }
    char* p[R];
    float* ps[R];
    const float* pg[R];
    uint64_t h[R];
#pragma unroll
    for (int r = 0; r < R; ++r) grp.load_key(r, a->keys);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t tc, rc;
        grp.entry(r, &a->n_tables, tc, rc);
        p[r] = reinterpret_cast<char*>(a->table[tc]) + rc * D * (BF16 ? 2 : 4);
        ps[r] = a->state[tc] + (ROWWISE ? rc : rc * D);
        pg[r] = grp.values(a->grads, r, D);
        h[r] = BF16 ? sr_row_hash(sr_link(h_step, (uint64_t)tc), rc * a->row_mul[tc] + a->row_add[tc]) : 0;
    }
    if (ROWWISE) {
        // pass 1: every lane adds the squares of its columns in ascending order, the group's lanes are combined by the fixed tree.  While the
        // row fits one float4 per lane (dim <= 4 Q: every dim up to 256) the gradient stays in registers for pass 2.
        const bool once = QLOG2 < 6 || D <= 4 * Q;     // (Q < 64 is chosen with 4 Q >= dim)
        float4 g0[R];
        float s_old[R], acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            s_old[r] = ps[r][0];
            acc[r] = 0.f;
            g0[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (VEC) {
            if (q * 4 < D) {
#pragma unroll
                for (int r = 0; r < R; ++r) g0[r] = nrx_ldg4(pg[r] + q * 4, 0);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                acc[r] = adagrad_sq(g0[r].w, adagrad_sq(g0[r].z, adagrad_sq(g0[r].y, adagrad_sq(g0[r].x, 0.f))));      // (zeros beyond dim add nothing)
            for (int k = q * 4 + 4 * Q; k < D; k += 4 * Q) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 g = nrx_ldg4(pg[r] + k, 0);
                    acc[r] = adagrad_sq(g.w, adagrad_sq(g.z, adagrad_sq(g.y, adagrad_sq(g.x, acc[r]))));
                }
            }
        } else {
            for (int k0 = q * 4; k0 < D; k0 += 4 * Q) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (k0 + c < D) {
#pragma unroll
                        for (int r = 0; r < R; ++r) acc[r] = adagrad_sq(pg[r][k0 + c], acc[r]);
                    }
                }
            }
        }
        float denom[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float tot = adagrad_group_sum<QLOG2>(acc[r]);
            const float s_new = s_old[r] + tot / (float)D;
            denom[r] = adagrad_denom(s_new, eps);
            if (grp.on[r] && q == 0) ps[r][0] = s_new;          // a 4-byte store to the row's own word: the neighbours in its 128-byte line are other rows'
        }
        if (VEC) {
            for (int k = q * 4; k < D; k += 4 * Q) {
                float4 g[R], w[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    g[r] = once ? g0[r] : nrx_ldg4(pg[r] + k, 0);
                    w[r] = row_load_w4<BF16>(p[r], k);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (grp.on[r]) {
                        float4 o;
                        o.x = adagrad_w(g[r].x, w[r].x, denom[r], lr, decay);
                        o.y = adagrad_w(g[r].y, w[r].y, denom[r], lr, decay);
                        o.z = adagrad_w(g[r].z, w[r].z, denom[r], lr, decay);
                        o.w = adagrad_w(g[r].w, w[r].w, denom[r], lr, decay);
                        row_store_w4<BF16>(p[r], k, o, h[r]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (!grp.on[r]) continue;
                for (int k0 = q * 4; k0 < D; k0 += 4 * Q)
                    for (int k = k0; k < k0 + 4 && k < D; ++k)
                        row_store_w<BF16>(p[r], k, adagrad_w(pg[r][k], row_load_w<BF16>(p[r], k), denom[r], lr, decay), h[r]);
            }
        }
    } else if (VEC) {
        for (int k = q * 4; k < D; k += 4 * Q) {
            float4 g[R], w[R], s[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                g[r] = nrx_ldg4(pg[r] + k, 0);
                w[r] = row_load_w4<BF16>(p[r], k);
                s[r] = nrx_ldg4(ps[r] + k, 0);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (grp.on[r]) {
                    float4 o;
                    s[r].x = adagrad_sq(g[r].x, s[r].x); o.x = adagrad_w(g[r].x, w[r].x, adagrad_denom(s[r].x, eps), lr, decay);
                    s[r].y = adagrad_sq(g[r].y, s[r].y); o.y = adagrad_w(g[r].y, w[r].y, adagrad_denom(s[r].y, eps), lr, decay);
                    s[r].z = adagrad_sq(g[r].z, s[r].z); o.z = adagrad_w(g[r].z, w[r].z, adagrad_denom(s[r].z, eps), lr, decay);
                    s[r].w = adagrad_sq(g[r].w, s[r].w); o.w = adagrad_w(g[r].w, w[r].w, adagrad_denom(s[r].w, eps), lr, decay);
                    nrx_stg4(ps[r] + k, 0, s[r]);
                    row_store_w4<BF16>(p[r], k, o, h[r]);
                }
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!grp.on[r]) continue;
            for (int k0 = q * 4; k0 < D; k0 += 4 * Q)
                for (int k = k0; k < k0 + 4 && k < D; ++k) {
                    const float g = pg[r][k], s = adagrad_sq(g, ps[r][k]);
                    ps[r][k] = s;
                    row_store_w<BF16>(p[r], k, adagrad_w(g, row_load_w<BF16>(p[r], k), adagrad_denom(s, eps), lr, decay), h[r]);
                }
        }
    }
}

}  // namespace

extern "C" int nrx_sparse_adagrad_step(void* const* tables, float* const* state, int32_t n_tables, int32_t dim, const int64_t* uniq_keys,
                                       const float* grads, int64_t n_unique, const int64_t* n_unique_dev, float lr, const float* lr_dev,
                                       float eps, float lr_times_weight_decay, uint32_t flags, uint64_t sr_seed, int64_t step,
                                       const int64_t* step_dev, const int64_t* row_mul, const int64_t* row_add, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n_tables >= 1 && n_tables <= NRX_MAX_FEATURES && dim >= 1 && n_unique >= 0, "nrx_sparse_adagrad_step: bad argument");
    NRX_REQUIRE((flags & ~(uint32_t)(NRX_ADAGRAD_ROWWISE | NRX_ADAGRAD_TABLE_BF16)) == 0, "nrx_sparse_adagrad_step: unknown flag bits 0x%x", flags);
    NRX_REQUIRE((row_mul == nullptr) == (row_add == nullptr), "nrx_sparse_adagrad_step: row_mul and row_add come together (both null: identity)");
    const bool rowwise = (flags & NRX_ADAGRAD_ROWWISE) != 0, bf16 = (flags & NRX_ADAGRAD_TABLE_BF16) != 0;
    NRX_REQUIRE(bf16 || row_mul == nullptr, "nrx_sparse_adagrad_step: row_mul / row_add belong to bf16 tables (NRX_ADAGRAD_TABLE_BF16)");
    if (n_unique == 0) return NRX_OK;
    NRX_REQUIRE(tables && state && uniq_keys && grads, "nrx_sparse_adagrad_step: null buffer");
    SparseAdagradArgs a;
    memset(a.row_mul, 0, sizeof(a.row_mul));
    memset(a.row_add, 0, sizeof(a.row_add));
    bool vec = (dim & 3) == 0 && nrx_aligned16(grads);
    for (int t = 0; t < n_tables; ++t) {
        NRX_REQUIRE(tables[t] && state[t], "nrx_sparse_adagrad_step: table %d: null pointer", t);
        NRX_REQUIRE((reinterpret_cast<uintptr_t>(tables[t]) & (bf16 ? 1u : 3u)) == 0 && (reinterpret_cast<uintptr_t>(state[t]) & 3u) == 0,
                    "nrx_sparse_adagrad_step: table %d: misaligned pointer", t);
        a.table[t] = tables[t];
        a.state[t] = state[t];
        a.row_mul[t] = row_mul != nullptr ? row_mul[t] : 1;
        a.row_add[t] = row_add != nullptr ? row_add[t] : 0;
        vec = vec && (reinterpret_cast<uintptr_t>(tables[t]) & (bf16 ? 7u : 15u)) == 0 && (rowwise || nrx_aligned16(state[t]));
    }
    a.keys = uniq_keys;
    a.grads = grads;
    a.n_dev = n_unique_dev;
    a.max_n = n_unique;
    a.n_tables = n_tables;
    a.dim = dim;
    a.lr = lr;
    a.lr_dev = lr_dev;
    a.eps = eps;
    a.decay = lr_times_weight_decay;
    a.seed = sr_seed;
    a.step = step;
    a.step_dev = step_dev;
    const RowLaunch L = row_launch(dim, n_unique);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_qlog2(L.ql, [&](auto QL) {
        dispatch_bool(vec, [&](auto V) {
            dispatch_bool(rowwise, [&](auto RW) {
                dispatch_bool(bf16, [&](auto BF) {
                    launch_blocks(sparse_adagrad_kernel<decltype(QL)::value, decltype(V)::value, decltype(RW)::value, decltype(BF)::value>, L.grid, st, a);
                });
            });
        });
    });
    NRX_LAUNCH_CHECK("nrx_sparse_adagrad_step");
    return NRX_OK;
}
