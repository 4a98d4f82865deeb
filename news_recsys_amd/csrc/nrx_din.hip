// DIN-style target attention over the click history, fused into the gather: the candidate's embedding is the query, the history rows are
// keys and values, read once straight from the table; forward and backward with nothing of size batch * bag_len kept in between.
// No reference counterpart (the reference's rankers see the history through array_feature_pooling's masked mean only); DESIGN 7h.
//
// Definition (include/nrx_embed.h restates it): e_l = table[ids[b, l]] widened to fp32; entry l is kept iff mask is null or mask[b, l] != 0;
// s_l = dot(query_b, e_l) * scale; p = softmax over the kept l; out_b = sum_l p_l e_l; lse_b = log sum_kept exp(s_l).  Backward, with
// delta = dot(g_out_b, out_b): dp_l = dot(g_out_b, e_l), ds_l = p_l (dp_l - delta), g_query_b = scale sum_l ds_l e_l,
// g_rows[b, l] = p_l g_out_b + scale ds_l query_b; s and p are recomputed from the table, the query and lse.
//
// Mapping: ONE WAVE OWNS ONE SAMPLE at a time (4 waves per workgroup, samples strided over the grid).  A row takes Q = DP / 4 lanes (DP = dim
// padded to 4, 8, 16, 32 or 64), one 16-byte load per lane (8 bytes of a bf16 table), so R = 64 / Q rows are in flight per step: lane =
// slot * Q + chunk, slot s of step t holds entry l = t R + s.  The sample's ids and mask are read coalesced once (lane i holds entries i,
// 64 + i, 128 + i, 192 + i as one word each: row | kept | out-of-range) -- the next sample's before the current one is consumed -- and
// handed to the slots by cross-lane moves.  The rows of step t + 1 are requested before step t is consumed, and every lane loads every step:
// an entry that reads nothing (masked, past the end, out of range) reads row 0, so no load sits behind a branch.
//   forward : each slot keeps its own running (max, sum, acc) over its steps; the slots are merged once per sample by a butterfly over the
//             slot bits (lowest first), then slot 0 writes out_b and lane 0 writes lse_b.
//   backward: one pass; p_l = exp(s_l - lse_b); the g_rows row of (b, l) is stored by the lanes that hold e_l (a step's rows are one
//             contiguous run); each slot accumulates its part of g_query, merged by the same butterfly.
// One owner per output row: no atomics, no workspace, no LDS.
// Summation order: a dot product over dim is one fma chain per 4-column chunk (columns 4c .. 4c + 3 in order, the first product rounded on
// its own), the chunks added as a balanced binary tree in chunk order; s = that * scale, rounded on its own -- the same bits in the
// forward and in the backward.  Slot s sums its entries in index order; the merge tree is fixed by (bag_len, dim).  A function of the one
// sample only: its bits depend neither on batch nor on its place in the batch.
// Reads: the rows named by in-range ids and row 0; ids, mask, query, out, lse, g_out inside their shapes.  Writes: float4s inside the first
// dim columns of a row of out / g_query (never the padding of a wider stride), lse[b], and the rows of g_rows.
#include "nrx_common.h"
#include <float.h>
#include <math.h>

namespace {

using nrx_u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

constexpr int DN_MAX_LEN = 256;
constexpr int DN_MAX_DIM = 64;
constexpr int DN_WAVES = 4;                    // waves (samples in flight) per workgroup
constexpr int DN_MAX_BLOCKS = 2048;            // 8 workgroups per compute unit; more samples than that are strided
constexpr int64_t DN_MAX_ROWS = 1LL << 30;     // an entry is one word: 30 bits of row, kept, out of range
constexpr uint32_t DN_ROW = (1u << 30) - 1, DN_KEEP = 1u << 30, DN_BAD = 1u << 31;

struct DinArgs {
    const void* table;       // [rows, dim] fp32 or bf16
    const void* ids;         // [batch, len] int32 or int64
    const float* mask;       // [batch, len] or null
    const float* query;      // [batch, q_ld]
    float* out;              // forward: written; backward: read
    float* lse;              // [batch]  forward: written; backward: read
    const float* g_out;      // backward: [batch, g_out_ld]
    float* g_query;          // backward: [batch, g_query_ld]
    float* g_rows;           // backward: [batch * len, dim]
    int32_t* status;
    int64_t rows, batch, q_ld, out_ld, g_out_ld, g_query_ld;
    int32_t dim, len, idx64;
    float scale;
};

struct DinIds {
    uint32_t w[4];           // entries lane, 64 + lane, 128 + lane, 192 + lane of the sample; 0 past the end
};

// the sample's entries, coalesced: row (0 unless the entry is kept and in range) | DN_KEEP | DN_BAD.  All eight loads are issued before the first
// is looked at and none sits behind a branch: a lane past the end reads the last entry again, and without a mask the "weight" is a word of
// the ids themselves (valid memory, never looked at)
template <bool I64>
__device__ __forceinline__ DinIds dn_load_ids(const DinArgs& a, int64_t b, int lane) {
    const int64_t base = b * a.len;
    const bool has_mask = a.mask != nullptr;
    const float* mk = has_mask ? a.mask : reinterpret_cast<const float*>(a.ids);
    int64_t id[4];
    float wt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + min(64 * k + lane, a.len - 1);
        if constexpr (I64) id[k] = reinterpret_cast<const int64_t*>(a.ids)[i];
        else id[k] = (int64_t)reinterpret_cast<const int32_t*>(a.ids)[i];
        wt[k] = mk[i];
    }
    DinIds r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool in = 64 * k + lane < a.len;
        const bool keep = !has_mask || wt[k] != 0.f;
        const bool ok = id[k] >= 0 && id[k] < a.rows;
        if (in && !ok) nrx_report_oob(a.status, 0, b, id[k]);
        r.w[k] = in ? (keep && ok ? (uint32_t)id[k] : 0u) | (keep ? DN_KEEP : 0u) | (ok ? 0u : DN_BAD) : 0u;
    }
    return r;
}

// the word of entry l = t R + slot, from the lane that loaded it (t R / 64 is the same in every lane: R divides 64); 0 past the last step
template <int R>
__device__ __forceinline__ uint32_t dn_entry(const DinIds& ids, int t, int nsteps, int slot) {
    const int k = (t * R) >> 6;
    const uint32_t mine = k == 0 ? ids.w[0] : k == 1 ? ids.w[1] : k == 2 ? ids.w[2] : ids.w[3];
    const uint32_t w = (uint32_t)__shfl((int)mine, (t * R + slot) & 63);
    return t < nsteps ? w : 0u;
}

template <bool BF16>
struct DinRaw;
template <>
struct DinRaw<false> {
    nrx_f32x4 v;
};
template <>
struct DinRaw<true> {
    nrx_u32x2 v;
};

// 4 columns of a row as they lie in memory (widened when they are consumed: the request of step t + 1 is not waited for in step t)
template <bool BF16>
__device__ __forceinline__ DinRaw<BF16> dn_load_row(const void* table, uint32_t row, int dim, int col) {
    DinRaw<BF16> r;
    const int64_t at = (int64_t)row * dim + col;
    if constexpr (BF16) r.v = *(const NRX_GLOBAL nrx_u32x2*)(reinterpret_cast<const uint16_t*>(table) + at);
    else r.v = *(const NRX_GLOBAL nrx_f32x4*)(reinterpret_cast<const float*>(table) + at);
    return r;
}
template <bool BF16>
__device__ __forceinline__ float4 dn_widen(const DinRaw<BF16>& r, bool active) {
    float4 t;
    if constexpr (BF16) t = nrx_bf16x4_to_f32(r.v.x, r.v.y);
    else t = make_float4(r.v.x, r.v.y, r.v.z, r.v.w);
    return make_float4(active ? t.x : 0.f, active ? t.y : 0.f, active ? t.z : 0.f, active ? t.w : 0.f);
}
__device__ __forceinline__ float4 dn_load4(const float* p, bool active) {
    const float4 t = nrx_ldg4(p, 0);
    return make_float4(active ? t.x : 0.f, active ? t.y : 0.f, active ? t.z : 0.f, active ? t.w : 0.f);
}

// sum over the Q lanes of a row, the same bits in each of them: a balanced binary tree in chunk order (data-parallel-primitive moves)
template <int Q>
__device__ __forceinline__ float dn_row_sum(float v) {
    if constexpr (Q >= 2) v += nrx_dpp<0xB1>(v);       // lane ^ 1
    if constexpr (Q >= 4) v += nrx_dpp<0x4E>(v);       // lane ^ 2
    if constexpr (Q >= 8) v += nrx_dpp<0x141>(v);      // the other quad of each 8 (every lane of a quad holds the quad's sum)
    if constexpr (Q >= 16) v += nrx_dpp<0x140>(v);     // the other half of each 16
    return v;
}
template <int Q>
__device__ __forceinline__ float dn_dot(float4 x, float4 e) {
    float c;
    {
#pragma clang fp contract(off)
        c = x.x * e.x;
    }
    c = fmaf(x.y, e.y, c);
    c = fmaf(x.z, e.z, c);
    c = fmaf(x.w, e.w, c);
    return dn_row_sum<Q>(c);
}
// s_l = chain * scale, rounded on its own (never contracted into the subtraction that follows): one value wherever it is formed
__device__ __forceinline__ float dn_score(float chain, float scale) {
#pragma clang fp contract(off)
    return chain * scale;
}

template <int Q, bool BF16, bool I64>
__global__ __launch_bounds__(DN_WAVES * 64) void din_fwd_kernel(const DinArgs a) {
    constexpr int R = 64 / Q;
    const int lane = threadIdx.x & 63;
    const int slot = lane / Q, c4 = 4 * (lane % Q);
    const bool active = c4 < a.dim;
    const int col = active ? c4 : 0;
    const int len = a.len, dim = a.dim;
    const int nsteps = (len + R - 1) / R, nlive = min(len, R);
    const float scale = a.scale;
    const int64_t stride = (int64_t)gridDim.x * DN_WAVES;
    int64_t b = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
    if (b >= a.batch) return;                                  // (the whole wave)
    DinIds cur = dn_load_ids<I64>(a, b, lane);
    for (; b < a.batch; b += stride) {
        DinIds nxt = {};
        if (b + stride < a.batch) nxt = dn_load_ids<I64>(a, b + stride, lane);
        const float4 q = dn_load4(a.query + b * a.q_ld + col, active);
        float m = -FLT_MAX, sum = 0.f;        // (-FLT_MAX, not -inf: exp(m - m) must be 1 while nothing is kept yet)
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        uint32_t w = dn_entry<R>(cur, 0, nsteps, slot);
        DinRaw<BF16> raw = dn_load_row<BF16>(a.table, w & DN_ROW, dim, col);
        for (int t = 0; t < nsteps; ++t) {
            const uint32_t wn = dn_entry<R>(cur, t + 1, nsteps, slot);
            const DinRaw<BF16> rawn = dn_load_row<BF16>(a.table, wn & DN_ROW, dim, col);
            const float4 e = dn_widen<BF16>(raw, active);
            const bool keep = (w & DN_KEEP) != 0;
            const float s = keep ? dn_score(dn_dot<Q>(q, e), scale) : -INFINITY;
            const float mn = fmaxf(m, s);
            const float alpha = expf(m - mn);
            const float p = keep ? expf(s - mn) : 0.f;
            sum = fmaf(sum, alpha, p);
            acc.x = fmaf(p, e.x, acc.x * alpha); acc.y = fmaf(p, e.y, acc.y * alpha);
            acc.z = fmaf(p, e.z, acc.z * alpha); acc.w = fmaf(p, e.w, acc.w * alpha);
            m = mn;
            w = wn;
            raw = rawn;
        }
        // merge the slots: partner = slot ^ 1, ^ 2, ...; a level whose partners of slot 0's group hold no entry is skipped (wave-uniform)
#pragma unroll
        for (int off = Q; off < 64; off <<= 1) {
            if (off / Q >= nlive) continue;
            const float mo = __shfl_xor(m, off), so = __shfl_xor(sum, off);
            const float4 ao = make_float4(__shfl_xor(acc.x, off), __shfl_xor(acc.y, off), __shfl_xor(acc.z, off), __shfl_xor(acc.w, off));
            const float mn = fmaxf(m, mo);
            const float ea = expf(m - mn), eb = expf(mo - mn);
            {
#pragma clang fp contract(off)
                // (products rounded on their own: both partners form the same bits)
                sum = sum * ea + so * eb;
                acc.x = acc.x * ea + ao.x * eb; acc.y = acc.y * ea + ao.y * eb;
                acc.z = acc.z * ea + ao.z * eb; acc.w = acc.w * ea + ao.w * eb;
            }
            m = mn;
        }
        // a kept entry at the running maximum contributes exp(0) = 1: sum == 0 exactly when no entry is kept
        const bool any = sum > 0.f;
        const float inv = any ? 1.f / sum : 0.f;
        if (lane == 0) a.lse[b] = any ? m + logf(sum) : -INFINITY;
        if (slot == 0 && active) nrx_stg4(a.out + b * a.out_ld + c4, 0, make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv));
        cur = nxt;
    }
}

template <int Q, bool BF16, bool I64>
__global__ __launch_bounds__(DN_WAVES * 64) void din_bwd_kernel(const DinArgs a) {
    constexpr int R = 64 / Q;
    const int lane = threadIdx.x & 63;
    const int slot = lane / Q, c4 = 4 * (lane % Q);
    const bool active = c4 < a.dim;
    const int col = active ? c4 : 0;
    const int len = a.len, dim = a.dim;
    const int nsteps = (len + R - 1) / R, nlive = min(len, R);
    const float scale = a.scale;
    const int64_t stride = (int64_t)gridDim.x * DN_WAVES;
    int64_t b = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
    if (b >= a.batch) return;                                  // (the whole wave)
    DinIds cur = dn_load_ids<I64>(a, b, lane);
    for (; b < a.batch; b += stride) {
        DinIds nxt = {};
        if (b + stride < a.batch) nxt = dn_load_ids<I64>(a, b + stride, lane);
        const float4 q = dn_load4(a.query + b * a.q_ld + col, active);
        const float4 go = dn_load4(a.g_out + b * a.g_out_ld + col, active);
        const float4 o = dn_load4(a.out + b * a.out_ld + col, active);
        const float lse = a.lse[b];
        uint32_t w = dn_entry<R>(cur, 0, nsteps, slot);
        DinRaw<BF16> raw = dn_load_row<BF16>(a.table, w & DN_ROW, dim, col);
        const float delta = dn_dot<Q>(go, o);
        float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
        float* grow = a.g_rows + (b * len + slot) * dim + c4;          // entry l = slot of this sample; a step moves it R rows on
        for (int t = 0; t < nsteps; ++t) {
            const uint32_t wn = dn_entry<R>(cur, t + 1, nsteps, slot);
            const DinRaw<BF16> rawn = dn_load_row<BF16>(a.table, wn & DN_ROW, dim, col);
            const float4 e = dn_widen<BF16>(raw, active);
            const bool keep = (w & DN_KEEP) != 0;
            const float s = dn_score(dn_dot<Q>(q, e), scale);
            const float p = keep ? expf(s - lse) : 0.f;                 // (selected, not multiplied: lse is -inf when nothing is kept)
            const float dp = dn_dot<Q>(go, e);
            const float ds = p * (dp - delta);
            gq.x = fmaf(ds, e.x, gq.x); gq.y = fmaf(ds, e.y, gq.y); gq.z = fmaf(ds, e.z, gq.z); gq.w = fmaf(ds, e.w, gq.w);
            const float sds = ds * scale;
            const bool give = keep && (w & DN_BAD) == 0;                // the lookup's own gradient: zeros for an entry that read nothing
            float4 gr;
            {
#pragma clang fp contract(off)
                const float4 pg = make_float4(p * go.x, p * go.y, p * go.z, p * go.w);
                gr = make_float4(give ? fmaf(sds, q.x, pg.x) : 0.f, give ? fmaf(sds, q.y, pg.y) : 0.f, give ? fmaf(sds, q.z, pg.z) : 0.f,
                                 give ? fmaf(sds, q.w, pg.w) : 0.f);
            }
            if (active && t * R + slot < len) nrx_stg4(grow + (int64_t)t * R * dim, 0, gr);
            w = wn;
            raw = rawn;
        }
#pragma unroll
        for (int off = Q; off < 64; off <<= 1) {
            if (off / Q >= nlive) continue;
            gq.x += __shfl_xor(gq.x, off); gq.y += __shfl_xor(gq.y, off); gq.z += __shfl_xor(gq.z, off); gq.w += __shfl_xor(gq.w, off);
        }
        if (slot == 0 && active)
            nrx_stg4(a.g_query + b * a.g_query_ld + c4, 0, make_float4(gq.x * scale, gq.y * scale, gq.z * scale, gq.w * scale));
        cur = nxt;
    }
}

template <bool BWD, int Q, bool BF16, bool I64>
void din_launch3(dim3 grid, hipStream_t st, const DinArgs& a) {
    const dim3 block(DN_WAVES * 64);
    if (BWD) hipLaunchKernelGGL((din_bwd_kernel<Q, BF16, I64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((din_fwd_kernel<Q, BF16, I64>), grid, block, 0, st, a);
}
template <bool BWD, int Q>
void din_launch2(bool bf16, dim3 grid, hipStream_t st, const DinArgs& a) {
    if (bf16) {
        if (a.idx64) din_launch3<BWD, Q, true, true>(grid, st, a);
        else din_launch3<BWD, Q, true, false>(grid, st, a);
    } else {
        if (a.idx64) din_launch3<BWD, Q, false, true>(grid, st, a);
        else din_launch3<BWD, Q, false, false>(grid, st, a);
    }
}
template <bool BWD>
void din_launch(int dim, bool bf16, dim3 grid, hipStream_t st, const DinArgs& a) {
    if (dim <= 4) din_launch2<BWD, 1>(bf16, grid, st, a);
    else if (dim <= 8) din_launch2<BWD, 2>(bf16, grid, st, a);
    else if (dim <= 16) din_launch2<BWD, 4>(bf16, grid, st, a);
    else if (dim <= 32) din_launch2<BWD, 8>(bf16, grid, st, a);
    else din_launch2<BWD, 16>(bf16, grid, st, a);
}

bool dn_f32_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the checks both entry points share; NRX_OK or the status to return
int din_check(const char* who, const void* table, int64_t rows, int32_t dim, int32_t flags, const void* ids, int32_t index_bits, const float* mask,
              const float* query, int64_t q_ld, int64_t batch, int32_t bag_len, float scale, const float* out, int64_t out_ld, const float* lse,
              const int32_t* status) {
    NRX_REQUIRE(batch >= 0 && bag_len >= 1 && dim >= 1 && rows >= 1, "%s: bad argument (batch %lld, bag_len %d, dim %d, rows %lld)", who,
                (long long)batch, bag_len, dim, (long long)rows);
    NRX_REQUIRE(index_bits == 32 || index_bits == 64, "%s: bad argument (index_bits %d: 32 or 64)", who, index_bits);
    NRX_REQUIRE((flags & ~1) == 0, "%s: bad argument (flags %d: bit 0 = bf16 table is the only one defined)", who, flags);
    NRX_REQUIRE(scale == scale && fabsf(scale) <= FLT_MAX, "%s: bad argument (scale must be finite)", who);
    NRX_REQUIRE(q_ld >= dim && out_ld >= dim, "%s: bad argument (row stride below dim: q_ld %lld or out_ld %lld < %d)", who, (long long)q_ld,
                (long long)out_ld, dim);
    if (batch > 0) {
        NRX_REQUIRE(table && ids && query && out && lse, "%s: null buffer", who);
        NRX_REQUIRE((reinterpret_cast<uintptr_t>(table) & ((flags & 1) ? 7u : 15u)) == 0 && nrx_aligned16(query) && nrx_aligned16(out) &&
                        (q_ld & 3) == 0 && (out_ld & 3) == 0,
                    "%s: misaligned rows (table / query / out and their row strides must keep every row 16-byte aligned; bf16 table rows 8-byte)", who);
        NRX_REQUIRE((reinterpret_cast<uintptr_t>(ids) & (index_bits == 64 ? 7u : 3u)) == 0 && dn_f32_ok(mask) && dn_f32_ok(lse) && dn_f32_ok(status),
                    "%s: misaligned pointer", who);
    }
    if ((dim & 3) != 0 || dim > DN_MAX_DIM || bag_len > DN_MAX_LEN || rows > DN_MAX_ROWS) {
        nrx_set_error("%s: supports dim %% 4 == 0 in 4..%d, bag_len 1..%d and rows <= 2^30 (got dim=%d, bag_len=%d, rows=%lld)", who, DN_MAX_DIM,
                      DN_MAX_LEN, dim, bag_len, (long long)rows);
        return NRX_ERR_UNSUPPORTED;
    }
    return NRX_OK;
}

dim3 din_grid(int64_t batch) {
    const int64_t blocks = (batch + DN_WAVES - 1) / DN_WAVES;
    return dim3((unsigned)(blocks < DN_MAX_BLOCKS ? blocks : DN_MAX_BLOCKS));
}

}  // namespace

extern "C" int nrx_din_pool_fwd(const void* table, int64_t rows, int32_t dim, int32_t flags, const void* ids, int32_t index_bits, const float* mask,
                                const float* query, int64_t q_ld, int64_t batch, int32_t bag_len, float scale, float* out, int64_t out_ld,
                                float* lse, int32_t* status, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_din_pool_fwd";
    const int rc = din_check(who, table, rows, dim, flags, ids, index_bits, mask, query, q_ld, batch, bag_len, scale, out, out_ld, lse, status);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    DinArgs a = {};
    a.table = table; a.ids = ids; a.mask = mask; a.query = query; a.out = out; a.lse = lse; a.status = status;
    a.rows = rows; a.batch = batch; a.q_ld = q_ld; a.out_ld = out_ld;
    a.dim = dim; a.len = bag_len; a.idx64 = index_bits == 64; a.scale = scale;
    din_launch<false>(dim, (flags & 1) != 0, din_grid(batch), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

extern "C" int nrx_din_pool_bwd(const void* table, int64_t rows, int32_t dim, int32_t flags, const void* ids, int32_t index_bits, const float* mask,
                                const float* query, int64_t q_ld, int64_t batch, int32_t bag_len, float scale, const float* out, int64_t out_ld,
                                const float* lse, const float* g_out, int64_t g_out_ld, float* g_query, int64_t g_query_ld, float* g_rows,
                                void* stream) {
    NRX_TRACE();
    const char* who = "nrx_din_pool_bwd";
    NRX_REQUIRE(dim < 1 || (g_out_ld >= dim && g_query_ld >= dim), "%s: bad argument (row stride below dim: g_out_ld %lld or g_query_ld %lld < %d)", who,
                (long long)g_out_ld, (long long)g_query_ld, dim);
    if (batch > 0) {
        NRX_REQUIRE(g_out && g_query && g_rows, "%s: null buffer", who);
        NRX_REQUIRE(nrx_aligned16(g_out) && nrx_aligned16(g_query) && nrx_aligned16(g_rows) && (g_out_ld & 3) == 0 && (g_query_ld & 3) == 0,
                    "%s: misaligned rows (g_out / g_query / g_rows and their row strides must keep every row 16-byte aligned)", who);
    }
    const int rc = din_check(who, table, rows, dim, flags, ids, index_bits, mask, query, q_ld, batch, bag_len, scale, out, out_ld, lse, nullptr);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    DinArgs a = {};
    a.table = table; a.ids = ids; a.mask = mask; a.query = query; a.out = const_cast<float*>(out); a.lse = const_cast<float*>(lse);
    a.g_out = g_out; a.g_query = g_query; a.g_rows = g_rows;
    a.rows = rows; a.batch = batch; a.q_ld = q_ld; a.out_ld = out_ld; a.g_out_ld = g_out_ld; a.g_query_ld = g_query_ld;
    a.dim = dim; a.len = bag_len; a.idx64 = index_bits == 64; a.scale = scale;
    din_launch<true>(dim, (flags & 1) != 0, din_grid(batch), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}
