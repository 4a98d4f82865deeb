// The data-parallel gradient of REPLICATED tables in the bound sharded step (shard_step.PreparedShardedStep(replicated_grads=True)): small
// tables held in full on every rank, whose row-sparse gradients every rank must end with identically -- same keys, same bits.  A dense
// reduce-scatter by chunks with a FIXED summation order, then an all-gather (no RCCL all-reduce: its order is not ours to fix):
//
//   pack         the local (keys, values) lists -> one dense buffer of `world` chunks [C = cf + cr words]: the gradient floats of every
//                replicated table (+0.0 where this rank looked nothing up) and an int32 touch count per row
//   all-to-all   equal splits: rank q receives chunk q of every rank
//   ordered sum  s = G_0; s = s + G_1; ...; s = s + G_{W-1} per float (rank order), counts added
//   all-gather   every rank holds the reduced buffer
//   compact      rows with count > 0 -> (keys, values) in row order, the count on the device
//
// Layout: float element i of the flat gradient (table t's (row, col): i = voff[t] + row * dim[t] + col) lives at word (i / cf) * C + i % cf;
// the touch count of row j (j = roff[t] + row) at word (j / cr) * C + cf + j % cr.  Definitions: tests/test_replicated_grads_gloo.py (numpy).
// No float atomics, no host reads; every store is a plain vector store.  No reference counterpart (the reference is single-device:
// src/model/sort/deep/train.py:38-44).
#include "nrx_common.h"

namespace {

constexpr int REP_MAX_LISTS = 8;
constexpr int REP_MAX_TABLES = NRX_MAX_FEATURES;
constexpr int REP_TILE = NRX_BLOCK;               // rows per block of the compaction (one per thread)
constexpr int64_t REP_ROW_MASK = (int64_t(1) << 40) - 1;

struct RepTables {
    int64_t voff[REP_MAX_TABLES];
    int64_t roff[REP_MAX_TABLES];
    int64_t rows[REP_MAX_TABLES];
    int32_t dim[REP_MAX_TABLES];
    int32_t key_table[REP_MAX_TABLES];
    int32_t n;
};

struct RepLists {
    const int64_t* keys[REP_MAX_LISTS];
    const float* values[REP_MAX_LISTS];
    const int64_t* n_keys[REP_MAX_LISTS];
    int64_t cap[REP_MAX_LISTS];
    int32_t dim[REP_MAX_LISTS];
};

// word of float element base + c, from base's chunk q0 = base / cf and offset r0 = base % cf (one 64-bit division per row, not per element)
__device__ __forceinline__ int64_t float_word_from(int64_t q0, int64_t r0, int c, int64_t cf, int64_t C) {
    int64_t q = q0, r = r0 + c;
    while (r >= cf) {
        r -= cf;
        ++q;
    }
    return q * C + r;
}

__device__ __forceinline__ int64_t count_word(int64_t j, int64_t cf, int64_t cr, int64_t C) {
    const int64_t q = j / cr;
    return q * C + cf + (j - q * cr);
}

// one wavefront per local key; list = blockIdx.y.  The buffer was zeroed before (nrx_zero_async).
__global__ __launch_bounds__(NRX_BLOCK) void rep_pack_kernel(RepLists L, RepTables T, int64_t cf, int64_t cr, int64_t C, float* __restrict__ buf) {
    const int li = blockIdx.y;
    const int64_t cap = L.cap[li];
    int64_t n = *L.n_keys[li];
    if (n > cap) n = cap;
    const int D = L.dim[li];
    const int lane = threadIdx.x & 63;
    const int64_t* __restrict__ keys = L.keys[li];
    const float* __restrict__ vals = L.values[li];
    int32_t* __restrict__ words = reinterpret_cast<int32_t*>(buf);
    for (int64_t k = (int64_t)blockIdx.x * (NRX_BLOCK / 64) + (threadIdx.x >> 6); k < n; k += (int64_t)gridDim.x * (NRX_BLOCK / 64)) {
        const int64_t key = keys[k];
        const int64_t t = key >> 40, row = key & REP_ROW_MASK;
        if (key < 0 || t >= T.n || row >= T.rows[t] || T.dim[t] != D) continue;     // (not a row of this layout: nothing to write)
        const float* src = vals + k * D;
        const int64_t base = T.voff[t] + row * D;
        const int64_t q0 = base / cf, r0 = base - q0 * cf;
        for (int c = lane; c < D; c += 64) buf[float_word_from(q0, r0, c, cf, C)] = src[c];
        if (lane == 0) words[count_word(T.roff[t] + row, cf, cr, C)] = 1;
    }
}

// out[w] = recv[0][w] + recv[1][w] + ... in rank order (floats: w < cf), the int32 sum of the counts (w >= cf).  16 bytes per lane.
__global__ __launch_bounds__(NRX_BLOCK) void rep_sum_kernel(const nrx_f32x4* __restrict__ recv, int world, int64_t C4, int64_t cf4,
                                                            nrx_f32x4* __restrict__ out) {
    for (int64_t w = (int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x; w < C4; w += (int64_t)gridDim.x * NRX_BLOCK) {
        if (w < cf4) {
            nrx_f32x4 s = recv[w];
            for (int r = 1; r < world; ++r) {
                const nrx_f32x4 x = recv[r * C4 + w];
                s.x = s.x + x.x;
                s.y = s.y + x.y;
                s.z = s.z + x.z;
                s.w = s.w + x.w;
            }
            out[w] = s;
        } else {
            const int4* ri = reinterpret_cast<const int4*>(recv);
            int4 s = ri[w];
            for (int r = 1; r < world; ++r) {
                const int4 x = ri[r * C4 + w];
                s.x += x.x;
                s.y += x.y;
                s.z += x.z;
                s.w += x.w;
            }
            reinterpret_cast<int4*>(out)[w] = s;
        }
    }
}

__device__ __forceinline__ int table_of_row(const RepTables& T, int64_t j) {
    int t = 0;
    while (t + 1 < T.n && j >= T.roff[t + 1]) ++t;
    return t;
}

// compaction, pass 1: touched rows per tile of REP_TILE rows of [row_lo, row_lo + n_rows)
__global__ __launch_bounds__(NRX_BLOCK) void rep_tile_count_kernel(const float* __restrict__ full, int64_t cf, int64_t cr, int64_t C, int64_t row_lo,
                                                                   int64_t n_rows, int32_t* __restrict__ tile_cnt) {
    __shared__ int s_w[NRX_BLOCK / 64];
    const int32_t* words = reinterpret_cast<const int32_t*>(full);
    const int64_t j0 = (int64_t)blockIdx.x * REP_TILE + threadIdx.x;
    int v = j0 < n_rows && words[count_word(row_lo + j0, cf, cr, C)] > 0;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < NRX_BLOCK / 64; ++w) s += s_w[w];
        tile_cnt[blockIdx.x] = s;
    }
}

// compaction, pass 2: the block's place = the touched rows of the tiles before it; a block scan orders its own rows; keys, then the rows' values
__global__ __launch_bounds__(NRX_BLOCK) void rep_emit_kernel(const float* __restrict__ full, int64_t cf, int64_t cr, int64_t C, RepTables T,
                                                             int64_t row_lo, int64_t n_rows, int32_t dim, const int32_t* __restrict__ tile_cnt,
                                                             int64_t n_tiles, int64_t* __restrict__ keys, float* __restrict__ values, int64_t cap,
                                                             int64_t* __restrict__ n_out) {
    __shared__ int64_t s_red[NRX_BLOCK / 64];
    __shared__ int s_wsum[NRX_BLOCK / 64];
    __shared__ int64_t s_q[REP_TILE];
    __shared__ int64_t s_r[REP_TILE];
    __shared__ int64_t s_dst[REP_TILE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int32_t* words = reinterpret_cast<const int32_t*>(full);
    // before = sum of tile_cnt[0 .. blockIdx.x); block 0 also forms the total (the device-side count)
    const int64_t upto = blockIdx.x == 0 ? n_tiles : (int64_t)blockIdx.x;
    int64_t acc = 0;
    for (int64_t i = threadIdx.x; i < upto; i += NRX_BLOCK) acc += tile_cnt[i];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) s_red[wid] = acc;
    __syncthreads();
    int64_t red = 0;
    for (int w = 0; w < NRX_BLOCK / 64; ++w) red += s_red[w];
    const int64_t before = blockIdx.x == 0 ? 0 : red;
    if (blockIdx.x == 0 && threadIdx.x == 0) n_out[0] = red;
    // this thread's row: a block scan of the flags gives its place
    const int64_t jl = (int64_t)blockIdx.x * REP_TILE + threadIdx.x;
    const int flag = jl < n_rows && words[count_word(row_lo + jl, cf, cr, C)] > 0;
    int incl = flag;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wsum[wid] = incl;
    __syncthreads();
    int wbase = 0, total = 0;
    for (int w = 0; w < NRX_BLOCK / 64; ++w) {
        if (w < wid) wbase += s_wsum[w];
        total += s_wsum[w];
    }
    const int local = wbase + incl - flag;
    if (flag) {
        const int64_t j = row_lo + jl;
        const int t = table_of_row(T, j);
        const int64_t row = j - T.roff[t];
        const int64_t pos = before + local;
        if (pos < cap) keys[pos] = ((int64_t)T.key_table[t] << 40) | row;
        const int64_t base = T.voff[t] + row * dim;
        s_q[local] = base / cf;
        s_r[local] = base - s_q[local] * cf;
        s_dst[local] = pos;
    }
    __syncthreads();
    // the touched rows' values: one wavefront per row, lanes over the columns
    for (int r = wid; r < total; r += NRX_BLOCK / 64) {
        const int64_t pos = s_dst[r], q0 = s_q[r], r0 = s_r[r];
        if (pos >= cap) continue;
        for (int c = lane; c < dim; c += 64) values[pos * dim + c] = full[float_word_from(q0, r0, c, cf, C)];
    }
}

int fill_tables(RepTables& T, const int64_t* voff, const int64_t* roff, const int64_t* rows, const int32_t* dims, const int32_t* key_table,
                int32_t n_tables, int64_t nf, int64_t nr, const char* what) {
    NRX_REQUIRE(n_tables >= 1 && n_tables <= REP_MAX_TABLES, "%s: 1 .. %d tables", what, REP_MAX_TABLES);
    NRX_REQUIRE(voff && roff && rows && dims, "%s: null table arrays", what);
    T.n = n_tables;
    for (int t = 0; t < n_tables; ++t) {
        NRX_REQUIRE(voff[t] >= 0 && roff[t] >= 0 && rows[t] >= 0 && dims[t] >= 1 && voff[t] + rows[t] * dims[t] <= nf && roff[t] + rows[t] <= nr,
                    "%s: table %d lies outside the buffer", what, t);
        T.voff[t] = voff[t];
        T.roff[t] = roff[t];
        T.rows[t] = rows[t];
        T.dim[t] = dims[t];
        T.key_table[t] = key_table ? key_table[t] : t;
    }
    return NRX_OK;
}

}  // namespace

extern "C" int nrx_rep_pack(const int64_t* const* keys, const float* const* values, const int64_t* const* n_keys, const int64_t* caps,
                            const int32_t* dims, int32_t n_lists, const int64_t* voff, const int64_t* roff, const int64_t* rows,
                            const int32_t* tdims, int32_t n_tables, int32_t world, int64_t cf, int64_t cr, float* buf, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n_lists >= 0 && n_lists <= REP_MAX_LISTS, "nrx_rep_pack: 0 .. %d lists", REP_MAX_LISTS);
    NRX_REQUIRE(world >= 1 && cf >= 4 && cr >= 4 && (cf & 3) == 0 && (cr & 3) == 0, "nrx_rep_pack: cf, cr must be positive multiples of 4");
    NRX_REQUIRE(buf != nullptr && nrx_aligned16(buf), "nrx_rep_pack: 16-byte aligned buffer");
    RepTables T;
    int rc = fill_tables(T, voff, roff, rows, tdims, nullptr, n_tables, (int64_t)world * cf, (int64_t)world * cr, "nrx_rep_pack");
    if (rc) return rc;
    const int64_t C = cf + cr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    rc = nrx_zero_async(buf, (size_t)(world * C) * 4, st);
    if (rc) return rc;
    if (n_lists == 0) return NRX_OK;
    RepLists L;
    int64_t maxcap = 0;
    for (int i = 0; i < n_lists; ++i) {
        NRX_REQUIRE(keys && values && n_keys && caps && dims && keys[i] && values[i] && n_keys[i] && caps[i] >= 0 && dims[i] >= 1,
                    "nrx_rep_pack: list %d is incomplete", i);
        L.keys[i] = keys[i];
        L.values[i] = values[i];
        L.n_keys[i] = n_keys[i];
        L.cap[i] = caps[i];
        L.dim[i] = dims[i];
        if (caps[i] > maxcap) maxcap = caps[i];
    }
    int64_t blocks = (maxcap + NRX_BLOCK / 64 - 1) / (NRX_BLOCK / 64);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(rep_pack_kernel, dim3((unsigned)blocks, (unsigned)n_lists), dim3(NRX_BLOCK), 0, st, L, T, cf, cr, C, buf);
    NRX_LAUNCH_CHECK("nrx_rep_pack");
    return NRX_OK;
}

extern "C" int nrx_rep_ordered_sum(const float* recv, int32_t world, int64_t cf, int64_t cr, float* out, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(recv != nullptr && out != nullptr && nrx_aligned16(recv) && nrx_aligned16(out), "nrx_rep_ordered_sum: 16-byte aligned buffers");
    NRX_REQUIRE(world >= 1 && cf >= 4 && cr >= 4 && (cf & 3) == 0 && (cr & 3) == 0, "nrx_rep_ordered_sum: cf, cr must be positive multiples of 4");
    const int64_t C4 = (cf + cr) / 4;
    int64_t blocks = (C4 + NRX_BLOCK - 1) / NRX_BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rep_sum_kernel, dim3((unsigned)blocks), dim3(NRX_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const nrx_f32x4*>(recv), (int)world, C4, cf / 4, reinterpret_cast<nrx_f32x4*>(out));
    NRX_LAUNCH_CHECK("nrx_rep_ordered_sum");
    return NRX_OK;
}

extern "C" int64_t nrx_rep_compact_workspace(int64_t n_rows) {
    return n_rows < 0 ? -1 : ((n_rows + REP_TILE - 1) / REP_TILE + 1) * 4;
}

extern "C" int nrx_rep_compact(const float* full, int32_t world, int64_t cf, int64_t cr, const int64_t* voff, const int64_t* roff,
                               const int64_t* rows, const int32_t* key_table, int32_t n_tables, int32_t dim, int64_t* keys, float* values,
                               int64_t cap, int64_t* n_out, void* workspace, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(full != nullptr && keys != nullptr && values != nullptr && n_out != nullptr && workspace != nullptr, "nrx_rep_compact: null buffer");
    NRX_REQUIRE(world >= 1 && cf >= 4 && cr >= 4 && (cf & 3) == 0 && (cr & 3) == 0 && dim >= 1, "nrx_rep_compact: bad layout");
    NRX_REQUIRE(key_table != nullptr, "nrx_rep_compact: null key_table");
    int32_t dims[REP_MAX_TABLES];
    for (int t = 0; t < n_tables && t < REP_MAX_TABLES; ++t) dims[t] = dim;
    RepTables T;
    int rc = fill_tables(T, voff, roff, rows, dims, key_table, n_tables, (int64_t)world * cf, (int64_t)world * cr, "nrx_rep_compact");
    if (rc) return rc;
    for (int t = 1; t < n_tables; ++t)
        NRX_REQUIRE(roff[t] == roff[t - 1] + rows[t - 1], "nrx_rep_compact: the tables of one call must be adjacent rows of the layout");
    const int64_t row_lo = roff[0];
    const int64_t n_rows = roff[n_tables - 1] + rows[n_tables - 1] - row_lo;
    NRX_REQUIRE(cap >= n_rows, "nrx_rep_compact: cap %lld < %lld rows", (long long)cap, (long long)n_rows);
    const int64_t C = cf + cr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_tiles = (n_rows + REP_TILE - 1) / REP_TILE;
    int32_t* tile_cnt = reinterpret_cast<int32_t*>(workspace);
    if (n_tiles == 0) return nrx_zero_async(n_out, 8, st);
    hipLaunchKernelGGL(rep_tile_count_kernel, dim3((unsigned)n_tiles), dim3(NRX_BLOCK), 0, st, full, cf, cr, C, row_lo, n_rows, tile_cnt);
    NRX_LAUNCH_CHECK("nrx_rep_compact");
    hipLaunchKernelGGL(rep_emit_kernel, dim3((unsigned)n_tiles), dim3(NRX_BLOCK), 0, st, full, cf, cr, C, T, row_lo, n_rows, dim, tile_cnt, n_tiles,
                       keys, values, cap, n_out);
    NRX_LAUNCH_CHECK("nrx_rep_compact");
    return NRX_OK;
}
