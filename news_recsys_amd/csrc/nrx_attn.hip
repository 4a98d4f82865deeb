// Self-attention over a short sequence (seq <= 128), forward and backward, with nothing of size seq^2 outside the compute unit.
// Reference counterpart: the core of MultiHeadSelfAttention.forward (src/model/model_utils/utils.py:31-40) -- softmax(q k^T / sqrt(hd)) v
// per head -- read in place from what qkv_proj gives and written in the layout out_proj takes; the key mask is this project's addition.
//
// Definition (include/nrx_embed.h restates it): s_ij = dot(q_i, k_j) * scale; key j of sample b is kept iff key_mask[b, j] != 0;
// p_ij = softmax over the kept j; out_i = sum_j p_ij v_j; row_lse_i = log sum_kept exp(s_ij).  Backward, with delta_i = dot(g_out_i, out_i):
// dV = P^T g_out, dP = g_out V^T, dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q; s and p are recomputed from qkv and row_lse.
//
// Tiling: ONE WORKGROUP OWNS ONE (sample, head); thread t owns row t of it (64 threads for seq <= 64, else 128).  The other side is staged
// in LDS in tiles of 64 rows ([64, HD] fp32, HD = head_dim padded to 4, 8, 12, 16, 32 or 64 with zeros) and every lane reads the SAME row of
// it at a time: a broadcast read, free of bank conflicts whatever HD is.  The arithmetic is VALU fma chains: at the history shape
// (seq 50, head_dim 8) a 16- or 32-row matrix-core tile would idle most of its rows on padding and the launch is bound by its bytes.
//   forward : thread i keeps q_i and the accumulator o_i; keys are taken 4 at a time with a running maximum (one rescale of o_i per 4 keys);
//             chunks whose 4 keys are all masked are skipped (block-uniform branch).
//   backward: phase A, thread i keeps q_i, g_out_i and dq_i and streams K, V tiles; delta_i goes to LDS.  Phase B, thread j keeps k_j, v_j and
//             the accumulators dk_j, dv_j (in slices of 32 columns at HD 64: registers) and streams Q, g_out tiles with lse_i and delta_i.
//             Each gradient row has one owner: no atomics, no cross-block reduction, no workspace.
// Summation order: a score is two fma chains, over the even and over the odd e, added, then * scale (the same bits in all three places it is formed); sums over keys
// or queries run in index order (forward: 4 keys added pairwise, then to the running sum).  A function of (seq, heads, head_dim, mask) of
// the one sample only: a sample's bits do not depend on the batch around it.
// Reads: rows of the tensors named, clamped to the last row where a tile or a thread passes the end.  Writes: whole float4s inside
// [h * hd, (h + 1) * hd) of a row, never the padding of a wider stride.
#include "nrx_common.h"
#include <float.h>
#include <math.h>

namespace {

using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int AT_TILE = 64;          // rows of a staged tile
constexpr int AT_MAX_SEQ = 128;
constexpr int AT_MAX_C = 256;

struct AttnArgs {
    const float* qkv;        // [batch, seq, qkv_ld]
    const float* mask;       // [batch, seq] or null
    float* out;              // forward: written; backward: read
    float* lse;              // [batch, heads, seq]  forward: written; backward: read
    const float* g_out;      // backward: [batch, seq, g_out_ld]
    float* g_qkv;            // backward: [batch, seq, g_qkv_ld]
    int64_t qkv_ld, out_ld, g_out_ld, g_qkv_ld;
    int32_t seq, heads, hd;
    float scale;
};

// s_ij = chain * scale, rounded on its own (never contracted into the subtraction that follows): one value wherever it is formed
__device__ __forceinline__ float at_score(float chain, float scale) {
#pragma clang fp contract(off)
    return chain * scale;
}
__device__ __forceinline__ float at_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

__device__ __forceinline__ float4 at_sel(bool ok, float4 t) { return make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f); }

// rows t0 .. t0 + nrows - 1 (clamped to seq - 1) of one head's columns of two tensors -> dst_a, dst_b [nrows, HD]; columns >= hd are zeros.
// A thread's four loads of a pass (two chunks of each tensor) are issued before any of them is stored: one memory latency per pass, and
// the history shape (50 rows of 8 columns on 64 threads) is one pass.
template <int HD>
__device__ __forceinline__ void at_stage2(float* dst_a, const float* src_a, int64_t ld_a, float* dst_b, const float* src_b, int64_t ld_b, int t0,
                                          int nrows, int seq, int hd) {
    constexpr int CH = HD / 4;
    const int total = nrows * CH, step = blockDim.x;
    for (int c0 = threadIdx.x; c0 < total; c0 += 2 * step) {
        const bool two = c0 + step < total;
        const int c1 = two ? c0 + step : c0;
        const int row0 = c0 / CH, ch0 = c0 % CH, row1 = c1 / CH, ch1 = c1 % CH;
        const int y0 = min(t0 + row0, seq - 1), y1 = min(t0 + row1, seq - 1);
        const bool ok0 = 4 * ch0 < hd, ok1 = 4 * ch1 < hd;
        const float4 a0 = nrx_ldg4(src_a + (int64_t)y0 * ld_a + (ok0 ? 4 * ch0 : 0), 0);
        const float4 b0 = nrx_ldg4(src_b + (int64_t)y0 * ld_b + (ok0 ? 4 * ch0 : 0), 0);
        const float4 a1 = nrx_ldg4(src_a + (int64_t)y1 * ld_a + (ok1 ? 4 * ch1 : 0), 0);
        const float4 b1 = nrx_ldg4(src_b + (int64_t)y1 * ld_b + (ok1 ? 4 * ch1 : 0), 0);
        *reinterpret_cast<float4*>(&dst_a[row0 * HD + 4 * ch0]) = at_sel(ok0, a0);
        *reinterpret_cast<float4*>(&dst_b[row0 * HD + 4 * ch0]) = at_sel(ok0, b0);
        if (two) {
            *reinterpret_cast<float4*>(&dst_a[row1 * HD + 4 * ch1]) = at_sel(ok1, a1);
            *reinterpret_cast<float4*>(&dst_b[row1 * HD + 4 * ch1]) = at_sel(ok1, b1);
        }
    }
}

template <int HD>
__device__ __forceinline__ void at_load_row(float* r, const float* src, int hd) {
#pragma unroll
    for (int v = 0; v < HD / 4; ++v) {
        const bool ok = 4 * v < hd;
        const float4 t = nrx_ldg4(src + (ok ? 4 * v : 0), 0);
        r[4 * v + 0] = ok ? t.x : 0.f; r[4 * v + 1] = ok ? t.y : 0.f;
        r[4 * v + 2] = ok ? t.z : 0.f; r[4 * v + 3] = ok ? t.w : 0.f;
    }
}

template <int HD>
__device__ __forceinline__ float at_dot(const float* r, const float* lds_row) {
    // two fma chains side by side -- the even elements and the odd ones -- so that the pair is one packed instruction (v_pk_fma_f32)
    f32x2 acc = {0.f, 0.f};
#pragma unroll
    for (int v = 0; v < HD / 4; ++v) {
        const float4 t = *reinterpret_cast<const float4*>(&lds_row[4 * v]);
        acc = __builtin_elementwise_fma(f32x2{r[4 * v + 0], r[4 * v + 1]}, f32x2{t.x, t.y}, acc);
        acc = __builtin_elementwise_fma(f32x2{r[4 * v + 2], r[4 * v + 3]}, f32x2{t.z, t.w}, acc);
    }
    return acc.x + acc.y;
}

// 1.0 = key kept, 0.0 = masked or past the end; every index below blockDim.x is written
__device__ __forceinline__ void at_stage_mask(float* km_s, const float* mask, int64_t b, int seq) {
    const int t = threadIdx.x;
    float keep = t < seq ? 1.f : 0.f;
    if (mask != nullptr && t < seq) keep = mask[b * seq + t] != 0.f ? 1.f : 0.f;
    km_s[t] = keep;
}

template <int HD>
__global__ __launch_bounds__(AT_MAX_SEQ) void attn_fwd_kernel(const AttnArgs a) {
    __shared__ __attribute__((aligned(16))) float k_s[AT_TILE * HD];
    __shared__ __attribute__((aligned(16))) float v_s[AT_TILE * HD];
    __shared__ __attribute__((aligned(16))) float km_s[AT_MAX_SEQ];

    const int tid = threadIdx.x;
    const int seq = a.seq, hd = a.hd, C = a.heads * hd;
    const int64_t b = blockIdx.x / a.heads;
    const int h = blockIdx.x % a.heads;
    const float scale = a.scale;
    const bool live = tid < seq;
    const int i = live ? tid : seq - 1;
    const float* base = a.qkv + b * seq * a.qkv_ld + h * hd;

    at_stage_mask(km_s, a.mask, b, seq);
    float q[HD], o[HD];
    at_load_row<HD>(q, base + (int64_t)i * a.qkv_ld, hd);
#pragma unroll
    for (int e = 0; e < HD; ++e) o[e] = 0.f;
    float m = -FLT_MAX, sum = 0.f;        // (-FLT_MAX, not -inf: exp(m - m) must be 1 while nothing is kept yet)

    for (int t0 = 0; t0 < seq; t0 += AT_TILE) {
        const int nt = min(AT_TILE, seq - t0), nr = (nt + 3) & ~3;
        __syncthreads();                  // the previous tile has been read by every wave (first pass: km_s is written)
        at_stage2<HD>(k_s, base + C, a.qkv_ld, v_s, base + 2 * C, a.qkv_ld, t0, nr, seq, hd);
        __syncthreads();
        for (int j = 0; j < nr; j += 4) {
            const float4 kf = *reinterpret_cast<const float4*>(&km_s[t0 + j]);
            if (kf.x == 0.f && kf.y == 0.f && kf.z == 0.f && kf.w == 0.f) continue;      // block-uniform
            const float keep[4] = {kf.x, kf.y, kf.z, kf.w};
            float s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float sc = at_score(at_dot<HD>(q, &k_s[(j + u) * HD]), scale);
                s[u] = keep[u] != 0.f ? sc : -INFINITY;
            }
            const float mn = fmaxf(m, fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])));
            const float alpha = at_exp(m - mn);
            float p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = at_exp(s[u] - mn);
            sum = sum * alpha + ((p[0] + p[1]) + (p[2] + p[3]));
            m = mn;
#pragma unroll
            for (int v = 0; v < HD / 4; ++v) {
                float4 acc = make_float4(o[4 * v] * alpha, o[4 * v + 1] * alpha, o[4 * v + 2] * alpha, o[4 * v + 3] * alpha);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 t = *reinterpret_cast<const float4*>(&v_s[(j + u) * HD + 4 * v]);
                    acc.x = fmaf(p[u], t.x, acc.x); acc.y = fmaf(p[u], t.y, acc.y);
                    acc.z = fmaf(p[u], t.z, acc.z); acc.w = fmaf(p[u], t.w, acc.w);
                }
                o[4 * v] = acc.x; o[4 * v + 1] = acc.y; o[4 * v + 2] = acc.z; o[4 * v + 3] = acc.w;
            }
        }
    }

    if (!live) return;
    // a kept key at the running maximum contributes exp(0) = 1: sum == 0 exactly when no key is kept
    const bool any = sum > 0.f;
    const float inv = any ? 1.f / sum : 0.f;
    a.lse[(b * a.heads + h) * seq + i] = any ? m + logf(sum) : -INFINITY;
    float* op = a.out + (b * seq + i) * a.out_ld + h * hd;
#pragma unroll
    for (int v = 0; v < HD / 4; ++v)
        if (4 * v < hd) nrx_stg4(op + 4 * v, 0, make_float4(o[4 * v] * inv, o[4 * v + 1] * inv, o[4 * v + 2] * inv, o[4 * v + 3] * inv));
}

template <int HD>
__global__ __launch_bounds__(AT_MAX_SEQ) void attn_bwd_kernel(const AttnArgs a) {
    constexpr int EH = HD > 32 ? 32 : HD;         // columns of dk_j, dv_j a thread accumulates per pass of phase B
    __shared__ __attribute__((aligned(16))) float a_s[AT_TILE * HD];      // phase A: K tile; phase B: Q tile
    __shared__ __attribute__((aligned(16))) float b_s[AT_TILE * HD];      // phase A: V tile; phase B: g_out tile
    __shared__ float km_s[AT_MAX_SEQ];
    __shared__ float lse_s[AT_MAX_SEQ];
    __shared__ float delta_s[AT_MAX_SEQ];

    const int tid = threadIdx.x;
    const int seq = a.seq, hd = a.hd, C = a.heads * hd;
    const int64_t b = blockIdx.x / a.heads;
    const int h = blockIdx.x % a.heads;
    const float scale = a.scale;
    const bool live = tid < seq;
    const int i = live ? tid : seq - 1;
    const float* base = a.qkv + b * seq * a.qkv_ld + h * hd;
    const float* gbase = a.g_out + b * seq * a.g_out_ld + h * hd;
    float* gq = a.g_qkv + (b * seq + i) * a.g_qkv_ld + h * hd;

    at_stage_mask(km_s, a.mask, b, seq);
    const float my_lse = a.lse[(b * a.heads + h) * seq + i];
    lse_s[tid] = my_lse;

    // ---- phase A: dq_i = scale sum_j p_ij (dP_ij - delta_i) k_j
    {
        float q[HD], go[HD], dq[HD];
        at_load_row<HD>(q, base + (int64_t)i * a.qkv_ld, hd);
        at_load_row<HD>(go, gbase + (int64_t)i * a.g_out_ld, hd);
        at_load_row<HD>(dq, a.out + (b * seq + i) * a.out_ld + h * hd, hd);       // out_i, for delta_i only
        float delta = 0.f;
#pragma unroll
        for (int e = 0; e < HD; ++e) delta = fmaf(go[e], dq[e], delta);
        delta_s[tid] = delta;
#pragma unroll
        for (int e = 0; e < HD; ++e) dq[e] = 0.f;

        for (int t0 = 0; t0 < seq; t0 += AT_TILE) {
            const int nt = min(AT_TILE, seq - t0);
            __syncthreads();
            at_stage2<HD>(a_s, base + C, a.qkv_ld, b_s, base + 2 * C, a.qkv_ld, t0, nt, seq, hd);
            __syncthreads();
            for (int j = 0; j < nt; ++j) {
                if (km_s[t0 + j] == 0.f) continue;                                // block-uniform
                const float s = at_score(at_dot<HD>(q, &a_s[j * HD]), scale);
                const float p = at_exp(s - my_lse);                               // (a kept key exists: my_lse is finite)
                const float dp = at_dot<HD>(go, &b_s[j * HD]);
                const float ds = p * (dp - delta);
#pragma unroll
                for (int v = 0; v < HD / 4; ++v) {
                    const float4 t = *reinterpret_cast<const float4*>(&a_s[j * HD + 4 * v]);
                    dq[4 * v + 0] = fmaf(ds, t.x, dq[4 * v + 0]); dq[4 * v + 1] = fmaf(ds, t.y, dq[4 * v + 1]);
                    dq[4 * v + 2] = fmaf(ds, t.z, dq[4 * v + 2]); dq[4 * v + 3] = fmaf(ds, t.w, dq[4 * v + 3]);
                }
            }
        }
        if (live) {
#pragma unroll
            for (int v = 0; v < HD / 4; ++v)
                if (4 * v < hd)
                    nrx_stg4(gq + 4 * v, 0, make_float4(dq[4 * v] * scale, dq[4 * v + 1] * scale, dq[4 * v + 2] * scale, dq[4 * v + 3] * scale));
        }
    }

    // ---- phase B: dv_j = sum_i p_ij g_out_i,  dk_j = scale sum_i p_ij (dP_ij - delta_i) q_i   (thread j = tid; a masked key gets zeros)
    {
        float k[HD], vv[HD];
        at_load_row<HD>(k, base + C + (int64_t)i * a.qkv_ld, hd);
        at_load_row<HD>(vv, base + 2 * C + (int64_t)i * a.qkv_ld, hd);
        for (int e0 = 0; e0 < HD; e0 += EH) {
            float dk[EH], dv[EH];
#pragma unroll
            for (int e = 0; e < EH; ++e) { dk[e] = 0.f; dv[e] = 0.f; }
            for (int t0 = 0; t0 < seq; t0 += AT_TILE) {
                const int nt = min(AT_TILE, seq - t0);
                __syncthreads();          // phase A's (or the previous pass's) tile has been read; delta_s and lse_s are written
                at_stage2<HD>(a_s, base, a.qkv_ld, b_s, gbase, a.g_out_ld, t0, nt, seq, hd);
                __syncthreads();
                const bool my_keep = km_s[tid] != 0.f;
                for (int r = 0; r < nt; ++r) {
                    const float s = at_score(at_dot<HD>(k, &a_s[r * HD]), scale);
                    const float p = my_keep ? at_exp(s - lse_s[t0 + r]) : 0.f;     // (selected, not multiplied: lse is -inf when no key is kept)
                    const float dp = at_dot<HD>(vv, &b_s[r * HD]);
                    const float ds = p * (dp - delta_s[t0 + r]);
#pragma unroll
                    for (int v = 0; v < EH / 4; ++v) {
                        const float4 tq = *reinterpret_cast<const float4*>(&a_s[r * HD + e0 + 4 * v]);
                        const float4 tg = *reinterpret_cast<const float4*>(&b_s[r * HD + e0 + 4 * v]);
                        dk[4 * v + 0] = fmaf(ds, tq.x, dk[4 * v + 0]); dk[4 * v + 1] = fmaf(ds, tq.y, dk[4 * v + 1]);
                        dk[4 * v + 2] = fmaf(ds, tq.z, dk[4 * v + 2]); dk[4 * v + 3] = fmaf(ds, tq.w, dk[4 * v + 3]);
                        dv[4 * v + 0] = fmaf(p, tg.x, dv[4 * v + 0]); dv[4 * v + 1] = fmaf(p, tg.y, dv[4 * v + 1]);
                        dv[4 * v + 2] = fmaf(p, tg.z, dv[4 * v + 2]); dv[4 * v + 3] = fmaf(p, tg.w, dv[4 * v + 3]);
                    }
                }
            }
            if (live) {
#pragma unroll
                for (int v = 0; v < EH / 4; ++v)
                    if (e0 + 4 * v < hd) {
                        nrx_stg4(gq + C + e0 + 4 * v, 0, make_float4(dk[4 * v] * scale, dk[4 * v + 1] * scale, dk[4 * v + 2] * scale, dk[4 * v + 3] * scale));
                        nrx_stg4(gq + 2 * C + e0 + 4 * v, 0, make_float4(dv[4 * v], dv[4 * v + 1], dv[4 * v + 2], dv[4 * v + 3]));
                    }
            }
        }
    }
}

template <bool BWD>
void attn_launch(int hd, dim3 grid, dim3 block, hipStream_t st, const AttnArgs& a) {
#define AT_CASE(HD_)                                                                              \
    do {                                                                                          \
        if (BWD) hipLaunchKernelGGL((attn_bwd_kernel<HD_>), grid, block, 0, st, a);               \
        else hipLaunchKernelGGL((attn_fwd_kernel<HD_>), grid, block, 0, st, a);                   \
    } while (0)
    if (hd <= 4) AT_CASE(4);
    else if (hd <= 8) AT_CASE(8);
    else if (hd <= 12) AT_CASE(12);
    else if (hd <= 16) AT_CASE(16);
    else if (hd <= 32) AT_CASE(32);
    else AT_CASE(64);
#undef AT_CASE
}

bool at_f32_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the checks both entry points share; NRX_OK or the status to return
int attn_check(const char* who, int64_t qkv_ld, int64_t batch, int32_t seq, int32_t heads, int32_t head_dim, float scale, int64_t out_ld) {
    NRX_REQUIRE(batch >= 0 && seq >= 1 && heads >= 1 && head_dim >= 1, "%s: bad argument (batch %lld, seq %d, heads %d, head_dim %d)", who,
                (long long)batch, seq, heads, head_dim);
    NRX_REQUIRE(scale == scale && fabsf(scale) <= FLT_MAX, "%s: bad argument (scale must be finite)", who);
    const int64_t C = (int64_t)heads * head_dim;
    NRX_REQUIRE(qkv_ld >= 3 * C && out_ld >= C, "%s: bad argument (token stride below the row width: qkv_ld %lld < %lld or out_ld %lld < %lld)", who,
                (long long)qkv_ld, (long long)(3 * C), (long long)out_ld, (long long)C);
    NRX_REQUIRE(batch * heads < 0x7fffffffLL, "%s: bad argument (batch * heads %lld: one workgroup each, below 2^31)", who, (long long)(batch * heads));
    if (seq > AT_MAX_SEQ || (head_dim & 3) != 0 || head_dim > 64 || C > AT_MAX_C) {
        nrx_set_error("%s: supports seq 1..%d, head_dim %% 4 == 0 in 4..64 and heads * head_dim <= %d (got seq=%d, heads=%d, head_dim=%d)", who,
                      AT_MAX_SEQ, AT_MAX_C, seq, heads, head_dim);
        return NRX_ERR_UNSUPPORTED;
    }
    return NRX_OK;
}

}  // namespace

extern "C" int nrx_attn_fwd(const float* qkv, int64_t qkv_ld, int64_t batch, int32_t seq, int32_t heads, int32_t head_dim, float scale,
                            const float* key_mask, float* out, int64_t out_ld, float* row_lse, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_attn_fwd";
    if (batch > 0) {
        NRX_REQUIRE(qkv && out && row_lse, "%s: null buffer", who);
        NRX_REQUIRE(nrx_aligned16(qkv) && nrx_aligned16(out) && (qkv_ld & 3) == 0 && (out_ld & 3) == 0,
                    "%s: misaligned rows (qkv / out and their token strides must keep every row 16-byte aligned)", who);
        NRX_REQUIRE(at_f32_ok(row_lse) && at_f32_ok(key_mask), "%s: misaligned pointer", who);
    }
    const int rc = attn_check(who, qkv_ld, batch, seq, heads, head_dim, scale, out_ld);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    AttnArgs a = {};
    a.qkv = qkv; a.mask = key_mask; a.out = out; a.lse = row_lse;
    a.qkv_ld = qkv_ld; a.out_ld = out_ld;
    a.seq = seq; a.heads = heads; a.hd = head_dim; a.scale = scale;
    attn_launch<false>(head_dim, dim3((unsigned)(batch * heads)), dim3(seq <= 64 ? 64 : 128), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

extern "C" int nrx_attn_bwd(const float* qkv, int64_t qkv_ld, int64_t batch, int32_t seq, int32_t heads, int32_t head_dim, float scale,
                            const float* key_mask, const float* out, int64_t out_ld, const float* row_lse, const float* g_out,
                            int64_t g_out_ld, float* g_qkv, int64_t g_qkv_ld, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_attn_bwd";
    if (batch > 0) {
        NRX_REQUIRE(qkv && out && row_lse && g_out && g_qkv, "%s: null buffer", who);
        NRX_REQUIRE(nrx_aligned16(qkv) && nrx_aligned16(out) && nrx_aligned16(g_out) && nrx_aligned16(g_qkv) && (qkv_ld & 3) == 0 &&
                        (out_ld & 3) == 0 && (g_out_ld & 3) == 0 && (g_qkv_ld & 3) == 0,
                    "%s: misaligned rows (qkv / out / g_out / g_qkv and their token strides must keep every row 16-byte aligned)", who);
        NRX_REQUIRE(at_f32_ok(row_lse) && at_f32_ok(key_mask), "%s: misaligned pointer", who);
    }
    NRX_REQUIRE(heads < 1 || head_dim < 1 || (g_out_ld >= (int64_t)heads * head_dim && g_qkv_ld >= 3 * (int64_t)heads * head_dim),
                "%s: bad argument (token stride below the row width: g_out_ld %lld, g_qkv_ld %lld)", who, (long long)g_out_ld, (long long)g_qkv_ld);
    const int rc = attn_check(who, qkv_ld, batch, seq, heads, head_dim, scale, out_ld);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    AttnArgs a = {};
    a.qkv = qkv; a.mask = key_mask; a.out = const_cast<float*>(out); a.lse = const_cast<float*>(row_lse);
    a.g_out = g_out; a.g_qkv = g_qkv;
    a.qkv_ld = qkv_ld; a.out_ld = out_ld; a.g_out_ld = g_out_ld; a.g_qkv_ld = g_qkv_ld;
    a.seq = seq; a.heads = heads; a.hd = head_dim; a.scale = scale;
    attn_launch<true>(head_dim, dim3((unsigned)(batch * heads)), dim3(seq <= 64 ? 64 : 128), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}
