// One interacting layer of AutoInt (Song et al., CIKM 2019): multi-head self-attention over the F fields of a sample with a residual projection
// and a ReLU, forward and backward on the matrix cores with no q / k / v / r tensor and nothing of size batch * F * F in global memory.  No
// reference counterpart; DESIGN 7l.
//
// Definition (include/nrx_embed.h restates it, with every fp32 chain): x_i = x[b * ld + field_off[i] .. + din), Wq, Wk, Wv, Wres [C, din],
//   q_i = Wq x_i, k_i = Wk x_i, v_i = Wv x_i, r_i = Wres x_i;  s^h_ij = scale <q^h_i, k^h_j>;  p^h_i. = softmax_j s^h_ij;
//   out[b, i C + c] = relu(concat_h(sum_j p^h_ij v^h_j) + r_i)[c];  row_lse[b, h, i] = log sum_j exp(s^h_ij).
//
// v_mfma_f32_32x32x2_f32 is bit for bit fma(a_k1, b_k1, fma(a_k0, b_k0, c)); its A operand is lane l <- A[l & 31][l >> 5], its B operand lane
// l <- B[l >> 5][l & 31], its C layout column l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.
//
// ONE WORKGROUP OF 4 WAVES OWNS ONE SAMPLE at a time: the weights are staged in LDS once per workgroup (odd row stride), the sample's fields
// and its q, k, v, r live in LDS as [F][C | 1].  Small shapes keep several workgroups on a CU; the corner of the envelope runs one.
//   project : wave w computes matrix w of (q, k, v, r):  M^T [c][field] = W X^T in 32 x 32 tiles, K = din.  The C layout has the field on the
//             lane, so the store to [field][c] with an odd stride is conflict free.
//   attend  : an item is (head, tile of 32 rows i); items go round the waves.  S^T [j][i] = K Q^T has the row i on the lane and 16 (32) columns j
//             in registers: max, exp and the sum are register arithmetic plus one exchange between the lane halves.  O^T = V^T E uses the
//             accumulator of S^T AS its B operand (the K order is the C layout's row order, the A operand is permuted to match: no exchange).
//             O / l overwrites the q rows of the item, which nobody else reads; out = relu(o + r) leaves LDS in whole coalesced rows.
//   backward: q, k, v again from x; dO = g_out where out > 0 (also dR).  Pass 1 (row tiles): P, dP, delta_i = sum_j P dP, dS = P (dP - delta),
//             dQ^T = K^T dS^T.  Pass 2 (column tiles): the same scores with the operands exchanged (the same bits: the products commute), so
//             that j is on the lane: dK^T = Q^T dS and dV^T = dO^T P accumulate over the row tiles, and overwrite the k and v rows that the item
//             alone reads.  Then wave w adds dM_w^T X of the sample into its REGISTER accumulator of g_W_w (a workgroup owns a slice of
//             consecutive samples; partials [slice][matrix][C][din] go to the workspace, autoint_reduce_kernel adds them in slice order), and
//             g_x^T = sum_m W_m^T dM_m^T is one GEMM per 32 x 32 tile with K = 4 C, written straight to the field columns.
// The corner of the envelope does not hold the four weight matrices beside the backward's six [F][C] arrays: there (WLDS = false) the weights
// are read from global memory (L2) as MFMA operands.  Loads are never behind a branch (a dead lane reads a valid address and selects 0).
#include "nrx_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int AI_MAX = 64;                     // F, din, C
constexpr int AI_WAVES = 4;
constexpr int AI_THREADS = AI_WAVES * 64;
constexpr int AI_MAX_BLOCKS = 1024;            // the bounded grid of the backward (slices)
constexpr int AI_FWD_BLOCKS = 2048;            // ... and of the forward (samples): 256 CUs hold 6 workgroups each at F = 26, din = 16, C = 32
constexpr int AI_LDS = 160 * 1024;

struct AiArgs {
    const float* x;
    const float* W[4];       // Wq, Wk, Wv, Wres (null when nm == 3)
    float* out;              // forward: written; backward: read
    float* lse;
    const float* g_out;
    float* g_x;
    float* part;             // [slices][nm][C][din]
    int64_t ld, out_ld, go_ld, gx_ld, batch;
    float scale;
    int32_t F, din, heads, hd, C, nm, slice;
    int32_t off[AI_MAX];
};

__device__ __forceinline__ int ai_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

template <bool WLDS>
__device__ __forceinline__ float ai_ldw(const float* p) {
    if constexpr (WLDS) return *p;
    else return *(const NRX_GLOBAL float*)p;
}

// the weights to LDS as [nm][C][WS]
__device__ __forceinline__ void ai_stage_weights(const NRX_CONST AiArgs* ka, const AiArgs& a, float* wl, int WS, int tid) {
    const int n = a.C * a.din;
    for (int m = 0; m < a.nm; ++m) {
        const float* w = ka->W[m];
        for (int idx = tid; idx < n; idx += AI_THREADS) {
            const int c = idx / a.din, d = idx - c * a.din;
            wl[(m * a.C + c) * WS + d] = ((const NRX_GLOBAL float*)w)[idx];
        }
    }
}

// the sample's field rows to LDS as [F][DS], 16-byte loads
__device__ __forceinline__ void ai_stage_fields(const NRX_CONST AiArgs* ka, const AiArgs& a, float* xs, int64_t b, int DS, int tid) {
    const int qd = a.din >> 2, nq = a.F * qd;
    const float* row = a.x + b * a.ld;
    for (int q = tid; q < nq; q += AI_THREADS) {
        const int f = q / qd, c = (q - f * qd) * 4;
        const nrx_f32x4 v = *(const NRX_GLOBAL nrx_f32x4*)(row + ka->off[f] + c);
        float* e = xs + f * DS + c;
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
    }
}

// M[f][c] = chain from 0 over d ascending of fmaf(W[c][d], x_f[d], .), all tiles of one matrix by one wave
template <bool WLDS>
__device__ __forceinline__ void ai_project(const float* W, int WS, const float* xs, int DS, float* M, int CS, int F, int din, int C, int r, int kk) {
    for (int ct = 0; 32 * ct < C; ++ct)
        for (int ft = 0; 32 * ft < F; ++ft) {
            const int c = 32 * ct + r, f = 32 * ft + r;
            const bool cok = c < C, fok = f < F;
            const float* wp = W + (cok ? c : 0) * WS;
            const float* xp = xs + (fok ? f : 0) * DS;
            f32x16 acc = {};
            for (int s = 0; s < (din >> 1); ++s) {
                const int d = 2 * s + kk;
                const float av = ai_ldw<WLDS>(wp + d), bv = xp[d];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cok ? av : 0.f, fok ? bv : 0.f, acc, 0, 0, 0);
            }
            if (fok) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int cc = 32 * ct + ai_row(q, kk);
                    if (cc < C) M[f * CS + cc] = acc[q];
                }
            }
        }
}

// T[row of A][row of B] = chain from 0 over c = 0 .. hd - 1 ascending of fmaf(A[ar][c0 + c], B[br][c0 + c], .): the row of B on the lane, the 32
// rows of A of the tile in the C layout's register order
__device__ __forceinline__ f32x16 ai_dot_tile(const float* A, int ar, bool aok, const float* B, int br, bool bok, int CS, int c0, int hd, int kk) {
    const float* ap = A + (aok ? ar : 0) * CS + c0;
    const float* bp = B + (bok ? br : 0) * CS + c0;
    f32x16 acc = {};
    for (int s = 0; s < (hd >> 1); ++s) {
        const int c = 2 * s + kk;
        const float av = ap[c], bv = bp[c];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aok ? av : 0.f, bok ? bv : 0.f, acc, 0, 0, 0);
    }
    return acc;
}

__global__ __launch_bounds__(AI_THREADS) void autoint_fwd_kernel(const AiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ai_smem[];
    const NRX_CONST AiArgs* ka = nrx_kernarg<AiArgs>();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
    const int F = a.F, din = a.din, C = a.C, hd = a.hd, nm = a.nm, DS = din | 1, WS = din | 1, CS = C | 1;
    const int FTn = F > 32 ? 2 : 1;
    float* wl = ai_smem;                                       // [nm][C][WS]
    float* xs = wl + nm * C * WS;                              // [F][DS]
    float* Q = xs + F * DS;                                    // [F][CS] each: q (then the attention output), k, v, r
    float* K = Q + F * CS;
    float* V = K + F * CS;
    float* R = V + F * CS;                                     // (not there when nm == 3)
    ai_stage_weights(ka, a, wl, WS, tid);
    for (int64_t b = blockIdx.x; b < a.batch; b += gridDim.x) {
        ai_stage_fields(ka, a, xs, b, DS, tid);
        __syncthreads();                                       // the fields (and the weights) are staged; the sample before this one is written
        if (wave < nm) ai_project<true>(wl + wave * C * WS, WS, xs, DS, Q + wave * F * CS, CS, F, din, C, r, kk);
        __syncthreads();
        for (int idx = wave; idx < a.heads * FTn; idx += AI_WAVES) {
            const int h = idx / FTn, it = idx - h * FTn, c0 = h * hd, i = 32 * it + r;
            const bool iok = i < F;
            f32x16 s[2];
            float m = -INFINITY;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
                if (jt < FTn) {
                    const int j = 32 * jt + r;
                    s[jt] = ai_dot_tile(K, j, j < F, Q, i, iok, CS, c0, hd, kk);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const float v = 32 * jt + ai_row(q, kk) < F ? a.scale * s[jt][q] : -INFINITY;
                        s[jt][q] = v;
                        m = fmaxf(m, v);
                    }
                }
            m = fmaxf(m, __shfl_xor(m, 32));
            float l = 0.f;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
                if (jt < FTn) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const float e = expf(s[jt][q] - m);
                        s[jt][q] = e;
                        l = l + e;
                    }
                }
            l = l + __shfl_xor(l, 32);
            for (int ct = 0; 32 * ct < hd; ++ct) {
                const int cc = 32 * ct + r;
                const bool cok = cc < hd;
                f32x16 acc = {};
#pragma unroll
                for (int jt = 0; jt < 2; ++jt)
                    if (jt < FTn) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int jr = 32 * jt + ai_row(q, kk);
                            const bool ok = cok && jr < F;
                            const float av = V[(ok ? jr : 0) * CS + c0 + (cok ? cc : 0)];
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? av : 0.f, s[jt][q], acc, 0, 0, 0);
                        }
                    }
                if (iok) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int c2 = 32 * ct + ai_row(q, kk);
                        if (c2 < hd) Q[i * CS + c0 + c2] = acc[q] / l;
                    }
                }
            }
            if (kk == 0 && iok) ((NRX_GLOBAL float*)a.lse)[(b * a.heads + h) * F + i] = m + logf(l);
        }
        __syncthreads();
        float* orow = a.out + b * a.out_ld;
        for (int idx = tid; idx < F * C; idx += AI_THREADS) {
            const int i = idx / C, c = idx - i * C;
            float v = Q[i * CS + c];
            if (nm == 4) v = v + R[i * CS + c];
            ((NRX_GLOBAL float*)orow)[idx] = v > 0.f ? v : 0.f;
        }
    }
}

// NT = 2: two 32-row tiles of C or two 32-column tiles of din (else one of each): the size of the weight gradient's register accumulator;
// FT: the 32-row tiles of F
template <int NT, int FT, bool WLDS>
__global__ __launch_bounds__(AI_THREADS) void autoint_bwd_kernel(const AiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ai_smem[];
    const NRX_CONST AiArgs* ka = nrx_kernarg<AiArgs>();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
    const int F = a.F, din = a.din, C = a.C, hd = a.hd, nm = a.nm, heads = a.heads, DS = din | 1, CS = C | 1;
    const int WS = WLDS ? (din | 1) : din;
    constexpr int FTn = FT;
    const int DTn = din > 32 ? 2 : 1;
    float* wl = ai_smem;                                       // [nm][C][WS] (WLDS)
    float* xs = wl + (WLDS ? nm * C * WS : 0);                 // [F][DS]
    float* Q = xs + F * DS;                                    // [F][CS] each
    float* K = Q + F * CS;                                     // k, then dK
    float* V = K + F * CS;                                     // v, then dV
    float* dO = V + F * CS;                                    // g_out where out > 0: dO and dR
    float* dQ = dO + F * CS;
    float* ls = dQ + F * CS;                                   // [heads][F] row_lse
    float* dl = ls + heads * F;                                // [heads][F] delta
    if constexpr (WLDS) ai_stage_weights(ka, a, wl, WS, tid);
    const float* wsrc = WLDS ? wl + wave * C * WS : ka->W[wave < nm ? wave : 0];
    const float* dM = wave == 0 ? dQ : wave == 1 ? K : wave == 2 ? V : dO;
    const int64_t slices = (a.batch + a.slice - 1) / a.slice;
    for (int64_t sl = blockIdx.x; sl < slices; sl += gridDim.x) {
        f32x16 accw[NT][NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int dt = 0; dt < NT; ++dt) accw[ct][dt] = f32x16{};
        const int64_t b0 = sl * a.slice, b1 = b0 + a.slice < a.batch ? b0 + a.slice : a.batch;
        for (int64_t b = b0; b < b1; ++b) {
            __syncthreads();                                   // the sample before this one is read
            ai_stage_fields(ka, a, xs, b, DS, tid);
            for (int idx = tid; idx < F * C; idx += AI_THREADS) {
                const int i = idx / C, c = idx - i * C;
                const float ov = ((const NRX_GLOBAL float*)a.out)[b * a.out_ld + idx], gv = ((const NRX_GLOBAL float*)a.g_out)[b * a.go_ld + idx];
                dO[i * CS + c] = ov > 0.f ? gv : 0.f;
            }
            for (int idx = tid; idx < heads * F; idx += AI_THREADS) ls[idx] = ((const NRX_GLOBAL float*)a.lse)[b * heads * F + idx];
            __syncthreads();
            if (wave < 3) ai_project<WLDS>(wsrc, WS, xs, DS, Q + wave * F * CS, CS, F, din, C, r, kk);
            __syncthreads();
            // pass 1: row tiles.  delta and dQ
            for (int idx = wave; idx < heads * FTn; idx += AI_WAVES) {
                const int h = idx / FTn, it = idx - h * FTn, c0 = h * hd, i = 32 * it + r;
                const bool iok = i < F;
                const float lsev = ls[h * F + (iok ? i : 0)];
                f32x16 p[FT], dp[FT];
                float de = 0.f;
#pragma unroll
                for (int jt = 0; jt < FT; ++jt) {
                    const int j = 32 * jt + r;
                    p[jt] = ai_dot_tile(K, j, j < F, Q, i, iok, CS, c0, hd, kk);
                    dp[jt] = ai_dot_tile(V, j, j < F, dO, i, iok, CS, c0, hd, kk);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const bool ok = iok && 32 * jt + ai_row(q, kk) < F;
                        const float pv = expf(a.scale * p[jt][q] - lsev);
                        p[jt][q] = ok ? pv : 0.f;
                        de = fmaf(p[jt][q], dp[jt][q], de);
                    }
                }
                de = de + __shfl_xor(de, 32);
                if (kk == 0 && iok) dl[h * F + i] = de;
#pragma unroll
                for (int jt = 0; jt < FT; ++jt) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) p[jt][q] = p[jt][q] * (dp[jt][q] - de);
                }
                for (int ct = 0; 32 * ct < hd; ++ct) {
                    const int cc = 32 * ct + r;
                    const bool cok = cc < hd;
                    f32x16 acc = {};
#pragma unroll
                    for (int jt = 0; jt < FT; ++jt) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int jr = 32 * jt + ai_row(q, kk);
                            const bool ok = cok && jr < F;
                            const float av = K[(ok ? jr : 0) * CS + c0 + (cok ? cc : 0)];
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? av : 0.f, p[jt][q], acc, 0, 0, 0);
                        }
                    }
                    if (iok) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int c2 = 32 * ct + ai_row(q, kk);
                            if (c2 < hd) dQ[i * CS + c0 + c2] = a.scale * acc[q];
                        }
                    }
                }
            }
            __syncthreads();
            // pass 2: column tiles.  dK and dV over the k and v rows the item alone reads
            for (int idx = wave; idx < heads * FTn; idx += AI_WAVES) {
                const int h = idx / FTn, jt = idx - h * FTn, c0 = h * hd, j = 32 * jt + r;
                const bool jok = j < F;
                f32x16 gk[NT], gv[NT];                          // (NT == 1: C <= 32, so the head fits one tile of 32 columns)
#pragma unroll
                for (int ct = 0; ct < NT; ++ct) gk[ct] = gv[ct] = f32x16{};
                for (int it = 0; it < FTn; ++it) {
                    const int i = 32 * it + r;
                    f32x16 p = ai_dot_tile(Q, i, i < F, K, j, jok, CS, c0, hd, kk);
                    f32x16 ds = ai_dot_tile(dO, i, i < F, V, j, jok, CS, c0, hd, kk);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int ir = 32 * it + ai_row(q, kk);
                        const bool ok = jok && ir < F;
                        const float lv = ls[h * F + (ir < F ? ir : 0)], dv = dl[h * F + (ir < F ? ir : 0)];
                        const float pv = expf(a.scale * p[q] - lv);
                        p[q] = ok ? pv : 0.f;
                        ds[q] = ok ? p[q] * (ds[q] - dv) : 0.f;
                    }
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        if (32 * ct < hd) {
                            const int cc = 32 * ct + r;
                            const bool cok = cc < hd;
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const int ir = 32 * it + ai_row(q, kk);
                                const bool ok = cok && ir < F;
                                const int at = (ok ? ir : 0) * CS + c0 + (cok ? cc : 0);
                                const float aq = Q[at], ao = dO[at];
                                gk[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? aq : 0.f, ds[q], gk[ct], 0, 0, 0);
                                gv[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? ao : 0.f, p[q], gv[ct], 0, 0, 0);
                            }
                        }
                }
                if (jok) {
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        if (32 * ct < hd) {
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const int c2 = 32 * ct + ai_row(q, kk);
                                if (c2 < hd) {
                                    K[j * CS + c0 + c2] = a.scale * gk[ct][q];
                                    V[j * CS + c0 + c2] = gv[ct][q];
                                }
                            }
                        }
                }
            }
            __syncthreads();
            // the weight gradient: wave w adds dM_w^T X of this sample to its accumulator
            if (wave < nm) {
                for (int s = 0; s < ((F + 1) >> 1); ++s) {
                    const int f = 2 * s + kk;
                    const bool fok = f < F;
                    float av[NT], bv[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int c = 32 * t + r, d = 32 * t + r;
                        const float x0 = dM[(fok ? f : 0) * CS + (c < C ? c : 0)], x1 = xs[(fok ? f : 0) * DS + (d < din ? d : 0)];
                        av[t] = fok && c < C ? x0 : 0.f;
                        bv[t] = fok && d < din ? x1 : 0.f;
                    }
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                        for (int dt = 0; dt < NT; ++dt)
                            if (32 * ct < C && 32 * dt < din) accw[ct][dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ct], bv[dt], accw[ct][dt], 0, 0, 0);
                }
            }
            // g_x: one tile (32 columns of din x 32 fields) per wave, K = nm C; the tiles go round the waves with the sample
            {
                const int t = (wave + (int)(b & 3)) & 3;
                if (t < DTn * FTn) {
                    const int dt = t / FTn, ft = t - dt * FTn, d = 32 * dt + r, f = 32 * ft + r;
                    const bool dok = d < din, fok = f < F;
                    f32x16 acc = {};
                    for (int m = 0; m < nm; ++m) {
                        const float* wm = WLDS ? wl + m * C * WS : ka->W[m];
                        const float* gm = m == 0 ? dQ : m == 1 ? K : m == 2 ? V : dO;
                        const float* wp = wm + (dok ? d : 0);
                        const float* gp = gm + (fok ? f : 0) * CS;
                        for (int s = 0; s < (C >> 1); ++s) {
                            const int c = 2 * s + kk;
                            const float aw = ai_ldw<WLDS>(wp + c * WS), bg = gp[c];
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dok ? aw : 0.f, fok ? bg : 0.f, acc, 0, 0, 0);
                        }
                    }
                    if (fok) {
                        float* grow = a.g_x + b * a.gx_ld + ka->off[f];
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int d2 = 32 * dt + ai_row(q, kk);
                            if (d2 < din) ((NRX_GLOBAL float*)grow)[d2] = acc[q];
                        }
                    }
                }
            }
        }
        if (wave < nm) {
            float* part = a.part + (sl * nm + wave) * (int64_t)(C * din);
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                for (int dt = 0; dt < NT; ++dt)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int c = 32 * ct + ai_row(q, kk), d = 32 * dt + r;
                        if (c < C && d < din) ((NRX_GLOBAL float*)part)[c * din + d] = accw[ct][dt][q];
                    }
        }
    }
}

// the partials added in slice order; element e of a partial: matrix e / (C din), then [C][din]
__global__ __launch_bounds__(256) void autoint_reduce_kernel(const float* part, float* g0, float* g1, float* g2, float* g3, int nw, int nm, int64_t slices) {
    const int n = nw * nm;
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float s = ((const NRX_GLOBAL float*)part)[e];
    int64_t t = 1;
    for (; t + 16 <= slices; t += 16) {                        // (16 loads in flight; added in slice order)
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = ((const NRX_GLOBAL float*)part)[(t + j) * n + e];
#pragma unroll
        for (int j = 0; j < 16; ++j) s += v[j];
    }
    for (; t < slices; ++t) s += ((const NRX_GLOBAL float*)part)[t * n + e];
    const int m = e / nw;
    float* g = m == 0 ? g0 : m == 1 ? g1 : m == 2 ? g2 : g3;
    ((NRX_GLOBAL float*)g)[e - m * nw] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------- host side
bool ai_shape_ok(int32_t F, int32_t din, int32_t heads, int32_t hd) {
    if (F < 2 || F > AI_MAX || din < 4 || din > AI_MAX || (din & 3) || heads < 1 || hd < 4 || (hd & 3) || heads > AI_MAX || hd > AI_MAX) return false;
    return heads * hd <= AI_MAX;
}

int ai_slice(int32_t din, int32_t C) { return C * din > 1024 ? 16 : 64; }

bool ai_f32_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

struct AiCall {
    const float* x; int64_t ld; const int32_t* off; int32_t F, din; const float* Wq; const float* Wk; const float* Wv; const float* Wres;
    int32_t heads, hd; float scale; int64_t batch; const float* out; int64_t out_ld; const float* lse;
};

int ai_unsupported(const char* who, const AiCall& c) {
    if (ai_shape_ok(c.F, c.din, c.heads, c.hd)) return NRX_OK;
    nrx_set_error("%s: supports n_fields 2..%d, din %% 4 == 0 in 4..%d, head_dim %% 4 == 0, heads * head_dim in 4..%d (got n_fields=%d, din=%d, heads=%d, "
                  "head_dim=%d)", who, AI_MAX, AI_MAX, AI_MAX, c.F, c.din, c.heads, c.hd);
    return NRX_ERR_UNSUPPORTED;
}

// the argument checks both entry points share (NRX_OK or NRX_ERR_BAD_ARG)
int ai_check(const char* who, const AiCall& c) {
    NRX_REQUIRE(c.F >= 1 && c.din >= 1 && c.heads >= 1 && c.hd >= 1 && c.batch >= 0, "%s: bad argument (n_fields %d, din %d, heads %d, head_dim %d, batch %lld)",
                who, c.F, c.din, c.heads, c.hd, (long long)c.batch);
    NRX_REQUIRE(c.scale == c.scale && c.scale - c.scale == 0.f, "%s: bad argument (scale is not finite)", who);
    NRX_REQUIRE(c.off != nullptr, "%s: null field_off", who);
    if (c.F > AI_MAX) return ai_unsupported(who, c);           // before field_off[0 .. F) is read: the caller's array may be sized for a supported F
    NRX_REQUIRE(c.ld >= c.din && (c.ld & 3) == 0, "%s: bad argument (ld %lld: the row stride must hold a field of din %d and be a multiple of 4)", who,
                (long long)c.ld, c.din);
    const int64_t row = (int64_t)c.F * c.heads * c.hd;
    NRX_REQUIRE(c.out_ld >= row, "%s: bad argument (out_ld %lld below n_fields * heads * head_dim = %lld)", who, (long long)c.out_ld, (long long)row);
    for (int32_t i = 0; i < c.F; ++i) {
        const int64_t o = c.off[i];
        NRX_REQUIRE(o >= 0 && o + c.din <= c.ld, "%s: bad argument (field_off[%d] = %lld: the field leaves the row of ld %lld)", who, i, (long long)o,
                    (long long)c.ld);
        NRX_REQUIRE((o & 3) == 0, "%s: misaligned field (field_off[%d] = %lld must be a multiple of 4)", who, i, (long long)o);
    }
    for (int32_t i = 1; i < c.F; ++i)
        for (int32_t k = 0; k < i; ++k) {
            const int64_t d = (int64_t)c.off[i] - c.off[k];
            NRX_REQUIRE(d >= c.din || -d >= c.din, "%s: bad argument (field_off[%d] = %d and field_off[%d] = %d overlap at din %d)", who, k, c.off[k], i,
                        c.off[i], c.din);
        }
    if (c.batch > 0) {
        NRX_REQUIRE(c.x != nullptr, "%s: null buffer (x)", who);
        NRX_REQUIRE(c.Wq != nullptr, "%s: null buffer (Wq)", who);
        NRX_REQUIRE(c.Wk != nullptr, "%s: null buffer (Wk)", who);
        NRX_REQUIRE(c.Wv != nullptr, "%s: null buffer (Wv)", who);
        NRX_REQUIRE(c.out != nullptr, "%s: null buffer (out)", who);
        NRX_REQUIRE(c.lse != nullptr, "%s: null buffer (row_lse)", who);
        NRX_REQUIRE(nrx_aligned16(c.x), "%s: misaligned x (every field row must be 16-byte aligned)", who);
        NRX_REQUIRE(ai_f32_ok(c.Wq), "%s: misaligned Wq", who);
        NRX_REQUIRE(ai_f32_ok(c.Wk), "%s: misaligned Wk", who);
        NRX_REQUIRE(ai_f32_ok(c.Wv), "%s: misaligned Wv", who);
        NRX_REQUIRE(ai_f32_ok(c.Wres), "%s: misaligned Wres", who);
        NRX_REQUIRE(ai_f32_ok(c.out), "%s: misaligned out", who);
        NRX_REQUIRE(ai_f32_ok(c.lse), "%s: misaligned row_lse", who);
    }
    return NRX_OK;
}

AiArgs ai_args(const AiCall& c) {
    AiArgs a = {};
    a.x = c.x; a.W[0] = c.Wq; a.W[1] = c.Wk; a.W[2] = c.Wv; a.W[3] = c.Wres; a.out = const_cast<float*>(c.out); a.lse = const_cast<float*>(c.lse);
    a.ld = c.ld; a.out_ld = c.out_ld; a.batch = c.batch; a.scale = c.scale; a.F = c.F; a.din = c.din; a.heads = c.heads; a.hd = c.hd;
    a.C = c.heads * c.hd; a.nm = c.Wres ? 4 : 3; a.slice = ai_slice(c.din, a.C);
    for (int i = 0; i < c.F; ++i) a.off[i] = c.off[i];
    return a;
}

size_t ai_fwd_lds(const AiArgs& a) { return (size_t)(a.nm * a.C * (a.din | 1) + a.F * (a.din | 1) + a.nm * a.F * (a.C | 1)) * 4; }
size_t ai_bwd_lds(const AiArgs& a, bool wlds) {
    return (size_t)((wlds ? a.nm * a.C * (a.din | 1) : 0) + a.F * (a.din | 1) + 5 * a.F * (a.C | 1) + 2 * a.heads * a.F) * 4;
}

bool ai_lds_ready() {
    static const bool ok = [] {
        // (the weights leave LDS only where C, din > 32 and F > 32: the other three WLDS = false instantiations cannot be reached)
        const void* ks[] = {reinterpret_cast<const void*>(&autoint_fwd_kernel),
                            reinterpret_cast<const void*>(&autoint_bwd_kernel<1, 1, true>), reinterpret_cast<const void*>(&autoint_bwd_kernel<1, 2, true>),
                            reinterpret_cast<const void*>(&autoint_bwd_kernel<2, 1, true>), reinterpret_cast<const void*>(&autoint_bwd_kernel<2, 2, true>),
                            reinterpret_cast<const void*>(&autoint_bwd_kernel<2, 2, false>)};
        for (const void* k : ks)
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, AI_LDS) != hipSuccess) return false;
        return true;
    }();
    return ok;
}

int64_t ai_slices(int64_t batch, int sl) { return batch > 0 ? (batch + sl - 1) / sl : 1; }

}  // namespace

extern "C" int nrx_autoint_supported(int32_t n_fields, int32_t din, int32_t heads, int32_t head_dim) {
    return ai_shape_ok(n_fields, din, heads, head_dim) ? 1 : 0;
}

extern "C" int64_t nrx_autoint_wgrad_slice(int32_t n_fields, int32_t din, int32_t heads, int32_t head_dim) {
    if (n_fields < 1 || din < 1 || heads < 1 || head_dim < 1) return 0;
    return (int64_t)heads * head_dim * din > 1024 ? 16 : 64;
}

extern "C" int64_t nrx_autoint_bwd_workspace(int64_t batch, int32_t n_fields, int32_t din, int32_t heads, int32_t head_dim) {
    if (batch < 0 || n_fields < 1 || din < 1 || heads < 1 || head_dim < 1) return 0;
    const int64_t C = (int64_t)heads * head_dim;
    return ai_slices(batch, (int)nrx_autoint_wgrad_slice(n_fields, din, heads, head_dim)) * 4 * C * din * 4;
}

extern "C" int nrx_autoint_layer_fwd(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t din, const float* Wq, const float* Wk,
                                     const float* Wv, const float* Wres, int32_t heads, int32_t head_dim, float scale, int64_t batch, float* out,
                                     int64_t out_ld, float* row_lse, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_autoint_layer_fwd";
    const AiCall c = {x, ld, field_off, n_fields, din, Wq, Wk, Wv, Wres, heads, head_dim, scale, batch, out, out_ld, row_lse};
    int rc = ai_check(who, c);
    if (rc == NRX_OK) rc = ai_unsupported(who, c);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    if (!ai_lds_ready()) {
        nrx_set_error("%s: the kernels' LDS size could not be set", who);
        return NRX_ERR_LAUNCH;
    }
    const AiArgs a = ai_args(c);
    const dim3 grid((unsigned)(batch < AI_FWD_BLOCKS ? batch : AI_FWD_BLOCKS)), block(AI_THREADS);
    hipLaunchKernelGGL(autoint_fwd_kernel, grid, block, ai_fwd_lds(a), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

extern "C" int nrx_autoint_layer_bwd(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t din, const float* Wq, const float* Wk,
                                     const float* Wv, const float* Wres, int32_t heads, int32_t head_dim, float scale, int64_t batch, const float* out,
                                     int64_t out_ld, const float* row_lse, const float* g_out, int64_t g_out_ld, float* g_x, int64_t gx_ld, float* g_Wq,
                                     float* g_Wk, float* g_Wv, float* g_Wres, void* workspace, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_autoint_layer_bwd";
    const AiCall c = {x, ld, field_off, n_fields, din, Wq, Wk, Wv, Wres, heads, head_dim, scale, batch, out, out_ld, row_lse};
    int rc = ai_check(who, c);
    if (rc != NRX_OK) return rc;
    NRX_REQUIRE(g_out_ld >= (int64_t)n_fields * heads * head_dim, "%s: bad argument (g_out_ld %lld below n_fields * heads * head_dim = %lld)", who,
                (long long)g_out_ld, (long long)n_fields * heads * head_dim);
    for (int32_t i = 0; i < n_fields; ++i)
        NRX_REQUIRE(field_off[i] + (int64_t)din <= gx_ld, "%s: bad argument (gx_ld %lld does not hold field %d: field_off %d + din %d)", who,
                    (long long)gx_ld, i, field_off[i], din);
    NRX_REQUIRE((Wres == nullptr) == (g_Wres == nullptr), "%s: bad argument (g_Wres must be null exactly when Wres is)", who);
    if (batch > 0) {
        NRX_REQUIRE(g_out != nullptr, "%s: null buffer (g_out)", who);
        NRX_REQUIRE(g_x != nullptr, "%s: null buffer (g_x)", who);
        NRX_REQUIRE(g_Wq != nullptr, "%s: null buffer (g_Wq)", who);
        NRX_REQUIRE(g_Wk != nullptr, "%s: null buffer (g_Wk)", who);
        NRX_REQUIRE(g_Wv != nullptr, "%s: null buffer (g_Wv)", who);
        NRX_REQUIRE(workspace != nullptr, "%s: null buffer (workspace)", who);
        NRX_REQUIRE(ai_f32_ok(g_out), "%s: misaligned g_out", who);
        NRX_REQUIRE(ai_f32_ok(g_x), "%s: misaligned g_x", who);
        NRX_REQUIRE(ai_f32_ok(g_Wq), "%s: misaligned g_Wq", who);
        NRX_REQUIRE(ai_f32_ok(g_Wk), "%s: misaligned g_Wk", who);
        NRX_REQUIRE(ai_f32_ok(g_Wv), "%s: misaligned g_Wv", who);
        NRX_REQUIRE(ai_f32_ok(g_Wres), "%s: misaligned g_Wres", who);
        NRX_REQUIRE(ai_f32_ok(workspace), "%s: misaligned workspace", who);
    }
    rc = ai_unsupported(who, c);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    if (!ai_lds_ready()) {
        nrx_set_error("%s: the kernels' LDS size could not be set", who);
        return NRX_ERR_LAUNCH;
    }
    AiArgs a = ai_args(c);
    a.g_out = g_out; a.go_ld = g_out_ld; a.g_x = g_x; a.gx_ld = gx_ld; a.part = reinterpret_cast<float*>(workspace);
    const int64_t slices = ai_slices(batch, a.slice);
    const dim3 grid((unsigned)(slices < AI_MAX_BLOCKS ? slices : AI_MAX_BLOCKS)), block(AI_THREADS);
    const bool wlds = ai_bwd_lds(a, true) <= (size_t)AI_LDS, two = a.C > 32 || din > 32;
    const size_t lds = ai_bwd_lds(a, wlds);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool f2 = n_fields > 32;
#define AI_BWD(NT, FT, WL) hipLaunchKernelGGL((autoint_bwd_kernel<NT, FT, WL>), grid, block, lds, st, a)
    if (!wlds && !(two && f2)) {
        nrx_set_error("%s: the weights do not fit in LDS at a shape that should hold them", who);
        return NRX_ERR_LAUNCH;
    }
    if (!wlds) AI_BWD(2, 2, false);
    else if (two && f2) AI_BWD(2, 2, true);
    else if (two) AI_BWD(2, 1, true);
    else if (f2) AI_BWD(1, 2, true);
    else AI_BWD(1, 1, true);
#undef AI_BWD
    NRX_LAUNCH_CHECK(who);
    const int nw = a.C * din;
    hipLaunchKernelGGL(autoint_reduce_kernel, dim3((unsigned)((nw * a.nm + 255) / 256)), dim3(256), 0, st, a.part, g_Wq, g_Wk, g_Wv, g_Wres, nw, a.nm, slices);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}
