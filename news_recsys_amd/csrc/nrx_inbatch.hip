// In-batch softmax loss of the two-tower recall model (DSSM `negatives: in_batch`), forward and backward, without the [B, B] matrix.
// No reference counterpart: the reference contrasts a user with 1-4 sampled items (src/model/recall/DSSM/model.py:65-99).
//
// Definition (include/nrx_embed.h restates it): s_ij = dot(U_i, V_j) * inv_t; column j is excluded for row i when ids are given, j != i and
// ids[j] == ids[i]; lse_i = log sum_kept exp(s_ij); l_i = lse_i - s_ii; p_ij = exp(s_ij - lse_i) (0 when excluded);
// dU_i = g_i inv_t sum_j (p_ij - [i==j]) V_j,  dV_j = inv_t sum_i g_i (p_ij - [i==j]) U_i.
//
// One kernel template, three modes.  A wavefront OWNS 32 rows of one side (users: forward and dU; items: dV) as the B operand of
// v_mfma_f32_32x32x2_f32, kept in registers, and the block's four waves STREAM 32-row tiles of the other side, staged once per block in LDS
// (double-buffered, one barrier per tile), as the A operand -- the layout of topk_mfma_kernel: lane (l31, hi) ends up with the 16 scores of ITS
// own row against the streamed rows  y(r) = t0 + 4 hi + (r & 3) + 8 (r >> 2),  r = 0..15.
//   forward : each lane keeps (max, sum) online over its 16 scores per tile; the two lanes of a row are combined at the end; the pairs of
//             the column splits (blockIdx.y) and the diagonal score go to the workspace and a finishing launch merges them in split order.
//   backward: the coefficient c(r) = g_i inv_t (exp(s - lse_i) - [i==j]) is formed in place, and the C fragment IS the B operand of the second
//             product: step r of  out[e][own] += sum_k Y[y_k][e] c[k][own]  has k = hi, so lane (own, hi) supplies c(r) as it stands and lane
//             (e, hi) reads Y[y(r)][e] from the LDS tile -- the K index runs over the tile's rows in the order the C layout hands them out; no
//             cross-lane move.  The result's C layout puts 4 consecutive e of one own row in 4 registers: float4 stores.
//             dU: own = users (lse_i, g_i in the lane).  dV: own = items; lse_i and g_i inv_t belong to the streamed side and are staged with the tile.
// The score is the fp32 fma chain of the MFMA over the element order (j, H + j) (H = half of dim padded to 8, 16, 32 or 64), THEN times inv_t:
// products commute, so forward, dU and dV see the same bits for s_ij whichever side is A -- a row whose only kept column is its diagonal has
// lse_i == s_ii, loss 0.0 and p_ii == 1.0 exactly.  (Folding inv_t log2(e) into the owned operand would save one VALU multiply per score and
// lose that identity between the two gradient roles.  The product is ib_score(): never contracted into the subtraction that follows it.)
// Summation order: a lane adds its 16 terms r = 0..15 per tile, tiles ascending, lanes hi = 0 then 1, splits ascending -- a function of
// (B, dim, splits) only.  No atomics.  Buffers: the inputs, the outputs and a workspace of B * splits * max(3, dim) floats.
//
// Candidate softmax (nrx_cand_softmax_*, DESIGN 7e: mixed negative sampling and the logQ correction): the same template over a rectangle.
// U [B, d], V [N, d] with N >= B: column i < B is row i's positive, columns B..N-1 are extra negatives; ids [N] and bias [N] belong to the
// candidates.  z_ij = s_ij + bias_j replaces s_ij everywhere above (ib_logit(): the product and the sum each rounded on their own, so the three
// roles still hold ONE value for z_ij and the exact-zero identity survives any finite bias); dV_j is formed for every j < N.
// The launches have two row counts: forward and dU own B users and stream N candidates, dV owns N candidates and streams B users.  The tail
// mask follows the streamed count; the diagonal test t0 == own0 holds as it is (positives sit at column i, both sides are cut at multiples
// of 32); an owned candidate x >= B meets no diagonal (dbit is cleared with the tail).  The bias is staged beside the ids (forward, dU) or
// kept in the lane like my_id (dV); BIAS is a template parameter, so the in-batch entry points (N == B, no bias) run the instruction stream
// they ran before.  Summation order: a function of (B, N, dim, splits) only.  Workspace: B (2 splits + 1) floats forward, splits * owned * dim
// per split backward role.  No instantiation uses scratch (-Rpass-analysis=kernel-resource-usage: 71..134 VGPRs).
#include "nrx_common.h"
#include <float.h>
#include <math.h>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int WAVES = NRX_BLOCK / 64;
constexpr int IB_MAX_SPLITS = 64;
enum { IB_FWD = 0, IB_DU = 1, IB_DV = 2 };

// B users, N >= B candidates (N == B: the in-batch form).  Forward and dU own the users and stream the candidates; dV owns the candidates and
// streams the users.  ids and bias are indexed by the candidate (row i's own id is ids[i]); lse and g by the user.
struct InbatchArgs {
    const float* own;        // [n_own, own_ld] the side whose rows the waves keep
    const float* str;        // [n_str, str_ld] the streamed side
    const void* ids;         // [N] or null
    const float* bias;       // [N] column bias (BIAS instantiations only)
    const float* lse;        // backward: row_lse [B] (of the USER index)
    const float* g;          // backward: g_row [B]
    float* out;              // backward: [splits][n_own, out_ld]
    float* pm;               // forward: [B, splits] partial max
    float* ps;               // forward: [B, splits] partial sum
    float* diag;             // forward: [B] z_ii
    int64_t own_ld, str_ld, out_ld, out_split_stride;
    int32_t n_own, n_str, dim, per_split, idx64;
    float inv_t;
};

// s_ij = chain * inv_t, rounded on its own: contracted into the subtraction that follows it (hipcc's default fuses a * b - c), the backward's
// s_ij would not be the value the forward took lse_i from.  (__fmul_rn is a plain product to the compiler and fuses all the same.)
__device__ __forceinline__ float ib_score(float chain, float inv_t) {
#pragma clang fp contract(off)
    return chain * inv_t;
}
// z_ij = s_ij + bias_j: the product and the sum each rounded on their own (no fma), so that the three roles hold one value for z_ij as they do for s_ij
__device__ __forceinline__ float ib_logit(float chain, float inv_t, float bias) {
#pragma clang fp contract(off)
    const float s = chain * inv_t;
    return s + bias;
}
__device__ __forceinline__ float ib_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// H4 = float4 loads per lane of an owned row (padded dim / 8)
template <int MODE, int H4, bool BIAS>
__global__ __launch_bounds__(NRX_BLOCK) void inbatch_kernel(const InbatchArgs a) {
    constexpr int H = 4 * H4, P = 8 * H4;
    constexpr int NB = (MODE != IB_FWD && P > 32) ? 2 : 1;         // 32-element blocks of the second product's output
    constexpr int LD = (MODE == IB_FWD ? P : 32 * NB) + 8;         // LDS row stride (floats): rows y and y + 4 land 32 banks apart
    constexpr int CH = 2 * H4;                                     // float4 chunks of a staged row
    constexpr int TOTAL = 32 * CH;
    constexpr int NL = (TOTAL + NRX_BLOCK - 1) / NRX_BLOCK;
    __shared__ __attribute__((aligned(16))) float t_s[2][32 * LD];
    __shared__ int64_t id_s[2][32];
    __shared__ float lse_s[2][32];
    __shared__ float gi_s[2][32];
    __shared__ float bias_s[2][32];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int NO = a.n_own, NS = a.n_str, dim = a.dim;
    const float inv_t = a.inv_t;
    const bool has_ids = a.ids != nullptr;
    const int own0 = (int)(((int64_t)blockIdx.x * WAVES + wid) * 32);      // (host: B + 32 * WAVES < 2^31)
    const int x = own0 + l31;
    const bool live = x < NO;
    const int xc = live ? x : NO - 1;
    const int e_base = hi * H;

    float qf[H];
#pragma unroll
    for (int v = 0; v < H4; ++v) {
        const bool ok = e_base + 4 * v < dim;
        const float4 t = nrx_ldg4(a.own + (int64_t)xc * a.own_ld + (ok ? e_base + 4 * v : 0), 0);
        qf[4 * v + 0] = ok ? t.x : 0.f; qf[4 * v + 1] = ok ? t.y : 0.f;
        qf[4 * v + 2] = ok ? t.z : 0.f; qf[4 * v + 3] = ok ? t.w : 0.f;
    }
    const int64_t my_id = has_ids ? nrx_load_id(a.ids, xc, a.idx64 != 0) : 0;
    float my_lse = 0.f, my_gi = 0.f;
    if (MODE == IB_DU) { my_lse = a.lse[xc]; my_gi = a.g[xc] * inv_t; }
    float my_bias = 0.f;                                                    // dV: the bias belongs to the owned side, like my_id
    if (BIAS && MODE == IB_DV) my_bias = a.bias[xc];

    // block-cooperative staging of a streamed tile: global -> registers (in flight during the previous tile's MFMAs) -> LDS
    float4 pre[NL];
    int64_t pre_id = 0;
    float pre_lse = 0.f, pre_gi = 0.f, pre_bias = 0.f;
    auto gload = [&](int t0) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int c = tid + n * NRX_BLOCK;
            if (c < TOTAL) {
                const int row = c / CH, ch = c % CH;
                const int y = min(t0 + row, NS - 1);                  // rows past the end: the last row's (finite) values, masked where used
                const bool ok = 4 * ch < dim;
                const float4 t = nrx_ldg4(a.str + (int64_t)y * a.str_ld + (ok ? 4 * ch : 0), 0);
                pre[n] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (tid < 32) {
            const int y = t0 + tid;
            const bool valid = y < NS;
            const int yc = valid ? y : NS - 1;
            if (has_ids) pre_id = nrx_load_id(a.ids, yc, a.idx64 != 0);
            if (BIAS && MODE != IB_DV) pre_bias = a.bias[yc];                 // (past the end: the last column's finite value, masked where used)
            if (MODE == IB_DV) {
                const float l = a.lse[yc], gg = a.g[yc];
                pre_lse = valid ? l : 0.f;
                pre_gi = valid ? gg * inv_t : 0.f;
            }
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int c = tid + n * NRX_BLOCK;
            if (c < TOTAL) {
                const int row = c / CH, ch = c % CH;
                *reinterpret_cast<float4*>(&t_s[buf][row * LD + 4 * ch]) = pre[n];
            }
        }
        if (tid < 32) {
            id_s[buf][tid] = pre_id;
            if (BIAS && MODE != IB_DV) bias_s[buf][tid] = pre_bias;
            if (MODE == IB_DV) { lse_s[buf][tid] = pre_lse; gi_s[buf][tid] = pre_gi; }
        }
    };

    float m = -FLT_MAX, sum = 0.f, dg = 0.f;          // forward state (-FLT_MAX, not -inf: exp(m - m) must be 1 while nothing is kept yet)
    bool have_dg = false;
    f32x16 o[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[nb][r] = 0.f;

    auto compute = [&](int buf, int t0) {
        const float* ts = t_s[buf];
        float af[H];
#pragma unroll
        for (int v = 0; v < H4; ++v) {
            const float4 t = *reinterpret_cast<const float4*>(&ts[l31 * LD + e_base + 4 * v]);
            af[4 * v + 0] = t.x; af[4 * v + 1] = t.y; af[4 * v + 2] = t.z; af[4 * v + 3] = t.w;
        }
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < H; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], qf[s], acc, 0, 0, 0);

        const bool diag_tile = t0 == own0;            // tiles and owned groups are both 32-aligned: the diagonal lives in one tile
        const bool tail = t0 + 32 > NS;
#define IB_ROW(r_) (4 * hi + ((r_) & 3) + 8 * ((r_) >> 2))
        unsigned keep = 0xFFFFu;
        if (has_ids) {
#pragma unroll
            for (int r = 0; r < 16; ++r) keep &= ~((id_s[buf][IB_ROW(r)] == my_id ? 1u : 0u) << r);
        }
        unsigned dbit = 0u;
        if (diag_tile) dbit = 1u << ((l31 & 3) + 4 * (l31 >> 3));        // the register whose row is x -- held by the lane half with hi == (l31 >> 2) & 1
        if (diag_tile && hi != ((l31 >> 2) & 1)) dbit = 0u;
        keep |= dbit;
        if (tail) {
#pragma unroll
            for (int r = 0; r < 16; ++r) keep &= ~((t0 + IB_ROW(r) >= NS ? 1u : 0u) << r);
            dbit &= keep;                             // dV of a rectangle: an owned candidate past the last user has no diagonal
        }
#define IB_Z(r_) (BIAS ? ib_logit(acc[r_], inv_t, MODE == IB_DV ? my_bias : bias_s[buf][IB_ROW(r_)]) : ib_score(acc[r_], inv_t))

        if (MODE == IB_FWD) {
            float sc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = ((keep >> r) & 1u) ? IB_Z(r) : -INFINITY;
            if (dbit != 0u) {
#pragma unroll
                for (int r = 0; r < 16; ++r) if ((dbit >> r) & 1u) dg = sc[r];
                have_dg = true;
            }
            float tm = sc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) tm = fmaxf(tm, sc[r]);
            const float mn = fmaxf(m, tm);
            float add = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) add += ib_exp(sc[r] - mn);
            sum = sum * ib_exp(m - mn) + add;
            m = mn;
        } else {
            float c[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = IB_Z(r);
                const float l = MODE == IB_DU ? my_lse : lse_s[buf][IB_ROW(r)];
                const float gi = MODE == IB_DU ? my_gi : gi_s[buf][IB_ROW(r)];
                float p = ((keep >> r) & 1u) ? ib_exp(s - l) : 0.f;
                if ((dbit >> r) & 1u) p -= 1.f;
                c[r] = gi * p;
            }
            // (columns >= P of a staged row are never written when the padded dim is below 32: lanes l31 >= P read whatever LDS holds.  Row e of
            // this product's A operand feeds output row e alone, and rows e >= dim are never stored.)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    o[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ts[IB_ROW(r) * LD + 32 * nb + l31], c[r], o[nb], 0, 0, 0);
        }
#undef IB_Z
#undef IB_ROW
    };

    const int split = blockIdx.y;
    const int64_t begin64 = (int64_t)split * a.per_split;
    const int begin = (int)(begin64 < NS ? begin64 : NS);
    const int end = (int)(begin64 + a.per_split < NS ? begin64 + a.per_split : NS);
    const int ntiles = (end - begin + 31) / 32;                 // block-uniform: every wave meets every barrier
    if (ntiles > 0) { gload(begin); sstore(0); }
    __syncthreads();
    for (int it = 0; it < ntiles; ++it) {
        const int t0 = begin + 32 * it;
        const bool more = it + 1 < ntiles;
        if (more) gload(t0 + 32);
        compute(it & 1, t0);
        if (more) sstore((it & 1) ^ 1);                        // last read in iteration it - 1, which every wave left through the barrier
        __syncthreads();
    }

    if (MODE == IB_FWD) {
        const float mo = __shfl_xor(m, 32, 64), so = __shfl_xor(sum, 32, 64);
        const float m0 = hi ? mo : m, m1 = hi ? m : mo, s0 = hi ? so : sum, s1 = hi ? sum : so;
        const float M = fmaxf(m0, m1);
        const float S = s0 * ib_exp(m0 - M) + s1 * ib_exp(m1 - M);
        if (live && hi == 0) {
            a.pm[(int64_t)x * gridDim.y + split] = M;
            a.ps[(int64_t)x * gridDim.y + split] = S;
        }
        if (live && have_dg) a.diag[x] = dg;
    } else if (live) {
        float* op = a.out + (int64_t)split * a.out_split_stride + (int64_t)x * a.out_ld;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e0 = 32 * nb + 8 * q + 4 * hi;
                if (e0 < dim) nrx_stg4(op + e0, 0, make_float4(o[nb][4 * q + 0], o[nb][4 * q + 1], o[nb][4 * q + 2], o[nb][4 * q + 3]));
            }
    }
}

// forward: merge the splits' (max, sum) pairs of a row in split order
__global__ __launch_bounds__(NRX_BLOCK) void inbatch_fwd_finish_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                                       const float* __restrict__ diag, int B, int splits,
                                                                       float* __restrict__ row_loss, float* __restrict__ row_lse) {
    const int x = blockIdx.x * NRX_BLOCK + threadIdx.x;
    if (x >= B) return;
    float M = -FLT_MAX;
    for (int k = 0; k < splits; ++k) M = fmaxf(M, pm[(int64_t)x * splits + k]);
    float S = 0.f;
    for (int k = 0; k < splits; ++k) S += ps[(int64_t)x * splits + k] * ib_exp(pm[(int64_t)x * splits + k] - M);
    const float lse = M + __builtin_amdgcn_logf(S) * 0.69314718055994530942f;
    row_lse[x] = lse;
    row_loss[x] = lse - diag[x];
}

// backward: out[x, :] = part[0][x, :] + part[1][x, :] + ...  (split order)
__global__ __launch_bounds__(NRX_BLOCK) void inbatch_bwd_finish_kernel(const float* __restrict__ part, int B, int dim, int splits,
                                                                       float* __restrict__ out, int64_t out_ld) {
    const int q = dim >> 2;
    const int64_t i = (int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x;
    if (i >= (int64_t)B * q) return;
    const int64_t x = i / q;
    const int e = (int)(i % q) * 4;
    float4 s = nrx_ldg4(part + x * dim + e, 0);
    for (int k = 1; k < splits; ++k) {
        const float4 t = nrx_ldg4(part + ((int64_t)k * B + x) * dim + e, 0);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    nrx_stg4(out + x * out_ld + e, 0, s);
}

// the splits of ONE launch: its owned rows make the blocks, its streamed rows are cut up (owned == streamed: the in-batch op's choice)
int choose_splits(int64_t owned, int64_t streamed) {
    if (streamed < 512 || owned < 1) return 1;       // (an empty side included)
    const int64_t xb = (owned + 32 * WAVES - 1) / (32 * WAVES);
    int64_t s = (512 + xb - 1) / xb;                 // aim at >= 512 blocks (2 per CU)
    const int64_t max_s = streamed / 256;            // ... of >= 256 streamed rows each
    if (s > max_s) s = max_s;
    if (s > 16) s = 16;
    if (s < 1) s = 1;
    return (int)s;
}

int resolve_splits(int32_t col_splits, int64_t owned, int64_t streamed) { return col_splits > 0 ? col_splits : choose_splits(owned, streamed); }

template <int MODE, bool BIAS>
void inbatch_launch_h4(int H4, dim3 grid, hipStream_t st, const InbatchArgs& a) {
    switch (H4) {
        case 1: hipLaunchKernelGGL((inbatch_kernel<MODE, 1, BIAS>), grid, dim3(NRX_BLOCK), 0, st, a); break;
        case 2: hipLaunchKernelGGL((inbatch_kernel<MODE, 2, BIAS>), grid, dim3(NRX_BLOCK), 0, st, a); break;
        case 4: hipLaunchKernelGGL((inbatch_kernel<MODE, 4, BIAS>), grid, dim3(NRX_BLOCK), 0, st, a); break;
        default: hipLaunchKernelGGL((inbatch_kernel<MODE, 8, BIAS>), grid, dim3(NRX_BLOCK), 0, st, a); break;
    }
}

template <int MODE>
void inbatch_launch(int H4, dim3 grid, hipStream_t st, const InbatchArgs& a) {
    if (a.bias != nullptr) inbatch_launch_h4<MODE, true>(H4, grid, st, a);
    else inbatch_launch_h4<MODE, false>(H4, grid, st, a);
}

// the checks every entry point shares (the in-batch ones pass n_cand = batch); NRX_OK or the status to return
int inbatch_check(const char* who, int64_t batch, int64_t n_cand, int32_t dim, int32_t col_splits) {
    if (batch < 0 || batch >= 0x7fffffffLL - 32 * WAVES) { nrx_set_error("%s: bad argument (batch %lld)", who, (long long)batch); return NRX_ERR_BAD_ARG; }
    if (n_cand < batch || n_cand >= 0x7fffffffLL - 32 * WAVES) {
        nrx_set_error("%s: bad argument (n_cand %lld: batch %lld <= n_cand < 2^31 - %d; column i < batch is row i's positive)", who,
                      (long long)n_cand, (long long)batch, 32 * WAVES);
        return NRX_ERR_BAD_ARG;
    }
    if (dim < 4 || (dim & 3) != 0 || dim > 128) {
        nrx_set_error("%s: bad argument (dim %d: rows are whole float4s, 4 <= dim <= 128)", who, dim);
        return NRX_ERR_BAD_ARG;
    }
    if (col_splits < 0 || col_splits > IB_MAX_SPLITS) {
        nrx_set_error("%s: bad argument (col_splits %d: 0 = choose, at most %d)", who, col_splits, IB_MAX_SPLITS);
        return NRX_ERR_BAD_ARG;
    }
    if (dim > 64) { nrx_set_error("%s: supports dim %% 4 == 0 with 4 <= dim <= 64 (got dim=%d)", who, dim); return NRX_ERR_UNSUPPORTED; }
    return NRX_OK;
}

bool inbatch_ids_ok(const void* ids, int32_t bits) {
    return ids == nullptr || (reinterpret_cast<uintptr_t>(ids) & (bits == 64 ? 7u : 3u)) == 0;
}

bool inbatch_f32_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int inbatch_h4(int dim) { return dim <= 8 ? 1 : (dim <= 16 ? 2 : (dim <= 32 ? 4 : 8)); }

float* inbatch_ws(void* workspace) { return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255); }

int32_t inbatch_per_split(int64_t streamed, int S) { return (int32_t)((((streamed + S - 1) / S) + 31) & ~31ll); }

// forward partials: batch * (2 splits + 1); backward partials of one role: splits * owned * dim (one split writes the output itself)
int64_t cand_workspace(const char* who, int64_t batch, int64_t n_cand, int32_t dim, int32_t col_splits) {
    if (inbatch_check(who, batch, n_cand, dim, col_splits) != NRX_OK) return -1;
    const int64_t Su = resolve_splits(col_splits, batch, n_cand), Sv = resolve_splits(col_splits, n_cand, batch);
    int64_t need = (2 * Su + 1) * batch;
    if (Su > 1 && Su * batch * dim > need) need = Su * batch * dim;
    if (Sv > 1 && Sv * n_cand * dim > need) need = Sv * n_cand * dim;
    return 4 * need + 256;
}

int cand_fwd(const char* who, const float* u, int64_t u_ld, const float* v, int64_t v_ld, int64_t batch, int64_t n_cand, int32_t dim,
             float inv_temperature, const void* cand_ids, int32_t index_bits, const float* col_bias, int32_t col_splits, float* row_loss,
             float* row_lse, void* workspace, void* stream) {
    const int rc = inbatch_check(who, batch, n_cand, dim, col_splits);
    if (rc != NRX_OK) return rc;
    NRX_REQUIRE(inv_temperature > 0.f && inv_temperature <= FLT_MAX, "%s: bad argument (inv_temperature must be positive and finite)", who);
    NRX_REQUIRE(index_bits == 32 || index_bits == 64, "%s: bad argument (index_bits %d: 32 or 64)", who, index_bits);
    NRX_REQUIRE(u_ld >= dim && v_ld >= dim, "%s: bad argument (row stride below dim)", who);
    if (batch == 0) return NRX_OK;
    NRX_REQUIRE(u && v && row_loss && row_lse && workspace, "%s: null buffer", who);
    NRX_REQUIRE(nrx_aligned16(u) && nrx_aligned16(v) && (u_ld & 3) == 0 && (v_ld & 3) == 0,
                "%s: misaligned rows (u / v and their row strides must keep every row 16-byte aligned)", who);
    NRX_REQUIRE(inbatch_f32_ok(row_loss) && inbatch_f32_ok(row_lse) && inbatch_f32_ok(col_bias) && inbatch_ids_ok(cand_ids, index_bits),
                "%s: misaligned pointer", who);
    const int S = resolve_splits(col_splits, batch, n_cand);
    float* ws = inbatch_ws(workspace);
    InbatchArgs a = {};
    a.own = u; a.own_ld = u_ld; a.str = v; a.str_ld = v_ld;
    a.ids = cand_ids; a.idx64 = index_bits == 64; a.bias = col_bias;
    a.pm = ws; a.ps = ws + (int64_t)S * batch; a.diag = ws + 2 * (int64_t)S * batch;
    a.n_own = (int32_t)batch; a.n_str = (int32_t)n_cand; a.dim = dim; a.inv_t = inv_temperature;
    a.per_split = inbatch_per_split(n_cand, S);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((batch + 32 * WAVES - 1) / (32 * WAVES)), (unsigned)S);
    inbatch_launch<IB_FWD>(inbatch_h4(dim), grid, st, a);
    hipLaunchKernelGGL(inbatch_fwd_finish_kernel, dim3((unsigned)((batch + NRX_BLOCK - 1) / NRX_BLOCK)), dim3(NRX_BLOCK), 0, st,
                       a.pm, a.ps, a.diag, (int)batch, S, row_loss, row_lse);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

int cand_bwd(const char* who, const float* u, int64_t u_ld, const float* v, int64_t v_ld, int64_t batch, int64_t n_cand, int32_t dim,
             float inv_temperature, const void* cand_ids, int32_t index_bits, const float* col_bias, int32_t col_splits, const float* row_lse,
             const float* g_row, float* g_u, int64_t gu_ld, float* g_v, int64_t gv_ld, void* workspace, void* stream) {
    const int rc = inbatch_check(who, batch, n_cand, dim, col_splits);
    if (rc != NRX_OK) return rc;
    NRX_REQUIRE(inv_temperature > 0.f && inv_temperature <= FLT_MAX, "%s: bad argument (inv_temperature must be positive and finite)", who);
    NRX_REQUIRE(index_bits == 32 || index_bits == 64, "%s: bad argument (index_bits %d: 32 or 64)", who, index_bits);
    NRX_REQUIRE(u_ld >= dim && v_ld >= dim && (g_u == nullptr || gu_ld >= dim) && (g_v == nullptr || gv_ld >= dim),
                "%s: bad argument (row stride below dim)", who);
    if (batch == 0 || (g_u == nullptr && g_v == nullptr)) return NRX_OK;
    NRX_REQUIRE(u && v && row_lse && g_row && workspace, "%s: null buffer", who);
    NRX_REQUIRE(nrx_aligned16(u) && nrx_aligned16(v) && (u_ld & 3) == 0 && (v_ld & 3) == 0 && nrx_aligned16(g_u) && nrx_aligned16(g_v) &&
                (g_u == nullptr || (gu_ld & 3) == 0) && (g_v == nullptr || (gv_ld & 3) == 0),
                "%s: misaligned rows (u / v / g_u / g_v and their row strides must keep every row 16-byte aligned)", who);
    NRX_REQUIRE(inbatch_f32_ok(row_lse) && inbatch_f32_ok(g_row) && inbatch_f32_ok(col_bias) && inbatch_ids_ok(cand_ids, index_bits),
                "%s: misaligned pointer", who);
    float* ws = inbatch_ws(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H4 = inbatch_h4(dim);
    InbatchArgs a = {};
    a.ids = cand_ids; a.idx64 = index_bits == 64; a.bias = col_bias;
    a.lse = row_lse; a.g = g_row;
    a.dim = dim; a.inv_t = inv_temperature;
    // the same kernel with the roles swapped; with splits the partial sums of the first role are folded before the second one reuses the workspace
    for (int role = 0; role < 2; ++role) {
        float* dst = role == 0 ? g_u : g_v;
        const int64_t dst_ld = role == 0 ? gu_ld : gv_ld;
        if (dst == nullptr) continue;
        const int64_t owned = role == 0 ? batch : n_cand, streamed = role == 0 ? n_cand : batch;
        const int S = resolve_splits(col_splits, owned, streamed);
        a.own = role == 0 ? u : v; a.own_ld = role == 0 ? u_ld : v_ld;
        a.str = role == 0 ? v : u; a.str_ld = role == 0 ? v_ld : u_ld;
        a.n_own = (int32_t)owned; a.n_str = (int32_t)streamed;
        a.per_split = inbatch_per_split(streamed, S);
        if (S > 1) { a.out = ws; a.out_ld = dim; a.out_split_stride = owned * (int64_t)dim; }
        else { a.out = dst; a.out_ld = dst_ld; a.out_split_stride = 0; }
        const dim3 grid((unsigned)((owned + 32 * WAVES - 1) / (32 * WAVES)), (unsigned)S);
        if (role == 0) inbatch_launch<IB_DU>(H4, grid, st, a);
        else inbatch_launch<IB_DV>(H4, grid, st, a);
        if (S > 1) {
            const unsigned fgrid = (unsigned)((owned * (dim >> 2) + NRX_BLOCK - 1) / NRX_BLOCK);
            hipLaunchKernelGGL(inbatch_bwd_finish_kernel, dim3(fgrid), dim3(NRX_BLOCK), 0, st, ws, (int)owned, (int)dim, S, dst, dst_ld);
        }
    }
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

}  // namespace

// ---- the in-batch op: the candidate set is the batch itself and no column carries a bias
extern "C" int64_t nrx_inbatch_softmax_workspace(int64_t batch, int32_t dim, int32_t col_splits) {
    return cand_workspace("nrx_inbatch_softmax_workspace", batch, batch, dim, col_splits);
}

extern "C" int nrx_inbatch_softmax_fwd(const float* u, int64_t u_ld, const float* v, int64_t v_ld, int64_t batch, int32_t dim,
                                       float inv_temperature, const void* item_ids, int32_t index_bits, int32_t col_splits, float* row_loss,
                                       float* row_lse, void* workspace, void* stream) {
    NRX_TRACE();
    return cand_fwd("nrx_inbatch_softmax_fwd", u, u_ld, v, v_ld, batch, batch, dim, inv_temperature, item_ids, index_bits, nullptr, col_splits,
                    row_loss, row_lse, workspace, stream);
}

extern "C" int nrx_inbatch_softmax_bwd(const float* u, int64_t u_ld, const float* v, int64_t v_ld, int64_t batch, int32_t dim,
                                       float inv_temperature, const void* item_ids, int32_t index_bits, int32_t col_splits,
                                       const float* row_lse, const float* g_row, float* g_u, int64_t gu_ld, float* g_v, int64_t gv_ld,
                                       void* workspace, void* stream) {
    NRX_TRACE();
    return cand_bwd("nrx_inbatch_softmax_bwd", u, u_ld, v, v_ld, batch, batch, dim, inv_temperature, item_ids, index_bits, nullptr, col_splits,
                    row_lse, g_row, g_u, gu_ld, g_v, gv_ld, workspace, stream);
}

// ---- the candidate op: n_cand >= batch rows of v (row i < batch is row i's positive), ids and bias per candidate
extern "C" int64_t nrx_cand_softmax_workspace(int64_t batch, int64_t n_cand, int32_t dim, int32_t col_splits) {
    return cand_workspace("nrx_cand_softmax_workspace", batch, n_cand, dim, col_splits);
}

extern "C" int nrx_cand_softmax_fwd(const float* u, int64_t u_ld, const float* v, int64_t v_ld, int64_t batch, int64_t n_cand, int32_t dim,
                                    float inv_temperature, const void* cand_ids, int32_t index_bits, const float* col_bias, int32_t col_splits,
                                    float* row_loss, float* row_lse, void* workspace, void* stream) {
    NRX_TRACE();
    return cand_fwd("nrx_cand_softmax_fwd", u, u_ld, v, v_ld, batch, n_cand, dim, inv_temperature, cand_ids, index_bits, col_bias, col_splits,
                    row_loss, row_lse, workspace, stream);
}

extern "C" int nrx_cand_softmax_bwd(const float* u, int64_t u_ld, const float* v, int64_t v_ld, int64_t batch, int64_t n_cand, int32_t dim,
                                    float inv_temperature, const void* cand_ids, int32_t index_bits, const float* col_bias, int32_t col_splits,
                                    const float* row_lse, const float* g_row, float* g_u, int64_t gu_ld, float* g_v, int64_t gv_ld,
                                    void* workspace, void* stream) {
    NRX_TRACE();
    return cand_bwd("nrx_cand_softmax_bwd", u, u_ld, v, v_ld, batch, n_cand, dim, inv_temperature, cand_ids, index_bits, col_bias, col_splits,
                    row_lse, g_row, g_u, gu_ld, g_v, gv_ld, workspace, stream);
}

