// Attentional pooling of pairwise field interactions (the pair-wise interaction and attention layers of the Attentional Factorization
// Machine; Xiao et al., IJCAI 2017): forward and backward on the matrix cores with nothing of size batch * P in between.  No reference
// counterpart; DESIGN 7k.
//
// Definition (include/nrx_embed.h restates it, with every fp32 chain): e_f = x[b * ld + field_off[f] .. + dim), pairs p = (i, j), j < i,
//   h_p = e_i (.) e_j,  z_p,t = b1[t] + sum_d W1[t, d] h_p[d],  a_p = sum_t w2[t] relu(z_p,t),  alpha = softmax_p(a),  out = sum_p alpha_p h_p.
//
// v_mfma_f32_32x32x2_f32 is bit for bit fma(a_k1, b_k1, fma(a_k0, b_k0, c)); its A operand is lane l <- A[l & 31][l >> 5], its B operand lane
// l <- B[l >> 5][l & 31], its C layout column l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.
//
// ONE WAVE OWNS ONE SAMPLE at a time (4 waves per workgroup; W1 -- zero padded to whole tiles --, b1 and w2 are staged in LDS once per
// workgroup, which walks samples in a bounded grid).  The wave stages the sample's F field rows in LDS with an odd row stride.
//   scores  : Z^T = W1 H^T in tiles of 32 pairs.  A operand: W1[t][2 s + kk] from LDS (lanes along t, odd stride).  B operand: lane (pair, kk)
//             multiplies out fl(e_i[2 s + kk] e_j[2 s + kk]) from two LDS reads.  The accumulator starts at b1.  C: the pair on the lane, 16 (32)
//             attention units in registers: relu, the w2 dot and one exchange between the lane halves are register arithmetic.
//   forward : pairs in tril order through a (i, j) table in LDS; the P scores go to LDS, the softmax is two-pass; the pooling is VALU work:
//             lane (d, q) runs the pairs p = q, q + G, .. (G = 64 / dim) and the G partial sums are added in ascending q.
//   backward: a tile has a FIXED i and 32 consecutive j: the walk covers the full F x F grid (every pair twice), which buys the reduction
//             onto field i inside the tile: one owner, a fixed order, no atomics.  Per tile: the scores again; alpha = exp(a - lse);
//             da; g_h^T = alpha g_out + W1^T U as a second GEMM whose B operand IS the score accumulator (the K order is the C layout's row
//             order, the A operand is permuted to match: no exchange); c = g_h (.) e_j goes through LDS and lane d adds the tile's 32 terms in
//             ascending j.
//   g_W1    : a third GEMM U H over the pairs j < i of the tile (each pair once), relu(z) transposed through LDS, accumulated IN REGISTERS
//             across the samples of a slice: a wave owns one slice of AFM_SLICE consecutive samples.  g_b1 and g_w2 are the running sums of the
//             same A operand.  Partials [slice][A dim + 2 A] go to the workspace; afm_reduce_kernel adds them in slice order.
// Loads are never behind a branch (a dead lane reads a valid address and selects 0).
#include "nrx_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int AFM_MAX = 64;                    // F, dim, A
constexpr int AFM_WAVES = 4;                   // waves (samples, slices in flight) per workgroup
constexpr int AFM_SLICE = 16;                  // samples per weight-gradient slice
constexpr int AFM_MAX_BLOCKS = 1024;           // the bounded grid
constexpr int AFM_LDS = 160 * 1024;
constexpr int AFM_TS = 33;                     // row stride of the 32-column transposition buffers

struct AfmArgs {
    const float* x;
    const float* W1;
    const float* b1;
    const float* w2;
    float* out;              // forward: written; backward: read
    float* lse;
    const float* g_out;
    float* g_x;
    float* part;             // [slices][A dim + 2 A]
    int64_t ld, out_ld, go_ld, gx_ld, batch;
    int32_t F, dim, A, P;
    int32_t off[AFM_MAX];
};

__device__ __forceinline__ int afm_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// W1 as [32 MT][WS] (rows t >= A and columns d >= dim hold 0), b1 and w2 as [64] (0 from A on)
__device__ __forceinline__ void afm_stage_params(const AfmArgs& a, float* w1s, float* b1s, float* w2s, int rows, int cols, int WS, int tid) {
    for (int idx = tid; idx < rows * cols; idx += AFM_WAVES * 64) {
        const int t = idx / cols, d = idx - t * cols;
        const bool in = t < a.A && d < a.dim;
        const float v = ((const NRX_GLOBAL float*)a.W1)[in ? t * a.dim + d : 0];
        w1s[t * WS + d] = in ? v : 0.f;
    }
    if (tid < 64) {
        const float vb = ((const NRX_GLOBAL float*)a.b1)[tid < a.A ? tid : 0], vw = ((const NRX_GLOBAL float*)a.w2)[tid < a.A ? tid : 0];
        b1s[tid] = tid < a.A ? vb : 0.f;
        w2s[tid] = tid < a.A ? vw : 0.f;
    }
}

// the sample's field rows to LDS as [F][DS], 16-byte loads
__device__ __forceinline__ void afm_stage_fields(const NRX_CONST AfmArgs* ka, const AfmArgs& a, float* E, int64_t b, int DS, int lane) {
    const int qd = a.dim >> 2, nq = a.F * qd;
    const float* row = a.x + b * a.ld;
    for (int q = lane; q < nq; q += 64) {
        const int f = q / qd, c = (q - f * qd) * 4;
        const nrx_f32x4 v = *(const NRX_GLOBAL nrx_f32x4*)(row + ka->off[f] + c);
        float* e = E + f * DS + c;
        e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
    }
}

// one tile of scores: z[t][pair] = chain from b1[t] over d ascending of fmaf(W1[t][d], fl(e_i[d] e_j[d]), .); BWD: dal = this lane half's
// part of <g_out, h_p>, the chain from 0 over its d (kk, kk + 2, ..) of fmaf(g_out[d], h_p[d], .)
template <int MT, bool BWD>
__device__ __forceinline__ void afm_score(f32x16 (&z)[MT], float& dal, const float* w1s, const float* b1s, const float* ei, const float* ej,
                                          const float* gs, bool valid, int D, int WS, int r, int kk) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) z[mt][q] = b1s[32 * mt + afm_row(q, kk)];
    dal = 0.f;
    const int nsteps = D >> 1;
    for (int s = 0; s < nsteps; ++s) {
        const int d = 2 * s + kk;
        const float pv = ei[d], qv = ej[d];
        const float h = valid ? pv * qv : 0.f;
        if constexpr (BWD) dal = fmaf(gs[d], h, dal);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) z[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1s[(32 * mt + r) * WS + d], h, z[mt], 0, 0, 0);
    }
}

// a_p: each lane half runs the chain from 0 over its rows t ascending of fmaf(w2[t], relu(z_t), .); the halves are added
template <int MT>
__device__ __forceinline__ float afm_logit(const f32x16 (&z)[MT], const float* w2s, int kk) {
    float sa = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) sa = fmaf(w2s[32 * mt + afm_row(q, kk)], z[mt][q] > 0.f ? z[mt][q] : 0.f, sa);
    return sa + __shfl_xor(sa, 32);
}

__device__ __forceinline__ float afm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

template <int MT>
__global__ __launch_bounds__(AFM_WAVES * 64) void afm_fwd_kernel(const AfmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float afm_smem[];
    const NRX_CONST AfmArgs* ka = nrx_kernarg<AfmArgs>();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
    const int F = a.F, D = a.dim, P = a.P, DS = D | 1, WS = D | 1, ntiles = (P + 31) >> 5;
    float* w1s = afm_smem;                                     // [32 MT][WS]
    float* b1s = w1s + 32 * MT * WS;
    float* w2s = b1s + 64;
    int* tab = (int*)(w2s + 64);                               // [32 ntiles]: i << 8 | j of pair p
    float* E = (float*)(tab + 32 * ntiles) + wave * (F * DS + 32 * ntiles + 64);
    float* sc = E + F * DS;                                    // [32 ntiles]: a_p, then exp(a_p - max), then alpha_p
    float* pbuf = sc + 32 * ntiles;                            // [64]
    afm_stage_params(a, w1s, b1s, w2s, 32 * MT, D, WS, tid);
    for (int p = tid; p < 32 * ntiles; p += AFM_WAVES * 64) {
        int i = 1, j = 0;
        if (p < P) {
            i = (int)((1.f + sqrtf(1.f + 8.f * (float)p)) * 0.5f);
            while (i * (i - 1) / 2 > p) --i;
            while ((i + 1) * i / 2 <= p) ++i;
            j = p - i * (i - 1) / 2;
        }
        tab[p] = (i << 8) | j;
    }
    const int G = 64 / D, q_l = lane / D, d_l = lane - q_l * D;
    const int64_t wstride = (int64_t)gridDim.x * AFM_WAVES;
    const int64_t iters = (a.batch + wstride - 1) / wstride;   // the same for every wave of the grid: the barriers below are uniform
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t b = (it * gridDim.x + blockIdx.x) * AFM_WAVES + wave;
        const bool live = b < a.batch;
        __syncthreads();                                       // the sample before this one is read (and the parameters are staged)
        afm_stage_fields(ka, a, E, live ? b : 0, DS, lane);
        __syncthreads();
        for (int tile = 0; tile < ntiles; ++tile) {
            const int p = 32 * tile + r;
            const bool valid = p < P;
            const int pr = tab[p];
            f32x16 z[MT];
            float dal;
            afm_score<MT, false>(z, dal, w1s, b1s, E + (pr >> 8) * DS, E + (pr & 255) * DS, nullptr, valid, D, WS, r, kk);
            const float av = afm_logit<MT>(z, w2s, kk);
            if (kk == 0 && valid) sc[p] = av;
        }
        __syncthreads();
        // two-pass softmax; a lane touches its own p = lane, lane + 64, .. only
        float m = -INFINITY;
        for (int p = lane; p < P; p += 64) m = fmaxf(m, sc[p]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float ls = 0.f;
        for (int p = lane; p < P; p += 64) {
            const float e = expf(sc[p] - m);
            sc[p] = e;
            ls = ls + e;
        }
        ls = afm_wave_sum(ls);
        for (int p = lane; p < P; p += 64) sc[p] = sc[p] / ls;
        __syncthreads();
        float acc = 0.f;
        if (q_l < G)
            for (int p = q_l; p < P; p += G) {
                const int pr = tab[p];
                const float h = E[(pr >> 8) * DS + d_l] * E[(pr & 255) * DS + d_l];
                acc = fmaf(sc[p], h, acc);
            }
        pbuf[lane] = acc;
        __syncthreads();
        if (lane < D) {
            float o = pbuf[lane];
            for (int q = 1; q < G; ++q) o = o + pbuf[q * D + lane];
            if (live) ((NRX_GLOBAL float*)a.out)[b * a.out_ld + lane] = o;
        }
        if (lane == 0 && live) ((NRX_GLOBAL float*)a.lse)[b] = m + logf(ls);
    }
}

template <int MT, int DT>
__global__ __launch_bounds__(AFM_WAVES * 64) void afm_bwd_kernel(const AfmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float afm_smem[];
    const NRX_CONST AfmArgs* ka = nrx_kernarg<AfmArgs>();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
    const int F = a.F, D = a.dim, A = a.A, DS = D | 1;
    constexpr int WS = 32 * DT + 1;
    float* w1s = afm_smem;                                     // [32 MT][WS]
    float* b1s = w1s + 32 * MT * WS;
    float* w2s = b1s + 64;
    float* E = w2s + 64 + wave * (F * DS + 128 + 32 * MT * AFM_TS + 32 + 32 * DT * AFM_TS);
    float* gs = E + F * DS;                                    // [64] g_out, 0 from dim on
    float* os = gs + 64;                                       // [64] out
    float* zb = os + 64;                                       // [32 MT][33] relu(z) of the tile, t major
    float* dab = zb + 32 * MT * AFM_TS;                        // [32] da of the tile's pairs
    float* cbuf = dab + 32;                                    // [32 DT][33] g_h (.) e_j of the tile, d major
    afm_stage_params(a, w1s, b1s, w2s, 32 * MT, 32 * DT, WS, tid);
    const int JB = F > 32 ? 2 : 1;
    const int64_t slices = (a.batch + AFM_SLICE - 1) / AFM_SLICE;
    const int64_t wstride = (int64_t)gridDim.x * AFM_WAVES;
    const int64_t iters = (slices + wstride - 1) / wstride;    // uniform over the grid
    const int n_el = A * D + 2 * A;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t slice0 = (it * gridDim.x + blockIdx.x) * AFM_WAVES, slice = slice0 + wave;
        // the samples of the workgroup's first slice bound the loop (uniform over the workgroup: a later slice has no more)
        const int64_t left = a.batch - slice0 * AFM_SLICE;
        const int cnt = left < 0 ? 0 : left < AFM_SLICE ? (int)left : AFM_SLICE;
        f32x16 acc3[MT][DT];
        float gb1[MT], gw2[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            gb1[mt] = 0.f;
            gw2[mt] = 0.f;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) acc3[mt][dt] = f32x16{};
        }
        for (int si = 0; si < cnt; ++si) {
            const int64_t b = slice * AFM_SLICE + si;
            const bool live = b < a.batch;
            const int64_t bb = live ? b : 0;
            __syncthreads();
            afm_stage_fields(ka, a, E, bb, DS, lane);
            {
                const int dc = lane < D ? lane : 0;
                const float gv = ((const NRX_GLOBAL float*)a.g_out)[bb * a.go_ld + dc], ov = ((const NRX_GLOBAL float*)a.out)[bb * a.out_ld + dc];
                gs[lane] = lane < D ? gv : 0.f;
                os[lane] = lane < D ? ov : 0.f;
            }
            const float lsev = ((const NRX_GLOBAL float*)a.lse)[bb];
            __syncthreads();
            float delta = 0.f;
            for (int d = 0; d < D; ++d) delta = fmaf(gs[d], os[d], delta);
            for (int i = 0; i < F; ++i) {
                float gacc = 0.f;
                for (int jb = 0; jb < JB; ++jb) {
                    const int j = 32 * jb + r;
                    const bool valid = live && j < F && j != i;
                    const float* ei = E + i * DS;
                    const float* ej = E + (valid ? j : 0) * DS;
                    f32x16 z[MT];
                    float dal;
                    afm_score<MT, true>(z, dal, w1s, b1s, ei, ej, gs, valid, D, WS, r, kk);
                    const float av = afm_logit<MT>(z, w2s, kk);
                    const float dalpha = dal + __shfl_xor(dal, 32);
                    const float alpha = valid ? expf(av - lsev) : 0.f;
                    const float da = alpha * (dalpha - delta);
                    // relu(z) of the tile to LDS, t major (the A operand of the weight gradient); da beside it
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int q = 0; q < 16; ++q) zb[(32 * mt + afm_row(q, kk)) * AFM_TS + r] = z[mt][q] > 0.f ? z[mt][q] : 0.f;
                    if (kk == 0) dab[r] = da;
                    // g_h^T [d][pair] = alpha g_out[d], then the chain over t in the C layout's row order of fmaf(W1[t][d], u_t, .)
                    f32x16 gh[DT];
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                        for (int q = 0; q < 16; ++q) gh[dt][q] = alpha * gs[32 * dt + afm_row(q, kk)];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const int rows = A - 32 * mt < 32 ? A - 32 * mt : 32;         // rows of this tile that exist: 8 per 4 steps
#pragma unroll
                        for (int s = 0; s < 16; ++s) {
                            if (8 * (s >> 2) < rows) {                                 // (wave-uniform)
                                const int t = 32 * mt + afm_row(s, kk);
                                const float u = z[mt][s] > 0.f ? da * w2s[t] : 0.f;
#pragma unroll
                                for (int dt = 0; dt < DT; ++dt)
                                    gh[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1s[t * WS + 32 * dt + r], u, gh[dt], 0, 0, 0);
                            }
                        }
                    }
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int d = 32 * dt + afm_row(q, kk);
                            cbuf[d * AFM_TS + r] = gh[dt][q] * ej[d < D ? d : 0];
                        }
                    __syncthreads();
                    // field i's gradient: lane d adds the tile's 32 terms in ascending j (a pair that does not exist adds 0)
                    if (lane < D)
                        for (int c = 0; c < 32; ++c) gacc = gacc + cbuf[lane * AFM_TS + c];
                    // the weight gradient over the tile's pairs j < i: steps 2 s + kk < i - 32 jb
                    const int npair = i - 32 * jb < 0 ? 0 : i - 32 * jb < 32 ? i - 32 * jb : 32;
                    const int nst = (npair + 1) >> 1;
                    for (int s = 0; s < nst; ++s) {
                        const int jl = 2 * s + kk;
                        const bool ok = jl < npair;
                        const float dav = ok ? dab[jl] : 0.f;
                        const float* e2 = E + (32 * jb + (ok ? jl : 0)) * DS;
                        float hv[DT];
#pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            const int d = 32 * dt + r;
                            const float pv = ei[d < D ? d : 0], qv = e2[d < D ? d : 0];
                            hv[dt] = ok && d < D ? pv * qv : 0.f;
                        }
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            const float rz = zb[(32 * mt + r) * AFM_TS + jl];
                            const float u = rz > 0.f ? dav * w2s[32 * mt + r] : 0.f;
                            gb1[mt] = gb1[mt] + u;
                            gw2[mt] = fmaf(dav, rz, gw2[mt]);
#pragma unroll
                            for (int dt = 0; dt < DT; ++dt) acc3[mt][dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(u, hv[dt], acc3[mt][dt], 0, 0, 0);
                        }
                    }
                    __syncthreads();                           // zb, dab and cbuf are read
                }
                if (live && lane < D) ((NRX_GLOBAL float*)a.g_x)[b * a.gx_ld + ka->off[i] + lane] = gacc;
            }
        }
        if (slice < slices) {
            float* part = a.part + slice * n_el;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int t = 32 * mt + afm_row(q, kk), d = 32 * dt + r;
                        if (t < A && d < D) ((NRX_GLOBAL float*)part)[t * D + d] = acc3[mt][dt][q];
                    }
                const float sb = gb1[mt] + __shfl_xor(gb1[mt], 32), sw = gw2[mt] + __shfl_xor(gw2[mt], 32);
                const int t = 32 * mt + r;
                if (kk == 0 && t < A) {
                    ((NRX_GLOBAL float*)part)[A * D + t] = sb;
                    ((NRX_GLOBAL float*)part)[A * D + A + t] = sw;
                }
            }
        }
    }
}

// the partials added in slice order; element e of a partial: g_W1 [A dim], then g_b1 [A], then g_w2 [A]
__global__ __launch_bounds__(256) void afm_reduce_kernel(const float* part, float* g_W1, float* g_b1, float* g_w2, int nw, int A, int64_t slices) {
    const int n = nw + 2 * A;
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
    if (e < nw) ((NRX_GLOBAL float*)g_W1)[e] = s;
    else if (e < nw + A) ((NRX_GLOBAL float*)g_b1)[e - nw] = s;
    else ((NRX_GLOBAL float*)g_w2)[e - nw - A] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------- host side
bool afm_shape_ok(int32_t F, int32_t dim, int32_t A) {
    return F >= 2 && F <= AFM_MAX && dim >= 4 && dim <= AFM_MAX && (dim & 3) == 0 && A >= 1 && A <= AFM_MAX;
}

bool afm_f32_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

struct AfmCall {
    const float* x; int64_t ld; const int32_t* off; int32_t F, dim; const float* W1; const float* b1; const float* w2; int32_t A; int64_t batch;
    const float* out; int64_t out_ld; const float* lse;
};

// the argument checks both entry points share (NRX_OK or NRX_ERR_BAD_ARG)
int afm_check(const char* who, const AfmCall& c) {
    NRX_REQUIRE(c.F >= 1 && c.dim >= 1 && c.A >= 1 && c.batch >= 0, "%s: bad argument (n_fields %d, dim %d, A %d, batch %lld)", who, c.F, c.dim, c.A,
                (long long)c.batch);
    NRX_REQUIRE(c.off != nullptr, "%s: null field_off", who);
    NRX_REQUIRE(c.ld >= c.dim && (c.ld & 3) == 0, "%s: bad argument (ld %lld: the row stride must hold a field of dim %d and be a multiple of 4)", who,
                (long long)c.ld, c.dim);
    NRX_REQUIRE(c.out_ld >= c.dim, "%s: bad argument (out_ld %lld below dim %d)", who, (long long)c.out_ld, c.dim);
    for (int32_t i = 0; i < c.F; ++i) {
        const int64_t o = c.off[i];
        NRX_REQUIRE(o >= 0 && o + c.dim <= c.ld, "%s: bad argument (field_off[%d] = %lld: the field leaves the row of ld %lld)", who, i, (long long)o,
                    (long long)c.ld);
        NRX_REQUIRE((o & 3) == 0, "%s: misaligned field (field_off[%d] = %lld must be a multiple of 4)", who, i, (long long)o);
    }
    if (c.F <= 4096)
        for (int32_t i = 1; i < c.F; ++i)
            for (int32_t k = 0; k < i; ++k) {
                const int64_t d = (int64_t)c.off[i] - c.off[k];
                NRX_REQUIRE(d >= c.dim || -d >= c.dim, "%s: bad argument (field_off[%d] = %d and field_off[%d] = %d overlap at dim %d)", who, k, c.off[k], i,
                            c.off[i], c.dim);
            }
    if (c.batch > 0) {
        NRX_REQUIRE(c.x != nullptr, "%s: null buffer (x)", who);
        NRX_REQUIRE(c.W1 != nullptr, "%s: null buffer (W1)", who);
        NRX_REQUIRE(c.b1 != nullptr, "%s: null buffer (b1)", who);
        NRX_REQUIRE(c.w2 != nullptr, "%s: null buffer (w2)", who);
        NRX_REQUIRE(c.out != nullptr, "%s: null buffer (out)", who);
        NRX_REQUIRE(c.lse != nullptr, "%s: null buffer (lse)", who);
        NRX_REQUIRE(nrx_aligned16(c.x), "%s: misaligned x (every field row must be 16-byte aligned)", who);
        NRX_REQUIRE(afm_f32_ok(c.W1), "%s: misaligned W1", who);
        NRX_REQUIRE(afm_f32_ok(c.b1), "%s: misaligned b1", who);
        NRX_REQUIRE(afm_f32_ok(c.w2), "%s: misaligned w2", who);
        NRX_REQUIRE(afm_f32_ok(c.out), "%s: misaligned out", who);
        NRX_REQUIRE(afm_f32_ok(c.lse), "%s: misaligned lse", who);
    }
    return NRX_OK;
}

int afm_unsupported(const char* who, const AfmCall& c) {
    if (afm_shape_ok(c.F, c.dim, c.A)) return NRX_OK;
    nrx_set_error("%s: supports n_fields 2..%d, dim %% 4 == 0 in 4..%d, A 1..%d (got n_fields=%d, dim=%d, A=%d)", who, AFM_MAX, AFM_MAX, AFM_MAX, c.F,
                  c.dim, c.A);
    return NRX_ERR_UNSUPPORTED;
}

AfmArgs afm_args(const AfmCall& c) {
    AfmArgs a = {};
    a.x = c.x; a.W1 = c.W1; a.b1 = c.b1; a.w2 = c.w2; a.out = const_cast<float*>(c.out); a.lse = const_cast<float*>(c.lse);
    a.ld = c.ld; a.out_ld = c.out_ld; a.batch = c.batch; a.F = c.F; a.dim = c.dim; a.A = c.A; a.P = c.F * (c.F - 1) / 2;
    for (int i = 0; i < c.F; ++i) a.off[i] = c.off[i];
    return a;
}

size_t afm_fwd_lds(int F, int dim, int A) {
    const int MT = A > 32 ? 2 : 1, DS = dim | 1, nt = (F * (F - 1) / 2 + 31) / 32;
    return (size_t)(32 * MT * DS + 128 + 32 * nt + AFM_WAVES * (F * DS + 32 * nt + 64)) * 4;
}
size_t afm_bwd_lds(int F, int dim, int A) {
    const int MT = A > 32 ? 2 : 1, DT = dim > 32 ? 2 : 1, DS = dim | 1;
    return (size_t)(32 * MT * (32 * DT + 1) + 128 + AFM_WAVES * (F * DS + 128 + 32 * MT * AFM_TS + 32 + 32 * DT * AFM_TS)) * 4;
}

bool afm_lds_ready() {
    static const bool ok = [] {
        const void* ks[] = {reinterpret_cast<const void*>(&afm_fwd_kernel<1>),    reinterpret_cast<const void*>(&afm_fwd_kernel<2>),
                            reinterpret_cast<const void*>(&afm_bwd_kernel<1, 1>), reinterpret_cast<const void*>(&afm_bwd_kernel<1, 2>),
                            reinterpret_cast<const void*>(&afm_bwd_kernel<2, 1>), reinterpret_cast<const void*>(&afm_bwd_kernel<2, 2>)};
        for (const void* k : ks)
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, AFM_LDS) != hipSuccess) return false;
        return true;
    }();
    return ok;
}

int64_t afm_slices(int64_t batch) { return batch > 0 ? (batch + AFM_SLICE - 1) / AFM_SLICE : 1; }

}  // namespace

extern "C" int nrx_afm_supported(int32_t n_fields, int32_t dim, int32_t A) { return afm_shape_ok(n_fields, dim, A) ? 1 : 0; }

extern "C" int64_t nrx_afm_wgrad_slice(int32_t n_fields, int32_t dim, int32_t A) { return n_fields >= 1 && dim >= 1 && A >= 1 ? AFM_SLICE : 0; }

extern "C" int64_t nrx_afm_bwd_workspace(int64_t batch, int32_t n_fields, int32_t dim, int32_t A) {
    if (batch < 0 || n_fields < 1 || dim < 1 || A < 1) return 0;
    return afm_slices(batch) * ((int64_t)A * dim + 2 * A) * 4;
}

extern "C" int nrx_afm_fwd(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t dim, const float* W1, const float* b1,
                           const float* w2, int32_t A, int64_t batch, float* out, int64_t out_ld, float* lse, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_afm_fwd";
    const AfmCall c = {x, ld, field_off, n_fields, dim, W1, b1, w2, A, batch, out, out_ld, lse};
    int rc = afm_check(who, c);
    if (rc == NRX_OK) rc = afm_unsupported(who, c);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    if (!afm_lds_ready()) {
        nrx_set_error("%s: the kernels' LDS size could not be set", who);
        return NRX_ERR_LAUNCH;
    }
    const AfmArgs a = afm_args(c);
    const int64_t want = (batch + AFM_WAVES - 1) / AFM_WAVES;
    const dim3 grid((unsigned)(want < AFM_MAX_BLOCKS ? want : AFM_MAX_BLOCKS)), block(AFM_WAVES * 64);
    const size_t lds = afm_fwd_lds(n_fields, dim, A);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (A > 32) hipLaunchKernelGGL((afm_fwd_kernel<2>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((afm_fwd_kernel<1>), grid, block, lds, st, a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

extern "C" int nrx_afm_bwd(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t dim, const float* W1, const float* b1,
                           const float* w2, int32_t A, int64_t batch, const float* out, int64_t out_ld, const float* lse, const float* g_out,
                           int64_t g_out_ld, float* g_x, int64_t gx_ld, float* g_W1, float* g_b1, float* g_w2, void* workspace, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_afm_bwd";
    const AfmCall c = {x, ld, field_off, n_fields, dim, W1, b1, w2, A, batch, out, out_ld, lse};
    int rc = afm_check(who, c);
    if (rc != NRX_OK) return rc;
    NRX_REQUIRE(g_out_ld >= dim, "%s: bad argument (g_out_ld %lld below dim %d)", who, (long long)g_out_ld, dim);
    for (int32_t i = 0; i < n_fields; ++i)
        NRX_REQUIRE(field_off[i] + (int64_t)dim <= gx_ld, "%s: bad argument (gx_ld %lld does not hold field %d: field_off %d + dim %d)", who,
                    (long long)gx_ld, i, field_off[i], dim);
    if (batch > 0) {
        NRX_REQUIRE(g_out != nullptr, "%s: null buffer (g_out)", who);
        NRX_REQUIRE(g_x != nullptr, "%s: null buffer (g_x)", who);
        NRX_REQUIRE(g_W1 != nullptr, "%s: null buffer (g_W1)", who);
        NRX_REQUIRE(g_b1 != nullptr, "%s: null buffer (g_b1)", who);
        NRX_REQUIRE(g_w2 != nullptr, "%s: null buffer (g_w2)", who);
        NRX_REQUIRE(workspace != nullptr, "%s: null buffer (workspace)", who);
        NRX_REQUIRE(afm_f32_ok(g_out), "%s: misaligned g_out", who);
        NRX_REQUIRE(afm_f32_ok(g_x), "%s: misaligned g_x", who);
        NRX_REQUIRE(afm_f32_ok(g_W1), "%s: misaligned g_W1", who);
        NRX_REQUIRE(afm_f32_ok(g_b1), "%s: misaligned g_b1", who);
        NRX_REQUIRE(afm_f32_ok(g_w2), "%s: misaligned g_w2", who);
        NRX_REQUIRE(afm_f32_ok(workspace), "%s: misaligned workspace", who);
    }
    rc = afm_unsupported(who, c);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    if (!afm_lds_ready()) {
        nrx_set_error("%s: the kernels' LDS size could not be set", who);
        return NRX_ERR_LAUNCH;
    }
    AfmArgs a = afm_args(c);
    a.g_out = g_out; a.go_ld = g_out_ld; a.g_x = g_x; a.gx_ld = gx_ld; a.part = reinterpret_cast<float*>(workspace);
    const int64_t slices = afm_slices(batch), want = (slices + AFM_WAVES - 1) / AFM_WAVES;
    const dim3 grid((unsigned)(want < AFM_MAX_BLOCKS ? want : AFM_MAX_BLOCKS)), block(AFM_WAVES * 64);
    const size_t lds = afm_bwd_lds(n_fields, dim, A);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool m2 = A > 32, d2 = dim > 32;
    if (m2 && d2) hipLaunchKernelGGL((afm_bwd_kernel<2, 2>), grid, block, lds, st, a);
    else if (m2) hipLaunchKernelGGL((afm_bwd_kernel<2, 1>), grid, block, lds, st, a);
    else if (d2) hipLaunchKernelGGL((afm_bwd_kernel<1, 2>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((afm_bwd_kernel<1, 1>), grid, block, lds, st, a);
    NRX_LAUNCH_CHECK(who);
    const int nw = A * dim, n = nw + 2 * A;
    hipLaunchKernelGGL(afm_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, g_W1, g_b1, g_w2, nw, A, slices);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}
