// Compressed Interaction Network (the explicit, vector-wise interaction of xDeepFM; Lian et al., KDD 2018, eq. 6-8): one layer per call, forward
// and backward on the matrix cores with nothing of size batch * Hp * m * dim in between.  No reference counterpart; DESIGN 7j.
//
// Definition (include/nrx_embed.h restates it): X0[b, j, :] = x0[b * x0_ld + field_off[j] .. + dim), Xp = X^{k-1} (layer 1: Xp = X0, Hp = m).
//   forward : xk[b, h, d] = sum_{i, j} W[h, i, j] Xp[b, i, d] X0[b, j, d],  p[b, h] = sum_d xk[b, h, d]
//   backward: G[b, h, d] = g_p[b, h] + g_xk[b, h, d];  g_xprev[b, i, d] = sum_{h, j} G W X0,  g_x0[b, j, d] (+)= sum_{h, i} G W Xp,
//             g_W[h, i, j] = sum_{b, d} G Xp X0
//
// ONE KERNEL FOR THE THREE PER-SAMPLE PRODUCTS.  All three are the same GEMM: out[(b, d), n] = sum over k = u V + v of
// fl(P[b, u, d] Q[b, v, d]) Wn[n; u, v], M = batch * dim rows, K = U V, N <= 64 columns -- with
//   forward : P = Xp (U = Hp), Q = X0 (V = m), n = h, Wn[n; u, v] = W[n, u, v]
//   g_x0    : P = G  (U = H),  Q = Xp (V = Hp), n = j, Wn[n; u, v] = W[u, v, n]
//   g_xprev : P = G  (U = H),  Q = X0 (V = m),  n = i, Wn[n; u, v] = W[u, n, v]
// (cin_pair_kernel: the operand sources and the strides of W travel in the arguments).  v_mfma_f32_32x32x2_f32 is bit for bit
// fma(a_k1, b_k1, fma(a_k0, b_k0, c)); its A operand is lane l <- A[l & 31][l >> 5], its B operand lane l <- B[l >> 5][l & 31], its C layout
// column l & 31, row (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.
//   rows    : a wave owns one tile of 32 (b, d) rows at a time.  dim <= 32: the tile holds S = 32 / dim whole samples (row s dim + d; rows from
//             S dim on idle), tile t the samples t S ...  dim > 32: S = 1 and the wave runs the sample's two tiles (d = 32 mt + row) one after
//             the other.  A sample never leaves its wave: p and every store have one owner.
//   A       : the wave stages its rows' P and Q vectors in LDS as [u][row] (conflict-free), and lane (row, kk) multiplies out one element per
//             instruction: a = P[u][row] * Q[v][row] for k = 2 t + kk -- one rounded v_mul, two 4-byte LDS reads, behind the 64-cycle instruction.
//   B       : Wn^T [k][n] in LDS, staged by the whole workgroup in K slabs of `ks` rows (all of K when it fits: then staged once per workgroup,
//             which walks tiles in a bounded grid).  The rows lie 32 NT + 1 floats apart: the staging stores (threads along k or along n,
//             whichever is contiguous in W) and the operand reads (lanes along n) are both conflict-free.  Rows k >= K and columns n >= N hold 0.
//             A lane walks its (u, v) by adding to two LDS offsets (no division in the loop) and reads the operands of 8 steps at a time.
//             The accumulators live across the slabs: a split K is still ONE chain over k ascending.
//   C       : n on the lane, rows in registers: registers 4 q .. 4 q + 3 are four consecutive d of one sample (dim % 4 == 0): one 16-byte store
//             (or load-add-store) per lane and q, no transpose.  p: the tile goes to the wave's LDS region as [row][n] and lane (s, n) sums its
//             sample's rows in ascending d (dim > 32: the sum carries over the two tiles in a register).
// g_W (cin_wgrad_kernel): M = h, N = (i, j), the reduction runs over (b, d).  A workgroup owns one SLICE of CIN_WG_CHUNKS * (64 / dim) samples
// and 8 column tiles; it stages chunks of 64 / dim samples (G, Xp, X0 as [row][.], odd strides) in LDS, 8 loads in flight per lane,
// lane (h, kk) feeds G, lane (k, kk) fl(Xp X0).  Partials [slice][H][K] go to the workspace; cin_wgrad_reduce_kernel adds them in slice order (one thread per element): no atomics.
// Loads are never behind a branch (a dead lane reads a valid address and selects 0).
#include "nrx_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int CIN_MAX = 64;                    // m, Hp, H
constexpr int CIN_MAX_DIM = 64;
constexpr int CIN_WAVES = 8;                   // pair kernel: waves (tiles in flight) per workgroup
constexpr int CIN_LDS = 160 * 1024;
constexpr int CIN_CUS = 256;                   // the bounded grid: CIN_CUS * (workgroups that fit one CU's LDS, at most 4)
constexpr int CIN_WG_WAVES = 4;                // wgrad kernel
constexpr int CIN_WG_NT = 2;                   // column tiles per wave
constexpr int CIN_WG_ROWS = 64;                // (b, d) rows per staged chunk, at most
constexpr int CIN_WG_CHUNKS = 32;              // chunks per slice

// one operand of the pair product: value(b, u, d) = mat[b * ld + col(u) + d] (+ vec[b * vld + u]); col(u) = off[u] (fields) or u * dim
struct CinSrc {
    const float* mat;
    const float* vec;
    int64_t ld, vld;
    int32_t fields, pad_;
};

struct CinArgs {
    CinSrc P, Q;
    const float* W;
    float* out;              // [batch, out_ld], column base of n: off[n] (out_fields) or n * dim; may be null
    float* p;                // [batch, p_ld] or null
    int64_t out_ld, p_ld, batch;
    int32_t sn, su, sv;      // W strides of n, u, v
    int32_t U, V, N, dim;
    int32_t out_fields, accumulate;
    int32_t ks, kfast;       // slab rows (even); staging threads run along k (else along n)
    int32_t region;          // floats of a wave's LDS region
    uint32_t magic;          // ceil(2^18 / V): k / V = (k * magic) >> 18 for k <= 4097
    int32_t off[CIN_MAX];
};

struct CinWgArgs {
    CinSrc G, Xp, X0;
    float* part;             // [slices][H][K]
    int64_t batch;
    int32_t H, Hp, m, dim;
    int32_t cs, sl;          // samples per chunk, per slice
    uint32_t magic;          // ceil(2^18 / m)
    int32_t off[CIN_MAX];
};

__device__ __forceinline__ int cin_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <typename A>
__device__ __forceinline__ float cin_load(const NRX_CONST A* ka, const CinSrc& s, int64_t b, int u, int d, int D) {
    const int col = (s.fields != 0 ? ka->off[u] : u * D) + d;
    float v = 0.f;
    if (s.mat != nullptr) v = ((const NRX_GLOBAL float*)s.mat)[b * s.ld + col];                                   // (wave-uniform branches)
    if (s.vec != nullptr) {
        const float w = ((const NRX_GLOBAL float*)s.vec)[b * s.vld + u];
        v = s.mat != nullptr ? w + v : w;
    }
    return v;
}

// Stage value(b, u, d) for u = first, first + step, .. < count into LDS at put(u), NB loads in flight at a time (a load past the end reads
// element `first` again and is dropped; u >= nvalid stores 0).  None of the loads is behind a branch.
constexpr int CIN_NB = 8;
template <typename A, typename F>
__device__ __forceinline__ void cin_stage(const NRX_CONST A* ka, const CinSrc& s, int64_t b, int d, int D, bool ok, int first, int step, int count,
                                          int nvalid, F&& put) {
    for (int u0 = first; u0 < count; u0 += CIN_NB * step) {
        float v[CIN_NB];
#pragma unroll
        for (int j = 0; j < CIN_NB; ++j) {
            const int u = u0 + j * step;
            v[j] = cin_load(ka, s, b, u < nvalid ? u : 0, d, D);
        }
#pragma unroll
        for (int j = 0; j < CIN_NB; ++j) {
            const int u = u0 + j * step;
            if (u < count) put(u, ok && u < nvalid ? v[j] : 0.f);
        }
    }
}

// A lane's place in the K loop: the LDS offsets of its P and Q rows for step k, advanced by 2 per step without a division
struct CinWalk {
    int pa, qa, k;
};

// G steps of the pair product's K loop, k ascending: the operands of all G steps are read from LDS before the first is consumed.  wsl: the
// lane's element of W^T's row kk; the rows lie 32 NT + 1 floats apart (staging stores along k and operand reads along n both conflict-free)
constexpr int CIN_G = 8;
template <int NT, int G>
__device__ __forceinline__ void cin_steps(f32x16 (&acc)[NT], const float* reg, const float* wsl, int t, CinWalk& w, int K, int dpa, int dqa, int qend,
                                          int V32) {
    constexpr int WS = 32 * NT + 1;
    const float* wb = wsl + 2 * t * WS;
    float pv[G], qv[G], bv[G][NT];
    bool live[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        pv[g] = reg[w.pa];                                     // (k = K, the pad of an odd K: row U = Q's row 0, unused)
        qv[g] = reg[w.qa];
        live[g] = w.k < K;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[g][nt] = wb[2 * g * WS + 32 * nt];
        w.k += 2;
        w.pa += dpa;
        w.qa += dqa;
        if (w.qa >= qend) {
            w.qa -= V32;
            w.pa += 32;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float av = live[g] ? pv[g] * qv[g] : 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[g][nt], acc[nt], 0, 0, 0);
    }
}

template <int NT>
__global__ __launch_bounds__(CIN_WAVES * 64) void cin_pair_kernel(const CinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cin_smem[];
    constexpr int HT = 32 * NT;
    const NRX_CONST CinArgs* ka = nrx_kernarg<CinArgs>();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
    const int U = a.U, V = a.V, N = a.N, D = a.dim, K = U * V, Kpad = K + (K & 1), ks = a.ks;
    const int nslabs = (Kpad + ks - 1) / ks;
    constexpr int WS = HT + 1;
    float* ws = cin_smem;                                      // [ks][WS]
    float* reg = cin_smem + ks * WS + wave * a.region;         // the wave's: P [U][32], Q [V][32]; then the result tile [32][HT]
    const int S = D <= 32 ? 32 / D : 1, MTL = D > 32 ? 2 : 1;
    const int64_t NU = (a.batch + S - 1) / S;
    const int64_t wstride = (int64_t)gridDim.x * CIN_WAVES;
    const int64_t iters = (NU + wstride - 1) / wstride;        // the same for every wave of the grid: the barriers below are uniform
    const int s_r = D <= 32 ? r / D : 0, d_r = r - s_r * D;
    bool staged = false;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t unit = (it * gridDim.x + blockIdx.x) * CIN_WAVES + wave;
        float pcarry = 0.f;
        for (int mt = 0; mt < MTL; ++mt) {
            const int64_t b = unit * S + s_r;
            const int d = d_r + 32 * mt;
            const bool rowok = unit < NU && s_r < S && b < a.batch && d < D;
            const int64_t bb = rowok ? b : 0;
            const int dd = rowok ? d : 0;
            f32x16 acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x16{};
            for (int slab = 0; slab < nslabs; ++slab) {
                const int k0 = slab * ks;
                const int ksl = Kpad - k0 < ks ? Kpad - k0 : ks;
                __syncthreads();                               // the slab before this one, and the wave's region, are read
                if (nslabs > 1 || !staged) {
                    staged = true;
                    // kfast: n = wave, wave + 8, ..; k = lane, lane + 64, ..   else: k = wave, ..; n = lane, ..  (lanes along what is contiguous in W)
                    const int n0 = a.kfast != 0 ? wave : lane, dn = a.kfast != 0 ? CIN_WAVES : 64;
                    const int q0 = a.kfast != 0 ? lane : wave, dq = a.kfast != 0 ? 64 : CIN_WAVES;
                    for (int n = n0; n < HT; n += dn)
                        for (int q = q0; q < ksl; q += 4 * dq) {          // (4 loads in flight)
                            float w[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int kl = q + j * dq, k = k0 + kl;
                                const bool in = n < N && k < K;
                                const int iu = (int)(((uint32_t)k * a.magic) >> 18), iv = k - iu * V;
                                w[j] = ((const NRX_GLOBAL float*)a.W)[in ? n * a.sn + iu * a.su + iv * a.sv : 0];
                            }
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int kl = q + j * dq;
                                if (kl < ksl) ws[kl * WS + n] = n < N && k0 + kl < K ? w[j] : 0.f;
                            }
                        }
                }
                if (slab == 0) {
                    cin_stage(ka, a.P, bb, dd, D, rowok, kk, 2, U, U, [&](int u, float v) { reg[u * 32 + r] = v; });
                    cin_stage(ka, a.Q, bb, dd, D, rowok, kk, 2, V, V, [&](int u, float v) { reg[(U + u) * 32 + r] = v; });
                }
                __syncthreads();
                const int nsteps = ksl >> 1;
                CinWalk w;
                w.k = k0 + kk;
                {
                    const int iu = (int)(((uint32_t)w.k * a.magic) >> 18), iv = w.k - iu * V;
                    w.pa = iu * 32 + r;
                    w.qa = (U + iv) * 32 + r;
                }
                const int dpa = (2 / V) * 32, dqa = (2 % V) * 32, qend = (U + V) * 32 + r;
                const float* wsl = ws + kk * WS + r;
                int t = 0;
                for (; t + CIN_G <= nsteps; t += CIN_G) cin_steps<NT, CIN_G>(acc, reg, wsl, t, w, K, dpa, dqa, qend, V * 32);
                for (; t < nsteps; ++t) cin_steps<NT, 1>(acc, reg, wsl, t, w, K, dpa, dqa, qend, V * 32);
            }
            // ---- the tile's stores, straight from the C layout: registers 4 q .. 4 q + 3 = rows 8 q + 4 kk .. + 3 = four d of one sample
            if (a.out != nullptr) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row0 = 8 * q + 4 * kk;
                    const int s = D <= 32 ? row0 / D : 0;
                    const int d0 = row0 - s * D + 32 * mt;
                    const int64_t bs = unit * S + s;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const int n = 32 * nt + r;
                        if (unit < NU && s < S && bs < a.batch && d0 < D && n < N) {
                            NRX_GLOBAL nrx_f32x4* o =
                                (NRX_GLOBAL nrx_f32x4*)(a.out + bs * a.out_ld + (a.out_fields != 0 ? ka->off[n] : n * D) + d0);
                            nrx_f32x4 v;
                            v.x = acc[nt][4 * q]; v.y = acc[nt][4 * q + 1]; v.z = acc[nt][4 * q + 2]; v.w = acc[nt][4 * q + 3];
                            if (a.accumulate != 0) {
                                const nrx_f32x4 old = *o;
                                v.x = old.x + v.x; v.y = old.y + v.y; v.z = old.z + v.z; v.w = old.w + v.w;
                            }
                            *o = v;
                        }
                    }
                }
            }
            // ---- p: the tile to the wave's region as [row][n]; lane (s, n) adds its sample's rows in ascending d
            if (a.p != nullptr) {                              // (uniform over the grid)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) reg[cin_row(rr, kk) * HT + 32 * nt + r] = acc[nt][rr];
                __syncthreads();
                const int rows = D <= 32 ? D : (D - 32 * mt < 32 ? D - 32 * mt : 32);
                for (int idx = lane; idx < S * HT; idx += 64) {
                    const int s = idx / HT, n = idx % HT;
                    float sum = mt == 0 ? 0.f : pcarry;        // (dim > 32: S * HT <= 64, one idx per lane carries over the two tiles)
                    for (int dl = 0; dl < rows; ++dl) sum += reg[(s * D + dl) * HT + n];
                    pcarry = sum;
                    const int64_t bs = unit * S + s;
                    if (mt == MTL - 1 && unit < NU && bs < a.batch && n < N) ((NRX_GLOBAL float*)a.p)[bs * a.p_ld + n] = sum;
                }
            }
        }
    }
}

// G steps of the weight gradient's reduction over a chunk's rows, ascending
template <int MT, int G>
__device__ __forceinline__ void cin_wg_steps(f32x16 (&acc)[MT][CIN_WG_NT], const float* gs, const float* xs, const float* x0s, int t, int kk, int r,
                                             int HS, int US, int VS, const int (&ci)[CIN_WG_NT], const int (&cj)[CIN_WG_NT],
                                             const bool (&cok)[CIN_WG_NT]) {
    float av[G][MT], pv[G][CIN_WG_NT], qv[G][CIN_WG_NT];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int row = 2 * (t + g) + kk;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[g][mt] = gs[row * HS + 32 * mt + r];
#pragma unroll
        for (int c = 0; c < CIN_WG_NT; ++c) {
            pv[g][c] = xs[row * US + ci[c]];
            qv[g][c] = x0s[row * VS + cj[c]];
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int c = 0; c < CIN_WG_NT; ++c) {
            const float bv = cok[c] ? pv[g][c] * qv[g][c] : 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g][mt], bv, acc[mt][c], 0, 0, 0);
        }
}

// g_W partials: grid (slices, column-tile groups); MT = row tiles of 32 h
template <int MT>
__global__ __launch_bounds__(CIN_WG_WAVES * 64) void cin_wgrad_kernel(const CinWgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cin_smem[];
    const NRX_CONST CinWgArgs* ka = nrx_kernarg<CinWgArgs>();
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, kk = lane >> 5;
    const int H = a.H, Hp = a.Hp, m = a.m, D = a.dim, K = Hp * m;
    const int HS = (32 * MT) | 1, US = Hp | 1, VS = m | 1;     // odd row strides: the staging stores (threads along rows) are conflict-free
    const int RC = a.cs * D;                                   // rows of a chunk (even: dim % 4 == 0)
    float* gs = cin_smem;                                      // [RC][HS]
    float* xs = gs + CIN_WG_ROWS * HS;                         // [RC][US]
    float* x0s = xs + CIN_WG_ROWS * US;                        // [RC][VS]
    const int64_t slice = blockIdx.x;
    const int tile0 = ((int)blockIdx.y * CIN_WG_WAVES + wave) * CIN_WG_NT;
    int ci[CIN_WG_NT], cj[CIN_WG_NT];
    bool cok[CIN_WG_NT];
#pragma unroll
    for (int t = 0; t < CIN_WG_NT; ++t) {
        const int k = 32 * (tile0 + t) + r;
        cok[t] = k < K;
        const int kc = cok[t] ? k : 0;
        ci[t] = (int)(((uint32_t)kc * a.magic) >> 18);
        cj[t] = kc - ci[t] * m;
    }
    // the staging lane's row: sample s_l of the chunk, column d_l
    const int s_l = lane / D, d_l = lane - s_l * D;
    f32x16 acc[MT][CIN_WG_NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < CIN_WG_NT; ++t) acc[mt][t] = f32x16{};
    for (int ch = 0; ch < CIN_WG_CHUNKS; ++ch) {
        const int64_t b0 = slice * a.sl + (int64_t)ch * a.cs;
        if (b0 >= a.batch) break;                              // (uniform)
        const int64_t b = b0 + s_l;
        const bool rowok = lane < RC && b < a.batch;
        const int64_t bb = rowok ? b : 0;
        __syncthreads();
        // (a lane past the chunk's rows writes zeros into rows the loop never reads)
        cin_stage(ka, a.G, bb, d_l, D, rowok, wave, CIN_WG_WAVES, 32 * MT, H, [&](int h, float v) { gs[lane * HS + h] = v; });
        cin_stage(ka, a.Xp, bb, d_l, D, rowok, wave, CIN_WG_WAVES, Hp, Hp, [&](int i, float v) { xs[lane * US + i] = v; });
        cin_stage(ka, a.X0, bb, d_l, D, rowok, wave, CIN_WG_WAVES, m, m, [&](int j, float v) { x0s[lane * VS + j] = v; });
        __syncthreads();
        const int nsteps = RC >> 1;
        int t = 0;
        for (; t + 4 <= nsteps; t += 4) cin_wg_steps<MT, 4>(acc, gs, xs, x0s, t, kk, r, HS, US, VS, ci, cj, cok);
        for (; t < nsteps; ++t) cin_wg_steps<MT, 1>(acc, gs, xs, x0s, t, kk, r, HS, US, VS, ci, cj, cok);
    }
    float* part = a.part + slice * (int64_t)H * K;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < CIN_WG_NT; ++t) {
            const int k = 32 * (tile0 + t) + r;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int h = 32 * mt + cin_row(rr, kk);
                if (h < H && k < K) ((NRX_GLOBAL float*)part)[(int64_t)h * K + k] = acc[mt][t][rr];
            }
        }
}

__global__ __launch_bounds__(256) void cin_wgrad_reduce_kernel(const float* part, float* g_W, int64_t n, int64_t slices) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
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
    ((NRX_GLOBAL float*)g_W)[e] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------- host side
int cin_chunk_samples(int dim) { return dim >= CIN_WG_ROWS ? 1 : CIN_WG_ROWS / dim; }
int cin_slice_samples(int dim) { return cin_chunk_samples(dim) * CIN_WG_CHUNKS; }
uint32_t cin_magic(int v) { return (uint32_t)(((1 << 18) + v - 1) / v); }

bool cin_shape_ok(int32_t m, int32_t Hp, int32_t H, int32_t dim) {
    return m >= 2 && m <= CIN_MAX && Hp >= 1 && Hp <= CIN_MAX && H >= 1 && H <= CIN_MAX && dim >= 4 && dim <= CIN_MAX_DIM && (dim & 3) == 0;
}

struct CinLayer {
    const float* x0; int64_t x0_ld; const int32_t* off; int32_t m, dim; const float* xprev; int64_t xprev_ld; int32_t Hp; const float* W; int32_t H;
    int64_t batch;
};

int cin_check(const char* who, const CinLayer& l) {
    NRX_REQUIRE(l.m >= 1 && l.Hp >= 1 && l.H >= 1 && l.dim >= 1 && l.batch >= 0, "%s: bad argument (m %d, Hp %d, H %d, dim %d, batch %lld)", who, l.m,
                l.Hp, l.H, l.dim, (long long)l.batch);
    NRX_REQUIRE(l.off != nullptr, "%s: null field_off", who);
    NRX_REQUIRE(l.x0_ld >= l.dim && (l.x0_ld & 3) == 0, "%s: bad argument (x0_ld %lld: the row stride must hold a field of dim %d and be a multiple of 4)",
                who, (long long)l.x0_ld, l.dim);
    for (int32_t i = 0; i < l.m; ++i) {
        const int64_t o = l.off[i];
        NRX_REQUIRE(o >= 0 && o + l.dim <= l.x0_ld, "%s: bad argument (field_off[%d] = %lld: the field leaves the row of x0_ld %lld)", who, i, (long long)o,
                    (long long)l.x0_ld);
        NRX_REQUIRE((o & 3) == 0, "%s: misaligned field (field_off[%d] = %lld must be a multiple of 4)", who, i, (long long)o);
    }
    if (l.m <= 4096)
        for (int32_t i = 1; i < l.m; ++i)
            for (int32_t k = 0; k < i; ++k) {
                const int64_t d = (int64_t)l.off[i] - l.off[k];
                NRX_REQUIRE(d >= l.dim || -d >= l.dim, "%s: bad argument (field_off[%d] = %d and field_off[%d] = %d overlap at dim %d)", who, k, l.off[k], i,
                            l.off[i], l.dim);
            }
    NRX_REQUIRE(l.xprev != nullptr || l.Hp == l.m, "%s: bad argument (xprev is null -- layer 1, X^{k-1} = X^0 -- but Hp %d != m %d)", who, l.Hp, l.m);
    NRX_REQUIRE(l.xprev == nullptr || (l.xprev_ld >= (int64_t)l.Hp * l.dim && (l.xprev_ld & 3) == 0),
                "%s: bad argument (xprev_ld %lld: the row stride must hold Hp * dim = %lld floats and be a multiple of 4)", who, (long long)l.xprev_ld,
                (long long)l.Hp * l.dim);
    if (l.batch > 0) {
        NRX_REQUIRE(l.x0 != nullptr && l.W != nullptr, "%s: null buffer (x0 or W)", who);
        NRX_REQUIRE(nrx_aligned16(l.x0), "%s: misaligned x0 (every field row must be 16-byte aligned)", who);
        NRX_REQUIRE(nrx_aligned16(l.xprev), "%s: misaligned xprev (16-byte aligned rows)", who);
        NRX_REQUIRE((reinterpret_cast<uintptr_t>(l.W) & 3u) == 0, "%s: misaligned W", who);
    }
    return NRX_OK;
}

// an output (or gradient input) matrix of `cols` columns: row stride, alignment
int cin_check_mat(const char* who, const char* name, const void* p, int64_t ld, int64_t cols, bool rows16, int64_t batch) {
    NRX_REQUIRE(ld >= cols && (!rows16 || (ld & 3) == 0), "%s: bad argument (%s row stride %lld: must hold %lld floats%s)", who, name, (long long)ld,
                (long long)cols, rows16 ? " and be a multiple of 4" : "");
    if (batch > 0) NRX_REQUIRE((reinterpret_cast<uintptr_t>(p) & (rows16 ? 15u : 3u)) == 0, "%s: misaligned %s", who, name);
    return NRX_OK;
}

int cin_unsupported(const char* who, const CinLayer& l) {
    if (cin_shape_ok(l.m, l.Hp, l.H, l.dim)) return NRX_OK;
    nrx_set_error("%s: supports m 2..%d, Hp and H 1..%d, dim %% 4 == 0 in 4..%d (got m=%d, Hp=%d, H=%d, dim=%d)", who, CIN_MAX, CIN_MAX, CIN_MAX_DIM,
                  l.m, l.Hp, l.H, l.dim);
    return NRX_ERR_UNSUPPORTED;
}

CinSrc cin_src(const float* mat, int64_t ld, bool fields, const float* vec = nullptr, int64_t vld = 0) {
    CinSrc s = {};
    s.mat = mat; s.ld = ld; s.fields = fields; s.vec = vec; s.vld = vld;
    return s;
}

bool cin_lds_ready() {
    static const bool ok = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&cin_pair_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, CIN_LDS) == hipSuccess &&
               hipFuncSetAttribute(reinterpret_cast<const void*>(&cin_pair_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, CIN_LDS) == hipSuccess &&
               hipFuncSetAttribute(reinterpret_cast<const void*>(&cin_wgrad_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, CIN_LDS) == hipSuccess &&
               hipFuncSetAttribute(reinterpret_cast<const void*>(&cin_wgrad_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, CIN_LDS) == hipSuccess;
    }();
    return ok;
}

// one pair product: fills the launch shape (slab rows, region, grid) and launches
void cin_pair_launch(CinArgs a, const int32_t* off, int32_t n_off, hipStream_t st) {
    for (int i = 0; i < n_off; ++i) a.off[i] = off[i];
    const int HT = a.N > 32 ? 64 : 32, K = a.U * a.V, Kpad = K + (K & 1);
    const int region = (a.U + a.V) * 32 > 32 * HT ? (a.U + a.V) * 32 : 32 * HT;
    int ks = ((CIN_LDS - CIN_WAVES * region * 4) / ((HT + 1) * 4)) & ~1;
    if (ks > Kpad) ks = Kpad;
    a.ks = ks; a.region = region; a.magic = cin_magic(a.V);
    const size_t lds = (size_t)(ks * (HT + 1) + CIN_WAVES * region) * 4;
    const int S = a.dim <= 32 ? 32 / a.dim : 1;
    const int64_t units = (a.batch + S - 1) / S, want = (units + CIN_WAVES - 1) / CIN_WAVES;
    int per_cu = (int)(CIN_LDS / lds);
    per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
    const int64_t cap = (int64_t)CIN_CUS * per_cu;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(CIN_WAVES * 64);
    if (HT == 64) hipLaunchKernelGGL((cin_pair_kernel<2>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((cin_pair_kernel<1>), grid, block, lds, st, a);
}

}  // namespace

extern "C" int nrx_cin_supported(int32_t m, int32_t Hp, int32_t H, int32_t dim) { return cin_shape_ok(m, Hp, H, dim) ? 1 : 0; }

extern "C" int64_t nrx_cin_wgrad_slice(int32_t dim) { return dim >= 1 ? cin_slice_samples(dim) : 0; }

extern "C" int64_t nrx_cin_layer_bwd_workspace(int64_t batch, int32_t m, int32_t Hp, int32_t H, int32_t dim) {
    if (batch < 0 || m < 1 || Hp < 1 || H < 1 || dim < 1) return 0;
    const int64_t sl = cin_slice_samples(dim), slices = batch > 0 ? (batch + sl - 1) / sl : 1;
    return slices * H * Hp * m * 4;
}

extern "C" int nrx_cin_layer_fwd(const float* x0, int64_t x0_ld, const int32_t* field_off, int32_t m, int32_t dim, const float* xprev, int64_t xprev_ld,
                                 int32_t Hp, const float* W, int32_t H, int64_t batch, float* xk, int64_t xk_ld, float* p, int64_t p_ld, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_cin_layer_fwd";
    const CinLayer l = {x0, x0_ld, field_off, m, dim, xprev, xprev_ld, Hp, W, H, batch};
    int rc = cin_check(who, l);
    if (rc != NRX_OK) return rc;
    if (xk != nullptr && (rc = cin_check_mat(who, "xk", xk, xk_ld, (int64_t)H * dim, true, batch)) != NRX_OK) return rc;
    if (batch > 0) NRX_REQUIRE(p != nullptr, "%s: null buffer (p)", who);
    if ((rc = cin_check_mat(who, "p", p, p_ld, H, false, batch)) != NRX_OK) return rc;
    if ((rc = cin_unsupported(who, l)) != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    if (!cin_lds_ready()) {
        nrx_set_error("%s: the kernels' LDS size could not be set", who);
        return NRX_ERR_LAUNCH;
    }
    CinArgs a = {};
    a.P = xprev != nullptr ? cin_src(xprev, xprev_ld, false) : cin_src(x0, x0_ld, true);
    a.Q = cin_src(x0, x0_ld, true);
    a.W = W; a.sn = Hp * m; a.su = m; a.sv = 1; a.kfast = 1;
    a.U = Hp; a.V = m; a.N = H; a.dim = dim; a.batch = batch;
    a.out = xk; a.out_ld = xk_ld; a.out_fields = 0; a.accumulate = 0;
    a.p = p; a.p_ld = p_ld;
    cin_pair_launch(a, field_off, m, reinterpret_cast<hipStream_t>(stream));
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

extern "C" int nrx_cin_layer_bwd(const float* x0, int64_t x0_ld, const int32_t* field_off, int32_t m, int32_t dim, const float* xprev, int64_t xprev_ld,
                                 int32_t Hp, const float* W, int32_t H, int64_t batch, const float* g_p, int64_t gp_ld, const float* g_xk, int64_t gxk_ld,
                                 float* g_xprev, int64_t gxprev_ld, float* g_x0, int64_t gx0_ld, int32_t accumulate_x0, float* g_W, void* workspace,
                                 void* stream) {
    NRX_TRACE();
    const char* who = "nrx_cin_layer_bwd";
    const CinLayer l = {x0, x0_ld, field_off, m, dim, xprev, xprev_ld, Hp, W, H, batch};
    int rc = cin_check(who, l);
    if (rc != NRX_OK) return rc;
    NRX_REQUIRE(accumulate_x0 == 0 || accumulate_x0 == 1, "%s: bad argument (accumulate_x0 %d: 0 or 1)", who, accumulate_x0);
    NRX_REQUIRE((xprev == nullptr) == (g_xprev == nullptr), "%s: bad argument (g_xprev must be null exactly when xprev is: layer 1 adds that term to g_x0)",
                who);
    if (batch > 0) NRX_REQUIRE(g_p != nullptr && g_x0 != nullptr && g_W != nullptr && workspace != nullptr, "%s: null buffer (g_p, g_x0, g_W or workspace)", who);
    if ((rc = cin_check_mat(who, "g_p", g_p, gp_ld, H, false, batch)) != NRX_OK) return rc;
    if (g_xk != nullptr && (rc = cin_check_mat(who, "g_xk", g_xk, gxk_ld, (int64_t)H * dim, true, batch)) != NRX_OK) return rc;
    if (g_xprev != nullptr && (rc = cin_check_mat(who, "g_xprev", g_xprev, gxprev_ld, (int64_t)Hp * dim, true, batch)) != NRX_OK) return rc;
    if ((rc = cin_check_mat(who, "g_x0", g_x0, gx0_ld, dim, true, batch)) != NRX_OK) return rc;
    for (int32_t i = 0; i < m; ++i)
        NRX_REQUIRE(field_off[i] + (int64_t)dim <= gx0_ld, "%s: bad argument (gx0_ld %lld does not hold field %d: field_off %d + dim %d)", who,
                    (long long)gx0_ld, i, field_off[i], dim);
    if (batch > 0) NRX_REQUIRE((reinterpret_cast<uintptr_t>(g_W) & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "%s: misaligned g_W or workspace", who);
    if ((rc = cin_unsupported(who, l)) != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    if (!cin_lds_ready()) {
        nrx_set_error("%s: the kernels' LDS size could not be set", who);
        return NRX_ERR_LAUNCH;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const CinSrc G = cin_src(g_xk, gxk_ld, false, g_p, gp_ld);
    const CinSrc Xp = xprev != nullptr ? cin_src(xprev, xprev_ld, false) : cin_src(x0, x0_ld, true);
    const CinSrc X0 = cin_src(x0, x0_ld, true);
    {   // g_x0[b, j, d] (+)= chain over k = h Hp + i of fl(G Xp) W[h, i, j]
        CinArgs a = {};
        a.P = G; a.Q = Xp; a.W = W; a.sn = 1; a.su = Hp * m; a.sv = m; a.kfast = 0;
        a.U = H; a.V = Hp; a.N = m; a.dim = dim; a.batch = batch;
        a.out = g_x0; a.out_ld = gx0_ld; a.out_fields = 1; a.accumulate = accumulate_x0;
        cin_pair_launch(a, field_off, m, st);
        NRX_LAUNCH_CHECK(who);
    }
    {   // g_xprev[b, i, d] = chain over k = h m + j of fl(G X0) W[h, i, j]; layer 1: added onto g_x0's field i
        CinArgs a = {};
        a.P = G; a.Q = X0; a.W = W; a.sn = m; a.su = Hp * m; a.sv = 1; a.kfast = 1;
        a.U = H; a.V = m; a.N = Hp; a.dim = dim; a.batch = batch;
        if (g_xprev != nullptr) {
            a.out = g_xprev; a.out_ld = gxprev_ld; a.out_fields = 0; a.accumulate = 0;
        } else {
            a.out = g_x0; a.out_ld = gx0_ld; a.out_fields = 1; a.accumulate = 1;
        }
        cin_pair_launch(a, field_off, m, st);
        NRX_LAUNCH_CHECK(who);
    }
    {   // g_W: per-slice partials, then their sum in slice order
        CinWgArgs a = {};
        a.G = G; a.Xp = Xp; a.X0 = X0; a.part = reinterpret_cast<float*>(workspace); a.batch = batch;
        a.H = H; a.Hp = Hp; a.m = m; a.dim = dim; a.cs = cin_chunk_samples(dim); a.sl = cin_slice_samples(dim); a.magic = cin_magic(m);
        for (int i = 0; i < m; ++i) a.off[i] = field_off[i];
        const int64_t slices = (batch + a.sl - 1) / a.sl;
        const int K = Hp * m, tiles = (K + 31) / 32, per_wg = CIN_WG_WAVES * CIN_WG_NT;
        const int MT = H > 32 ? 2 : 1;
        const size_t lds = (size_t)CIN_WG_ROWS * (((32 * MT) | 1) + (Hp | 1) + (m | 1)) * 4;
        const dim3 grid((unsigned)slices, (unsigned)((tiles + per_wg - 1) / per_wg)), block(CIN_WG_WAVES * 64);
        if (MT == 2) hipLaunchKernelGGL((cin_wgrad_kernel<2>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((cin_wgrad_kernel<1>), grid, block, lds, st, a);
        NRX_LAUNCH_CHECK(who);
        const int64_t n = (int64_t)H * K;
        hipLaunchKernelGGL(cin_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, g_W, n, slices);
        NRX_LAUNCH_CHECK(who);
    }
    return NRX_OK;
}
