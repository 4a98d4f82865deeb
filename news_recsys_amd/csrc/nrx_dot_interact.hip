// Pairwise dot-product interaction (the product layer of the inner-product PNN, the interaction op of DLRM): every pair of a sample's field
// embeddings multiplied out to its own feature, forward and backward on the matrix cores with nothing of size batch * F * F in between.
// No reference counterpart (the reference has neither PNN nor DLRM); DESIGN 7i.
//
// Definition (include/nrx_embed.h restates it): e_f = x[b * ld + field_off[f] .. + dim).
//   forward : z[b, i (i - 1) / 2 + j] = dot(e_i, e_j) for j < i  (NRX_DOT_SELF: j <= i, index i (i + 1) / 2 + j), with
//             dot = one fp32 fma chain from 0 over k in the order 0, D/2, 1, D/2 + 1, ..., D/2 - 1, D - 1
//   backward: g_e_f[c] = one fp32 fma chain from 0 over j = 0 .. F - 1 ascending of S[f][j] e_j[c], S = G + G^T, G the (strict) lower
//             triangle of g_z (NRX_DOT_SELF: S[f][f] = 2 g_z[f, f]); an odd F appends one term 0 * 0 (the matrix instruction takes k in pairs)
//
// Mapping: ONE WAVE OWNS ONE SAMPLE at a time (4 waves per workgroup, samples strided over a bounded grid).  v_mfma_f32_32x32x2_f32 is bit
// for bit fma(a_k1, b_k1, fma(a_k0, b_k0, c)) (profiles/r01_mfma_f32_semantics.txt), its A operand is lane l <- A[l & 31][l >> 5] and its B
// operand lane l <- B[l >> 5][l & 31].
//   forward : Z = E E^T, so A and B are THE SAME REGISTER: lane (f = l & 31, h = l >> 5) loads the half row e_f[h D/2 .. (h + 1) D/2) with
//             16-byte (dim % 8 == 0) or 8-byte loads, and step s feeds element s of it: D/2 matrix instructions per 32 x 32 tile, one tile
//             for F <= 32, the three tiles of the lower triangle for F <= 64.  Lanes f >= F load field 0 and take zeros (no load behind a
//             branch); the next sample's rows are requested before the current one is consumed.  The triangle is stored straight from the
//             C layout (column j on the lane, row i = (r & 3) + 8 (r >> 2) + 4 h in register r): row i of the triangle is one contiguous
//             run of i floats, a half wave stores it as one run.
//   backward: g_E = S E: S is the A operand (lane (f, h) gathers S[f][2 t + h] from the sample's g_z row, an L1-resident 4 P bytes), E the B
//             operand (lane (c, h) reads e_{2 t + h}[c]: a half wave reads one field row as a run); ceil(F / 2) steps per (32 fields, 32
//             columns) tile pair; the operands of step t + 1 are requested before step t is consumed.  The result's C layout has the column c
//             on the lane and the field in the register: a half wave stores (or adds onto) one field's gradient as a run.
// One owner per output element: no atomics, no workspace, no LDS.  A function of the one sample only: its bits depend neither on batch nor
// on its place in it.
// Reads: the fields of x, the first P columns of g_z, and (accumulate) the field columns of g_x.  Writes: the first P columns of a z row,
// the field columns of a g_x row -- nothing else (pad columns, off-field columns).  The field offsets travel by value in the kernel
// arguments and are read through the constant address space (never copied to scratch).
#include "nrx_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int DI_MAX_FIELDS = 64;
constexpr int DI_MAX_DIM = 64;
constexpr int DI_WAVES = 4;                    // waves (samples in flight) per workgroup
constexpr int DI_MAX_BLOCKS = 2048;            // 8 workgroups per compute unit; more samples than that are strided

struct DotArgs {
    const float* x;          // [batch, ld]
    float* z;                // forward: [batch, z_ld]
    const float* g_z;        // backward: [batch, gz_ld]
    float* g_x;              // backward: [batch, gx_ld]
    int64_t ld, z_ld, gz_ld, gx_ld, batch;
    int32_t nf, dim, self, accumulate;
    int32_t off[DI_MAX_FIELDS];
};

// row of the C layout that register r of lane half h holds
__device__ __forceinline__ int di_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int VW>
struct DiVec {
    using type = __attribute__((ext_vector_type(VW))) float;
};

// the lane's half rows of one sample, as they lie in memory: NL loads per tile row, none behind a branch (a load past the half row reads
// its last piece again; a lane past the last field reads field 0 -- `col` says so)
template <int VW, int NL, int T>
__device__ __forceinline__ void di_load(const float* row, const int (&col)[T], int nl, typename DiVec<VW>::type (&raw)[T][NL]) {
    using V = typename DiVec<VW>::type;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < NL; ++i) raw[t][i] = *(const NRX_GLOBAL V*)(row + col[t] + VW * (i < nl ? i : nl - 1));
}

// the triangle's part of one 32 x 32 tile, straight from the C layout
__device__ __forceinline__ void di_store_tile(const f32x16& acc, float* zrow, int i0, int j0, int f, int h, int F, int self) {
    const int j = j0 + f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + di_row(r, h);
        const bool ok = i < F && (j < i || (self != 0 && j == i));
        const int at = (self != 0 ? i * (i + 1) / 2 : i * (i - 1) / 2) + j;
        if (ok) ((NRX_GLOBAL float*)zrow)[at] = acc[r];
    }
}

template <int VW, int NL, int T>
__global__ __launch_bounds__(DI_WAVES * 64) void dot_fwd_kernel(const DotArgs a) {
    using V = typename DiVec<VW>::type;
    const NRX_CONST DotArgs* ka = nrx_kernarg<DotArgs>();
    const int lane = threadIdx.x & 63;
    const int f = lane & 31, h = lane >> 5;
    const int F = a.nf, half = a.dim >> 1, nl = half / VW, self = a.self;
    const int64_t stride = (int64_t)gridDim.x * DI_WAVES;
    int64_t b = (int64_t)blockIdx.x * DI_WAVES + (threadIdx.x >> 6);
    if (b >= a.batch) return;                                  // (the whole wave)
    int col[T];
    bool live[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        live[t] = 32 * t + f < F;
        col[t] = ka->off[live[t] ? 32 * t + f : 0] + h * half;
    }
    V cur[T][NL];
    di_load<VW, NL, T>(a.x + b * a.ld, col, nl, cur);
    for (; b < a.batch; b += stride) {
        V nxt[T][NL];
        di_load<VW, NL, T>(a.x + (b + stride < a.batch ? b + stride : b) * a.ld, col, nl, nxt);     // (the last sample again: never used)
        f32x16 z00 = {}, z10 = {}, z11 = {};
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            if (i < nl) {                                      // (wave-uniform: a skipped step, never a padded one)
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    const float v0 = live[0] ? cur[0][i][e] : 0.f;
                    z00 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, v0, z00, 0, 0, 0);
                    if constexpr (T == 2) {
                        const float v1 = live[1] ? cur[1][i][e] : 0.f;
                        z10 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, v0, z10, 0, 0, 0);
                        z11 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, v1, z11, 0, 0, 0);
                    }
                }
            }
        }
        float* zrow = a.z + b * a.z_ld;
        di_store_tile(z00, zrow, 0, 0, f, h, F, self);
        if constexpr (T == 2) {
            di_store_tile(z10, zrow, 32, 0, f, h, F, self);
            di_store_tile(z11, zrow, 32, 32, f, h, F, self);
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < NL; ++i) cur[t][i] = nxt[t][i];
    }
}

// the operands of backward step t as they lie in memory: S[32 m + f][2 t + h] from the sample's g_z row and e_{2 t + h}[32 n + f]; a lane
// whose element does not exist reads element 0 of the row (valid memory) and di_bwd_mask makes it 0 when it is consumed
template <int MT, int NT>
struct DiOps {
    float s[MT], e[NT];
};
template <int MT, int NT>
__device__ __forceinline__ DiOps<MT, NT> di_bwd_load(const NRX_CONST DotArgs* ka, const float* xrow, const float* gzrow, int t, int f, int h, int F,
                                                     int D, int self) {
    DiOps<MT, NT> o;
    const int j = 2 * t + h;
    const bool jin = j < F;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int i = 32 * m + f;
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        const bool ok = jin && i < F && (i != j || self != 0);
        const int at = (self != 0 ? hi * (hi + 1) / 2 : hi * (hi - 1) / 2) + lo;
        o.s[m] = ((const NRX_GLOBAL float*)gzrow)[ok ? at : 0];
    }
    const int fo = ka->off[jin ? j : 0];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int c = 32 * n + f;
        o.e[n] = ((const NRX_GLOBAL float*)xrow)[fo + (c < D ? c : 0)];
    }
    return o;
}
template <int MT, int NT>
__device__ __forceinline__ void di_bwd_mask(DiOps<MT, NT>& o, int t, int f, int h, int F, int D, int self) {
    const int j = 2 * t + h;
    const bool jin = j < F;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int i = 32 * m + f;
        const bool ok = jin && i < F && (i != j || self != 0);
        o.s[m] = ok ? (i == j ? 2.f * o.s[m] : o.s[m]) : 0.f;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) o.e[n] = (jin && 32 * n + f < D) ? o.e[n] : 0.f;
}

template <int MT, int NT>
__global__ __launch_bounds__(DI_WAVES * 64) void dot_bwd_kernel(const DotArgs a) {
    const NRX_CONST DotArgs* ka = nrx_kernarg<DotArgs>();
    const int lane = threadIdx.x & 63;
    const int f = lane & 31, h = lane >> 5;
    const int F = a.nf, D = a.dim, self = a.self;
    const int nsteps = (F + 1) >> 1;
    const int64_t stride = (int64_t)gridDim.x * DI_WAVES;
    for (int64_t b = (int64_t)blockIdx.x * DI_WAVES + (threadIdx.x >> 6); b < a.batch; b += stride) {
        const float* xrow = a.x + b * a.ld;
        const float* gzrow = a.g_z + b * a.gz_ld;
        f32x16 acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = f32x16{};
        DiOps<MT, NT> cur = di_bwd_load<MT, NT>(ka, xrow, gzrow, 0, f, h, F, D, self);
        for (int t = 0; t < nsteps; ++t) {
            const DiOps<MT, NT> nxt = di_bwd_load<MT, NT>(ka, xrow, gzrow, t + 1 < nsteps ? t + 1 : t, f, h, F, D, self);
            di_bwd_mask<MT, NT>(cur, t, f, h, F, D, self);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.s[m], cur.e[n], acc[m][n], 0, 0, 0);
            cur = nxt;
        }
        // every read of the sample's g_z row is behind us (the accumulators depend on all of them): g_x may share its buffer
        float* gxrow = a.g_x + b * a.gx_ld;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * m + di_row(r, h);
                const int fo = ka->off[i];                     // (i <= 63: inside the array; a slot past n_fields holds 0 and is not used)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int c = 32 * n + f;
                    if (i < F && c < D) {
                        NRX_GLOBAL float* p = (NRX_GLOBAL float*)gxrow + fo + c;
                        *p = a.accumulate != 0 ? *p + acc[m][n][r] : acc[m][n][r];
                    }
                }
            }
    }
}

template <int VW, int NL>
void dot_fwd_launch2(bool two, dim3 grid, hipStream_t st, const DotArgs& a) {
    const dim3 block(DI_WAVES * 64);
    if (two) hipLaunchKernelGGL((dot_fwd_kernel<VW, NL, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dot_fwd_kernel<VW, NL, 1>), grid, block, 0, st, a);
}
// the loads of a half row: 16-byte pieces when it divides into them (dim % 8 == 0), else 8-byte ones; NL = their count rounded up to a
// power of two (the kernel skips the steps past the real count)
void dot_fwd_launch(dim3 grid, hipStream_t st, const DotArgs& a) {
    const bool two = a.nf > 32;
    if ((a.dim & 7) == 0) {
        const int nl = a.dim / 8;
        if (nl <= 1) dot_fwd_launch2<4, 1>(two, grid, st, a);
        else if (nl <= 2) dot_fwd_launch2<4, 2>(two, grid, st, a);
        else if (nl <= 4) dot_fwd_launch2<4, 4>(two, grid, st, a);
        else dot_fwd_launch2<4, 8>(two, grid, st, a);
    } else {
        const int nl = a.dim / 4;
        if (nl <= 1) dot_fwd_launch2<2, 1>(two, grid, st, a);
        else if (nl <= 4) dot_fwd_launch2<2, 4>(two, grid, st, a);
        else if (nl <= 8) dot_fwd_launch2<2, 8>(two, grid, st, a);
        else dot_fwd_launch2<2, 16>(two, grid, st, a);
    }
}
void dot_bwd_launch(dim3 grid, hipStream_t st, const DotArgs& a) {
    const dim3 block(DI_WAVES * 64);
    const bool m2 = a.nf > 32, n2 = a.dim > 32;
    if (m2 && n2) hipLaunchKernelGGL((dot_bwd_kernel<2, 2>), grid, block, 0, st, a);
    else if (m2) hipLaunchKernelGGL((dot_bwd_kernel<2, 1>), grid, block, 0, st, a);
    else if (n2) hipLaunchKernelGGL((dot_bwd_kernel<1, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dot_bwd_kernel<1, 1>), grid, block, 0, st, a);
}

bool di_f32_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the argument checks both entry points share (NRX_OK or NRX_ERR_BAD_ARG).  `out` / `out_ld` / `out_name`: z of the forward, g_z of the backward
// (P columns each); `inside`: the buffer whose rows `out` may be a column range of (x in the forward, g_x in the backward: the in-place cat
// form), where it must not overlap a field
int dot_check(const char* who, const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t dim, int64_t batch, int32_t flags,
              const float* out, int64_t out_ld, const char* out_name, const float* inside, int64_t inside_ld) {
    NRX_REQUIRE(n_fields >= 1 && dim >= 1 && batch >= 0, "%s: bad argument (n_fields %d, dim %d, batch %lld)", who, n_fields, dim, (long long)batch);
    NRX_REQUIRE((flags & ~NRX_DOT_SELF) == 0, "%s: bad argument (flags %d: bit 0 = NRX_DOT_SELF is the only one defined)", who, flags);
    NRX_REQUIRE(field_off != nullptr, "%s: null field_off", who);
    NRX_REQUIRE(ld >= dim && (ld & 3) == 0, "%s: bad argument (ld %lld: the row stride must hold a field of dim %d and be a multiple of 4)", who,
                (long long)ld, dim);
    const int64_t P = (flags & NRX_DOT_SELF) ? (int64_t)n_fields * (n_fields + 1) / 2 : (int64_t)n_fields * (n_fields - 1) / 2;
    NRX_REQUIRE(out_ld >= P, "%s: bad argument (%s %lld below the %lld pair columns)", who, out_name[0] == 'z' ? "z_ld" : "gz_ld", (long long)out_ld,
                (long long)P);
    for (int32_t i = 0; i < n_fields; ++i) {
        const int64_t o = field_off[i];
        NRX_REQUIRE(o >= 0 && o + dim <= ld, "%s: bad argument (field_off[%d] = %lld: the field leaves the row of ld %lld)", who, i, (long long)o,
                    (long long)ld);
        NRX_REQUIRE((o & 3) == 0, "%s: misaligned field (field_off[%d] = %lld must be a multiple of 4)", who, i, (long long)o);
    }
    if (n_fields <= 4096)          // (far beyond any supported count the quadratic check is not worth its time: NRX_ERR_UNSUPPORTED follows)
        for (int32_t i = 1; i < n_fields; ++i)
            for (int32_t k = 0; k < i; ++k) {
                const int64_t d = (int64_t)field_off[i] - field_off[k];
                NRX_REQUIRE(d >= dim || -d >= dim, "%s: bad argument (field_off[%d] = %d and field_off[%d] = %d overlap at dim %d)", who, k, field_off[k],
                            i, field_off[i], dim);
            }
    if (batch > 0) {
        NRX_REQUIRE(x && out, "%s: null buffer (x or %s)", who, out_name);
        NRX_REQUIRE(nrx_aligned16(x), "%s: misaligned x (every field row must be 16-byte aligned)", who);
        NRX_REQUIRE(di_f32_ok(out), "%s: misaligned %s", who, out_name);
        const uintptr_t lo = reinterpret_cast<uintptr_t>(inside), at_b = reinterpret_cast<uintptr_t>(out) - lo;
        if (inside != nullptr && out_ld == inside_ld && reinterpret_cast<uintptr_t>(out) >= lo && at_b < (uintptr_t)inside_ld * 4 && P > 0) {
            const int64_t at = (int64_t)(at_b / 4);
            NRX_REQUIRE(at + P <= inside_ld, "%s: bad argument (%s starts at column %lld of a row of stride %lld and leaves it)", who, out_name,
                        (long long)at, (long long)inside_ld);
            for (int32_t i = 0; i < n_fields; ++i)
                NRX_REQUIRE(field_off[i] + (int64_t)dim <= at || field_off[i] >= at + P, "%s: bad argument (%s overlaps field %d)", who, out_name, i);
        }
    }
    return NRX_OK;
}

int dot_unsupported(const char* who, int32_t n_fields, int32_t dim) {
    if (n_fields >= 2 && n_fields <= DI_MAX_FIELDS && (dim & 3) == 0 && dim <= DI_MAX_DIM) return NRX_OK;
    nrx_set_error("%s: supports n_fields 2..%d and dim %% 4 == 0 in 4..%d (got n_fields=%d, dim=%d)", who, DI_MAX_FIELDS, DI_MAX_DIM, n_fields, dim);
    return NRX_ERR_UNSUPPORTED;
}

dim3 dot_grid(int64_t batch) {
    const int64_t blocks = (batch + DI_WAVES - 1) / DI_WAVES;
    return dim3((unsigned)(blocks < DI_MAX_BLOCKS ? blocks : DI_MAX_BLOCKS));
}

DotArgs dot_args(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t dim, int64_t batch, int32_t flags) {
    DotArgs a = {};
    a.x = x; a.ld = ld; a.batch = batch; a.nf = n_fields; a.dim = dim; a.self = (flags & NRX_DOT_SELF) != 0;
    for (int i = 0; i < n_fields; ++i) a.off[i] = field_off[i];
    return a;
}

}  // namespace

extern "C" int nrx_dot_interact_fwd(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t dim, int64_t batch, int32_t flags,
                                    float* z, int64_t z_ld, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_dot_interact_fwd";
    int rc = dot_check(who, x, ld, field_off, n_fields, dim, batch, flags, z, z_ld, "z", x, ld);
    if (rc == NRX_OK) rc = dot_unsupported(who, n_fields, dim);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    DotArgs a = dot_args(x, ld, field_off, n_fields, dim, batch, flags);
    a.z = z; a.z_ld = z_ld;
    dot_fwd_launch(dot_grid(batch), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}

extern "C" int nrx_dot_interact_bwd(const float* x, int64_t ld, const int32_t* field_off, int32_t n_fields, int32_t dim, int64_t batch, int32_t flags,
                                    const float* g_z, int64_t gz_ld, float* g_x, int64_t gx_ld, int32_t accumulate, void* stream) {
    NRX_TRACE();
    const char* who = "nrx_dot_interact_bwd";
    NRX_REQUIRE(accumulate == 0 || accumulate == 1, "%s: bad argument (accumulate %d: 0 or 1)", who, accumulate);
    int rc = dot_check(who, x, ld, field_off, n_fields, dim, batch, flags, g_z, gz_ld, "g_z", g_x, gx_ld);
    if (rc != NRX_OK) return rc;
    for (int32_t i = 0; i < n_fields; ++i)
        NRX_REQUIRE(field_off[i] + (int64_t)dim <= gx_ld, "%s: bad argument (gx_ld %lld does not hold field %d: field_off %d + dim %d)", who,
                    (long long)gx_ld, i, field_off[i], dim);
    if (batch > 0) {
        NRX_REQUIRE(g_x != nullptr, "%s: null buffer (g_x)", who);
        NRX_REQUIRE(di_f32_ok(g_x), "%s: misaligned g_x", who);
    }
    rc = dot_unsupported(who, n_fields, dim);
    if (rc != NRX_OK) return rc;
    if (batch == 0) return NRX_OK;
    DotArgs a = dot_args(x, ld, field_off, n_fields, dim, batch, flags);
    a.g_z = g_z; a.gz_ld = gz_ld; a.g_x = g_x; a.gx_ld = gx_ld; a.accumulate = accumulate;
    dot_bwd_launch(dot_grid(batch), reinterpret_cast<hipStream_t>(stream), a);
    NRX_LAUNCH_CHECK(who);
    return NRX_OK;
}
