// ---------------------------------------------------------------------------------------------------
// Global gradient norm of row-sparse table gradients, and the clipping scale (nrx_rows_sqnorm / nrx_rows_sqnorm_finish / nrx_rows_scale;
// the definition every bit below is pinned to is written down in nrx_embed.h).  The (keys, values) lists of an ops.SparseGradSink never
// become .grad tensors, so torch.nn.utils.clip_grad_norm_ does not see them; these three launches measure and bound them on the device.
//   * a row's sum of squares is formed in DOUBLE in an order that depends on dim only (the lane mapping of sparse_adam_kernel /
//     sparse_adagrad_kernel: Q lanes per row, a float4 per lane, R = 4 rows in flight per lane group), rounded once to fp32;
//   * that fp32 value is added as an INTEGER (its 24-bit significand) into the bin of its exponent: integer adds are associative, so the
//     258 words are a function of the SET of live rows -- whatever the order of a list, its split over calls or over ranks;
//   * the finish launch turns the bins into the norm and the clip coefficient with a fixed ascending sum in double.
// No float atomic anywhere.
// ---------------------------------------------------------------------------------------------------
#include "nrx_common.h"

namespace {

constexpr int NRX_GN_BINS = 258;
constexpr unsigned NRX_GN_MAX_GRID = 1024;      // <= 1024 blocks x (the non-zero bins of a block: a gradient's rows share a handful of exponents) global adds per launch

struct RowsSqnormArgs {
    const int64_t* keys;
    const float* grads;
    const int64_t* n_dev;
    int64_t max_n;
    uint64_t skip_tables;
    unsigned long long* bins;
    int32_t n_tables;
    int32_t dim;
};

template <int CTRL>
__device__ __forceinline__ double gn_dpp(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// x[l] = x[l] + x[l ^ s] for s = 1, 2, 4, ... over the Q = 2^QLOG2 lanes of a row's group, the result in every lane.  After the steps 1 and 2 the four
// lanes of a quad hold the same bits, so the mirror inside each 8 lanes (lane ^ 7) delivers what lane ^ 4 holds, and likewise lane ^ 15 for lane ^ 8:
// the data-parallel moves of adagrad_group_sum serve the plain xor tree.  IEEE addition commutes, so both partners of a step get the same bits.
template <int QLOG2>
__device__ __forceinline__ double gn_group_sum(double v) {
    if (QLOG2 >= 1) v += gn_dpp<0xB1>(v);
    if (QLOG2 >= 2) v += gn_dpp<0x4E>(v);
    if (QLOG2 >= 3) v += gn_dpp<0x141>(v);
    if (QLOG2 >= 4) v += gn_dpp<0x140>(v);
    if (QLOG2 >= 5) v += __shfl_xor(v, 16, 64);
    if (QLOG2 >= 6) v += __shfl_xor(v, 32, 64);
    return v;
}

// (the product of two floats is exact in double, so `acc + g * g` and fma(g, g, acc) are the same bits: contraction cannot change the sum)
__device__ __forceinline__ double gn_sq(float g, double acc) {
    const double d = (double)g;
    return acc + d * d;
}

// VEC: dim % 4 == 0 and 16-byte aligned rows -> one float4 per chunk; otherwise the same chunk element by element.  Lane q of a row's group owns the
// chunks j with j % Q == q in BOTH forms, so the bits do not depend on the alignment of the buffer.  Every load is unconditional (a row that is not
// live, a chunk beyond dim: the address is clamped to one that exists) and masked where the value is used.
template <int QLOG2, bool VEC>
__global__ __launch_bounds__(NRX_BLOCK) void rows_sqnorm_kernel(const RowsSqnormArgs args_in_kernarg) {
    const NRX_CONST RowsSqnormArgs* a = nrx_kernarg<RowsSqnormArgs>();
    constexpr int Q = 1 << QLOG2;
    constexpr int TB = NRX_BLOCK / Q;
    constexpr int R = 4;
    __shared__ unsigned long long lbins[NRX_GN_BINS];
    for (int i = threadIdx.x; i < NRX_GN_BINS; i += NRX_BLOCK) lbins[i] = 0ull;
    __syncthreads();
    const int q = threadIdx.x & (Q - 1);
    const int D = a->dim;
    const int chunks = (D + 3) >> 2;
    const int iters = (chunks + Q - 1) >> QLOG2;          // uniform: every lane of a group walks the same number of chunks
    int64_t n = a->max_n;
    if (a->n_dev != nullptr) {
        const int64_t nd = nrx_gconst<int64_t>(a->n_dev)[0];
        n = nd < n ? nd : n;
    }
    const uint64_t skip = a->skip_tables;
    const int n_tables = a->n_tables;
    // (the trip count is the same for every lane of the block: no lane leaves before the cross-lane sums and the barrier below)
    for (int64_t base = (int64_t)blockIdx.x * (TB * R); base < n; base += (int64_t)gridDim.x * (TB * R)) {
        const int64_t u0 = base + (int64_t)(threadIdx.x >> QLOG2) * R;
        const float* pg[R];
        bool on[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t key = u0 + r < n ? nrx_gconst<int64_t>(a->keys)[u0 + r] : -1;
            const int64_t t = key >> 40, row = key & ((1ll << 40) - 1);
            on[r] = key >= 0 && row != 0 && t < n_tables && ((skip >> (t & 63)) & 1ull) == 0;      // (INT64_MAX names table 2^23 - 1)
            pg[r] = a->grads + (on[r] ? u0 + r : 0) * (int64_t)D;
        }
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        for (int it = 0; it < iters; ++it) {
            const int k = ((it << QLOG2) + q) * 4;
            if (VEC) {
                const bool have = k < D;
                const int kc = have ? k : 0;
                float4 g[R];
#pragma unroll
                for (int r = 0; r < R; ++r) g[r] = nrx_ldg4(pg[r] + kc, 0);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double s = gn_sq(g[r].w, gn_sq(g[r].z, gn_sq(g[r].y, gn_sq(g[r].x, acc[r]))));
                    acc[r] = have ? s : acc[r];
                }
            } else {
                float g[R][4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int kc = k + c < D ? k + c : 0;
#pragma unroll
                    for (int r = 0; r < R; ++r) g[r][c] = nrx_gconst<float>(pg[r])[kc];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool have = k + c < D;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double s = gn_sq(g[r][c], acc[r]);
                        acc[r] = have ? s : acc[r];
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double S = gn_group_sum<QLOG2>(acc[r]);
            const float s32 = (float)S;                              // round to nearest even; a sum beyond FLT_MAX becomes +inf
            const uint32_t b = __builtin_bit_cast(uint32_t, s32) & 0x7FFFFFFFu;
            const uint32_t e = b >> 23, m = b & 0x7FFFFFu;
            uint32_t bin, add;
            if (e == 0) { bin = 1; add = m; }
            else if (e < 255) { bin = e; add = m | 0x800000u; }
            else { bin = m == 0 ? 256 : 257; add = 1; }
            if (on[r] && q == 0 && add != 0) atomicAdd(&lbins[bin], (unsigned long long)add);          // LDS, integer
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NRX_GN_BINS; i += NRX_BLOCK) {
        const unsigned long long v = lbins[i];
        if (v != 0ull) atomicAdd(a->bins + i, v);                  // one integer add per non-zero bin of the block
    }
}

template <bool VEC>
void rows_sqnorm_launch(int ql, unsigned grid, hipStream_t st, const RowsSqnormArgs& a) {
    switch (ql) {
        case 0: hipLaunchKernelGGL((rows_sqnorm_kernel<0, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
        case 1: hipLaunchKernelGGL((rows_sqnorm_kernel<1, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
        case 2: hipLaunchKernelGGL((rows_sqnorm_kernel<2, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
        case 3: hipLaunchKernelGGL((rows_sqnorm_kernel<3, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
        case 4: hipLaunchKernelGGL((rows_sqnorm_kernel<4, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
        case 5: hipLaunchKernelGGL((rows_sqnorm_kernel<5, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
        default: hipLaunchKernelGGL((rows_sqnorm_kernel<6, VEC>), dim3(grid), dim3(NRX_BLOCK), 0, st, a); break;
    }
}

// One block.  Every thread scales its bin(s) into a double in LDS (exact: a power of two), thread 0 adds them in ascending order.
__global__ __launch_bounds__(NRX_BLOCK) void rows_sqnorm_finish_kernel(unsigned long long* __restrict__ bins, const double* __restrict__ extra_sq,
                                                                       double max_norm, double* __restrict__ norm_out, float* __restrict__ coef_out,
                                                                       int rearm) {
    __shared__ double term[NRX_GN_BINS];
    __shared__ unsigned long long special[2];
    for (int i = threadIdx.x; i < NRX_GN_BINS; i += NRX_BLOCK) {
        const unsigned long long v = bins[i];
        double t = 0.0;
        if (i >= 1 && i <= 254) t = (double)v * __builtin_bit_cast(double, (uint64_t)(i + 873) << 52);      // 2^(i - 150)
        term[i] = t;
        if (i >= 256) special[i - 256] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
#pragma unroll 8
        for (int e = 1; e <= 254; ++e) total = total + term[e];
        if (extra_sq != nullptr) total = total + extra_sq[0];
        double norm = sqrt(total);
        if (special[1] > 0ull || total != total) norm = __builtin_nan("");
        else if (special[0] > 0ull) norm = __builtin_inf();
        double c = max_norm / (norm + 1e-6);
        c = c > 1.0 ? 1.0 : c;                  // (a NaN stays a NaN, as in torch.nn.utils.clip_grad_norm_)
        norm_out[0] = norm;
        coef_out[0] = (float)c;
    }
    if (rearm) {
        for (int i = threadIdx.x; i < NRX_GN_BINS; i += NRX_BLOCK) bins[i] = 0ull;      // (every thread zeroes the words it read itself)
    }
}

template <bool VEC>
__global__ __launch_bounds__(NRX_BLOCK) void rows_scale_kernel(float* __restrict__ values, int64_t total, const float* __restrict__ coef_dev) {
    const float coef = nrx_gconst<float>(coef_dev)[0];
    if (coef == 1.0f) return;                   // nothing to clip: no load or store of `values`
    const int64_t stride = (int64_t)gridDim.x * NRX_BLOCK;
    if (VEC) {
        for (int64_t i = (int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x; i < (total >> 2); i += stride) {
            float4 v = nrx_ldg4(values, i);
            v.x = v.x * coef; v.y = v.y * coef; v.z = v.z * coef; v.w = v.w * coef;
            nrx_stg4(values, i, v);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * NRX_BLOCK + threadIdx.x; i < total; i += stride) values[i] = values[i] * coef;
    }
}

}  // namespace

extern "C" int nrx_rows_sqnorm(const int64_t* uniq_keys, const float* grads, int64_t n, const int64_t* n_dev, int32_t n_tables, int32_t dim,
                               uint64_t skip_tables, uint64_t* bins, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(n_tables >= 1 && n_tables <= NRX_MAX_FEATURES && dim >= 1 && n >= 0, "nrx_rows_sqnorm: bad argument");
    if (n == 0) return NRX_OK;
    NRX_REQUIRE(uniq_keys && grads && bins, "nrx_rows_sqnorm: null buffer");
    NRX_REQUIRE((reinterpret_cast<uintptr_t>(uniq_keys) & 7u) == 0 && (reinterpret_cast<uintptr_t>(grads) & 3u) == 0 &&
                (reinterpret_cast<uintptr_t>(bins) & 7u) == 0, "nrx_rows_sqnorm: misaligned pointer");
    RowsSqnormArgs a;
    a.keys = uniq_keys;
    a.grads = grads;
    a.n_dev = n_dev;
    a.max_n = n;
    a.skip_tables = skip_tables;
    a.bins = reinterpret_cast<unsigned long long*>(bins);
    a.n_tables = n_tables;
    a.dim = dim;
    const bool vec = (dim & 3) == 0 && nrx_aligned16(grads);
    const int ql = nrx_row_qlog2(dim);
    const int tb = NRX_BLOCK >> ql;
    const int64_t groups = (n + 3) / 4;                          // 4 rows per lane group and pass
    const int64_t blocks = (groups + tb - 1) / tb;
    const unsigned grid = (unsigned)(blocks < (int64_t)NRX_GN_MAX_GRID ? blocks : (int64_t)NRX_GN_MAX_GRID);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) rows_sqnorm_launch<true>(ql, grid, st, a);
    else rows_sqnorm_launch<false>(ql, grid, st, a);
    NRX_LAUNCH_CHECK("nrx_rows_sqnorm");
    return NRX_OK;
}

extern "C" int nrx_rows_sqnorm_finish(uint64_t* bins, const double* extra_sq_dev, double max_norm, double* norm_out, float* coef_out,
                                      int32_t rearm, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(max_norm > 0.0, "nrx_rows_sqnorm_finish: bad argument (max_norm must be positive)");
    NRX_REQUIRE(bins && norm_out && coef_out, "nrx_rows_sqnorm_finish: null buffer");
    NRX_REQUIRE((reinterpret_cast<uintptr_t>(bins) & 7u) == 0 && (reinterpret_cast<uintptr_t>(extra_sq_dev) & 7u) == 0 &&
                (reinterpret_cast<uintptr_t>(norm_out) & 7u) == 0 && (reinterpret_cast<uintptr_t>(coef_out) & 3u) == 0,
                "nrx_rows_sqnorm_finish: misaligned pointer");
    hipLaunchKernelGGL(rows_sqnorm_finish_kernel, dim3(1), dim3(NRX_BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<unsigned long long*>(bins), extra_sq_dev, max_norm, norm_out, coef_out, (int)rearm);
    NRX_LAUNCH_CHECK("nrx_rows_sqnorm_finish");
    return NRX_OK;
}

extern "C" int nrx_rows_scale(float* values, int64_t n, int32_t dim, const float* coef_dev, void* stream) {
    NRX_TRACE();
    NRX_REQUIRE(dim >= 1 && n >= 0, "nrx_rows_scale: bad argument");
    if (n == 0) return NRX_OK;
    NRX_REQUIRE(values && coef_dev, "nrx_rows_scale: null buffer");
    NRX_REQUIRE((reinterpret_cast<uintptr_t>(values) & 3u) == 0 && (reinterpret_cast<uintptr_t>(coef_dev) & 3u) == 0,
                "nrx_rows_scale: misaligned pointer");
    const int64_t total = n * (int64_t)dim;
    const bool vec = (total & 3) == 0 && nrx_aligned16(values);
    const int64_t work = vec ? total >> 2 : total;
    const int64_t blocks = (work + NRX_BLOCK - 1) / NRX_BLOCK;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(rows_scale_kernel<true>, dim3(grid), dim3(NRX_BLOCK), 0, st, values, total, coef_dev);
    else hipLaunchKernelGGL(rows_scale_kernel<false>, dim3(grid), dim3(NRX_BLOCK), 0, st, values, total, coef_dev);
    NRX_LAUNCH_CHECK("nrx_rows_scale");
    return NRX_OK;
}
