// Per-user ranking metrics of the validation loop (base_model.py:333-435): the body of nrx_user_rank_metrics, one user segment at a time.
// Readable by a plain C++ compiler (tests/test_rank_metrics_host.py builds a stand-alone program from this header alone) and by hipcc, where the
// same function runs on the device.
//
// Input: one user's samples scores[lo .. hi) / labels[lo .. hi) in the order the caller ranked them (score descending, arrival order among equal
// scores); labels == 1.0f is a positive, anything else a negative.  P / N = the user's positives / negatives.
//   auc   AUC with ties at 1/2 (sklearn.roc_auc_score) over the groups of equal adjacent scores.  NaN when the user has one class only, when the
//         segment is empty, and when ANY score is NaN or +-inf: the reference wraps roc_auc_score in try/except (base_model.py:380-386), sklearn
//         raises ValueError for a non-finite score, so the reference skips that user's AUC exactly as it skips a single-class user.
//   ndcg, hr, mrr (@k)   from the first min(k, hi - lo) entries IN THE ORDER GIVEN, whatever the scores are (a NaN score is never compared):
//         always finite and in [0, 1]; 0 for a user without a positive and for an empty segment.
// Termination: every pass of the tie loop consumes at least entry i itself (j starts at i + 1), so the loop ends after at most hi - lo passes on any
// input.  (The earlier form started j at i and tested scores[j] == scores[i]: false for a NaN against itself, so it never advanced.)
#ifndef NRX_RANK_METRICS_H
#define NRX_RANK_METRICS_H
#include <math.h>
#include <stdint.h>

#ifndef NRX_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define NRX_HOST_DEVICE __host__ __device__
#else
#define NRX_HOST_DEVICE
#endif
#endif

// NaN and +-inf: all exponent bits set (a bit test, so no compiler flag about finite math can fold it away)
NRX_HOST_DEVICE inline bool nrx_score_nonfinite(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof(u));
    return (u & 0x7f800000u) == 0x7f800000u;
}

NRX_HOST_DEVICE inline void nrx_rank_metrics_user(const float* scores, const float* labels, int64_t lo, int64_t hi, int k,
                                                  double* auc, double* ndcg, double* hr, double* mrr) {
    double P = 0.0;
    bool finite = true;
    for (int64_t i = lo; i < hi; ++i) {
        P += labels[i] == 1.0f ? 1.0 : 0.0;
        if (nrx_score_nonfinite(scores[i])) finite = false;
    }
    const double N = (double)(hi - lo) - P;
    // AUC with ties at 1/2: groups of equal score, descending
    double num = 0.0, neg_above = 0.0;
    if (finite) {
        for (int64_t i = lo; i < hi;) {
            int64_t j = i + 1;          // entry i is always consumed
            double p = labels[i] == 1.0f ? 1.0 : 0.0;
            while (j < hi && scores[j] == scores[i]) {
                p += labels[j] == 1.0f ? 1.0 : 0.0;
                ++j;
            }
            const double q = (double)(j - i) - p;
            num += p * (N - neg_above - q + 0.5 * q);
            neg_above += q;
            i = j;
        }
    }
    *auc = (finite && P > 0.0 && N > 0.0) ? num / (P * N) : __builtin_nan("");
    // top-k metrics (base_model.py:381-433)
    double dcg = 0.0, first = 0.0, hit = 0.0;
    const int64_t top = (hi - lo) < k ? (hi - lo) : k;
    for (int64_t r = 1; r <= top; ++r) {
        if (labels[lo + r - 1] == 1.0f) {
            dcg += 1.0 / log2((double)(r + 1));
            if (first == 0.0) first = 1.0 / (double)r;
            hit = 1.0;
        }
    }
    double idcg = 0.0;
    const int64_t ideal = P < (double)k ? (int64_t)P : k;
    for (int64_t r = 1; r <= ideal; ++r) idcg += 1.0 / log2((double)(r + 1));
    const bool any_pos = P > 0.0;
    *hr = any_pos ? hit : 0.0;
    *ndcg = (any_pos && idcg > 0.0) ? dcg / idcg : 0.0;
    *mrr = any_pos ? first : 0.0;
}
#endif
