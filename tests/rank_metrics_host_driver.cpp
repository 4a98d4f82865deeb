// Stand-alone host program over news_recsys_amd/csrc/nrx_rank_metrics.h alone (plain C++, no HIP, no library): the per-user body of
// nrx_user_rank_metrics run on the CPU.  tests/test_rank_metrics_host.py builds it, runs it under a time limit and compares with the oracle --
// the proof that the function returns on NaN scores, before the same arrays go to the device.
// Input file (argv[1]): "<n_segments>", then per segment "<k> <n>" and n pairs "<score bits> <label bits>" (float32 words in hex, so NaN
// payloads and -0.0 arrive as they are).  Output: per segment one line of four float64 words in hex: auc ndcg hr mrr.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nrx_rank_metrics.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    long n_seg = 0;
    if (fscanf(f, "%ld", &n_seg) != 1) return 2;
    for (long s = 0; s < n_seg; ++s) {
        int k = 0;
        long n = 0;
        if (fscanf(f, "%d %ld", &k, &n) != 2 || n < 0) return 2;
        // two entries of padding in front, so that lo != 0 is exercised too
        std::vector<float> scores(n + 2, 123.0f), labels(n + 2, 1.0f);
        for (long i = 0; i < n; ++i) {
            uint32_t a, b;
            if (fscanf(f, "%" SCNx32 " %" SCNx32, &a, &b) != 2) return 2;
            memcpy(&scores[i + 2], &a, 4);
            memcpy(&labels[i + 2], &b, 4);
        }
        double out[4];
        nrx_rank_metrics_user(scores.data(), labels.data(), 2, n + 2, k, &out[0], &out[1], &out[2], &out[3]);
        uint64_t w[4];
        memcpy(w, out, sizeof(w));
        printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", w[0], w[1], w[2], w[3]);
    }
    fclose(f);
    return 0;
}
