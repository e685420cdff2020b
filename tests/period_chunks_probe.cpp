// tests/period_chunks_probe.cpp -- plan_period_chunks (csrc/hf_launch_plan.h) for tests/test_period_chunks.py: compiled with plain g++ (no ROCm
// include path) as a shared library the test calls through ctypes, and once more with -DHF_PROBE_MAIN as a stand-alone program that walks the
// same grid of n_out vectors under -fsanitize=address,undefined.
#include <stdio.h>

#include "hf_launch_plan.h"

extern "C" {

// out: [0] = n_chunks, then kMaxPeriodChunks rows of kMaxFlowBatch counts
int hfc_plan_period_chunks(int n, const int* n_out, int* out) {
    const hf::PeriodChunks P = hf::plan_period_chunks(n, n_out);
    out[0] = P.n_chunks;
    for (int c = 0; c < hf::kMaxPeriodChunks; c++)
        for (int m = 0; m < hf::kMaxFlowBatch; m++) out[1 + c * hf::kMaxFlowBatch + m] = P.count[c][m];
    return P.n_chunks;
}

void hfc_constants(int* out) {
    out[0] = hf::kMaxWarpOutputs; out[1] = hf::kMaxPeriodOutputsWide; out[2] = hf::kMaxPeriodChunks; out[3] = hf::kMaxFlowBatch;
}

}  // extern "C"

#ifdef HF_PROBE_MAIN
// The properties the Python test states, over every n_out vector of the test's values for 1 and 2 members and the same cyclic vectors of 32.
static int check(int n, const int* n_out) {
    const hf::PeriodChunks P = hf::plan_period_chunks(n, n_out);
    int want_chunks = 0;
    for (int m = 0; m < n; m++) {
        int seen = 0;
        for (int c = 0; c < hf::kMaxPeriodChunks; c++) {
            const int k = P.count[c][m];
            if (k > hf::kMaxWarpOutputs) return 1;
            if (c >= P.n_chunks && k) return 2;
            if (k && seen != c * hf::kMaxWarpOutputs) return 3;   // in order, no gap
            seen += k;
        }
        if (seen != n_out[m]) return 4;
        if ((n_out[m] > 0) != (P.count[0][m] > 0)) return 5;
        const int need = (n_out[m] + hf::kMaxWarpOutputs - 1) / hf::kMaxWarpOutputs;
        want_chunks = need > want_chunks ? need : want_chunks;
    }
    return P.n_chunks == want_chunks ? 0 : 6;
}

int main() {
    const int values[8] = {0, 1, 5, 6, 7, 12, 13, 24};
    int n_out[hf::kMaxFlowBatch];
    long cases = 0;
    for (int a = 0; a < 8; a++) {
        n_out[0] = values[a];
        if (int rc = check(1, n_out)) { printf("period_chunks_probe: 1 member, case %d: %d\n", a, rc); return 1; }
        cases++;
        for (int b = 0; b < 8; b++) {
            n_out[1] = values[b];
            if (int rc = check(2, n_out)) { printf("period_chunks_probe: 2 members, case %d %d: %d\n", a, b, rc); return 1; }
            for (int s = 0; s < 8; s++) {   // 32 members: a, b, then the values cyclically from s
                for (int m = 2; m < hf::kMaxFlowBatch; m++) n_out[m] = values[(s + m) % 8];
                if (int rc = check(hf::kMaxFlowBatch, n_out)) { printf("period_chunks_probe: 32 members, case %d %d %d: %d\n", a, b, s, rc); return 1; }
                cases++;
            }
            cases++;
        }
    }
    printf("period_chunks_probe ok (%ld cases)\n", cases);
    return 0;
}
#endif
