// tests/auto_period_plan_probe.cpp -- plan_auto_period (csrc/hf_launch_plan.h) for tests/test_auto_period_plan.py: compiled with plain g++ (no
// ROCm include path) as a shared library the test calls through ctypes, and once more with -DHF_PROBE_MAIN as a stand-alone program that
// walks the same grid of inputs under -fsanitize=address,undefined.
#include <stdio.h>

#include "hf_launch_plan.h"

extern "C" {

// out: kMaxAutoPeriodSteps pairs (kind, chunk); returns the number of steps, *early = the plan's early flag
int hfa_plan_auto_period(int defers, int flag, int pending, int mode, int all_have, int chunks, int* out, int* early) {
    const hf::AutoPeriodPlan P = hf::plan_auto_period(defers != 0, flag != 0, pending != 0, mode, all_have != 0, chunks);
    for (int k = 0; k < hf::kMaxAutoPeriodSteps; k++) { out[2 * k] = P.step[k].kind; out[2 * k + 1] = P.step[k].chunk; }
    *early = P.early;
    return P.n_steps;
}

// kMaxAutoPeriodSteps, kMaxPeriodChunks, the six step kinds, the three parts and their union
void hfa_constants(int* out) {
    out[0] = hf::kMaxAutoPeriodSteps; out[1] = hf::kMaxPeriodChunks;
    out[2] = hf::kStepEarlyWarps; out[3] = hf::kStepChain; out[4] = hf::kStepDecide; out[5] = hf::kStepWarps; out[6] = hf::kStepCopy; out[7] = hf::kStepConvert;
    out[8] = hf::kPartWarps; out[9] = hf::kPartCopy; out[10] = hf::kPartConvert; out[11] = hf::kPartsAll;
}

}  // extern "C"

#ifdef HF_PROBE_MAIN
// The properties the Python test states, restated: the whole sequence, step for step.
static int check(bool defers, bool flag, bool pending, int mode, bool all_have, int chunks) {
    const hf::AutoPeriodPlan P = hf::plan_auto_period(defers, flag, pending, mode, all_have, chunks);
    const int n_chunks = chunks < 1 ? 1 : chunks > hf::kMaxPeriodChunks ? hf::kMaxPeriodChunks : chunks;
    const bool early = defers && flag && pending && mode >= 0 && mode <= 2 && all_have && chunks >= 1;
    if ((P.early != 0) != early) return 1;
    if (P.n_steps != 2 + 3 * n_chunks || P.n_steps > hf::kMaxAutoPeriodSteps) return 2;
    int k = 0;
    auto is = [&](int kind, int chunk) { const bool ok = P.step[k].kind == kind && P.step[k].chunk == chunk; k++; return ok; };
    if (early && !is(hf::kStepEarlyWarps, 0)) return 3;
    if (!is(hf::kStepChain, 0) || !is(hf::kStepDecide, 0)) return 4;
    for (int c = 0; c < n_chunks; c++) {
        if (!(early && c == 0) && !is(hf::kStepWarps, c)) return 5;
        if (!is(hf::kStepCopy, c) || !is(hf::kStepConvert, c)) return 6;
    }
    return k == P.n_steps ? 0 : 7;
}

int main() {
    long cases = 0;
    for (int bits = 0; bits < 16; bits++)
        for (int mode = -1; mode <= 7; mode++)
            for (int chunks = -1; chunks <= hf::kMaxPeriodChunks + 1; chunks++) {
                if (int rc = check(bits & 1, bits & 2, bits & 4, mode, bits & 8, chunks)) {
                    printf("auto_period_plan_probe: bits %d mode %d chunks %d: %d\n", bits, mode, chunks, rc);
                    return 1;
                }
                cases++;
            }
    printf("auto_period_plan_probe ok (%ld cases)\n", cases);
    return 0;
}
#endif
