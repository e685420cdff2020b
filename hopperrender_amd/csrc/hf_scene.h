// hopperrender_amd/csrc/hf_scene.h -- the filter's scene-change decision (warp or copy for a source period) as ONE function that the host
// and a kernel both run.
//
// HIP-free (plain g++ -std=c++17, no ROCm include path) and __host__ __device__ under hipcc, like hf_launch_plan.h: integer arithmetic on
// at most 12 numbers, no allocation, no I/O.  It restates hf_filter.cpp:130-161 (hf_filter_push_frame_delta / hf_filter_detect_scene_change,
// themselves HopperRender.cpp:959-972, 1126-1176) with exactly its types and casts; tests/scene_probe.cpp exposes it to
// tests/test_scene_decide.py, which compares it record for record with those two calls of the built library.  The scene_decide kernel of
// hf_scene.hip runs it per batch member behind the member's chain (hf_batch_run_period_auto), so no host waits for m_totalFrameDelta.
//
// What the 3-second window of :959-972 amounts to: the decision looks at the last 12 deltas at most (the average of up to 10, the current
// and the next one), and a history whose pushes are contiguous in m_frameCount holds at most frames_in_3s + 1 entries.  So the state is a
// ring of 12 deltas and the window is a cap on the number held: scene_history_cap().  The 1-second peak statistics (:1151-1158) are
// read-outs that do not feed the decision; they stay with hf_filter.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HF_SCENE_HD __host__ __device__ __forceinline__
#else
#define HF_SCENE_HD inline
#endif

namespace hf {

constexpr int kSceneHistory = 12;   // deltas the decision can look at: average of <= 10 + current + next

// Per member.  All zero = a history that has never seen a delta.
struct SceneState {
    uint32_t delta[kSceneHistory];   // the last n values of m_totalFrameDelta, oldest first
    int32_t n;                       // how many are held
    int32_t average, d1, d2;         // of the last decision that had >= 3 deltas (hf_filter_state: average_frame_delta, scene_change_delta1 / 2)
};

struct SceneDecision {
    int32_t kind;                    // 1: no scene change (warp), 0: scene change (copy)
    int32_t average, d1, d2;
};

// frames_in_3s of hf_filter.cpp:132 as the cap on the number of deltas held: min(12, frames_in_3s + 1)
HF_SCENE_HD int scene_history_cap(int64_t source_frame_time) {
    const int frames_in_3s = (int)(3.0 * 10000000.0 / (double)source_frame_time);
    return frames_in_3s + 1 < kSceneHistory ? frames_in_3s + 1 : kSceneHistory;
}

// NewSegment (hf_filter.cpp:40-46): the history starts over; the read-outs of the last decision stay, as hf_filter's do
HF_SCENE_HD void scene_clear(SceneState& s) { s.n = 0; }

// hf_filter_detect_scene_change (hf_filter.cpp:140-160) on the deltas held
HF_SCENE_HD SceneDecision scene_decide(SceneState& s, uint32_t threshold) {
    const int n = s.n;
    if (n < 3) return SceneDecision{1, s.average, s.d1, s.d2};                          // :143
    const int count = n - 2 < 10 ? n - 2 : 10;                                           // :144
    unsigned long long sum = 0;
    for (int i = 0; i < count; i++) sum += s.delta[n - 2 - i];                           // :146
    const int average = (int)(sum / (unsigned long long)count);                          // :147
    const int next = (int)s.delta[n - 1], current = (int)s.delta[n - 2];                 // :148
    // :149 `current - average`, `current - next` in int.  Deltas at or above 2^31 make the casts negative and the differences can leave the
    // int range; the subtraction is done on the unsigned representations, which is what the two's-complement machine does for the int
    // form and is defined on host and device alike.
    const int d1 = (int)((uint32_t)current - (uint32_t)average), d2 = (int)((uint32_t)current - (uint32_t)next);
    s.average = average; s.d1 = d1; s.d2 = d2;                                           // :150
    const uint32_t thr = threshold;                                                      // :159
    const bool cut = (uint32_t)d1 >= thr && d1 > 0 && (uint32_t)d2 >= thr && d2 > 0;     // :160
    return SceneDecision{cut ? 0 : 1, average, d1, d2};
}

// hf_filter_push_frame_delta (:130-135) + the decision.  cap = scene_history_cap(source_frame_time), in [1, 12].
HF_SCENE_HD SceneDecision scene_push(SceneState& s, uint32_t total_frame_delta, int cap, uint32_t threshold) {
    if (cap < 1) cap = 1;
    if (cap > kSceneHistory) cap = kSceneHistory;
    int n = s.n < 0 ? 0 : s.n;
    if (n >= cap) {                                  // the oldest entries leave the window (:134)
        const int drop = n - cap + 1;
        for (int i = 0; i + drop < n; i++) s.delta[i] = s.delta[i + drop];
        n -= drop;
    }
    s.delta[n] = total_frame_delta;                  // :133
    s.n = n + 1;
    return scene_decide(s, threshold);
}

}  // namespace hf
