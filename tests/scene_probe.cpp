// tests/scene_probe.cpp -- C face of hopperrender_amd/csrc/hf_scene.h for tests/test_scene_decide.py: the scene-change decision that the
// scene_decide kernel runs per batch member, compiled with plain g++ (no ROCm include path: the compile proves the header HIP-free).
#include "hf_scene.h"

#include <new>

extern "C" {

void* hsp_new() { return new (std::nothrow) hf::SceneState(); }   // value-initialised: all zero
void hsp_free(void* s) { delete static_cast<hf::SceneState*>(s); }
void hsp_clear(void* s) { hf::scene_clear(*static_cast<hf::SceneState*>(s)); }
int hsp_cap(long long source_frame_time) { return hf::scene_history_cap(source_frame_time); }
int hsp_held(const void* s) { return static_cast<const hf::SceneState*>(s)->n; }
int hsp_history() { return hf::kSceneHistory; }

// out: kind, average, d1, d2
void hsp_push(void* s, unsigned delta, int cap, unsigned threshold, int* out) {
    const hf::SceneDecision d = hf::scene_push(*static_cast<hf::SceneState*>(s), delta, cap, threshold);
    out[0] = d.kind; out[1] = d.average; out[2] = d.d1; out[3] = d.d2;
}

// a whole sequence: n deltas pushed in order, out[4 * i ..] = the decision after push i
void hsp_push_many(void* s, const unsigned* deltas, int n, int cap, unsigned threshold, int* out) {
    for (int i = 0; i < n; i++) hsp_push(s, deltas[i], cap, threshold, out + 4 * i);
}

}  // extern "C"
