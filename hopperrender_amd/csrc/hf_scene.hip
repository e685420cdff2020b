// hopperrender_amd/csrc/hf_scene.hip -- scene-cut copy periods of a batch, decided on the device (hf_batch_run_period_auto,
// include/hopperflow.h).  The reference's filter decides per source period whether its outputs are warpFrames or copyFrame from the
// m_totalFrameDelta history (HopperRender.cpp:959-972, 1126-1183), i.e. from a number the period's own chain produces.  A host that asks for
// it waits once per period; a batch exists to never wait.  So the decision follows the chain onto the stream:
//
//   scene_decide_kernel   one thread per member behind the chain's last launch: reads the member's m_totalFrameDelta where the chain
//                         published it, runs scene_push (hf_scene.h: the same function the host tests run), leaves the member's kind in
//                         device memory and one record in mapped host memory (read after hf_batch_sync; precedent: the blur kernel's
//                         still_out).
//   scene_copy_kernel     behind the period's unchanged fused warp launch: workgroups of a member whose kind is copy overwrite its
//                         outputs with copyFrame's bytes (copy_kernel's element arithmetic, hf_levels.h); all others leave after one
//                         uniform load.  Cuts are rare: a cut period wastes its warp, a cut-free period pays two near-empty launches.
//
// Work item of the copy = 16 bytes of one output row (16 / 8 elements), valid columns only: padding columns and everything around the
// frames keep what the warp launch left there, as after hf_copy_frame.  16-byte accesses where strides and bases allow; element by
// element otherwise and for a row's ragged tail.  Grid-stride over at most kSceneCopyBlocks workgroups per member.
#include "hf_kernels.h"
#include "hf_levels.h"
#include "hf_scene.h"

namespace hf {
namespace {

constexpr int kSceneCopyBlock = 256;
constexpr int kSceneCopyBlocks = 64;   // per member: 2160p HDR is 1.5 M items = 95 rounds of a cut member's 64 workgroups

static_assert(sizeof(SceneRecord) == 24, "hf_scene_record (include/hopperflow.h) is six 32-bit words");

__global__ void __launch_bounds__(64) scene_decide_kernel(const SceneDecideArgs a, SceneState* __restrict__ states, int32_t* __restrict__ kinds,
                                                          SceneRecord* __restrict__ records, uint32_t ring) {
    const int m = (int)threadIdx.x;
    if (m >= a.n) return;
    HF_DBG_CHECK(m < kMaxFlowBatch && a.slot[m] < ring && a.cap[m] >= 1 && a.cap[m] <= kSceneHistory, 230);
    SceneState& s = states[m];
    if (a.clear[m]) scene_clear(s);
    uint32_t delta = 0;
    SceneDecision d;
    if (a.push[m]) {
        delta = *(const volatile uint32_t*)a.total_delta[m];   // read once: the chain of this period is done with it
        d = scene_push(s, delta, a.cap[m], a.threshold[m]);
    } else {
        d = scene_decide(s, a.threshold[m]);
    }
    HF_DBG_CHECK(s.n >= 0 && s.n <= kSceneHistory, 231);
    // warpFrames iff m_frameCount >= 3 and no scene change (HopperRender.cpp:1179), unless the host forced the kind
    const int32_t kind = a.force[m] >= 0 ? (a.force[m] ? 1 : 0) : (a.frame_count[m] >= 3u && d.kind ? 1 : 0);
    kinds[m] = kind;
    SceneRecord r;
    r.frame_count = a.frame_count[m]; r.total_delta = delta;
    r.kind = kind; r.average = d.average; r.d1 = d.d1; r.d2 = d.d2;
    records[(size_t)m * ring + a.slot[m]] = r;
}

template <typename E>
__global__ void __launch_bounds__(kSceneCopyBlock) scene_copy_kernel(const Geom g, const SceneCopyArgs a, const int32_t* __restrict__ kinds,
                                                                      const int vec_ok) {
    const int m = (int)blockIdx.y;
    if (kinds[m] != 0) return;   // uniform: this member's period stays warped
    constexpr int VEC = 16 / (int)sizeof(E);
    const SceneCopyArgs::Member& M = a.m[m];
    const int n_out = M.n_out;
    const uint32_t rows = (uint32_t)(g.H + (g.H >> 1));                 // UV plane starts at row H
    const uint32_t per_row = (uint32_t)((g.W + VEC - 1) / VEC);
    const uint32_t items = rows * per_row;
    const Levels lv = make_levels(M.black, M.white);
    const E* __restrict__ src = static_cast<const E*>(M.src);
    for (uint32_t it = blockIdx.x * kSceneCopyBlock + threadIdx.x; it < items; it += gridDim.x * kSceneCopyBlock) {
        const uint32_t row = it / per_row;
        const int cx0 = (int)(it - row * per_row) * VEC;
        const int cz = row >= (uint32_t)g.H;
        HF_DBG_CHECK(row < rows && cx0 < g.W, 232);
        const E* s = src + (size_t)row * g.in_stride + cx0;
        const size_t doff = (size_t)row * g.out_stride + cx0;
        if (vec_ok && cx0 + VEC <= g.W) {
            __attribute__((aligned(16))) E v[VEC];
            *(uint4*)v = *(const uint4*)s;
#pragma unroll
            for (int i = 0; i < VEC; i++) v[i] = (E)(cz ? levels_uv<E>((float)v[i], lv) : levels_y<E>((float)v[i], lv));
            for (int o = 0; o < n_out; o++) *(uint4*)(static_cast<E*>(M.outs[o]) + doff) = *(const uint4*)v;
        } else {
            for (int i = 0; i < VEC && cx0 + i < g.W; i++) {
                const E e = (E)(cz ? levels_uv<E>((float)s[i], lv) : levels_y<E>((float)s[i], lv));
                for (int o = 0; o < n_out; o++) static_cast<E*>(M.outs[o])[doff + i] = e;
            }
        }
    }
}

}  // namespace

void launch_scene_decide(const SceneDecideArgs& a, SceneState* states, int32_t* kinds, SceneRecord* records, uint32_t ring, hipStream_t stream) {
    HF_LAUNCH("scene_decide", scene_decide_kernel, dim3(1), dim3(64), 0, stream, a, states, kinds, records, ring);
}

void launch_scene_copy(const Geom& g, const SceneCopyArgs& a, const int32_t* kinds, hipStream_t stream) {
    const int vec = 16 / (g.hdr ? 2 : 1);
    uintptr_t bits = 0;
    for (int m = 0; m < a.n; m++) {
        bits |= (uintptr_t)a.m[m].src;
        for (int o = 0; o < a.m[m].n_out; o++) bits |= (uintptr_t)a.m[m].outs[o];
    }
    const int vec_ok = (g.in_stride % vec) == 0 && (g.out_stride % vec) == 0 && (bits & 15) == 0;   // plan_copy's condition, for the whole launch
    const size_t items = (size_t)(g.H + (g.H >> 1)) * (size_t)((g.W + vec - 1) / vec);
    const size_t want = (items + kSceneCopyBlock - 1) / kSceneCopyBlock;
    const dim3 grid((unsigned)(want < (size_t)kSceneCopyBlocks ? want : (size_t)kSceneCopyBlocks), (unsigned)a.n);
    if (g.hdr) HF_LAUNCH("scene_copy", scene_copy_kernel<uint16_t>, grid, dim3(kSceneCopyBlock), 0, stream, g, a, kinds, vec_ok);
    else       HF_LAUNCH("scene_copy", scene_copy_kernel<uint8_t>, grid, dim3(kSceneCopyBlock), 0, stream, g, a, kinds, vec_ok);
}

bool dbg_bounds_read_scene(unsigned out[5], bool reset) {
#ifdef HF_DEBUG_BOUNDS
    unsigned rec[5] = {0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(rec, HIP_SYMBOL(g_dbg_bounds), sizeof(rec)) != hipSuccess) return false;
    if (rec[0] && !out[0]) for (int i = 1; i < 5; i++) out[i] = rec[i];
    out[0] += rec[0];
    if (reset) { const unsigned zero[5] = {0, 0, 0, 0, 0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_bounds), zero, sizeof(zero)); }
    return true;
#else
    (void)out; (void)reset;
    return false;
#endif
}

}  // namespace hf
