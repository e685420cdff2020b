// hopperrender_amd/csrc/hf_levels.h -- the element traits and the output-levels arithmetic (warpFrameKernel{SDR,HDR}.h:3-9) every kernel
// that writes output frames shares: warp_kernel / warp_fast_kernel / warp_wg_kernel / copy_kernel (hf_kernels.hip) and the predicated copy
// of hf_scene.hip.  Device code only; include inside a .hip translation unit.
//
// fp32 flavour: the levels reproduce the reference AS IT RUNS ON gfx950 through AMD OpenCL (measured, tests/golden/levels_ramp.npz): the
// division in apply_levels* is x * v_rcp_f32(y); "q*max + mid" is fma(q, max, mid).
#pragma once
#include <stdint.h>

namespace hf {
namespace {

template <typename E> struct ElemTraits;
template <> struct ElemTraits<uint8_t> {
    static constexpr bool hdr = false;
    static constexpr float maxv = 255.0f;
    static constexpr float mid = 128.0f;
    static constexpr unsigned midu = 128u;
    __device__ static __forceinline__ unsigned top8(uint8_t v) { return v; }
};
template <> struct ElemTraits<uint16_t> {
    static constexpr bool hdr = true;
    static constexpr float maxv = 65535.0f;
    static constexpr float mid = 32768.0f;
    static constexpr unsigned midu = 32768u;
    __device__ static __forceinline__ unsigned top8(uint16_t v) { return (unsigned)(v >> 8); }  // calcDeltaSumsKernelHDR.h:98
};

struct Levels {
    float black, white, rcp_y, rcp_uv;
};
__device__ __forceinline__ Levels make_levels(float black, float white) {
    Levels l;
    l.black = black;
    l.white = white;
    l.rcp_y = __builtin_amdgcn_rcpf(white - black);
    l.rcp_uv = __builtin_amdgcn_rcpf(white);
    return l;
}
template <typename E>
__device__ __forceinline__ unsigned levels_y(float v, const Levels& l) {  // warpFrameKernelSDR.h:3-5
    using T = ElemTraits<E>;
    float f = ((v - l.black) * l.rcp_y) * T::maxv;
    f = fmaxf(fminf(f, T::maxv), 0.0f);
    return (unsigned)f & 0xFFFFu;
}
template <typename E>
__device__ __forceinline__ unsigned levels_uv(float v, const Levels& l) {  // warpFrameKernelSDR.h:7-9
    using T = ElemTraits<E>;
    float f = __builtin_fmaf((v - T::mid) * l.rcp_uv, T::maxv, T::mid);
    f = fmaxf(fminf(f, T::maxv), 0.0f);
    return (unsigned)f & 0xFFFFu;
}

}  // namespace
}  // namespace hf
