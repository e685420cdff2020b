// hopperrender_amd/csrc/hf_planar.hip -- planar 4:2:0 frames at the device boundary (HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT,
// include/hopperflow.h): the re-layout between a planar frame (Y plane, U plane, V plane; yuv420p / yuv420p10le) and the semi-planar
// frame every other kernel works on (NV12 / P010).
//
// Both layouts hold 1.5 H S elements and every plane is one flat run of elements, row padding included:
//     planar        Y [0, H S)      U [H S, H S + N)      V [H S + N, H S + 2 N)          N = (H/2) (S/2)
//     semi-planar   Y [0, H S)      UV [H S, H S + 2 N), U(i) at H S + 2 i, V(i) at H S + 2 i + 1
// so the conversion needs no row arithmetic: luma is a flat copy (HDR: << 6 on the way in, >> 6 on the way out, wrapping in 16 bits
// like numpy's uint16 shifts in y4m.py) and chroma a flat (de-)interleave of two runs of N elements.  Padding columns are converted
// like any other element (a planar input's padding reaches only the slot's padding, which no kernel reads).
//
// One work item = 16 bytes of the semi-planar frame: 16 / 8 luma elements (8 / 16 bit) or 8 U + 8 V elements.  Wide accesses (16-byte
// luma and UV, 8- / 16-byte U and V) where the launcher found every plane base aligned for them and the item is whole; element by
// element otherwise (ragged strides put the U / V bases at any element offset).  Grid-stride over at most 2048 workgroups.
//
// Batches (HF_FLAG_BATCH_PLANAR_IN / HF_FLAG_BATCH_PLANAR_OUT, hf_batch.hip) convert many frames of one shape in ONE launch: the same
// work items (planar_in_item / planar_out_item below, shared with the single-frame kernels), blockIdx.y selects a (source, destination)
// pair from a table in the kernel arguments -- up to 32 new frames in, up to 32 x 6 outputs out -- and the wide-access decision is one
// flag pair for the whole launch.  The x extent is capped so the whole launch stays around 2048 workgroups, one at least per frame.
#include "hf_kernels.h"

namespace hf {
namespace {

constexpr int kPlanarBlock = 256;
constexpr int kPlanarMaxBlocks = 2048;

__device__ __forceinline__ uint32_t shl6_u16x2(uint32_t w) { return (w << 6) & 0xFFC0FFC0u; }   // two u16 lanes, each (v << 6) & 0xFFFF
__device__ __forceinline__ uint32_t shr6_u16x2(uint32_t w) { return (w >> 6) & 0x03FF03FFu; }   // two u16 lanes, each v >> 6
__device__ __forceinline__ uint32_t spread8(uint32_t x) { return (x & 0xFFu) | ((x & 0xFF00u) << 8); }          // bytes 0, 1 -> 0, 2
__device__ __forceinline__ uint32_t gather8(uint32_t x) { return (x & 0xFFu) | ((x >> 8) & 0xFF00u); }          // bytes 0, 2 -> 0, 1

struct PlanarShape {     // what every frame of a launch shares
    size_t n_y;          // luma elements H S
    size_t n_c;          // elements of one chroma plane (H/2) (S/2)
    size_t items_y;      // luma work items
    size_t items;        // all work items
    int hdr;
    int vec_y, vec_c;    // the luma / chroma bases (of every frame of the launch) allow the wide accesses
};
struct PlanarArgs {
    const void* src;     // frame read
    void* dst;           // frame written
    PlanarShape sh;
};
// N (source, destination) pairs of one shape; blockIdx.y selects the pair
template <int N>
struct PlanarBatchArgs {
    PlanarShape sh;
    int n;
    const void* src[N];
    void* dst[N];
};
static_assert(sizeof(PlanarBatchArgs<kMaxPlanarOutPairs>) <= 4096, "kernel arguments: 4 KB");

// planar -> semi-planar, work item `it` of one frame; SITE: the first of four debug-bounds site ids of the calling kernel
template <typename T, int SITE>
__device__ __forceinline__ void planar_in_item(const T* __restrict__ s, T* __restrict__ d, const PlanarShape& a, const size_t it) {
    constexpr size_t EL = 16 / sizeof(T);   // luma elements per item
    const T* su = s + a.n_y;
    const T* sv = su + a.n_c;
    T* duv = d + a.n_y;
    if (it < a.items_y) {
        const size_t i0 = it * EL;
        if (a.vec_y && i0 + EL <= a.n_y) {
            HF_DBG_CHECK(i0 + EL <= a.n_y, SITE + 0);
            uint4 v = *reinterpret_cast<const uint4*>(s + i0);
            if (sizeof(T) == 2 && a.hdr) { v.x = shl6_u16x2(v.x); v.y = shl6_u16x2(v.y); v.z = shl6_u16x2(v.z); v.w = shl6_u16x2(v.w); }
            *reinterpret_cast<uint4*>(d + i0) = v;
        } else {
            for (size_t i = i0; i < i0 + EL && i < a.n_y; i++) {
                HF_DBG_CHECK(i < a.n_y, SITE + 1);
                const uint32_t v = s[i];
                d[i] = (T)(a.hdr ? (v << 6) & 0xFFFFu : v);
            }
        }
    } else {
        const size_t k0 = (it - a.items_y) * 8;   // chroma elements k0 .. k0 + 7 of each plane
        if (a.vec_c && k0 + 8 <= a.n_c) {
            HF_DBG_CHECK(k0 + 8 <= a.n_c, SITE + 2);
            if (sizeof(T) == 1) {
                const uint2 u = *reinterpret_cast<const uint2*>(su + k0);
                const uint2 v = *reinterpret_cast<const uint2*>(sv + k0);
                uint4 o;
                o.x = spread8(u.x) | spread8(v.x) << 8;
                o.y = spread8(u.x >> 16) | spread8(v.x >> 16) << 8;
                o.z = spread8(u.y) | spread8(v.y) << 8;
                o.w = spread8(u.y >> 16) | spread8(v.y >> 16) << 8;
                *reinterpret_cast<uint4*>(duv + 2 * k0) = o;
            } else {
                uint4 u = *reinterpret_cast<const uint4*>(su + k0);
                uint4 v = *reinterpret_cast<const uint4*>(sv + k0);
                if (a.hdr) {
                    u.x = shl6_u16x2(u.x); u.y = shl6_u16x2(u.y); u.z = shl6_u16x2(u.z); u.w = shl6_u16x2(u.w);
                    v.x = shl6_u16x2(v.x); v.y = shl6_u16x2(v.y); v.z = shl6_u16x2(v.z); v.w = shl6_u16x2(v.w);
                }
                uint4 o0, o1;
                o0.x = (u.x & 0xFFFFu) | (v.x << 16); o0.y = (u.x >> 16) | (v.x & 0xFFFF0000u);
                o0.z = (u.y & 0xFFFFu) | (v.y << 16); o0.w = (u.y >> 16) | (v.y & 0xFFFF0000u);
                o1.x = (u.z & 0xFFFFu) | (v.z << 16); o1.y = (u.z >> 16) | (v.z & 0xFFFF0000u);
                o1.z = (u.w & 0xFFFFu) | (v.w << 16); o1.w = (u.w >> 16) | (v.w & 0xFFFF0000u);
                *reinterpret_cast<uint4*>(duv + 2 * k0) = o0;
                *reinterpret_cast<uint4*>(duv + 2 * k0 + 8) = o1;
            }
        } else {
            for (size_t k = k0; k < k0 + 8 && k < a.n_c; k++) {
                HF_DBG_CHECK(k < a.n_c, SITE + 3);
                const uint32_t u = su[k], v = sv[k];
                duv[2 * k] = (T)(a.hdr ? (u << 6) & 0xFFFFu : u);
                duv[2 * k + 1] = (T)(a.hdr ? (v << 6) & 0xFFFFu : v);
            }
        }
    }
}

// semi-planar -> planar, work item `it` of one frame
template <typename T, int SITE>
__device__ __forceinline__ void planar_out_item(const T* __restrict__ s, T* __restrict__ d, const PlanarShape& a, const size_t it) {
    constexpr size_t EL = 16 / sizeof(T);
    const T* suv = s + a.n_y;
    T* du = d + a.n_y;
    T* dv = du + a.n_c;
    if (it < a.items_y) {
        const size_t i0 = it * EL;
        if (a.vec_y && i0 + EL <= a.n_y) {
            HF_DBG_CHECK(i0 + EL <= a.n_y, SITE + 0);
            uint4 v = *reinterpret_cast<const uint4*>(s + i0);
            if (sizeof(T) == 2 && a.hdr) { v.x = shr6_u16x2(v.x); v.y = shr6_u16x2(v.y); v.z = shr6_u16x2(v.z); v.w = shr6_u16x2(v.w); }
            *reinterpret_cast<uint4*>(d + i0) = v;
        } else {
            for (size_t i = i0; i < i0 + EL && i < a.n_y; i++) {
                HF_DBG_CHECK(i < a.n_y, SITE + 1);
                const uint32_t v = s[i];
                d[i] = (T)(a.hdr ? v >> 6 : v);
            }
        }
    } else {
        const size_t k0 = (it - a.items_y) * 8;
        if (a.vec_c && k0 + 8 <= a.n_c) {
            HF_DBG_CHECK(k0 + 8 <= a.n_c, SITE + 2);
            if (sizeof(T) == 1) {
                const uint4 w = *reinterpret_cast<const uint4*>(suv + 2 * k0);
                uint2 u, v;
                u.x = gather8(w.x) | gather8(w.y) << 16;
                v.x = gather8(w.x >> 8) | gather8(w.y >> 8) << 16;
                u.y = gather8(w.z) | gather8(w.w) << 16;
                v.y = gather8(w.z >> 8) | gather8(w.w >> 8) << 16;
                *reinterpret_cast<uint2*>(du + k0) = u;
                *reinterpret_cast<uint2*>(dv + k0) = v;
            } else {
                const uint4 w0 = *reinterpret_cast<const uint4*>(suv + 2 * k0);
                const uint4 w1 = *reinterpret_cast<const uint4*>(suv + 2 * k0 + 8);
                uint4 u, v;
                u.x = (w0.x & 0xFFFFu) | (w0.y << 16); v.x = (w0.x >> 16) | (w0.y & 0xFFFF0000u);
                u.y = (w0.z & 0xFFFFu) | (w0.w << 16); v.y = (w0.z >> 16) | (w0.w & 0xFFFF0000u);
                u.z = (w1.x & 0xFFFFu) | (w1.y << 16); v.z = (w1.x >> 16) | (w1.y & 0xFFFF0000u);
                u.w = (w1.z & 0xFFFFu) | (w1.w << 16); v.w = (w1.z >> 16) | (w1.w & 0xFFFF0000u);
                if (a.hdr) {
                    u.x = shr6_u16x2(u.x); u.y = shr6_u16x2(u.y); u.z = shr6_u16x2(u.z); u.w = shr6_u16x2(u.w);
                    v.x = shr6_u16x2(v.x); v.y = shr6_u16x2(v.y); v.z = shr6_u16x2(v.z); v.w = shr6_u16x2(v.w);
                }
                *reinterpret_cast<uint4*>(du + k0) = u;
                *reinterpret_cast<uint4*>(dv + k0) = v;
            }
        } else {
            for (size_t k = k0; k < k0 + 8 && k < a.n_c; k++) {
                HF_DBG_CHECK(k < a.n_c, SITE + 3);
                const uint32_t u = suv[2 * k], v = suv[2 * k + 1];
                du[k] = (T)(a.hdr ? u >> 6 : u);
                dv[k] = (T)(a.hdr ? v >> 6 : v);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(kPlanarBlock) planar_in_kernel(const PlanarArgs a) {
    for (size_t it = (size_t)blockIdx.x * kPlanarBlock + threadIdx.x; it < a.sh.items; it += (size_t)gridDim.x * kPlanarBlock)
        planar_in_item<T, 216>(static_cast<const T*>(a.src), static_cast<T*>(a.dst), a.sh, it);
}

template <typename T>
__global__ void __launch_bounds__(kPlanarBlock) planar_out_kernel(const PlanarArgs a) {
    for (size_t it = (size_t)blockIdx.x * kPlanarBlock + threadIdx.x; it < a.sh.items; it += (size_t)gridDim.x * kPlanarBlock)
        planar_out_item<T, 220>(static_cast<const T*>(a.src), static_cast<T*>(a.dst), a.sh, it);
}

// the new frames of a batch's members: pair blockIdx.y, planar -> the member's ring slot
template <typename T>
__global__ void __launch_bounds__(kPlanarBlock) planar_in_batch_kernel(const PlanarBatchArgs<kMaxFlowBatch> a) {
    const unsigned f = blockIdx.y;
    HF_DBG_CHECK(f < (unsigned)a.n && f < (unsigned)kMaxFlowBatch, 240);
    const T* s = static_cast<const T*>(a.src[f]);
    T* d = static_cast<T*>(a.dst[f]);
    for (size_t it = (size_t)blockIdx.x * kPlanarBlock + threadIdx.x; it < a.sh.items; it += (size_t)gridDim.x * kPlanarBlock)
        planar_in_item<T, 241>(s, d, a.sh, it);
}

// the outputs of a batch's period: pair blockIdx.y, the library's semi-planar stage -> the caller's planar buffer
template <typename T>
__global__ void __launch_bounds__(kPlanarBlock) planar_out_batch_kernel(const PlanarBatchArgs<kMaxPlanarOutPairs> a) {
    const unsigned f = blockIdx.y;
    HF_DBG_CHECK(f < (unsigned)a.n && f < (unsigned)kMaxPlanarOutPairs, 245);
    const T* s = static_cast<const T*>(a.src[f]);
    T* d = static_cast<T*>(a.dst[f]);
    for (size_t it = (size_t)blockIdx.x * kPlanarBlock + threadIdx.x; it < a.sh.items; it += (size_t)gridDim.x * kPlanarBlock)
        planar_out_item<T, 246>(s, d, a.sh, it);
}

bool aligned(const void* p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// the shape of a launch; vec_y / vec_c start out true and planar_shape_add clears them for every frame whose bases rule them out
PlanarShape planar_shape(int hdr, int H, int stride) {
    const size_t EL = 16 / (hdr ? 2 : 1);
    PlanarShape a{};
    a.hdr = hdr;
    a.n_y = (size_t)H * stride;
    a.n_c = (size_t)(H / 2) * (stride / 2);
    a.items_y = (a.n_y + EL - 1) / EL;
    a.items = a.items_y + (a.n_c + 7) / 8;
    a.vec_y = a.vec_c = 1;
    return a;
}

void planar_shape_add(PlanarShape& a, const void* planar_frame, const void* semi_frame) {
    const size_t bpp = a.hdr ? 2 : 1;
    const char* planar = static_cast<const char*>(planar_frame);
    const char* semi = static_cast<const char*>(semi_frame);
    a.vec_y = a.vec_y && aligned(planar, 16) && aligned(semi, 16);
    // U / V runs: 8 elements per access (8 bytes at 8 bit, 16 at 16 bit); the UV run: 16-byte accesses
    a.vec_c = a.vec_c && aligned(planar + a.n_y * bpp, 8 * bpp) && aligned(planar + (a.n_y + a.n_c) * bpp, 8 * bpp) && aligned(semi + a.n_y * bpp, 16);
}

void launch_planar(bool to_planar, int hdr, int H, int stride, const void* src, void* dst, hipStream_t stream) {
    PlanarArgs a{};
    a.src = src; a.dst = dst;
    a.sh = planar_shape(hdr, H, stride);
    planar_shape_add(a.sh, to_planar ? dst : src, to_planar ? src : dst);
    const size_t want = (a.sh.items + kPlanarBlock - 1) / kPlanarBlock;
    const dim3 grid((unsigned)(want < (size_t)kPlanarMaxBlocks ? want : (size_t)kPlanarMaxBlocks));
    if (to_planar) {
        if (hdr) HF_LAUNCH("planar_out_kernel", planar_out_kernel<uint16_t>, grid, dim3(kPlanarBlock), 0, stream, a);
        else     HF_LAUNCH("planar_out_kernel", planar_out_kernel<uint8_t>, grid, dim3(kPlanarBlock), 0, stream, a);
    } else {
        if (hdr) HF_LAUNCH("planar_in_kernel", planar_in_kernel<uint16_t>, grid, dim3(kPlanarBlock), 0, stream, a);
        else     HF_LAUNCH("planar_in_kernel", planar_in_kernel<uint8_t>, grid, dim3(kPlanarBlock), 0, stream, a);
    }
}

template <int N>
dim3 planar_batch_fill(PlanarBatchArgs<N>& a, bool to_planar, int hdr, int H, int stride, int n, const PlanarPair* pairs) {
    a.sh = planar_shape(hdr, H, stride);
    a.n = n;
    for (int i = 0; i < n; i++) {
        a.src[i] = pairs[i].src; a.dst[i] = pairs[i].dst;
        planar_shape_add(a.sh, to_planar ? pairs[i].dst : pairs[i].src, to_planar ? pairs[i].src : pairs[i].dst);   // the AND over all frames
    }
    // around kPlanarMaxBlocks workgroups in the whole launch, one at least per frame
    const size_t want = (a.sh.items + kPlanarBlock - 1) / kPlanarBlock;
    const size_t cap = (size_t)kPlanarMaxBlocks / (size_t)n > 0 ? (size_t)kPlanarMaxBlocks / (size_t)n : 1;
    return dim3((unsigned)(want < cap ? want : cap), (unsigned)n);
}

}  // namespace

void launch_planar_in_batch(int hdr, int H, int stride, int n, const PlanarPair* pairs, hipStream_t stream) {
    if (n < 1 || n > kMaxFlowBatch) return;
    PlanarBatchArgs<kMaxFlowBatch> a{};
    const dim3 grid = planar_batch_fill(a, false, hdr, H, stride, n, pairs);
    if (hdr) HF_LAUNCH("planar_in_batch", planar_in_batch_kernel<uint16_t>, grid, dim3(kPlanarBlock), 0, stream, a);
    else     HF_LAUNCH("planar_in_batch", planar_in_batch_kernel<uint8_t>, grid, dim3(kPlanarBlock), 0, stream, a);
}

void launch_planar_out_batch(int hdr, int H, int stride, int n, const PlanarPair* pairs, hipStream_t stream) {
    if (n < 1 || n > kMaxPlanarOutPairs) return;
    PlanarBatchArgs<kMaxPlanarOutPairs> a{};
    const dim3 grid = planar_batch_fill(a, true, hdr, H, stride, n, pairs);
    if (hdr) HF_LAUNCH("planar_out_batch", planar_out_batch_kernel<uint16_t>, grid, dim3(kPlanarBlock), 0, stream, a);
    else     HF_LAUNCH("planar_out_batch", planar_out_batch_kernel<uint8_t>, grid, dim3(kPlanarBlock), 0, stream, a);
}

void launch_planar_in(int hdr, int H, int stride, const void* planar, void* semi, hipStream_t stream) {
    launch_planar(false, hdr, H, stride, planar, semi, stream);
}

void launch_planar_out(int hdr, int H, int stride, const void* semi, void* planar, hipStream_t stream) {
    launch_planar(true, hdr, H, stride, semi, planar, stream);
}

bool dbg_bounds_read_planar(unsigned out[5], bool reset) {
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
