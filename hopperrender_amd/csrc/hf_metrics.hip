// hopperrender_amd/csrc/hf_metrics.hip -- frame error sums on the device (hf_frame_error*, include/hopperflow.h): how far two frames of
// the context's geometry are apart, per plane, as integer sums -- what a leave-one-out quality evaluation (hopperrender_amd/quality.py)
// and the build's own tests need instead of reading both frames back (24.9 MB per 2160p HDR frame over PCIe, and a host sync per period).
//
// One launch compares up to kMaxErrorPairs pairs (a[i], b[i]); blockIdx.y selects the pair from a pointer table in the kernel arguments
// (the PlanarBatchArgs pattern of hf_planar.hip, the same 4 KB).  Per plane Y, U, V: sum of squared differences, sum of absolute
// differences, largest absolute difference, number of differing elements, number of elements compared -- all integers, so the result does
// not depend on the order of the additions and a test holds it exactly.
//
// A frame is a list of rows, each with `w` compared elements and a pitch (both sides have their own):
//     semi-planar   H luma rows of W, pitch S;   H/2 chroma rows of 2 (W/2) interleaved U, V elements, pitch S, from element H S
//     planar        H luma rows of W, pitch S;   2 (H/2) chroma rows of W/2, pitch S/2, from element H S: the first H/2 are U, the rest V
// Only columns [0, w) of a row are read: the padding [w, pitch) of an output is unspecified (hopperflow.h) and never reaches a sum.
// One work item = 16 bytes of a row on each side (16 / 8 elements): one 16-byte load per side where the launcher found the bases and
// row pitches of EVERY frame of the launch 16-byte aligned and the item lies whole inside [0, w); element by element otherwise (ragged
// row tail, unaligned frames).  Elements at even / odd columns are summed apart -- in an interleaved chroma row that is U / V.
// Per lane: 64-bit sums over its items (two 16-bit elements already overflow 32 bits of squares); then the wave (shuffles), the
// workgroup's waves (LDS), and ONE atomicAdd / atomicMax per quantity, plane and workgroup into the pair's slot, which a hipMemsetAsync
// ahead of the launch zeroed.  Grid-stride over at most ~2048 workgroups per launch, one at least per pair.
#include <type_traits>

#include "hf_ctx.h"

namespace hf {
namespace {

constexpr int kErrBlock = 256;
constexpr int kErrMaxBlocks = 2048;

static_assert(sizeof(FrameErrorSlot) == sizeof(struct hf_frame_error) && offsetof(FrameErrorSlot, max_abs) == offsetof(struct hf_frame_error, max_abs) &&
              offsetof(FrameErrorSlot, count) == offsetof(struct hf_frame_error, count), "FrameErrorSlot is hf_frame_error");

struct ErrorShape {      // what every pair of a launch shares
    uint32_t w_y, w_c;               // compared elements of a luma / chroma row
    uint32_t pitch_ya, pitch_yb;     // row pitches of side a / b, elements
    uint32_t pitch_ca, pitch_cb;
    uint32_t rows_u;                 // planar: chroma rows below this one are U, the others V
    uint32_t segs_y, segs_c;         // work items per row
    uint32_t items_y, items_c;
    FastDiv div_y, div_c;            // item -> row
    size_t base_ca, base_cb;         // first chroma row, elements
    size_t elems_a, elems_b;         // extent of a frame of side a / b (debug-bounds)
    int vec_y, vec_c;                // every luma / chroma row of every frame of the launch starts 16-byte aligned
};
struct ErrorArgs {
    ErrorShape sh;
    int n;
    FrameErrorSlot* slots;           // slot of pair 0
    const void* a[kMaxErrorPairs];
    const void* b[kMaxErrorPairs];
};
static_assert(sizeof(ErrorArgs) <= 4096, "kernel arguments: 4 KB");

// the sums of one work item, elements at even ([0]) and odd ([1]) columns apart; 16 8-bit squares fit 32 bits, two 16-bit ones do not.
// An item is summed by add() alone or by add2() alone; mx and nd hold two 16-bit lanes (add2 keeps them packed, add uses the low one:
// an item has 16 elements at the most), which max_abs() and n_differ() fold.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
template <typename T>
struct Part {
    using Sq = typename std::conditional<sizeof(T) == 1, uint32_t, uint64_t>::type;
    Sq sse[2] = {0, 0};
    uint32_t sad[2] = {0, 0}, mx[2] = {0, 0}, nd[2] = {0, 0};
    template <int PAR>
    __device__ __forceinline__ void add(uint32_t d) {   // one difference, d < 65536
        sse[PAR] += (Sq)d * d; sad[PAR] += d; mx[PAR] = d > mx[PAR] ? d : mx[PAR]; nd[PAR] += d != 0u;
    }
    // two differences of one parity in the 16-bit lanes of d, each below 256: two v_dot2_u32_u16 (squares; times one), one v_pk_max_u16,
    // and (x + 255) >> 8 = [x != 0] per lane
    template <int PAR>
    __device__ __forceinline__ void add2(uint32_t d) {
        const u16x2 v = __builtin_bit_cast(u16x2, d), one = {1, 1};
        sse[PAR] = (Sq)__builtin_amdgcn_udot2(v, v, (uint32_t)sse[PAR], false);
        sad[PAR] = __builtin_amdgcn_udot2(v, one, sad[PAR], false);
        nd[PAR] += ((d + 0x00FF00FFu) >> 8) & 0x00010001u;
        mx[PAR] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(v, __builtin_bit_cast(u16x2, mx[PAR])));
    }
    __device__ __forceinline__ uint32_t max_abs(int par) const { const uint32_t lo = mx[par] & 0xFFFFu, hi = mx[par] >> 16; return lo > hi ? lo : hi; }
    __device__ __forceinline__ uint32_t n_differ(int par) const { return (nd[par] & 0xFFFFu) + (nd[par] >> 16); }
};

struct PlaneAcc {        // one plane's sums of a lane, a wave, a workgroup
    unsigned long long sse, sad;
    uint32_t mx, nd, cnt;
    template <typename P>
    __device__ __forceinline__ void add(const P& p, int par) {
        sse += p.sse[par]; sad += p.sad[par]; const uint32_t m = p.max_abs(par); mx = m > mx ? m : mx; nd += p.n_differ(par);
    }
};

// |a - b| of two 16-bit lanes (v_pk_max_u16, v_pk_min_u16, v_pk_sub_u16)
__device__ __forceinline__ uint32_t absdiff_u16x2(uint32_t a, uint32_t b) {
    const u16x2 va = __builtin_bit_cast(u16x2, a), vb = __builtin_bit_cast(u16x2, b);
    const u16x2 d = __builtin_elementwise_max(va, vb) - __builtin_elementwise_min(va, vb);
    return __builtin_bit_cast(uint32_t, d);
}

// four bytes / two 16-bit words of a row, the first at an even column
template <typename T>
__device__ __forceinline__ void add_word(Part<T>& p, uint32_t a, uint32_t b) {
    if (sizeof(T) == 1) {
        const uint32_t de = absdiff_u16x2(a & 0x00FF00FFu, b & 0x00FF00FFu);                 // columns 0, 2
        const uint32_t dq = absdiff_u16x2((a >> 8) & 0x00FF00FFu, (b >> 8) & 0x00FF00FFu);   // columns 1, 3
        p.template add2<0>(de); p.template add2<1>(dq);
    } else {
        const uint32_t d = absdiff_u16x2(a, b);
        p.template add<0>(d & 0xFFFFu); p.template add<1>(d >> 16);
    }
}

// work item `seg` of one row: ra / rb = the row on either side, oa / ob = the row's first element within its frame (debug-bounds);
// returns the elements compared.  SITE: the first of two debug-bounds site ids.
template <typename T, int SITE>
__device__ __forceinline__ uint32_t row_item(const T* __restrict__ ra, const T* __restrict__ rb, size_t oa, size_t ob, const ErrorShape& s,
                                             uint32_t seg, uint32_t w, int vec, Part<T>& p) {
    constexpr uint32_t EL = 16 / sizeof(T);
    const uint32_t x0 = seg * EL;
    if (vec && x0 + EL <= w) {
        HF_DBG_CHECK(oa + x0 + EL <= s.elems_a && ob + x0 + EL <= s.elems_b, SITE + 0);
        const uint4 va = *reinterpret_cast<const uint4*>(ra + x0), vb = *reinterpret_cast<const uint4*>(rb + x0);
        add_word<T>(p, va.x, vb.x); add_word<T>(p, va.y, vb.y); add_word<T>(p, va.z, vb.z); add_word<T>(p, va.w, vb.w);
        return EL;
    }
    const uint32_t x1 = x0 + EL < w ? x0 + EL : w;
    for (uint32_t x = x0; x < x1; x++) {
        HF_DBG_CHECK(oa + x < s.elems_a && ob + x < s.elems_b, SITE + 1);
        const uint32_t a = ra[x], b = rb[x], d = a > b ? a - b : b - a;
        if (x & 1u) p.template add<1>(d); else p.template add<0>(d);
    }
    return x1 - x0;
}

__device__ __forceinline__ void wave_reduce(PlaneAcc& p) {
    for (int o = 32; o > 0; o >>= 1) {
        p.sse += __shfl_down(p.sse, o); p.sad += __shfl_down(p.sad, o);
        const uint32_t m = __shfl_down(p.mx, o);
        p.mx = m > p.mx ? m : p.mx;
        p.nd += __shfl_down(p.nd, o); p.cnt += __shfl_down(p.cnt, o);
    }
}

template <typename T, bool PLANAR>
__global__ void __launch_bounds__(kErrBlock) frame_error_kernel(const ErrorArgs a) {
    const unsigned f = blockIdx.y;
    HF_DBG_CHECK(f < (unsigned)a.n && f < (unsigned)kMaxErrorPairs, 250);
    const T* __restrict__ fa = static_cast<const T*>(a.a[f]);
    const T* __restrict__ fb = static_cast<const T*>(a.b[f]);
    const ErrorShape& s = a.sh;
    const uint32_t step = gridDim.x * kErrBlock, first = blockIdx.x * kErrBlock + threadIdx.x;
    PlaneAcc acc[3] = {};   // Y, U, V (indexed by constants only)
    for (uint32_t it = first; it < s.items_y; it += step) {
        const uint32_t row = fastdiv(it, s.div_y), seg = it - row * s.segs_y;
        const size_t oa = (size_t)row * s.pitch_ya, ob = (size_t)row * s.pitch_yb;
        Part<T> p;
        acc[0].cnt += row_item<T, 251>(fa + oa, fb + ob, oa, ob, s, seg, s.w_y, s.vec_y, p);
        acc[0].add(p, 0); acc[0].add(p, 1);
    }
    for (uint32_t it = first; it < s.items_c; it += step) {
        const uint32_t row = fastdiv(it, s.div_c), seg = it - row * s.segs_c;
        const size_t oa = s.base_ca + (size_t)row * s.pitch_ca, ob = s.base_cb + (size_t)row * s.pitch_cb;
        Part<T> p;
        const uint32_t n = row_item<T, 253>(fa + oa, fb + ob, oa, ob, s, seg, s.w_c, s.vec_c, p);
        if (PLANAR) {
            if (row < s.rows_u) { acc[1].add(p, 0); acc[1].add(p, 1); acc[1].cnt += n; }
            else                { acc[2].add(p, 0); acc[2].add(p, 1); acc[2].cnt += n; }
        } else {   // interleaved: even columns U, odd columns V; items start at even columns and w_c is even
            acc[1].add(p, 0); acc[2].add(p, 1);
            acc[1].cnt += (n + 1) / 2; acc[2].cnt += n / 2;
        }
    }
    __shared__ PlaneAcc red[3][kErrBlock / 64];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) {
        wave_reduce(acc[pl]);
        if (lane == 0) red[pl][wave] = acc[pl];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned pl = threadIdx.x;
        PlaneAcc t = red[pl][0];
        for (int w = 1; w < kErrBlock / 64; w++) {
            const PlaneAcc& o = red[pl][w];
            t.sse += o.sse; t.sad += o.sad; t.mx = o.mx > t.mx ? o.mx : t.mx; t.nd += o.nd; t.cnt += o.cnt;
        }
        FrameErrorSlot* out = a.slots + f;
        if (t.nd) {   // (a workgroup that saw no difference has nothing but its count to add)
            atomicAdd(reinterpret_cast<unsigned long long*>(&out->sse[pl]), t.sse);
            atomicAdd(reinterpret_cast<unsigned long long*>(&out->sad[pl]), t.sad);
            atomicAdd(reinterpret_cast<unsigned long long*>(&out->n_differ[pl]), (unsigned long long)t.nd);
            atomicMax(&out->max_abs[pl], t.mx);
        }
        if (t.cnt) atomicAdd(reinterpret_cast<unsigned long long*>(&out->count[pl]), (unsigned long long)t.cnt);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

bool launch_frame_errors(int hdr, int H, int W, int stride_a, int stride_b, bool planar, int n, const void* const* a, const void* const* b,
                         FrameErrorSlot* slots, hipStream_t stream) {
    if (n < 1 || n > kMaxErrorPairs) return false;
    const uint32_t bpp = hdr ? 2 : 1, EL = 16 / bpp;
    ErrorArgs k{};
    ErrorShape& s = k.sh;
    s.w_y = (uint32_t)W;
    s.pitch_ya = (uint32_t)stride_a; s.pitch_yb = (uint32_t)stride_b;
    const uint32_t rows_y = (uint32_t)H, rows_c = planar ? 2u * (uint32_t)(H / 2) : (uint32_t)(H / 2);
    s.w_c = planar ? (uint32_t)(W / 2) : 2u * (uint32_t)(W / 2);
    s.pitch_ca = planar ? (uint32_t)(stride_a / 2) : (uint32_t)stride_a;
    s.pitch_cb = planar ? (uint32_t)(stride_b / 2) : (uint32_t)stride_b;
    s.rows_u = (uint32_t)(H / 2);
    s.base_ca = (size_t)H * (size_t)stride_a; s.base_cb = (size_t)H * (size_t)stride_b;
    s.elems_a = s.base_ca + (size_t)rows_c * s.pitch_ca; s.elems_b = s.base_cb + (size_t)rows_c * s.pitch_cb;
    s.segs_y = (s.w_y + EL - 1) / EL; s.segs_c = (s.w_c + EL - 1) / EL;
    const uint64_t items_y = (uint64_t)rows_y * s.segs_y, items_c = (uint64_t)rows_c * s.segs_c;
    if (items_y + (uint64_t)kErrMaxBlocks * kErrBlock >= (1ull << 32) || items_c + (uint64_t)kErrMaxBlocks * kErrBlock >= (1ull << 32)) return false;
    s.items_y = (uint32_t)items_y; s.items_c = (uint32_t)items_c;
    s.div_y = make_fastdiv(s.segs_y ? s.segs_y : 1u, items_y);
    s.div_c = make_fastdiv(s.segs_c ? s.segs_c : 1u, items_c);
    // wide accesses: every row of every frame starts 16-byte aligned (the chroma base is a whole number of luma rows behind the frame's)
    s.vec_y = (s.pitch_ya * bpp) % 16 == 0 && (s.pitch_yb * bpp) % 16 == 0;
    s.vec_c = s.vec_y && (s.pitch_ca * bpp) % 16 == 0 && (s.pitch_cb * bpp) % 16 == 0;
    k.n = n;
    k.slots = slots;
    for (int i = 0; i < n; i++) {
        k.a[i] = a[i]; k.b[i] = b[i];
        if (!aligned16(a[i]) || !aligned16(b[i])) s.vec_y = s.vec_c = 0;
    }
    // around kErrMaxBlocks workgroups in the whole launch, one at least per pair
    const size_t most = items_y > items_c ? (size_t)items_y : (size_t)items_c;
    const size_t want = most ? (most + kErrBlock - 1) / kErrBlock : 1;
    const size_t cap = (size_t)kErrMaxBlocks / (size_t)n > 0 ? (size_t)kErrMaxBlocks / (size_t)n : 1;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)n);
    if (hdr) {
        if (planar) HF_LAUNCH("frame_error", (frame_error_kernel<uint16_t, true>), grid, dim3(kErrBlock), 0, stream, k);
        else        HF_LAUNCH("frame_error", (frame_error_kernel<uint16_t, false>), grid, dim3(kErrBlock), 0, stream, k);
    } else {
        if (planar) HF_LAUNCH("frame_error", (frame_error_kernel<uint8_t, true>), grid, dim3(kErrBlock), 0, stream, k);
        else        HF_LAUNCH("frame_error", (frame_error_kernel<uint8_t, false>), grid, dim3(kErrBlock), 0, stream, k);
    }
    return true;
}

bool dbg_bounds_read_metrics(unsigned out[5], bool reset) {
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

using namespace hfi;

// slots [first, first + n) zeroed, then pair i compared into slot first + i -- behind everything the context has enqueued: warps on a
// second stream (HF_FLAG_DUAL_STREAM) are waited for like hf_download_frame_device does, a batch member issues on the batch's stream.
// max_slot: HF_ERROR_SLOTS for the public range, one more for hf_frame_error's own slot.
static int enqueue_errors(hf_ctx* c, const char* who, int n, const void* const* a, const void* const* b, int stride_a, int stride_b, int planar,
                          int first_slot, int max_slot) {
    HF_CHECK_CTX(c);
    if (!a || !b) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: null frame table", who);
    if (n < 1 || n > HF_MAX_ERROR_PAIRS) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: %d pairs, one launch takes 1 .. %d", who, n, HF_MAX_ERROR_PAIRS);
    if (first_slot < 0 || first_slot > max_slot - n) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: slots [%d, %d + %d) outside [0, %d)", who, first_slot, first_slot, n, HF_ERROR_SLOTS);
    for (int i = 0; i < n; i++)
        if (!a[i] || !b[i]) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: null frame in pair %d", who, i);
    if (stride_a < c->g.W || stride_b < c->g.W) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: strides %d / %d below the frame width %d", who, stride_a, stride_b, c->g.W);
    if (planar && ((stride_a | stride_b) & 1)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: planar frames need even strides (%d / %d)", who, stride_a, stride_b);
    if (int rc = set_device(c)) return rc;
    if (!c->error_slots) HF_HIP(c, alloc_device(c->error_slots, (size_t)(HF_ERROR_SLOTS + 1) * sizeof(hf::FrameErrorSlot)));
    if (int rc = leave_warp_stream(c)) return rc;
    hf::FrameErrorSlot* slots = c->error_slots.get() + first_slot;
    HF_HIP(c, hipMemsetAsync(slots, 0, (size_t)n * sizeof(hf::FrameErrorSlot), c->stream));
    if (!hf::launch_frame_errors(c->g.hdr, c->g.H, c->g.W, stride_a, stride_b, planar != 0, n, a, b, slots, c->stream))
        return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: the frame is too large for one launch", who);
    HF_HIP(c, hipGetLastError());
    return HF_OK;
}

static int read_errors(hf_ctx* c, int first_slot, int n, int max_slot, struct hf_frame_error* out) {
    HF_CHECK_CTX(c);
    if (!out || n < 1 || first_slot < 0 || first_slot > max_slot - n)
        return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_frame_error_read: slots [%d, %d + %d) outside [0, %d), or null", first_slot, first_slot, n, HF_ERROR_SLOTS);
    if (!c->error_slots) return fail(c, HF_ERR_STATE, "hf_frame_error_read: nothing was enqueued");
    if (int rc = set_device(c)) return rc;
    if (int rc = leave_warp_stream(c)) return rc;
    HF_HIP(c, hipMemcpyAsync(out, c->error_slots.get() + first_slot, (size_t)n * sizeof(struct hf_frame_error), hipMemcpyDeviceToHost, c->stream));
    return sync_ctx(c);
}

extern "C" {

int hf_frame_error_enqueue(hf_ctx* c, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b, int planar,
                           int first_slot) {
    return enqueue_errors(c, "hf_frame_error_enqueue", n, device_a, device_b, stride_a, stride_b, planar, first_slot, HF_ERROR_SLOTS);
}

int hf_frame_error_read(hf_ctx* c, int first_slot, int n, struct hf_frame_error* out) { return read_errors(c, first_slot, n, HF_ERROR_SLOTS, out); }

int hf_frame_error(hf_ctx* c, const void* device_a, const void* device_b, int stride_a, int stride_b, int planar, struct hf_frame_error* out) {
    HF_CHECK_CTX(c);
    if (!out) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_frame_error: null result");
    if (int rc = enqueue_errors(c, "hf_frame_error", 1, &device_a, &device_b, stride_a, stride_b, planar, HF_ERROR_SLOTS, HF_ERROR_SLOTS + 1)) return rc;
    return read_errors(c, HF_ERROR_SLOTS, 1, HF_ERROR_SLOTS + 1, out);
}

}  // extern "C"
