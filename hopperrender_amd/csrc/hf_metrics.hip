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
//
// Further down: the windowed SSIM of the same pairs (hf_frame_ssim*), with its own kernel and slots; the per-tile error maps
// (hf_frame_error_map*): the same sums per tile of 16, 32 or 64 luma pixels, every entry stored once -- no atomics, no memset; and the
// per-tile SSIM maps (hf_frame_ssim_map*), which run the SSIM kernel's block step (ssim_fetch, ssim_sums, ssim_unit_windows: written
// once, over a lane's positions SsimPos) on patches cut to the tile grid.  Then the host side, written once for the four launches:
// frame_layout() (how a frame lies in memory and whether the launch may load 16 bytes at a time), the pointer tables, ssim_plane(),
// the kernel of a format and resident_workgroups(); and the C calls: one enqueue and one read for both families of slots, one shape and
// one enqueue for both kinds of maps.
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

// ---- Windowed SSIM (hf_frame_ssim*; the definition is in include/hopperflow.h) ----
// Per plane: integer sums s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b over the 4 x 4 blocks of the plane; a window is
// 2 x 2 blocks; its score goes through five double operations and comes back as the integer loss 2^32 - round(ssim 2^32).  The same
// pointer table, layouts and pitches as the error sums above, and the same work item: 16 bytes of a row on each side -- here of four
// rows, a UNIT = 4 (8 bit) or 2 (16 bit) blocks; in an interleaved UV row half as many blocks of U and of V each.
// A workgroup takes TILES of kSsimUnitsX units by kSsimRows block rows, the last unit and the last block row of which are halo (read
// again by the neighbouring tile, mostly from L2: 32 / 31 x 16 / 15 = 1.10 of the frame); every lane has two (unit, block row) positions:
//     0. the four 16-byte loads per side of each position are issued (where the launcher found every frame of the launch aligned and
//        the unit lies whole inside the row) -- for the tile AFTER the current one, so that they fly while step 2 computes;
//     1. the blocks of the two units are summed (from those rows; element by element otherwise -- the same integers) and left in LDS;
//     2. after a barrier: per position the column sums of the unit's blocks and of the first block of the unit to the right over this
//        block row and the next, and from two neighbouring column sums each window.
// Tiles are numbered through the planes of a frame (luma, then chroma); a workgroup strides over them, keeps loss sum, largest loss and
// window count per plane in registers, and ends like the error kernel: wave shuffles, LDS, one atomic per quantity and plane.
constexpr int kSsimBlock = 256;
constexpr int kSsimUnitsX = 32, kSsimRows = 16;     // a tile, halo included
constexpr int kSsimItems = kSsimUnitsX * kSsimRows;

static_assert(sizeof(FrameSsimSlot) == sizeof(struct hf_frame_ssim) && offsetof(FrameSsimSlot, max_loss_q32) == offsetof(struct hf_frame_ssim, max_loss_q32) &&
              offsetof(FrameSsimSlot, count) == offsetof(struct hf_frame_ssim, count), "FrameSsimSlot is hf_frame_ssim");

struct SsimPlane {
    uint32_t bw, bh;                 // blocks across / down, per channel
    uint32_t w_row;                  // elements of a row that may be read (interleaved UV: of both channels)
    uint32_t pitch_a, pitch_b;       // elements
    uint32_t tiles_x, tile_first;    // tiles across; number of the plane's first tile within the frame
    int vec;                         // every row of the plane starts 16-byte aligned in every frame of the launch
    size_t base_a, base_b;           // first row, elements
};
struct SsimShape {
    SsimPlane pl[3];                 // luma; interleaved UV, or U and V
    uint32_t tiles;
    size_t elems_a, elems_b;         // extent of a frame of side a / b (debug-bounds)
    long long c1, c2;
};
struct SsimArgs {
    SsimShape sh;
    int n;
    FrameSsimSlot* slots;            // slot of pair 0
    const void* a[kMaxErrorPairs];
    const void* b[kMaxErrorPairs];
};
static_assert(sizeof(SsimArgs) <= 4096, "kernel arguments: 4 KB");

// the sums of a block, of a column of two, of a window: 64 8-bit elements fit 32 bits everywhere, one 16-bit product already fills them
template <typename T>
struct SsimBlk {
    using Q = typename std::conditional<sizeof(T) == 1, uint32_t, uint64_t>::type;
    uint32_t s1, s2;
    Q ss, s12;
    __device__ __forceinline__ void add1(uint32_t a, uint32_t b) { s1 += a; s2 += b; ss += (Q)a * a + (Q)b * b; s12 += (Q)a * b; }
    __device__ __forceinline__ SsimBlk operator+(const SsimBlk& o) const { return SsimBlk{s1 + o.s1, s2 + o.s2, ss + o.ss, s12 + o.s12}; }
};

// a block summed from whole words of its rows (bytes or halves masked away are zero on both sides and add nothing), full-rate dot
// products only.  8 bit: four elements per word, five v_dot4_u32_u8.  16 bit: two elements per word; a 64-bit multiply-add per product
// runs at a quarter of the rate, so the products are taken byte-wise, a = 256 ah + al:  a b = 65536 ah bh + 256 (ah bl + al bh) + al bl.
// Over the bytes of a word, dot4(a, b) = sum (al bl + ah bh), dot4(a & 0x00FF00FF, b) = sum al bl, and against b with the bytes of each
// half swapped, sum (al bh + ah bl); the three 32-bit sums of a block's 16 elements (each below 2^23) go together once, in finish().
template <typename T>
struct SsimWide;
template <>
struct SsimWide<uint8_t> {
    SsimBlk<uint8_t> b = {0, 0, 0, 0};
    __device__ __forceinline__ void add(uint32_t x, uint32_t y) {
        b.s1 = __builtin_amdgcn_udot4(x, 0x01010101u, b.s1, false); b.s2 = __builtin_amdgcn_udot4(y, 0x01010101u, b.s2, false);
        b.ss = __builtin_amdgcn_udot4(x, x, __builtin_amdgcn_udot4(y, y, b.ss, false), false);
        b.s12 = __builtin_amdgcn_udot4(x, y, b.s12, false);
    }
    __device__ __forceinline__ SsimBlk<uint8_t> finish() const { return b; }
};
template <>
struct SsimWide<uint16_t> {
    uint32_t s1 = 0, s2 = 0;
    uint32_t q_all = 0, q_lo = 0, q_x = 0;   // of a^2 + b^2: sum (l^2 + h^2), sum l^2, sum 2 l h
    uint32_t p_all = 0, p_lo = 0, p_x = 0;   // of a b: sum (al bl + ah bh), sum al bl, sum (al bh + ah bl)
    __device__ __forceinline__ void add(uint32_t x, uint32_t y) {
        const u16x2 one = {1, 1};
        s1 = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, x), one, s1, false); s2 = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, y), one, s2, false);
        const uint32_t xs = __builtin_amdgcn_perm(x, x, 0x02030001u), ys = __builtin_amdgcn_perm(y, y, 0x02030001u);   // bytes of each half swapped
        const uint32_t xl = x & 0x00FF00FFu, yl = y & 0x00FF00FFu;
        q_all = __builtin_amdgcn_udot4(x, x, __builtin_amdgcn_udot4(y, y, q_all, false), false);
        q_lo = __builtin_amdgcn_udot4(xl, x, __builtin_amdgcn_udot4(yl, y, q_lo, false), false);
        q_x = __builtin_amdgcn_udot4(x, xs, __builtin_amdgcn_udot4(y, ys, q_x, false), false);
        p_all = __builtin_amdgcn_udot4(x, y, p_all, false); p_lo = __builtin_amdgcn_udot4(xl, y, p_lo, false); p_x = __builtin_amdgcn_udot4(x, ys, p_x, false);
    }
    __device__ __forceinline__ SsimBlk<uint16_t> finish() const {
        return SsimBlk<uint16_t>{s1, s2, ((uint64_t)(q_all - q_lo) << 16) + ((uint64_t)q_x << 8) + q_lo, ((uint64_t)(p_all - p_lo) << 16) + ((uint64_t)p_x << 8) + p_lo};
    }
};

struct SsimAcc {         // one plane's windows of a wave, a workgroup
    unsigned long long sum, mx;
    uint32_t cnt;
};
// ... and of a lane: losses are integers up to 2^33, and a lane sees fewer than 2^20 windows of a plane in a launch (the launcher holds it
// to that), so doubles carry their sum and their maximum exactly -- an add and a max per window where 64-bit integers take a conversion,
// two additions with carry and a three-instruction maximum
struct SsimLane {
    double sum, mx;
    uint32_t cnt;
};
constexpr uint32_t kSsimMaxTilesPerWorkgroup = 1u << 17;   // x 8 windows of a plane per lane and tile

// 2^32 - round(ssim 2^32) of a window's sums, an integer in a double.  Every term is below 2^53 in magnitude, so its conversion is exact;
// two multiplications, one (correctly rounded) division; the scaling is exact, v_rndne_f64 rounds to nearest even, the difference is exact.
template <typename T>
__device__ __forceinline__ double ssim_loss(const SsimBlk<T>& w, long long c1, long long c2) {
    if constexpr (sizeof(T) == 1) {
        // 8 bit: S1, S2 <= 64 * 255, so every term fits 32 bits (2 S1 S2, S1^2 + S2^2, 64 SS <= 2^29; c2 < 2^18) -- the same integers
        // as below through a fraction of the instructions, and one v_cvt_f64_i32 each
        const uint32_t p12 = w.s1 * w.s2, sq = w.s1 * w.s1 + w.s2 * w.s2;
        const int32_t vars = (int32_t)(64u * w.ss - sq), covar = (int32_t)(64u * w.s12) - (int32_t)p12;
        const int32_t A = (int32_t)(2u * p12) + (int32_t)c1, B = 2 * covar + (int32_t)c2, C = (int32_t)sq + (int32_t)c1, D = vars + (int32_t)c2;
        const double num = (double)A * (double)B, den = (double)C * (double)D;
        const double ssim = num / den;
        return 4294967296.0 - rint(ssim * 4294967296.0);
    }
    const long long S1 = w.s1, S2 = w.s2, SS = (long long)w.ss, S12 = (long long)w.s12;
    const long long vars = 64 * SS - S1 * S1 - S2 * S2, covar = 64 * S12 - S1 * S2;
    const long long A = 2 * S1 * S2 + c1, B = 2 * covar + c2, C = S1 * S1 + S2 * S2 + c1, D = vars + c2;
    const double num = (double)A * (double)B, den = (double)C * (double)D;
    const double ssim = num / den;
    return 4294967296.0 - rint(ssim * 4294967296.0);
}

// 16 bytes of a unit's row on either side into the unit's blocks w[channel * BPU + block]
template <typename T, int CH>
__device__ __forceinline__ void ssim_add_row(SsimWide<T>* w, const uint4& a, const uint4& b) {
    if (sizeof(T) == 1) {
        if (CH == 1) { w[0].add(a.x, b.x); w[1].add(a.y, b.y); w[2].add(a.z, b.z); w[3].add(a.w, b.w); }
        else {   // U V U V: even bytes U (blocks 0, 1), odd bytes V (blocks 2, 3)
            constexpr uint32_t m = 0x00FF00FFu;
            w[0].add(a.x & m, b.x & m); w[0].add(a.y & m, b.y & m); w[1].add(a.z & m, b.z & m); w[1].add(a.w & m, b.w & m);
            w[2].add((a.x >> 8) & m, (b.x >> 8) & m); w[2].add((a.y >> 8) & m, (b.y >> 8) & m);
            w[3].add((a.z >> 8) & m, (b.z >> 8) & m); w[3].add((a.w >> 8) & m, (b.w >> 8) & m);
        }
    } else {
        if (CH == 1) { w[0].add(a.x, b.x); w[0].add(a.y, b.y); w[1].add(a.z, b.z); w[1].add(a.w, b.w); }
        else {   // U V: the low halves of two words are two U elements (block 0), the high halves two V elements (block 1); v_perm_b32
            constexpr uint32_t lo = 0x05040100u, hi = 0x07060302u;
            w[0].add(__builtin_amdgcn_perm(a.y, a.x, lo), __builtin_amdgcn_perm(b.y, b.x, lo));
            w[0].add(__builtin_amdgcn_perm(a.w, a.z, lo), __builtin_amdgcn_perm(b.w, b.z, lo));
            w[1].add(__builtin_amdgcn_perm(a.y, a.x, hi), __builtin_amdgcn_perm(b.y, b.x, hi));
            w[1].add(__builtin_amdgcn_perm(a.w, a.z, hi), __builtin_amdgcn_perm(b.w, b.z, hi));
        }
    }
}

// where a tile (or a patch of the map kernel below) starts: plane (0 luma; 1 interleaved UV or U; 2 V), first unit, first block row
struct SsimAt {
    uint32_t pl, u0, j0;
};
// where tile t of a frame lies.  at() is formed at every use: as products carried through the tile loop, u0 and j0 cost the 8-bit
// kernels 4 .. 7 % more instructions
struct SsimTileAt {
    uint32_t pl, tx, ty;
    __device__ __forceinline__ SsimAt at() const { return SsimAt{pl, tx * (uint32_t)(kSsimUnitsX - 1), ty * (uint32_t)(kSsimRows - 1)}; }
};
template <bool PLANAR>
__device__ __forceinline__ SsimTileAt ssim_locate(const SsimShape& s, uint32_t t) {
    const uint32_t pl = t < s.pl[1].tile_first ? 0u : (!PLANAR || t < s.pl[2].tile_first) ? 1u : 2u;
    const uint32_t l = t - s.pl[pl].tile_first, ty = l / s.pl[pl].tiles_x;
    return SsimTileAt{pl, l - ty * s.pl[pl].tiles_x, ty};
}

// a lane's two positions (unit, block row) within its tile or patch; lr = kSsimNoRow: no such position
constexpr int kSsimPerLane = kSsimItems / kSsimBlock;
constexpr uint32_t kSsimNoRow = ~0u;
struct SsimPos {
    uint32_t lu[kSsimPerLane], lr[kSsimPerLane];
    __device__ __forceinline__ bool none(uint32_t n) const { return lr[n] == kSsimNoRow; }
};
// ... of a tile: its shape is a compile-time constant, so every use folds into shifts and masks of threadIdx.x and none() into false
__device__ __forceinline__ SsimPos ssim_tile_pos() {
    SsimPos ps;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)kSsimPerLane; n++) {
        const uint32_t it = threadIdx.x + n * kSsimBlock;
        ps.lu[n] = it % kSsimUnitsX; ps.lr[n] = it / kSsimUnitsX;
    }
    return ps;
}
struct SsimRows {        // the 16-byte loads of a tile still in flight: [position][row] of either side
    uint4 a[kSsimPerLane][4], b[kSsimPerLane][4];
};
template <typename T>
__device__ __forceinline__ bool ssim_wide(const SsimPlane& p, uint32_t u, uint32_t j) {   // unit u of block row j: one 16-byte load per row and side
    constexpr uint32_t EL = 16 / sizeof(T);
    return p.vec && j < p.bh && u * EL + EL <= p.w_row;
}

// The block step of the SSIM kernel and of the map kernel below, over the positions ps of the tile or patch at `at`.  SITE: the first of
// two debug-bounds site ids (elems_a / elems_b: the extent of a frame of either side); LW: units of a row of blocks in LDS.
// step 0: issue the wide loads.  Called for the NEXT tile ahead of the windows of the current one, which hide their latency.
template <typename T, int SITE>
__device__ __forceinline__ void ssim_fetch(const T* __restrict__ fa, const T* __restrict__ fb, size_t elems_a, size_t elems_b, const SsimPlane& p,
                                           const SsimAt& at, const SsimPos& ps, SsimRows& rows) {
    constexpr uint32_t EL = 16 / sizeof(T);
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)kSsimPerLane; n++) {
        const uint32_t u = at.u0 + ps.lu[n], j = at.j0 + ps.lr[n];
        if (ps.none(n) || !ssim_wide<T>(p, u, j)) continue;
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const size_t ia = p.base_a + (size_t)(4u * j + r) * p.pitch_a + u * EL, ib = p.base_b + (size_t)(4u * j + r) * p.pitch_b + u * EL;
            HF_DBG_CHECK(ia + EL <= elems_a && ib + EL <= elems_b && u * EL + EL <= p.w_row, SITE + 0);
            rows.a[n][r] = *reinterpret_cast<const uint4*>(fa + ia); rows.b[n][r] = *reinterpret_cast<const uint4*>(fb + ib);
        }
    }
}

// step 1: the block sums into LDS, from the rows fetched or -- unaligned frames, the ragged end of a row -- element by element.
// CH = 2: an interleaved UV plane.
template <typename T, int CH, int LW, int SITE>
__device__ __forceinline__ void ssim_sums(const T* __restrict__ fa, const T* __restrict__ fb, size_t elems_a, size_t elems_b, const SsimPlane& p,
                                          const SsimAt& at, const SsimPos& ps, const SsimRows& rows, SsimBlk<T> (*lds)[4 / sizeof(T)][LW]) {
    constexpr uint32_t NB = 4 / sizeof(T), BPU = NB / CH;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)kSsimPerLane; n++) {
        const uint32_t lu = ps.lu[n], lr = ps.lr[n], u = at.u0 + lu, j = at.j0 + lr;
        if (ps.none(n) || j >= p.bh || u * BPU >= p.bw) continue;
        SsimBlk<T> blk[NB] = {};
        if (ssim_wide<T>(p, u, j)) {
            SsimWide<T> w[NB];
#pragma unroll
            for (uint32_t r = 0; r < 4; r++) ssim_add_row<T, CH>(w, rows.a[n][r], rows.b[n][r]);
#pragma unroll
            for (uint32_t k = 0; k < NB; k++) blk[k] = w[k].finish();
        } else {
            const size_t oa = p.base_a + (size_t)(4u * j) * p.pitch_a, ob = p.base_b + (size_t)(4u * j) * p.pitch_b;
#pragma unroll
            for (uint32_t c = 0; c < (uint32_t)CH; c++)
#pragma unroll
                for (uint32_t k = 0; k < BPU; k++) {
                    const uint32_t i = u * BPU + k;
                    if (i >= p.bw) continue;   // (a unit past the last whole block of the row: nothing of it is read)
                    for (uint32_t r = 0; r < 4; r++)
                        for (uint32_t e = 0; e < 4; e++) {
                            const uint32_t x = (4u * i + e) * CH + c;
                            const size_t ia = oa + (size_t)r * p.pitch_a + x, ib = ob + (size_t)r * p.pitch_b + x;
                            HF_DBG_CHECK(x < p.w_row && ia < elems_a && ib < elems_b, SITE + 1);
                            blk[c * BPU + k].add1(fa[ia], fb[ib]);
                        }
                }
        }
#pragma unroll
        for (uint32_t k = 0; k < NB; k++) lds[lr][k][lu] = blk[k];   // (units side by side: lanes 16 or 24 bytes apart)
    }
}

// step 2, behind a barrier, for one position that owns windows: the column sums of unit u (at lu, lr in LDS) and of the first block to
// its right over this block row and the next, and each window of the unit as each(loss, channel, block within the unit)
template <typename T, int CH, int LW, typename F>
__device__ __forceinline__ void ssim_unit_windows(const SsimPlane& p, uint32_t u, uint32_t lu, uint32_t lr, long long c1, long long c2,
                                                  const SsimBlk<T> (*lds)[4 / sizeof(T)][LW], F&& each) {
    constexpr uint32_t NB = 4 / sizeof(T), BPU = NB / CH;
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)CH; c++) {
        SsimBlk<T> col[BPU + 1];   // blocks (i, j) + (i, j + 1) of the unit's blocks and of the first one to the right
#pragma unroll
        for (uint32_t k = 0; k < BPU; k++) col[k] = lds[lr][c * BPU + k][lu] + lds[lr + 1][c * BPU + k][lu];
        col[BPU] = lds[lr][c * BPU][lu + 1] + lds[lr + 1][c * BPU][lu + 1];   // (never written where no block is: then no window uses it)
#pragma unroll
        for (uint32_t k = 0; k < BPU; k++) {
            if (u * BPU + k + 1 >= p.bw) continue;
            each(ssim_loss<T>(col[k] + col[k + 1], c1, c2), c, k);
        }
    }
}

// ... of a tile; channel 0 into acc0 and channel 1 into acc1 (CH = 1: acc0 alone)
template <typename T, int CH>
__device__ __forceinline__ void ssim_windows(const SsimShape& s, const SsimPlane& p, const SsimAt& at, const SsimPos& ps,
                                             const SsimBlk<T> (*lds)[4 / sizeof(T)][kSsimUnitsX], SsimLane& acc0, SsimLane& acc1) {
    constexpr uint32_t BPU = 4 / sizeof(T) / CH;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)kSsimPerLane; n++) {
        const uint32_t lu = ps.lu[n], lr = ps.lr[n], u = at.u0 + lu, j = at.j0 + lr;
        if (lu + 1 >= (uint32_t)kSsimUnitsX || lr + 1 >= (uint32_t)kSsimRows || j + 1 >= p.bh || u * BPU + 1 >= p.bw) continue;
        ssim_unit_windows<T, CH, kSsimUnitsX>(p, u, lu, lr, s.c1, s.c2, lds, [&](double loss, uint32_t c, uint32_t) {
            SsimLane& acc = c ? acc1 : acc0;
            acc.sum += loss; acc.mx = fmax(acc.mx, loss); acc.cnt++;
        });
    }
}

template <typename T, bool PLANAR>
__global__ void __launch_bounds__(kSsimBlock) frame_ssim_kernel(const SsimArgs a) {
    __shared__ SsimBlk<T> lds[kSsimRows][4 / sizeof(T)][kSsimUnitsX];
    const unsigned f = blockIdx.y;
    HF_DBG_CHECK(f < (unsigned)a.n && f < (unsigned)kMaxErrorPairs, 257);
    const T* __restrict__ fa = static_cast<const T*>(a.a[f]);
    const T* __restrict__ fb = static_cast<const T*>(a.b[f]);
    const SsimShape& s = a.sh;
    SsimLane acc[3] = {};   // Y, U, V (indexed by constants only)
    SsimRows rows = {};
    uint32_t t = blockIdx.x;
    SsimTileAt at = {0, 0, 0};
    const SsimPos ps = ssim_tile_pos();
    if (t < s.tiles) { at = ssim_locate<PLANAR>(s, t); ssim_fetch<T, 255>(fa, fb, s.elems_a, s.elems_b, s.pl[at.pl], at.at(), ps, rows); }
    while (t < s.tiles) {
        if (at.pl == 0)   ssim_sums<T, 1, kSsimUnitsX, 255>(fa, fb, s.elems_a, s.elems_b, s.pl[0], at.at(), ps, rows, lds);
        else if (!PLANAR) ssim_sums<T, 2, kSsimUnitsX, 255>(fa, fb, s.elems_a, s.elems_b, s.pl[1], at.at(), ps, rows, lds);
        else              ssim_sums<T, 1, kSsimUnitsX, 255>(fa, fb, s.elems_a, s.elems_b, s.pl[at.pl], at.at(), ps, rows, lds);
        __syncthreads();
        const uint32_t tn = t + gridDim.x;
        SsimTileAt nx = at;
        if (tn < s.tiles) { nx = ssim_locate<PLANAR>(s, tn); ssim_fetch<T, 255>(fa, fb, s.elems_a, s.elems_b, s.pl[nx.pl], nx.at(), ps, rows); }
        if (at.pl == 0)       ssim_windows<T, 1>(s, s.pl[0], at.at(), ps, lds, acc[0], acc[0]);
        else if (!PLANAR)     ssim_windows<T, 2>(s, s.pl[1], at.at(), ps, lds, acc[1], acc[2]);
        else if (at.pl == 1)  ssim_windows<T, 1>(s, s.pl[1], at.at(), ps, lds, acc[1], acc[1]);
        else                  ssim_windows<T, 1>(s, s.pl[2], at.at(), ps, lds, acc[2], acc[2]);
        __syncthreads();   // the next tile overwrites the blocks
        t = tn; at = nx;
    }
    __shared__ SsimAcc red[3][kSsimBlock / 64];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) {
        SsimAcc p{(unsigned long long)acc[pl].sum, (unsigned long long)acc[pl].mx, acc[pl].cnt};
        for (int o = 32; o > 0; o >>= 1) {
            p.sum += __shfl_down(p.sum, o);
            const unsigned long long m = __shfl_down(p.mx, o);
            p.mx = m > p.mx ? m : p.mx;
            p.cnt += __shfl_down(p.cnt, o);
        }
        if (lane == 0) red[pl][wave] = p;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned pl = threadIdx.x;
        SsimAcc t = red[pl][0];
        for (int w = 1; w < kSsimBlock / 64; w++) {
            const SsimAcc& o = red[pl][w];
            t.sum += o.sum; t.mx = o.mx > t.mx ? o.mx : t.mx; t.cnt += o.cnt;
        }
        FrameSsimSlot* out = a.slots + f;
        if (t.mx) {   // (windows that are equal add nothing but their number)
            atomicAdd(reinterpret_cast<unsigned long long*>(&out->sum_loss_q32[pl]), t.sum);
            atomicMax(reinterpret_cast<unsigned long long*>(&out->max_loss_q32[pl]), t.mx);
        }
        if (t.cnt) atomicAdd(reinterpret_cast<unsigned long long*>(&out->count[pl]), (unsigned long long)t.cnt);
    }
}

// ---- Per-tile error maps (hf_frame_error_map*; the definition is in include/hopperflow.h) ----
// The error sums above per tile of `tile` x `tile` luma pixels (16, 32 or 64) and plane: one hf_error_tile {sse, sad, max_abs} each, in
// one caller-owned buffer for all pairs of the launch.  Same pointer table, layouts, pitches and work item (16 bytes of a row on each
// side, wide where every frame of the launch is aligned, element by element otherwise) as the error kernel, whose ErrorShape, Part,
// add_word and row_item it uses as they are.
//
// The mapping.  A BAND is the `tile` luma rows of one tile row and the tile / 2 chroma rows under them.  A workgroup (4 waves) owns a
// band of its pair -- blockIdx.x is the band, so workgroups start in the order of the bands in memory -- and reads it the way it lies
// there: a plane's rows one after the other, each row by neighbouring lanes, 16 bytes a lane.  Rows of more than 128 items (2 KB) are
// SWEPT 256 items at a time by the four waves side by side, every wave walking all rows of its 64 items; rows of 65 .. 128 items take two
// waves side by side and the other two the odd rows; shorter rows one wave, and each wave every fourth row.  A lane keeps ONE Part
// over all its rows (at most 64: 64 x 8 squares of 8-bit differences stay far below 2^32).  A tile is 2^lg = tile bytes-per-element /
// 16 items across (1 .. 8), a power of two that divides 64: the lanes of a tile are neighbours inside one wave, and an item never
// straddles two tiles -- but for the two cases below.  So a tile's lanes are reduced by lg xor-shuffle steps; where the rows were dealt
// to several waves, those add up through LDS (one 16-byte entry per wave and tile, two buffers in turn so that one barrier per sweep
// is enough: the waves of the first rows read buffer k & 1 while the next sweep fills the other); and the tile's first lane writes the
// entry as one 16-byte store (neighbouring tiles: neighbouring stores).  Every tile of every plane belongs to exactly one workgroup,
// nothing is added in device memory -- no atomics, no memset -- and every entry is stored exactly once, zeros included.
//   interleaved UV   an item holds U (even columns) and V (odd columns) of ONE tile: Part keeps the parities apart already, each
//                    goes to its own plane's entry (MODE 1: two values per lane)
//   planar, 8 bit, tile 16   a chroma tile row is 8 bytes, an item holds TWO tiles: its halves are summed apart (row_item_halves) and
//                    nothing is shuffled (MODE 2: two values per lane, tiles 2 seg and 2 seg + 1)
// What was measured on the way is in DESIGN.md ("Per-tile error maps"): two mappings that cut a band into strips of 64 items (1 KB of
// a row) -- the rows of a strip dealt to the four waves and combined through LDS, or a strip per wave with neither LDS nor barrier --
// both ran at 1.3 x the error launch at tile 16: not the barrier but the strips were the cost, 1 KB read from every row, where the
// error kernel's workgroups read 4 KB runs in memory order.  Hence whole rows.
// Why not a tile per wave: at tile 16 of 8-bit elements a tile row is ONE item, 16 lanes of a wave would have work and each would read
// 16 bytes of a line of 128.
// LDS: 2 x 4 x 2 x 64 entries = 16 KB a workgroup, no limit below the 8 workgroups a CU holds by waves.
constexpr int kMapBlock = 256, kMapWaves = kMapBlock / 64;
constexpr int kMapMaxBlocks = 1 << 16;   // (341 bands a pair at kMaxErrorPairs: 5456 rows at tile 16)

struct alignas(16) TileSum {   // the layout of hf_error_tile
    unsigned long long sse;
    uint32_t sad, mx;
};
static_assert(sizeof(TileSum) == sizeof(struct hf_error_tile) && offsetof(TileSum, sad) == offsetof(struct hf_error_tile, sad) &&
              offsetof(TileSum, mx) == offsetof(struct hf_error_tile, max_abs), "TileSum is hf_error_tile");

struct MapArgs {
    ErrorShape sh;
    int n;
    uint32_t rows_y;                 // H
    uint32_t tile, lg;               // tile edge in luma pixels; a luma tile is 2^lg work items across
    uint32_t tw, th;
    size_t entries;                  // n 3 th tw (debug-bounds)
    TileSum* maps;                   // [n][3][th][tw]
    const void* a[kMaxErrorPairs];
    const void* b[kMaxErrorPairs];
};
static_assert(sizeof(MapArgs) <= 4096, "kernel arguments: 4 KB");

struct MapPass {         // the rows of one band in one plane (interleaved UV: in both)
    size_t base_a, base_b;           // the plane's first row, elements
    uint32_t pitch_a, pitch_b, w, segs;
    uint32_t r0, r1;                 // the band's rows of the plane
    int vec;
    uint32_t lg;                     // a tile of the plane is 2^lg items across (MODE 2: unused, a tile is half an item)
    uint32_t pl;                     // plane of a lane's first value
};

template <typename P>
__device__ __forceinline__ TileSum tile_sum(const P& p, int par) { return TileSum{p.sse[par], p.sad[par], p.max_abs(par)}; }
__device__ __forceinline__ void merge(TileSum& t, const TileSum& o) { t.sse += o.sse; t.sad += o.sad; t.mx = o.mx > t.mx ? o.mx : t.mx; }

// row_item for 8-bit rows whose tiles are 8 elements across: bytes 0 .. 7 of the item into lo, 8 .. 15 into hi
template <int SITE>
__device__ __forceinline__ void row_item_halves(const uint8_t* __restrict__ ra, const uint8_t* __restrict__ rb, size_t oa, size_t ob, const ErrorShape& s,
                                                uint32_t seg, uint32_t w, int vec, Part<uint8_t>& lo, Part<uint8_t>& hi) {
    const uint32_t x0 = seg * 16u;
    if (vec && x0 + 16u <= w) {
        HF_DBG_CHECK(oa + x0 + 16u <= s.elems_a && ob + x0 + 16u <= s.elems_b, SITE + 0);
        const uint4 va = *reinterpret_cast<const uint4*>(ra + x0), vb = *reinterpret_cast<const uint4*>(rb + x0);
        add_word<uint8_t>(lo, va.x, vb.x); add_word<uint8_t>(lo, va.y, vb.y); add_word<uint8_t>(hi, va.z, vb.z); add_word<uint8_t>(hi, va.w, vb.w);
        return;
    }
    const uint32_t x1 = x0 + 16u < w ? x0 + 16u : w, xm = x0 + 8u < x1 ? x0 + 8u : x1;
    for (uint32_t x = x0; x < x1; x++) {
        HF_DBG_CHECK(oa + x < s.elems_a && ob + x < s.elems_b, SITE + 1);
        const uint32_t a = ra[x], b = rb[x], d = a > b ? a - b : b - a;
        if (x < xm) lo.template add<0>(d); else hi.template add<0>(d);
    }
}

// the finished values of a lane: the entries of its tile(s), where the frame has such a tile
template <int MODE, int NV>
__device__ __forceinline__ void store_tiles(const MapArgs& a, const MapPass& ps, unsigned f, uint32_t j, uint32_t seg, const TileSum (&v)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const uint32_t tx = MODE == 2 ? 2u * seg + (uint32_t)k : seg >> ps.lg;
        const uint32_t pl = MODE == 1 ? ps.pl + (uint32_t)k : ps.pl;
        if (tx < a.tw) {
            const size_t at = (((size_t)f * 3u + pl) * a.th + j) * a.tw + tx;
            HF_DBG_CHECK(at < a.entries && pl < 3u && j < a.th, 267);
            *reinterpret_cast<uint4*>(a.maps + at) = uint4{(uint32_t)v[k].sse, (uint32_t)(v[k].sse >> 32), v[k].sad, v[k].mx};
        }
    }
}

// One plane's rows of band j, by the whole workgroup.  MODE 0: a lane's item lies in one tile of plane ps.pl; 1: interleaved UV, the
// even columns in plane ps.pl and the odd ones in the next; 2: the two halves of the item in two tiles of plane ps.pl.
// step counts the workgroup's trips through LDS (which buffer); every branch around a barrier or a shuffle is uniform.
template <typename T, int MODE, int SITE>
__device__ __forceinline__ void map_pass(const T* __restrict__ fa, const T* __restrict__ fb, const MapArgs& a, const MapPass& ps, unsigned f, uint32_t j,
                                         TileSum (*red)[kMapWaves][2][64], uint32_t& step) {
    constexpr int NV = MODE == 0 ? 1 : 2;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lg_wa = ps.segs > 128u ? 2u : ps.segs > 64u ? 1u : 0u;            // 4, 2 or 1 waves side by side ...
    const uint32_t wa = 1u << lg_wa, phases = (uint32_t)kMapWaves >> lg_wa;          // ... and the rows dealt to 1, 2 or 4 of them
    const uint32_t wc = wave & (wa - 1u), ph = wave >> lg_wa;
    const uint32_t across = 1u << ps.lg;                                             // lanes of a tile (MODE 2: unused)
    const uint32_t slots = MODE == 2 ? 64u : 64u >> ps.lg;                           // lanes of a wave that hold finished values
    const uint32_t sweeps = (ps.segs + 64u * wa - 1u) / (64u * wa);
    for (uint32_t c = 0; c < sweeps; c++) {
        const uint32_t seg0 = (c * wa + wc) * 64u, seg = seg0 + lane;
        Part<T> p, q;
        if (seg < ps.segs) {
            for (uint32_t r = ps.r0 + ph; r < ps.r1; r += phases) {
                const size_t oa = ps.base_a + (size_t)r * ps.pitch_a, ob = ps.base_b + (size_t)r * ps.pitch_b;
                if constexpr (MODE == 2) row_item_halves<SITE>(fa + oa, fb + ob, oa, ob, a.sh, seg, ps.w, ps.vec, p, q);
                else (void)row_item<T, SITE>(fa + oa, fb + ob, oa, ob, a.sh, seg, ps.w, ps.vec, p);
            }
        }
        TileSum v[NV];
        if constexpr (MODE == 0) { v[0] = tile_sum(p, 0); merge(v[0], tile_sum(p, 1)); }
        if constexpr (MODE == 1) { v[0] = tile_sum(p, 0); v[1] = tile_sum(p, 1); }
        if constexpr (MODE == 2) { v[0] = tile_sum(p, 0); merge(v[0], tile_sum(p, 1)); v[1] = tile_sum(q, 0); merge(v[1], tile_sum(q, 1)); }
        if constexpr (MODE != 2) {
            for (uint32_t o = 1; o < across; o <<= 1) {
#pragma unroll
                for (int k = 0; k < NV; k++) {
                    const TileSum t{__shfl_xor(v[k].sse, (int)o), __shfl_xor(v[k].sad, (int)o), __shfl_xor(v[k].mx, (int)o)};
                    merge(v[k], t);
                }
            }
        }
        const bool first = MODE == 2 || (lane & (across - 1u)) == 0u;   // the tile's first lane
        if (phases == 1u) {   // the wave has seen every row of its tiles
            if (first) store_tiles<MODE, NV>(a, ps, f, j, seg, v);
            continue;
        }
        TileSum (*buf)[2][64] = red[step++ & 1u];
        if (first) {
            const uint32_t slot = MODE == 2 ? lane : lane >> ps.lg;
#pragma unroll
            for (int k = 0; k < NV; k++) buf[wave][k][slot] = v[k];
        }
        __syncthreads();
        if (ph == 0u && lane < slots) {   // the waves of the first rows add the others' tiles to their own
#pragma unroll
            for (int k = 0; k < NV; k++) {
                v[k] = buf[wc][k][lane];
                for (uint32_t o = 1; o < phases; o++) merge(v[k], buf[wc + o * wa][k][lane]);
            }
            store_tiles<MODE, NV>(a, ps, f, j, MODE == 2 ? seg0 + lane : seg0 + (lane << ps.lg), v);
        }
    }
}

template <typename T, bool PLANAR>
__global__ void __launch_bounds__(kMapBlock) frame_error_map_kernel(const MapArgs a) {
    __shared__ TileSum red[2][kMapWaves][2][64];
    const unsigned f = blockIdx.y;
    HF_DBG_CHECK(f < (unsigned)a.n && f < (unsigned)kMaxErrorPairs, 260);
    const T* __restrict__ fa = static_cast<const T*>(a.a[f]);
    const T* __restrict__ fb = static_cast<const T*>(a.b[f]);
    const ErrorShape& s = a.sh;
    uint32_t step = 0;
    for (uint32_t j = blockIdx.x; j < a.th; j += gridDim.x) {
        const uint32_t y0 = j * a.tile, y1 = y0 + a.tile < a.rows_y ? y0 + a.tile : a.rows_y;
        const uint32_t c0 = j * (a.tile / 2u), c1 = c0 + a.tile / 2u < s.rows_u ? c0 + a.tile / 2u : s.rows_u;
        map_pass<T, 0, 261>(fa, fb, a, MapPass{0, 0, s.pitch_ya, s.pitch_yb, s.w_y, s.segs_y, y0, y1, s.vec_y, a.lg, 0u}, f, j, red, step);
        if constexpr (!PLANAR) {
            map_pass<T, 1, 263>(fa, fb, a, MapPass{s.base_ca, s.base_cb, s.pitch_ca, s.pitch_cb, s.w_c, s.segs_c, c0, c1, s.vec_c, a.lg, 1u}, f, j, red, step);
        } else {
            for (uint32_t ch = 0; ch < 2u; ch++) {   // V's rows follow U's
                const MapPass ps{s.base_ca + (size_t)ch * s.rows_u * s.pitch_ca, s.base_cb + (size_t)ch * s.rows_u * s.pitch_cb, s.pitch_ca, s.pitch_cb,
                                 s.w_c, s.segs_c, c0, c1, s.vec_c, a.lg ? a.lg - 1u : 0u, 1u + ch};
                if constexpr (sizeof(T) == 1) {
                    if (a.lg == 0u) { map_pass<T, 2, 265>(fa, fb, a, ps, f, j, red, step); continue; }
                }
                map_pass<T, 0, 263>(fa, fb, a, ps, f, j, red, step);
            }
        }
    }
}

// ---- Per-tile SSIM maps (hf_frame_ssim_map*; the definition is in include/hopperflow.h) ----
// The windowed SSIM above kept per tile of the error maps' grid: one hf_ssim_tile {sum_loss_q32, max_loss_q32, count} per tile and plane,
// in one caller-owned buffer for all pairs of the launch.  A window belongs to the tile that holds its first block.  Same pointer table,
// layouts, pitches, unit (16 bytes of four rows on each side) and block step as the SSIM kernel: ssim_fetch, ssim_sums and
// ssim_unit_windows run here over the positions of a patch (smap_pos) and an LDS row of kSmapWidth units.
//
// The mapping.  A PATCH is what a workgroup takes at a time: kSmapRows = 16 block rows of windows by pu units of windows, and one block
// row and one unit of halo behind them (read again by the neighbouring patch: 17 / 16 x (pu + 1) / pu = 1.10 of the frame, as in the
// SSIM kernel).  16 block rows are a whole number of tile rows for every tile (a tile is tb = 2 .. 16 blocks down), and pu is the largest
// multiple of the units a tile is across (tu = 1, 2, 4 or 8) that leaves (pu + 1) x 17 positions within two per lane: 29, 28, 28 or 24.
// So a tile lies whole inside ONE patch and patches start at tile corners: nothing is exchanged between workgroups, every entry is
// stored once by the workgroup that owns it -- no atomics, no memset.  Per patch:
//     0. / 1.  as in the SSIM kernel: the wide loads of the NEXT patch are issued ahead of the windows of this one; block sums into LDS;
//     2. behind a barrier: every position that owns windows (neither halo) scores the windows of its unit and leaves their summed and
//        largest loss in LDS -- as ONE value (the unit lies in one tile), or two: U and V of an interleaved row, or the two halves of a
//        unit that holds two tiles (8-bit planar chroma at tile 16, a tile 2 blocks across and the unit 4);
//     3. behind a second barrier: lanes in rows of 32 (lane = unit, row = value and tile row of the patch; two rounds where there are more
//        than 8) add the tb positions below each other, the tu lanes of a tile meet in xor-shuffles, the tile's first lane stores the
//        24-byte entry -- neighbouring tiles, neighbouring stores.  count is not summed: a tile's windows follow from bw, bh and tb.
// Losses are integers up to 2^33 and a tile has at most 256 windows, so doubles carry sum and maximum exactly (SsimLane).
// Patches are numbered through the planes of a frame and a workgroup strides over them; every plane has at least one patch (a plane
// without a window still has entries, all zero), and tiles past the plane's last window come out of step 3 as zeros.
// LDS: 17 x 4 x 30 blocks of 16 bytes (8 bit; 17 x 2 x 30 of 24 bytes at 16 bit) + 16 x 2 x 32 values of 16 bytes = 48 / 40 KB.
constexpr int kSmapBlock = 256;
constexpr int kSmapRows = 16;       // block rows of windows a patch owns
constexpr int kSmapWidth = 30;      // units of a patch at the most, halo included
constexpr int kSmapOwn = kSmapWidth - 1;
static_assert(kSmapWidth * (kSmapRows + 1) <= kSsimPerLane * kSmapBlock, "a patch is two positions per lane");
static_assert(kSmapOwn <= 32, "step 3: a lane per unit in rows of 32");

struct SsimTileOut {     // the layout of hf_ssim_tile
    unsigned long long sum, mx;
    uint32_t cnt, reserved;
};
static_assert(sizeof(SsimTileOut) == sizeof(struct hf_ssim_tile) && offsetof(SsimTileOut, mx) == offsetof(struct hf_ssim_tile, max_loss_q32) &&
              offsetof(SsimTileOut, cnt) == offsetof(struct hf_ssim_tile, count), "SsimTileOut is hf_ssim_tile");

struct SmapPlane {
    SsimPlane p;                     // (tiles_x, tile_first: patches across, number of the plane's first patch)
    uint32_t pu;                     // units of windows a patch owns
    uint32_t tb, lg_tb;              // tile edge in blocks, 2^lg_tb
    uint32_t lg_tu;                  // a tile is 2^lg_tu units across ...
    uint32_t halves;                 // ... or half a unit
};
struct SmapArgs {
    SmapPlane pl[3];                 // luma; interleaved UV, or U and V
    uint32_t patches;
    uint32_t tw, th;
    int n;
    size_t elems_a, elems_b;         // extent of a frame of side a / b (debug-bounds)
    size_t entries;                  // n 3 th tw (debug-bounds)
    long long c1, c2;
    SsimTileOut* maps;               // [n][3][th][tw]
    const void* a[kMaxErrorPairs];
    const void* b[kMaxErrorPairs];
};
static_assert(sizeof(SmapArgs) <= 4096, "kernel arguments: 4 KB");

template <bool PLANAR>
__device__ __forceinline__ SsimAt smap_locate(const SmapArgs& a, uint32_t t) {   // where patch t of a frame lies
    const uint32_t pl = t < a.pl[1].p.tile_first ? 0u : (!PLANAR || t < a.pl[2].p.tile_first) ? 1u : 2u;
    const uint32_t l = t - a.pl[pl].p.tile_first, py = l / a.pl[pl].p.tiles_x;
    return SsimAt{pl, (l - py * a.pl[pl].p.tiles_x) * a.pl[pl].pu, py * (uint32_t)kSmapRows};
}
// a lane's two positions within a patch pw units wide (halo included) and kSmapRows + 1 block rows high
__device__ __forceinline__ SsimPos smap_pos(uint32_t pw) {
    SsimPos ps;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)kSsimPerLane; n++) {
        const uint32_t it = threadIdx.x + n * kSmapBlock, lr = it / pw;
        ps.lr[n] = lr > (uint32_t)kSmapRows ? kSsimNoRow : lr; ps.lu[n] = it - lr * pw;
    }
    return ps;
}
struct SmapPart {        // the windows of one position in one tile: summed and largest loss
    double sum, mx;
};

// step 2, behind a barrier: the windows of every position that owns some, per position into part[block row][value][unit]
template <typename T, int CH>
__device__ __forceinline__ void smap_windows(const SmapArgs& a, const SmapPlane& m, const SsimAt& at, const SsimPos& ps,
                                             const SsimBlk<T> (*lds)[4 / sizeof(T)][kSmapWidth], SmapPart (*part)[2][32]) {
    constexpr uint32_t BPU = 4 / sizeof(T) / CH;
    const SsimPlane& p = m.p;
#pragma unroll
    for (uint32_t n = 0; n < (uint32_t)kSsimPerLane; n++) {
        const uint32_t lu = ps.lu[n], lr = ps.lr[n], u = at.u0 + lu, j = at.j0 + lr;
        if (lu >= m.pu || lr >= (uint32_t)kSmapRows) continue;   // halo (or no position): its windows are the next patch's
        SmapPart v[2] = {{0.0, 0.0}, {0.0, 0.0}};
        if (j + 1 < p.bh && u * BPU + 1 < p.bw)
            ssim_unit_windows<T, CH, kSmapWidth>(p, u, lu, lr, a.c1, a.c2, lds, [&](double loss, uint32_t c, uint32_t k) {
                const bool second = CH == 2 ? c == 1u : (BPU == 4 && k >= 2u && m.halves);
                SmapPart& t = v[second ? 1 : 0];
                t.sum += loss; t.mx = fmax(t.mx, loss);
            });
        part[lr][0][lu] = v[0]; part[lr][1][lu] = v[1];
    }
}

// N positions below each other in part[][value][unit]
template <int N>
__device__ __forceinline__ void smap_column(const SmapPart* col, double& sum, double& mx) {
    constexpr int G = N < 4 ? N : 4;   // reads in flight at once (16 registers: more would cost the 16-bit kernels a wave per SIMD)
#pragma unroll 1
    for (int r0 = 0; r0 < N; r0 += G) {
        SmapPart v[G];
#pragma unroll
        for (int r = 0; r < G; r++) v[r] = col[(r0 + r) * 2 * 32];
#pragma unroll
        for (int r = 0; r < G; r++) { sum += v[r].sum; mx = fmax(mx, v[r].mx); }
    }
}

// step 3, behind a second barrier: the tiles of the patch out of part[][][] into the pair's map
template <int CH>
__device__ __forceinline__ void smap_store(const SmapArgs& a, const SmapPlane& m, const SsimAt& at, unsigned f, const SmapPart (*part)[2][32]) {
    const uint32_t lu = threadIdx.x & 31u, g = threadIdx.x >> 5;
    const uint32_t two = (CH == 2 || m.halves) ? 1u : 0u;                       // two values per position
    const uint32_t combos = ((uint32_t)kSmapRows >> m.lg_tb) << two;                // (value, tile row of the patch)
    const uint32_t tu = 1u << m.lg_tu;
    for (uint32_t c0 = 0; c0 < combos; c0 += (uint32_t)kSmapBlock / 32u) {      // (uniform: the shuffles below are met by every lane)
        const uint32_t cb = c0 + g, k = two ? cb & 1u : 0u, tr = cb >> two;
        const bool live = cb < combos && lu < m.pu;
        double sum = 0.0, mx = 0.0;
        if (live) {   // the tb positions below each other, all reads in flight at once
            const SmapPart* col = &part[tr << m.lg_tb][k][lu];
            switch (m.lg_tb) {
                case 1: smap_column<2>(col, sum, mx); break;
                case 2: smap_column<4>(col, sum, mx); break;
                case 3: smap_column<8>(col, sum, mx); break;
                default: smap_column<16>(col, sum, mx); break;
            }
        }
        if (!m.halves)
            for (uint32_t o = 1; o < tu; o <<= 1) { sum += __shfl_xor(sum, (int)o); mx = fmax(mx, __shfl_xor(mx, (int)o)); }
        if (!live || (!m.halves && (lu & (tu - 1u)))) continue;
        const uint32_t tx = m.halves ? 2u * (at.u0 + lu) + k : (at.u0 + lu) >> m.lg_tu, ty = (at.j0 >> m.lg_tb) + tr;
        const uint32_t pl = CH == 2 ? at.pl + k : at.pl;
        if (tx >= a.tw || ty >= a.th) continue;
        // the tile's windows: first blocks [tx tb, (tx + 1) tb) x [ty tb, (ty + 1) tb) among [0, bw - 1) x [0, bh - 1)
        const int tb = (int)m.tb, left = (int)m.p.bw - 1 - (int)(tx * m.tb), below = (int)m.p.bh - 1 - (int)(ty * m.tb);
        const int nx = left < 0 ? 0 : left < tb ? left : tb, ny = below < 0 ? 0 : below < tb ? below : tb;
        const size_t e = (((size_t)f * 3u + pl) * a.th + ty) * a.tw + tx;
        HF_DBG_CHECK(e < a.entries && pl < 3u, 273);
        unsigned long long* out = reinterpret_cast<unsigned long long*>(a.maps + e);
        out[0] = (unsigned long long)sum; out[1] = (unsigned long long)mx; out[2] = (unsigned long long)(uint32_t)(nx * ny);
    }
}

template <typename T, bool PLANAR>
__global__ void __launch_bounds__(kSmapBlock) frame_ssim_map_kernel(const SmapArgs a) {
    __shared__ SsimBlk<T> lds[kSmapRows + 1][4 / sizeof(T)][kSmapWidth];
    __shared__ SmapPart part[kSmapRows][2][32];
    const unsigned f = blockIdx.y;
    HF_DBG_CHECK(f < (unsigned)a.n && f < (unsigned)kMaxErrorPairs, 270);
    const T* __restrict__ fa = static_cast<const T*>(a.a[f]);
    const T* __restrict__ fb = static_cast<const T*>(a.b[f]);
    SsimRows rows = {};
    uint32_t t = blockIdx.x;
    SsimAt at = {0, 0, 0};
    SsimPos ps = {};
    if (t < a.patches) {
        at = smap_locate<PLANAR>(a, t); ps = smap_pos(a.pl[at.pl].pu + 1u);
        ssim_fetch<T, 271>(fa, fb, a.elems_a, a.elems_b, a.pl[at.pl].p, at, ps, rows);
    }
    while (t < a.patches) {
        const SmapPlane& m = a.pl[at.pl];
        const bool uv = !PLANAR && at.pl != 0;   // an interleaved UV plane: two channels
        if (uv) ssim_sums<T, 2, kSmapWidth, 271>(fa, fb, a.elems_a, a.elems_b, m.p, at, ps, rows, lds);
        else    ssim_sums<T, 1, kSmapWidth, 271>(fa, fb, a.elems_a, a.elems_b, m.p, at, ps, rows, lds);
        __syncthreads();
        const uint32_t tn = t + gridDim.x;
        SsimAt nx = at;
        SsimPos pn = ps;
        if (tn < a.patches) {
            nx = smap_locate<PLANAR>(a, tn);
            if (a.pl[nx.pl].pu != m.pu) pn = smap_pos(a.pl[nx.pl].pu + 1u);
            ssim_fetch<T, 271>(fa, fb, a.elems_a, a.elems_b, a.pl[nx.pl].p, nx, pn, rows);
        }
        if (uv) smap_windows<T, 2>(a, m, at, ps, lds, part);
        else    smap_windows<T, 1>(a, m, at, ps, lds, part);
        __syncthreads();   // the next patch overwrites the blocks; its windows, behind its own barrier, the values
        if (uv) smap_store<2>(a, m, at, f, part);
        else    smap_store<1>(a, m, at, f, part);
        t = tn; at = nx; ps = pn;
    }
}

// ---- The host side of the four launches ----
// How a frame lies in memory (the layouts at the top of this file), derived HERE for all four launchers, and the one decision it takes:
// wide loads need the row pitches of both sides AND the base of every frame of the launch 16-byte aligned (the chroma bases are whole
// numbers of rows behind the frame's), so one unaligned frame turns them off for the whole launch.  ok = false: n outside 1 .. kMaxErrorPairs.
struct FrameLayout {
    bool ok, planar;
    uint32_t H, W;
    uint32_t bpp;                    // bytes per element
    uint32_t pitch_ya, pitch_yb;     // row pitches of side a / b, elements
    uint32_t pitch_ca, pitch_cb;
    size_t base_ca, base_cb;         // first chroma row, elements
    uint32_t rows_c;                 // chroma rows (planar: U's, then V's)
    size_t elems_a, elems_b;         // extent of a frame of side a / b (debug-bounds)
    int vec_y, vec_c;                // every luma / chroma row of every frame of the launch starts 16-byte aligned
};
FrameLayout frame_layout(int hdr, int H, int W, int stride_a, int stride_b, bool planar, int n, const void* const* a, const void* const* b) {
    FrameLayout l{};
    if (n < 1 || n > kMaxErrorPairs) return l;
    l.ok = true; l.planar = planar; l.H = (uint32_t)H; l.W = (uint32_t)W;
    l.bpp = hdr ? 2 : 1;
    l.pitch_ya = (uint32_t)stride_a; l.pitch_yb = (uint32_t)stride_b;
    l.pitch_ca = planar ? (uint32_t)(stride_a / 2) : (uint32_t)stride_a;
    l.pitch_cb = planar ? (uint32_t)(stride_b / 2) : (uint32_t)stride_b;
    l.base_ca = (size_t)H * (size_t)stride_a; l.base_cb = (size_t)H * (size_t)stride_b;
    l.rows_c = planar ? 2u * (uint32_t)(H / 2) : (uint32_t)(H / 2);
    l.elems_a = l.base_ca + (size_t)l.rows_c * l.pitch_ca; l.elems_b = l.base_cb + (size_t)l.rows_c * l.pitch_cb;
    l.vec_y = (l.pitch_ya * l.bpp) % 16 == 0 && (l.pitch_yb * l.bpp) % 16 == 0;
    for (int i = 0; i < n; i++)
        if (((uintptr_t)a[i] | (uintptr_t)b[i]) & 15u) l.vec_y = 0;
    l.vec_c = l.vec_y && (l.pitch_ca * l.bpp) % 16 == 0 && (l.pitch_cb * l.bpp) % 16 == 0;
    return l;
}

// the pointer tables of a launch into its kernel arguments
template <typename Args>
void copy_pairs(Args& k, int n, const void* const* a, const void* const* b) {
    k.n = n;
    for (int i = 0; i < n; i++) { k.a[i] = a[i]; k.b[i] = b[i]; }
}

// what every pair of a launch shares and the pointer tables, into the arguments of the error kernel or of the error map kernel; false: n
// out of range, or a frame beyond 2^32 work items
template <typename Args>
bool fill_error_args(Args& k, int hdr, int H, int W, int stride_a, int stride_b, bool planar, int n, const void* const* a, const void* const* b) {
    const FrameLayout l = frame_layout(hdr, H, W, stride_a, stride_b, planar, n, a, b);
    if (!l.ok) return false;
    const uint32_t EL = 16 / l.bpp;
    ErrorShape& s = k.sh;
    s.w_y = l.W; s.w_c = planar ? l.W / 2 : 2u * (l.W / 2);
    s.pitch_ya = l.pitch_ya; s.pitch_yb = l.pitch_yb; s.pitch_ca = l.pitch_ca; s.pitch_cb = l.pitch_cb;
    s.rows_u = l.H / 2;
    s.base_ca = l.base_ca; s.base_cb = l.base_cb; s.elems_a = l.elems_a; s.elems_b = l.elems_b;
    s.segs_y = (s.w_y + EL - 1) / EL; s.segs_c = (s.w_c + EL - 1) / EL;
    const uint64_t items_y = (uint64_t)l.H * s.segs_y, items_c = (uint64_t)l.rows_c * s.segs_c;
    if (items_y + (uint64_t)kErrMaxBlocks * kErrBlock >= (1ull << 32) || items_c + (uint64_t)kErrMaxBlocks * kErrBlock >= (1ull << 32)) return false;
    s.items_y = (uint32_t)items_y; s.items_c = (uint32_t)items_c;
    s.div_y = make_fastdiv(s.segs_y ? s.segs_y : 1u, items_y);
    s.div_c = make_fastdiv(s.segs_c ? s.segs_c : 1u, items_c);
    s.vec_y = l.vec_y; s.vec_c = l.vec_c;
    copy_pairs(k, n, a, b);
    return true;
}

// plane i of a frame (0 luma; 1 interleaved UV, or U; 2 V) as both SSIM kernels see it, and the channels of its rows; tiles_x and
// tile_first are the launcher's
SsimPlane ssim_plane(const FrameLayout& l, int i, uint32_t* ch) {
    const uint32_t w = i ? l.W / 2 : l.W, h = i ? l.H / 2 : l.H;
    *ch = i && !l.planar ? 2u : 1u;
    SsimPlane p{};
    p.bw = w >> 2; p.bh = h >> 2; p.w_row = w * *ch;
    p.pitch_a = i ? l.pitch_ca : l.pitch_ya; p.pitch_b = i ? l.pitch_cb : l.pitch_yb;
    p.base_a = i ? l.base_ca + (i == 2 ? (size_t)h * l.pitch_ca : 0) : 0;
    p.base_b = i ? l.base_cb + (i == 2 ? (size_t)h * l.pitch_cb : 0) : 0;
    p.vec = i ? l.vec_c : l.vec_y;
    return p;
}

// KERNEL<uint8_t | uint16_t, planar> of a launch
#define HF_METRIC_KERNEL(KERNEL, hdr, planar) \
    ((hdr) ? ((planar) ? KERNEL<uint16_t, true> : KERNEL<uint16_t, false>) : ((planar) ? KERNEL<uint8_t, true> : KERNEL<uint8_t, false>))

// the workgroups of `block` lanes that the whole device holds of this kernel at once: a launch whose workgroups stride over their pair's
// tiles wants no more (the rest would run in a second, mostly empty round).  Asked once per kernel (the same answer from every thread).
template <typename Args>
int resident_workgroups(void (*kernel)(const Args), int block, int hdr, bool planar) {
    static int resident[2][2];   // by kernel of this Args
    int& res = resident[hdr ? 1 : 0][planar ? 1 : 0];
    if (!res) {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 || cus < 1) { per_cu = 2; cus = 256; }
        res = per_cu * cus;
    }
    return res;
}

}  // namespace

bool launch_frame_errors(int hdr, int H, int W, int stride_a, int stride_b, bool planar, int n, const void* const* a, const void* const* b,
                         FrameErrorSlot* slots, hipStream_t stream) {
    ErrorArgs k{};
    if (!fill_error_args(k, hdr, H, W, stride_a, stride_b, planar, n, a, b)) return false;
    k.slots = slots;
    // around kErrMaxBlocks workgroups in the whole launch, one at least per pair
    const size_t most = k.sh.items_y > k.sh.items_c ? (size_t)k.sh.items_y : (size_t)k.sh.items_c;
    const size_t want = most ? (most + kErrBlock - 1) / kErrBlock : 1;
    const size_t cap = (size_t)kErrMaxBlocks / (size_t)n > 0 ? (size_t)kErrMaxBlocks / (size_t)n : 1;
    const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)n);
    HF_LAUNCH("frame_error", HF_METRIC_KERNEL(frame_error_kernel, hdr, planar), grid, dim3(kErrBlock), 0, stream, k);
    return true;
}

// one map per pair into maps[i][3][th][tw]; tile 16, 32 or 64; every entry is stored by the launch
bool launch_frame_error_map(int hdr, int H, int W, int stride_a, int stride_b, bool planar, int tile, int n, const void* const* a,
                            const void* const* b, void* maps, hipStream_t stream) {
    if (tile != 16 && tile != 32 && tile != 64) return false;
    MapArgs k{};
    if (!fill_error_args(k, hdr, H, W, stride_a, stride_b, planar, n, a, b)) return false;
    k.rows_y = (uint32_t)H;
    k.tile = (uint32_t)tile;
    const uint32_t across = (uint32_t)tile * (hdr ? 2u : 1u) / 16u;   // 1, 2, 4 or 8
    k.lg = across >= 8 ? 3u : across >= 4 ? 2u : across >= 2 ? 1u : 0u;
    k.tw = ((uint32_t)W + k.tile - 1) / k.tile; k.th = ((uint32_t)H + k.tile - 1) / k.tile;
    k.entries = (size_t)n * 3u * k.th * k.tw;
    k.maps = static_cast<TileSum*>(maps);
    // a workgroup per band, in the order of the bands in memory; a launch of more than kMapMaxBlocks workgroups strides over them
    const uint32_t cap = (uint32_t)kMapMaxBlocks / (uint32_t)n;
    const dim3 grid(k.th < cap ? k.th : cap, (unsigned)n);
    HF_LAUNCH("frame_error_map", HF_METRIC_KERNEL(frame_error_map_kernel, hdr, planar), grid, dim3(kMapBlock), 0, stream, k);
    return true;
}

bool launch_frame_ssim(int hdr, int H, int W, int stride_a, int stride_b, bool planar, long long c1, long long c2, int n, const void* const* a,
                       const void* const* b, FrameSsimSlot* slots, hipStream_t stream) {
    const FrameLayout l = frame_layout(hdr, H, W, stride_a, stride_b, planar, n, a, b);
    if (!l.ok) return false;
    SsimArgs k{};
    SsimShape& s = k.sh;
    for (int i = 0; i < (planar ? 3 : 2); i++) {   // (interleaved: V comes with U, pl[2] stays empty)
        uint32_t ch;
        SsimPlane& p = s.pl[i] = ssim_plane(l, i, &ch);
        const uint32_t per_tile_x = (uint32_t)(kSsimUnitsX - 1) * (16 / l.bpp / 4 / ch), per_tile_y = (uint32_t)(kSsimRows - 1);   // windows
        const bool any = p.bw > 1 && p.bh > 1;
        p.tiles_x = any ? (p.bw - 1 + per_tile_x - 1) / per_tile_x : 0;
        p.tile_first = s.tiles;
        s.tiles += any ? p.tiles_x * ((p.bh - 1 + per_tile_y - 1) / per_tile_y) : 0;
    }
    s.elems_a = l.elems_a; s.elems_b = l.elems_b;
    s.c1 = c1; s.c2 = c2;
    copy_pairs(k, n, a, b);
    k.slots = slots;
    void (*kernel)(const SsimArgs) = HF_METRIC_KERNEL(frame_ssim_kernel, hdr, planar);
    // as many workgroups in the whole launch as the device holds at once, one at least per pair (a frame without a window: its slot stays zero)
    const uint32_t res = (uint32_t)resident_workgroups(kernel, kSsimBlock, hdr, planar);
    const uint32_t cap = res / (uint32_t)n > 0 ? res / (uint32_t)n : 1u;
    const uint32_t want = s.tiles ? s.tiles : 1u;
    const dim3 grid(want < cap ? want : cap, (unsigned)n);
    if ((s.tiles + grid.x - 1) / grid.x >= kSsimMaxTilesPerWorkgroup) return false;   // (SsimLane; 2160p has 864 tiles)
    HF_LAUNCH("frame_ssim", kernel, grid, dim3(kSsimBlock), 0, stream, k);
    return true;
}

// one SSIM map per pair into maps[i][3][th][tw] of hf_ssim_tile; tile 16, 32 or 64; every entry is stored by the launch
bool launch_frame_ssim_map(int hdr, int H, int W, int stride_a, int stride_b, bool planar, long long c1, long long c2, int tile, int n,
                           const void* const* a, const void* const* b, void* maps, hipStream_t stream) {
    const FrameLayout l = frame_layout(hdr, H, W, stride_a, stride_b, planar, n, a, b);
    if (!l.ok || (tile != 16 && tile != 32 && tile != 64)) return false;
    SmapArgs k{};
    k.tw = ((uint32_t)W + (uint32_t)tile - 1) / (uint32_t)tile; k.th = ((uint32_t)H + (uint32_t)tile - 1) / (uint32_t)tile;
    for (int i = 0; i < (planar ? 3 : 2); i++) {
        uint32_t ch;
        SmapPlane& m = k.pl[i];
        SsimPlane& p = m.p = ssim_plane(l, i, &ch);
        const uint32_t bpu = 16 / l.bpp / 4 / ch;           // blocks of a channel in a unit: 1, 2 or 4
        m.tb = (uint32_t)(i ? tile / 2 : tile) / 4;         // 2 .. 16
        m.lg_tb = m.tb >= 16 ? 4u : m.tb >= 8 ? 3u : m.tb >= 4 ? 2u : 1u;
        m.halves = m.tb < bpu;                              // (tb 2, bpu 4)
        const uint32_t tu = m.halves ? 1u : m.tb / bpu;     // 1, 2, 4 or 8
        m.lg_tu = tu >= 8 ? 3u : tu >= 4 ? 2u : tu >= 2 ? 1u : 0u;
        m.pu = (uint32_t)kSmapOwn / tu * tu;
        const uint32_t tiles_across = m.halves ? 2u * m.pu : m.pu / tu, tiles_down = (uint32_t)kSmapRows / m.tb;
        p.tiles_x = (k.tw + tiles_across - 1) / tiles_across;
        p.tile_first = k.patches;
        k.patches += p.tiles_x * ((k.th + tiles_down - 1) / tiles_down);
    }
    if (!planar) { k.pl[2] = k.pl[1]; k.pl[2].p.tile_first = k.patches; }   // (no patch of its own: V comes with U)
    k.elems_a = l.elems_a; k.elems_b = l.elems_b;
    k.entries = (size_t)n * 3u * k.th * k.tw;
    k.c1 = c1; k.c2 = c2;
    copy_pairs(k, n, a, b);
    k.maps = static_cast<SsimTileOut*>(maps);
    void (*kernel)(const SmapArgs) = HF_METRIC_KERNEL(frame_ssim_map_kernel, hdr, planar);
    // as many workgroups in the whole launch as the device holds at once, one at least per pair: a workgroup strides over its pair's patches
    const uint32_t res = (uint32_t)resident_workgroups(kernel, kSmapBlock, hdr, planar);
    const uint32_t cap = res / (uint32_t)n > 0 ? res / (uint32_t)n : 1u;
    const dim3 grid(k.patches < cap ? k.patches : cap, (unsigned)n);
    HF_LAUNCH("frame_ssim_map", kernel, grid, dim3(kSmapBlock), 0, stream, k);
    return true;
}
#undef HF_METRIC_KERNEL

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

// what both enqueue calls refuse, each with nothing enqueued; n_slots: the public slot range named in the message
static int check_pairs(hf_ctx* c, const char* who, int n, const void* const* a, const void* const* b, int stride_a, int stride_b, int planar,
                       int first_slot, int max_slot, int n_slots) {
    if (!a || !b) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: null frame table", who);
    if (n < 1 || n > HF_MAX_ERROR_PAIRS) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: %d pairs, one launch takes 1 .. %d", who, n, HF_MAX_ERROR_PAIRS);
    if (first_slot < 0 || first_slot > max_slot - n) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: slots [%d, %d + %d) outside [0, %d)", who, first_slot, first_slot, n, n_slots);
    for (int i = 0; i < n; i++)
        if (!a[i] || !b[i]) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: null frame in pair %d", who, i);
    if (stride_a < c->g.W || stride_b < c->g.W) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: strides %d / %d below the frame width %d", who, stride_a, stride_b, c->g.W);
    if (planar && ((stride_a | stride_b) & 1)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: planar frames need even strides (%d / %d)", who, stride_a, stride_b);
    return HF_OK;
}

// the peak rule and the integer constants of the SSIM calls (hopperflow.h, step 3); refuses a peak outside its range
static int ssim_constants(hf_ctx* c, const char* who, int planar, int peak, long long* c1, long long* c2) {
    const int top = c->g.hdr ? 65535 : 255;
    if (peak < 0 || peak > top) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: peak %d outside 1 .. %d (0: the format's own)", who, peak, top);
    const long long pk = peak ? peak : !c->g.hdr ? 255 : planar ? 1023 : 65535;
    *c1 = (64 * pk * pk + 5000) / 10000; *c2 = (9 * 64 * 63 * pk * pk + 5000) / 10000;
    return HF_OK;
}

// The two families of result slots -- error sums, and the windowed SSIM of the same pairs in slots of its own -- go through ONE enqueue
// and ONE read.  A family: the context's buffer of n_slots public slots and one more for the blocking call, the read call's name, and
// whether a fresh buffer is zeroed whole (the SSIM slots: one never used reads as zeros; the error slots are not, as they never were).
template <typename Slot>
struct SlotFamily {
    DevBuf<Slot> hf_ctx::*buf;
    int n_slots;
    const char* read_name;
    bool zero_fresh;
};
static constexpr SlotFamily<hf::FrameErrorSlot> kErrorSlots{&hf_ctx::error_slots, HF_ERROR_SLOTS, "hf_frame_error_read", false};
static constexpr SlotFamily<hf::FrameSsimSlot> kSsimSlots{&hf_ctx::ssim_slots, HF_SSIM_SLOTS, "hf_frame_ssim_read", true};

// slots [first, first + n) zeroed, then pair i measured into slot first + i by launch(slots, c1, c2) -- behind everything the context has
// enqueued: warps on a second stream (HF_FLAG_DUAL_STREAM) are waited for like hf_download_frame_device does, a batch member issues on the
// batch's stream.  max_slot: n_slots for the public range, one more for the blocking call's own slot.  peak: of the SSIM calls, whose
// constants are settled between the checks of the pairs and the first use of the device; null for the error sums.
template <typename Slot, typename Launch>
static int enqueue_slots(hf_ctx* c, const SlotFamily<Slot>& fam, const char* who, int n, const void* const* a, const void* const* b, int stride_a,
                         int stride_b, int planar, const int* peak, int first_slot, int max_slot, Launch launch) {
    HF_CHECK_CTX(c);
    if (int rc = check_pairs(c, who, n, a, b, stride_a, stride_b, planar, first_slot, max_slot, fam.n_slots)) return rc;
    long long c1 = 0, c2 = 0;
    if (peak)
        if (int rc = ssim_constants(c, who, planar, *peak, &c1, &c2)) return rc;
    if (int rc = set_device(c)) return rc;
    DevBuf<Slot>& buf = c->*fam.buf;
    const size_t all = (size_t)(fam.n_slots + 1) * sizeof(Slot);
    const bool fresh = !buf;
    if (fresh) HF_HIP(c, alloc_device(buf, all));
    if (int rc = leave_warp_stream(c)) return rc;
    if (fresh && fam.zero_fresh) HF_HIP(c, hipMemsetAsync(buf.get(), 0, all, c->stream));
    Slot* slots = buf.get() + first_slot;
    HF_HIP(c, hipMemsetAsync(slots, 0, (size_t)n * sizeof(Slot), c->stream));
    if (!launch(slots, c1, c2)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: the frame is too large for one launch", who);
    HF_HIP(c, hipGetLastError());
    return HF_OK;
}

template <typename Slot, typename Out>
static int read_slots(hf_ctx* c, const SlotFamily<Slot>& fam, int first_slot, int n, int max_slot, Out* out) {
    static_assert(sizeof(Out) == sizeof(Slot), "a slot is its public struct");
    HF_CHECK_CTX(c);
    if (!out || n < 1 || first_slot < 0 || first_slot > max_slot - n)
        return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: slots [%d, %d + %d) outside [0, %d), or null", fam.read_name, first_slot, first_slot, n, fam.n_slots);
    if (!(c->*fam.buf)) return fail(c, HF_ERR_STATE, "%s: nothing was enqueued", fam.read_name);
    if (int rc = set_device(c)) return rc;
    if (int rc = leave_warp_stream(c)) return rc;
    HF_HIP(c, hipMemcpyAsync(out, (c->*fam.buf).get() + first_slot, (size_t)n * sizeof(Out), hipMemcpyDeviceToHost, c->stream));
    return sync_ctx(c);
}

static int enqueue_errors(hf_ctx* c, const char* who, int n, const void* const* a, const void* const* b, int stride_a, int stride_b, int planar,
                          int first_slot, int max_slot) {
    return enqueue_slots(c, kErrorSlots, who, n, a, b, stride_a, stride_b, planar, nullptr, first_slot, max_slot, [&](hf::FrameErrorSlot* slots, long long, long long) {
        return hf::launch_frame_errors(c->g.hdr, c->g.H, c->g.W, stride_a, stride_b, planar != 0, n, a, b, slots, c->stream);
    });
}

static int enqueue_ssim(hf_ctx* c, const char* who, int n, const void* const* a, const void* const* b, int stride_a, int stride_b, int planar, int peak,
                        int first_slot, int max_slot) {
    return enqueue_slots(c, kSsimSlots, who, n, a, b, stride_a, stride_b, planar, &peak, first_slot, max_slot, [&](hf::FrameSsimSlot* slots, long long c1, long long c2) {
        return hf::launch_frame_ssim(c->g.hdr, c->g.H, c->g.W, stride_a, stride_b, planar != 0, c1, c2, n, a, b, slots, c->stream);
    });
}

// The two kinds of per-tile maps share the tile grid; an entry is `entry` bytes
static int map_shape(const hf_ctx* c, int tile, size_t entry, int* tiles_x, int* tiles_y, size_t* bytes_per_map) {
    if (!c || !HF_ERROR_MAP_TILES_OK(tile)) return HF_ERR_INVALID_ARGUMENT;
    const int tw = (c->g.W + tile - 1) / tile, th = (c->g.H + tile - 1) / tile;
    if (tiles_x) *tiles_x = tw;
    if (tiles_y) *tiles_y = th;
    if (bytes_per_map) *bytes_per_map = 3 * entry * (size_t)tw * (size_t)th;
    return HF_OK;
}

// ... and one enqueue, ordered like enqueue_slots; no slots, no memset: launch(c1, c2) stores every entry of the caller's buffer
template <typename Launch>
static int enqueue_map(hf_ctx* c, const char* who, int n, const void* const* a, const void* const* b, int stride_a, int stride_b, int planar,
                       const int* peak, int tile, void* device_maps, Launch launch) {
    HF_CHECK_CTX(c);
    if (int rc = check_pairs(c, who, n, a, b, stride_a, stride_b, planar, 0, n, n)) return rc;
    long long c1 = 0, c2 = 0;
    if (peak)
        if (int rc = ssim_constants(c, who, planar, *peak, &c1, &c2)) return rc;
    if (!HF_ERROR_MAP_TILES_OK(tile)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: tile %d, not 16, 32 or 64", who, tile);
    if (!device_maps || ((uintptr_t)device_maps & 15u)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: the map buffer %p is null or not 16-byte aligned", who, device_maps);
    if (int rc = set_device(c)) return rc;
    if (int rc = leave_warp_stream(c)) return rc;
    if (!launch(c1, c2)) return fail(c, HF_ERR_INVALID_ARGUMENT, "%s: the frame is too large for one launch", who);
    HF_HIP(c, hipGetLastError());
    return HF_OK;
}

extern "C" {

int hf_frame_error_enqueue(hf_ctx* c, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b, int planar,
                           int first_slot) {
    return enqueue_errors(c, "hf_frame_error_enqueue", n, device_a, device_b, stride_a, stride_b, planar, first_slot, HF_ERROR_SLOTS);
}

int hf_frame_error_read(hf_ctx* c, int first_slot, int n, struct hf_frame_error* out) { return read_slots(c, kErrorSlots, first_slot, n, HF_ERROR_SLOTS, out); }

int hf_frame_error(hf_ctx* c, const void* device_a, const void* device_b, int stride_a, int stride_b, int planar, struct hf_frame_error* out) {
    HF_CHECK_CTX(c);
    if (!out) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_frame_error: null result");
    if (int rc = enqueue_errors(c, "hf_frame_error", 1, &device_a, &device_b, stride_a, stride_b, planar, HF_ERROR_SLOTS, HF_ERROR_SLOTS + 1)) return rc;
    return read_slots(c, kErrorSlots, HF_ERROR_SLOTS, 1, HF_ERROR_SLOTS + 1, out);
}

int hf_frame_error_map_shape(const hf_ctx* c, int tile, int* tiles_x, int* tiles_y, size_t* bytes_per_map) {
    return map_shape(c, tile, sizeof(struct hf_error_tile), tiles_x, tiles_y, bytes_per_map);
}

int hf_frame_error_map_enqueue(hf_ctx* c, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b, int planar,
                               int tile, void* device_maps) {
    return enqueue_map(c, "hf_frame_error_map_enqueue", n, device_a, device_b, stride_a, stride_b, planar, nullptr, tile, device_maps, [&](long long, long long) {
        return hf::launch_frame_error_map(c->g.hdr, c->g.H, c->g.W, stride_a, stride_b, planar != 0, tile, n, device_a, device_b, device_maps, c->stream);
    });
}

int hf_frame_ssim_enqueue(hf_ctx* c, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b, int planar,
                          int peak, int first_slot) {
    return enqueue_ssim(c, "hf_frame_ssim_enqueue", n, device_a, device_b, stride_a, stride_b, planar, peak, first_slot, HF_SSIM_SLOTS);
}

int hf_frame_ssim_read(hf_ctx* c, int first_slot, int n, struct hf_frame_ssim* out) { return read_slots(c, kSsimSlots, first_slot, n, HF_SSIM_SLOTS, out); }

int hf_frame_ssim(hf_ctx* c, const void* device_a, const void* device_b, int stride_a, int stride_b, int planar, int peak, struct hf_frame_ssim* out) {
    HF_CHECK_CTX(c);
    if (!out) return fail(c, HF_ERR_INVALID_ARGUMENT, "hf_frame_ssim: null result");
    if (int rc = enqueue_ssim(c, "hf_frame_ssim", 1, &device_a, &device_b, stride_a, stride_b, planar, peak, HF_SSIM_SLOTS, HF_SSIM_SLOTS + 1)) return rc;
    return read_slots(c, kSsimSlots, HF_SSIM_SLOTS, 1, HF_SSIM_SLOTS + 1, out);
}

int hf_frame_ssim_map_shape(const hf_ctx* c, int tile, int* tiles_x, int* tiles_y, size_t* bytes_per_map) {
    return map_shape(c, tile, sizeof(struct hf_ssim_tile), tiles_x, tiles_y, bytes_per_map);
}

int hf_frame_ssim_map_enqueue(hf_ctx* c, int n, const void* const* device_a, const void* const* device_b, int stride_a, int stride_b, int planar,
                              int peak, int tile, void* device_maps) {
    return enqueue_map(c, "hf_frame_ssim_map_enqueue", n, device_a, device_b, stride_a, stride_b, planar, &peak, tile, device_maps, [&](long long c1, long long c2) {
        return hf::launch_frame_ssim_map(c->g.hdr, c->g.H, c->g.W, stride_a, stride_b, planar != 0, c1, c2, tile, n, device_a, device_b, device_maps, c->stream);
    });
}

}  // extern "C"
