// fp32 convolution on the 16-bit matrix pipe: split-bf16 arithmetic on fp32 storage (gfx950) -- tiles 211-216 (NP = 6 products) and 221-226 (NP = 8), the opt-in fast form
// of the fp32 mode (engine.Plan: YOLORT_AMD_F32_SPLIT=6 / 8).
//
// v_mfma_f32_32x32x2_f32 is the ceiling of tiles 201-206 (conv_f32_pipe.hip: 0.53 MFMA-busy of 157 TFLOP/s); v_mfma_f32_32x32x16_bf16 retires 16 times the k per instruction.
// Storage, operand movement, the three operand forms, ConvArgs, the two-level summation and the epilogue are those of conv_f32_pipe_kernel -- the SAME kernel template
// (conv_f32_ring.hpp), instantiated with another arithmetic for one 16-deep step:
//   * a lane below 32 reads k 0..7 of its row (two ds_read_b128: chunks 0, 1), a lane from 32 up k 8..15 (chunks 2, 3): the fragment v_mfma_f32_32x32x16_bf16 takes, for
//     both operands by the same mapping -- no permlane32_swap;
//   * every fp32 operand x is split in registers, round-to-nearest-even, into hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): both subtractions are exact in fp32
//     and hi + mid + lo == x (include/yolort_amd.h, "fp32 mode on the 16-bit matrix pipe", derives this and the error contract).  A pair of values costs three
//     v_cvt_pk_bf16_f32, four shifts / masks and four subtractions: 5.5 VALU instructions per element;
//   * the weight fragments of a step are split once and reused by the wave's M tiles; all fragments are split before the step's first MFMA, so that the MFMAs of a step
//     form one uninterrupted stream and the other resident waves' splits run under it (two blocks per CU = two waves per SIMD);
//   * products, smallest first, into the tile's `part` accumulator (w-term . x-term): [lo.mid, mid.lo,] lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi.  NP = 6 drops
//     lo.mid, mid.lo and lo.lo (<= (2^-23 + 2^-32) |x||w| per product), NP = 8 drops lo.lo only (<= 2^-32 |x||w|).  Every bf16 x bf16 product is exact in fp32;
//   * the product loop is outermost, the tiles inner: consecutive MFMAs write different accumulators (TM x TN independent chains).
// Pre-split weights (hi / mid / lo planes packed on the host) would halve the VALU work; they need a new packing and are left out here.
#include "conv_f32_ring.hpp"

namespace ymi {

struct Bf16x3 { bf16x8 hi, mid, lo; };

// eight consecutive k of one row (two ds_read_b128) -> three bf16 fragments, element e of each = term of k e
__device__ __forceinline__ Bf16x3 split_bf16x3(const f32x4& k03, const f32x4& k47) {
    u32x4 h, m, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2 x = q < 2 ? f32x2{k03[2 * q], k03[2 * q + 1]} : f32x2{k47[2 * q - 4], k47[2 * q - 3]};
        h[q] = cvt_pk16<YMI_BF16>(x);                                                                  // v_cvt_pk_bf16_f32: element 0 in the low half
        const f32x2 r = {x[0] - __uint_as_float(h[q] << 16), x[1] - __uint_as_float(h[q] & 0xffff0000u)};   // exact: at most 16 significant bits
        m[q] = cvt_pk16<YMI_BF16>(r);
        const f32x2 t = {r[0] - __uint_as_float(m[q] << 16), r[1] - __uint_as_float(m[q] & 0xffff0000u)};   // exact: at most 8 significant bits, so lo is exact too
        l[q] = cvt_pk16<YMI_BF16>(t);
    }
    Bf16x3 o;
    __builtin_memcpy(&o.hi, &h, 16);
    __builtin_memcpy(&o.mid, &m, 16);
    __builtin_memcpy(&o.lo, &l, 16);
    return o;
}

template <int NP>
struct SplitBf16Math {
    static_assert(NP == 6 || NP == 8, "6 products (lo.mid, mid.lo, lo.lo dropped) or 8 (lo.lo dropped)");
    struct Pos { int p0, p1; };   // byte offsets of k-chunks 2 hi and 2 hi + 1 within a row
    static __device__ __forceinline__ Pos positions(int hi, int swz) { return {((2 * hi) ^ swz) * 16, ((2 * hi + 1) ^ swz) * 16}; }

    template <int TM, int TN>
    static __device__ __forceinline__ void step(const unsigned char* as, const unsigned char* ws, int frow, Pos p, f32x16 (&part)[TN][TM]) {
        Bf16x3 wf[TN], af[TM];
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const unsigned char* row = ws + (i * 32 + frow) * 64;
            wf[i] = split_bf16x3(*reinterpret_cast<const f32x4*>(row + p.p0), *reinterpret_cast<const f32x4*>(row + p.p1));
        }
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const unsigned char* row = as + (j * 32 + frow) * 64;
            af[j] = split_bf16x3(*reinterpret_cast<const f32x4*>(row + p.p0), *reinterpret_cast<const f32x4*>(row + p.p1));
        }
        // term of w, term of x (0 = hi, 1 = mid, 2 = lo), smallest products first; NP = 6 starts at the third
        constexpr int TW[8] = {2, 1, 2, 0, 1, 1, 0, 0}, TX[8] = {1, 2, 0, 2, 1, 0, 1, 0};
        auto term = [](const Bf16x3& f, int t) -> const bf16x8& { return t == 0 ? f.hi : (t == 1 ? f.mid : f.lo); };
#pragma unroll
        for (int q = 8 - NP; q < 8; ++q)
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(term(wf[i], TW[q]), term(af[j], TX[q]), part[i][j], 0, 0, 0);
    }
};

template <int BM, int BN, int WM, int WN, int STAGES, int MODE, int NP>
constexpr auto conv_f32_split_kernel = conv_f32_pipe_kernel<BM, BN, WM, WN, STAGES, MODE, SplitBf16Math<NP>>;

template <int BM, int BN, int WM, int WN, int STAGES, int NP>
static int launch_f32_split(const ConvArgs& a, bool is1x1, hipStream_t s) {
    return launch_f32_ring<BM, BN, STAGES>(a, is1x1, s, "conv_f32_split_kernel", [](int mode) -> void (*)(const ConvArgs) {
        if (mode == 1) return conv_f32_split_kernel<BM, BN, WM, WN, STAGES, 1, NP>;
        if (mode == 2) return conv_f32_split_kernel<BM, BN, WM, WN, STAGES, 2, NP>;
        return conv_f32_split_kernel<BM, BN, WM, WN, STAGES, 0, NP>;
    });
}

template <int NP>
static int launch_f32_split_tile(const ConvArgs& a, bool is1x1, int geometry, hipStream_t s) {
    switch (geometry) {   // the block and wave tiles of 201-206
        case 1: return launch_f32_split<128, 128, 64, 64, 3, NP>(a, is1x1, s);
        case 2: return launch_f32_split<128, 64, 64, 32, 3, NP>(a, is1x1, s);
        case 3: return launch_f32_split<64, 64, 32, 32, 3, NP>(a, is1x1, s);
        case 4: return launch_f32_split<256, 64, 64, 64, 3, NP>(a, is1x1, s);
        case 5: return launch_f32_split<256, 32, 64, 32, 3, NP>(a, is1x1, s);
        default: return launch_f32_split<128, 32, 32, 32, 3, NP>(a, is1x1, s);
    }
}

// tiles 211-216 (NP = 6) / 221-226 (NP = 8): the checks of the matching 20x tile, then its geometry
int conv_f32_split_launch(const ConvArgs& a0, bool is1x1, int tile, hipStream_t s) {
    const int np = tile / 10 == 21 ? 6 : (tile / 10 == 22 ? 8 : 0), geometry = tile % 10;
    if (np == 0 || geometry < 1 || geometry > 6) {
        set_error("ymi_conv2d (fp32): unknown split-bf16 tile id %d (211-216: 6 products, 221-226: 8 products)", tile);
        return YMI_EINVAL;
    }
    ConvArgs a = a0;
    { const int rc = conv_f32_ring_prepare(a); if (rc != YMI_OK) return rc; }
    return np == 6 ? launch_f32_split_tile<6>(a, is1x1, geometry, s) : launch_f32_split_tile<8>(a, is1x1, geometry, s);
}

}  // namespace ymi
