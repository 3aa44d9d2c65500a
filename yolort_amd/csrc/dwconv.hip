// Depthwise convolution y = act(dwconv(x, W) + bias) (+ res) for gfx950 (ymi_dwconv2d, include/yolort_amd.h): the kernel of DWConv, GhostConv, GhostBottleneck and
// C3Ghost (reference common.py:76-91, :378-416).  Every output channel reduces over the k x k taps of ONE input channel, so there is no GEMM here: an MFMA tile
// would multiply a diagonal.  NO MATRIX INSTRUCTIONS are used; the kernel is a streaming one (k * k multiply-adds per 2 bytes loaded) built so that every input byte
// is read from memory about once and every global access is 16 bytes.
//
// THE ARITHMETIC (the contract, restated from the header): products of the 16-bit operands in fp32 (exact), summed in fp32 in raster tap order (ky outer, kx inner)
// starting from +0; an out-of-image tap contributes x = 0 (for finite weights: the same as skipping it); then + fp32 bias, the activation, + the residual in fp32, ONE
// round-to-nearest-even to the storage type.  Each step is one fmaf(x, w, acc) on operands converted to fp32 -- the product is exact, so this IS product-then-add; for
// fp16 the compiler folds the conversions into v_fma_mix_f32 (fp32 arithmetic on 16-bit sources).  No fp16 accumulation, no packed-half math.
//
// WORK SPLIT.  A workgroup of 256 threads owns TH x TW output pixels x a slab of 64 channels (128 bytes per pixel: one full line per row of 8 lanes); grid =
// (tiles, slabs, images), so 20 x 20 x 256 at 32 images is 6 x 4 x 32 = 768 workgroups.  Stride 1: 8 x 16 outputs, stride 2: 8 x 8 (the squarer input halo).
// A thread owns 8 adjacent channels (lane & 7: one 16-byte packet) of RUN vertically adjacent outputs of one column (RUN = 4 / 2).
// DATA FLOW.  (1) The input halo tile ((TH-1)s + k) x ((TW-1)s + k) x 64 channels goes to LDS with 16-byte loads, ZEROS for out-of-image pixels and for channels past
// c (a partial last slab), so the tap loop has no bounds checks; the slab's weights go to LDS as [tap][64].  (2) A thread walks its input rows top to bottom: the k
// packets of a row are read from LDS ONCE into registers and feed every output of the run whose window holds that row (a sliding window: each output still sees its
// taps in raster order), each tap's weights being one 16-byte LDS read shared by all lanes of the same channel group.  (3) Epilogue in registers, one 16-byte store.
// LDS BANKS.  The 8 lanes of a pixel read 128 contiguous bytes and, at stride 1, the 8 pixels of a wave 1 KiB contiguous.  At stride 2 neighbouring outputs are 256
// bytes apart -- the same half of the banks -- so pixel slot p is stored at p ^ ((p >> 1) & 1): neighbours alternate between the two halves.
// LDS BYTES: k5 s1 12 x 20 x 128 + 25 x 128 = 33.1 KiB, k3 s1 22.4 KiB, k5 s2 48.6 KiB, k3 s2 37.4 KiB: three to seven workgroups per CU.
#include "conv_common.hpp"

namespace ymi {

constexpr int DW_SLAB = 64;   // channels per workgroup

template <int K, int S>
struct DwTile {
    static constexpr int TH = YMI_DWCONV_TILE_H, TW = S == 1 ? YMI_DWCONV_TILE_W_S1 : YMI_DWCONV_TILE_W_S2;
    static constexpr int RG = 256 / (8 * TW), RUN = TH / RG;        // row groups of the workgroup, outputs per thread
    static constexpr int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;   // input halo tile
    static constexpr int ROWS = (RUN - 1) * S + K;                  // input rows one thread walks
    static constexpr int NPIX = (IH * IW + 3) / 4 * 4;              // slots (the stride-2 swizzle permutes inside groups of four)
    static_assert(RG * RUN == TH && RG * 8 * TW == 256, "tile does not divide the workgroup");
};

template <int S>
__device__ __forceinline__ int dw_slot(int p) {
    if constexpr (S == 2) return p ^ ((p >> 1) & 1);
    else return p;
}

// acc[0..7] += x[0..7] * w[0..7], 16-bit operands converted to fp32, one fmaf each
template <int DT>
__device__ __forceinline__ void dw_fma8(float (&acc)[8], const u32x4& x, const u32x4& w) {
    if constexpr (DT == YMI_F16) {
        const f16x8 xh = __builtin_bit_cast(f16x8, x), wh = __builtin_bit_cast(f16x8, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf((float)xh[i], (float)wh[i], acc[i]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[2 * q] = __builtin_fmaf(__uint_as_float(x[q] << 16), __uint_as_float(w[q] << 16), acc[2 * q]);
            acc[2 * q + 1] = __builtin_fmaf(__uint_as_float(x[q] & 0xffff0000u), __uint_as_float(w[q] & 0xffff0000u), acc[2 * q + 1]);
        }
    }
}

struct DwArgs {
    const uint16_t* x;
    const uint16_t* w;
    const float* bias;
    uint16_t* y;
    const uint16_t* res;
    int h, w_in, c, x_cs, ho, wo, y_cs, res_cs, act, tiles_x;
};

template <int DT, int K, int S>
__global__ __launch_bounds__(256) void dwconv_kernel(const DwArgs a) {
    using T = DwTile<K, S>;
    constexpr int P = K / 2;
    __shared__ __attribute__((aligned(16))) u32x4 sx[T::NPIX * 8];   // [slot][channel group]
    __shared__ __attribute__((aligned(16))) u32x4 sw[K * K * 8];     // [tap][channel group]
    const int tid = threadIdx.x;
    const int ty0 = (blockIdx.x / a.tiles_x) * T::TH, tx0 = (blockIdx.x % a.tiles_x) * T::TW;
    const int c0 = blockIdx.y * DW_SLAB, img = blockIdx.z;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    // (1) stage the halo tile and the weights: chunk i = (pixel i / 8, channel group i % 8)
    const int iy0 = ty0 * S - P, ix0 = tx0 * S - P;
    const uint16_t* ximg = a.x + (int64_t)img * a.h * a.w_in * a.x_cs + c0;
    constexpr int NCH = T::IH * T::IW * 8;
#pragma unroll
    for (int i0 = 0; i0 < NCH; i0 += 256) {
        const int i = i0 + tid;
        if (i < NCH) {
            const int p = i >> 3, g = i & 7;
            const int py = p / T::IW, px = p - py * T::IW;
            const int gy = iy0 + py, gx = ix0 + px;
            u32x4 v = zero;
            if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w_in && c0 + g * 8 < a.c)
                v = *reinterpret_cast<const u32x4*>(ximg + ((int64_t)gy * a.w_in + gx) * a.x_cs + g * 8);
            sx[dw_slot<S>(p) * 8 + g] = v;
        }
    }
    if (tid < K * K * 8) {
        const int tap = tid >> 3, g = tid & 7;
        sw[tid] = c0 + g * 8 < a.c ? *reinterpret_cast<const u32x4*>(a.w + (int64_t)tap * a.c + c0 + g * 8) : zero;
    }
    __syncthreads();

    // (2) the sliding window: input row j of the thread's column feeds output r through tap row ky = j - r * S
    const int g = tid & 7, col = (tid >> 3) % T::TW, rg = (tid >> 3) / T::TW;
    float acc[T::RUN][8];
#pragma unroll
    for (int r = 0; r < T::RUN; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[r][i] = 0.0f;
    const int pbase = rg * T::RUN * S * T::IW + col * S;
    // (the row loop is a real loop: unrolled, the compiler merges the repeated reads of a tap's weights and keeps all k * k packets in registers -- 100 VGPRs for
    // k = 5, 256 + AGPR copies in all, one wave per SIMD; rolled, a wave holds the run's accumulators, one input row and the weights in flight)
#pragma unroll 1
    for (int j = 0; j < T::ROWS; ++j) {
        u32x4 xr[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) xr[kx] = sx[dw_slot<S>(pbase + j * T::IW + kx) * 8 + g];
#pragma unroll
        for (int r = 0; r < T::RUN; ++r) {
            const int ky = j - r * S;   // wave-uniform
            if (ky >= 0 && ky < K) {
                const u32x4* wrow = sw + ky * K * 8 + g;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) dw_fma8<DT>(acc[r], xr[kx], wrow[kx * 8]);
            }
        }
    }

    // (3) bias, activation, residual, one rounding, one 16-byte store
    const int ox = tx0 + col, cc = c0 + g * 8;
    if (ox >= a.wo || cc >= a.c) return;
    float bb[8];
    *reinterpret_cast<f32x4*>(bb) = *reinterpret_cast<const f32x4*>(a.bias + cc);
    *reinterpret_cast<f32x4*>(bb + 4) = *reinterpret_cast<const f32x4*>(a.bias + cc + 4);
#pragma unroll
    for (int r = 0; r < T::RUN; ++r) {
        const int oy = ty0 + rg * T::RUN + r;
        if (oy >= a.ho) break;
        const int64_t pix = ((int64_t)img * a.ho + oy) * a.wo + ox;
        u32x4 rv = zero;
        if (a.res != nullptr) rv = *reinterpret_cast<const u32x4*>(a.res + pix * a.res_cs + cc);
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x2 v = {acc[r][2 * q] + bb[2 * q], acc[r][2 * q + 1] + bb[2 * q + 1]};
            if (a.act == YMI_ACT_SILU) {
                v[0] = silu<DT>(v[0]);
                v[1] = silu<DT>(v[1]);
            } else if (a.act != YMI_ACT_NONE) {
                v[0] = act_legacy_f32(v[0], a.act);
                v[1] = act_legacy_f32(v[1], a.act);
            }
            if (a.res != nullptr) {
                v[0] += from16<DT>((uint16_t)(rv[q] & 0xffff));
                v[1] += from16<DT>((uint16_t)(rv[q] >> 16));
            }
            o[q] = cvt_pk16<DT>(v);
        }
        *reinterpret_cast<u32x4*>(a.y + pix * a.y_cs + cc) = o;
    }
}

template <int DT, int K, int S>
static int dwconv_launch_one(const DwArgs& a, int n, hipStream_t s) {
    using T = DwTile<K, S>;
    DwArgs b = a;
    b.tiles_x = cdiv(a.wo, T::TW);
    const dim3 grid((unsigned)(b.tiles_x * cdiv(a.ho, T::TH)), (unsigned)cdiv(a.c, DW_SLAB), (unsigned)n);
    hipLaunchKernelGGL((dwconv_kernel<DT, K, S>), grid, dim3(256), 0, s, b);
    return check_launch("dwconv_kernel");
}

int dwconv_check(const ymi_dwconv_desc* d) {
    YMI_REQUIRE(d != nullptr, "ymi_dwconv2d: null descriptor");
    YMI_REQUIRE(d->x && d->w && d->bias && d->y, "ymi_dwconv2d: null x / w / bias / y");
    YMI_REQUIRE(d->dtype == YMI_F16 || d->dtype == YMI_BF16, "ymi_dwconv2d: dtype must be F16 or BF16 (got %d; the fp32 parity mode has no depthwise kernel)", d->dtype);
    YMI_REQUIRE((d->k == 3 || d->k == 5) && (d->s == 1 || d->s == 2) && d->p == d->k / 2, "ymi_dwconv2d: k in {3, 5}, s in {1, 2}, p = k / 2 (got k %d s %d p %d)", d->k, d->s, d->p);
    YMI_REQUIRE(d->c > 0 && d->c % 8 == 0, "ymi_dwconv2d: c must be a positive multiple of 8 (got %d)", d->c);
    YMI_REQUIRE(d->x_cstride >= d->c && d->y_cstride >= d->c && d->x_cstride % 8 == 0 && d->y_cstride % 8 == 0 && (d->res == nullptr || (d->res_cstride >= d->c && d->res_cstride % 8 == 0)),
                "ymi_dwconv2d: channel strides must be multiples of 8 and >= c (x %d y %d res %d, c %d)", d->x_cstride, d->y_cstride, d->res_cstride, d->c);
    YMI_REQUIRE(d->n >= 0 && d->n <= 65535 && d->h >= 1 && d->w_in >= 1, "ymi_dwconv2d: bad extent n %d h %d w %d (n <= 65535)", d->n, d->h, d->w_in);
    YMI_REQUIRE(d->ho == (d->h + 2 * d->p - d->k) / d->s + 1 && d->wo == (d->w_in + 2 * d->p - d->k) / d->s + 1, "ymi_dwconv2d: output size %d x %d does not follow from the input's (%d x %d, k %d s %d)",
                d->ho, d->wo, d->h, d->w_in, d->k, d->s);
    YMI_REQUIRE(d->act >= YMI_ACT_NONE && d->act <= YMI_ACT_LEAKY, "ymi_dwconv2d: unknown activation %d", d->act);
    YMI_REQUIRE(((uintptr_t)d->x | (uintptr_t)d->w | (uintptr_t)d->bias | (uintptr_t)d->y | (uintptr_t)d->res) % 16 == 0, "ymi_dwconv2d: pointers must be 16-byte aligned");
    YMI_REQUIRE((int64_t)d->ho * d->wo < ((int64_t)1 << 31) / 256, "ymi_dwconv2d: output map too large");
    return YMI_OK;
}

int dwconv_launch(const ymi_dwconv_desc* d, hipStream_t s) {
    if (const int rc = dwconv_check(d)) return rc;
    if (d->n == 0) return YMI_OK;
    DwArgs a;
    a.x = (const uint16_t*)d->x; a.w = (const uint16_t*)d->w; a.bias = d->bias; a.y = (uint16_t*)d->y; a.res = (const uint16_t*)d->res;
    a.h = d->h; a.w_in = d->w_in; a.c = d->c; a.x_cs = d->x_cstride; a.ho = d->ho; a.wo = d->wo; a.y_cs = d->y_cstride; a.res_cs = d->res_cstride; a.act = d->act; a.tiles_x = 0;
    const int key = (d->dtype == YMI_BF16 ? 4 : 0) | (d->k == 5 ? 2 : 0) | (d->s == 2 ? 1 : 0);
    switch (key) {
        case 0: return dwconv_launch_one<YMI_F16, 3, 1>(a, d->n, s);
        case 1: return dwconv_launch_one<YMI_F16, 3, 2>(a, d->n, s);
        case 2: return dwconv_launch_one<YMI_F16, 5, 1>(a, d->n, s);
        case 3: return dwconv_launch_one<YMI_F16, 5, 2>(a, d->n, s);
        case 4: return dwconv_launch_one<YMI_BF16, 3, 1>(a, d->n, s);
        case 5: return dwconv_launch_one<YMI_BF16, 3, 2>(a, d->n, s);
        case 6: return dwconv_launch_one<YMI_BF16, 5, 1>(a, d->n, s);
        default: return dwconv_launch_one<YMI_BF16, 5, 2>(a, d->n, s);
    }
}

}  // namespace ymi

extern "C" int ymi_dwconv2d(const ymi_dwconv_desc* d, void* stream) { return ymi::dwconv_launch(d, (hipStream_t)stream); }
