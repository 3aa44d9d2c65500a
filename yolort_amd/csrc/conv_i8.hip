// INT8 convolution with a requantising epilogue, and the quantise kernel that produces its input, for gfx950 (ymi_conv2d_i8 / ymi_quantize_i8, include/yolort_amd.h).
//     y = requant(act(float(acc) * scale[co] + bias[co]) + res_scale * res),   acc = exact int32 sum of int8 products (v_mfma_i32_32x32x32_i8)
//
// THE PRODUCT RUNS TRANSPOSED: D[co][pixel] = sum_k W[co][k] X[pixel][k].  Output channels lie along the instruction's M (the A operand is the WEIGHTS), pixels along N
// (the B operand is the ACTIVATIONS).  Lane l = 32 g + i (g = l / 32, i = l % 32) supplies 16 bytes of row i of A and 16 bytes of column i of B for the K half g, and
// receives, in accumulator register r, D[8 (r / 4) + 4 g + r % 4][i]: four runs of FOUR CONSECUTIVE OUTPUT CHANNELS of ONE pixel.  An int8 result is therefore one
// packed 32-bit store per run and a 16-bit result one 64-bit store; no LDS transpose on either side of the product.
// K ORDER.  Which of the instruction's 32 k indices a lane's byte j stands for does not matter to a dot product as long as A's and B's lanes of the same K half g agree
// on it -- and they do by construction: byte j of half g is input channel 16 (2 q + g) + j of one tap in BOTH operands (the weight blob is packed that way, the
// activation packet is 16 consecutive channels of one pixel).  The exact-value tests carry a distinct weight per (co, ci, tap) and pin it.
//
// OPERANDS.  cin % 16 == 0, so a lane's B fragment is ONE aligned 16-byte load: 16 consecutive channels ("a packet") of one pixel at one tap -- no im2col table.  The
// weights are packed at pack time in fragment order [tap][packet (padded to even)][cout (padded to 32)][16 bytes] (conv_i8_pack below), so a lane's A fragment is one
// 16-byte read and 32 lanes read 512 contiguous bytes.  A k32 step consumes packets 2 q and 2 q + 1; an odd packet count ends in a step whose second half is zero
// weights against zero activations.
// WORK SPLIT.  A workgroup of four waves owns 128 output pixels x a slab of 64 output channels (two 32 x 32 accumulator tiles per wave; a slab whose second half lies
// past cout runs one).  Every wave owns 32 pixels and all of the slab, so the slab's weights are shared by the four waves through LDS.
//   k = 3 (conv_i8_k3_kernel): the pixels are an 8 x 16 spatial tile of one image, wave w rows 2 w and 2 w + 1.  Per chunk of 32 input channels the input HALO tile
//     ((8 - 1) s + 3) x ((16 - 1) s + 3) pixels x 32 bytes is staged in LDS with 16-byte loads, ZEROS outside the image, and all nine taps read it; the chunk's weights
//     [9 taps][2][64][16] (18 KiB) sit beside it.  LDS: 23.6 KiB at stride 1, 35.5 KiB at stride 2.
//   k = 1 (conv_i8_k1_kernel): the pixels are 128 consecutive ones of the (n, ho, wo) raster (a tile may span images); the activations go STRAIGHT TO REGISTERS, four
//     k32 steps (128 channels) per chunk, and only the weights [8 packets][64][16] (8 KiB) pass through LDS.
// PIPELINE.  One LDS buffer, register-staged: the global loads of chunk c + 1 are issued before the MFMAs of chunk c and written to LDS after them, so they are in
// flight under the matrix work (two barriers per chunk).
// EPILOGUE (conv_i8_epilogue): the contract's six steps in registers -- (float)acc, ONE fmaf with scale / bias, the activation (silu<> / act_legacy_f32 of the other
// epilogues), ONE fmaf with the shortcut, ONE rounding -- and plain vector stores of words built in C++.  No atomics.
#include <string.h>

#include "conv_common.hpp"

namespace ymi {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int Q_SLAB = 64;            // output channels per workgroup
constexpr int Q_TH = 8, Q_TW = 16;    // k = 3: output tile of a workgroup (4 waves x 2 rows x 16 columns)
constexpr int Q_PIX = 128;            // k = 1: output pixels per workgroup
constexpr int Q_K1_STEPS = 4;         // k = 1: k32 steps per weight chunk

struct QArgs {
    const int8_t* x;
    const int8_t* w;
    const float* scale;
    const float* bias;
    void* y;
    const void* res;
    int n, h, w_in, cin, x_cs, ho, wo, cout, cout_pad, y_cs, res_cs, s, act;
    int P, P2;          // 16-channel packets per tap, rounded up to even
    int tiles_x, M;     // k = 3: tiles per row of tiles;  k = 1: n * ho * wo
    float inv_out, res_scale;
};

__device__ __forceinline__ i32x16 q_mfma(const u32x4& a, const u32x4& b, const i32x16& c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
}

// the final rounding to an int8 code: rint (ties to even) of v * inv, clamped to +-127; NaN -> 0
__device__ __forceinline__ int q_code(float v, float inv) {
    const float q = __builtin_rintf(v * inv);
    return q == q ? (int)fminf(fmaxf(q, -127.0f), 127.0f) : 0;   // (fmaxf would turn a NaN into -127: the test comes first)
}

// steps 2 .. 6 of the contract for the lane's accumulators: pixel `pix` (index into the (n, ho, wo) raster), channels co0 + 32 t + 8 j + 4 g + [0, 4)
template <int OUT>
__device__ __forceinline__ void conv_i8_epilogue(const QArgs& a, const i32x16 (&acc)[2], int nt, int64_t pix, int co0, int g) {
    constexpr int SDT = OUT == YMI_BF16 ? YMI_BF16 : YMI_F16;   // which form of silu<>
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (t >= nt) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + 32 * t + 8 * j + 4 * g;
            if (co >= a.cout) continue;   // cout % 8 == 0: a run of four is inside or outside as a whole
            const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + co), bi = *reinterpret_cast<const f32x4*>(a.bias + co);
            float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.res != nullptr) {
                if constexpr (OUT == YMI_I8) {
                    const uint32_t rw = *reinterpret_cast<const uint32_t*>((const int8_t*)a.res + pix * a.res_cs + co);
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = (float)(int8_t)(rw >> (8 * e));
                } else {
                    const u32x2 rw = *reinterpret_cast<const u32x2*>((const uint16_t*)a.res + pix * a.res_cs + co);
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = from16<OUT>((uint16_t)(rw[e >> 1] >> (16 * (e & 1))));
                }
            }
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float f = __builtin_fmaf((float)acc[t][4 * j + e], sc[e], bi[e]);
                if (a.act == YMI_ACT_SILU) f = silu<SDT>(f);
                else if (a.act != YMI_ACT_NONE) f = act_legacy_f32(f, a.act);
                if (a.res != nullptr) f = __builtin_fmaf(r[e], a.res_scale, f);
                v[e] = f;
            }
            if constexpr (OUT == YMI_I8) {
                uint32_t o = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) o |= ((uint32_t)q_code(v[e], a.inv_out) & 0xffu) << (8 * e);
                *reinterpret_cast<uint32_t*>((int8_t*)a.y + pix * a.y_cs + co) = o;
            } else {
                const f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
                const u32x2 o = {cvt_pk16<OUT>(lo), cvt_pk16<OUT>(hi)};
                *reinterpret_cast<u32x2*>((uint16_t*)a.y + pix * a.y_cs + co) = o;
            }
        }
    }
}

// ---- k = 3 ----
template <int S>
struct QTile {
    static constexpr int IH = (Q_TH - 1) * S + 3, IW = (Q_TW - 1) * S + 3;   // input halo tile
    static constexpr int NX = IH * IW * 2;                                    // 16-byte chunks of one staged channel chunk: [pixel][K half]
    static constexpr int NW = 9 * 2 * Q_SLAB;                                 // [tap][K half][co]
    static constexpr int RX = (NX + 255) / 256, RW = (NW + 255) / 256;       // prefetch registers (x 4 dwords) per thread
};

template <int S, int OUT>
__global__ __launch_bounds__(256) void conv_i8_k3_kernel(const QArgs a) {
    using T = QTile<S>;
    __shared__ __attribute__((aligned(16))) u32x4 sx[T::NX];
    __shared__ __attribute__((aligned(16))) u32x4 sw[T::NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, g = lane >> 5;
    const int ty0 = (blockIdx.x / a.tiles_x) * Q_TH, tx0 = (blockIdx.x % a.tiles_x) * Q_TW;
    const int co0 = blockIdx.y * Q_SLAB, img = blockIdx.z;
    const int nt = a.cout - co0 > 32 ? 2 : 1;
    const int iy0 = ty0 * S - 1, ix0 = tx0 * S - 1;
    const int8_t* ximg = a.x + (int64_t)img * a.h * a.w_in * a.x_cs;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 px[T::RX], pw[T::RW];

    // global -> registers of channel chunk c (packets 2 c and 2 c + 1): zeros outside the image, past the last packet and past the padded cout
    auto fetch = [&](int c) {
#pragma unroll
        for (int r = 0; r < T::RX; ++r) {
            const int e = r * 256 + tid;
            u32x4 v = zero;
            if (e < T::NX) {
                const int p = e >> 1, pk = 2 * c + (e & 1);
                const int py = p / T::IW, gy = iy0 + py, gx = ix0 + (p - py * T::IW);
                if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w_in && pk < a.P)
                    v = *reinterpret_cast<const u32x4*>(ximg + ((int64_t)gy * a.w_in + gx) * a.x_cs + pk * 16);
            }
            px[r] = v;
        }
#pragma unroll
        for (int r = 0; r < T::RW; ++r) {
            const int e = r * 256 + tid;
            u32x4 v = zero;
            if (e < T::NW) {
                const int tap = e >> 7, pk = 2 * c + ((e >> 6) & 1), co = co0 + (e & 63);
                if (co < a.cout_pad) v = *reinterpret_cast<const u32x4*>(a.w + (((int64_t)tap * a.P2 + pk) * a.cout_pad + co) * 16);
            }
            pw[r] = v;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int r = 0; r < T::RX; ++r)
            if (r * 256 + tid < T::NX) sx[r * 256 + tid] = px[r];
#pragma unroll
        for (int r = 0; r < T::RW; ++r)
            if (r * 256 + tid < T::NW) sw[r * 256 + tid] = pw[r];
    };

    i32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0;
    const int row = 2 * wave + (i >> 4), col = i & 15;
    const int xbase = ((row * S) * T::IW + col * S) * 2 + g;
    const int nch = a.P2 >> 1;
    fetch(0);
    stash();
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) fetch(c + 1);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const u32x4 b = sx[xbase + ((tap / 3) * T::IW + tap % 3) * 2];
            acc[0] = q_mfma(sw[(tap * 2 + g) * Q_SLAB + i], b, acc[0]);
            if (nt == 2) acc[1] = q_mfma(sw[(tap * 2 + g) * Q_SLAB + 32 + i], b, acc[1]);
        }
        __syncthreads();
        if (c + 1 < nch) {
            stash();
            __syncthreads();
        }
    }
    const int oy = ty0 + row, ox = tx0 + col;
    if (oy < a.ho && ox < a.wo) conv_i8_epilogue<OUT>(a, acc, nt, ((int64_t)img * a.ho + oy) * a.wo + ox, co0, g);
}

// ---- k = 1 ----
template <int OUT>
__global__ __launch_bounds__(256) void conv_i8_k1_kernel(const QArgs a) {
    constexpr int NW = 2 * Q_K1_STEPS * Q_SLAB;   // [packet of the chunk][co]
    __shared__ __attribute__((aligned(16))) u32x4 sw[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, g = lane >> 5;
    const int co0 = blockIdx.y * Q_SLAB;
    const int nt = a.cout - co0 > 32 ? 2 : 1;
    const int64_t m = (int64_t)blockIdx.x * Q_PIX + wave * 32 + i;   // the lane's output pixel
    const bool live = m < a.M;
    const int8_t* xp = a.x;
    if (live) {
        int64_t ipix = m;
        if (a.s != 1) {
            const int hw = a.ho * a.wo, im = (int)(m / hw), rem = (int)(m - (int64_t)im * hw), oy = rem / a.wo, ox = rem - oy * a.wo;
            ipix = ((int64_t)im * a.h + oy * a.s) * a.w_in + ox * a.s;
        }
        xp += ipix * a.x_cs;
    }
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 bx[Q_K1_STEPS], nx[Q_K1_STEPS], pw[NW / 256];

    auto fetch = [&](int c, u32x4 (&dst)[Q_K1_STEPS]) {
#pragma unroll
        for (int st = 0; st < Q_K1_STEPS; ++st) {
            const int pk = 2 * (c * Q_K1_STEPS + st) + g;
            dst[st] = (live && pk < a.P) ? *reinterpret_cast<const u32x4*>(xp + pk * 16) : zero;
        }
#pragma unroll
        for (int r = 0; r < NW / 256; ++r) {
            const int e = r * 256 + tid, pk = 2 * c * Q_K1_STEPS + (e >> 6), co = co0 + (e & 63);
            pw[r] = (pk < a.P2 && co < a.cout_pad) ? *reinterpret_cast<const u32x4*>(a.w + ((int64_t)pk * a.cout_pad + co) * 16) : zero;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int r = 0; r < NW / 256; ++r) sw[r * 256 + tid] = pw[r];
    };

    i32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0;
    const int nsteps = a.P2 >> 1, nch = cdiv(nsteps, Q_K1_STEPS);
    fetch(0, bx);
    stash();
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) fetch(c + 1, nx);
#pragma unroll
        for (int st = 0; st < Q_K1_STEPS; ++st) {
            if (c * Q_K1_STEPS + st < nsteps) {   // workgroup-uniform
                acc[0] = q_mfma(sw[(2 * st + g) * Q_SLAB + i], bx[st], acc[0]);
                if (nt == 2) acc[1] = q_mfma(sw[(2 * st + g) * Q_SLAB + 32 + i], bx[st], acc[1]);
            }
        }
        __syncthreads();
        if (c + 1 < nch) {
            stash();
#pragma unroll
            for (int st = 0; st < Q_K1_STEPS; ++st) bx[st] = nx[st];
            __syncthreads();
        }
    }
    if (live) conv_i8_epilogue<OUT>(a, acc, nt, m, co0, g);
}

// ---- quantise ----
template <int DT>
__global__ __launch_bounds__(256) void quantize_i8_kernel(const void* x, int8_t* y, int64_t npix, int c, int x_cs, int y_cs, float inv, int vec) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {   // 16 channels per thread: 16-byte accesses
        const int groups = c >> 4;
        if (idx >= npix * groups) return;
        const int64_t pix = idx / groups;
        const int ch = (int)(idx - pix * groups) * 16;
        float f[16];
        if constexpr (DT == YMI_F32) {
            const f32x4* src = reinterpret_cast<const f32x4*>((const float*)x + pix * x_cs + ch);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = src[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) f[4 * q + e] = v[e];
            }
        } else {
            const u32x4* src = reinterpret_cast<const u32x4*>((const uint16_t*)x + pix * x_cs + ch);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32x4 v = src[q];
#pragma unroll
                for (int e = 0; e < 8; ++e) f[8 * q + e] = from16<DT>((uint16_t)(v[e >> 1] >> (16 * (e & 1))));
            }
        }
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e >> 2] |= ((uint32_t)q_code(f[e], inv) & 0xffu) << (8 * (e & 3));
        *reinterpret_cast<u32x4*>(y + pix * y_cs + ch) = o;
    } else {
        if (idx >= npix * c) return;
        const int64_t pix = idx / c;
        const int ch = (int)(idx - pix * c);
        y[pix * y_cs + ch] = (int8_t)q_code(load_elem<DT>(x, pix * x_cs + ch), inv);
    }
}

// ---- host side ----
static bool finite_f(float v) { return v == v && v - v == 0.0f; }

int conv_i8_check(const ymi_conv_i8_desc* d) {
    YMI_REQUIRE(d != nullptr, "ymi_conv2d_i8: null descriptor");
    YMI_REQUIRE(d->x && d->w && d->scale && d->bias && d->y, "ymi_conv2d_i8: null x / w / scale / bias / y");
    YMI_REQUIRE(d->cin > 0 && d->cin % 16 == 0, "ymi_conv2d_i8: cin must be a positive multiple of 16 (got %d)", d->cin);
    YMI_REQUIRE(d->cout > 0 && d->cout % 8 == 0, "ymi_conv2d_i8: cout must be a positive multiple of 8 (got %d)", d->cout);
    YMI_REQUIRE((d->k == 1 || d->k == 3) && (d->s == 1 || d->s == 2) && d->p == d->k / 2, "ymi_conv2d_i8: k in {1, 3}, s in {1, 2}, p = k / 2 (got k %d s %d p %d)", d->k, d->s, d->p);
    YMI_REQUIRE((int64_t)d->k * d->k * d->cin <= 133120, "ymi_conv2d_i8: k * k * cin = %lld products of +-127 * 127 do not fit int32", (long long)d->k * d->k * d->cin);
    YMI_REQUIRE(d->x_cstride >= d->cin && d->x_cstride % 16 == 0 && d->y_cstride >= d->cout && d->y_cstride % 8 == 0 && (d->res == nullptr || (d->res_cstride >= d->cout && d->res_cstride % 8 == 0)),
                "ymi_conv2d_i8: pixel strides must be >= c and multiples of 16 (x) / 8 (y, res) (x %d cin %d, y %d res %d cout %d)", d->x_cstride, d->cin, d->y_cstride, d->res_cstride, d->cout);
    YMI_REQUIRE(d->out_dtype == YMI_I8 || d->out_dtype == YMI_F16 || d->out_dtype == YMI_BF16, "ymi_conv2d_i8: out_dtype must be I8, F16 or BF16 (got %d)", d->out_dtype);
    YMI_REQUIRE(d->out_dtype != YMI_I8 || (finite_f(d->out_scale) && d->out_scale > 0.0f), "ymi_conv2d_i8: an int8 output needs a finite out_scale > 0 (got %g)", (double)d->out_scale);
    YMI_REQUIRE(d->res == nullptr || finite_f(d->res_scale), "ymi_conv2d_i8: res_scale must be finite");
    YMI_REQUIRE(d->act >= YMI_ACT_NONE && d->act <= YMI_ACT_LEAKY, "ymi_conv2d_i8: unknown activation %d", d->act);
    YMI_REQUIRE(d->n >= 0 && d->n <= 65535 && d->h >= 1 && d->w_in >= 1, "ymi_conv2d_i8: bad extent n %d h %d w %d (n <= 65535)", d->n, d->h, d->w_in);
    YMI_REQUIRE(d->ho == (d->h + 2 * d->p - d->k) / d->s + 1 && d->wo == (d->w_in + 2 * d->p - d->k) / d->s + 1, "ymi_conv2d_i8: output size %d x %d does not follow from the input's (%d x %d, k %d s %d)",
                d->ho, d->wo, d->h, d->w_in, d->k, d->s);
    YMI_REQUIRE((int64_t)d->n * d->ho * d->wo < ((int64_t)1 << 31) - Q_PIX && (int64_t)d->n * d->h * d->w_in < ((int64_t)1 << 31), "ymi_conv2d_i8: n * ho * wo must stay below 2^31 - 128");
    YMI_REQUIRE(((uintptr_t)d->x | (uintptr_t)d->w | (uintptr_t)d->scale | (uintptr_t)d->bias) % 16 == 0 && ((uintptr_t)d->y | (uintptr_t)d->res) % 8 == 0,
                "ymi_conv2d_i8: x / w / scale / bias must be 16-byte aligned, y / res 8-byte aligned");
    return YMI_OK;
}

template <int OUT>
static int conv_i8_launch_out(const ymi_conv_i8_desc* d, QArgs& a, hipStream_t s) {
    const unsigned slabs = (unsigned)cdiv(d->cout, Q_SLAB);
    if (d->k == 1) {
        hipLaunchKernelGGL((conv_i8_k1_kernel<OUT>), dim3((unsigned)cdiv(a.M, Q_PIX), slabs), dim3(256), 0, s, a);
    } else {
        a.tiles_x = cdiv(d->wo, Q_TW);
        const dim3 grid((unsigned)(a.tiles_x * cdiv(d->ho, Q_TH)), slabs, (unsigned)d->n);
        if (d->s == 1) hipLaunchKernelGGL((conv_i8_k3_kernel<1, OUT>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv_i8_k3_kernel<2, OUT>), grid, dim3(256), 0, s, a);
    }
    return check_launch("conv_i8_kernel");
}

int conv_i8_launch(const ymi_conv_i8_desc* d, hipStream_t s) {
    if (const int rc = conv_i8_check(d)) return rc;
    if (d->n == 0) return YMI_OK;
    QArgs a;
    a.x = (const int8_t*)d->x; a.w = (const int8_t*)d->w; a.scale = d->scale; a.bias = d->bias; a.y = d->y; a.res = d->res;
    a.n = d->n; a.h = d->h; a.w_in = d->w_in; a.cin = d->cin; a.x_cs = d->x_cstride; a.ho = d->ho; a.wo = d->wo; a.cout = d->cout; a.cout_pad = (d->cout + 31) / 32 * 32;
    a.y_cs = d->y_cstride; a.res_cs = d->res_cstride; a.s = d->s; a.act = d->act;
    a.P = d->cin / 16; a.P2 = (a.P + 1) / 2 * 2; a.tiles_x = 0; a.M = d->n * d->ho * d->wo;
    a.inv_out = d->out_dtype == YMI_I8 ? 1.0f / d->out_scale : 0.0f;
    a.res_scale = d->res ? d->res_scale : 0.0f;
    if (d->out_dtype == YMI_I8) return conv_i8_launch_out<YMI_I8>(d, a, s);
    if (d->out_dtype == YMI_F16) return conv_i8_launch_out<YMI_F16>(d, a, s);
    return conv_i8_launch_out<YMI_BF16>(d, a, s);
}

int quantize_i8_check(const ymi_quant_i8_desc* d) {
    YMI_REQUIRE(d != nullptr, "ymi_quantize_i8: null descriptor");
    YMI_REQUIRE(d->x && d->y, "ymi_quantize_i8: null x / y");
    YMI_REQUIRE(d->dtype == YMI_F16 || d->dtype == YMI_BF16 || d->dtype == YMI_F32, "ymi_quantize_i8: dtype must be F16, BF16 or F32 (got %d)", d->dtype);
    YMI_REQUIRE(d->c >= 1 && d->npix >= 0, "ymi_quantize_i8: bad extent npix %d c %d", d->npix, d->c);
    YMI_REQUIRE(d->x_cstride >= d->c && d->y_cstride >= d->c, "ymi_quantize_i8: pixel strides must be >= c (x %d y %d, c %d)", d->x_cstride, d->y_cstride, d->c);
    YMI_REQUIRE(finite_f(d->scale) && d->scale > 0.0f, "ymi_quantize_i8: scale must be finite and > 0 (got %g)", (double)d->scale);
    YMI_REQUIRE((int64_t)d->npix * d->c < ((int64_t)1 << 39), "ymi_quantize_i8: npix * c must stay below 2^39");
    YMI_REQUIRE((uintptr_t)d->x % (d->dtype == YMI_F32 ? 4 : 2) == 0, "ymi_quantize_i8: x is not aligned to its element size");
    return YMI_OK;
}

int quantize_i8_launch(const ymi_quant_i8_desc* d, hipStream_t s) {
    if (const int rc = quantize_i8_check(d)) return rc;
    if (d->npix == 0) return YMI_OK;
    const uintptr_t esz = d->dtype == YMI_F32 ? 4 : 2;
    const int vec = d->c % 16 == 0 && d->x_cstride % 16 == 0 && d->y_cstride % 16 == 0 && (uintptr_t)d->x % (16 * esz) == 0 && (uintptr_t)d->y % 16 == 0;
    const int64_t work = (int64_t)d->npix * (vec ? d->c / 16 : d->c);
    const dim3 grid((unsigned)((work + 255) / 256));
    const float inv = 1.0f / d->scale;
    if (d->dtype == YMI_F16) hipLaunchKernelGGL((quantize_i8_kernel<YMI_F16>), grid, dim3(256), 0, s, d->x, (int8_t*)d->y, (int64_t)d->npix, d->c, d->x_cstride, d->y_cstride, inv, vec);
    else if (d->dtype == YMI_BF16) hipLaunchKernelGGL((quantize_i8_kernel<YMI_BF16>), grid, dim3(256), 0, s, d->x, (int8_t*)d->y, (int64_t)d->npix, d->c, d->x_cstride, d->y_cstride, inv, vec);
    else hipLaunchKernelGGL((quantize_i8_kernel<YMI_F32>), grid, dim3(256), 0, s, d->x, (int8_t*)d->y, (int64_t)d->npix, d->c, d->x_cstride, d->y_cstride, inv, vec);
    return check_launch("quantize_i8_kernel");
}

}  // namespace ymi

extern "C" int ymi_conv2d_i8(const ymi_conv_i8_desc* d, void* stream) { return ymi::conv_i8_launch(d, (hipStream_t)stream); }
extern "C" int ymi_quantize_i8(const ymi_quant_i8_desc* d, void* stream) { return ymi::quantize_i8_launch(d, (hipStream_t)stream); }

extern "C" int64_t ymi_conv_i8_pack_bytes(int cout, int cin, int k) {
    if (cout <= 0 || cout % 8 || cin <= 0 || cin % 16 || (k != 1 && k != 3)) return -1;
    const int64_t P2 = (cin / 16 + 1) / 2 * 2, CP = (cout + 31) / 32 * 32;
    return (int64_t)k * k * P2 * CP * 16;
}

// int8 OIHW -> [tap][P2][CP][16] (the layout stated in the header); host pointers
extern "C" int ymi_conv_i8_pack(const int8_t* w, int cout, int cin, int k, void* blob, int64_t blob_bytes) {
    YMI_REQUIRE(w && blob, "ymi_conv_i8_pack: null argument");
    const int64_t need = ymi_conv_i8_pack_bytes(cout, cin, k);
    YMI_REQUIRE(need > 0, "ymi_conv_i8_pack: cin %% 16 == 0, cout %% 8 == 0 and k in {1, 3} are required (got cout %d cin %d k %d)", cout, cin, k);
    YMI_REQUIRE(blob_bytes >= need, "ymi_conv_i8_pack: the blob needs %lld bytes, %lld were given", (long long)need, (long long)blob_bytes);
    const int P = cin / 16, P2 = (P + 1) / 2 * 2, CP = (cout + 31) / 32 * 32;
    int8_t* b = (int8_t*)blob;
    memset(b, 0, (size_t)need);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < k * k; ++tap)
                b[(((int64_t)tap * P2 + ci / 16) * CP + co) * 16 + ci % 16] = w[((int64_t)co * cin + ci) * k * k + tap];
    return YMI_OK;
}
