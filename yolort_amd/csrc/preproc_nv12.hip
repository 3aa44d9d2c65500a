// NV12 video frames (include/yolort_amd.h, "NV12 ingest"): the YCbCr -> RGB conversion fused into the letterbox, and the stand-alone conversion to interleaved RGB8.
// The conversion is integer arithmetic (coefficients in units of 2^-14, one rounding shift, clamp), so every kernel of this file -- and a NumPy int64 restatement --
// gives the same bytes; the letterbox is then ymi_letterbox(YMI_U8_HWC) of those bytes, operation for operation: float(byte) / 255.0f per tap, the nested unfused
// lerp of letterbox_kernel, one rounding to the output type.
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "draw_common.hpp"

namespace ymi {

// {cy, crv, cgu, cgv, cbu} per [matrix][range]: round-to-nearest multiples of 2^-14 of the real coefficients (listed in the header)
static const int NV12_COEF[2][2][5] = {{{19077, 26149, -6419, -13320, 33050}, {16384, 22970, -5638, -11700, 29032}},
                                       {{19077, 29372, -3494, -8731, 34610}, {16384, 25802, -3069, -7670, 30402}}};
struct Nv12Coef {
    int yoff, cy, crv, cgu, cgv, cbu;
};

constexpr int NV12_MAX = 64;   // frames per launch: 48 bytes of kernarg each
struct Nv12Args {
    const unsigned char* y[NV12_MAX];
    const unsigned char* uv[NV12_MAX];
    int geom[NV12_MAX][6];    // h_in, w_in, h_res, w_res, pad_top, pad_left
    int pitch[NV12_MAX][2];   // bytes per Y row, per CbCr row
    void* out;
    int n, hb, wb, c_out;
    float fill;
    Nv12Coef k;
    int tiles_x, tiles_y;     // tiled kernel only
};
static_assert(sizeof(Nv12Args) < 4096, "the by-value descriptor table must stay under 4 KiB of kernarg");

// ---- the one conversion: chroma terms (shared by the two pixels of a pair), then luma + rounding shift + clamp + pack ----
__device__ __forceinline__ void nv12_chroma(int cb, int cr, const Nv12Coef& k, int& rt, int& gt, int& bt) {
    const int u = cb - 128, v = cr - 128;
    rt = k.crv * v;
    gt = k.cgu * u + k.cgv * v;
    bt = k.cbu * u;
}
__device__ __forceinline__ uint32_t nv12_pack(int y, int rt, int gt, int bt, const Nv12Coef& k) {
    const int yc = (y - k.yoff) * k.cy + 8192;
    int r = (yc + rt) >> 14, g = (yc + gt) >> 14, b = (yc + bt) >> 14;   // arithmetic shifts
    r = min(max(r, 0), 255);
    g = min(max(g, 0), 255);
    b = min(max(b, 0), 255);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);       // RGBX8: R in the low byte
}
__device__ __forceinline__ uint32_t nv12_rgbx(int y, int cb, int cr, const Nv12Coef& k) {
    int rt, gt, bt;
    nv12_chroma(cb, cr, k, rt, gt, bt);
    return nv12_pack(y, rt, gt, bt, k);
}
// pixel (y, x) of a frame: nearest chroma = the pair at chroma row y >> 1, byte offset x & ~1 (Cb, then Cr)
__device__ __forceinline__ uint32_t nv12_pixel(const unsigned char* yp, const unsigned char* up, int py, int puv, int y, int x, const Nv12Coef& k) {
    const int l = yp[(int64_t)y * py + x];
    const uint32_t c = *reinterpret_cast<const uint16_t*>(up + (int64_t)(y >> 1) * puv + (x & ~1));   // 2-byte aligned: uv and pitch_uv are even
    return nv12_rgbx(l, (int)(c & 255u), (int)(c >> 8), k);
}
__device__ __forceinline__ float nv12_chan(uint32_t rgbx, int c) { return (float)((rgbx >> (8 * c)) & 255u) / 255.0f; }   // load_elem<YMI_U8_HWC> of that byte

// exactly the tap arithmetic of letterbox_kernel
__device__ __forceinline__ void nv12_src(float s, int d, int n_in, int& i0, int& i1, float& l1) {
    float f = __fsub_rn(__fmul_rn(s, (float)d + 0.5f), 0.5f);
    f = f < 0.f ? 0.f : f;
    i0 = (int)f;
    i0 = i0 > n_in - 1 ? n_in - 1 : i0;
    i1 = i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
    l1 = f - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
}
__device__ __forceinline__ void nv12_lerp(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, float lx0, float lx1, float ly0, float ly1, float* v) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = __fadd_rn(__fmul_rn(nv12_chan(t00, c), lx0), __fmul_rn(nv12_chan(t01, c), lx1));
        const float bot = __fadd_rn(__fmul_rn(nv12_chan(t10, c), lx0), __fmul_rn(nv12_chan(t11, c), lx1));
        v[c] = __fadd_rn(__fmul_rn(top, ly0), __fmul_rn(bot, ly1));
    }
}

// ---------------------------------------------------------------------------------------------
// Per-pixel form: one thread per output pixel, four taps converted on the fly, any c_out.  The fallback of the tiled kernel and its bit-identical counterpart
// (YOLORT_AMD_LETTERBOX=pixel).
// ---------------------------------------------------------------------------------------------
template <int ODT>
__global__ __launch_bounds__(256) void letterbox_nv12_kernel(const Nv12Args a) {
    const int64_t npix = (int64_t)a.hb * a.wb;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= npix * a.n) return;
    const int img = (int)(gid / npix);
    const int rem = (int)(gid - (int64_t)img * npix);
    const int y = rem / a.wb, x = rem - y * a.wb;
    const int hin = a.geom[img][0], win = a.geom[img][1], hr = a.geom[img][2], wr = a.geom[img][3];
    const int yy = y - a.geom[img][4], xx = x - a.geom[img][5];
    float v[3] = {a.fill, a.fill, a.fill};
    if ((unsigned)yy < (unsigned)hr && (unsigned)xx < (unsigned)wr) {
        int y0, y1, x0, x1;
        float ly1, lx1;
        nv12_src((float)hin / (float)hr, yy, hin, y0, y1, ly1);
        nv12_src((float)win / (float)wr, xx, win, x0, x1, lx1);
        const unsigned char* yp = a.y[img];
        const unsigned char* up = a.uv[img];
        const int py = a.pitch[img][0], puv = a.pitch[img][1];
        nv12_lerp(nv12_pixel(yp, up, py, puv, y0, x0, a.k), nv12_pixel(yp, up, py, puv, y0, x1, a.k), nv12_pixel(yp, up, py, puv, y1, x0, a.k),
                  nv12_pixel(yp, up, py, puv, y1, x1, a.k), 1.f - lx1, lx1, 1.f - ly1, ly1, v);
    }
    if constexpr (ODT == YMI_F32) {
        float* o = (float*)a.out + gid * a.c_out;
        for (int c = 0; c < a.c_out; ++c) o[c] = c < 3 ? v[c] : 0.f;
    } else {
        uint16_t* o = (uint16_t*)a.out + gid * a.c_out;
        u32x2 w01;
        w01[0] = (uint32_t)to16<ODT>(v[0]) | ((uint32_t)to16<ODT>(v[1]) << 16);
        w01[1] = (uint32_t)to16<ODT>(v[2]);
        if (a.c_out == 4) {
            *reinterpret_cast<u32x2*>(o) = w01;
        } else if (a.c_out == 8) {
            u32x4 w = {w01[0], w01[1], 0u, 0u};
            *reinterpret_cast<u32x4*>(o) = w;
        } else {
            for (int c = 0; c < a.c_out; ++c) o[c] = c < 3 ? to16<ODT>(v[c]) : (uint16_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Tiled form: the data flow of letterbox_tile2_kernel (csrc/preproc_pool.hip) -- a 256-thread block owns (4 * RPW) x (128 * CG) output pixels of one frame, stages its
// source footprint [ry0, ry1] x [cx0, cx1] in flat chunk order (every lane of every load busy, one multiply-high per chunk), wave w resamples rows w, w + 4, ... with
// the column taps computed once -- with ONE new stage: the staging converts.  A thread loads one aligned 16-byte chunk of a Y row (16 pixels, columns xk .. xk + 15)
// and the chroma bytes of the same columns from chroma row r >> 1, converts the 16 pixels in registers and stores them as packed RGBX8, one 32-bit word per source
// pixel (four 16-byte LDS stores).  No raw bytes are staged, there is one barrier, and a tap is ONE 32-bit LDS read that yields the three channels (four reads per
// output pixel where the RGB8 path issues twelve byte reads).  LDS: 4 bytes per staged source pixel.
// The chroma row sits at its own 16-byte alignment: the 16 (18 when the Y base is odd) chroma bytes of a chunk start `rel` bytes into an aligned chunk, so the thread
// loads the two aligned chunks around them -- each only if it holds a needed byte: the guarantee of the RGB8 kernel, per plane -- and shifts the window out of the
// eight dwords with selects and one funnel shift per dword (rel is even).  With rows and bases aligned alike (decoder surfaces) rel is 0 and the second chunk is
// never needed.  The chroma chunk is read once per luma row (twice per chroma row): that keeps the chunk -> lane map flat.
// ---------------------------------------------------------------------------------------------
template <int ODD>   // the parity of the Y plane's base address = of every chunk's first column xk (the pitches are even)
__device__ __forceinline__ void nv12_convert16(const u32x4 yv, const uint32_t* c, const Nv12Coef& k, u32x4* dst) {
    int rt[8 + ODD], gt[8 + ODD], bt[8 + ODD];   // chroma pair p = bytes 2p, 2p + 1 of the window, which starts at the even column xk - ODD
#pragma unroll
    for (int p = 0; p < 8 + ODD; ++p) {
        const uint32_t pr = (c[p >> 1] >> (16 * (p & 1))) & 0xffffu;
        nv12_chroma((int)(pr & 255u), (int)(pr >> 8), k, rt[p], gt[p], bt[p]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {   // four pixels = one 16-byte LDS store
        u32x4 q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = (4 * m + j + ODD) >> 1;
            q[j] = nv12_pack((int)((yv[m] >> (8 * j)) & 255u), rt[p], gt[p], bt[p], k);
        }
        dst[m] = q;
    }
}

template <int ODT, int RPW, int CG>
__global__ __launch_bounds__(256) void letterbox_nv12_tile_kernel(const Nv12Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nv12_sm[];
    constexpr int TH = 4 * RPW, TW = 128 * CG;
    const int img = blockIdx.y, tile = blockIdx.x;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int y0t = ty * TH, x0t = tx * TW;
    const int hin = a.geom[img][0], win = a.geom[img][1], hr = a.geom[img][2], wr = a.geom[img][3];
    const int pt = a.geom[img][4], pl = a.geom[img][5];
    const float sy = (float)hin / (float)hr, sx = (float)win / (float)wr;
    const int ya = max(y0t, pt), yb = min(y0t + TH, min(pt + hr, a.hb));
    const int xa = max(x0t, pl), xb = min(x0t + TW, min(pl + wr, a.wb));
    const bool any = ya < yb && xa < xb;
    int ry0 = 0, ry1 = -1, cx0 = 0, cx1 = -1;
    if (any) {
        int i0, i1;
        float l;
        nv12_src(sy, ya - pt, hin, ry0, i1, l);
        nv12_src(sy, yb - 1 - pt, hin, i0, ry1, l);
        nv12_src(sx, xa - pl, win, cx0, i1, l);
        nv12_src(sx, xb - 1 - pl, win, i0, cx1, l);
    }
    const int nrows = ry1 - ry0 + 1;
    const int span = cx1 - cx0 + 1;                // source pixels = Y bytes of a staged row
    const int pitch = ((span + 15 + 15) >> 4) << 4;   // staged pixels per row: whole chunks, whatever the alignment shift
    const unsigned char* ybase = a.y[img];
    const unsigned char* ubase = a.uv[img];
    const int py = a.pitch[img][0], puv = a.pitch[img][1];
    // 16-byte alignment of the first needed byte of Y row r: (al_a + r * al_r) & 15; of the start of chroma row q: (al_b + q * al_p) & 15
    const int al_a = (int)(((uintptr_t)ybase + (uintptr_t)cx0) & 15), al_r = py & 15;
    const int al_b = (int)((uintptr_t)ubase & 15), al_p = puv & 15;
    const bool odd = ((uintptr_t)ybase & 1) != 0;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* sm32 = reinterpret_cast<uint32_t*>(nv12_sm);
    if (any) {
        // flat chunk order: chunk i is 16-pixel column (i % cpr) of staged row (i / cpr) and lands at LDS byte 64 * i
        const unsigned cpr = (unsigned)pitch >> 4;
        const unsigned total = (unsigned)nrows * cpr;
        const unsigned magic = cpr == 1 ? 0u : 0xffffffffu / cpr + 1u;   // i / cpr == mulhi(i, magic) for i < 2^16 (total <= 64 KiB / 64); cpr == 1: the chunk IS the row
        const unsigned char* safe_y = (const unsigned char*)((uintptr_t)ybase & ~(uintptr_t)15);    // a chunk that is not needed reads this one instead (never used)
        const unsigned char* safe_uv = (const unsigned char*)((uintptr_t)ubase & ~(uintptr_t)15);
        for (unsigned i0 = threadIdx.x; i0 < total; i0 += 512) {
            u32x4 yv[2], clo[2], chi[2];
            bool have[2];
            int rel[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {   // all loads of two chunks in flight, then two conversions
                const unsigned i = i0 + 256u * u;
                const unsigned job = cpr == 1 ? i : __umulhi(i, magic), kc = i - job * cpr;
                const int r = ry0 + (int)job;
                const int sh = (al_a + r * al_r) & 15;
                const int xk = cx0 - sh + (int)(kc << 4);                 // first pixel column of the chunk (may lie left of cx0, even of 0: such columns are not needed)
                have[u] = i < total && (int)(kc << 4) < sh + span;        // aligned chunks holding at least one needed byte (an aligned chunk never crosses a page)
                const unsigned char* g = ybase + (int64_t)r * py + xk;
                yv[u] = *reinterpret_cast<const u32x4*>(have[u] ? g : safe_y);
                const int a0 = xk & ~1;                                   // the chroma window starts at the even column at or below xk
                rel[u] = (al_b + (r >> 1) * al_p + a0) & 15;
                const int lo = a0 - rel[u];                               // row offset of the aligned chunk that holds the window's first byte
                const int n_lo = max(xk, cx0) & ~1, n_hi = min(xk + 15, cx1) | 1;   // first and last NEEDED chroma byte (cx1 | 1 <= w - 1: w is even)
                const unsigned char* cu = ubase + (int64_t)(r >> 1) * puv + lo;
                clo[u] = *reinterpret_cast<const u32x4*>(have[u] && n_lo < lo + 16 ? cu : safe_uv);
                chi[u] = *reinterpret_cast<const u32x4*>(have[u] && n_hi >= lo + 16 ? cu + 16 : safe_uv);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!have[u]) continue;
                // the 20-byte window at byte `rel` of the two chunks: dword selects on bits 2 and 3 of rel, then one funnel shift per dword on bit 1 (named scalars: an
                // array here turns the selects into a dynamically indexed load from scratch)
                const uint32_t w0 = clo[u][0], w1 = clo[u][1], w2 = clo[u][2], w3 = clo[u][3], w4 = chi[u][0], w5 = chi[u][1], w6 = chi[u][2], w7 = chi[u][3];
                const bool q1 = (rel[u] & 4) != 0, q2 = (rel[u] & 8) != 0;
                const unsigned s = (unsigned)(rel[u] & 2) * 8u;
                const uint32_t t0 = q1 ? w1 : w0, t1 = q1 ? w2 : w1, t2 = q1 ? w3 : w2, t3 = q1 ? w4 : w3, t4 = q1 ? w5 : w4, t5 = q1 ? w6 : w5, t6 = q1 ? w7 : w6;
                const uint32_t d0 = q2 ? t2 : t0, d1 = q2 ? t3 : t1, d2 = q2 ? t4 : t2, d3 = q2 ? t5 : t3, d4 = q2 ? t6 : t4;
                auto fsh = [s](uint32_t lo, uint32_t hi) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> s); };
                const uint32_t c[5] = {fsh(d0, d1), fsh(d1, d2), fsh(d2, d3), fsh(d3, d4), fsh(d4, 0u)};   // only the low half of c[4] is used
                u32x4* dst = reinterpret_cast<u32x4*>(nv12_sm + (size_t)(i0 + 256u * u) * 64);
                if (odd) nv12_convert16<1>(yv[u], c, a.k, dst);
                else nv12_convert16<0>(yv[u], c, a.k, dst);
            }
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int cg = 0; cg < CG; ++cg) {
        const int x = x0t + cg * 128 + (threadIdx.x & 63) * 2;
        if (x >= a.wb) break;
        // column taps of the thread's two pixels: word offsets inside a staged row, weights
        bool inx[2];
        int ox0[2], ox1[2];
        float lx0[2], lx1[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int xx = x + p - pl;
            inx[p] = (unsigned)xx < (unsigned)wr && x + p < a.wb;
            ox0[p] = ox1[p] = 0;
            lx0[p] = lx1[p] = 0.f;
            if (inx[p]) {
                int sx0, sx1;
                nv12_src(sx, xx, win, sx0, sx1, lx1[p]);
                lx0[p] = 1.f - lx1[p];
                ox0[p] = sx0 - cx0;
                ox1[p] = sx1 - cx0;
            }
        }
        const bool two = x + 1 < a.wb;
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int y = y0t + 4 * j + wv;
            if (y >= a.hb) break;   // wave-uniform
            float v[2][3];
#pragma unroll
            for (int p = 0; p < 2; ++p) v[p][0] = v[p][1] = v[p][2] = a.fill;
            const int yy = y - pt;
            if ((unsigned)yy < (unsigned)hr && (inx[0] || inx[1])) {
                int sy0, sy1;
                float ly1;
                nv12_src(sy, yy, hin, sy0, sy1, ly1);
                const float ly0 = 1.f - ly1;
                const uint32_t* r0 = sm32 + (sy0 - ry0) * pitch + ((al_a + sy0 * al_r) & 15);
                const uint32_t* r1 = sm32 + (sy1 - ry0) * pitch + ((al_a + sy1 * al_r) & 15);
#pragma unroll
                for (int p = 0; p < 2; ++p) {   // branch-free: a pixel outside the resized region reads word 0 of the rows and keeps the fill value
                    float val[3];
                    nv12_lerp(r0[ox0[p]], r0[ox1[p]], r1[ox0[p]], r1[ox1[p]], lx0[p], lx1[p], ly0, ly1, val);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[p][c] = inx[p] ? val[c] : a.fill;
                }
            }
            const int64_t o = (((int64_t)img * a.hb + y) * a.wb + x) * 4;
            if constexpr (ODT == YMI_F32) {
                float* op = (float*)a.out + o;
                f32x4 q0 = {v[0][0], v[0][1], v[0][2], 0.f};
                *reinterpret_cast<f32x4*>(op) = q0;
                if (two) {
                    f32x4 q1 = {v[1][0], v[1][1], v[1][2], 0.f};
                    *reinterpret_cast<f32x4*>(op + 4) = q1;
                }
            } else {
                uint16_t* op = (uint16_t*)a.out + o;
                u32x4 q;
                q[0] = cvt_pk16<ODT>(f32x2{v[0][0], v[0][1]});
                q[1] = cvt_pk16<ODT>(f32x2{v[0][2], 0.f});
                q[2] = cvt_pk16<ODT>(f32x2{v[1][0], v[1][1]});
                q[3] = cvt_pk16<ODT>(f32x2{v[1][2], 0.f});
                if (two && (a.wb & 1) == 0) *reinterpret_cast<u32x4*>(op) = q;
                else {
                    u32x2 h0 = {q[0], q[1]};
                    *reinterpret_cast<u32x2*>(op) = h0;
                    if (two) { u32x2 h1 = {q[2], q[3]}; *reinterpret_cast<u32x2*>(op + 4) = h1; }
                }
            }
        }
    }   // column groups
}

// ---------------------------------------------------------------------------------------------
// NV12 -> interleaved RGB8 (h, w, 3): a thread converts a run of 4 pixels of one row (2 at the end of a row whose width is no multiple of 4) and stores 12
// contiguous bytes.  The image ops.crop_detections / ops.draw_detections take for video frames, and the device-side statement of the conversion contract.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nv12_to_rgb_kernel(const unsigned char* yp, const unsigned char* up, int py, int puv, int h, int w, Nv12Coef k,
                                                          unsigned char* rgb, int dword_ok) {
    const int wq = (w + 3) >> 2;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)h * wq) return;
    const int y = (int)(gid / wq), x = (int)(gid - (int64_t)y * wq) * 4;
    const int npx = min(4, w - x);   // 4 or 2
    uint32_t p[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < npx; ++i) p[i] = nv12_pixel(yp, up, py, puv, y, x + i, k);
    unsigned char* o = rgb + ((int64_t)y * w + x) * 3;
    // RGBX RGBX RGBX RGBX -> RGBR GBRG BRGB
    const uint32_t d0 = (p[0] & 0xffffffu) | (p[1] << 24), d1 = ((p[1] >> 8) & 0xffffu) | (p[2] << 16), d2 = ((p[2] >> 16) & 0xffu) | (p[3] << 8);
    if (npx == 4 && dword_ok) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = d0; o4[1] = d1; o4[2] = d2;
    } else {   // 2-byte stores: (y * w + x) is even
        uint16_t* o2 = reinterpret_cast<uint16_t*>(o);
        o2[0] = (uint16_t)d0; o2[1] = (uint16_t)(d0 >> 16); o2[2] = (uint16_t)d1;
        if (npx == 4) { o2[3] = (uint16_t)(d1 >> 16); o2[4] = (uint16_t)d2; o2[5] = (uint16_t)(d2 >> 16); }
    }
}

// dynamic LDS of the tiled kernel for tiles of th x tw: letterbox_tile_lds's bound on the footprint (csrc/preproc_pool.hip), 4 bytes per staged pixel; 0 = over the cap
static size_t nv12_tile_lds(const Nv12Args& a, int th, int tw, size_t cap = 64 * 1024) {
    size_t need = 64;
    for (int i = 0; i < a.n; ++i) {
        const double sy = (double)a.geom[i][0] / a.geom[i][2], sx = (double)a.geom[i][1] / a.geom[i][3];
        const int rows = (int)(th * sy) + 3, cols = (int)(tw * sx) + 3;
        const size_t pitch = (((size_t)(cols < a.geom[i][1] ? cols : a.geom[i][1]) + 30) >> 4) << 4;
        const size_t b = (size_t)(rows < a.geom[i][0] ? rows : a.geom[i][0]) * pitch * 4;
        need = b > need ? b : need;
    }
    return need <= cap ? need : 0;   // the largest dynamic LDS request that needs no opt-in
}

// ---------------------------------------------------------------------------------------------
// The far end of the video path (include/yolort_amd.h, "NV12 drawing and cropping"): detections drawn straight into the Y and CbCr planes, and cut out of them.
// RGB -> YCbCr is the integer contract of the header -- nine coefficients in units of 2^-14 per [matrix][range], one rounding shift, offset, clamp -- and is applied
// ONCE PER LIST ENTRY (the box colour of a listed detection) and once to the text colour, never per pixel.
// ---------------------------------------------------------------------------------------------
// {cyr, cyg, cyb, cbr, cbg, cbb, crr, crg, crb} per [matrix][range]: round-to-nearest multiples of 2^-14 of the real coefficients (listed in the header)
static const int YCC_COEF[2][2][9] = {{{4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170}, {4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332}},
                                      {{2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660}, {3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751}}};
struct YccCoef {
    int yoff, c[9];
};
// r | g << 8 | b << 16  ->  Y | Cb << 8 | Cr << 16
__device__ __forceinline__ uint32_t rgb_to_ycc(uint32_t rgb, const YccCoef& k) {
    const int r = (int)(rgb & 255u), g = (int)((rgb >> 8) & 255u), b = (int)((rgb >> 16) & 255u);
    int y = ((k.c[0] * r + k.c[1] * g + k.c[2] * b + 8192) >> 14) + k.yoff;   // arithmetic shifts
    int cb = ((k.c[3] * r + k.c[4] * g + k.c[5] * b + 8192) >> 14) + 128;
    int cr = ((k.c[6] * r + k.c[7] * g + k.c[8] * b + 8192) >> 14) + 128;
    y = min(max(y, 0), 255);
    cb = min(max(cb, 0), 255);
    cr = min(max(cr, 0), 255);
    return (uint32_t)y | ((uint32_t)cb << 8) | ((uint32_t)cr << 16);
}

// ---------------------------------------------------------------------------------------------
// render_nv12_kernel: ymi_render's rule per LUMA pixel (render_list and render_decide of csrc/draw_common.hpp: the code render_kernel runs), written into NV12 planes.
// A workgroup of 256 threads owns a 64 x 16 luma tile = 32 x 8 chroma pairs, one per thread; frame sides are even, so a tile never splits a pair.
//   Phase 1  the tile's list in slot order (render_list); the entry stored at position i also gets ycc[i] = the {Y, Cb, Cr} of its box colour.  An empty list: return,
//            nothing of the frame is read or written.
//   Phase 2  a thread owns four adjacent luma pixels of a row, decides them, writes their four 16-bit codes -- 0: untouched, else (list position + 1) << 1 | glyph --
//            to the 64 x 16 code tile in LDS as ONE 8-byte store, and stores Y: one 32-bit store when all four are decided and the address is 4-byte aligned (it
//            depends on the plane's base, the pitch and the row), byte stores of the decided ones otherwise.
//   Barrier.
//   Phase 3  a thread reads the 2 x 2 codes of its pair (two 32-bit LDS reads), takes the FIRST non-zero one in raster order, looks (Cb, Cr) up in ycc[] (or takes the
//            text colour's) and stores the pair as ONE 16-bit store.  A pair none of whose four pixels is decided is not written.
// No atomics on pixels, no races (a byte has one owner per phase), no allocation.  LDS: 36 B per slab slot + 2 064 B (k = 300: 12 864 B, k = 1024: 38 928 B).
// ---------------------------------------------------------------------------------------------
struct RenderNv12Args {
    unsigned char* y[NV12_MAX];   // frames img_base .. img_base + img_n - 1
    unsigned char* uv[NV12_MAX];
    int pitch[NV12_MAX][2];       // bytes per Y row, per CbCr row
    int hw[NV12_MAX][2];
    int lwfs[NV12_MAX][2];        // outline width, font scale
    int tile_end[NV12_MAX];       // inclusive prefix of the frames' tile counts
    const float* boxes;
    const float* scores;
    const int64_t* labels;
    const int32_t* counts;
    const uint8_t* names;
    const uint8_t* colors;
    int32_t* status;
    int img_base, img_n, k, m, num_classes, draw_labels, draw_conf;
    uint32_t txt;                 // r | g << 8 | b << 16
    YccCoef c;
};
static_assert(sizeof(RenderNv12Args) < 4096, "the by-value descriptor table must stay under 4 KiB of kernarg");
constexpr size_t RD_CODES_BYTES = (size_t)RD_TW * RD_TH * sizeof(uint16_t);
static size_t render_nv12_lds(int k) { return (size_t)k * (sizeof(RenderEntry) + sizeof(uint32_t)) + RD_CODES_BYTES + 4 * sizeof(int); }

__global__ __launch_bounds__(256) void render_nv12_kernel(const RenderNv12Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nv12_sm[];
    RenderEntry* list = reinterpret_cast<RenderEntry*>(nv12_sm);                                           // k entries
    uint16_t* codes = reinterpret_cast<uint16_t*>(nv12_sm + (size_t)a.k * sizeof(RenderEntry));            // RD_TH rows of RD_TW codes (16-byte aligned)
    int* wcnt = reinterpret_cast<int*>(nv12_sm + (size_t)a.k * sizeof(RenderEntry) + RD_CODES_BYTES);      // the four wave totals of a pass
    uint32_t* ycc = reinterpret_cast<uint32_t*>(wcnt + 4);                                                 // k words: Y | Cb << 8 | Cr << 16 of entry i's box colour
    const int tid = (int)threadIdx.x;
    int li = 0;
    for (int i = 0; i < a.img_n - 1; ++i) li += (int)blockIdx.x >= a.tile_end[i] ? 1 : 0;   // block-uniform
    const int tile = (int)blockIdx.x - (li ? a.tile_end[li - 1] : 0);
    const int H = a.hw[li][0], W = a.hw[li][1], lw = a.lwfs[li][0], fs = a.lwfs[li][1];
    const int tiles_x = (W + RD_TW - 1) / RD_TW;
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int tx0 = txi * RD_TW, ty0 = tyi * RD_TH;
    // ---- phase 1 ----
    const int nlist = render_list(a, a.img_base + li, tile, tx0, ty0, fs, wcnt, [&](int off, const RenderEntry& e) {
        list[off] = e;
        ycc[off] = rgb_to_ycc(e.rgb, a.c);
    });
    if (nlist == 0) return;   // block-uniform: nothing meets this tile, the frame is neither read nor written
    const uint32_t txt = rgb_to_ycc(a.txt, a.c);   // uniform: once per workgroup, in scalar registers
    // ---- phase 2: four adjacent luma pixels per thread ----
    {
        const int yl = tid >> 4, xl = (tid & 15) * 4;
        const int y = ty0 + yl, x = tx0 + xl;
        uint32_t code[4] = {0u, 0u, 0u, 0u}, lum[4] = {0u, 0u, 0u, 0u};
        unsigned found = 0;
        if (y < H && x < W) {
            const unsigned want = x + 3 < W ? 0xfu : ((1u << (W - x)) - 1u);
            found = render_decide(list, nlist, x, y, want, lw, fs, a.names, [&](int p, int i, const RenderEntry&, bool glyph) {
                code[p] = ((uint32_t)(i + 1) << 1) | (glyph ? 1u : 0u);
                lum[p] = (glyph ? txt : ycc[i]) & 255u;
            });
        }
        const u32x2 cw = {code[0] | (code[1] << 16), code[2] | (code[3] << 16)};
        *reinterpret_cast<u32x2*>(codes + yl * RD_TW + xl) = cw;   // every thread, also outside the frame: phase 3 reads whole 2 x 2 blocks
        if (found) {
            unsigned char* o = a.y[li] + (int64_t)y * a.pitch[li][0] + x;
            if (found == 0xfu && ((uintptr_t)o & 3) == 0) {
                *reinterpret_cast<uint32_t*>(o) = lum[0] | (lum[1] << 8) | (lum[2] << 16) | (lum[3] << 24);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if ((found >> p) & 1u) o[p] = (unsigned char)lum[p];
            }
        }
    }
    __syncthreads();
    // ---- phase 3: one chroma pair per thread ----
    const int cyl = tid >> 5, cxl = tid & 31;
    const int yy = ty0 + 2 * cyl, xx = tx0 + 2 * cxl;   // the pair's top-left luma pixel; the sides are even, so the other three exist with it
    if (yy >= H || xx >= W) return;
    const uint32_t top = *reinterpret_cast<const uint32_t*>(codes + (2 * cyl) * RD_TW + 2 * cxl);
    const uint32_t bot = *reinterpret_cast<const uint32_t*>(codes + (2 * cyl + 1) * RD_TW + 2 * cxl);
    const uint32_t c = (top & 0xffffu) ? (top & 0xffffu) : ((top >> 16) ? (top >> 16) : ((bot & 0xffffu) ? (bot & 0xffffu) : (bot >> 16)));
    if (c == 0u) return;
    const uint32_t v = (c & 1u) ? txt : ycc[(c >> 1) - 1u];
    *reinterpret_cast<uint16_t*>(a.uv[li] + (int64_t)(yy >> 1) * a.pitch[li][1] + xx) = (uint16_t)(v >> 8);   // Cb, then Cr; 2-byte aligned: uv, the pitch and xx are even
}

// ---------------------------------------------------------------------------------------------
// crop_resize_nv12_kernel: crop_resize_kernel's body (crop_resize_body, csrc/draw_common.hpp) with ONE difference, the source fetch: a tap is nv12_pixel -- the frame's
// luma byte and its nearest chroma pair converted by the ingest contract -- read as float(byte) / 255.0f, exactly what crop_resize_kernel<YMI_U8_HWC> reads from
// ymi_nv12_to_rgb's image.  Bit for bit ymi_crop_resize of that image, without the image.
// ---------------------------------------------------------------------------------------------
struct CropNv12Args {
    const unsigned char* y[NV12_MAX];   // frames img_base .. img_base + img_n - 1
    const unsigned char* uv[NV12_MAX];
    int pitch[NV12_MAX][2];
    int hw[NV12_MAX][2];
    const float* boxes;
    const int32_t* counts;
    void* crops;
    int32_t* index;
    int32_t* total;
    int n, img_base, img_n, k, cap, out_h, out_w, tiles, square, normalize;
    float gain, pad, mean[3], std[3];
    Nv12Coef c;
};
static_assert(sizeof(CropNv12Args) < 4096, "the by-value descriptor table must stay under 4 KiB of kernarg");
struct CropSrcNv12 {
    typedef uint32_t Pixel;   // RGBX8
    const unsigned char *yp, *up;
    int py, puv;
    const Nv12Coef& k;
    __device__ __forceinline__ CropSrcNv12(const CropNv12Args& a, int li, int, int) : yp(a.y[li]), up(a.uv[li]), py(a.pitch[li][0]), puv(a.pitch[li][1]), k(a.c) {}
    __device__ __forceinline__ Pixel pixel(int y, int x) const { return nv12_pixel(yp, up, py, puv, y, x, k); }
    __device__ __forceinline__ float chan(Pixel t, int c) const { return nv12_chan(t, c); }
};

template <int ODT, int PX>
__global__ __launch_bounds__(256) void crop_resize_nv12_kernel(const CropNv12Args a) {
    crop_resize_body<CropSrcNv12, ODT, PX>(a);
}

// the frame rules of ops.nv12_planes: even sides >= 2, even pitches >= the width, a 2-byte-aligned chroma plane
static int nv12_frame_ok(const char* who, int i, const void* y, const void* uv, int h, int w, int py, int puv) {
    YMI_REQUIRE(y && uv, "%s: frame %d has a null plane", who, i);
    YMI_REQUIRE(((uintptr_t)uv & 1) == 0, "%s: the CbCr plane of frame %d is not 2-byte aligned", who, i);
    YMI_REQUIRE(h >= 2 && w >= 2 && (h & 1) == 0 && (w & 1) == 0 && (int64_t)h * w < ((int64_t)1 << 31), "%s: frame %d is %dx%d: NV12 sides are even and >= 2", who, i, h, w);
    YMI_REQUIRE(py >= w && puv >= w && ((py | puv) & 1) == 0, "%s: frame %d: pitches %d / %d must be even and >= the width %d", who, i, py, puv, w);
    return YMI_OK;
}

static bool nv12_coef(int matrix, int range, Nv12Coef& k) {
    if ((unsigned)matrix > 1u || (unsigned)range > 1u) return false;
    const int* c = NV12_COEF[matrix][range];
    k.yoff = range == YMI_NV12_LIMITED ? 16 : 0;
    k.cy = c[0]; k.crv = c[1]; k.cgu = c[2]; k.cgv = c[3]; k.cbu = c[4];
    return true;
}

constexpr int NV12_CG_DEFAULT = 1;

static int nv12_dispatch(Nv12Args& a, int out_dtype, hipStream_t s) {
    // Default: the per-pixel kernel.  Measured on 32 frames of 1080 x 1920 -> 640 fp16 (a 3x down-scale; profiles/nv12_bench.txt): per-pixel 82 us, tiled 97 us at two
    // rows per wave (four do not fit 64 KiB) and 105 us at one -- the staging converts all nine source pixels under an output pixel, the taps need four.  The tiled
    // kernel is selected with the knob of ymi_letterbox, YOLORT_AMD_LETTERBOX = "1" | "2" | "4" (rows per wave: the largest value not above it that fits), with
    // YOLORT_AMD_LB_CG column groups; "pixel" names the default.
    const char* lb_env = getenv("YOLORT_AMD_LETTERBOX");
    const int rpw_max = (lb_env && (lb_env[0] == '1' || lb_env[0] == '2' || lb_env[0] == '4') && lb_env[1] == 0) ? lb_env[0] - '0' : 0;
    const bool lb_pixel = rpw_max == 0;
    if (a.c_out == 4 && !lb_pixel) {
        const char* cge = getenv("YOLORT_AMD_LB_CG");
        const int cg_max = cge ? (atoi(cge) >= 2 ? 2 : 1) : NV12_CG_DEFAULT;
        for (int rpw = rpw_max; rpw >= 1; rpw >>= 1) {
            int cg = cg_max;
            size_t lds = nv12_tile_lds(a, 4 * rpw, 128 * cg);
            if (lds == 0 && cg > 1) lds = nv12_tile_lds(a, 4 * rpw, 128 * (cg = 1));
            if (lds == 0) continue;
            a.tiles_x = cdiv(a.wb, 128 * cg);
            a.tiles_y = cdiv(a.hb, 4 * rpw);
            dim3 gt((unsigned)(a.tiles_x * a.tiles_y), (unsigned)a.n), bt(256);
#define YMI_NVT2C(ODT_, CG_)                                                                                \
    if (rpw == 4) hipLaunchKernelGGL((letterbox_nv12_tile_kernel<ODT_, 4, CG_>), gt, bt, lds, s, a);         \
    else if (rpw == 2) hipLaunchKernelGGL((letterbox_nv12_tile_kernel<ODT_, 2, CG_>), gt, bt, lds, s, a);    \
    else hipLaunchKernelGGL((letterbox_nv12_tile_kernel<ODT_, 1, CG_>), gt, bt, lds, s, a);
#define YMI_NVT2(ODT_)                                  \
    if (cg == 2) { YMI_NVT2C(ODT_, 2) } else { YMI_NVT2C(ODT_, 1) }
            switch (out_dtype) {
                case YMI_F16: YMI_NVT2(YMI_F16) break;
                case YMI_BF16: YMI_NVT2(YMI_BF16) break;
                default: YMI_NVT2(YMI_F32) break;
            }
#undef YMI_NVT2
#undef YMI_NVT2C
            return check_launch("letterbox_nv12_tile_kernel");
        }
    }
    const int64_t total = (int64_t)a.n * a.hb * a.wb;
    dim3 grid((unsigned)((total + 255) / 256)), block(256);
    switch (out_dtype) {
        case YMI_F16: hipLaunchKernelGGL((letterbox_nv12_kernel<YMI_F16>), grid, block, 0, s, a); break;
        case YMI_BF16: hipLaunchKernelGGL((letterbox_nv12_kernel<YMI_BF16>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((letterbox_nv12_kernel<YMI_F32>), grid, block, 0, s, a); break;
    }
    return check_launch("letterbox_nv12_kernel");
}

}  // namespace ymi

using namespace ymi;

extern "C" int ymi_letterbox_nv12(const ymi_nv12_desc* d, void* stream) {
    YMI_REQUIRE(d != nullptr, "ymi_letterbox_nv12: null descriptor");
    YMI_REQUIRE(d->n >= 0 && d->out && (d->n == 0 || (d->y && d->uv && d->pitch && d->geom)), "ymi_letterbox_nv12: null argument");
    YMI_REQUIRE(d->c_out >= 3, "ymi_letterbox_nv12: c_out must be >= 3");
    YMI_REQUIRE(d->hb >= 1 && d->wb >= 1, "ymi_letterbox_nv12: bad canvas %dx%d", d->hb, d->wb);
    YMI_REQUIRE(d->out_dtype == YMI_F16 || d->out_dtype == YMI_BF16 || d->out_dtype == YMI_F32, "ymi_letterbox_nv12: bad out_dtype %d", d->out_dtype);
    Nv12Args a;
    YMI_REQUIRE(nv12_coef(d->matrix, d->range, a.k), "ymi_letterbox_nv12: bad matrix %d / range %d", d->matrix, d->range);
    const size_t esz = d->out_dtype == YMI_F32 ? 4 : 2;
    a.hb = d->hb; a.wb = d->wb; a.c_out = d->c_out; a.fill = d->fill;
    a.tiles_x = a.tiles_y = 0;
    for (int base = 0; base < d->n; base += NV12_MAX) {   // validate every frame before the first launch
        const int m = (d->n - base) < NV12_MAX ? (d->n - base) : NV12_MAX;
        for (int i = base; i < base + m; ++i) {
            const int32_t* g = d->geom + (size_t)i * 6;
            YMI_REQUIRE(d->y[i] && d->uv[i], "ymi_letterbox_nv12: frame %d has a null plane", i);
            YMI_REQUIRE(((uintptr_t)d->uv[i] & 1) == 0, "ymi_letterbox_nv12: the CbCr plane of frame %d is not 2-byte aligned", i);
            YMI_REQUIRE(g[0] >= 2 && g[1] >= 2 && (g[0] & 1) == 0 && (g[1] & 1) == 0, "ymi_letterbox_nv12: frame %d is %dx%d: NV12 sides are even and >= 2", i, g[0], g[1]);
            YMI_REQUIRE(d->pitch[2 * i] >= g[1] && d->pitch[2 * i + 1] >= g[1] && ((d->pitch[2 * i] | d->pitch[2 * i + 1]) & 1) == 0,
                        "ymi_letterbox_nv12: frame %d: pitches %d / %d must be even and >= the width %d", i, d->pitch[2 * i], d->pitch[2 * i + 1], g[1]);
            YMI_REQUIRE(g[2] >= 1 && g[3] >= 1 && g[2] + g[4] <= d->hb && g[3] + g[5] <= d->wb && g[4] >= 0 && g[5] >= 0,
                        "ymi_letterbox_nv12: frame %d (%dx%d at %d,%d) does not fit the %dx%d canvas", i, g[2], g[3], g[4], g[5], d->hb, d->wb);
        }
    }
    for (int base = 0; base < d->n; base += NV12_MAX) {
        a.n = (d->n - base) < NV12_MAX ? (d->n - base) : NV12_MAX;
        for (int i = 0; i < a.n; ++i) {
            a.y[i] = (const unsigned char*)d->y[base + i];
            a.uv[i] = (const unsigned char*)d->uv[base + i];
            a.pitch[i][0] = d->pitch[2 * (base + i)];
            a.pitch[i][1] = d->pitch[2 * (base + i) + 1];
            for (int k = 0; k < 6; ++k) a.geom[i][k] = d->geom[(size_t)(base + i) * 6 + k];
        }
        a.out = (char*)d->out + (size_t)base * d->hb * d->wb * d->c_out * esz;
        const int rc = nv12_dispatch(a, d->out_dtype, (hipStream_t)stream);
        if (rc != YMI_OK) return rc;
    }
    return YMI_OK;
}

extern "C" int ymi_nv12_to_rgb(const void* y, const void* uv, int pitch_y, int pitch_uv, int h, int w, int matrix, int range, void* rgb, void* stream) {
    YMI_REQUIRE(y && uv && rgb, "ymi_nv12_to_rgb: null argument");
    YMI_REQUIRE(((uintptr_t)uv & 1) == 0, "ymi_nv12_to_rgb: the CbCr plane is not 2-byte aligned");
    YMI_REQUIRE(h >= 2 && w >= 2 && (h & 1) == 0 && (w & 1) == 0, "ymi_nv12_to_rgb: the frame is %dx%d: NV12 sides are even and >= 2", h, w);
    YMI_REQUIRE(pitch_y >= w && pitch_uv >= w && ((pitch_y | pitch_uv) & 1) == 0, "ymi_nv12_to_rgb: pitches %d / %d must be even and >= the width %d", pitch_y, pitch_uv, w);
    Nv12Coef k;
    YMI_REQUIRE(nv12_coef(matrix, range, k), "ymi_nv12_to_rgb: bad matrix %d / range %d", matrix, range);
    const int64_t total = (int64_t)h * ((w + 3) >> 2);
    const int dword_ok = (w & 3) == 0 && ((uintptr_t)rgb & 3) == 0;
    hipLaunchKernelGGL(nv12_to_rgb_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)y, (const unsigned char*)uv,
                       pitch_y, pitch_uv, h, w, k, (unsigned char*)rgb, dword_ok);
    return check_launch("nv12_to_rgb_kernel");
}

extern "C" int ymi_render_nv12(const ymi_render_nv12_desc* d, void* stream) {
    YMI_REQUIRE(d != nullptr, "ymi_render_nv12: null descriptor");
    YMI_REQUIRE(d->n >= 0 && d->k >= 0, "ymi_render_nv12: negative batch size %d or slab depth %d", d->n, d->k);
    YMI_REQUIRE(d->k <= YMI_RENDER_MAX_K, "ymi_render_nv12: slab depth %d above YMI_RENDER_MAX_K = %d", d->k, YMI_RENDER_MAX_K);
    if (d->n == 0) return YMI_OK;
    YMI_REQUIRE(d->y && d->uv && d->pitch && d->hw && d->lw && d->fs && d->boxes && d->scores && d->labels && d->counts && d->colors && d->status,
                "ymi_render_nv12: null buffer (planes, pitches, sizes, lw, fs, boxes, scores, labels, counts, colors or status)");
    YMI_REQUIRE(d->m >= 1 && d->num_classes >= 1, "ymi_render_nv12: %d colours (m) or %d classes, below 1", d->m, d->num_classes);
    YMI_REQUIRE((unsigned)d->matrix <= 1u && (unsigned)d->range <= 1u, "ymi_render_nv12: bad matrix %d / range %d", d->matrix, d->range);
    for (int c = 0; c < 3; ++c) YMI_REQUIRE(d->txt_color[c] >= 0 && d->txt_color[c] <= 255, "ymi_render_nv12: txt_color[%d] = %d outside 0..255", c, d->txt_color[c]);
    for (int i = 0; i < d->n; ++i) {   // every frame before the first launch
        const int rc = nv12_frame_ok("ymi_render_nv12", i, d->y[i], d->uv[i], d->hw[2 * i], d->hw[2 * i + 1], d->pitch[2 * i], d->pitch[2 * i + 1]);
        if (rc != YMI_OK) return rc;
        YMI_REQUIRE(d->lw[i] >= 1 && d->lw[i] <= 65535, "ymi_render_nv12: lw[%d] = %d outside [1, 65535]", i, d->lw[i]);
        YMI_REQUIRE(d->fs[i] >= 1 && d->fs[i] <= 65535, "ymi_render_nv12: fs[%d] = %d outside [1, 65535]", i, d->fs[i]);
    }
    const size_t lds = render_nv12_lds(d->k);
    for (int base = 0; base < d->n; base += NV12_MAX) {
        RenderNv12Args a;
        a.img_n = d->n - base < NV12_MAX ? d->n - base : NV12_MAX;
        int64_t blocks = 0;
        for (int i = 0; i < a.img_n; ++i) {
            const int h = d->hw[2 * (base + i)], w = d->hw[2 * (base + i) + 1];
            a.y[i] = (unsigned char*)d->y[base + i];
            a.uv[i] = (unsigned char*)d->uv[base + i];
            a.pitch[i][0] = d->pitch[2 * (base + i)];
            a.pitch[i][1] = d->pitch[2 * (base + i) + 1];
            a.hw[i][0] = h;
            a.hw[i][1] = w;
            a.lwfs[i][0] = d->lw[base + i];
            a.lwfs[i][1] = d->fs[base + i];
            blocks += (int64_t)cdiv(w, RD_TW) * cdiv(h, RD_TH);
            a.tile_end[i] = (int)blocks;
            YMI_REQUIRE(blocks < ((int64_t)1 << 31), "ymi_render_nv12: %lld workgroups in one launch", (long long)blocks);
        }
        a.boxes = d->boxes; a.scores = d->scores; a.labels = d->labels; a.counts = d->counts; a.names = d->names; a.colors = d->colors; a.status = d->status;
        a.img_base = base; a.k = d->k; a.m = d->m; a.num_classes = d->num_classes; a.draw_labels = d->draw_labels ? 1 : 0; a.draw_conf = d->draw_conf ? 1 : 0;
        a.txt = (uint32_t)d->txt_color[0] | ((uint32_t)d->txt_color[1] << 8) | ((uint32_t)d->txt_color[2] << 16);
        a.c.yoff = d->range == YMI_NV12_LIMITED ? 16 : 0;
        for (int j = 0; j < 9; ++j) a.c.c[j] = YCC_COEF[d->matrix][d->range][j];
        hipLaunchKernelGGL(render_nv12_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, a);
        const int rc = check_launch("render_nv12_kernel");
        if (rc != YMI_OK) return rc;
    }
    return YMI_OK;
}

extern "C" int ymi_crop_resize_nv12(const ymi_crop_nv12_desc* d, void* stream) {
    YMI_REQUIRE(d != nullptr, "ymi_crop_resize_nv12: null descriptor");
    YMI_REQUIRE(d->n >= 0 && d->k >= 0, "ymi_crop_resize_nv12: negative batch size %d or slab depth %d", d->n, d->k);
    YMI_REQUIRE(d->total && (d->n == 0 || (d->y && d->uv && d->pitch && d->hw && d->counts && (d->boxes || d->k == 0))),
                "ymi_crop_resize_nv12: null buffer (planes, pitches, sizes, boxes, counts or total)");
    YMI_REQUIRE(d->cap >= 0, "ymi_crop_resize_nv12: negative capacity %d", d->cap);
    YMI_REQUIRE(d->cap == 0 || (d->crops && d->index), "ymi_crop_resize_nv12: null output buffer (crops or index) with capacity %d", d->cap);
    YMI_REQUIRE(d->out_h >= 1 && d->out_w >= 1, "ymi_crop_resize_nv12: output size %d x %d below 1", d->out_h, d->out_w);
    YMI_REQUIRE(d->out_dtype == YMI_F16 || d->out_dtype == YMI_BF16 || d->out_dtype == YMI_F32, "ymi_crop_resize_nv12: unsupported out_dtype %d (F16 / BF16 / F32)", d->out_dtype);
    CropNv12Args a;
    YMI_REQUIRE(nv12_coef(d->matrix, d->range, a.c), "ymi_crop_resize_nv12: bad matrix %d / range %d", d->matrix, d->range);
    const float big = 3.0e38f;
    YMI_REQUIRE(fabsf(d->gain) <= big && fabsf(d->pad) <= big, "ymi_crop_resize_nv12: gain and pad must be finite");
    if (d->normalize)
        for (int c = 0; c < 3; ++c)
            YMI_REQUIRE(fabsf(d->mean[c]) <= big && fabsf(d->std[c]) <= big && d->std[c] != 0.f, "ymi_crop_resize_nv12: std[%d] is 0 (or mean / std not finite)", c);
    for (int i = 0; i < d->n; ++i) {
        const int rc = nv12_frame_ok("ymi_crop_resize_nv12", i, d->y[i], d->uv[i], d->hw[2 * i], d->hw[2 * i + 1], d->pitch[2 * i], d->pitch[2 * i + 1]);
        if (rc != YMI_OK) return rc;
    }
    YMI_REQUIRE((int64_t)d->n * d->k < ((int64_t)1 << 31) && (int64_t)d->out_h * d->out_w < ((int64_t)1 << 31), "ymi_crop_resize_nv12: n * k or out_h * out_w does not fit 31 bits");
    // the launch geometry of ymi_crop_resize: four pixels per thread where a row is a whole number of 4-pixel groups and the stores are aligned (YOLORT_AMD_CROP=pixel: one)
    const char* env = getenv("YOLORT_AMD_CROP");
    const size_t esz = d->out_dtype == YMI_F32 ? 4 : 2;
    const bool wide = d->out_w % 4 == 0 && ((uintptr_t)d->crops & (4 * esz - 1)) == 0 && !(env && !strcmp(env, "pixel"));
    const int64_t tiles = ((int64_t)d->out_h * (d->out_w / (wide ? 4 : 1)) + 255) / 256;
    a.boxes = d->boxes; a.counts = d->counts; a.crops = d->crops; a.index = d->index; a.total = d->total;
    a.n = d->n; a.k = d->k; a.cap = d->cap; a.out_h = d->out_h; a.out_w = d->out_w; a.tiles = (int)tiles;
    a.square = d->square ? 1 : 0; a.normalize = d->normalize ? 1 : 0;
    a.gain = d->gain; a.pad = d->pad;
    for (int c = 0; c < 3; ++c) { a.mean[c] = d->mean[c]; a.std[c] = d->std[c]; }
    for (int base = 0; base < d->n || base == 0; base += NV12_MAX) {   // every launch reads the WHOLE counts array: row offsets are global; the first one writes total[]
        a.img_base = base;
        a.img_n = d->n - base < NV12_MAX ? d->n - base : NV12_MAX;
        for (int i = 0; i < a.img_n; ++i) {
            a.y[i] = (const unsigned char*)d->y[base + i];
            a.uv[i] = (const unsigned char*)d->uv[base + i];
            a.pitch[i][0] = d->pitch[2 * (base + i)];
            a.pitch[i][1] = d->pitch[2 * (base + i) + 1];
            a.hw[i][0] = d->hw[2 * (base + i)];
            a.hw[i][1] = d->hw[2 * (base + i) + 1];
        }
        int64_t blocks = (int64_t)a.img_n * d->k * tiles;
        if (d->cap == 0 || blocks == 0) blocks = base == 0 ? 1 : 0;   // nothing to cut: one workgroup of the first launch still writes total[]
        if (blocks == 0) continue;
        YMI_REQUIRE(blocks < ((int64_t)1 << 31), "ymi_crop_resize_nv12: %lld workgroups in one launch", (long long)blocks);
        dim3 grid((unsigned)blocks), block(256);
        hipStream_t s = (hipStream_t)stream;
#define YMI_CROP_NV12(ODT_)                                                              \
    if (wide) hipLaunchKernelGGL((crop_resize_nv12_kernel<ODT_, 4>), grid, block, 0, s, a); \
    else hipLaunchKernelGGL((crop_resize_nv12_kernel<ODT_, 1>), grid, block, 0, s, a);
        switch (d->out_dtype) {
            case YMI_F16: YMI_CROP_NV12(YMI_F16) break;
            case YMI_BF16: YMI_CROP_NV12(YMI_BF16) break;
            default: YMI_CROP_NV12(YMI_F32) break;
        }
#undef YMI_CROP_NV12
        const int rc = check_launch("crop_resize_nv12_kernel");
        if (rc != YMI_OK) return rc;
    }
    return YMI_OK;
}
