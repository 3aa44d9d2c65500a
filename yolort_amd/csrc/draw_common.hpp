// Device code shared by the drawing and cropping kernels over RGB images (render_kernel, crop_resize_kernel: csrc/preproc_pool.hip) and over NV12 frames
// (render_nv12_kernel, crop_resize_nv12_kernel: csrc/preproc_nv12.hip): the rectangle and tap arithmetic and the whole body of the crop with the SOURCE FETCH as its
// one template, the list-building phase of the renderer and THE decision of a pixel (which list entry decides it, and whether as outline, background or glyph).
// The rules are the contracts of include/yolort_amd.h (ymi_crop_resize, ymi_render); nothing here knows how an image is stored.
#pragma once
#include "common.hpp"

namespace ymi {

// ---------------------------------------------------------------------------------------------
// Detection crops
// ---------------------------------------------------------------------------------------------
// the rectangle of one detection, r = {x1, y1, x2, y2}; false = nothing to cut: a non-finite coordinate (r all zero) or an empty rectangle (r = the clipped corners)
__device__ __forceinline__ bool crop_rect(const float b[4], int H, int W, int square, float gain, float pad, int r[4]) {
    r[0] = r[1] = r[2] = r[3] = 0;
    const float lim = 3.0e38f;   // |v| <= lim is false for NaN and +-inf
    if (!(fabsf(b[0]) <= lim && fabsf(b[1]) <= lim && fabsf(b[2]) <= lim && fabsf(b[3]) <= lim)) return false;
    const float cx = __fdiv_rn(__fadd_rn(b[0], b[2]), 2.0f), cy = __fdiv_rn(__fadd_rn(b[1], b[3]), 2.0f);   // xyxy2xywh, general.py:397-400
    float w = __fsub_rn(b[2], b[0]), h = __fsub_rn(b[3], b[1]);
    if (square) { const float m = w > h ? w : h; w = m; h = m; }                                            // plots.py:550
    w = __fadd_rn(__fmul_rn(w, gain), pad);                                                                  // plots.py:551
    h = __fadd_rn(__fmul_rn(h, gain), pad);
    const float hw2 = __fdiv_rn(w, 2.0f), hh2 = __fdiv_rn(h, 2.0f);
    const float c[4] = {__fsub_rn(cx, hw2), __fsub_rn(cy, hh2), __fadd_rn(cx, hw2), __fadd_rn(cy, hh2)};     // xywh2xyxy, general.py:410-413
    if (!(fabsf(c[0]) <= lim && fabsf(c[1]) <= lim && fabsf(c[2]) <= lim && fabsf(c[3]) <= lim)) return false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // .long() truncates toward zero, clip_coords clamps the integer into [0, W] / [0, H]: the same as this, for every finite value
        const int hi = (i & 1) ? H : W;
        r[i] = c[i] <= 0.f ? 0 : (c[i] >= (float)hi ? hi : (int)c[i]);
    }
    return r[2] > r[0] && r[3] > r[1];   // an empty rectangle keeps the clipped corners the reference gives it (the index reports them); its crop is all zero
}

// scale_view_kernel's source taps of destination index d: indices i0, i1 inside [0, n_in), weight l1 of i1
__device__ __forceinline__ void crop_taps(float s, int d, int n_in, int& i0, int& i1, float& l1) {
    float f = fmaf(s, (float)d + 0.5f, -0.5f);
    f = f < 0.f ? 0.f : f;
    i0 = (int)f;
    i0 = i0 > n_in - 1 ? n_in - 1 : i0;
    i1 = i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
    l1 = f - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
}

// The crop of one workgroup.  Args: the by-value table of the launch (CropArgs, CropNv12Args: the fields read here are common to both).  Src: the source fetch --
// Src(a, li, H, W) binds image li of the launch, pixel(y, x) fetches (or addresses) source pixel (y, x) and chan(pixel, c) is its channel c as the float in [0, 1] the
// resize reads.
template <class Src, int ODT, int PX, class Args>
__device__ __forceinline__ void crop_resize_body(const Args& a) {
    const int kk = a.k > 0 ? a.k : 1;
    const int slot = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)slot * (unsigned)a.tiles);
    const int li = slot / kk, det = slot - li * kk;
    const int img = a.img_base + li;
    // exclusive prefix of min(counts, k) at `img`, the grand total and the own count: lane l takes images l, l + 64, ...; wave-uniform trip count
    int before = 0, all = 0, mine = 0, bad = 0;
    const int lane = threadIdx.x & 63;
    for (int i0 = 0; i0 < a.n; i0 += 64) {
        const int i = i0 + lane;
        const int c = i < a.n ? a.counts[i] : 0;
        const int cc = c < 0 ? 0 : (c > a.k ? a.k : c);
        bad |= (c != cc) ? 1 : 0;
        all += cc;
        before += i < img ? cc : 0;
        mine += i == img ? cc : 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        before += __shfl_xor(before, m);
        all += __shfl_xor(all, m);
        mine += __shfl_xor(mine, m);
        bad |= __shfl_xor(bad, m);
    }
    if (blockIdx.x == 0 && a.img_base == 0 && threadIdx.x == 0) {
        a.total[0] = all < a.cap ? all : a.cap;
        a.total[1] = (all > a.cap ? YMI_CROP_STATUS_CAPACITY : 0) | (bad ? YMI_CROP_STATUS_BAD_COUNT : 0);
    }
    if (li >= a.img_n || det >= mine) return;
    const int row = before + det;
    if (row >= a.cap) return;
    const int H = a.hw[li][0], W = a.hw[li][1];
    const float* bp = a.boxes + ((int64_t)img * a.k + det) * 4;
    const float b[4] = {bp[0], bp[1], bp[2], bp[3]};
    int r[4];
    const bool any = crop_rect(b, H, W, a.square, a.gain, a.pad, r);
    if (tile == 0 && threadIdx.x < 6) {
        const int t = (int)threadIdx.x;
        a.index[(int64_t)row * 6 + t] = t == 0 ? img : (t == 1 ? det : r[t - 2]);
    }
    const int wq = a.out_w / PX;
    const int q = tile * 256 + (int)threadIdx.x;
    if (q >= a.out_h * wq) return;
    const int y = q / wq, x = (q - y * wq) * PX;
    float v[PX][3];
#pragma unroll
    for (int p = 0; p < PX; ++p) v[p][0] = v[p][1] = v[p][2] = 0.f;
    if (any) {
        const int rh = r[3] - r[1], rw = r[2] - r[0];
        const float sy = (float)rh / (float)a.out_h, sx = (float)rw / (float)a.out_w;
        int y0, y1;
        float ly1;
        crop_taps(sy, y, rh, y0, y1, ly1);
        const float ly0 = 1.f - ly1;
        y0 += r[1];
        y1 += r[1];
        const Src src(a, li, H, W);
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            int x0, x1;
            float lx1;
            crop_taps(sx, x + p, rw, x0, x1, lx1);
            const float lx0 = 1.f - lx1;
            x0 += r[0];
            x1 += r[0];
            const float w00 = __fmul_rn(ly0, lx0), w01 = __fmul_rn(ly0, lx1), w10 = __fmul_rn(ly1, lx0), w11 = __fmul_rn(ly1, lx1);
            const typename Src::Pixel t00 = src.pixel(y0, x0), t01 = src.pixel(y0, x1), t10 = src.pixel(y1, x0), t11 = src.pixel(y1, x1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p00 = src.chan(t00, c), p01 = src.chan(t01, c);
                const float p10 = src.chan(t10, c), p11 = src.chan(t11, c);
                float val = fmaf(w11, p11, fmaf(w10, p10, fmaf(w00, p00, __fmul_rn(w01, p01))));
                if (a.normalize) val = __fdiv_rn(__fsub_rn(val, a.mean[c]), a.std[c]);
                v[p][c] = val;
            }
        }
    }
    const int64_t oplane = (int64_t)a.out_h * a.out_w;
    const int64_t o = (int64_t)row * 3 * oplane + (int64_t)q * PX;   // a plane is contiguous: pixel (y, x) is element y * out_w + x = q * PX
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (PX == 4 && ODT == YMI_F32) {
            const f32x4 w = {v[0][c], v[1][c], v[2][c], v[3][c]};
            *reinterpret_cast<f32x4*>((float*)a.crops + o + c * oplane) = w;
        } else if constexpr (PX == 4) {
            u32x2 w;
            w[0] = cvt_pk16<ODT>(f32x2{v[0][c], v[1][c]});
            w[1] = cvt_pk16<ODT>(f32x2{v[2][c], v[3][c]});
            *reinterpret_cast<u32x2*>((uint16_t*)a.crops + o + c * oplane) = w;
        } else if constexpr (ODT == YMI_F32) {
            ((float*)a.crops)[o + c * oplane] = v[0][c];
        } else {
            ((uint16_t*)a.crops)[o + c * oplane] = to16<ODT>(v[0][c]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Annotated images
// ---------------------------------------------------------------------------------------------
#include "render_font.hpp"

constexpr int RD_TW = 64, RD_TH = 16;
constexpr int RD_MAX_L = 27 + 1 + 5;   // the longest label: a 27-byte name, ' ', "-0.00"  (names = null: at most 10 digits)
struct RenderEntry {          // 32 bytes of LDS per listed detection
    int x0, y0, x1, y1;
    int ty;                   // top row of the label
    int label;
    uint32_t info;            // L | name length << 8 | score code << 16 (hundredths 0..100, 101: "?.??") | negative zero << 24
    uint32_t rgb;
};

// character `ci` of the label of entry e (ci < L)
__device__ __forceinline__ int render_char(const RenderEntry& e, int ci, const uint8_t* names) {
    const int nl = (int)((e.info >> 8) & 0xff);
    int ch;
    if (ci < nl) {
        if (names) {
            ch = names[(int64_t)e.label * YMI_RENDER_NAME_STRIDE + 1 + ci];
        } else {   // the class index in decimal: digit nl - 1 - ci counted from the units
            int v = e.label;
            for (int i = nl - 1 - ci; i > 0; --i) v /= 10;
            ch = '0' + v % 10;
        }
    } else {
        const int code = (int)((e.info >> 16) & 0xff), neg = (int)((e.info >> 24) & 1);
        int t = ci - nl - 1;   // -1: the blank
        if (t < 0) return ' ';
        if (neg) {
            if (t == 0) return '-';
            --t;
        }
        if (t == 1) return '.';
        if (code > 100) return '?';
        ch = '0' + (t == 0 ? code / 100 : (t == 2 ? code / 10 % 10 : code % 10));
    }
    return (ch < 32 || ch > 126) ? '?' : ch;
}

// Phase 1 of a rendering workgroup: the list of the detections of image `img` whose drawing extent meets the tile [tx0, tx0 + RD_TW) x [ty0, ty0 + RD_TH), IN SLOT
// ORDER -- the 256 threads walk the slots below the count, 256 a pass, and compact the hits with a wave ballot and a prefix over the four wave totals (wcnt: four
// ints of LDS).  store(position, entry) keeps an entry (every hit is stored exactly once, positions 0 .. n - 1); tile 0 of an image ORs the status bits into
// a.status.  Returns n.  Args: the launch's by-value table (RenderArgs, RenderNv12Args: the fields read here are common to both).
template <class Args, class Store>
__device__ __forceinline__ int render_list(const Args& a, int img, int tile, int tx0, int ty0, int fs, int* wcnt, Store store) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx1 = tx0 + RD_TW - 1, ty1 = ty0 + RD_TH - 1;   // the tile, inclusive
    const int craw = a.counts[img];
    const int cnt = craw < 0 ? 0 : (craw > a.k ? a.k : craw);
    int bits = craw < 0 ? YMI_RENDER_STATUS_STALE_ROW : (craw > a.k ? YMI_RENDER_STATUS_BAD_COUNT : 0);
    const int cw = 6 * fs, chh = 11 * fs;   // a character cell on the image
    const float lim = 16777216.0f;
    int nlist = 0;
    for (int base = 0; base < cnt; base += 256) {
        const int s = base + tid;
        bool hit = false;
        RenderEntry e = {};
        if (s < cnt) {
            const float* bp = a.boxes + ((int64_t)img * a.k + s) * 4;
            const float b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
            const bool finite = fabsf(b0) < lim && fabsf(b1) < lim && fabsf(b2) < lim && fabsf(b3) < lim;   // false for NaN and +-inf
            e.x0 = finite ? (int)b0 : 0; e.y0 = finite ? (int)b1 : 0; e.x1 = finite ? (int)b2 : -1; e.y1 = finite ? (int)b3 : -1;
            const bool drawn = finite && e.x1 >= e.x0 && e.y1 >= e.y0;
            e.ty = e.y0 - chh >= 0 ? e.y0 - chh : e.y0;
            // the outline's rectangle, or the background of the longest possible label, reaches the tile (tile 0 reads every label: it reports the bad ones)
            const bool box_in = e.x0 <= tx1 && e.x1 >= tx0 && e.y0 <= ty1 && e.y1 >= ty0;
            const bool lab_in = a.draw_labels && e.x0 <= tx1 && e.x0 + cw * RD_MAX_L + 1 >= tx0 && e.ty <= ty1 && e.ty + chh + 1 >= ty0;
            if (tile == 0 || (drawn && (box_in || lab_in))) {
                const int64_t lab = a.labels[(int64_t)img * a.k + s];
                if (lab < 0 || lab >= (int64_t)a.num_classes) {
                    bits |= YMI_RENDER_STATUS_BAD_LABEL;
                } else if (drawn) {
                    e.label = (int)lab;
                    int L = 0, nl = 0, code = 0, neg = 0;
                    if (a.draw_labels) {
                        if (a.names) {
                            nl = a.names[lab * YMI_RENDER_NAME_STRIDE];
                            nl = nl > YMI_RENDER_NAME_STRIDE - 1 ? YMI_RENDER_NAME_STRIDE - 1 : nl;
                        } else {
                            nl = 1;
                            for (int v = (int)lab; v >= 10; v /= 10) ++nl;
                        }
                        L = nl;
                        if (a.draw_conf) {
                            const float sc = a.scores[(int64_t)img * a.k + s];
                            if (sc >= 0.f && sc <= 1.f) {
                                code = (int)rint((double)sc * 100.0);   // the product is exact: 24 + 7 bits
                                neg = (int)(__float_as_uint(sc) >> 31);   // -0.0
                            } else {
                                code = 101;
                            }
                            L += 1 + neg + 4;
                        }
                    }
                    e.info = (uint32_t)L | ((uint32_t)nl << 8) | ((uint32_t)code << 16) | ((uint32_t)neg << 24);
                    const uint8_t* cp = a.colors + (lab % a.m) * 3;
                    e.rgb = (uint32_t)cp[0] | ((uint32_t)cp[1] << 8) | ((uint32_t)cp[2] << 16);
                    hit = box_in || (L > 0 && e.x0 <= tx1 && e.x0 + cw * L + 1 >= tx0 && e.ty <= ty1 && e.ty + chh + 1 >= ty0);
                }
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wcnt[wv] = __popcll(mask);
        __syncthreads();
        int off = nlist + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < 4; ++w) {
            off += w < wv ? wcnt[w] : 0;
            nlist += wcnt[w];
        }
        if (hit) store(off, e);
        __syncthreads();   // the list is complete up to nlist, and wcnt is free for the next pass
    }
    if (tile == 0) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) bits |= __shfl_xor(bits, m);
        if (lane == 0 && bits) atomicOr(a.status, (int32_t)bits);
    }
    return nlist;
}

// THE decision (phase 2): the thread's four adjacent pixels (x .. x + 3, y), of which those in `want` exist, walk the list from the lowest slot up; the first entry
// whose outline or label background covers a pixel decides it.  decided(p, i, e, glyph) is called once per decided pixel p with the list position i, the entry and
// whether a glyph bit of that entry's label is set there (the text colour) or not (the box colour).  Returns the mask of decided pixels.
template <class Decided>
__device__ __forceinline__ unsigned render_decide(const RenderEntry* list, int nlist, int x, int y, unsigned want, int lw, int fs, const uint8_t* names, Decided decided) {
    const int cw = 6 * fs, chh = 11 * fs;
    unsigned found = 0;
    for (int i = 0; i < nlist && found != want; ++i) {
        const RenderEntry e = list[i];
        const int L = (int)(e.info & 0xff);
        const int lx1 = e.x0 + cw * L + 1, ly1 = e.ty + chh + 1;   // the label background's last column and row
        const bool row_box = y >= e.y0 && y <= e.y1, row_lab = L > 0 && y >= e.ty && y <= ly1;
        if (!row_box && !row_lab) continue;
        const bool row_edge = y < e.y0 + lw || y > e.y1 - lw;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int xp = x + p;
            if ((found >> p) & 1u || !((want >> p) & 1u)) continue;
            const bool in_box = row_box && xp >= e.x0 && xp <= e.x1 && (row_edge || xp < e.x0 + lw || xp > e.x1 - lw);
            const bool in_lab = row_lab && xp >= e.x0 && xp <= lx1;
            if (!in_box && !in_lab) continue;
            bool glyph = false;
            if (in_lab && xp < lx1 - 1 && y < ly1 - 1) {   // inside [X0, X0 + w) x [ty, ty + h): a glyph cell
                const int dx = xp - e.x0, ci = dx / cw;
                const int gc = (dx - ci * cw) / fs, gr = (y - e.ty) / fs;
                const int ch = render_char(e, ci, names);
                glyph = ((YMI_RENDER_FONT[(ch - 32) * YMI_RENDER_FONT_H + gr] >> (YMI_RENDER_FONT_W - 1 - gc)) & 1) != 0;
            }
            decided(p, i, e, glyph);
            found |= 1u << p;
        }
    }
    return found;
}

}  // namespace ymi
