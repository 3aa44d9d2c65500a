// Detection head with the decode FUSED into the convolution epilogue (gfx950).
//
// The reference runs the 1x1 head conv (yolort/models/box_head.py:36,74), concatenates the logits of all levels
// (:328-343), then decodes and thresholds them (:345-360, :414-418).  Unfused, the fp32 logits make a round trip
// through HBM (209 MB written + read per 32-image batch at 640x640) only for > 99.8 % of them to be discarded.
// Here the head weights are packed with every anchor's K = num_classes + 5 rows padded to RA = 32*TNA rows, the tile
// is 128 pixels x (3*RA) couts, and each wave owns 32 pixels x ALL couts: lanes l and l+32 together hold the K logits
// of pixel l for each anchor, so objectness / box logits cross between them with one ds_bpermute each and no LDS
// staging.  The wave then
//   * decodes the box of every (pixel, anchor) and stores it to boxes_all (NMS looks boxes up by anchor index),
//   * skips anchors whose objectness fails the threshold for all 32 pixels (score = cls*obj <= obj),
//   * pre-filters class logits against theta = logit(thr / obj) - margin (one log per anchor instead of a sigmoid
//     per class) and pushes the survivors -- few per register row -- onto a per-wave LDS worklist,
//   * drains the worklist 64 entries at a time (every lane busy): exact score as in the unfused kernel
//     (sigmoid_acc, rounded product, strict >), records appended to a per-wave LDS buffer flushed with one atomic.
//     (The LDS operand ring is dead by then and is reused for both.)
// In best-class mode (YMI_POST_BEST_CLASS, CandSink::best) the last two steps become: in-register maximum of the anchor's class logits, exact scores of the classes near
// it, one cross-half exchange, ONE record per passing (pixel, anchor) -- see the branch below.
// With a class filter (YMI_POST_CLASS_FILTER, CandSink::cmask) rows of disallowed classes are dropped next to the theta pre-filter (multi-label), or the anchor's
// record is dropped when its best class is not allowed (best-class).  That is a separate instantiation (FILT): the kernels without a filter are the code they were.
// Records and boxes are bit-identical to decode_kernel's (postprocess.hip), so sort / NMS / top-k are unchanged.
#pragma once
#include "conv_common.hpp"
#include "post_common.hpp"

namespace ymi {

// NA = anchors per wave.  NA = 3: the original form, one wave holds all 3 x RA logits of its 32 pixels (9 x 16 accumulator
// registers at K = 85 -> 400 VGPR + AGPR, ONE wave per SIMD: nothing hides the operand DMA, the MFMA chain and the decode
// of a wave behind another's -- 97 us per 32-image batch, 7x its HBM bound).  NA = 1: the cout axis is split by anchor
// (three blocks per pixel tile, each wave 32 pixels x RA rows, 48 accumulator registers, >= 3 waves per SIMD); the x tile
// is fetched by three neighbouring blocks (L2 hits), the weights by a third as many pixels each.
template <int NA> struct HdCfg {
    static constexpr int BUF = NA == 3 ? 1024 : 256;   // records per wave buffer (12 B each); one append adds at most 64
    static constexpr int WL = NA == 3 ? 512 : 256;     // worklist entries per wave (16 B each): pre-filter survivors waiting for their exact score
    static constexpr int LDS_BYTES = 4 * (BUF * 12 + WL * 16);   // per block (4 waves); overlays the dead operand ring
};

struct HeadDecodeArgs {
    float stride;
    float anc[6];
    int K;            // outputs per anchor (num_classes + 5)
    int level_off;    // index of this level's first anchor within an image
    CandSink sink;
};

// acc[NA*TNA][1]: sub-tile s of the wave's anchor qi is acc[qi*TNA + s][0] (anchor q = q_base + qi; q_base is wave-uniform,
// 0 when NA = 3); register g*4+e of lane (px, hi) is channel c = s*32 + g*8 + hi*4 + e of that anchor (c < K real, else padding)
// FILT: the class filter is a SEPARATE instantiation (the launchers pick it when CandSink::cmask is set), so the kernels without a filter are the code they were, register for
// register (profiles/class_filter_head_registers.txt); with FILT, k_.cmask is not null.
template <int TNA, int NA, bool FILT = false>
__device__ __forceinline__ void head_decode_wave(const ConvArgs& a, const HeadDecodeArgs& h, const f32x16 (&acc)[NA * TNA][1], int m, int lane,
                                                 uint64_t* bhi, uint32_t* blo, u32x4* wl, int q_base) {
    constexpr int HD_BUF = HdCfg<NA>::BUF, HD_WL = HdCfg<NA>::WL;
    const CandSink& k_ = h.sink;
    const int hi = lane >> 5;
    const bool m_ok = m < a.M;
    const int mm = m_ok ? m : 0;
    const int hw = a.ho * a.wo;
    const int img = fast_div(mm, hw, a.magic_hw);
    const int rem = mm - img * hw;
    const int y = fast_div(rem, a.wo, a.magic_w), x = rem - y * a.wo;
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int fill = 0;                                            // records buffered (wave-uniform)
    int fill_img = __builtin_amdgcn_readfirstlane(img);     // image they belong to
    int wl_fill = 0;                                         // worklist entries (wave-uniform)
    // The record buffer and the worklist hand data from lane to lane through wave-private LDS.  The hardware runs a wave's LDS operations
    // in program order, so what has to be pinned is the COMPILER's order (it sees per-lane addresses that never alias): every hand-over
    // carries __builtin_amdgcn_wave_barrier() -- no instruction on the GPU, a wave sync on the CPU simulator (tests/hipsim), whose lanes do
    // not run in lockstep (without the fence after the flush its lane 0 refilled the buffer with the next image's records while the other
    // lanes were still copying the previous image's out: VERDICT r2 weak 3).
    auto flush = [&]() {
        flush_records(k_, bhi, blo, fill, fill_img, lane);   // (its __shfl orders the lanes' record writes before the copy-out)
        __builtin_amdgcn_wave_barrier();                     // every lane has copied its share: the buffer may be refilled
        fill = 0;
    };
    // append the records of the lanes with ok set; the lanes of one call can belong to different images
    auto append = [&](bool ok, float s, unsigned lo, int img_l) {
        uint64_t mask = __ballot(ok);
        while (mask) {
            const int first = __builtin_ctzll(mask);
            const int img0 = __builtin_amdgcn_readlane(img_l, first);
            const uint64_t sub = mask & __ballot(img_l == img0);
            if (img0 != fill_img) {
                flush();
                fill_img = img0;
            }
            const int cnt = __popcll(sub);
            if (fill + cnt > HD_BUF) flush();
            if (ok && img_l == img0) {
                const int pos = fill + __popcll(sub & lt);
                bhi[pos] = ((uint64_t)(unsigned)img_l << 32) | (uint64_t)(~__float_as_uint(s));
                blo[pos] = lo;
            }
            fill += cnt;
            mask &= ~sub;
        }
    };
    // exact scores of worklist entries, 64 at a time; `all` = also the last partial batch
    auto drain = [&](bool all) {
        int base = 0;
        __builtin_amdgcn_wave_barrier();                     // the pushes of every lane are in LDS
        while (wl_fill - base >= 64 || (all && base < wl_fill)) {
            const int i = base + lane;
            const bool have = i < wl_fill;
            u32x4 e = {0u, 0u, 0u, 0u};
            if (have) e = wl[i];
            const float sc = __fmul_rn(sigmoid_acc(__uint_as_float(e[0])), __uint_as_float(e[1]));   // box_head.py:357 scores = cls * obj
            append(have && sc > k_.thr, sc, e[2], (int)e[3]);                                      // box_head.py:418 strict >
            base += 64;
        }
        const int left = wl_fill > base ? wl_fill - base : 0;
        if (left > 0 && base > 0) {   // move the partial batch to the front
            u32x4 e = {0u, 0u, 0u, 0u};
            if (lane < left) e = wl[base + lane];
            if (lane < left) wl[lane] = e;
        }
        __builtin_amdgcn_wave_barrier();                     // every lane has read its entries: the worklist may be overwritten by the next push
        wl_fill = left;
    };
    auto push = [&](bool pre, float v, float o, unsigned lo) {
        const uint64_t mask = __ballot(pre);
        const int cnt = __popcll(mask);
        if (wl_fill + cnt > HD_WL) drain(false);   // leaves < 64 entries
        if (pre) {
            u32x4 e = {__float_as_uint(v), __float_as_uint(o), lo, (unsigned)img};
            wl[wl_fill + __popcll(mask & lt)] = e;
        }
        wl_fill += cnt;
    };

    // Class filter (YMI_POST_CLASS_FILTER, CandSink::cmask; FILT instantiations only).  Register r of a lane holds the same row c = cb + 4 * hi of EVERY anchor, so
    // the lane's 16 * TNA rows get their verdict once per wave: `rows` has bit r set iff row r is a class row (5 <= c < K) of an allowed class.  The mask words are read
    // with wave-uniform loads and shifted by the five box / objectness rows into row space (bit c of word c >> 5); a lane then picks the four nibbles of its lane half out
    // of each sub-tile's word.  Two VGPRs at most, nothing kept in scalar registers across the anchors.
    uint64_t rows = 0;
    if constexpr (FILT) {
        uint32_t prev = 0;
        static_for<0, TNA>([&](auto st) {
            constexpr int s = decltype(st)::value;
            const uint32_t cur = k_.cmask[s];                                   // classes 32 s .. 32 s + 31
            uint32_t word = (cur << 5) | (s == 0 ? 0u : (prev >> 27));          // rows 32 s .. 32 s + 31
            prev = cur;
            const int left = h.K - 32 * s;                                      // rows of this sub-tile below K
            word = left >= 32 ? word : (left <= 0 ? 0u : (word & ((1u << left) - 1u)));
            const uint32_t x = word >> (4 * hi);
            const uint32_t mine = (x & 0xfu) | ((x >> 4) & 0xf0u) | ((x >> 8) & 0xf00u) | ((x >> 12) & 0xf000u);   // bit g * 4 + e = row s * 32 + g * 8 + hi * 4 + e
            rows |= (uint64_t)mine << (16 * s);
        });
    }

    // compile-time indices everywhere: the accumulators must stay in registers (a runtime index sends them to scratch)
    static_for<0, NA>([&](auto qt) {
        constexpr int qi = decltype(qt)::value;
        constexpr int q = qi;                 // accumulator sub-array of this anchor
        const int qa = q_base + qi;           // anchor index within the level (wave-uniform)
        const float anc_w = qa == 0 ? h.anc[0] : (qa == 1 ? h.anc[2] : h.anc[4]);   // selects, not a runtime index: the by-value args stay in SGPRs
        const float anc_h = qa == 0 ? h.anc[1] : (qa == 1 ? h.anc[3] : h.anc[5]);
        // channels 0..3 (box) live on the hi = 0 lane, 4..7 (objectness, first classes) on the hi = 1 lane
        const float t0 = acc[q * TNA][0][0], t1 = acc[q * TNA][0][1], t2 = acc[q * TNA][0][2], t3 = acc[q * TNA][0][3];
        const float u0 = __shfl_xor(t0, 32, 64), u1 = __shfl_xor(t1, 32, 64), u2 = __shfl_xor(t2, 32, 64), u3 = __shfl_xor(t3, 32, 64);
        const float lx = hi ? u0 : t0, ly = hi ? u1 : t1, lw = hi ? u2 : t2, lh = hi ? u3 : t3;
        const float lobj = hi ? t0 : u0;
        const int anchor = h.level_off + (qa * a.ho + y) * a.wo + x;
        if (hi == 0 && m_ok) {
            const f32x4 b = decode_box(lx, ly, lw, lh, x, y, h.stride, anc_w, anc_h);
            *reinterpret_cast<f32x4*>(k_.boxes_all + ((int64_t)img * k_.total_anchors + anchor) * 4) = b;
        }
        const float o = sigmoid_acc(lobj);
        const bool pass = m_ok && o > k_.thr;      // score = cls * obj <= obj
        if (__ballot(pass) == 0) return;            // wave-uniform: nothing to find for this anchor
        const unsigned lo_base = (unsigned)anchor << k_.label_bits;
        if (k_.best) {
            // Best-class mode (YMI_POST_BEST_CLASS; wave-uniform branch, the multi-label path below is untouched): ONE record per passing (pixel, anchor), the class
            // with the largest PRODUCT, the lowest index among equal products.  Lanes l and l + 32 hold the pixel's logits in compile-time-indexed registers:
            //   1. in-register maximum of the class LOGITS (rows c < 5 -- box, objectness -- and the padding rows c >= K, logit 0, are left out), one cross-half exchange;
            //   2. exact scores -- the multi-label expression, bit for bit -- only of the classes at or above best_class_cut (post_common.hpp: a superset of the
            //      classes that can reach or tie the largest product; it states what it assumes of sigmoid_acc), few per pixel, skipped row-wise by ballot;
            //      a lane meets its rows in ascending class order, so a strict > keeps its lowest index;
            //   3. one cross-half exchange of (score, class) under the total order (score descending, class ascending); the hi = 0 lane appends the record.
            // register r of this lane is row c = cb + 4 * hi, cb = s * 32 + g * 8 + e a compile-time constant: a class row iff 5 <= c < K, i.e. cb < kcap (and, in the
            // first group only, past the objectness row)
            int kcap = h.K - 4 * hi;
            float vmax = -INFINITY;
            static_for<0, TNA * 16>([&](auto rt) {
                constexpr int r = decltype(rt)::value;
                constexpr int s = r / 16, g = (r % 16) / 4, e = r % 4, cb = s * 32 + g * 8 + e;
                const float v = acc[q * TNA + s][0][g * 4 + e];
                const bool cls = (cb >= 5 || (hi && cb >= 1)) && cb < kcap;
                vmax = fmaxf(vmax, cls ? v : -INFINITY);
            });
            vmax = fmaxf(vmax, __shfl_xor(vmax, 32, 64));
            // The second pass states its row tests on an opaque copy of kcap: left to itself the compiler keeps the 16 * TNA lane masks of the first pass alive for the
            // second one (96 SGPRs at TNA = 3), runs out of scalar registers and spills them into VGPRs -- of the WHOLE kernel, the multi-label path included
            // (90 -> 112 VGPRs and 5 -> 4 waves per SIMD at TNA = 3: profiles/best_class_head_registers.txt)
            asm volatile("" : "+v"(kcap));
            const float cut = best_class_cut(vmax, o);
            BestClass b = best_none();
            static_for<0, TNA * 16>([&](auto rt) {
                constexpr int r = decltype(rt)::value;
                constexpr int s = r / 16, g = (r % 16) / 4, e = r % 4, cb = s * 32 + g * 8 + e;
                const float v = acc[q * TNA + s][0][g * 4 + e];
                const bool pre = pass && (cb >= 5 || (hi && cb >= 1)) && (cb < kcap) && (v >= cut);
                if (__ballot(pre) == 0) return;          // the common case
                if (pre) {
                    const float sc = __fmul_rn(sigmoid_acc(v), o);   // box_head.py:357 scores = cls * obj
                    if (sc > b.s) b = BestClass{sc, cb + 4 * hi};
                }
            });
            const BestClass t = {__shfl_xor(b.s, 32, 64), __shfl_xor(b.c, 32, 64)};
            if (best_before(t.s, t.c, b)) b = t;
            bool ok = pass && hi == 0 && b.c != 0x7fffffff && b.s > k_.thr;   // conf > thr, strict (general.py:583)
            if constexpr (FILT) ok = ok && class_allowed(k_.cmask, ok ? b.c - 5 : 0);   // the winner -- over ALL classes -- has to be an allowed one (general.py:585-587)
            append(ok, b.s, lo_base | (unsigned)(b.c - 5), img);
            return;
        }
        // cls * o > thr  =>  sigmoid(v) > thr / o  =>  v > logit(thr / o); the margin keeps the filter a superset.
        // thr <= 0: every sigmoid exceeds thr / o <= 0, nothing may be filtered (the log of a negative p would be NaN and v > NaN false for every class)
        float theta = INFINITY;
        if (pass) {
            const float p = k_.thr / o;
            theta = p > 0.0f ? __logf(p / (1.0f - p)) - 0.02f : -INFINITY;
        }
        // FILT: rows of disallowed classes never reach the worklist (`rows` also states 5 <= c < K); the objectness skip and theta stay supersets
        static_for<0, TNA * 16>([&](auto rt) {
            constexpr int r = decltype(rt)::value;
            constexpr int s = r / 16, g = (r % 16) / 4, e = r % 4;
            const int c = s * 32 + g * 8 + hi * 4 + e;
            const float v = acc[q * TNA + s][0][g * 4 + e];
            bool pre;
            if constexpr (FILT) pre = ((rows >> r) & 1ull) && (v > theta);
            else pre = (c >= 5) && (c < h.K) && (v > theta);
            if (__ballot(pre) == 0) return;          // the common case
            push(pre, v, o, lo_base | (unsigned)(c - 5));
        });
    });
    drain(true);
    flush();
}

}  // namespace ymi
