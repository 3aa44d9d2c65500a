// Detection post-process for gfx950: anchor decode + sigmoid + multi-label threshold compaction,
// stable radix sort, class-aware greedy NMS with wave64 ballot/shuffle, top-k + box rescale.
// Integer/index work is bit-exact w.r.t. the oracle contract; float
// arithmetic uses explicitly un-fused fp32 ops so that it follows torch's per-op rounding.
//
// Replaces: yolort/models/box_head.py:328-360 (_concat_pred_logits/_decode_pred_logits),
//           :414-427 (per-image threshold / batched_nms / top-k loop), yolort/models/_utils.py:59-60,
//           yolort/models/anchor_utils.py:19-60 (grids/shifts in closed form),
//           yolort/models/transform.py:354-367 (scale_coords).
//
// Record format (96 bits): hi = img << 32 | ~score_bits (u64), lo = cand = anchor << L | label (u32)
// with L = label bits.  Sorting records ascending by (hi, lo) gives, per image, score descending
// with ties in candidate order (anchor asc, class asc) == a stable descending sort of the
// reference's torch.where order (box_head.py:418).  ~score_bits descends only for non-negative floats: that is the range of the in-plan producers
// (decode_kernel, the head epilogue: sigmoid * sigmoid above a threshold), whose records are bit-inverted back into the score by the top-k gather.  The stand-alone
// ymi_batched_nms takes ANY non-NaN float score (torchvision's contract) and builds its key with nms_score_key instead.
//
// Best-class mode (YMI_POST_BEST_CLASS in ymi_post_desc.flags; Python: multi_label=False).  The default above is yolort's multi-label PostProcess; this is the contract of
// ultralytics' non_max_suppression(..., multi_label=False) (yolort/v5/utils/general.py:572-583, used by AutoShape), under which checkpoints ingested with load_from_yolov5
// were trained and evaluated: per anchor conf = max_c s_c with s_c = fmul_rn(sigmoid(cls_c), sigmoid(obj)) -- the multi-label score, bit for bit --, label = the lowest class
// with s_c == conf (torch.max(1)), candidate iff conf > score_thresh (strict), record lo = anchor << L | label: at most one record per anchor, status[4] = passing anchors.
// Only the candidate producers know the mode (CandSink::best: decode_kernel here, the head epilogue in head_decode.hpp); sort (ties by anchor), class-aware NMS, top-k,
// rescale, slab and status words are the ones above.  num_classes == 1: bit-identical to the default; thresholds <= 0: every anchor yields its best class.
// Differences from ultralytics: the NMS is the true class-aware NMS of this file, not boxes offset by 4096 pixels per class; no max_nms = 30000 cut of the candidates;
// scores stay fp32.
//
// Class filter (YMI_POST_CLASS_FILTER in ymi_post_desc.flags; Python: classes=[...]; ultralytics' non_max_suppression(..., classes=...), yolort/v5/utils/general.py:585-587).
// The set of allowed classes is a bit set in the workspace (Workspace::cmask, written by ymi_post_set_classes).  Only the candidate producers read it (CandSink::cmask:
// decode_kernel here, the head epilogue in head_decode.hpp): multi-label mode writes a record for a passing (anchor, class) pair only if the class is allowed; best-class
// mode takes the best class over ALL classes as before and writes the anchor's record only if that class is allowed.  Sort, NMS (class-aware or agnostic), top-k, rescale,
// slab and status words see fewer records and are unchanged; status[4] counts what was produced after the filter.
//
// Class-agnostic NMS (YMI_POST_AGNOSTIC in ymi_post_desc.flags; Python: agnostic=True; stand-alone: ymi_nms).  Candidates, sort, top-k, rescale, slab, status words and the
// labels of the kept detections are those above; only the suppression changes: one greedy NMS over all candidates of an image (torchvision.ops.nms on the unshifted boxes,
// ultralytics' agnostic=True).  The host keys P with label 0 -- P is G's order, a segment is an image -- and nms_block_kernel (section 3b) walks each segment with a workgroup.
#include "post_common.hpp"
#include <cstdlib>
#include <cstring>

namespace ymi {


// ------------------------------------------------------------------------------------------
// 1. decode + threshold.  One wave per feature-map pixel: its 3 x K logits are contiguous in the
//    NHWC fp32 head output, so the wave reads them with coalesced float4 loads (lane l holds
//    channels 4l..4l+3).  Objectness is broadcast with wave shuffles; since cls < 1,
//    score = cls*obj > thr requires obj > thr, so pixels whose three anchors all fail that test
//    skip the class work (the common case).
// ------------------------------------------------------------------------------------------
struct DecodeArgs {
    const float* logits;
    int h, w, cs;          // level geometry, channel stride
    float stride;
    float anc[6];
    int n, K;              // images, outputs per anchor (num_classes + 5)
    int level_off;         // index of this level's first anchor within an image
    CandSink sink;
};

constexpr int DEC_PIX_PER_WAVE = 8;     // pixels walked by one wave
constexpr int DEC_BUF = 512;            // candidate records buffered per wave in LDS before ONE global atomic

// a view's box back on the full canvas (_descale_pred, yolo.py:181-197): y' = y / scale, x' = x / scale, or mirrored x1' = W - x2 / scale, x2' = W - x1 / scale; every
// operation an explicitly rounded fp32 one
__device__ __forceinline__ f32x4 descale_box(const f32x4 b, float scale, float flip_w) {
    const float x1 = __fdiv_rn(b[0], scale), y1 = __fdiv_rn(b[1], scale), x2 = __fdiv_rn(b[2], scale), y2 = __fdiv_rn(b[3], scale);
    f32x4 o = {x1, y1, x2, y2};
    if (flip_w > 0.f) {
        o[0] = __fsub_rn(flip_w, x2);
        o[2] = __fsub_rn(flip_w, x1);
    }
    return o;
}

// The one body of decode_kernel (VIEW = false) and decode_view_kernel (VIEW = true: section 1b; `scale` and `flip_w` are read only there).  The two entry points declare
// the record buffers -- (4 waves, DEC_BUF) each, in LDS -- and pass them in.
template <bool VIEW>
__device__ __forceinline__ void decode_body(const DecodeArgs& a, float scale, float flip_w, uint64_t* buf_hi, uint32_t* buf_lo) {
    // One wave walks DEC_PIX_PER_WAVE consecutive pixels.  Candidates are appended to a per-wave LDS
    // buffer and flushed with a single atomicAdd on the global counter (one hot word saturates at
    // ~88 atomics/us: one atomic per pixel made this kernel atomic-bound).
    const CandSink& k_ = a.sink;
    const int lane = threadIdx.x & 63;
    const int wl = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * 4 + wl;
    const int64_t npix = (int64_t)a.n * a.h * a.w;
    const int hw = a.h * a.w;
    const int nch = 3 * a.K;
    const int npass = cdiv(nch, 256);
    uint64_t* bhi = buf_hi + wl * DEC_BUF;
    uint32_t* blo = buf_lo + wl * DEC_BUF;
    int fill = 0;      // records in the LDS buffer (wave-uniform)
    int fill_img = 0;  // image the buffered records belong to (per-image path flushes on image change)

    auto flush = [&]() {
        flush_records(k_, bhi, blo, fill, fill_img, lane);
        // every lane has copied its share before the buffer is refilled: no instruction on the GPU (a wave's LDS accesses stay in order), a wave sync on the CPU
        // simulator (tests/hipsim), whose lanes do not run in lockstep -- the flush in the MIDDLE of a pixel (more than DEC_BUF records: nc >= 171) is followed by
        // the record writes without any shuffle in between, and its lane 0 overwrote records the other lanes had not copied yet (cf. head_decode.hpp)
        __builtin_amdgcn_wave_barrier();
        fill = 0;
    };

    for (int pp = 0; pp < DEC_PIX_PER_WAVE; ++pp) {
        const int64_t pix = wave * DEC_PIX_PER_WAVE + pp;
        if (pix >= npix) break;
        const int img = (int)(pix / hw);
        const int rem = (int)(pix - (int64_t)img * hw);
        const int y = rem / a.w, x = rem - y * a.w;
        const float* row = a.logits + pix * a.cs;
        float obj[3];
        bool any_obj = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            obj[k] = sigmoid_acc(row[k * a.K + 4]);
            any_obj |= obj[k] > k_.thr;
        }
        if (lane < 3) {
            const float* r = row + lane * a.K;
            f32x4 b = decode_box(r[0], r[1], r[2], r[3], x, y, a.stride, a.anc[2 * lane], a.anc[2 * lane + 1]);
            if constexpr (VIEW) b = descale_box(b, scale, flip_w);
            const int anchor = a.level_off + (lane * a.h + y) * a.w + x;
            *reinterpret_cast<f32x4*>(k_.boxes_all + ((int64_t)img * k_.total_anchors + anchor) * 4) = b;
        }
        if (!any_obj) continue;
        if (fill + (k_.best ? 3 : nch) > DEC_BUF || img != fill_img) flush();   // a pixel yields at most nch - 15 records (best-class mode: one per anchor)
        fill_img = img;
        if (k_.best) {
            // Best-class mode (wave-uniform branch): per anchor whose objectness passes, every lane keeps the best (score, class) of the channels it holds -- over all
            // passes, so nch > 256 needs nothing else -- then a butterfly over the 64 lanes leaves the anchor's best pair in every lane.  "Best" is a total order
            // (score descending, class ascending): the lowest class among equal PRODUCTS wins whatever the lane order.  Lane 0 writes the (at most three) records.
            BestClass b0 = best_none(), b1 = best_none(), b2 = best_none();
            for (int p = 0; p < npass; ++p) {
                const int c0 = (p * 64 + lane) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (c0 + 3 < nch) v = *reinterpret_cast<const f32x4*>(row + c0);
                else
                    for (int e = 0; e < 4; ++e)
                        if (c0 + e < nch) v[e] = row[c0 + e];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = c0 + e;
                    const int k = c / a.K, cls = c - k * a.K - 5;
                    const float o = k == 0 ? obj[0] : (k == 1 ? obj[1] : obj[2]);
                    if (c < nch && cls >= 0 && o > k_.thr) {
                        const float s = __fmul_rn(sigmoid_acc(v[e]), o);   // the multi-label score, bit for bit
                        BestClass& b = k == 0 ? b0 : (k == 1 ? b1 : b2);
                        if (best_before(s, cls, b)) b = BestClass{s, cls};
                    }
                }
            }
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (!(obj[k] > k_.thr)) continue;            // wave-uniform: every lane computed the same objectness
                BestClass& b = k == 0 ? b0 : (k == 1 ? b1 : b2);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const BestClass t = {__shfl_xor(b.s, d, 64), __shfl_xor(b.c, d, 64)};
                    if (best_before(t.s, t.c, b)) b = t;
                }
                // conf > thr, strict (general.py:583); YMI_POST_CLASS_FILTER: the best class -- taken over ALL classes -- has to be an allowed one (general.py:585-587)
                if (b.c != 0x7fffffff && b.s > k_.thr && (k_.cmask == nullptr || class_allowed(k_.cmask, b.c))) {
                    if (lane == 0) {
                        const int anchor = a.level_off + (k * a.h + y) * a.w + x;
                        bhi[fill + cnt] = ((uint64_t)(unsigned)img << 32) | (uint64_t)(~__float_as_uint(b.s));
                        blo[fill + cnt] = ((unsigned)anchor << k_.label_bits) | (unsigned)b.c;
                    }
                    ++cnt;
                }
            }
            fill += cnt;
            continue;
        }
        for (int p = 0; p < npass; ++p) {
            const int c0 = (p * 64 + lane) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c0 + 3 < nch) v = *reinterpret_cast<const f32x4*>(row + c0);
            else
                for (int e = 0; e < 4; ++e)
                    if (c0 + e < nch) v[e] = row[c0 + e];
            float sc[4];
            unsigned cand[4];
            int cnt = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + e;
                const int k = c / a.K, cls = c - k * a.K - 5;
                bool ok = (c < nch) && (cls >= 0);
                float s = 0.f;
                if (ok) {
                    const float o = k == 0 ? obj[0] : (k == 1 ? obj[1] : obj[2]);
                    s = __fmul_rn(sigmoid_acc(v[e]), o);  // box_head.py:357 scores = cls * obj
                    ok = s > k_.thr;                       // box_head.py:418 strict >
                    if (k_.cmask != nullptr) ok = ok && class_allowed(k_.cmask, cls);   // YMI_POST_CLASS_FILTER (wave-uniform pointer test)
                }
                sc[e] = s;
                const int anchor = a.level_off + (k * a.h + y) * a.w + x;
                cand[e] = ((unsigned)anchor << k_.label_bits) | (unsigned)(cls < 0 ? 0 : cls);
                if (!ok) cand[e] = 0xffffffffu;
                cnt += ok ? 1 : 0;
            }
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d, 64);
                if (lane >= d) incl += t;
            }
            const int total = __shfl(incl, 63, 64);
            if (total == 0) continue;
            if (fill + total > DEC_BUF) flush();   // only reachable when nch > DEC_BUF (many classes)
            int pos = fill + incl - cnt;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (cand[e] != 0xffffffffu) {
                    if (pos < DEC_BUF) {
                        bhi[pos] = ((uint64_t)(unsigned)img << 32) | (uint64_t)(~__float_as_uint(sc[e]));
                        blo[pos] = cand[e];
                    }
                    ++pos;
                }
            }
            fill += total;
            if (fill > DEC_BUF) fill = DEC_BUF;   // unreachable for total <= DEC_BUF; guards the buffer
        }
    }
    flush();
}

__global__ __launch_bounds__(256) void decode_kernel(const DecodeArgs a) {
    __shared__ uint64_t buf_hi[4][DEC_BUF];
    __shared__ uint32_t buf_lo[4][DEC_BUF];
    decode_body<false>(a, 1.f, 0.f, &buf_hi[0][0], &buf_lo[0][0]);
}

// ------------------------------------------------------------------------------------------
// 1b. decode + threshold of ONE VIEW of augmented inference (ymi_post_decode_view; ultralytics' _forward_augment, yolort/v5/models/yolo.py:152-163): decode_body<true>.
//     A view changes two things, both in the three box lanes: the decoded corners are brought back to the full canvas (descale_box), and `level_off` already holds the
//     view's anchor base plus the kept levels in front of this one, so records and boxes land in the view's range of the concatenated anchor axis (torch.cat(y, 1) after
//     _clip_augmented).
// ------------------------------------------------------------------------------------------
struct DecodeViewArgs {
    DecodeArgs d;
    float scale;           // the view's scale (boxes are divided by it)
    float flip_w;          // > 0: the view was mirrored left-right, the full canvas width W as a float; 0: not mirrored
};

__global__ __launch_bounds__(256) void decode_view_kernel(const DecodeViewArgs va) {
    __shared__ uint64_t buf_hi[4][DEC_BUF];
    __shared__ uint32_t buf_lo[4][DEC_BUF];
    decode_body<true>(va.d, va.scale, va.flip_w, &buf_hi[0][0], &buf_lo[0][0]);
}

__global__ void finalize_count_kernel(int* status, int cap) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (status[ST_NCAND] > cap) status[ST_OVERFLOW] = 1;
    }
}

__device__ __forceinline__ int ncand(const int* status, int cap) {
    const int n = status[ST_NCAND];
    return n < cap ? n : cap;
}

// ------------------------------------------------------------------------------------------
// 2. LSD radix sort, 8 bits per pass, stable.  Three kernels per pass (histogram / scan / scatter).
//    The record count lives on the device (no host sync): blocks past the end exit at once.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned digit_of(uint64_t hi, uint32_t lo, int shift) {
    return shift < 32 ? (lo >> shift) & 0xffu : (unsigned)(hi >> (shift - 32)) & 0xffu;
}

__global__ __launch_bounds__(256) void radix_hist_kernel(const uint64_t* hi, const uint32_t* lo, const int* status, int cap, int shift, uint32_t* hist) {
    __shared__ unsigned cnt[256];
    const int n = ncand(status, cap);
    const int base = blockIdx.x * SORT_ITEMS;
    if (base >= n) return;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int end = min(n, base + SORT_ITEMS);
    for (int i = base + threadIdx.x; i < end; i += 256) atomicAdd(&cnt[digit_of(hi[i], lo[i], shift)], 1u);
    __syncthreads();
    hist[(int64_t)blockIdx.x * 256 + threadIdx.x] = cnt[threadIdx.x];
}

// One block per digit d (256 blocks): exclusive scan of hist[b][d] over the blocks b of the pass,
// 256 entries per sweep (wave shuffles + LDS), total of the digit left in tot[d].  The scatter
// kernel turns tot[] into digit bases itself (a 256-value LDS scan), so the serial chain of the
// classic single-block scan is gone.
__global__ __launch_bounds__(256) void radix_scan_kernel(const int* status, int cap, uint32_t* hist, uint32_t* tot) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned carry_s;
    const int n = ncand(status, cap);
    const int nblk = cdiv(n, SORT_ITEMS);
    const int d = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += 256) {
        const int b = b0 + t;
        const unsigned c = b < nblk ? hist[(int64_t)b * 256 + d] : 0u;
        unsigned incl = c;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned v = __shfl_up(incl, s, 64);
            if (lane >= s) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned off = carry_s;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (b < nblk) hist[(int64_t)b * 256 + d] = off + incl - c;
        __syncthreads();
        if (t == 255) carry_s = off + incl;
        __syncthreads();
    }
    if (t == 0) tot[d] = carry_s;
}

// scatter: wave w of the block owns the contiguous records [base + w*512, +512), 8 rounds of 64.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t* hi_in, const uint32_t* lo_in, uint64_t* hi_out, uint32_t* lo_out,
                                                            const int* status, int cap, int shift, const uint32_t* hist, const uint32_t* tot) {
    __shared__ unsigned wave_hist[4][256];
    __shared__ unsigned wave_base[4][256];
    __shared__ unsigned dsum[256];
    const int n = ncand(status, cap);
    const int base = blockIdx.x * SORT_ITEMS;
    if (base >= n) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 1024; i += 256) (&wave_hist[0][0])[i] = 0;
    {   // digit bases: inclusive scan of the 256 digit totals (Hillis-Steele in LDS)
        const int d = threadIdx.x;
        const unsigned mine = tot[d];
        dsum[d] = mine;
        __syncthreads();
        for (int st = 1; st < 256; st <<= 1) {
            const unsigned v = d >= st ? dsum[d - st] : 0u;
            __syncthreads();
            dsum[d] += v;
            __syncthreads();
        }
        dsum[d] -= mine;  // exclusive
    }
    __syncthreads();
    uint64_t rhi[8];
    uint32_t rlo[8];
    unsigned dig[8];
    uint64_t peers[8];
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int i = base + wave * 512 + r * 64 + lane;
        const bool valid = i < n;
        rhi[r] = valid ? hi_in[i] : 0;
        rlo[r] = valid ? lo_in[i] : 0;
        const unsigned dg = valid ? digit_of(rhi[r], rlo[r], shift) : 0x100u;  // 0x100 = invalid marker
        dig[r] = dg;
        // peer mask: lanes of this round with the same digit
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bm = __ballot((dg >> b) & 1u);
            m &= ((dg >> b) & 1u) ? bm : ~bm;
        }
        peers[r] = valid ? m : 0ull;
        if (valid && (m & lt) == 0) wave_hist[wave][dg] += __popcll(m);  // leader lane of the peer group
        // (distinct digits -> distinct LDS addresses; rounds are sequential within the wave)
    }
    __syncthreads();
    {
        const int d = threadIdx.x;
        unsigned run = hist[(int64_t)blockIdx.x * 256 + d] + dsum[d];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            wave_base[w][d] = run;
            run += wave_hist[w][d];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (dig[r] != 0x100u) {
            const unsigned rank = __popcll(peers[r] & lt);
            const unsigned dst = wave_base[wave][dig[r]] + rank;
            hi_out[dst] = rhi[r];
            lo_out[dst] = rlo[r];
        }
        // make every lane's read of wave_base[..] precede the leaders' update for this round
        __builtin_amdgcn_wave_barrier();
        if (dig[r] != 0x100u && (peers[r] & lt) == 0) wave_base[wave][dig[r]] += __popcll(peers[r]);
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------
// 2b. per-image sort in LDS (the common case: <= 16384 candidates per image).  decode appended each
//     image's records to its own region, so ONE launch (a 1024-thread block per image) replaces the
//     ten three-kernel radix passes: bitonic sort of the unique 64-bit keys (~score << 32 | cand)
//     gives the G order (score descending, ties by candidate index), a second bitonic sort of
//     (label << 32 | rank) gives the per-class P order the NMS walks.  G and P are written compactly
//     (image offsets = prefix of the counts), exactly as the radix path leaves them.
// ------------------------------------------------------------------------------------------
constexpr int IMG_SORT_MAX = 16384;

__device__ __forceinline__ void bitonic_sort_lds(uint64_t* key, int np2) {
    // Compare-exchange steps with distance j < chunk stay inside one wave's contiguous chunk of the array, so they need
    // no block-wide barrier (the wave's own LDS accesses are ordered): with 16 waves on 4096 keys that is 68 of the 78
    // steps -- the sort was barrier-latency bound (~1.5 us per __syncthreads of 16 waves), not work bound.
    // Small arrays (the common case: ~1000 candidates per image at score_thresh 0.25) keep 128-key chunks on the first
    // np2 / 128 waves and leave the others idle: with 16 x 64-key chunks every one of the 55 steps of a 1024-key sort was a
    // 1024-thread barrier (197 us for two sorts); 8 x 128 leaves 6 block-level steps.
    const int nwaves = blockDim.x >> 6;
    const int min_chunk = np2 < 128 ? np2 : 128;
    const int chunk = np2 / nwaves >= min_chunk ? np2 / nwaves : min_chunk;   // keys per wave (power of two)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 2; k <= np2; k <<= 1) {
        int j = k >> 1;
        for (; j > 0 && j >= chunk; j >>= 1) {   // partners in other waves' chunks
            for (int i = threadIdx.x; i < np2; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t x = key[i], y = key[ixj];
                    const bool asc = (i & k) == 0;
                    if ((x > y) == asc) { key[i] = y; key[ixj] = x; }
                }
            }
            __syncthreads();
        }
        if (j > 0) {                              // the remaining distances: this wave sorts within its own chunk
            uint64_t* mine = key + wave * chunk;
            const int base = wave * chunk;
            const bool active = base < np2;       // waves past the array idle (wave-uniform)
            for (; active && j > 0; j >>= 1) {
                for (int t = lane; t < chunk; t += 64) {
                    const int txj = t ^ j;
                    if (txj > t) {
                        const uint64_t x = mine[t], y = mine[txj];
                        const bool asc = ((base + t) & k) == 0;
                        if ((x > y) == asc) { mine[t] = y; mine[txj] = x; }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();                      // next phase starts with cross-chunk distances (or the sort is done)
        }
    }
}

// number of keys of the sorted run `run[0..len)` that are < key (keys are unique)
__device__ __forceinline__ int lower_bound_u64(const uint64_t* run, int len, uint64_t key) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (run[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sorts keys[0..n) (HBM, unique 64-bit keys) ascending into dst order: runs of up to `lds_keys` keys are
// bitonic-sorted in LDS and written back; with more than one run every key's final rank is its rank
// in its own run plus its lower_bound in every other run (merge by ranking, fully parallel).
// rank_out[i] receives the final rank of the key stored at position i after the run sort.
__device__ void sort_runs(uint64_t* keys, int n, uint64_t* lds_key, int lds_keys, uint32_t* rank_out) {
    const int nruns = (n + lds_keys - 1) / lds_keys;
    for (int r = 0; r < nruns; ++r) {
        const int r0 = r * lds_keys;
        const int len = n - r0 < lds_keys ? n - r0 : lds_keys;
        int np2 = 64;
        while (np2 < len) np2 <<= 1;
        for (int i = threadIdx.x; i < np2; i += blockDim.x) lds_key[i] = i < len ? keys[r0 + i] : ~0ull;
        __syncthreads();
        bitonic_sort_lds(lds_key, np2);
        for (int i = threadIdx.x; i < len; i += blockDim.x) keys[r0 + i] = lds_key[i];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = i / lds_keys;
        int rank = i - r * lds_keys;
        if (nruns > 1) {
            const uint64_t k = keys[i];
            for (int q = 0; q < nruns; ++q) {
                if (q == r) { rank += 0; continue; }
                const int q0 = q * lds_keys;
                const int qlen = n - q0 < lds_keys ? n - q0 : lds_keys;
                rank += lower_bound_u64(keys + q0, qlen, k);
            }
            // ranks of earlier runs' elements are already counted through lower_bound; add nothing else
        }
        rank_out[i] = (uint32_t)rank;
    }
    __syncthreads();
}

// Score-prefix selection (per-image path).  Greedy NMS decides each box from higher-scored boxes only, and the
// output keeps the K best survivors: if a score-ordered prefix of an image's candidates already yields K survivors,
// candidates behind it cannot change the result.  For an image with more than 1.5 * sel_t records this kernel keeps
// the records of the best linear score bins (1/4096 wide) that together hold >= sel_t records, compacts them to the
// front of the image's region and flags the image as truncated; gather_topk_kernel raises YMI_STATUS_PREFIX_SHORT
// if such an image ends with fewer than K survivors (the host then re-runs with YMI_POST_EXACT_FULL).
constexpr int SEL_BINS = 4096;
constexpr int RANK_MAX = 6144;   // images with at most this many records (after the prefix selection) are sorted by multi-block ranking

__device__ __forceinline__ int score_bin(uint64_t hi) {
    const float s = __uint_as_float(~(uint32_t)hi);
    const int b = (int)((1.0f - s) * (float)SEL_BINS);
    return b < 0 ? 0 : (b >= SEL_BINS ? SEL_BINS - 1 : b);
}

// histogram increment with the saturated case in mind: when every valid lane of the wave holds the SAME bin (thousands of records with equal or
// near-equal scores: the case the refinement below exists for) one lane adds the wave's count -- 64 lanes hammering one LDS address serialise
__device__ __forceinline__ void hist_add(int* hist, int bin, bool valid) {
    const uint64_t mv = __ballot(valid);
    if (mv == 0ull) return;
    const int first = __builtin_ctzll(mv);
    const int b0 = __builtin_amdgcn_readlane(bin, first);
    const uint64_t same = __ballot(valid && bin == b0);
    if (same == mv) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[b0], __popcll(same));
    } else if (valid) {
        atomicAdd(&hist[bin], 1);
    }
}

// Multi-block form of the selection's two streaming passes (round 3).  ONE block per image streams the image twice -- histogram, then the
// in-place compaction -- and at 8 images of 218 k records (yolov5l6 at 1280 x 1280) that is 8 CUs moving 35 MB: 0.39 ms of a 0.52 ms post-process.
// For images with regions of >= 2 * SEL_SLICE records the passes are split over slices of SEL_SLICE records:
//   sel_hist_kernel      (slices x images)  LDS histogram of a slice, non-empty bins added to the image's global histogram
//   select_prefix_kernel (images)           the cut from that histogram; unless the boundary bin is fat (refinement: the one-block path above stays
//                                           in charge of the whole image) it only PUBLISHES the cut: mode 1, b*, and the count it implies
//   sel_compact_kernel   (slices x images)  records of bins <= b* appended to the image's staging region (arrays [1], free until scatter_ranks)
//                                           at positions handed out by one atomic per wave -- their order does not matter: every consumer ranks
//                                           by the records' unique keys
//   sel_copyback_kernel                     staging -> the front of the image's own region (<= max(RANK_MAX, sel_t) records: blocks stride over the selection)
// An in-place multi-block compaction would overwrite records of slice 0 that its block may not have read yet.
// A fat boundary bin (saturated scores: the benchmark configurations' synthetic weights put most images there) is refined by the same exact radix selection as
// in the one-block kernel, as a fixed LADDER of six (sel_rhist_kernel, sel_rpick_kernel) pairs -- 11 key bits per level; the launch sequence does not depend on the
// data, levels an image does not need return at once.  C5 (8 images of 218 k records): post-process 0.52 -> 0.23 ms; C3 (64 images): 0.90 -> 0.73 ms, but the extra
// passes cost the pipelined throughput 1 %, so batches of 32 or more images keep the one-block form by default (profiles/r03z12_sel_ladder_ab.txt).
constexpr int SEL_SLICE = 16384;

__global__ __launch_bounds__(1024) void sel_hist_kernel(const uint64_t* in_hi, const int* img_count, int cap_img, int sel_t, int* ghist) {
    __shared__ int hist[SEL_BINS];
    const int img = blockIdx.y;
    const int raw = img_count[img];
    const int n_i = raw < cap_img ? raw : cap_img;
    if (sel_t <= 0 || n_i <= sel_t + sel_t / 2) return;
    const int i0 = blockIdx.x * SEL_SLICE;
    const int i1 = i0 + SEL_SLICE < n_i ? i0 + SEL_SLICE : n_i;
    if (i0 >= i1) return;
    const uint64_t* hi = in_hi + (int64_t)img * cap_img;
    for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int c0 = i0; c0 < i1; c0 += 4 * blockDim.x) {   // (whole waves enter hist_add: its ballots need every lane)
        uint64_t hv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
            hv[u] = i < i1 ? hi[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool v = c0 + u * (int)blockDim.x + (int)threadIdx.x < i1;
            hist_add(hist, v ? score_bin(hv[u]) : 0, v);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x)
        if (hist[b] != 0) atomicAdd(&ghist[(int64_t)img * SEL_BINS + b], hist[b]);
}

// per-image state of the multi-block selection: {mode, b*, shift, need, have, prefix lo, prefix hi, -}.  mode 0: nothing to do here (no cut, or the one-block kernel did
// it); 1: plain cut at bin b*; 2: the boundary bin is fat, refinement in progress; 3: refined -- records of b* are taken iff (g >> shift) <= prefix
constexpr int SEL_STATE = 8;
constexpr int SEL_RB = 11, SEL_RBINS = 1 << SEL_RB, SEL_LEVELS = (64 + SEL_RB - 1) / SEL_RB;   // 11 key bits per refinement level: six levels exhaust the 64-bit key

// one refinement level, counting half: digit histogram of the records of bin b* that share the prefix chosen so far (slices x images)
__global__ __launch_bounds__(1024) void sel_rhist_kernel(const uint64_t* in_hi, const uint32_t* in_lo, const int* img_count, int cap_img, const int* sel_state, int* rhist) {
    __shared__ int hist[SEL_RBINS];
    const int img = blockIdx.y;
    const int* st = sel_state + SEL_STATE * img;
    if (st[0] != 2) return;
    const int bstar = st[1], shift = st[2];
    const uint64_t prefix = (uint64_t)(uint32_t)st[5] | ((uint64_t)(uint32_t)st[6] << 32);
    const int width = shift >= SEL_RB ? SEL_RB : shift, nshift = shift - width;
    const int raw = img_count[img];
    const int n_i = raw < cap_img ? raw : cap_img;
    const int i0 = blockIdx.x * SEL_SLICE;
    const int i1 = i0 + SEL_SLICE < n_i ? i0 + SEL_SLICE : n_i;
    if (i0 >= i1) return;
    const uint64_t* hi = in_hi + (int64_t)img * cap_img;
    const uint32_t* lo = in_lo + (int64_t)img * cap_img;
    for (int i = threadIdx.x; i < SEL_RBINS; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int c0 = i0; c0 < i1; c0 += 4 * blockDim.x) {
        uint64_t hv[4];
        uint32_t lv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
            hv[u] = i < i1 ? hi[i] : 0ull;
            lv[u] = i < i1 ? lo[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bool v = c0 + u * (int)blockDim.x + (int)threadIdx.x < i1 && score_bin(hv[u]) == bstar;
            const uint64_t g = ((uint64_t)(uint32_t)hv[u] << 32) | lv[u];
            v = v && (shift >= 64 || (g >> shift) == prefix);
            hist_add(hist, (int)((g >> nshift) & (uint64_t)((1 << width) - 1)), v);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SEL_RBINS; b += blockDim.x)
        if (hist[b] != 0) atomicAdd(&rhist[(int64_t)img * SEL_RBINS + b], hist[b]);
}

// ... deciding half (one wave per image): whole digit bins are kept in key order until the target is reached; descend into the bin that crosses it, or stop when the
// selection fits RANK_MAX (the arithmetic of select_prefix_kernel's one-block refinement).  Leaves the image's digit histogram zeroed for the next level.
__global__ __launch_bounds__(64) void sel_rpick_kernel(int* sel_state, int* rhist, int* sel_count) {
    const int img = blockIdx.x, lane = threadIdx.x;
    int* st = sel_state + SEL_STATE * img;
    if (st[0] != 2) return;
    int* h = rhist + (int64_t)img * SEL_RBINS;
    const int shift = st[2], need = st[3], have = st[4];
    const uint64_t prefix = (uint64_t)(uint32_t)st[5] | ((uint64_t)(uint32_t)st[6] << 32);
    const int width = shift >= SEL_RB ? SEL_RB : shift, nshift = shift - width;
    constexpr int PER = SEL_RBINS / 64;
    int sum = 0;
    for (int b = 0; b < PER; ++b) sum += h[lane * PER + b];
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    const int excl = incl - sum;
    int digit = 0, before = 0, inbin = 0;
    const bool mine = excl < need && incl >= need;   // exactly one lane
    if (mine) {
        int c = excl, b = lane * PER;
        for (; b < lane * PER + PER; ++b) {
            if (c + h[b] >= need) break;
            c += h[b];
        }
        digit = b;
        before = c;
        inbin = h[b];
    }
    const uint64_t owner = __ballot(mine);
    const int src = owner ? __builtin_ctzll(owner) : 0;
    digit = __shfl(digit, src, 64);
    before = __shfl(before, src, 64);
    inbin = __shfl(inbin, src, 64);
    __builtin_amdgcn_wave_barrier();   // every lane has read its counts before they are cleared
    for (int b = 0; b < PER; ++b) h[lane * PER + b] = 0;
    if (lane == 0) {
        const uint64_t np = (shift < 64 ? (prefix << width) : 0ull) | (uint64_t)digit;
        st[2] = nshift;
        st[5] = (int)(uint32_t)np;
        st[6] = (int)(uint32_t)(np >> 32);
        if (have + before + inbin <= RANK_MAX || nshift == 0) {   // keep the whole crossing digit bin: the selection fits (or the key is exhausted: unique keys)
            st[0] = 3;
            sel_count[img] = have + before + inbin;
        } else {
            st[4] = have + before;   // digit bins below the crossing one are taken whole
            st[3] = need - before;
        }
    }
}

__global__ __launch_bounds__(1024) void sel_compact_kernel(const uint64_t* in_hi, const uint32_t* in_lo, const int* img_count, int cap_img, const int* sel_state, int* gfill,
                                                           uint64_t* st_hi, uint32_t* st_lo) {
    const int img = blockIdx.y;
    const int* st = sel_state + SEL_STATE * img;
    const int mode = st[0];
    if (mode != 1 && mode != 3) return;
    const int bstar = st[1];
    const int sel_shift = mode == 3 ? st[2] : 64;
    const uint64_t sel_prefix = (uint64_t)(uint32_t)st[5] | ((uint64_t)(uint32_t)st[6] << 32);
    const int raw = img_count[img];
    const int n_i = raw < cap_img ? raw : cap_img;
    const int i0 = blockIdx.x * SEL_SLICE;
    const int i1 = i0 + SEL_SLICE < n_i ? i0 + SEL_SLICE : n_i;
    if (i0 >= i1) return;
    const uint64_t* hi = in_hi + (int64_t)img * cap_img;
    const uint32_t* lo = in_lo + (int64_t)img * cap_img;
    uint64_t* sh = st_hi + (int64_t)img * cap_img;
    uint32_t* sl = st_lo + (int64_t)img * cap_img;
    const int lane = threadIdx.x & 63;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int c0 = i0; c0 < i1; c0 += 4 * blockDim.x) {
        uint64_t h[4];
        uint32_t l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
            h[u] = i < i1 ? hi[i] : 0ull;
            l[u] = i < i1 ? lo[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = score_bin(h[u]);
            const bool take = c0 + u * (int)blockDim.x + (int)threadIdx.x < i1 &&
                              (b < bstar || (b == bstar && (sel_shift >= 64 || ((((uint64_t)(uint32_t)h[u] << 32) | l[u]) >> sel_shift) <= sel_prefix)));
            const uint64_t m = __ballot(take);
            if (m == 0ull) continue;   // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&gfill[img], __popcll(m));
            base = __shfl(base, 0, 64);
            if (take) {
                const int pos = base + __popcll(m & lt);
                sh[pos] = h[u];
                sl[pos] = l[u];
            }
        }
    }
}

__global__ __launch_bounds__(256) void sel_copyback_kernel(uint64_t* hi0, uint32_t* lo0, const uint64_t* st_hi, const uint32_t* st_lo, const int* sel_state, const int* sel_count,
                                                           int cap_img) {
    const int img = blockIdx.y;
    const int mode = sel_state[SEL_STATE * img];
    if (mode != 1 && mode != 3) return;
    // EVERY selected record: a refined selection holds up to RANK_MAX records, but with sel_t > RANK_MAX (detections_per_img > 1536) the ladder ends at the exhausted
    // key with exactly sel_t.  sel_count <= the image's record count <= cap_img.
    const int n_sel = sel_count[img];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_sel; i += gridDim.x * 256) {
        hi0[(int64_t)img * cap_img + i] = st_hi[(int64_t)img * cap_img + i];
        lo0[(int64_t)img * cap_img + i] = st_lo[(int64_t)img * cap_img + i];
    }
}

// ghist / sel_mode non-null: the multi-block form (see above) -- the image's level-0 histogram is already in ghist, and an image whose cut needs no refinement is
// left to sel_compact_kernel
__global__ __launch_bounds__(1024) void select_prefix_kernel(uint64_t* in_hi, uint32_t* in_lo, const int* img_count, int cap_img, int n_img, int sel_t,
                                                             int* sel_count, uint32_t* rank_g, uint32_t* rank_p, const int* ghist, int* sel_mode) {
    __shared__ int hist[SEL_BINS];
    __shared__ int s_bstar, s_nsel, s_fill;
    const int img = blockIdx.x;
    const int raw = img_count[img];
    const int n_i = raw < cap_img ? raw : cap_img;
    if (rank_g != nullptr) {   // rank counters of the multi-block ranking sort (rank_image_kernel adds into them)
        // the first RANK_MAX only: an image that keeps more records (sel_t > RANK_MAX, or YMI_POST_EXACT_FULL) is sort_image_kernel's and never touches the counters
        const int nz = n_i < RANK_MAX ? n_i : RANK_MAX;
        for (int i = threadIdx.x; i < nz; i += blockDim.x) { rank_g[(int64_t)img * cap_img + i] = 0u; rank_p[(int64_t)img * cap_img + i] = 0u; }
    }
    if (sel_t <= 0 || n_i <= sel_t + sel_t / 2) {
        if (threadIdx.x == 0) { sel_count[img] = n_i; sel_count[n_img + img] = 0; }
        return;
    }
    uint64_t* hi = in_hi + (int64_t)img * cap_img;
    uint32_t* lo = in_lo + (int64_t)img * cap_img;
    if (ghist != nullptr) {   // wave-uniform: sel_hist_kernel has counted the bins
        for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x) hist[i] = ghist[(int64_t)img * SEL_BINS + i];
    } else {
        for (int i = threadIdx.x; i < SEL_BINS; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        // One block streams a whole image (up to cap_img records: 2.6 MB at 218 k): four loads in flight per thread, or the pass is bound by one
        // CU's load latency (a single 8-byte load per thread and iteration streamed ~60 GB/s)
        for (int c0 = 0; c0 < n_i; c0 += 4 * blockDim.x) {   // (whole waves enter hist_add: its ballots need every lane)
            uint64_t hv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
                hv[u] = i < n_i ? hi[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool v = c0 + u * (int)blockDim.x + (int)threadIdx.x < n_i;
                hist_add(hist, v ? score_bin(hv[u]) : 0, v);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // first wave: lane l owns bins [64 l, 64 l + 64)
        const int lane = threadIdx.x;
        int sum = 0;
        for (int b = 0; b < 64; ++b) sum += hist[lane * 64 + b];
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        const int excl = incl - sum;
        if (excl < sel_t && incl >= sel_t) {   // exactly one lane (n_i > sel_t)
            int c = excl, b = lane * 64;
            for (; b < lane * 64 + 64; ++b) {
                c += hist[b];
                if (c >= sel_t) break;
            }
            s_bstar = b;
            s_nsel = c;
        }
        if (lane == 0) s_fill = 0;
    }
    __syncthreads();
    const int bstar = s_bstar, nsel = s_nsel;
    if (nsel >= n_i && nsel <= RANK_MAX) {   // the best bins hold everything and the ranking sort takes it: nothing to cut
        if (threadIdx.x == 0) { sel_count[img] = n_i; sel_count[n_img + img] = 0; }
        return;
    }
    // (nsel >= n_i > RANK_MAX: the crossing bin is the image's LAST populated bin and fat -- every score equal, or the tail of the image within 1 / 4096 of the
    // threshold.  It is refined like any other fat bin; leaving the image whole sent all of it to the one-block sort the refinement exists to avoid.)
    if (sel_mode != nullptr) {   // multi-block form: publish the cut (plain), or hand the fat boundary bin to the refinement ladder; sel_compact_kernel moves the records
        if (threadIdx.x == 0) {
            int* st = sel_mode + SEL_STATE * img;
            st[1] = bstar;
            sel_count[n_img + img] = 1;
            if (nsel <= RANK_MAX) {
                st[0] = 1;
                sel_count[img] = nsel;
            } else {
                const int before_bin = nsel - hist[bstar];   // records of the better bins
                st[0] = 2;
                st[2] = 64;
                st[3] = sel_t - before_bin;   // still wanted from the boundary bin (>= 1)
                st[4] = before_bin;           // taken for sure
                st[5] = st[6] = 0;
            }
        }
        return;
    }
    // Round 3: a FAT boundary bin (saturated scores: thousands of records within 1/4096 of each other, or exactly equal) used to push the
    // image past RANK_MAX and onto the one-block-per-image sort (C3: 1.0 ms, C5: 0.33 ms of the post-process).  The cut is refined inside
    // that bin by an exact radix selection on the records' full sort key g = ~score << 32 | lo (unique): 11 bits per level from the top, at
    // each level the digit bins of the records that share the chosen prefix are counted, whole digit bins are kept in key order until the
    // target is reached, and the level descends into the bin that crosses it -- until the selection fits RANK_MAX (any set "every record
    // with key <= T" is a score-ordered prefix, so stopping early with a superset is exact).  Level 0 is the linear bin cut above, so
    // images that never had a fat bin are selected exactly as before.
    uint64_t sel_prefix = 0ull;   // records of bin bstar are taken iff (g >> sel_shift) <= sel_prefix
    int sel_shift = 64;           // 64: the whole bin (no refinement)
    if (nsel > RANK_MAX) {
        constexpr int RB = 11, RBINS = 1 << RB;
        __shared__ int s_digit, s_before;
        const int lane0 = threadIdx.x & 63;
        int before_bin = nsel - hist[bstar];          // records of the better bins (hist is intact: read-only since the scan)
        int need = sel_t - before_bin;                // still wanted from the boundary bin (>= 1)
        int have = before_bin;                        // taken for sure so far
        uint64_t prefix = 0ull;
        int shift = 64;
        __syncthreads();
        while (shift > 0) {
            const int width = shift >= RB ? RB : shift;
            const int nshift = shift - width;
            for (int i = threadIdx.x; i < RBINS; i += blockDim.x) hist[i] = 0;   // (SEL_BINS >= RBINS; bin counts of level 0 are no longer needed)
            __syncthreads();
            for (int c0 = 0; c0 < n_i; c0 += 4 * blockDim.x) {
                uint64_t hv[4];
                uint32_t lv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {   // all eight loads of the thread first
                    const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
                    hv[u] = i < n_i ? hi[i] : 0ull;
                    lv[u] = i < n_i ? lo[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    bool v = c0 + u * (int)blockDim.x + (int)threadIdx.x < n_i && score_bin(hv[u]) == bstar;
                    const uint64_t g = ((uint64_t)(uint32_t)hv[u] << 32) | lv[u];
                    v = v && (shift >= 64 || (g >> shift) == prefix);
                    hist_add(hist, (int)((g >> nshift) & (uint64_t)((1 << width) - 1)), v);
                }
            }
            __syncthreads();
            if (threadIdx.x < 64) {   // first wave: lane l owns digits [32 l, 32 l + 32)
                int sum = 0;
                for (int b = 0; b < RBINS / 64; ++b) sum += hist[lane0 * (RBINS / 64) + b];
                int incl = sum;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_up(incl, d, 64);
                    if (lane0 >= d) incl += t;
                }
                const int excl = incl - sum;
                if (excl < need && incl >= need) {   // exactly one lane
                    int c = excl, b = lane0 * (RBINS / 64);
                    for (; b < lane0 * (RBINS / 64) + RBINS / 64; ++b) {
                        if (c + hist[b] >= need) break;
                        c += hist[b];
                    }
                    s_digit = b;
                    s_before = c;
                }
            }
            __syncthreads();
            const int digit = s_digit, before = s_before, inbin = hist[digit];
            prefix = (shift < 64 ? (prefix << width) : 0ull) | (uint64_t)digit;
            shift = nshift;
            if (have + before + inbin <= RANK_MAX || shift == 0) break;   // keep the whole crossing digit bin: the selection fits (or the key is exhausted: unique keys)
            have += before;          // digit bins below the crossing one are taken whole
            need -= before;
            __syncthreads();
        }
        sel_prefix = prefix;
        sel_shift = shift;
        __syncthreads();
        if (threadIdx.x == 0) s_fill = 0;
        __syncthreads();
    }
    // in-place compaction: a chunk is read completely before any of its survivors is written, and survivors only move to positions at or
    // before indices already read.  Chunks of 8 records per thread (two block barriers per 8192 records: with one record per thread the
    // barriers of this loop were most of the kernel -- 213 iterations for a 218 k-record image)
    const int lane = threadIdx.x & 63;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    constexpr int CU_ = 8;
    for (int c0 = 0; c0 < n_i; c0 += CU_ * blockDim.x) {
        uint64_t h[CU_];
        uint32_t l[CU_];
        bool take[CU_];
#pragma unroll
        for (int u = 0; u < CU_; ++u) {
            const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
            h[u] = i < n_i ? hi[i] : 0ull;
            l[u] = i < n_i ? lo[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < CU_; ++u) {
            const int i = c0 + u * (int)blockDim.x + (int)threadIdx.x;
            const int b = score_bin(h[u]);
            take[u] = i < n_i && (b < bstar || (b == bstar && (sel_shift >= 64 || ((((uint64_t)(uint32_t)h[u] << 32) | l[u]) >> sel_shift) <= sel_prefix)));
        }
        __syncthreads();   // the whole chunk has been read
#pragma unroll
        for (int u = 0; u < CU_; ++u) {
            const uint64_t m = __ballot(take[u]);
            int base = 0;
            if (lane == 0 && m) base = atomicAdd(&s_fill, __popcll(m));
            base = __shfl(base, 0, 64);
            if (take[u]) {
                const int pos = base + __popcll(m & lt);
                hi[pos] = h[u];
                lo[pos] = l[u];
            }
        }
        __syncthreads();   // its survivors are written (all at positions below c0 + 8192)
    }
    if (threadIdx.x == 0) { sel_count[img] = s_fill; sel_count[n_img + img] = 1; }   // s_fill == nsel when the cut was not refined
}

// ------------------------------------------------------------------------------------------
// 2c. multi-block sort by RANKING (images of <= RANK_MAX records -- every image after the score-prefix selection, which
//     keeps <= 1.5 x 4096).  One 1024-thread block per image made the batch wait for its most crowded image (C2: 32 images,
//     1 k records on average but 5 k in one of them: 194 us for two bitonic sorts of 8192 keys on ONE CU while 255 idled).
//     Keys are unique, so the position of a key is the number of keys below it: block (bi, bj, img) counts, for its 256 keys,
//     the keys of j-slice bj that are smaller -- under BOTH orders at once (G: ~score << 32 | cand; P: label, then G order,
//     i.e. label << (64-L) | G >> L) -- and adds the counts to the keys' rank counters; scatter_ranks_kernel then writes G and
//     P directly in place.  n^2 / 64 wave-iterations of two 64-bit compares: 25 M pairs for 5 k records = ~10 us on a few
//     hundred blocks, and no block-wide barrier in the loop.
// ------------------------------------------------------------------------------------------
constexpr int RANK_IT = 256;    // keys ranked per block
constexpr int RANK_JT = 256;    // keys of a j-slice (4 KiB of LDS: G and P key of each)
constexpr int RANK_GRID = 1024; // blocks of the ranking kernel (they walk the pair list of the whole batch)
constexpr int RANK_NIMG = 1024; // images per batch the ranking kernel's per-block table holds; post_check_batch refuses a larger batch (there is no fallback)

__device__ __forceinline__ uint64_t p_key_of(uint64_t g, int label_bits) {
    if (label_bits == 0) return g;   // class-agnostic suppression (YMI_POST_AGNOSTIC): P is G's order
    return ((g & ((1ull << label_bits) - 1ull)) << (64 - label_bits)) | (g >> label_bits);
}

__global__ __launch_bounds__(RANK_IT) void rank_image_kernel(const uint64_t* in_hi, const uint32_t* in_lo, const int* sel_count, int n_img, int cap_img, int label_bits,
                                                             uint32_t* rank_g, uint32_t* rank_p) {
    // round 6: a fixed grid walks the (256-key tile, 256-key j-slice) pairs of ALL images as one list.  The grid used to be sized for RANK_MAX records per image (24 x 6
    // tiles: on C2 -- 1 k records per image, 5 k in one -- 97 % of 4 608 blocks found nothing to do and the others each scanned 1 024 keys: 42 us); blocks per image
    // fixed at 16 made the crowded image's 400 pairs the tail (124 us).  profiles/r06zz_post_kernels.txt
    __shared__ __attribute__((aligned(16))) uint64_t keys[RANK_JT][2];
    __shared__ int s_cnt[RANK_NIMG];   // records per image (0: none of this kernel's), read ONCE per block (a chain of dependent scalar loads per pair cost 15 us)
    for (int m = threadIdx.x; m < n_img; m += RANK_IT) {
        const int c = sel_count[m];
        s_cnt[m] = (c > 0 && c <= RANK_MAX) ? c : 0;
    }
    __syncthreads();
    int total = 0;
    for (int m = 0; m < n_img; ++m) {   // block-uniform
        const int c = s_cnt[m];
        total += ((c + RANK_IT - 1) / RANK_IT) * ((c + RANK_JT - 1) / RANK_JT);
    }
    for (int item = blockIdx.x; item < total; item += gridDim.x) {   // block-uniform trip count
        int img = 0, local = item, n_i = 0, nti = 1;
        for (; img < n_img; ++img) {
            n_i = s_cnt[img];
            nti = (n_i + RANK_IT - 1) / RANK_IT;
            const int cnt = nti * ((n_i + RANK_JT - 1) / RANK_JT);
            if (local < cnt) break;
            local -= cnt;
        }
        const int64_t base = (int64_t)img * cap_img;
        const int bj = local / nti, bi = local - bj * nti;
        const int i0 = bi * RANK_IT, j0 = bj * RANK_JT;
        const int jn = n_i - j0 < RANK_JT ? n_i - j0 : RANK_JT;
        __syncthreads();   // the previous pair's scan is over: the slice may be replaced
        for (int t = threadIdx.x; t < jn; t += RANK_IT) {
            const uint64_t g = ((uint64_t)(uint32_t)in_hi[base + j0 + t] << 32) | in_lo[base + j0 + t];   // ~score << 32 | cand
            keys[t][0] = g;
            keys[t][1] = p_key_of(g, label_bits);
        }
        __syncthreads();
        const int i = i0 + threadIdx.x;
        uint64_t gi = 0ull, pi = 0ull;   // threads past the end count nothing
        if (i < n_i) {
            gi = ((uint64_t)(uint32_t)in_hi[base + i] << 32) | in_lo[base + i];
            pi = p_key_of(gi, label_bits);
        }
        uint32_t cg = 0u, cp = 0u;
#pragma unroll 8
        for (int t = 0; t < jn; ++t) {   // wave-uniform LDS address: one broadcast 16-byte read per key
            const uint64_t kg = keys[t][0], kp = keys[t][1];
            cg += kg < gi ? 1u : 0u;
            cp += kp < pi ? 1u : 0u;
        }
        if (i < n_i) {
            atomicAdd(&rank_g[base + i], cg);
            atomicAdd(&rank_p[base + i], cp);
        }
    }
}

__global__ __launch_bounds__(RANK_IT) void scatter_ranks_kernel(const uint64_t* in_hi, const uint32_t* in_lo, const int* img_count, const int* sel_count, int cap_img,
                                                                int label_bits, const uint32_t* rank_g, const uint32_t* rank_p, uint64_t* ghi, uint32_t* glo,
                                                                uint64_t* phi, uint32_t* plo, uint8_t* keep, int* status) {
    __shared__ int s_off;
    const int img = blockIdx.y;
    const int n_i = sel_count[img];
    if (n_i > RANK_MAX) return;   // sort_image_kernel's image
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int raw = img_count[img];
        atomicAdd(&status[ST_NCAND], n_i);
        if (raw > cap_img) { atomicOr(&status[ST_OVERFLOW], YMI_STATUS_OVERFLOW_CAPACITY); atomicMax(&status[ST_RSV], raw); }
    }
    const int i = blockIdx.x * RANK_IT + threadIdx.x;
    if (blockIdx.x * RANK_IT >= n_i) return;
    if (threadIdx.x < 64) {   // first wave: offset of this image in the compact arrays = sum of the counts before it
        int part = 0;
        for (int j = threadIdx.x; j < img; j += 64) part += sel_count[j];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
        if (threadIdx.x == 0) s_off = part;
    }
    __syncthreads();
    if (i >= n_i) return;
    const int off = s_off;
    const int64_t base = (int64_t)img * cap_img;
    const uint64_t g = ((uint64_t)(uint32_t)in_hi[base + i] << 32) | in_lo[base + i];
    const uint32_t r = rank_g[base + i], p = rank_p[base + i];
    ghi[off + r] = ((uint64_t)(unsigned)img << 32) | (g >> 32);
    glo[off + r] = (uint32_t)g;
    keep[off + r] = 0;
    phi[off + p] = ((uint64_t)(unsigned)img << 16) | (g & ((1ull << label_bits) - 1ull));
    plo[off + p] = (uint32_t)off + r;
}

__global__ __launch_bounds__(1024) void sort_image_kernel(uint64_t* in_hi, uint32_t* in_lo, const int* img_count, const int* sel_count, int cap_img, int n_img,
                                                          int label_bits, int lds_keys, int rank_max, uint64_t* ghi, uint32_t* glo, uint64_t* phi, uint32_t* plo,
                                                          uint8_t* keep, int* status) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_key[];
    __shared__ int s_off;
    const int img = blockIdx.x;
    const int raw = img_count[img];
    const int n_i = sel_count[img];   // records that take part (== min(raw, cap_img) unless the prefix selection cut the image)
    if (n_i <= rank_max) return;      // sorted by rank_image_kernel / scatter_ranks_kernel
    if (threadIdx.x < 64) {   // first wave: offset of this image in the compact arrays = sum of the counts before it
        int part = 0;
        for (int j = threadIdx.x; j < img; j += 64) part += sel_count[j];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
        if (threadIdx.x == 0) s_off = part;
    }
    if (threadIdx.x == 0) {
        atomicAdd(&status[ST_NCAND], n_i);
        if (raw > cap_img) { atomicOr(&status[ST_OVERFLOW], YMI_STATUS_OVERFLOW_CAPACITY); atomicMax(&status[ST_RSV], raw); }
    }
    const int64_t base = (int64_t)img * cap_img;
    uint64_t* keys = in_hi + base;      // this image's region doubles as key scratch (u64 per record)
    uint32_t* rank = in_lo + base;      // ... and as rank scratch once the candidate ids moved into the keys
    const uint32_t lmask = (1u << label_bits) - 1u;
    if (n_i <= lds_keys) {
        // single run (the common case after the prefix selection): both sorts stay in LDS, HBM is touched only to read
        // the records once and to write G and P -- no scratch round trips between the phases
        __syncthreads();   // s_off
        const int off = s_off;
        int np2 = 64;
        while (np2 < n_i) np2 <<= 1;
        for (int i = threadIdx.x; i < np2; i += blockDim.x)
            lds_key[i] = i < n_i ? (((uint64_t)(uint32_t)keys[i] << 32) | rank[i]) : ~0ull;   // ~score << 32 | cand; padding sorts last
        __syncthreads();
        bitonic_sort_lds(lds_key, np2);   // G order: score descending, ties by candidate index
        for (int i = threadIdx.x; i < n_i; i += blockDim.x) {
            const uint64_t k = lds_key[i];
            ghi[off + i] = ((uint64_t)(unsigned)img << 32) | (k >> 32);
            glo[off + i] = (uint32_t)k;
            keep[off + i] = 0;
            lds_key[i] = ((uint64_t)((uint32_t)k & lmask) << 32) | (uint32_t)i;   // label << 32 | rank in G (same index read / written)
        }
        __syncthreads();
        bitonic_sort_lds(lds_key, np2);   // P order: by label, then by G rank
        for (int i = threadIdx.x; i < n_i; i += blockDim.x) {
            const uint64_t k = lds_key[i];
            phi[off + i] = ((uint64_t)(unsigned)img << 16) | (k >> 32);
            plo[off + i] = (uint32_t)off + (uint32_t)k;
        }
        return;
    }
    for (int i = threadIdx.x; i < n_i; i += blockDim.x)
        keys[i] = ((uint64_t)(uint32_t)keys[i] << 32) | rank[i];   // ~score << 32 | cand  (same index read / written)
    __syncthreads();
    const int off = s_off;
    // G order: score descending, ties by candidate index
    sort_runs(keys, n_i, lds_key, lds_keys, rank);
    for (int i = threadIdx.x; i < n_i; i += blockDim.x) {
        const uint64_t k = keys[i];
        const uint32_t r = rank[i];
        ghi[off + r] = ((uint64_t)(unsigned)img << 32) | (k >> 32);
        glo[off + r] = (uint32_t)k;
        keep[off + r] = 0;
        keys[i] = ((uint64_t)((uint32_t)k & lmask) << 32) | r;   // label << 32 | rank in G (unique)
    }
    __syncthreads();
    // P order: by label, then by G rank
    sort_runs(keys, n_i, lds_key, lds_keys, rank);
    for (int i = threadIdx.x; i < n_i; i += blockDim.x) {
        const uint64_t k = keys[i];
        const uint32_t r = rank[i];
        phi[off + r] = ((uint64_t)(unsigned)img << 16) | (k >> 32);
        plo[off + r] = (uint32_t)off + (uint32_t)k;
    }
}

// ------------------------------------------------------------------------------------------
// 3. class-aware NMS.  After the global sort G, records are re-keyed as
//      hi' = img << 16 | label,  lo' = r (rank in G)
//    and stably sorted by label, so each (label, img) segment lists its candidates in score order.
//    One wave per segment runs the exact greedy algorithm: 64 candidates per step are tested against
//    the kept boxes so far (uniform loads), then resolved among themselves with ballots/shuffles.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void make_label_records_kernel(const uint64_t* ghi, const uint32_t* glo, uint64_t* phi, uint32_t* plo,
                                                                 const int* status, int cap, int label_bits, uint8_t* keep) {
    const int n = ncand(status, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned label = glo[i] & ((1u << label_bits) - 1u);
    const unsigned img = (unsigned)(ghi[i] >> 32);
    phi[i] = ((uint64_t)img << 16) | label;
    plo[i] = (uint32_t)i;
    keep[i] = 0;
}

__global__ __launch_bounds__(256) void find_segments_kernel(const uint64_t* phi, int* status, int cap, uint32_t* seg_start) {
    const int n = ncand(status, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || phi[i] != phi[i - 1]) seg_start[atomicAdd(&status[ST_NSEG], 1)] = (uint32_t)i;
}

__device__ __forceinline__ bool iou_gt(const f32x4 bi, float area_i, const f32x4 bj, float area_j, float thr) {
    // torchvision nms: inter / (iarea + jarea - inter) > thr, fp32, no fused ops
    const float xx1 = fmaxf(bi[0], bj[0]), yy1 = fmaxf(bi[1], bj[1]);
    const float xx2 = fminf(bi[2], bj[2]), yy2 = fminf(bi[3], bj[3]);
    const float w = fmaxf(0.f, __fsub_rn(xx2, xx1)), h = fmaxf(0.f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(w, h);
    const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_i, area_j), inter));
    return iou > thr;
}

// ---- the greedy step both NMS kernels (3, 3b) are made of: lane l holds candidate l of the step's 64 ----
__device__ __forceinline__ float box_area(const f32x4 b) { return __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1])); }

// candidate at position p of the order P: its rank r in G, its box (looked up by image and anchor) and area; zeros for a lane without a candidate
struct NmsCand { f32x4 box; float area; unsigned r; };
__device__ __forceinline__ NmsCand nms_load_candidate(bool valid, int p, const uint32_t* plo, const uint64_t* ghi, const uint32_t* glo, const float* boxes_all,
                                                      int total_anchors, int label_bits) {
    NmsCand c = {{0.f, 0.f, 0.f, 0.f}, 0.f, 0u};
    if (valid) {
        c.r = plo[p];
        const unsigned img = (unsigned)(ghi[c.r] >> 32);
        const unsigned anchor = glo[c.r] >> label_bits;
        c.box = *reinterpret_cast<const f32x4*>(boxes_all + ((int64_t)img * total_anchors + anchor) * 4);
    }
    c.area = box_area(c.box);
    return c;
}

// against the boxes already kept in the segment (higher score), entries first, first + stride, ...: LDS broadcast reads of `kl` below kcap, the spill area `kb` beyond
// (kcap is a multiple of stride)
__device__ __forceinline__ bool nms_test_kept(bool alive, const NmsCand& c, const f32x4* kl, const f32x4* kb, int kept_cnt, int kcap, int first, int stride, float thr) {
    const int in_lds = kept_cnt < kcap ? kept_cnt : kcap;
    for (int j = first; j < in_lds; j += stride) {
        const f32x4 k = kl[j];
        if (alive && iou_gt(k, box_area(k), c.box, c.area, thr)) alive = false;
    }
    for (int j = kcap + first; j < kept_cnt; j += stride) {
        const f32x4 k = kb[j];
        if (alive && iou_gt(k, box_area(k), c.box, c.area, thr)) alive = false;
    }
    return alive;
}

// The third piece of the step -- the 64 candidates resolved among themselves by ballot and shuffle, the survivors appended to the kept list -- stays written out in
// both kernels: as a shared helper it compiled nms_block_kernel to a different register assignment that cost ymi_nms 2 to 4 % at 16384 boxes
// (profiles/post_refactor_bench_ab.txt); written out, both kernels have the parent's instructions but for the order of a few prologue lines.

constexpr int NMS_KCAP = 384;   // kept boxes per wave held in LDS (6 KiB / wave); the rest spills to HBM scratch

__global__ __launch_bounds__(256) void nms_segments_kernel(const uint64_t* phi, const uint32_t* plo, const uint64_t* ghi, const uint32_t* glo,
                                                           const float* boxes_all, int total_anchors, int label_bits, const int* status, int cap,
                                                           const uint32_t* seg_start, float* kept_box, uint8_t* keep, float thr) {
    __shared__ f32x4 kept_lds[4][NMS_KCAP];
    const int n = ncand(status, cap);
    const int nseg = status[ST_NSEG];
    const int lane = threadIdx.x & 63;
    const int wave_local = threadIdx.x >> 6;
    const int wave_global = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    f32x4* kl = kept_lds[wave_local];
    for (int s = wave_global; s < nseg; s += nwaves) {
        const int start = (int)seg_start[s];
        const uint64_t key = phi[start];
        int kept_cnt = 0;
        f32x4* kb = reinterpret_cast<f32x4*>(kept_box) + start;   // spill area: kept <= segment length
        for (int c = start;; c += 64) {
            const int p = c + lane;
            const bool valid = p < n && phi[p] == key;
            const uint64_t vmask = __ballot(valid);
            if (vmask == 0) break;
            const NmsCand cand = nms_load_candidate(valid, p, plo, ghi, glo, boxes_all, total_anchors, label_bits);
            bool alive = nms_test_kept(valid, cand, kl, kb, kept_cnt, NMS_KCAP, 0, 1, thr);
            uint64_t mask = __ballot(alive);
            // among the 64 candidates of this step, in order
            uint64_t todo = mask;
            while (todo) {
                const int i = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                f32x4 bi;
                bi[0] = __shfl(cand.box[0], i, 64);
                bi[1] = __shfl(cand.box[1], i, 64);
                bi[2] = __shfl(cand.box[2], i, 64);
                bi[3] = __shfl(cand.box[3], i, 64);
                const float ai = __shfl(cand.area, i, 64);
                if (alive && lane > i && iou_gt(bi, ai, cand.box, cand.area, thr)) alive = false;
                mask = __ballot(alive);
                todo &= mask;
            }
            if (alive) {
                const int slot = kept_cnt + __popcll(mask & lt);
                if (slot < NMS_KCAP) kl[slot] = cand.box; else kb[slot] = cand.box;
                keep[cand.r] = 1;
            }
            kept_cnt += __popcll(mask);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // kept boxes (LDS / HBM) visible to this wave's later reads
            if (vmask != ~0ull) break;  // last (partial) step of the segment
        }
    }
}

// ------------------------------------------------------------------------------------------
// 3b. class-AGNOSTIC NMS (YMI_POST_AGNOSTIC, ymi_nms): one segment per IMAGE, whatever the labels.  nms_segments_kernel would give the whole image to one
//     wave -- the greedy scan of a crowded image on 1/1024 of the chip -- so here a segment gets a WORKGROUP of NMSB_WAVES waves.  The step is the one
//     above -- the same two helpers and the same resolve loop --, hence bit-identical to it: candidates in score order, 64 per step; every wave holds the step's 64 candidates (lane l = candidate
//     l) and tests them against ITS share of the kept list (kept boxes j = wave, wave + NMSB_WAVES, ...: LDS broadcast reads, the spill area beyond
//     NMSB_KCAP); the per-wave alive masks meet in LDS; wave 0 ANDs them, resolves the 64 among themselves by ballot and shuffle, appends the survivors to
//     the kept list and publishes the step's final mask.  Suppression is an OR over the kept boxes, so splitting the list over waves cannot change a bit.
//     Two block barriers per step; every trip count of a loop with a barrier (segments, steps) comes from LDS words read after a barrier.
// ------------------------------------------------------------------------------------------
constexpr int NMSB_WAVES = 16;      // waves per segment (one 1024-thread block)
constexpr int NMSB_KCAP = 2048;     // kept boxes of the block held in LDS (32 KiB); the rest spills to Workspace::kept_box

__global__ __launch_bounds__(NMSB_WAVES * 64) void nms_block_kernel(const uint64_t* phi, const uint32_t* plo, const uint64_t* ghi, const uint32_t* glo,
                                                                    const float* boxes_all, int total_anchors, int label_bits, const int* status, int cap,
                                                                    const uint32_t* seg_start, float* kept_box, uint8_t* keep, float thr) {
    __shared__ f32x4 kept_lds[NMSB_KCAP];
    __shared__ uint64_t s_alive[NMSB_WAVES];
    __shared__ uint64_t s_final;
    __shared__ int s_nseg, s_neg_end;
    (void)phi;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int n = ncand(status, cap);
    if (threadIdx.x == 0) s_nseg = status[ST_NSEG];
    __syncthreads();
    const int nseg = s_nseg;
    for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int start = (int)seg_start[s];
        // the segment ends at the smallest segment start behind its own (seg_start is unordered), or at n
        if (threadIdx.x == 0) s_neg_end = -n;
        __syncthreads();
        for (int t = threadIdx.x; t < nseg; t += NMSB_WAVES * 64) {
            const int o = (int)seg_start[t];
            if (o > start) atomicMax(&s_neg_end, -o);
        }
        __syncthreads();
        const int end = -s_neg_end;
        const int nsteps = (end - start + 63) >> 6;
        int kept_cnt = 0;
        f32x4* kb = reinterpret_cast<f32x4*>(kept_box) + start;   // spill area: kept <= segment length
        for (int st = 0; st < nsteps; ++st) {
            const int p = start + st * 64 + lane;
            const bool valid = p < end;
            const NmsCand cand = nms_load_candidate(valid, p, plo, ghi, glo, boxes_all, total_anchors, label_bits);
            // this wave's share of the boxes already kept
            const uint64_t mine = __ballot(nms_test_kept(valid, cand, kept_lds, kb, kept_cnt, NMSB_KCAP, wave, NMSB_WAVES, thr));
            if (lane == 0) s_alive[wave] = mine;
            __syncthreads();
            if (wave == 0) {
                uint64_t mask = s_alive[0];
#pragma unroll
                for (int w = 1; w < NMSB_WAVES; ++w) mask &= s_alive[w];
                bool alive = (mask >> lane) & 1ull;
                // among the 64 candidates of this step, in order
                uint64_t todo = mask;
                while (todo) {
                    const int i = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    f32x4 bi;
                    bi[0] = __shfl(cand.box[0], i, 64);
                    bi[1] = __shfl(cand.box[1], i, 64);
                    bi[2] = __shfl(cand.box[2], i, 64);
                    bi[3] = __shfl(cand.box[3], i, 64);
                    const float ai = __shfl(cand.area, i, 64);
                    if (alive && lane > i && iou_gt(bi, ai, cand.box, cand.area, thr)) alive = false;
                    mask = __ballot(alive);
                    todo &= mask;
                }
                if (alive) {
                    const int slot = kept_cnt + __popcll(mask & lt);
                    if (slot < NMSB_KCAP) kept_lds[slot] = cand.box; else kb[slot] = cand.box;
                    keep[cand.r] = 1;
                }
                if (lane == 0) s_final = mask;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // kept boxes (LDS / HBM) visible to the block's later reads
            }
            __syncthreads();
            kept_cnt += __popcll(s_final);
        }
        __syncthreads();   // the last step's s_final / this segment's s_neg_end have been read by every wave before the next segment resets them
    }
}

// ------------------------------------------------------------------------------------------
// 4. top-k + rescale.  One block per image: binary-search the image's range in G, then an ordered
//    compaction of the keep flags in rank order; first K kept are written to the fixed slab.
// ------------------------------------------------------------------------------------------
struct GatherArgs {
    const uint64_t* ghi;
    const uint32_t* glo;
    const uint8_t* keep;
    const float* boxes_all;
    const float* rescale;
    const int* status;
    const int* truncated;   // per image: 1 = only a score prefix of its candidates was processed (NULL: never)
    const int* img_count;   // per image: raw candidate count (per-image path; NULL: the global sort, whose status[ST_NCAND] is the raw count)
    float* out_slab;        // (n, 6K + 1) packed wire slab or NULL (ymi_post_desc.out_slab)
    int* status_rw;
    int cap, total_anchors, label_bits, K;
    float* out_boxes;
    float* out_scores;
    int64_t* out_labels;
    int* out_count;
};

__device__ int lower_bound_img(const uint64_t* ghi, int n, unsigned img) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)(ghi[mid] >> 32) < img) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void gather_topk_kernel(const GatherArgs a) {
    __shared__ int wave_cnt[4];
    __shared__ int s_taken;
    __shared__ int s_last;
    const int n = ncand(a.status, a.cap);
    const unsigned img = blockIdx.x;
    const int begin = lower_bound_img(a.ghi, n, img), end = lower_bound_img(a.ghi, n, img + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (threadIdx.x == 0) s_taken = 0;
    __syncthreads();
    float gain = 0.f, padx = 0.f, pady = 0.f;
    if (a.rescale) { gain = a.rescale[img * 3]; padx = a.rescale[img * 3 + 1]; pady = a.rescale[img * 3 + 2]; }
    for (int c = begin; c < end; c += 256) {
        const int taken = s_taken;
        if (taken >= a.K) break;
        const int r = c + threadIdx.x;
        const bool k = r < end && a.keep[r] != 0;
        const uint64_t m = __ballot(k);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = taken;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        const int rank = off + __popcll(m & lt);
        if (k && rank < a.K) {
            const uint64_t hi = a.ghi[r];
            const uint32_t lo = a.glo[r];
            const unsigned anchor = lo >> a.label_bits;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes_all + ((int64_t)img * a.total_anchors + anchor) * 4);
            f32x4 o = b;
            if (gain > 0.f) {  // transform.py:362-365
                o[0] = __fdiv_rn(__fsub_rn(b[0], padx), gain);
                o[2] = __fdiv_rn(__fsub_rn(b[2], padx), gain);
                o[1] = __fdiv_rn(__fsub_rn(b[1], pady), gain);
                o[3] = __fdiv_rn(__fsub_rn(b[3], pady), gain);
            }
            const int64_t slot = (int64_t)img * a.K + rank;
            *reinterpret_cast<f32x4*>(a.out_boxes + slot * 4) = o;
            a.out_scores[slot] = __uint_as_float(~(uint32_t)hi);
            a.out_labels[slot] = (int64_t)(lo & ((1u << a.label_bits) - 1u));
            if (a.out_slab != nullptr) {   // the same detection in the packed wire slab (rows of 6K + 1 floats: only 4-byte aligned)
                float* row = a.out_slab + (int64_t)img * (6 * a.K + 1);
                row[4 * rank] = o[0]; row[4 * rank + 1] = o[1]; row[4 * rank + 2] = o[2]; row[4 * rank + 3] = o[3];
                row[4 * a.K + rank] = __uint_as_float(~(uint32_t)hi);
                row[5 * a.K + rank] = (float)(lo & ((1u << a.label_bits) - 1u));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) s_taken = taken + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const int cnt = s_taken < a.K ? s_taken : a.K;
    if (a.out_slab != nullptr) {   // slots past the count are zero: the slab is a function of the detections alone
        float* row = a.out_slab + (int64_t)img * (6 * a.K + 1);
        for (int t = cnt + (int)threadIdx.x; t < a.K; t += 256) {
            row[4 * t] = 0.f; row[4 * t + 1] = 0.f; row[4 * t + 2] = 0.f; row[4 * t + 3] = 0.f;
            row[4 * a.K + t] = 0.f;
            row[5 * a.K + t] = 0.f;
        }
        if (threadIdx.x == 0) row[6 * a.K] = (float)cnt;
    }
    if (threadIdx.x == 0) {
        a.out_count[img] = cnt;
        // a truncated image must reach K survivors on its prefix alone, else the cut may have mattered
        if (a.truncated != nullptr && a.truncated[img] != 0 && s_taken < a.K) atomicOr(&a.status_rw[ST_OVERFLOW], YMI_STATUS_PREFIX_SHORT);
        if (a.img_count != nullptr) atomicAdd(&a.status_rw[ST_RAW], a.img_count[img]);
        else if (img == 0) atomicAdd(&a.status_rw[ST_RAW], n);
        // last-block fix-up: the status word is final only when every image's block has finished (ST_DONE is zeroed by post_begin)
        __threadfence();
        s_last = atomicAdd(&a.status_rw[ST_DONE], 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (s_last && a.out_slab != nullptr) {
        __threadfence();
        if (atomicOr(&a.status_rw[ST_OVERFLOW], 0) != 0)   // the caller will re-run this batch: mark every row stale (yolort_amd/dist.py SLAB_STALE)
            for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) a.out_slab[(int64_t)i * (6 * a.K + 1) + 6 * a.K] = YMI_SLAB_STALE;
    }
}

// ------------------------------------------------------------------------------------------
// 4a. the pieces of the gather as __device__ functions of the block size, for merge_gather_kernel (4b): its images outside the merge bound run gather_image /
//     gather_finish -- gather_topk_kernel's statements, word for word -- and its merged images end with the same write_detection / gather_finish.  gather_topk_kernel
//     itself keeps its own text above: restated through these functions it compiled to the same registers but not to the same instructions, and the default path is
//     to stay byte for byte what it was.
// ------------------------------------------------------------------------------------------
// One detection into slot `rank` of image `img`: the box (already rescaled), the score bit-inverted back out of the record, the label; the same in the packed wire slab
__device__ __forceinline__ void write_detection(const GatherArgs& a, unsigned img, int rank, const f32x4 o, uint64_t hi, uint32_t lo) {
    const int64_t slot = (int64_t)img * a.K + rank;
    *reinterpret_cast<f32x4*>(a.out_boxes + slot * 4) = o;
    a.out_scores[slot] = __uint_as_float(~(uint32_t)hi);
    a.out_labels[slot] = (int64_t)(lo & ((1u << a.label_bits) - 1u));
    if (a.out_slab != nullptr) {   // the same detection in the packed wire slab (rows of 6K + 1 floats: only 4-byte aligned)
        float* row = a.out_slab + (int64_t)img * (6 * a.K + 1);
        row[4 * rank] = o[0]; row[4 * rank + 1] = o[1]; row[4 * rank + 2] = o[2]; row[4 * rank + 3] = o[3];
        row[4 * a.K + rank] = __uint_as_float(~(uint32_t)hi);
        row[5 * a.K + rank] = (float)(lo & ((1u << a.label_bits) - 1u));
    }
}

__device__ __forceinline__ f32x4 rescale_box(const f32x4 b, float gain, float padx, float pady) {
    f32x4 o = b;
    if (gain > 0.f) {  // transform.py:362-365
        o[0] = __fdiv_rn(__fsub_rn(b[0], padx), gain);
        o[2] = __fdiv_rn(__fsub_rn(b[2], padx), gain);
        o[1] = __fdiv_rn(__fsub_rn(b[1], pady), gain);
        o[3] = __fdiv_rn(__fsub_rn(b[3], pady), gain);
    }
    return o;
}

// gather_topk_kernel's loop for ONE image and a block of NT threads: an ordered compaction of the keep flags of G's range [begin, end), the first K kept written out.
// Leaves the number of kept records it counted (it stops counting once K are taken) in *s_taken.  The path of merge_gather_kernel's images outside the merge bound.
template <int NT>
__device__ __forceinline__ void gather_image(const GatherArgs& a, unsigned img, int begin, int end, float gain, float padx, float pady, int* wave_cnt, int* s_taken) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int c = begin; c < end; c += NT) {
        const int taken = *s_taken;
        if (taken >= a.K) break;
        const int r = c + threadIdx.x;
        const bool k = r < end && a.keep[r] != 0;
        const uint64_t m = __ballot(k);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = taken;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        const int rank = off + __popcll(m & lt);
        if (k && rank < a.K) {
            const uint64_t hi = a.ghi[r];
            const uint32_t lo = a.glo[r];
            const unsigned anchor = lo >> a.label_bits;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.boxes_all + ((int64_t)img * a.total_anchors + anchor) * 4);
            write_detection(a, img, rank, rescale_box(b, gain, padx, pady), hi, lo);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = taken;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) sum += wave_cnt[w];
            *s_taken = sum;
        }
        __syncthreads();
    }
}

// gather_topk_kernel's epilogue, whatever filled the image's slots: `cnt` detections were written, `taken` kept records were counted.  Zeroes the slab past the count, writes the
// count, raises YMI_STATUS_PREFIX_SHORT for a truncated image that fell short, adds the raw count, and runs the last-block protocol (ST_DONE, YMI_SLAB_STALE).
template <int NT>
__device__ __forceinline__ void gather_finish(const GatherArgs& a, unsigned img, int n, int cnt, const int* s_taken, int* s_last) {
    if (a.out_slab != nullptr) {   // slots past the count are zero: the slab is a function of the detections alone
        float* row = a.out_slab + (int64_t)img * (6 * a.K + 1);
        for (int t = cnt + (int)threadIdx.x; t < a.K; t += NT) {
            row[4 * t] = 0.f; row[4 * t + 1] = 0.f; row[4 * t + 2] = 0.f; row[4 * t + 3] = 0.f;
            row[4 * a.K + t] = 0.f;
            row[5 * a.K + t] = 0.f;
        }
        if (threadIdx.x == 0) row[6 * a.K] = (float)cnt;
    }
    if (threadIdx.x == 0) {
        a.out_count[img] = cnt;
        // a truncated image must reach K survivors on its prefix alone, else the cut may have mattered
        if (a.truncated != nullptr && a.truncated[img] != 0 && *s_taken < a.K) atomicOr(&a.status_rw[ST_OVERFLOW], YMI_STATUS_PREFIX_SHORT);
        if (a.img_count != nullptr) atomicAdd(&a.status_rw[ST_RAW], a.img_count[img]);
        else if (img == 0) atomicAdd(&a.status_rw[ST_RAW], n);
        // last-block fix-up: the status word is final only when every image's block has finished (ST_DONE is zeroed by post_begin)
        __threadfence();
        *s_last = atomicAdd(&a.status_rw[ST_DONE], 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (*s_last && a.out_slab != nullptr) {
        __threadfence();
        if (atomicOr(&a.status_rw[ST_OVERFLOW], 0) != 0)   // the caller will re-run this batch: mark every row stale (yolort_amd/dist.py SLAB_STALE)
            for (int i = threadIdx.x; i < (int)gridDim.x; i += NT) a.out_slab[(int64_t)i * (6 * a.K + 1) + 6 * a.K] = YMI_SLAB_STALE;
    }
}

// ------------------------------------------------------------------------------------------
// 4b. merge-NMS (YMI_POST_MERGE; Python: merge=True; ultralytics' non_max_suppression with its local `merge = True`, yolort/v5/utils/general.py:604-613).  Launched
//     INSTEAD of gather_topk_kernel, one workgroup of MRG_WAVES waves per image.  An image of n candidates is merged iff 1 < n < YMI_MERGE_MAX_N; every other image
//     runs gather_image / gather_finish above and comes out as without the flag.  A merged image:
//       1. its records (< YMI_MERGE_MAX_N of them: box, score, label) are staged in LDS in rank order;
//       2. the first K kept ranks are compacted, in order, into an LDS list (the kept list is taken BEFORE the merge, general.py:604-605);
//       3. wave w takes the kept records q = w, w + MRG_WAVES, ...: lane l walks the candidates j = l, l + 64, ... and, for those of the same label (any label under
//          YMI_POST_AGNOSTIC) whose IoU with the kept box is > nms_thresh (iou_gt: the suppression's own test, so the box itself counts unless its area is 0), adds
//          score_j and score_j * box_j to five partial sums with explicitly rounded fp32 multiplies and adds, and counts them; a fixed xor butterfly (32, 16, .., 1)
//          sums the lanes -- fp32 addition commutes, so every lane ends with the same bits, and the order is a function of the candidate's rank alone;
//       4. merged box = sums / weight (fp32 division) if the weight is > 0, else the NMS box; without YMI_POST_MERGE_KEEP_SINGLE a kept record with <= 1 contributors
//          is dropped (general.py:612-613);
//       5. the survivors are compacted in rank order, rescaled and written like any detection (write_detection); slots are not refilled.
//     Dynamic LDS: merge_lds_bytes(K), 75000 + 16 * min(K, YMI_MERGE_MAX_N - 1) bytes (78 KiB at K = 300).
// ------------------------------------------------------------------------------------------
constexpr int MRG_WAVES = 16;
constexpr int MRG_THREADS = MRG_WAVES * 64;
constexpr int MRG_N = YMI_MERGE_MAX_N;

inline int merge_kept_cap(int K) { return K < MRG_N - 1 ? K : MRG_N - 1; }   // a merged image has fewer than MRG_N records, hence fewer kept ones
inline size_t merge_lds_bytes(int K) { return (size_t)MRG_N * (16 + 4 + 2 + 2 + 1) + (size_t)merge_kept_cap(K) * 16; }

__global__ __launch_bounds__(MRG_THREADS) void merge_gather_kernel(const GatherArgs a, float thr, int agnostic, int keep_single, int kept_cap) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_key[];
    __shared__ int wave_cnt[MRG_WAVES];
    __shared__ int s_taken, s_kept;
    __shared__ int s_last;
    const int n = ncand(a.status, a.cap);
    const unsigned img = blockIdx.x;
    const int begin = lower_bound_img(a.ghi, n, img), end = lower_bound_img(a.ghi, n, img + 1);
    const int ns = end - begin;                                              // records staged: the image's range in G
    const int n_i = a.img_count != nullptr ? a.img_count[img] : ns;          // the image's candidate count
    if (threadIdx.x == 0) s_taken = 0;
    __syncthreads();
    float gain = 0.f, padx = 0.f, pady = 0.f;
    if (a.rescale) { gain = a.rescale[img * 3]; padx = a.rescale[img * 3 + 1]; pady = a.rescale[img * 3 + 2]; }
    if (!(n_i > 1 && n_i < MRG_N) || ns >= MRG_N) {   // block-uniform: not a merged image (general.py:606).  A truncated image has > 6144 records: never merged
        gather_image<MRG_THREADS>(a, img, begin, end, gain, padx, pady, wave_cnt, &s_taken);
        gather_finish<MRG_THREADS>(a, img, n, s_taken < a.K ? s_taken : a.K, &s_taken, &s_last);
        return;
    }
    f32x4* box = reinterpret_cast<f32x4*>(lds_key);                          // [MRG_N]
    f32x4* merged = box + MRG_N;                                             // [kept_cap]
    float* score = reinterpret_cast<float*>(merged + kept_cap);              // [MRG_N]
    uint16_t* label = reinterpret_cast<uint16_t*>(score + MRG_N);            // [MRG_N]  (num_classes <= 4096)
    uint16_t* kept = label + MRG_N;                                          // [MRG_N]  local rank of the q-th kept record
    uint8_t* drop = reinterpret_cast<uint8_t*>(kept + MRG_N);                // [MRG_N]  1 = redundant
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint32_t lmask = (1u << a.label_bits) - 1u;
    // 1. stage
    for (int j = threadIdx.x; j < ns; j += MRG_THREADS) {
        const uint64_t hi = a.ghi[begin + j];
        const uint32_t lo = a.glo[begin + j];
        box[j] = *reinterpret_cast<const f32x4*>(a.boxes_all + ((int64_t)img * a.total_anchors + (lo >> a.label_bits)) * 4);
        score[j] = __uint_as_float(~(uint32_t)hi);
        label[j] = (uint16_t)(lo & lmask);
    }
    // 2. the first K kept ranks, in order (gather_image's compaction, into the list)
    for (int c = 0; c < ns; c += MRG_THREADS) {
        const int taken = s_taken;
        if (taken >= a.K) break;
        const int j = c + threadIdx.x;
        const bool k = j < ns && a.keep[begin + j] != 0;
        const uint64_t m = __ballot(k);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = taken;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        const int rank = off + __popcll(m & lt);
        if (k && rank < a.K) kept[rank] = (uint16_t)j;
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = taken;
#pragma unroll
            for (int w = 0; w < MRG_WAVES; ++w) sum += wave_cnt[w];
            s_taken = sum;
        }
        __syncthreads();
    }
    __syncthreads();   // the staged records and the list are complete (ns == 0 runs neither loop)
    const int taken_all = s_taken;
    const int nk = taken_all < a.K ? taken_all : a.K;   // <= kept_cap: nk <= ns < MRG_N
    // 3. + 4. one wave per kept record
    for (int q = wave; q < nk; q += MRG_WAVES) {   // wave-uniform
        const int i = kept[q];
        const f32x4 bi = box[i];
        const float ai = __fmul_rn(__fsub_rn(bi[2], bi[0]), __fsub_rn(bi[3], bi[1]));
        const unsigned li = label[i];
        float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int m = 0;
        for (int j = lane; j < ns; j += 64) {
            if (!agnostic && label[j] != li) continue;
            const f32x4 bj = box[j];
            const float aj = __fmul_rn(__fsub_rn(bj[2], bj[0]), __fsub_rn(bj[3], bj[1]));
            if (iou_gt(bi, ai, bj, aj, thr)) {
                const float s = score[j];
                sw = __fadd_rn(sw, s);
                s0 = __fadd_rn(s0, __fmul_rn(s, bj[0]));
                s1 = __fadd_rn(s1, __fmul_rn(s, bj[1]));
                s2 = __fadd_rn(s2, __fmul_rn(s, bj[2]));
                s3 = __fadd_rn(s3, __fmul_rn(s, bj[3]));
                ++m;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sw = __fadd_rn(sw, __shfl_xor(sw, d, 64));
            s0 = __fadd_rn(s0, __shfl_xor(s0, d, 64));
            s1 = __fadd_rn(s1, __shfl_xor(s1, d, 64));
            s2 = __fadd_rn(s2, __shfl_xor(s2, d, 64));
            s3 = __fadd_rn(s3, __shfl_xor(s3, d, 64));
            m += __shfl_xor(m, d, 64);
        }
        if (lane == 0) {
            f32x4 o = bi;
            if (sw > 0.f) {   // all-zero scores (a non-positive score_thresh): the box keeps its NMS coordinates (the reference would divide by 0)
                o[0] = __fdiv_rn(s0, sw); o[1] = __fdiv_rn(s1, sw); o[2] = __fdiv_rn(s2, sw); o[3] = __fdiv_rn(s3, sw);
            }
            merged[q] = o;
            drop[q] = (!keep_single && m <= 1) ? 1 : 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { s_kept = taken_all; s_taken = 0; }   // s_kept: what gather_finish compares with K for a truncated image (a merged image never is one)
    __syncthreads();
    // 5. the survivors, compacted in rank order
    for (int c = 0; c < nk; c += MRG_THREADS) {
        const int base = s_taken;
        const int q = c + threadIdx.x;
        const bool k = q < nk && drop[q] == 0;
        const uint64_t m = __ballot(k);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        if (k) {
            const int r = begin + kept[q];
            write_detection(a, img, off + __popcll(m & lt), rescale_box(merged[q], gain, padx, pady), a.ghi[r], a.glo[r]);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = base;
#pragma unroll
            for (int w = 0; w < MRG_WAVES; ++w) sum += wave_cnt[w];
            s_taken = sum;
        }
        __syncthreads();
    }
    gather_finish<MRG_THREADS>(a, img, n, s_taken, &s_kept, &s_last);
}

// ------------------------------------------------------------------------------------------
// host-side orchestration
// ------------------------------------------------------------------------------------------

struct SortState {
    int cur;  // index of the array pair holding the current order
};

static int radix_pass(const Workspace& w, SortState& st, int* status, int cap, int shift, hipStream_t s) {
    const int nblk = cdiv(cap, SORT_ITEMS);
    const int src = st.cur, dst = st.cur ^ 1;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(256), 0, s, w.hi[src], w.lo[src], status, cap, shift, w.hist);
    uint32_t* tot = w.hist + (int64_t)nblk * 256;  // 256 words after the per-block table
    hipLaunchKernelGGL(radix_scan_kernel, dim3(256), dim3(256), 0, s, status, cap, w.hist, tot);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(256), 0, s, w.hi[src], w.lo[src], w.hi[dst], w.lo[dst], status, cap, shift, w.hist, tot);
    st.cur = dst;
    return check_launch("radix pass");
}

// YOLORT_AMD_NMS_BLOCK (default 1; read once per process): 0 sends the class-agnostic segments -- P keyed with label 0 -- through nms_segments_kernel, one wave per image:
// the bit-identical counterpart of nms_block_kernel, for tests and A/B
static bool nms_block_enabled() {
    static const bool on = getenv("YOLORT_AMD_NMS_BLOCK") ? atoi(getenv("YOLORT_AMD_NMS_BLOCK")) != 0 : true;
    return on;
}

// the radix passes over the key bits [lo, hi), 8 per pass
static int radix_passes(const Workspace& w, SortState& st, int* status, int cap, int lo, int hi, hipStream_t s) {
    int rc;
    for (int sh = lo; sh < hi; sh += 8)
        if ((rc = radix_pass(w, st, status, cap, sh, s)) != YMI_OK) return rc;
    return YMI_OK;
}

// The order P the NMS walks, from G (arrays w.hi/lo[g]): every record re-keyed with the low p_bits of its label (make_label_records_kernel, into the other pair), then
// stably sorted by that label.  p_bits == 0: every record is keyed with label 0 and no pass follows -- P is G's order, a segment is an image.  The label passes
// ping-pong between P and a scratch pair carved from kept_box / seg_start, which are not live yet (G must stay intact); a P that ends in the scratch is copied back.
static int label_order(const Workspace& w, int g, int* status, int cap, int p_bits, hipStream_t s, const uint64_t*& phi, const uint32_t*& plo) {
    const int p = g ^ 1;
    hipLaunchKernelGGL(make_label_records_kernel, dim3(cdiv(cap, 256)), dim3(256), 0, s, w.hi[g], w.lo[g], w.hi[p], w.lo[p], status, cap, p_bits, w.keep);
    Workspace wl = w;
    wl.hi[0] = w.hi[p];
    wl.lo[0] = w.lo[p];
    wl.hi[1] = reinterpret_cast<uint64_t*>(w.kept_box);        // cap * 16 bytes >= cap * 8
    wl.lo[1] = w.seg_start;                                   // cap * 4 bytes
    SortState sl{0};
    int rc;
    if ((rc = radix_passes(wl, sl, status, cap, 32, 32 + p_bits, s)) != YMI_OK) return rc;
    if (sl.cur == 1) {
        YMI_CHECK_HIP(hipMemcpyAsync(w.hi[p], wl.hi[1], (size_t)cap * 8, hipMemcpyDeviceToDevice, s));
        YMI_CHECK_HIP(hipMemcpyAsync(w.lo[p], wl.lo[1], (size_t)cap * 4, hipMemcpyDeviceToDevice, s));
    }
    phi = w.hi[p];
    plo = w.lo[p];
    return YMI_OK;
}

// segments of P, then the greedy NMS over them: a workgroup per segment (nms_block_kernel; `block`: the caller's segments are whole images) or a wave per segment
static void segments_nms(const Workspace& w, int g, const uint64_t* phi, const uint32_t* plo, int* status, int cap, int total_anchors, int label_bits, float nms_thresh,
                         bool block, int grid, hipStream_t s) {
    hipLaunchKernelGGL(find_segments_kernel, dim3(cdiv(cap, 256)), dim3(256), 0, s, phi, status, cap, w.seg_start);
    if (block)
        hipLaunchKernelGGL(nms_block_kernel, dim3(grid), dim3(NMSB_WAVES * 64), 0, s, phi, plo, w.hi[g], w.lo[g], w.boxes_all, total_anchors, label_bits, status, cap,
                           w.seg_start, w.kept_box, w.keep, nms_thresh);
    else
        hipLaunchKernelGGL(nms_segments_kernel, dim3(grid), dim3(256), 0, s, phi, plo, w.hi[g], w.lo[g], w.boxes_all, total_anchors, label_bits, status, cap,
                           w.seg_start, w.kept_box, w.keep, nms_thresh);
}

// segments -> NMS -> top-k gather of a descriptor's batch, given G (arrays w.hi/lo[g]) and the order P the NMS walks: per (image, class) by default, per image under
// YMI_POST_AGNOSTIC, where a segment gets a workgroup instead of a wave
static int nms_gather(const ymi_post_desc* d, const PostLayout& L, const Workspace& w, int g, const uint64_t* phi, const uint32_t* plo, hipStream_t s) {
    const bool agnostic = (d->flags & YMI_POST_AGNOSTIC) != 0;
    const bool block = agnostic && nms_block_enabled();   // at most n segments
    segments_nms(w, g, phi, plo, d->status, d->cand_cap, L.total_anchors, L.label_bits, d->nms_thresh, block, block ? d->n : 1024, s);
    const int K = d->detections_per_img;
    GatherArgs ga;
    ga.ghi = w.hi[g]; ga.glo = w.lo[g]; ga.keep = w.keep; ga.boxes_all = w.boxes_all; ga.rescale = d->rescale; ga.status = d->status;
    ga.truncated = L.per_image ? w.sel_count + d->n : nullptr; ga.status_rw = d->status; ga.out_slab = d->out_slab; ga.img_count = L.per_image ? w.img_count : nullptr;
    ga.cap = d->cand_cap; ga.total_anchors = L.total_anchors; ga.label_bits = L.label_bits; ga.K = K;
    ga.out_boxes = d->out_boxes; ga.out_scores = d->out_scores; ga.out_labels = d->out_labels; ga.out_count = d->out_count;
    if (d->flags & YMI_POST_MERGE) {   // merge-NMS: the reduction and the gather in one kernel, launched instead of the plain gather
        const size_t lds = merge_lds_bytes(K);
        if (lds > 64 * 1024) { const int rc_lds = allow_big_lds((const void*)merge_gather_kernel, (int)lds); if (rc_lds != YMI_OK) return rc_lds; }
        hipLaunchKernelGGL(merge_gather_kernel, dim3(d->n), dim3(MRG_THREADS), lds, s, ga, d->nms_thresh, agnostic ? 1 : 0, (d->flags & YMI_POST_MERGE_KEEP_SINGLE) ? 1 : 0,
                           merge_kept_cap(K));
        return check_launch("nms/merge_gather");
    }
    hipLaunchKernelGGL(gather_topk_kernel, dim3(d->n), dim3(256), 0, s, ga);
    return check_launch("nms/gather");
}

// the global-sort path: sorts the records in w.hi/lo[0] by (img, score desc, cand asc), then runs NMS + gather
static int sort_nms_gather(const ymi_post_desc* d, const PostLayout& L, const Workspace& w, hipStream_t s) {
    int rc;
    SortState st{0};
    if ((rc = radix_passes(w, st, d->status, d->cand_cap, 0, L.label_bits + L.anchor_bits, s)) != YMI_OK) return rc;
    if ((rc = radix_passes(w, st, d->status, d->cand_cap, 32, 64 + bits_for(d->n), s)) != YMI_OK) return rc;   // score, then image
    const uint64_t* phi;
    const uint32_t* plo;
    if ((rc = label_order(w, st.cur, d->status, d->cand_cap, (d->flags & YMI_POST_AGNOSTIC) ? 0 : L.label_bits, s, phi, plo)) != YMI_OK) return rc;
    return nms_gather(d, L, w, st.cur, phi, plo, s);
}

// The batch size a descriptor may carry: the per-image path ranks the whole batch through one LDS table (rank_image_kernel), and include/yolort_amd.h gives that limit
// for every path.  Checked when an op is added to a plan (api.cpp) and first thing in every stage, so a larger batch is refused before anything is enqueued.
int post_check_batch(const ymi_post_desc* d) {
    YMI_REQUIRE(d != nullptr, "ymi_postprocess: null descriptor");
    YMI_REQUIRE(d->n >= 1, "ymi_postprocess: batch size %d out of range", d->n);
    YMI_REQUIRE(d->n <= RANK_NIMG, "ymi_postprocess: more than %d images in a batch (got %d); split the batch", RANK_NIMG, d->n);
    return YMI_OK;
}

static int post_validate(const ymi_post_desc* d, bool need_logits, PostLayout& L, Workspace& w) {
    if (const int rc = post_check_batch(d)) return rc;
    YMI_REQUIRE(d->num_levels >= 1 && d->num_levels <= YMI_MAX_LEVELS, "ymi_postprocess: num_levels %d out of range", d->num_levels);
    YMI_REQUIRE(d->num_classes >= 1 && d->num_classes <= 4096, "ymi_postprocess: num_classes %d out of range", d->num_classes);
    YMI_REQUIRE(d->out_boxes && d->out_scores && d->out_labels && d->out_count && d->status && d->ws, "ymi_postprocess: null buffer");
    YMI_REQUIRE(d->detections_per_img >= 1 && d->cand_cap >= 1, "ymi_postprocess: detections_per_img and cand_cap must be positive");
    YMI_REQUIRE((d->flags & YMI_POST_MERGE) != 0 || (d->flags & YMI_POST_MERGE_KEEP_SINGLE) == 0, "ymi_postprocess: YMI_POST_MERGE_KEEP_SINGLE without YMI_POST_MERGE");
    for (int l = 0; l < d->num_levels; ++l) {
        YMI_REQUIRE(d->lh[l] >= 1 && d->lw[l] >= 1, "ymi_postprocess: level %d has an empty grid", l);
        if (need_logits) {
            YMI_REQUIRE(d->logits[l] != nullptr, "ymi_postprocess: logits[%d] is null", l);
            YMI_REQUIRE(d->lcstride[l] >= 3 * (d->num_classes + 5) && d->lcstride[l] % 4 == 0, "ymi_postprocess: lcstride[%d]=%d too small / not a multiple of 4", l, d->lcstride[l]);
        }
    }
    L = post_layout(d);
    YMI_REQUIRE(L.label_bits + L.anchor_bits <= 32, "ymi_postprocess: %d anchors x %d classes exceed the 32-bit candidate index", L.total_anchors, d->num_classes);
    w = carve(d->ws, d->n, L.total_anchors, d->cand_cap);
    YMI_REQUIRE(d->ws_bytes >= w.total, "ymi_postprocess: workspace too small (%lld < %lld)", (long long)d->ws_bytes, (long long)w.total);
    return YMI_OK;
}

// the three counter arrays of a batch in ONE launch (three hipMemsetAsync were three fill kernels of ~5.7 us each on the conv stack's stream, in front of the head:
// profiles/r06u_layer_table_c2.csv "other kernels")
__global__ __launch_bounds__(256) void post_reset_kernel(int* a, int na, int* b, int nb, int* c, int nc) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < na + nb + nc; i += gridDim.x * 256) {
        if (i < na) a[i] = 0;
        else if (i < na + nb) b[i - na] = 0;
        else c[i - na - nb] = 0;
    }
}

// stage 1 of 3: reset the counters the candidate producers append to
int post_begin_launch(const ymi_post_desc* d, hipStream_t s) {
    PostLayout L;
    Workspace w;
    int rc = post_validate(d, false, L, w);
    if (rc != YMI_OK) return rc;
    const int nc = L.per_image ? d->n : 0;
    hipLaunchKernelGGL(post_reset_kernel, dim3(cdiv(ST_WORDS + d->n + nc, 256)), dim3(256), 0, s, (int*)d->status, (int)ST_WORDS, (int*)d->out_count, d->n, nc ? (int*)w.img_count : nullptr, nc);
    return check_launch("post_reset_kernel");
}

// ---- class filter (YMI_POST_CLASS_FILTER): the allowed-class bit set lives in the workspace (Workspace::cmask), so changing the SET needs no new descriptor, no
// re-record of a plan and no re-capture of a graph.  The words travel BY VALUE as the kernel's argument: the caller's list is dead weight once the call returns, the
// launch is ordered on `s` like any other and can be captured.
struct ClassMaskWords { uint32_t w[CLASS_MASK_WORDS]; };
__global__ __launch_bounds__(CLASS_MASK_WORDS) void class_mask_write_kernel(uint32_t* dst, const ClassMaskWords m) {
    dst[threadIdx.x] = m.w[threadIdx.x];
}

int post_set_classes_launch(const ymi_post_desc* d, const int32_t* classes, int count, hipStream_t s) {
    YMI_REQUIRE(d != nullptr, "ymi_post_set_classes: null descriptor");
    YMI_REQUIRE((d->flags & YMI_POST_CLASS_FILTER) != 0, "ymi_post_set_classes: the descriptor's flags lack YMI_POST_CLASS_FILTER");
    YMI_REQUIRE(d->n >= 1 && d->cand_cap >= 1 && d->ws != nullptr, "ymi_post_set_classes: descriptor without a workspace");
    YMI_REQUIRE(d->num_levels >= 1 && d->num_levels <= YMI_MAX_LEVELS, "ymi_post_set_classes: num_levels %d out of range", d->num_levels);
    YMI_REQUIRE(d->num_classes >= 1 && d->num_classes <= 32 * CLASS_MASK_WORDS, "ymi_post_set_classes: num_classes %d out of range", d->num_classes);
    YMI_REQUIRE(count >= 0 && (count == 0 || classes != nullptr), "ymi_post_set_classes: bad class list");
    ClassMaskWords m;
    memset(&m, 0, sizeof(m));
    for (int i = 0; i < count; ++i) {
        const int c = classes[i];
        YMI_REQUIRE(c >= 0 && c < d->num_classes, "ymi_post_set_classes: class index %d outside [0, %d)", c, d->num_classes);
        m.w[c >> 5] |= 1u << (c & 31);
    }
    const PostLayout L = post_layout(d);
    const Workspace w = carve(d->ws, d->n, L.total_anchors, d->cand_cap);
    YMI_REQUIRE(d->ws_bytes >= w.total, "ymi_post_set_classes: workspace too small (%lld < %lld)", (long long)d->ws_bytes, (long long)w.total);
    hipLaunchKernelGGL(class_mask_write_kernel, dim3(1), dim3(CLASS_MASK_WORDS), 0, s, w.cmask, m);
    return check_launch("class_mask_write_kernel");
}

// DecodeArgs of level l of `src` feeding the sink of `d`.  `src` is the descriptor itself or a view (ymi_post_view): the two structs give a level's fields the same names
// (logits, lh, lw, lcstride, stride, anchors), which is all this template relies on.
template <class Levels>
static DecodeArgs level_args(const ymi_post_desc* d, const Workspace& w, const PostLayout& L, const Levels* src, int l, int level_off) {
    DecodeArgs a;
    a.logits = src->logits[l]; a.h = src->lh[l]; a.w = src->lw[l]; a.cs = src->lcstride[l]; a.stride = src->stride[l];
    for (int k = 0; k < 6; ++k) a.anc[k] = src->anchors[l][k];
    a.n = d->n; a.K = d->num_classes + 5; a.level_off = level_off;
    a.sink = make_sink(d, w, L);
    return a;
}
// blocks of four waves that walk DEC_PIX_PER_WAVE pixels each
static dim3 decode_grid(const DecodeArgs& a) {
    const int64_t npix = (int64_t)a.n * a.h * a.w;
    return dim3((unsigned)((npix + 4 * DEC_PIX_PER_WAVE - 1) / (4 * DEC_PIX_PER_WAVE)));
}

// stage 2 of 3 (unfused form): decode + threshold of the fp32 head outputs
static int post_decode_launch(const ymi_post_desc* d, hipStream_t s) {
    PostLayout L;
    Workspace w;
    int rc = post_validate(d, true, L, w);
    if (rc != YMI_OK) return rc;
    int level_off = 0;
    for (int l = 0; l < d->num_levels; ++l) {
        const DecodeArgs a = level_args(d, w, L, d, l, level_off);
        hipLaunchKernelGGL(decode_kernel, decode_grid(a), dim3(256), 0, s, a);
        level_off += 3 * a.h * a.w;
    }
    return check_launch("decode_kernel");
}

// stage 2 of 3, augmented inference: decode + threshold of one view's fp32 head outputs into its range of the sink's concatenated anchor axis
int post_decode_view_launch(const ymi_post_desc* d, const ymi_post_view* v, hipStream_t s) {
    YMI_REQUIRE(v != nullptr, "ymi_post_decode_view: null view");
    PostLayout L;
    Workspace w;
    int rc = post_validate(d, false, L, w);
    if (rc != YMI_OK) return rc;
    YMI_REQUIRE(v->num_levels >= 1 && v->num_levels <= YMI_MAX_LEVELS, "ymi_post_decode_view: num_levels %d out of range", v->num_levels);
    YMI_REQUIRE(v->scale > 0.f && v->scale <= 1.f, "ymi_post_decode_view: scale %g outside (0, 1]", (double)v->scale);
    YMI_REQUIRE(v->flip_w >= 0 && v->flip_w < (1 << 24), "ymi_post_decode_view: flip_w %d out of range", v->flip_w);
    YMI_REQUIRE(v->anchor_base >= 0 && (v->skip_mask >> v->num_levels) == 0, "ymi_post_decode_view: negative anchor_base / skip_mask names a level the view does not have");
    int64_t kept = 0;
    for (int l = 0; l < v->num_levels; ++l) {
        if ((v->skip_mask >> l) & 1) continue;
        YMI_REQUIRE(v->lh[l] >= 1 && v->lw[l] >= 1, "ymi_post_decode_view: level %d has an empty grid", l);
        YMI_REQUIRE(v->logits[l] != nullptr, "ymi_post_decode_view: logits[%d] is null", l);
        YMI_REQUIRE(v->lcstride[l] >= 3 * (d->num_classes + 5) && v->lcstride[l] % 4 == 0, "ymi_post_decode_view: lcstride[%d]=%d too small / not a multiple of 4", l, v->lcstride[l]);
        kept += (int64_t)3 * v->lh[l] * v->lw[l];
    }
    YMI_REQUIRE((int64_t)v->anchor_base + kept <= L.total_anchors, "ymi_post_decode_view: anchors [%d, %lld) of the view exceed the sink's %d", v->anchor_base,
                (long long)(v->anchor_base + kept), L.total_anchors);
    int level_off = v->anchor_base;
    for (int l = 0; l < v->num_levels; ++l) {
        if ((v->skip_mask >> l) & 1) continue;   // a clipped tail: no launch, no anchor indices
        const DecodeViewArgs va = {level_args(d, w, L, v, l, level_off), v->scale, (float)v->flip_w};
        hipLaunchKernelGGL(decode_view_kernel, decode_grid(va.d), dim3(256), 0, s, va);
        level_off += 3 * va.d.h * va.d.w;
    }
    return check_launch("decode_view_kernel");
}

// stage 3 of 3: sort, class-aware NMS, top-k + rescale, from the records the producers appended
int post_finish_launch(const ymi_post_desc* d, hipStream_t s) {
    PostLayout L;
    Workspace w;
    int rc = post_validate(d, false, L, w);
    if (rc != YMI_OK) return rc;
    if (L.per_image) {
        const int p_bits = (d->flags & YMI_POST_AGNOSTIC) ? 0 : L.label_bits;   // label bits of the P keys: none under YMI_POST_AGNOSTIC (P is G's order, one segment per image)
        const int cap_img = L.cap_img;
        const bool exact_full = (d->flags & YMI_POST_EXACT_FULL) != 0;
        const int sel_t = exact_full ? 0 : (4 * d->detections_per_img > 4096 ? 4 * d->detections_per_img : 4096);
        // rank counters live in seg_start / kept_box, which are not in use before find_segments
        uint32_t* rank_g = w.seg_start;
        uint32_t* rank_p = reinterpret_cast<uint32_t*>(w.kept_box);
        // multi-block selection for large per-image regions; its scratch -- (n, 4096) bin and (n, 2048) digit histograms, n fill counters, n states -- lives in the P
        // arrays, which nothing uses before scatter_ranks_kernel (cap_img * 8 bytes per image against 24 KiB + 36)
        // (few images only: with 32 or more the one-block-per-image form already spreads over enough CUs, and the ladder's extra passes cost throughput)
        static const int multi_max_n = getenv("YOLORT_AMD_SEL_MULTI_MAXN") ? atoi(getenv("YOLORT_AMD_SEL_MULTI_MAXN")) : 32;   // tuning aid
        const bool multi = sel_t > 0 && cap_img >= 2 * SEL_SLICE && d->n < multi_max_n && getenv("YOLORT_AMD_SEL_SINGLE") == nullptr;
        int* ghist = reinterpret_cast<int*>(w.p_hi);
        int* rhist = ghist + (int64_t)d->n * SEL_BINS;
        int* gfill = rhist + (int64_t)d->n * SEL_RBINS;
        int* sel_state = gfill + d->n;
        const int nslices = cdiv(cap_img, SEL_SLICE);
        if (multi) {
            YMI_CHECK_HIP(hipMemsetAsync(ghist, 0, (size_t)d->n * (SEL_BINS + SEL_RBINS + 1 + SEL_STATE) * sizeof(int), s));
            hipLaunchKernelGGL(sel_hist_kernel, dim3(nslices, d->n), dim3(1024), 0, s, w.hi[0], w.img_count, cap_img, sel_t, ghist);
        }
        hipLaunchKernelGGL(select_prefix_kernel, dim3(d->n), dim3(1024), 0, s, w.hi[0], w.lo[0], w.img_count, cap_img, d->n, sel_t, w.sel_count, rank_g, rank_p,
                           multi ? ghist : nullptr, multi ? sel_state : nullptr);
        if (multi) {
            // the refinement ladder: a fixed number of (count, decide) pairs -- the launch sequence must not depend on the data; levels an image does not need return at once
            for (int l = 0; l < SEL_LEVELS; ++l) {
                hipLaunchKernelGGL(sel_rhist_kernel, dim3(nslices, d->n), dim3(1024), 0, s, w.hi[0], w.lo[0], w.img_count, cap_img, sel_state, rhist);
                hipLaunchKernelGGL(sel_rpick_kernel, dim3(d->n), dim3(64), 0, s, sel_state, rhist, w.sel_count);
            }
            hipLaunchKernelGGL(sel_compact_kernel, dim3(nslices, d->n), dim3(1024), 0, s, w.hi[0], w.lo[0], w.img_count, cap_img, sel_state, gfill, w.hi[1], w.lo[1]);
            hipLaunchKernelGGL(sel_copyback_kernel, dim3(cdiv(RANK_MAX, 256), d->n), dim3(256), 0, s, w.hi[0], w.lo[0], w.hi[1], w.lo[1], sel_state, w.sel_count, cap_img);
        }
        const int rank_cap = cap_img < RANK_MAX ? cap_img : RANK_MAX;   // no image holds more than cap_img records; one that keeps more than RANK_MAX is sort_image_kernel's
        hipLaunchKernelGGL(rank_image_kernel, dim3(RANK_GRID), dim3(RANK_IT), 0, s, w.hi[0], w.lo[0], w.sel_count, d->n, cap_img,
                           p_bits, rank_g, rank_p);
        hipLaunchKernelGGL(scatter_ranks_kernel, dim3(cdiv(rank_cap, RANK_IT), d->n), dim3(RANK_IT), 0, s, w.hi[0], w.lo[0], w.img_count, w.sel_count, cap_img, p_bits,
                           rank_g, rank_p, w.hi[1], w.lo[1], w.p_hi, w.p_lo, w.keep, d->status);
        // LDS run length of the sort: with the prefix selection images rarely exceed 8192 records (longer ones take the
        // multi-run merge path), and 64 KiB instead of 128 leaves room for a convolution block on the same CU
        const int run_max = exact_full ? IMG_SORT_MAX : IMG_SORT_MAX / 2;
        const int lds_keys = cap_img < run_max ? cap_img : run_max;
        const size_t lds = (size_t)lds_keys * 8;
        if (lds > 64 * 1024) { const int rc_lds = allow_big_lds((const void*)sort_image_kernel, (int)lds); if (rc_lds != YMI_OK) return rc_lds; }
        // the producers wrote arrays [0] (per-image regions); G goes to arrays [1] (compact), P to its own pair
        if (cap_img > RANK_MAX)   // only then can an image exceed the ranking path
            hipLaunchKernelGGL(sort_image_kernel, dim3(d->n), dim3(1024), lds, s, w.hi[0], w.lo[0], w.img_count, w.sel_count, cap_img, d->n, p_bits, lds_keys,
                               RANK_MAX, w.hi[1], w.lo[1], w.p_hi, w.p_lo, w.keep, d->status);
        if ((rc = check_launch("select_prefix/sort_image")) != YMI_OK) return rc;
        return nms_gather(d, L, w, 1, w.p_hi, w.p_lo, s);
    }
    hipLaunchKernelGGL(finalize_count_kernel, dim3(1), dim3(64), 0, s, d->status, d->cand_cap);
    rc = check_launch("finalize_count");
    if (rc != YMI_OK) return rc;
    return sort_nms_gather(d, L, w, s);
}

int postprocess_launch(const ymi_post_desc* d, hipStream_t s) {
    int rc = post_begin_launch(d, s);
    if (rc != YMI_OK) return rc;
    if ((rc = post_decode_launch(d, s)) != YMI_OK) return rc;
    return post_finish_launch(d, s);
}

// ---- stand-alone batched NMS (one image) -------------------------------------------------
constexpr int NMS_LABEL_BITS = 12;

// Sort key of an arbitrary (non-NaN) float score, ascending key == descending score: the order-preserving map of IEEE floats to unsigned (all bits of a negative
// value flipped, the sign bit of a non-negative one set), complemented.  -0.0 is +0.0 first: the two compare equal, so they must tie (and fall back to index order).
__device__ __forceinline__ uint32_t nms_score_key(float score) {
    uint32_t u = __float_as_uint(score);
    if (u == 0x80000000u) u = 0u;
    const uint32_t ascending = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~ascending;
}

__global__ __launch_bounds__(256) void nms_make_records_kernel(const float* boxes, const float* scores, const int* labels, int n, float* boxes_all,
                                                               uint64_t* hi, uint32_t* lo, int* status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { status[ST_NCAND] = n; status[ST_OVERFLOW] = 0; status[ST_NSEG] = 0; status[ST_RSV] = 0; }
    if (i >= n) return;
    *reinterpret_cast<f32x4*>(boxes_all + (int64_t)i * 4) = *reinterpret_cast<const f32x4*>(boxes + (int64_t)i * 4);
    hi[i] = (uint64_t)nms_score_key(scores[i]);
    lo[i] = ((unsigned)i << NMS_LABEL_BITS) | (labels != nullptr ? (unsigned)labels[i] & ((1u << NMS_LABEL_BITS) - 1u) : 0u);   // labels == NULL: ymi_nms
}

__global__ __launch_bounds__(256) void nms_emit_keep_kernel(const uint32_t* glo, const uint8_t* keep, int n, int* keep_out, int* count_out) {
    // single block: ordered compaction of kept ranks -> original indices
    __shared__ int wave_cnt[4];
    __shared__ int s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (int c = 0; c < n; c += 256) {
        const int r = c + threadIdx.x;
        const bool k = r < n && keep[r] != 0;
        const uint64_t m = __ballot(k);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; ++w) off += wave_cnt[w];
        if (k) keep_out[off + __popcll(m & lt)] = (int)(glo[r] >> NMS_LABEL_BITS);
        __syncthreads();
        if (threadIdx.x == 0) s_base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count_out = s_base;
}

// ------------------------------------------------------------------------------------------
// 7. COCO matching (ymi_eval_match, include/yolort_amd.h): the greedy detection <-> ground-truth matching of yolort_amd/utils/metrics.py coco_ap for the slab, every
//    (class, threshold) of one (image, area range) in one workgroup.  The image's detections and ground truths are staged in LDS; a detection's rank within its
//    (image, class) score order is a count over the staged detections; the waves take the classes present in the image in turn (the n-th rank-0 detection of the
//    slab names the n-th class).  Per class a wave lists its detections in rank order and its ground truths in walk order (non-ignored first), then walks the
//    detections: lanes run over walk positions strided by 64 and keep, per threshold, the largest key (non-ignored << 63 | IoU bits << 16 | walk position) among
//    the unused ground truths that qualify -- a qualifying IoU is a positive float, whose bits order as the floats do; the larger position breaks a tie as the
//    host's `not <` does --, a wave arg-max picks the winner, and the lane that owns the winner's position sets bit t of its 16-bit `used` word.
//    (double)IoU >= t' is evaluated as IoU >= thr with thr the smallest fp32 not below t' (the launcher computes it): the same predicate on fp32 IoUs.
// ------------------------------------------------------------------------------------------
constexpr int EVM_WAVES = 16;     // a power of two: classes are dealt to the waves round-robin (an image of the C2 workload holds ~60 classes)
constexpr int EVM_IGN = 0x4000;   // a staged ground-truth label carries its ignore flag here (num_classes <= 4096)

struct EvalArgs {
    const float* boxes;
    const float* scores;
    const int64_t* labels;
    const int* counts;
    const float* gt_boxes;
    const int* gt_labels;
    const int* gt_counts;
    uint16_t* tp;
    uint16_t* ig;
    int* rank;
    int* n_gt;
    int* status;
    int N, K, G, T, R, C, max_dets;
    float thr[YMI_EVAL_MAX_THRS];
    float lo[YMI_EVAL_MAX_RNGS], hi[YMI_EVAL_MAX_RNGS];
};

// byte offsets of the kernel's LDS arrays for slabs of K detections and G ground truths per image
struct EvalLds {
    int db, gb, ds, dl, dr, gl, wave0, wave_bytes, ord, walk, used, total;
};
__host__ __device__ inline EvalLds eval_lds(int K, int G) {
    EvalLds L;
    auto up = [](int v) { return (v + 15) & ~15; };
    int off = 0;
    L.db = off; off += K * 16;          // f32x4[K] detection boxes
    L.gb = off; off += G * 16;          // f32x4[G] ground-truth boxes
    L.ds = off; off += up(K * 4);       // float[K] scores
    L.dl = off; off += up(K * 2);       // int16[K] labels, -1 = skipped
    L.dr = off; off += up(K * 2);       // int16[K] ranks, -1 = takes no part
    L.gl = off; off += up(G * 2);       // int16[G] labels | EVM_IGN, -1 = skipped
    L.wave0 = off;
    L.ord = 0;                          // per wave: uint16[K] slab slot of the class's rank-th detection
    L.walk = up(K * 2);                 //           uint16[G] ground-truth slot at each walk position
    L.used = L.walk + up(G * 2);        //           uint16[G] bit t = taken at threshold t, by walk position
    L.wave_bytes = L.used + up(G * 2);
    L.total = off + EVM_WAVES * L.wave_bytes;
    return L;
}

__device__ __forceinline__ float eval_area(const f32x4 b) { return __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1])); }

// metrics.py _iou_matrix in its order: inter / (((aa + ab) - inter) + 1e-12f)
__device__ __forceinline__ float eval_iou(const f32x4 a, float aa, const f32x4 b) {
    const float x1 = a[0] > b[0] ? a[0] : b[0], y1 = a[1] > b[1] ? a[1] : b[1];
    const float x2 = a[2] < b[2] ? a[2] : b[2], y2 = a[3] < b[3] ? a[3] : b[3];
    float iw = __fsub_rn(x2, x1), ih = __fsub_rn(y2, y1);
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = __fmul_rn(iw, ih);
    const float ab = eval_area(b);
    return __fdiv_rn(inter, __fadd_rn(__fsub_rn(__fadd_rn(aa, ab), inter), 1e-12f));
}

__global__ __launch_bounds__(EVM_WAVES * 64) void eval_match_kernel(const EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_key[];
    const int img = blockIdx.x, r = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const EvalLds L = eval_lds(a.K, a.G);
    char* lds = reinterpret_cast<char*>(lds_key);
    f32x4* db = reinterpret_cast<f32x4*>(lds + L.db);
    f32x4* gb = reinterpret_cast<f32x4*>(lds + L.gb);
    float* ds = reinterpret_cast<float*>(lds + L.ds);
    int16_t* dl = reinterpret_cast<int16_t*>(lds + L.dl);
    int16_t* dr = reinterpret_cast<int16_t*>(lds + L.dr);
    int16_t* gl = reinterpret_cast<int16_t*>(lds + L.gl);
    uint16_t* ord = reinterpret_cast<uint16_t*>(lds + L.wave0 + wave * L.wave_bytes + L.ord);
    uint16_t* walk = reinterpret_cast<uint16_t*>(lds + L.wave0 + wave * L.wave_bytes + L.walk);
    uint16_t* used = reinterpret_cast<uint16_t*>(lds + L.wave0 + wave * L.wave_bytes + L.used);

    const int kd_raw = a.counts[img];
    if (kd_raw < 0) {   // a stale slab row: the image is skipped (block-uniform, before any barrier)
        if (threadIdx.x == 0) atomicOr(&a.status[1], YMI_EVAL_STATUS_STALE_ROW);
        return;
    }
    const int kd = kd_raw < a.K ? kd_raw : a.K;
    const int gn_raw = a.gt_counts[img];
    const int gn = gn_raw < 0 ? 0 : (gn_raw < a.G ? gn_raw : a.G);
    const float lo = a.lo[r], hi = a.hi[r];
    const int64_t drow = (int64_t)img * a.K, grow = (int64_t)img * a.G, orow = ((int64_t)r * a.N + img) * a.K;

    // ---- stage the image; count its non-ignored ground truths ----
    bool bad = false;
    for (int j = threadIdx.x; j < kd; j += EVM_WAVES * 64) {
        db[j] = *reinterpret_cast<const f32x4*>(a.boxes + (drow + j) * 4);
        ds[j] = a.scores[drow + j];
        const int64_t l = a.labels[drow + j];
        const bool ok = l >= 0 && l < a.C;
        dl[j] = ok ? (int16_t)l : (int16_t)-1;
        bad |= !ok;
    }
    for (int g = threadIdx.x; g < gn; g += EVM_WAVES * 64) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.gt_boxes + (grow + g) * 4);
        gb[g] = b;
        const int l = a.gt_labels[grow + g];
        const bool ok = l >= 0 && l < a.C;
        bad |= !ok;
        int16_t v = -1;
        if (ok) {
            const float ar = eval_area(b);
            const bool ign = ar < lo || ar > hi;
            v = (int16_t)(l | (ign ? EVM_IGN : 0));
            if (!ign) atomicAdd(&a.n_gt[r * a.C + l], 1);
        }
        gl[g] = v;
    }
    if (bad) atomicOr(&a.status[1], YMI_EVAL_STATUS_BAD_LABEL);
    __syncthreads();

    // ---- rank within (image, class): detections of the class that sort before this one (score descending, slab order among equals, NaN last) ----
    for (int j = threadIdx.x; j < kd; j += EVM_WAVES * 64) {
        const int l = dl[j];
        int rk = -1;
        if (l >= 0) {
            const float s = ds[j];
            const bool s_nan = s != s;   // a total order, as the host's stable argsort of -score has it: NaN scores last, in slab order among themselves
            rk = 0;
            for (int q = 0; q < kd; ++q) {
                const float sq = ds[q];
                const bool before = s_nan ? (sq == sq || q < j) : (sq > s || (sq == s && q < j));
                rk += (dl[q] == l && before) ? 1 : 0;
            }
            if (a.max_dets > 0 && rk >= a.max_dets) rk = -1;
        }
        dr[j] = (int16_t)rk;
        if (r == 0) a.rank[drow + j] = rk;
        if (rk < 0) {   // takes no part: its flags are defined (0) all the same
            a.tp[orow + j] = 0;
            a.ig[orow + j] = 0;
        }
    }
    __syncthreads();

    // ---- the classes present, dealt to the waves in slab order of their rank-0 detections (wave-uniform from here on: no block barrier below) ----
    int leader = 0;
    for (int b0 = 0; b0 < kd; b0 += 64) {
        uint64_t lead = __ballot(b0 + lane < kd && dr[b0 + lane < kd ? b0 + lane : 0] == 0);
        while (lead) {
            const int li = __ffsll((long long)lead) - 1;
            lead &= lead - 1;
            if ((leader++ & (EVM_WAVES - 1)) != wave) continue;
            const int c = dl[b0 + li];

            // the class's detections by rank, its ground truths by walk position
            int nd = 0;
            for (int b = 0; b < kd; b += 64) {
                const int j = b + lane;
                const bool m = j < kd && dl[j] == c && dr[j] >= 0;
                if (m) ord[dr[j]] = (uint16_t)j;
                nd += __popcll(__ballot(m));
            }
            int nn = 0;
            for (int b = 0; b < gn; b += 64) {
                const int g = b + lane;
                const bool m = g < gn && gl[g] == c;
                const uint64_t mm = __ballot(m);
                if (m) walk[nn + __popcll(mm & lt)] = (uint16_t)g;
                nn += __popcll(mm);
            }
            int ngc = nn;
            for (int b = 0; b < gn; b += 64) {
                const int g = b + lane;
                const bool m = g < gn && gl[g] == (c | EVM_IGN);
                const uint64_t mm = __ballot(m);
                if (m) walk[ngc + __popcll(mm & lt)] = (uint16_t)g;
                ngc += __popcll(mm);
            }
            for (int p = lane; p < ngc; p += 64) used[p] = 0;
            __builtin_amdgcn_wave_barrier();   // ord / walk: written by one lane, read by the others

            for (int k = 0; k < nd; ++k) {
                const int j = ord[k];
                const f32x4 bd = db[j];
                const float ad = eval_area(bd);
                const bool d_out = ad < lo || ad > hi;
                uint64_t best[YMI_EVAL_MAX_THRS];
#pragma unroll
                for (int t = 0; t < YMI_EVAL_MAX_THRS; ++t) best[t] = 0ull;
                for (int p = lane; p < ngc; p += 64) {
                    const float iou = eval_iou(bd, ad, gb[walk[p]]);
                    const unsigned u = used[p];
                    const uint64_t key = ((uint64_t)(p < nn ? 1 : 0) << 63) | ((uint64_t)__float_as_uint(iou) << 16) | (uint64_t)p;
#pragma unroll
                    for (int t = 0; t < YMI_EVAL_MAX_THRS; ++t)
                        if (t < a.T && !((u >> t) & 1u) && iou >= a.thr[t] && key > best[t]) best[t] = key;
                }
                unsigned tpw = 0, igw = 0;
#pragma unroll
                for (int t = 0; t < YMI_EVAL_MAX_THRS; ++t) {
                    if (t >= a.T) continue;
                    uint64_t kb = best[t];
                    const uint64_t has = __ballot(kb != 0ull);
                    if (has == 0ull) {
                        if (d_out) igw |= 1u << t;
                        continue;
                    }
                    if (has & (has - 1)) {
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) {
                            const uint64_t other = __shfl_xor(kb, o, 64);
                            kb = other > kb ? other : kb;
                        }
                    } else {
                        kb = __shfl(kb, __ffsll((long long)has) - 1, 64);
                    }
                    const int p = (int)(kb & 0xffffull);
                    if ((p & 63) == lane) used[p] = (uint16_t)(used[p] | (1u << t));   // read back by this lane only (its own positions)
                    if (kb >> 63) tpw |= 1u << t; else igw |= 1u << t;
                }
                if (lane == 0) {
                    a.tp[orow + j] = (uint16_t)tpw;
                    a.ig[orow + j] = (uint16_t)igw;
                }
            }
            __builtin_amdgcn_wave_barrier();   // the next class rewrites ord / walk
        }
    }
}

static int eval_match_launch(const ymi_eval_desc* d, hipStream_t s) {
    YMI_REQUIRE(d != nullptr, "ymi_eval_match: null descriptor");
    YMI_REQUIRE(d->n >= 0 && d->k >= 0 && d->k <= YMI_EVAL_MAX_PER_IMAGE && d->g >= 0 && d->g <= YMI_EVAL_MAX_PER_IMAGE,
                "ymi_eval_match: n=%d k=%d g=%d out of range (k, g <= %d per image)", d->n, d->k, d->g, YMI_EVAL_MAX_PER_IMAGE);
    YMI_REQUIRE(d->num_thrs >= 1 && d->num_thrs <= YMI_EVAL_MAX_THRS, "ymi_eval_match: %d thresholds (1 .. %d)", d->num_thrs, YMI_EVAL_MAX_THRS);
    YMI_REQUIRE(d->num_rngs >= 1 && d->num_rngs <= YMI_EVAL_MAX_RNGS, "ymi_eval_match: %d area ranges (1 .. %d)", d->num_rngs, YMI_EVAL_MAX_RNGS);
    YMI_REQUIRE(d->num_classes >= 1 && d->num_classes <= 4096, "ymi_eval_match: num_classes=%d (1 .. 4096)", d->num_classes);
    YMI_REQUIRE(d->max_dets >= 0, "ymi_eval_match: max_dets=%d (0 = no cut)", d->max_dets);
    EvalArgs a;
    for (int t = 0; t < YMI_EVAL_MAX_THRS; ++t) a.thr[t] = INFINITY;
    for (int t = 0; t < d->num_thrs; ++t) {
        YMI_REQUIRE(d->thrs[t] > 0.0 && d->thrs[t] <= 1.0, "ymi_eval_match: threshold %d = %g outside (0, 1]", t, d->thrs[t]);
        const double tq = d->thrs[t] < 1.0 - 1e-10 ? d->thrs[t] : 1.0 - 1e-10;   // min(t, 1 - 1e-10) of the host loop
        float f = (float)tq;
        if ((double)f < tq) f = nextafterf(f, INFINITY);   // the smallest fp32 not below it: (double)iou >= tq  <=>  iou >= f
        a.thr[t] = f;
    }
    for (int r = 0; r < YMI_EVAL_MAX_RNGS; ++r) {
        a.lo[r] = r < d->num_rngs ? d->area_rng[r][0] : 0.f;
        a.hi[r] = r < d->num_rngs ? d->area_rng[r][1] : 0.f;
    }
    if (d->n == 0) return YMI_OK;
    YMI_REQUIRE(d->counts && d->gt_counts && d->tp && d->ig && d->rank && d->n_gt && d->status, "ymi_eval_match: null buffer");
    YMI_REQUIRE(d->k == 0 || (d->boxes && d->scores && d->labels), "ymi_eval_match: null detection buffer");
    YMI_REQUIRE(d->g == 0 || (d->gt_boxes && d->gt_labels), "ymi_eval_match: null ground-truth buffer");
    a.boxes = d->boxes; a.scores = d->scores; a.labels = d->labels; a.counts = d->counts;
    a.gt_boxes = d->gt_boxes; a.gt_labels = d->gt_labels; a.gt_counts = d->gt_counts;
    a.tp = d->tp; a.ig = d->ig; a.rank = d->rank; a.n_gt = d->n_gt; a.status = d->status;
    a.N = d->n; a.K = d->k; a.G = d->g; a.T = d->num_thrs; a.R = d->num_rngs; a.C = d->num_classes; a.max_dets = d->max_dets;
    const size_t lds = (size_t)eval_lds(d->k, d->g).total;
    if (lds > 64 * 1024) { const int rc_lds = allow_big_lds((const void*)eval_match_kernel, (int)lds); if (rc_lds != YMI_OK) return rc_lds; }
    hipLaunchKernelGGL(eval_match_kernel, dim3(d->n, d->num_rngs), dim3(EVM_WAVES * 64), lds, s, a);
    return check_launch("eval_match_kernel");
}

}  // namespace ymi

using namespace ymi;

extern "C" int64_t ymi_postprocess_ws_bytes(int n, int total_anchors, int cand_cap) {
    if (n <= 0 || total_anchors <= 0 || cand_cap <= 0) return 0;
    return carve(nullptr, n, total_anchors, cand_cap).total;
}

extern "C" int64_t ymi_post_class_mask_offset(int n, int total_anchors, int cand_cap) {
    if (n <= 0 || total_anchors <= 0 || cand_cap <= 0) return YMI_EINVAL;
    return carve(nullptr, n, total_anchors, cand_cap).cmask_off;
}
extern "C" int ymi_post_set_classes(const ymi_post_desc* d, const int32_t* classes, int count, void* stream) { return post_set_classes_launch(d, classes, count, (hipStream_t)stream); }

extern "C" int ymi_postprocess(const ymi_post_desc* d, void* stream) { return postprocess_launch(d, (hipStream_t)stream); }
extern "C" int ymi_post_begin(const ymi_post_desc* d, void* stream) { return post_begin_launch(d, (hipStream_t)stream); }
extern "C" int ymi_post_finish(const ymi_post_desc* d, void* stream) { return post_finish_launch(d, (hipStream_t)stream); }
extern "C" int ymi_post_decode_view(const ymi_post_desc* sink, const ymi_post_view* view, void* stream) { return post_decode_view_launch(sink, view, (hipStream_t)stream); }

extern "C" int ymi_eval_match(const ymi_eval_desc* d, void* stream) { return eval_match_launch(d, (hipStream_t)stream); }

extern "C" int64_t ymi_nms_ws_bytes(int n) {
    if (n <= 0) n = 1;
    return carve(nullptr, 1, n, n).total + 256 /* status */ + 2 * 256;
}

// the two stand-alone entry points: records from the caller's arrays, sort by (score desc, index asc), P keyed by label, segments + NMS, ordered emit of the kept indices.
// labels == NULL is ymi_nms (torchvision.ops.nms): every record is keyed with label 0 -- nothing to sort below the index, no label passes, ONE segment -- and the
// segment gets a workgroup (nms_block_kernel) unless YOLORT_AMD_NMS_BLOCK=0
static int nms_standalone(const char* what, const float* boxes, const float* scores, const int32_t* labels, bool need_labels, int n, float nms_thresh, int32_t* keep_out,
                          int32_t* count_out, void* ws, int64_t ws_bytes, hipStream_t s) {
    YMI_REQUIRE(count_out && ws, "%s: null buffer", what);
    if (n == 0) {
        YMI_CHECK_HIP(hipMemsetAsync(count_out, 0, sizeof(int), s));
        return YMI_OK;
    }
    YMI_REQUIRE(boxes && scores && (labels || !need_labels) && keep_out, "%s: null buffer", what);
    YMI_REQUIRE(n > 0 && n < (1 << (32 - NMS_LABEL_BITS)), "%s: n=%d out of range (max %d)", what, n, (1 << (32 - NMS_LABEL_BITS)) - 1);
    YMI_REQUIRE(ws_bytes >= ymi_nms_ws_bytes(n), "%s: workspace too small", what);
    int* status = (int*)ws;
    const Workspace w = carve((char*)ws + 256, 1, n, n);
    hipLaunchKernelGGL(nms_make_records_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, boxes, scores, labels, n, w.boxes_all, w.hi[0], w.lo[0], status);
    // (no slab outputs: the stand-alone path skips the gather and emits the kept indices itself)
    const int p_bits = labels ? NMS_LABEL_BITS : 0;
    int rc;
    SortState st{0};
    if ((rc = radix_passes(w, st, status, n, NMS_LABEL_BITS - p_bits, NMS_LABEL_BITS + bits_for(n), s)) != YMI_OK) return rc;
    if ((rc = radix_passes(w, st, status, n, 32, 64, s)) != YMI_OK) return rc;
    const uint64_t* phi;
    const uint32_t* plo;
    if ((rc = label_order(w, st.cur, status, n, p_bits, s, phi, plo)) != YMI_OK) return rc;
    const bool block = labels == nullptr && nms_block_enabled();
    segments_nms(w, st.cur, phi, plo, status, n, n, NMS_LABEL_BITS, nms_thresh, block, labels ? 256 : 1, s);
    hipLaunchKernelGGL(nms_emit_keep_kernel, dim3(1), dim3(256), 0, s, w.lo[st.cur], w.keep, n, keep_out, count_out);
    return check_launch(what);
}

extern "C" int ymi_batched_nms(const float* boxes, const float* scores, const int32_t* labels, int n, float nms_thresh, int32_t* keep_out,
                               int32_t* count_out, void* ws, int64_t ws_bytes, void* stream) {
    return nms_standalone("ymi_batched_nms", boxes, scores, labels, true, n, nms_thresh, keep_out, count_out, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ymi_nms(const float* boxes, const float* scores, int n, float nms_thresh, int32_t* keep_out, int32_t* count_out, void* ws, int64_t ws_bytes, void* stream) {
    return nms_standalone("ymi_nms", boxes, scores, nullptr, false, n, nms_thresh, keep_out, count_out, ws, ws_bytes, (hipStream_t)stream);
}
