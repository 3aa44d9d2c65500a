// YOLOv5 validation matching (ymi_val_match, include/yolort_amd.h): the one-to-one detection <-> ground-truth assignment by IoU of ultralytics' val.py -- the
// confusion matrix (yolort/v5/utils/metrics.py:133-171) and the per-threshold true-positive flags ap_per_class consumes -- for the detection slab, one workgroup
// per image, one launch per batch.
//
// How the work is split.  The image's ground truths are staged in LDS (boxes, classes, one 64-bit key each); the detections are NOT staged: a detection is looked at
// by exactly one group of lanes, which reads its box, score and label straight from the slab.
//   pass 1   A wave is cut into 64 / W groups of W lanes, W = the power of two in [8, 64] that covers the image's ground truths (an image of the C2 workload holds
//            ~10: eight detections per wave step instead of one).  A group takes one detection; its lanes run over the ground truths strided by W and keep the
//            largest key (IoU bits << 32 | ~ground-truth index) among the admissible pairs -- an admissible IoU is a non-negative float, whose bits order as the
//            floats do, and the inverted index sends a tie to the lowest ground truth.  A xor-butterfly of log2 W steps (it never leaves the group) is the arg-max.
//            The group's first lane leaves (IoU, ground truth, label) in the LDS table of the detection and folds (IoU bits << 32 | ~slot) into the ground truth's
//            key with ONE 64-bit LDS atomic max.
//   pass 2   is that atomic: after the barrier a ground truth's key names, among the detections that chose it, the one of the largest IoU, the lowest slot among
//            equals.  No IoU is computed twice, nothing is sorted, and the order in which the waves arrive cannot change the result (max is order-free).
//   outputs  A thread per slot compares its table entry with its ground truth's key: equal slot = matched, anything else = unmatched (a displaced detection does
//            not fall back).  Every slot of the slab row is written.
//   matrix   When (nc + 1)^2 counters fit beside the staging in 64 KiB of LDS (nc = 80: 26 KiB) the image's additions go to an LDS matrix and only its non-zero
//            cells are flushed with global atomics; otherwise they go straight to global memory.  Integer atomics both ways.
#include <math.h>

#include "post_common.hpp"

namespace ymi {

constexpr int VM_WAVES = 8;
constexpr int VM_THREADS = VM_WAVES * 64;
constexpr int VM_LDS_BUDGET = 64 * 1024 - 64;   // the default LDS limit less the kernel's static word: the kernel never asks for more

struct ValArgs {
    const float* boxes;
    const float* scores;
    const int64_t* labels;
    const int* counts;
    const float* gt_boxes;
    const int* gt_labels;
    const int* gt_counts;
    int* match;
    float* iou;
    uint8_t* tp;
    int* matrix;
    int* status;
    int N, K, G, T, C, class_aware, all_fp;
    float conf;
    float thr[YMI_VAL_MAX_THRS];
};

// byte offsets of the kernel's LDS arrays for slabs of K detections and G ground truths per image and C classes
struct ValLds {
    int gb, gkey, diou, dgt, dlab, gl, mat, total;
    bool lds_mat;
};
__host__ __device__ inline ValLds val_lds(int K, int G, int C, bool want_matrix) {
    ValLds L;
    auto up = [](int v) { return (v + 15) & ~15; };
    int off = 0;
    L.gb = off; off += G * 16;          // f32x4[G] ground-truth boxes
    L.gkey = off; off += G * 8;         // uint64[G] pass 2: IoU bits << 32 | ~slot of the best detection that chose this ground truth, 0 = none
    L.diou = off; off += up(K * 4);     // float[K] pass 1: the detection's best admissible IoU
    L.dgt = off; off += up(K * 2);      // int16[K]         its ground truth, -1 = none
    L.dlab = off; off += up(K * 2);     // int16[K]         its label, -1 = takes no part
    L.gl = off; off += up(G * 2);       // int16[G] classes, -1 = skipped
    L.mat = off;
    const int cells = (C + 1) * (C + 1);
    L.lds_mat = want_matrix && off + cells * 4 <= VM_LDS_BUDGET;
    if (L.lds_mat) off += cells * 4;    // int[(C + 1)^2] the image's additions
    L.total = off;
    return L;
}

__device__ __forceinline__ float val_area(const f32x4 b) { return __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1])); }

// the suppression's expression (postprocess.hip iou_gt, torchvision box_iou): inter / ((area_a + area_b) - inter), no epsilon: 0 / 0 = NaN
__device__ __forceinline__ float val_iou(const f32x4 a, float aa, const f32x4 b) {
    const float xx1 = fmaxf(a[0], b[0]), yy1 = fmaxf(a[1], b[1]);
    const float xx2 = fminf(a[2], b[2]), yy2 = fminf(a[3], b[3]);
    const float w = fmaxf(0.f, __fsub_rn(xx2, xx1)), h = fmaxf(0.f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(w, h);
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(aa, val_area(b)), inter));
}

__global__ __launch_bounds__(VM_THREADS) void val_match_kernel(const ValArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t val_lds_raw[];
    __shared__ int s_any;   // the image has at least one match
    const int img = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const ValLds L = val_lds(a.K, a.G, a.C, a.matrix != nullptr);
    char* lds = reinterpret_cast<char*>(val_lds_raw);
    f32x4* gb = reinterpret_cast<f32x4*>(lds + L.gb);
    unsigned long long* gkey = reinterpret_cast<unsigned long long*>(lds + L.gkey);
    float* diou = reinterpret_cast<float*>(lds + L.diou);
    int16_t* dgt = reinterpret_cast<int16_t*>(lds + L.dgt);
    int16_t* dlab = reinterpret_cast<int16_t*>(lds + L.dlab);
    int16_t* gl = reinterpret_cast<int16_t*>(lds + L.gl);
    int* lm = reinterpret_cast<int*>(lds + L.mat);
    const int64_t drow = (int64_t)img * a.K, grow = (int64_t)img * a.G;
    const int C1 = a.C + 1;

    const int kd_raw = a.counts[img];
    if (kd_raw < 0) {   // a stale slab row: the image is skipped, its outputs defined (block-uniform, before any barrier)
        if (tid == 0) atomicOr(&a.status[1], YMI_VAL_STATUS_STALE_ROW);
        for (int j = tid; j < a.K; j += VM_THREADS) {
            a.match[drow + j] = -1;
            a.iou[drow + j] = 0.f;
            for (int t = 0; t < a.T; ++t) a.tp[(drow + j) * a.T + t] = 0;
        }
        return;
    }
    if (kd_raw > a.K && tid == 0) atomicOr(&a.status[1], YMI_VAL_STATUS_BAD_COUNT);
    const int kd = kd_raw < a.K ? kd_raw : a.K;
    const int gn_raw = a.gt_counts[img];
    const int gn = gn_raw < 0 ? 0 : (gn_raw < a.G ? gn_raw : a.G);

    // ---- stage the ground truth; clear the keys and the LDS matrix ----
    bool bad = false;
    for (int g = tid; g < gn; g += VM_THREADS) {
        gb[g] = *reinterpret_cast<const f32x4*>(a.gt_boxes + (grow + g) * 4);
        const int l = a.gt_labels[grow + g];
        const bool ok = l >= 0 && l < a.C;
        bad |= !ok;
        gl[g] = ok ? (int16_t)l : (int16_t)-1;
        gkey[g] = 0ull;
    }
    if (L.lds_mat)
        for (int c = tid; c < C1 * C1; c += VM_THREADS) lm[c] = 0;
    if (tid == 0) s_any = 0;
    __syncthreads();

    // ---- pass 1 (+ the atomic of pass 2): a group of W lanes per detection ----
    const int W = gn > 32 ? 64 : (gn > 16 ? 32 : (gn > 8 ? 16 : 8));
    const int wshift = __ffs(W) - 1, per = 64 >> wshift;
    const float thr0 = a.thr[0];
    for (int j0 = wave * per; j0 < kd; j0 += VM_WAVES * per) {   // wave-uniform trip count: the butterfly below runs with every lane
        const int j = j0 + (lane >> wshift), sl = lane & (W - 1);
        const bool live = j < kd;
        int lab = -1;
        f32x4 bd = {0.f, 0.f, 0.f, 0.f};
        float ad = 0.f;
        if (live) {
            const float s = a.scores[drow + j];
            const int64_t l = a.labels[drow + j];
            const bool ok = l >= 0 && l < a.C;
            bad |= !ok;
            if (ok && s > a.conf) {   // strict; NaN never passes
                lab = (int)l;
                bd = *reinterpret_cast<const f32x4*>(a.boxes + (drow + j) * 4);
                ad = val_area(bd);
            }
        }
        unsigned long long best = 0ull;
        if (lab >= 0) {
            for (int g = sl; g < gn; g += W) {
                const int c = gl[g];
                float iou = val_iou(bd, ad, gb[g]);
                const bool adm = c >= 0 && (a.class_aware ? (iou >= thr0 && c == lab) : (iou > thr0));
                if (adm) {
                    if (iou == 0.f) iou = 0.f;   // 0 / negative union is -0: a zero IoU is +0, so that admissible IoUs order as their bits do
                    const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned long long)(0xffffffffu - (unsigned)g);
                    best = key > best ? key : best;
                }
            }
        }
        for (int o = W >> 1; o >= 1; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other > best ? other : best;
        }
        if (live && sl == 0) {
            dlab[j] = (int16_t)lab;
            if (best != 0ull) {
                const int g = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
                dgt[j] = (int16_t)g;
                diou[j] = __uint_as_float((unsigned)(best >> 32));
                atomicMax(&gkey[g], (best & 0xffffffff00000000ull) | (unsigned long long)(0xffffffffu - (unsigned)j));
            } else {
                dgt[j] = (int16_t)-1;
                diou[j] = 0.f;
            }
        }
    }
    if (bad) atomicOr(&a.status[1], YMI_VAL_STATUS_BAD_LABEL);
    __syncthreads();

    // ---- the matrix's ground-truth column entries: matched -> [label(d), c], unmatched -> [nc, c] ----
    if (a.matrix != nullptr) {
        for (int g = tid; g < gn; g += VM_THREADS) {
            const int c = gl[g];
            if (c < 0) continue;
            const unsigned long long key = gkey[g];
            int cell = a.C * C1 + c;
            if (key != 0ull) {
                const int j = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
                cell = (int)dlab[j] * C1 + c;
                s_any = 1;   // every writer stores the same value
            }
            if (L.lds_mat) atomicAdd(&lm[cell], 1); else atomicAdd(&a.matrix[cell], 1);
        }
    }
    __syncthreads();

    // ---- a thread per slot: the outputs, and the matrix's unmatched candidates -> [label(d), nc] ----
    const bool count_fp = a.matrix != nullptr && (s_any != 0 || a.all_fp != 0);
    for (int j = tid; j < a.K; j += VM_THREADS) {
        int m = -1;
        float io = 0.f;
        if (j < kd) {
            const int lab = dlab[j], g = dgt[j];
            if (lab >= 0 && g >= 0 && (unsigned)(gkey[g] & 0xffffffffull) == 0xffffffffu - (unsigned)j) {
                m = g;
                io = diou[j];
            } else if (lab >= 0 && count_fp) {
                const int cell = lab * C1 + a.C;
                if (L.lds_mat) atomicAdd(&lm[cell], 1); else atomicAdd(&a.matrix[cell], 1);
            }
        }
        a.match[drow + j] = m;
        a.iou[drow + j] = io;
        for (int t = 0; t < a.T; ++t) a.tp[(drow + j) * a.T + t] = (m >= 0 && io >= a.thr[t]) ? 1 : 0;
    }

    // ---- flush the non-zero cells of the LDS matrix ----
    if (L.lds_mat) {
        __syncthreads();
        for (int c = tid; c < C1 * C1; c += VM_THREADS) {
            const int v = lm[c];
            if (v != 0) atomicAdd(&a.matrix[c], v);
        }
    }
}

static int val_match_launch(const ymi_val_desc* d, hipStream_t s) {
    YMI_REQUIRE(d != nullptr, "ymi_val_match: null descriptor");
    YMI_REQUIRE(d->n >= 0 && d->k >= 0 && d->k <= YMI_VAL_MAX_PER_IMAGE && d->g >= 0 && d->g <= YMI_VAL_MAX_PER_IMAGE,
                "ymi_val_match: n=%d k=%d g=%d out of range (k, g <= %d per image)", d->n, d->k, d->g, YMI_VAL_MAX_PER_IMAGE);
    YMI_REQUIRE(d->num_thrs >= 1 && d->num_thrs <= YMI_VAL_MAX_THRS, "ymi_val_match: %d thresholds (1 .. %d)", d->num_thrs, YMI_VAL_MAX_THRS);
    YMI_REQUIRE(d->num_classes >= 1 && d->num_classes <= 4096, "ymi_val_match: num_classes=%d (1 .. 4096)", d->num_classes);
    YMI_REQUIRE((d->flags & ~YMI_VAL_COUNT_ALL_FP) == 0, "ymi_val_match: unknown flags 0x%x", d->flags);
    YMI_REQUIRE(d->conf == d->conf, "ymi_val_match: conf is NaN");
    ValArgs a;
    for (int t = 0; t < YMI_VAL_MAX_THRS; ++t) a.thr[t] = INFINITY;
    for (int t = 0; t < d->num_thrs; ++t) {
        YMI_REQUIRE(d->thrs[t] >= 0.f && d->thrs[t] <= 1.f, "ymi_val_match: threshold %d = %g outside [0, 1]", t, (double)d->thrs[t]);
        a.thr[t] = d->thrs[t];
    }
    if (d->n == 0) return YMI_OK;
    YMI_REQUIRE(d->counts && d->gt_counts && d->status, "ymi_val_match: null buffer");
    YMI_REQUIRE(d->k == 0 || (d->boxes && d->scores && d->labels && d->match && d->iou && d->tp), "ymi_val_match: null detection or output buffer");
    YMI_REQUIRE(d->g == 0 || (d->gt_boxes && d->gt_labels), "ymi_val_match: null ground-truth buffer");
    YMI_REQUIRE(((uintptr_t)d->boxes & 15) == 0 && ((uintptr_t)d->gt_boxes & 15) == 0, "ymi_val_match: boxes and gt_boxes must be 16-byte aligned");
    a.boxes = d->boxes; a.scores = d->scores; a.labels = d->labels; a.counts = d->counts;
    a.gt_boxes = d->gt_boxes; a.gt_labels = d->gt_labels; a.gt_counts = d->gt_counts;
    a.match = d->match; a.iou = d->iou; a.tp = d->tp; a.matrix = d->matrix; a.status = d->status;
    a.N = d->n; a.K = d->k; a.G = d->g; a.T = d->num_thrs; a.C = d->num_classes;
    a.class_aware = d->class_aware != 0; a.all_fp = (d->flags & YMI_VAL_COUNT_ALL_FP) != 0;
    a.conf = d->conf;
    const size_t lds = (size_t)val_lds(d->k, d->g, d->num_classes, d->matrix != nullptr).total;
    hipLaunchKernelGGL(val_match_kernel, dim3(d->n), dim3(VM_THREADS), lds, s, a);
    return check_launch("val_match_kernel");
}

}  // namespace ymi

extern "C" int ymi_val_match(const ymi_val_desc* d, void* stream) { return ymi::val_match_launch(d, (hipStream_t)stream); }
