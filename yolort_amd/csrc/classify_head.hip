// Second-stage classification (ymi_classify_head, ymi_second_stage_filter; contracts in include/yolort_amd.h).
//
// pool_fc_kernel: logits / hidden = epilogue(A x W^T + bias) for an A of n rows (one row per crop or image) that is either reduced out of up to four NHWC maps
// (global average pool, the maps' channel ranges side by side along K) or copied from a contiguous (n, K) matrix.  M is 1 .. a few thousand, so the tile is the
// opposite of the conv kernels': a workgroup of 8 waves owns BM = 32 rows and keeps the WHOLE A block (32 x K 16-bit values, 80 KiB at K = 1280) in LDS for the
// whole K; every wave owns 32-column slices of N and streams their weights global -> registers (a lane's fragment of the (N_pad, K) K-contiguous weights is one
// 16-byte load), a K step of 64 ahead of the MFMAs.  Nothing of W is shared between waves, so it never enters LDS.  grid = (ceil(n / 32), n_split): with few rows
// the N slices are spread over n_split workgroups (each re-pools its block: cheap exactly then), with many rows n_split is 1 and a map is pooled once.
// MFMA form: the project's swapped 32x32x16 (D[column of N][row of A]): the weights are the A operand, the LDS block the B operand; lane l owns row (l & 31) of the
// block and accumulator register g*4+e holds column g*8 + 4*(l>>5) + e of the slice.
//
// second_stage_filter_kernel: the last line of apply_classifier on the detection slab -- a workgroup per image, a wave per detection (arg-max of its logits row by
// a wave reduction), kept rows compacted in slab order by ballot + prefix.
#include <limits.h>
#include <stdlib.h>

#include "conv_common.hpp"

namespace ymi {

constexpr int CH_BM = 32;        // rows of A per workgroup = the M of the MFMA
constexpr int CH_WAVES = 8;
constexpr int CH_THREADS = CH_WAVES * 64;
constexpr int CH_KSTEP = 64;     // K elements per main-loop step: four MFMAs, four 16-byte weight loads per lane in flight ahead of them
constexpr int CH_LDS_PAD = 8;    // halfs added to a row of the A block: a row stride of 16 bytes mod 128, as LDS_PITCH does for the conv tiles
constexpr int CH_LDS_MAX = 160 * 1024;
enum { CH_SRC_POOL = 0, CH_SRC_ROWS = 1 };
enum { CH_EPI_HIDDEN = 0, CH_EPI_LOGITS = 1 };

struct PoolFcArgs {
    const uint16_t* map[YMI_CLASSIFY_MAX_MAPS];   // CH_SRC_POOL: NHWC views (n, hw[i], c[i]) with pixel stride cs[i]
    int hw[YMI_CLASSIFY_MAX_MAPS], c[YMI_CLASSIFY_MAX_MAPS], cs[YMI_CLASSIFY_MAX_MAPS], koff[YMI_CLASSIFY_MAX_MAPS];   // koff: first k of map i
    float inv[YMI_CLASSIFY_MAX_MAPS];             // 1 / hw[i], rounded to fp32 on the host
    int nmaps;
    const uint16_t* rows;   // CH_SRC_ROWS: contiguous (n, K)
    const uint16_t* w;      // (nslices * 32, K) K-contiguous, rows >= N zero
    const float* bias;      // (nslices * 32), entries >= N zero
    void* out;              // (n, N): 16-bit (hidden) or fp32 (logits)
    int n, K, Kpad, N, nslices, pitch;
};

__device__ __forceinline__ float hardswish(float x) { return x * fminf(fmaxf(x + 3.0f, 0.0f), 6.0f) / 6.0f; }

template <int DT>
__device__ __forceinline__ void add8(float (&acc)[8], const u32x4& t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        acc[2 * e] += from16<DT>((uint16_t)(t[e] & 0xffffu));
        acc[2 * e + 1] += from16<DT>((uint16_t)(t[e] >> 16));
    }
}

template <int DT, int SRC, int EPI>
__global__ __launch_bounds__(CH_THREADS) void pool_fc_kernel(const PoolFcArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t ch_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * CH_BM;

    // ---- the A block: CH_BM rows x Kpad values; rows >= n and k >= K are zero ----
    const int chunks = a.Kpad >> 3;
    for (int item = tid; item < CH_BM * chunks; item += CH_THREADS) {
        const int r = item / chunks, k = (item - r * chunks) * 8;   // adjacent lanes: adjacent 16-byte chunks of one row
        const int row = row0 + r;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < a.n && k < a.K) {
            if constexpr (SRC == CH_SRC_ROWS) {
                v = *reinterpret_cast<const u32x4*>(a.rows + (int64_t)row * a.K + k);
            } else {
                const uint16_t* p = a.map[0];
                int hw = a.hw[0], cs = a.cs[0], k0 = 0;
                float inv = a.inv[0];
#pragma unroll
                for (int m = 1; m < YMI_CLASSIFY_MAX_MAPS; ++m)   // (constant indices: the arguments stay in scalar registers)
                    if (m < a.nmaps && k >= a.koff[m]) { p = a.map[m]; hw = a.hw[m]; cs = a.cs[m]; k0 = a.koff[m]; inv = a.inv[m]; }
                const uint16_t* src = p + (int64_t)row * hw * cs + (k - k0);
                float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int q = 0; q < hw; ++q) add8<DT>(acc, *reinterpret_cast<const u32x4*>(src + (int64_t)q * cs));   // pixels in order, fp32
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = cvt_pk16<DT>(f32x2{acc[2 * e] * inv, acc[2 * e + 1] * inv});     // the one rounding of a pooled value
            }
        }
        *reinterpret_cast<u32x4*>(ch_lds + r * a.pitch + k) = v;
    }
    __syncthreads();

    // ---- the wave's slices of N ----
    typedef typename Mfma<DT>::frag frag;
    const int hi = lane >> 5, l31 = lane & 31;
    const uint16_t* arow = ch_lds + l31 * a.pitch + hi * 8;
    const int row = row0 + l31;
    for (int s = blockIdx.y + gridDim.y * wave; s < a.nslices; s += gridDim.y * CH_WAVES) {
        const uint16_t* wrow = a.w + (int64_t)(s * 32 + l31) * a.K + hi * 8;
        f32x4 b[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const f32x4*>(a.bias + s * 32 + g * 8 + hi * 4);
        u32x4 cur[4], nxt[4];
        auto fetch = [&](u32x4 (&f)[4], int k0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                f[c] = z;
                if (k0 + c * 16 + hi * 8 < a.K) f[c] = *reinterpret_cast<const u32x4*>(wrow + k0 + c * 16);   // K tail: nothing past a weight row is read
            }
        };
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        fetch(cur, 0);
        for (int k0 = 0; k0 < a.Kpad; k0 += CH_KSTEP) {
            if (k0 + CH_KSTEP < a.Kpad) fetch(nxt, k0 + CH_KSTEP);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const u32x4 af = *reinterpret_cast<const u32x4*>(arow + k0 + c * 16);
                acc = Mfma<DT>::run(__builtin_bit_cast(frag, cur[c]), __builtin_bit_cast(frag, af), acc);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) cur[c] = nxt[c];
        }
        if (row >= a.n) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = s * 32 + g * 8 + hi * 4;
            if (col >= a.N) continue;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = acc[g * 4 + e] + b[g][e];
                if constexpr (EPI == CH_EPI_HIDDEN) v[e] = hardswish(v[e]);
            }
            const int64_t o = (int64_t)row * a.N + col;
            if constexpr (EPI == CH_EPI_HIDDEN) {
                uint16_t* yp = reinterpret_cast<uint16_t*>(a.out) + o;
                if ((a.N & 3) == 0) {   // col + 3 < N and an 8-byte aligned address
                    const u32x2 pk = {cvt_pk16<DT>(f32x2{v[0], v[1]}), cvt_pk16<DT>(f32x2{v[2], v[3]})};
                    *reinterpret_cast<u32x2*>(yp) = pk;
                } else {
                    for (int e = 0; e < 4 && col + e < a.N; ++e) yp[e] = to16<DT>(v[e]);
                }
            } else {
                float* yp = reinterpret_cast<float*>(a.out) + o;
                if ((a.N & 3) == 0) {
                    const f32x4 pk = {v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(yp) = pk;
                } else {
                    for (int e = 0; e < 4 && col + e < a.N; ++e) yp[e] = v[e];
                }
            }
        }
    }
}

// the grid's second axis.  Few rows: the slices of N are spread so that the grid covers the CUs (a handful of crops would otherwise stream every weight through
// one CU); every split re-pools its block, which is cheap exactly then.  Many rows: 1, a map is pooled once.  YOLORT_AMD_CLASSIFY_NSPLIT=<k> overrides (A/B runs).
static int choose_n_split(int nblk, int nslices, int requested) {
    if (requested <= 0) {
        if (const char* e = getenv("YOLORT_AMD_CLASSIFY_NSPLIT")) requested = atoi(e);
    }
    int v = requested;
    if (v <= 0) {
        static int cus = 0;
        if (cus == 0) {
            int dev = 0, c = 0;
            if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0) cus = c;
            else cus = 256;
        }
        v = cus / nblk;
    }
    return v < 1 ? 1 : (v > nslices ? nslices : v);
}

template <int DT, int SRC, int EPI>
static int pool_fc_launch(const PoolFcArgs& a, int n_split, hipStream_t s) {
    auto kfn = pool_fc_kernel<DT, SRC, EPI>;
    const size_t lds = (size_t)CH_BM * a.pitch * sizeof(uint16_t);
    if (lds > 64 * 1024) { const int rc_lds = allow_big_lds((const void*)kfn, (int)lds); if (rc_lds != YMI_OK) return rc_lds; }
    const int nblk = cdiv(a.n, CH_BM);
    const dim3 grid(nblk, choose_n_split(nblk, a.nslices, n_split));
    hipLaunchKernelGGL(kfn, grid, dim3(CH_THREADS), lds, s, a);
    return check_launch("pool_fc_kernel");
}

template <int DT>
static int classify_launch(const ymi_classify_desc* d, PoolFcArgs a, hipStream_t s) {
    const bool two = d->mode == YMI_CLASSIFY_HIDDEN_LOGITS;
    a.w = (const uint16_t*)d->w1; a.bias = d->b1; a.N = d->n1; a.nslices = cdiv(d->n1, 32);
    if (!two) {
        a.out = d->logits;
        return pool_fc_launch<DT, CH_SRC_POOL, CH_EPI_LOGITS>(a, d->n_split, s);
    }
    a.out = d->hidden;
    const int rc = pool_fc_launch<DT, CH_SRC_POOL, CH_EPI_HIDDEN>(a, d->n_split, s);
    if (rc != YMI_OK) return rc;
    PoolFcArgs r = {};
    r.rows = (const uint16_t*)d->hidden; r.n = d->n; r.K = d->n1; r.Kpad = cdiv(d->n1, CH_KSTEP) * CH_KSTEP; r.pitch = r.Kpad + CH_LDS_PAD;
    r.w = (const uint16_t*)d->w2; r.bias = d->b2; r.N = d->n2; r.nslices = cdiv(d->n2, 32); r.out = d->logits;
    return pool_fc_launch<DT, CH_SRC_ROWS, CH_EPI_LOGITS>(r, d->n_split, s);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------
// second_stage_filter_kernel
// ---------------------------------------------------------------------------------------------------
constexpr int SF_WAVES = 8;
constexpr int SF_THREADS = SF_WAVES * 64;

// torch.argmax's order on the CPU: a NaN beats every number, equal values (and two NaNs) go to the lower index
__device__ __forceinline__ bool argmax_before(float a, int ia, float b, int ib) {
    if (a != a) return (b != b) ? ia < ib : true;
    if (b != b) return false;
    return a == b ? ia < ib : a > b;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(SF_THREADS) void second_stage_filter_kernel(const ymi_filter_desc a) {
    extern __shared__ unsigned char sf_keep[];   // k flags
    __shared__ int red[3][SF_WAVES];
    __shared__ int kept_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = blockIdx.x;
    // the image's first row = the exclusive prefix of the clamped counts (the crop kernel's rule), the sum of all of them, and whether any count is out of range
    int before = 0, sum = 0, bad = 0;
    for (int j = tid; j < a.n; j += SF_THREADS) {
        const int c = a.counts[j];
        bad |= (c < 0 || c > a.k) ? 1 : 0;
        const int cc = c < 0 ? 0 : (c > a.k ? a.k : c);
        sum += cc;
        if (j < i) before += cc;
    }
    before = wave_sum(before); sum = wave_sum(sum); bad = wave_sum(bad);
    if (lane == 0) { red[0][wave] = before; red[1][wave] = sum; red[2][wave] = bad; }
    __syncthreads();
    before = sum = bad = 0;
#pragma unroll
    for (int w = 0; w < SF_WAVES; ++w) { before += red[0][w]; sum += red[1][w]; bad += red[2][w]; }
    const int written = a.total[0];
    const int limit = written < 0 ? 0 : (written > a.cap ? a.cap : written);   // logits rows that hold a crop's result
    if (i == 0 && tid == 0)
        a.status[0] = (bad ? YMI_FILTER_STATUS_BAD_COUNT : 0) | (written != (sum < a.cap ? sum : a.cap) ? YMI_FILTER_STATUS_TOTAL : 0) | (sum > a.cap ? YMI_FILTER_STATUS_CAPACITY : 0);
    if (i >= a.n) return;   // (n == 0: one workgroup writes the status word)
    int cnt = a.counts[i];
    cnt = cnt < 0 ? 0 : (cnt > a.k ? a.k : cnt);
    const int64_t slab0 = (int64_t)i * a.k;

    for (int j = wave; j < cnt; j += SF_WAVES) {   // a wave per detection
        const int row = before + j;
        int cls = -1;
        bool keep = false;
        if (row < limit) {   // wave-uniform
            const float* lg = a.logits + (int64_t)row * a.nc2;
            float best = -INFINITY;
            int bi = INT_MAX;
            for (int c = lane; c < a.nc2; c += 64) {
                const float v = lg[c];
                if (argmax_before(v, c, best, bi)) { best = v; bi = c; }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float ov = __shfl_xor(best, d);
                const int oi = __shfl_xor(bi, d);
                if (argmax_before(ov, oi, best, bi)) { best = ov; bi = oi; }
            }
            cls = bi;
            const int64_t mapped = a.class_map ? (int64_t)a.class_map[cls] : (int64_t)cls;
            keep = mapped == a.labels[slab0 + j];
        }
        if (lane == 0) { a.cls2[slab0 + j] = cls; sf_keep[j] = keep ? 1 : 0; }
    }
    for (int j = cnt + tid; j < a.k; j += SF_THREADS) a.cls2[slab0 + j] = -1;
    __syncthreads();

    if (wave == 0) {   // kept rows in slab order: ballot + prefix, 64 detections a step
        int running = 0;
        for (int base = 0; base < cnt; base += 64) {
            const int j = base + lane;
            const bool f = j < cnt && sf_keep[j] != 0;
            const unsigned long long mask = __ballot(f);
            if (f) {
                const int64_t src = slab0 + j, dst = slab0 + running + __popcll(mask & ((1ull << lane) - 1ull));
                *reinterpret_cast<f32x4*>(a.out_boxes + dst * 4) = *reinterpret_cast<const f32x4*>(a.boxes + src * 4);
                a.out_scores[dst] = a.scores[src];
                a.out_labels[dst] = a.labels[src];
            }
            running += __popcll(mask);
        }
        if (lane == 0) { a.out_counts[i] = running; kept_total = running; }
    }
    __syncthreads();
    for (int j = kept_total + tid; j < a.k; j += SF_THREADS) {   // the slots past the new count are zero
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(a.out_boxes + (slab0 + j) * 4) = z;
        a.out_scores[slab0 + j] = 0.f;
        a.out_labels[slab0 + j] = 0;
    }
}

}  // namespace ymi

using namespace ymi;

extern "C" int ymi_classify_head(const ymi_classify_desc* d, void* stream) {
    YMI_REQUIRE(d != nullptr, "ymi_classify_head: null descriptor");
    YMI_REQUIRE(d->dtype == YMI_F16 || d->dtype == YMI_BF16, "ymi_classify_head: dtype %d (the head computes in YMI_F16 or YMI_BF16; the fp32 parity mode has no head)", d->dtype);
    YMI_REQUIRE(d->mode == YMI_CLASSIFY_LOGITS || d->mode == YMI_CLASSIFY_HIDDEN_LOGITS, "ymi_classify_head: bad mode %d", d->mode);
    YMI_REQUIRE(d->num_maps >= 1 && d->num_maps <= YMI_CLASSIFY_MAX_MAPS, "ymi_classify_head: %d maps (1 .. %d)", d->num_maps, YMI_CLASSIFY_MAX_MAPS);
    YMI_REQUIRE(d->n >= 0 && d->n <= (INT_MAX / CH_BM), "ymi_classify_head: n = %d out of range", d->n);
    const bool two = d->mode == YMI_CLASSIFY_HIDDEN_LOGITS;
    YMI_REQUIRE(d->n1 >= 1 && (!two || d->n2 >= 1), "ymi_classify_head: output widths n1 = %d, n2 = %d below 1", d->n1, d->n2);
    YMI_REQUIRE(d->w1 && d->b1 && d->logits && (!two || (d->w2 && d->b2 && d->hidden)), "ymi_classify_head: null buffer (weights, biases, hidden or logits)");
    YMI_REQUIRE(aligned16(d->w1) && aligned16(d->b1) && (!two || (aligned16(d->w2) && aligned16(d->b2) && aligned16(d->hidden))) && aligned16(d->logits),
                "ymi_classify_head: weights, biases, hidden and logits must be 16-byte aligned");
    YMI_REQUIRE(!two || d->n1 % 8 == 0, "ymi_classify_head: the hidden width %d is not a multiple of 8", d->n1);
    PoolFcArgs a = {};
    int K = 0;
    for (int m = 0; m < d->num_maps; ++m) {
        YMI_REQUIRE(d->maps[m] != nullptr && aligned16(d->maps[m]), "ymi_classify_head: map %d is null or not 16-byte aligned", m);
        YMI_REQUIRE(d->c[m] >= 8 && d->c[m] % 8 == 0 && d->cs[m] >= d->c[m] && d->cs[m] % 8 == 0, "ymi_classify_head: map %d has c = %d, channel stride %d (multiples of 8, stride >= c)", m, d->c[m], d->cs[m]);
        YMI_REQUIRE(d->hw[m] >= 1 && (int64_t)d->hw[m] * d->cs[m] < ((int64_t)1 << 31), "ymi_classify_head: map %d has %d pixels (>= 1, pixels x stride below 2^31)", m, d->hw[m]);
        a.map[m] = (const uint16_t*)d->maps[m]; a.hw[m] = d->hw[m]; a.c[m] = d->c[m]; a.cs[m] = d->cs[m]; a.koff[m] = K;
        a.inv[m] = 1.0f / (float)d->hw[m];
        K += d->c[m];
        YMI_REQUIRE(K <= YMI_CLASSIFY_MAX_K, "ymi_classify_head: %d or more channels in all (a workgroup keeps 32 rows of them in LDS: at most %d)", K, YMI_CLASSIFY_MAX_K);
    }
    YMI_REQUIRE(!two || d->n1 <= YMI_CLASSIFY_MAX_K, "ymi_classify_head: hidden width %d above %d", d->n1, YMI_CLASSIFY_MAX_K);
    a.nmaps = d->num_maps; a.n = d->n; a.K = K; a.Kpad = cdiv(K, CH_KSTEP) * CH_KSTEP; a.pitch = a.Kpad + CH_LDS_PAD;
    static_assert((size_t)CH_BM * (((YMI_CLASSIFY_MAX_K + CH_KSTEP - 1) / CH_KSTEP) * CH_KSTEP + CH_LDS_PAD) * 2 <= CH_LDS_MAX, "the A block of the widest head fits the LDS");
    if (d->n == 0) return YMI_OK;
    return d->dtype == YMI_F16 ? classify_launch<YMI_F16>(d, a, (hipStream_t)stream) : classify_launch<YMI_BF16>(d, a, (hipStream_t)stream);
}

extern "C" int ymi_second_stage_filter(const ymi_filter_desc* d, void* stream) {
    YMI_REQUIRE(d != nullptr, "ymi_second_stage_filter: null descriptor");
    YMI_REQUIRE(d->n >= 0 && d->k >= 0 && d->cap >= 0, "ymi_second_stage_filter: negative n %d, k %d or capacity %d", d->n, d->k, d->cap);
    YMI_REQUIRE(d->k <= YMI_FILTER_MAX_K, "ymi_second_stage_filter: slab depth %d above %d", d->k, YMI_FILTER_MAX_K);
    YMI_REQUIRE(d->nc2 >= 1, "ymi_second_stage_filter: %d second-stage classes", d->nc2);
    YMI_REQUIRE(d->total && d->status && (d->cap == 0 || d->logits), "ymi_second_stage_filter: null buffer (logits, total or status)");
    YMI_REQUIRE(d->n == 0 || (d->counts && d->out_counts), "ymi_second_stage_filter: null counts");
    YMI_REQUIRE(d->n == 0 || d->k == 0 || (d->boxes && d->scores && d->labels && d->out_boxes && d->out_scores && d->out_labels && d->cls2), "ymi_second_stage_filter: null slab buffer");
    YMI_REQUIRE(d->n == 0 || d->k == 0 || (aligned16(d->boxes) && aligned16(d->out_boxes)), "ymi_second_stage_filter: boxes must be 16-byte aligned");
    YMI_REQUIRE(d->n == 0 || d->k == 0 || (d->out_boxes != d->boxes && d->out_scores != d->scores && d->out_labels != d->labels), "ymi_second_stage_filter: the output slab must not be the input slab");
    YMI_REQUIRE((int64_t)d->n * d->k < ((int64_t)1 << 31), "ymi_second_stage_filter: n * k does not fit 31 bits");
    hipLaunchKernelGGL(second_stage_filter_kernel, dim3(d->n > 0 ? d->n : 1), dim3(SF_THREADS), (size_t)((d->k + 15) & ~15), (hipStream_t)stream, *d);
    return check_launch("second_stage_filter_kernel");
}
