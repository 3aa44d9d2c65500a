// Multi-head self-attention over the pixels of an NHWC map (ymi_attention; contract in include/yolort_amd.h):
//     O[n, i, h*d:(h+1)*d] = softmax_j(scale * Q[n, i, h] . K[n, j, h]) @ V[n, j, h],   i, j in [0, S), d in {32, 64, 128}, fp16 / bf16.
//
// attention_kernel<DT, D>: ONE launch, no S x S matrix in memory.  A workgroup of AT_WAVES = 2 waves owns one (image, head, tile of AT_TQ = 64 queries); a wave owns
// 32 queries.  grid = n * heads * ceil(S / 64) workgroups, the query tiles of one (image, head) adjacent: the tile axis is what fills the CUs when n * heads is small
// (32 images x 4 heads x 400 pixels = 896 workgroups of 2 waves), and K / V of a head (S * d * 4 bytes) stay in L2 for its tiles.
//
// Both products run TRANSPOSED on the 32x32x16 MFMA, so that the soft-max weights leave the first product in the register layout the second one reads:
//   S^T[key][query] = K Q^T :  A = a K row (lane l: key l & 31, 8 values of d at 16 s + 8 (l >> 5)), B = the Q fragment of query l & 31 -- d / 16 fragments loaded
//                              from global ONCE with 16-byte loads and held in registers for the whole key loop.  Lane l then holds, for ITS query l & 31, the scores
//                              of keys 8 g + 4 (l >> 5) + e in accumulator register 4 g + e: a row of the soft-max lives in two lanes (l, l ^ 32).
//   O^T[dcol][query] = V^T P^T: B = P^T, which needs 8 keys of query l & 31 per lane and K step: accumulator registers 8 t .. 8 t + 7, rounded to the storage type in
//                              registers (cvt_pk16), ARE that fragment if the K axis of step t is taken in the order key(j) = 8 (2 t + j / 4) + 4 (l >> 5) + j % 4.
//                              A = V^T in the same order: two 8-byte LDS reads of 4 consecutive keys each.
// LDS, one buffer per operand, chosen for the two read patterns:
//   K chunk  [AT_TK = 64 keys][d + 8]   read along d: a lane's fragment is one 16-byte read, the row pitch is 16 bytes mod 128 (the conv tiles' LDS_PITCH rule)
//   V chunk  [d][64 + 4]  TRANSPOSED    read along keys.  A thread loads the same 8 channels of two adjacent keys (two 16-byte global loads) and writes eight 32-bit
//                                       key pairs; lanes run along key pairs, so the writes of a half-wave fall into 32 consecutive words
// Pipeline: the 16-byte global loads of chunk c + 1 are issued into registers right after chunk c has been written to LDS and stay in flight while chunk c is
// multiplied; barrier, store, barrier.  Rows of keys >= S are ZERO in both chunks.
// Soft-max: running maximum / running sum per query (S is not bounded by LDS), everything in fp32: t = scale * s;  keys >= S take NO part in the maximum and get the
// weight 0.0f itself (not exp of a large negative number);  m' = max(m, max_j t);  p = exp(t - m');  O and the row sum are multiplied by exp(m - m') (exactly 0 on the
// first chunk).  THE ROW SUM IS TAKEN FROM THE UNROUNDED fp32 WEIGHTS; the weights are rounded to the storage type only as the MFMA operand.  The two lanes of a query
// keep partial sums over their own keys and add them once at the end; then one fp32 division per output and ONE rounding.  Queries >= S compute on zeros and are not
// stored.  No atomics, no host synchronisation, no scratch: capturable.
#include <math.h>

#include "conv_common.hpp"

namespace ymi {

constexpr int AT_TQ = YMI_ATTN_TILE_Q;   // queries per workgroup
constexpr int AT_TK = YMI_ATTN_TILE_K;   // keys per LDS chunk
constexpr int AT_WAVES = AT_TQ / 32;
constexpr int AT_THREADS = AT_WAVES * 64;
constexpr int AT_VPITCH = AT_TK + 4;     // halfs per row of the transposed V chunk: 8-byte aligned rows, 16 consecutive rows cover the 32 banks in 8-byte reads
static_assert(AT_TK == 64 && AT_THREADS == 128, "the chunk loaders below are written for 64 keys and 128 threads");

struct AttnArgs {
    const uint16_t *q, *k, *v;
    uint16_t* o;
    int S, heads, tiles, q_cs, k_cs, v_cs, o_cs;
    float scale;
};

template <int DT, int D>
__global__ __launch_bounds__(AT_THREADS) void attention_kernel(const AttnArgs a) {
    constexpr int KP = D + 8;            // K chunk row pitch (halfs)
    constexpr int NS = D / 16;           // K steps of Q K^T = Q fragments
    constexpr int NB = D / 32;           // 32-row blocks of O^T
    constexpr int KPK = D / 16;          // 16-byte packets of the K chunk per thread (64 * D / 8 / 128)
    constexpr int VIT = D / 32;          // (key pair, 8 channels) items of the V chunk per thread (32 * D / 8 / 128)
    typedef typename Mfma<DT>::frag frag;
    __shared__ __attribute__((aligned(16))) uint16_t k_lds[AT_TK * KP];
    __shared__ __attribute__((aligned(16))) uint16_t v_lds[D * AT_VPITCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int tile = blockIdx.x % a.tiles, rest = blockIdx.x / a.tiles, head = rest % a.heads, img = rest / a.heads;
    const int64_t row0 = (int64_t)img * a.S;   // first pixel of the image
    const uint16_t* qp = a.q + head * D;
    const uint16_t* kp = a.k + head * D;
    const uint16_t* vp = a.v + head * D;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    // ---- this lane's query: d / 16 fragments, in registers for the whole key loop ----
    const int qi = tile * AT_TQ + wave * 32 + l31;
    u32x4 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        qf[s] = zero;
        if (qi < a.S) qf[s] = *reinterpret_cast<const u32x4*>(qp + (row0 + qi) * a.q_cs + 16 * s + 8 * hi);
    }

    // ---- chunk loaders: global -> registers (16-byte loads, zeros for keys >= S), registers -> LDS ----
    u32x4 kreg[KPK], vreg[VIT][2];
    auto fetch = [&](int key0) {
#pragma unroll
        for (int i = 0; i < KPK; ++i) {
            const int p = tid + AT_THREADS * i, key = key0 + p / (D / 8), oct = p % (D / 8);   // adjacent lanes: adjacent packets of one key row
            kreg[i] = zero;
            if (key < a.S) kreg[i] = *reinterpret_cast<const u32x4*>(kp + (row0 + key) * a.k_cs + 8 * oct);
        }
#pragma unroll
        for (int i = 0; i < VIT; ++i) {
            const int it = tid + AT_THREADS * i, key = key0 + 2 * (it & 31), oct = it >> 5;           // adjacent lanes: adjacent key pairs of one channel octet
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                vreg[i][r] = zero;
                if (key + r < a.S) vreg[i][r] = *reinterpret_cast<const u32x4*>(vp + (row0 + key + r) * a.v_cs + 8 * oct);
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < KPK; ++i) {
            const int p = tid + AT_THREADS * i;
            *reinterpret_cast<u32x4*>(k_lds + (p / (D / 8)) * KP + 8 * (p % (D / 8))) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < VIT; ++i) {
            const int it = tid + AT_THREADS * i, pair = it & 31, oct = it >> 5;
            uint32_t* dst = reinterpret_cast<uint32_t*>(v_lds + (8 * oct) * AT_VPITCH + 2 * pair);
#pragma unroll
            for (int e = 0; e < 4; ++e) {   // channels 8 oct + 2 e, + 1 of keys (2 pair, 2 pair + 1) -> one word each
                const uint32_t lo = vreg[i][0][e], up = vreg[i][1][e];
                dst[(2 * e) * (AT_VPITCH / 2)] = (lo & 0xffffu) | (up << 16);
                dst[(2 * e + 1) * (AT_VPITCH / 2)] = (lo >> 16) | (up & 0xffff0000u);
            }
        }
    };

    f32x16 o[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
    float m = -INFINITY, lsum = 0.f;   // running maximum of the query (both lanes agree), running sum over THIS lane's keys

    fetch(0);
    for (int key0 = 0; key0 < a.S; key0 += AT_TK) {
        __syncthreads();   // every wave is done reading the previous chunk
        stash();
        __syncthreads();
        if (key0 + AT_TK < a.S) fetch(key0 + AT_TK);   // in flight while this chunk is multiplied

        // ---- S^T = K Q^T for the chunk's two 32-key blocks ----
        f32x16 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
            const uint16_t* krow = k_lds + (kb * 32 + l31) * KP + 8 * hi;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(krow + 16 * s);
                st[kb] = Mfma<DT>::run(__builtin_bit_cast(frag, kf), __builtin_bit_cast(frag, qf[s]), st[kb]);
            }
        }
        // ---- soft-max step: register 4 g + e of block kb is key key0 + 32 kb + 8 g + 4 hi + e of query l31 ----
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + 32 * kb + 8 * (r >> 2) + 4 * hi + (r & 3);
                const float t = st[kb][r] * a.scale;
                st[kb][r] = t;
                if (key < a.S) mx = fmaxf(mx, t);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));       // the other half of the row; every chunk holds a key < S, so mx is a score
        const float mn = fmaxf(m, mx);
        const float alpha = __expf(m - mn);       // first chunk: exp(-inf) = 0
        m = mn;
        float part = 0.f;
        uint32_t pk[2][8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int key = key0 + 32 * kb + 8 * (r >> 2) + 4 * hi + (r & 3);
                const float p0 = key < a.S ? __expf(st[kb][r] - mn) : 0.f;
                const float p1 = key + 1 < a.S ? __expf(st[kb][r + 1] - mn) : 0.f;
                part += p0;
                part += p1;
                pk[kb][r >> 1] = cvt_pk16<DT>(f32x2{p0, p1});   // the weights as the MFMA reads them: rounded to the storage type
            }
        lsum = lsum * alpha + part;
        // ---- O^T = O^T * alpha + V^T P^T ----
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
            const uint16_t* vrow = v_lds + (b * 32 + l31) * AT_VPITCH + 4 * hi;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const u32x2 v0 = *reinterpret_cast<const u32x2*>(vrow + 32 * kb + 16 * t);       // keys 8 (2 t) + 4 hi + 0 .. 3 of the block
                    const u32x2 v1 = *reinterpret_cast<const u32x2*>(vrow + 32 * kb + 16 * t + 8);   // keys 8 (2 t + 1) + 4 hi + 0 .. 3
                    const u32x4 vf = {v0[0], v0[1], v1[0], v1[1]};
                    const u32x4 pf = {pk[kb][4 * t], pk[kb][4 * t + 1], pk[kb][4 * t + 2], pk[kb][4 * t + 3]};
                    o[b] = Mfma<DT>::run(__builtin_bit_cast(frag, vf), __builtin_bit_cast(frag, pf), o[b]);
                }
        }
    }

    // ---- epilogue: one division, one rounding; register 4 g + e of block b is channel 32 b + 8 g + 4 hi + e of query l31 ----
    lsum += __shfl_xor(lsum, 32);
    if (qi >= a.S) return;
    uint16_t* op = a.o + (row0 + qi) * a.o_cs + head * D + 4 * hi;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2 w = {cvt_pk16<DT>(f32x2{o[b][4 * g] / lsum, o[b][4 * g + 1] / lsum}), cvt_pk16<DT>(f32x2{o[b][4 * g + 2] / lsum, o[b][4 * g + 3] / lsum})};
            *reinterpret_cast<u32x2*>(op + 32 * b + 8 * g) = w;
        }
}

template <int DT, int D>
static int attention_launch_one(const AttnArgs& a, int n, hipStream_t s) {
    hipLaunchKernelGGL((attention_kernel<DT, D>), dim3((unsigned)(n * a.heads * a.tiles)), dim3(AT_THREADS), 0, s, a);
    return check_launch("attention_kernel");
}

int attention_check(const ymi_attn_desc* d) {
    YMI_REQUIRE(d != nullptr, "ymi_attention: null descriptor");
    YMI_REQUIRE(d->q && d->k && d->v && d->o, "ymi_attention: null q / k / v / o");
    YMI_REQUIRE(d->dtype == YMI_F16 || d->dtype == YMI_BF16, "ymi_attention: dtype must be F16 or BF16 (got %d; the fp32 parity mode has no attention kernel)", d->dtype);
    YMI_REQUIRE(d->d == 32 || d->d == 64 || d->d == 128, "ymi_attention: head dimension d in {32, 64, 128} (got %d)", d->d);
    YMI_REQUIRE(d->heads >= 1 && d->c == (int64_t)d->heads * d->d, "ymi_attention: c must equal heads * d (c %d, heads %d, d %d)", d->c, d->heads, d->d);
    YMI_REQUIRE(d->S >= 1 && d->n >= 0, "ymi_attention: S >= 1 tokens and n >= 0 images (got S %d, n %d)", d->S, d->n);
    YMI_REQUIRE(d->q_cstride >= d->c && d->k_cstride >= d->c && d->v_cstride >= d->c && d->o_cstride >= d->c,
                "ymi_attention: pixel strides must be >= c (q %d k %d v %d o %d, c %d)", d->q_cstride, d->k_cstride, d->v_cstride, d->o_cstride, d->c);
    YMI_REQUIRE((d->q_cstride | d->k_cstride | d->v_cstride | d->o_cstride) % 8 == 0, "ymi_attention: pixel strides must be multiples of 8 (q %d k %d v %d o %d)",
                d->q_cstride, d->k_cstride, d->v_cstride, d->o_cstride);
    YMI_REQUIRE(((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->o) % 16 == 0, "ymi_attention: pointers must be 16-byte aligned");
    YMI_REQUIRE(isfinite(d->scale), "ymi_attention: scale must be finite");
    YMI_REQUIRE((int64_t)d->n * d->heads * cdiv(d->S, AT_TQ) < ((int64_t)1 << 31), "ymi_attention: n * heads * ceil(S / %d) does not fit 31 bits", AT_TQ);
    return YMI_OK;
}

int attention_launch(const ymi_attn_desc* d, hipStream_t s) {
    if (const int rc = attention_check(d)) return rc;
    if (d->n == 0) return YMI_OK;
    AttnArgs a;
    a.q = (const uint16_t*)d->q; a.k = (const uint16_t*)d->k; a.v = (const uint16_t*)d->v; a.o = (uint16_t*)d->o;
    a.S = d->S; a.heads = d->heads; a.tiles = cdiv(d->S, AT_TQ); a.q_cs = d->q_cstride; a.k_cs = d->k_cstride; a.v_cs = d->v_cstride; a.o_cs = d->o_cstride; a.scale = d->scale;
    const bool bf = d->dtype == YMI_BF16;
    switch (d->d) {
        case 32: return bf ? attention_launch_one<YMI_BF16, 32>(a, d->n, s) : attention_launch_one<YMI_F16, 32>(a, d->n, s);
        case 64: return bf ? attention_launch_one<YMI_BF16, 64>(a, d->n, s) : attention_launch_one<YMI_F16, 64>(a, d->n, s);
        default: return bf ? attention_launch_one<YMI_BF16, 128>(a, d->n, s) : attention_launch_one<YMI_F16, 128>(a, d->n, s);
    }
}

}  // namespace ymi

extern "C" int ymi_attention(const ymi_attn_desc* d, void* stream) { return ymi::attention_launch(d, (hipStream_t)stream); }
