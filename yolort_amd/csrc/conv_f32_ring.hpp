// The fp32 mode's LDS-DMA ring, two-level summation and epilogue, shared by its two kernel families:
//   conv_f32_pipe.hip   tiles 201-206: exact fp32 arithmetic on v_mfma_f32_32x32x2_f32
//   conv_f32_split.hip  tiles 211-216 / 221-226: every fp32 operand split in registers into three bf16 terms, 6 / 8 products per 16-deep step on v_mfma_f32_32x32x16_bf16
// Everything but the arithmetic of one step lives here -- operand movement (global_load_lds_dwordx4 into a STAGES-deep ring of 64-byte rows, XOR swizzle on the source
// side, counted vmcnt, one s_barrier per step), the three operand forms, `part` folded into `acc` every 4 steps, and the epilogue (+ bias, exact SiLU, + shortcut,
// 16-byte stores, channel split, x2-upsampled second output).  A family supplies `Math::step`: LDS rows of this wave's tile -> MFMAs into `part`.
#pragma once
#include "conv_common.hpp"

namespace ymi {

extern __shared__ __attribute__((aligned(16))) unsigned char f32p_sm[];   // the ONLY LDS object of a unit that includes this header

constexpr int FBK = 16;   // floats per main-loop step (64-byte rows)

__device__ __forceinline__ float silu_exact_f32(float v) { return v / (1.0f + expf(-v)); }   // torch CPU: x / (1 + exp(-x))

__device__ __forceinline__ void glds16f(const float* g, unsigned char* lds_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)lds_wave_uniform, 16, 0, 0);
}

// MODE 0: im2col table (any cin % 8 == 0: the stem's super-pixels), 1: pointwise (k1 s1 p0), 2: uniform tap (cin % 16 == 0: a step lies inside one tap)
// Math::positions(hi, swz) -> the byte offsets of a lane's k-chunks within its rows (row r holds its k-chunk c of four floats at byte (c ^ ((r >> 2) & 3)) * 16; swz is that
// XOR term for the rows frow, 32 + frow, ... a lane reads); Math::step<TM, TN>(as, ws, frow, pos, part): `as` / `ws` = this wave's first activation / weight row of the
// landed stage; part[i][j] += W-tile i x A-tile j.
// The kernel itself is the template (not a body called from per-family kernels): handing the by-value kernel argument on to a callee changed where its fields are loaded and
// cost tiles 201 / 204 / 206 up to 8 VGPRs; instantiated with F32PairMath it compiles to the registers, scratch and LDS of the parent's unit (profiles/f32_split_registers.txt).
template <int BM, int BN, int WM, int WN, int STAGES, int MODE, class Math>
__global__ __launch_bounds__(256, 2) void conv_f32_pipe_kernel(const ConvArgs a) {
    constexpr int NW = 4;
    static_assert((BM / WM) * (BN / WN) == NW, "4 waves per block");
    static_assert(BM % 16 == 0 && BN % 16 == 0 && (BM / 16) % NW == 0, "activation pieces are dealt evenly to the waves");
    static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int PA = BM / 16 / NW;             // activation pieces (1 KiB = 16 rows x 64 B) per wave per stage
    constexpr int W_PIECES = BN / 16;
    constexpr int PW = (W_PIECES + NW - 1) / NW; // weight pieces per wave per stage (surplus waves re-send the last piece: identical bytes)
    constexpr int P = PA + PW;                   // DMA instructions per wave per stage, the same for every wave
    constexpr int STAGE_BYTES = (BM + BN) * 64;

    const float* __restrict__ X = reinterpret_cast<const float*>(a.x);
    const float* __restrict__ Wt = reinterpret_cast<const float*>(a.w);
    int2* ktab_lds = reinterpret_cast<int2*>(f32p_sm + STAGES * STAGE_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = (wave / WAVES_N) * WM, wave_n = (wave % WAVES_N) * WN;
    const int hi = lane >> 5, frow = lane & 31;

    const int nblk = a.nblk_m * a.nblk_n;
    const int lb = xcd_remap(blockIdx.x, nblk);
    const int bm = lb / a.nblk_n, bn = lb % a.nblk_n;   // cout tile fastest: the blocks sharing an activation tile run back to back on one XCD
    const int m0 = bm * BM, n0 = bn * BN;
    const int nsteps = a.k_pad / FBK;

    // bias first: these loads retire before every operand DMA issued behind them (in-order return), so the counted waits below stay exact
    f32x4 bias_regs[TN][4];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = n0 + wave_n + i * 32 + g * 8 + hi * 4;
            bias_regs[i][g] = *reinterpret_cast<const f32x4*>(a.bias + (co < a.cout_pad ? co : 0));   // rows past cout_pad are never stored
        }

    if constexpr (MODE == 0) {
        for (int i = tid; i < a.k_pad / 8; i += 64 * NW) ktab_lds[i] = a.ktab[i];
    }

    // ---- per-lane DMA geometry (element = float offsets against a.x / a.w; out-of-range chunks read the zero page in x's own tail) ----
    const int sub_row = lane >> 2;
    const int chunk = (lane & 3) ^ ((lane >> 4) & 3);      // k-chunk fetched = position ^ ((row >> 2) & 3): linear destination, permuted source
    int a_off[PA], a_aux[PA];
#pragma unroll
    for (int j = 0; j < PA; ++j) {
        const int pi = wave * PA + j;
        const int m = m0 + pi * 16 + sub_row;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        if constexpr (MODE == 1) {
            a_off[j] = mm * a.x_cs;
            a_aux[j] = ok ? 0 : -1;
        } else {
            const int hw_o = a.ho * a.wo;
            const int img = fast_div(mm, hw_o, a.magic_hw);
            const int rem = mm - img * hw_o;
            const int oy = fast_div(rem, a.wo, a.magic_w), ox = rem - oy * a.wo;
            const int iy0 = oy * a.sh - a.ph, ix0 = ox * a.sw - a.pw;
            a_off[j] = ((img * a.h + iy0) * a.w_in + ix0) * a.x_cs;
            if constexpr (MODE == 2) {
                unsigned mask = 0;
                int t = 0;
                for (int dy = 0; dy < a.kh; ++dy) {
                    const bool yin = (unsigned)(iy0 + dy) < (unsigned)a.h;
                    for (int dx = 0; dx < a.kw; ++dx, ++t) mask |= ((yin && ((unsigned)(ix0 + dx) < (unsigned)a.w_in)) ? 1u : 0u) << t;
                }
                a_aux[j] = ok ? (int)mask : 0;
            } else {
                a_aux[j] = ok ? (((iy0 + 16384) << 16) | ((ix0 + 16384) & 0xffff)) : -1;
            }
        }
    }
    int w_off[PW], w_slot[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        int pi = wave * PW + j;
        pi = pi < W_PIECES ? pi : W_PIECES - 1;
        w_slot[j] = (BM / 16 + pi) * 1024;
        w_off[j] = (n0 + pi * 16 + sub_row) * a.k_pad + chunk * 4;   // rows are zero-padded to a multiple of 128 (engine.PackedConv)
    }

    int u_tap = 0, u_c0 = 0, u_dx = 0, u_kbase = 0;   // MODE 2 running state (stages are issued in order): wave-uniform scalars
    // one stage = issue_begin(step); issue_piece(0 .. P-1); issue_end()   (pieces 0 .. PA-1 activations, PA .. P-1 weights)
    unsigned char* cur_stage = f32p_sm;
    int cur_koff = 0, cur_dy = 0, cur_dx = 0, cur_step = 0;
    bool cur_tap_ok = true;
    auto issue_begin = [&](int step) {
        cur_stage = f32p_sm + (step % STAGES) * STAGE_BYTES;
        cur_step = step;
        if constexpr (MODE == 2) {
            cur_koff = u_kbase + chunk * 4;
        } else if constexpr (MODE == 1) {
            cur_koff = step * FBK + chunk * 4;
            cur_tap_ok = cur_koff < a.cin;
        } else {
            const int2 t = ktab_lds[step * 2 + (chunk >> 1)];   // one table entry per 8 elements: two 4-float chunks
            cur_koff = t.x + (chunk & 1) * 4;
            cur_tap_ok = t.y >= 0;
            cur_dy = t.y >> 16;
            cur_dx = t.y & 0xffff;
        }
    };
    auto issue_piece = [&](auto jt) {
        constexpr int j = decltype(jt)::value;
        if constexpr (j < PA) {
            bool ok;
            if constexpr (MODE == 2) {
                ok = (a_aux[j] >> u_tap) & 1;
            } else {
                ok = cur_tap_ok & (a_aux[j] >= 0);
                if constexpr (MODE == 0) {
                    const int iy = (a_aux[j] >> 16) - 16384 + cur_dy, ix = (a_aux[j] & 0xffff) - 16384 + cur_dx;
                    ok = ok & ((unsigned)iy < (unsigned)a.h) & ((unsigned)ix < (unsigned)a.w_in);
                }
            }
            glds16f(X + (ok ? a_off[j] + cur_koff : a.x_zero_off), cur_stage + (wave * PA + j) * 1024);
        } else if constexpr (j < P) {
            glds16f(Wt + (w_off[j - PA] + cur_step * FBK), cur_stage + w_slot[j - PA]);
        }
    };
    auto issue_end = [&]() {
        if constexpr (MODE == 2) {
            u_c0 += FBK;
            u_kbase += FBK;
            if (u_c0 == a.cin) {
                u_c0 = 0;
                ++u_tap;
                ++u_dx;
                u_kbase += a.x_cs - a.cin;
                if (u_dx == a.kw) {
                    u_dx = 0;
                    u_kbase += (a.w_in - a.kw) * a.x_cs;
                }
            }
        }
    };
    auto issue = [&](int step) {
        issue_begin(step);
        static_for<0, P>(issue_piece);
        issue_end();
    };

    f32x16 acc[TN][TM], part[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; part[i][j][r] = 0.f; }

    if constexpr (MODE == 0) __syncthreads();   // table visible (no DMA in flight yet)
    const int swz = (lane >> 2) & 3;
    const auto pos = Math::positions(hi, swz);   // byte offsets of this lane's k-chunks within its rows
    auto fold = [&](int step) {
        if ((step & 3) == 3 || step + 1 == nsteps) {   // 64 k per partial sum
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { acc[i][j][r] += part[i][j][r]; part[i][j][r] = 0.f; }
        }
    };

#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
        if (s < nsteps) issue(s);

    for (int step = 0; step < nsteps; ++step) {
        // this wave's pieces of stage `step` have landed once at most `ahead` later stages are pending
        const int issued = (step + STAGES - 1 < nsteps) ? step + STAGES - 1 : nsteps;
        const int ahead = issued - (step + 1);
        if (ahead >= 2) wait_vmcnt<2 * P>();
        else if (ahead == 1) wait_vmcnt<P>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();          // every wave's pieces landed; everyone is done with stage step - 1
        __builtin_amdgcn_sched_barrier(0);
        if (step + STAGES - 1 < nsteps) issue(step + STAGES - 1);   // refill the slot freed by step - 1
        const unsigned char* as = f32p_sm + (step % STAGES) * STAGE_BYTES + wave_m * 64;
        const unsigned char* ws = f32p_sm + (step % STAGES) * STAGE_BYTES + (BM + wave_n) * 64;
        Math::template step<TM, TN>(as, ws, frow, pos, part);
        fold(step);
    }

    // ---- epilogue: + bias, exact SiLU, + shortcut (after the activation), 16-byte fp32 stores ----
    const float* __restrict__ R = reinterpret_cast<const float*>(a.res);
    const int hw_o = a.ho * a.wo;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int64_t mo = (int64_t)m0 + wave_m + j * 32 + frow;
        if (mo >= a.M) continue;
        int64_t m_up = 0;
        if (a.up2) {   // wave-uniform flag: pixel (img, oy, ox) -> top-left of its 2 x 2 block in the (n, 2 ho, 2 wo) view y2
            const int img = fast_div((int)mo, hw_o, a.magic_hw);
            const int rem = (int)mo - img * hw_o;
            const int oy = fast_div(rem, a.wo, a.magic_w), ox = rem - oy * a.wo;
            m_up = ((int64_t)img * 2 * a.ho + 2 * oy) * (2 * a.wo) + 2 * ox;
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = n0 + wave_n + i * 32 + g * 8 + hi * 4;
                if (co >= a.cout) continue;
                f32x4 rr = {0.f, 0.f, 0.f, 0.f};
                const bool full = co + 3 < a.cout;
                if (R != nullptr) {
                    if (full && (a.res_cs & 3) == 0) rr = *reinterpret_cast<const f32x4*>(R + mo * a.res_cs + co);
                    else
                        for (int e = 0; e < 4 && co + e < a.cout; ++e) rr[e] = R[mo * a.res_cs + co + e];
                }
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[i][j][g * 4 + e] + bias_regs[i][g][e];
                    if (a.act == YMI_ACT_SILU) t = silu_exact_f32(t);
                    if (R != nullptr) t += rr[e];
                    v[e] = t;
                }
                float* yp;
                int cs;
                if (a.split > 0 && co >= a.split) { yp = reinterpret_cast<float*>(a.y2) + mo * a.y2_cs + (co - a.split); cs = a.y2_cs; }
                else { yp = reinterpret_cast<float*>(a.y) + mo * a.y_cs + co; cs = a.y_cs; }
                if (full && (cs & 3) == 0 && (a.split & 3) == 0) {
                    *reinterpret_cast<f32x4*>(yp) = v;
                } else {
                    for (int e = 0; e < 4 && co + e < a.cout; ++e) yp[e] = v[e];
                }
                if (a.up2) {   // launch checks: cout % 4 == 0, y2_cs % 4 == 0, no split
                    float* up = reinterpret_cast<float*>(a.y2) + m_up * a.y2_cs + co;
                    const int64_t row = (int64_t)2 * a.wo * a.y2_cs;
                    *reinterpret_cast<f32x4*>(up) = v;
                    *reinterpret_cast<f32x4*>(up + a.y2_cs) = v;
                    *reinterpret_cast<f32x4*>(up + row) = v;
                    *reinterpret_cast<f32x4*>(up + row + a.y2_cs) = v;
                }
            }
        }
    }
}

// Launch-time checks of the pipelined fp32 families (zero page, strides, 32-bit offsets); fills a.x_zero_off.
inline int conv_f32_ring_prepare(ConvArgs& a) {
    YMI_REQUIRE(a.zeros != nullptr, "ymi_conv2d (fp32, pipelined tiles): desc.zeros is required (the 256-byte zero tail of x's buffer)");
    YMI_REQUIRE(a.chain_w == nullptr, "ymi_conv2d: the fp32 mode has no chained convolution");
    YMI_REQUIRE(a.x_cs % 4 == 0 && a.cin % 8 == 0 && a.k_pad % 32 == 0, "ymi_conv2d (fp32): x_cstride %% 4, cin %% 8 and k_pad %% 32 must be 0");
    YMI_REQUIRE(a.split == 0 || a.split % 4 == 0, "ymi_conv2d (fp32): cout_split must be a multiple of 4");
    YMI_REQUIRE(!a.up2 || (a.cout % 4 == 0 && a.y2_cs % 4 == 0 && a.split == 0 && a.y_cs % 4 == 0), "ymi_conv2d (fp32): the upsampled second output needs cout %% 4 == 0 and 16-byte aligned pixel strides");
    const int64_t dz = ((const char*)a.zeros - (const char*)a.x);
    YMI_REQUIRE(dz % 16 == 0 && dz / 4 > -((int64_t)1 << 31) && dz / 4 < ((int64_t)1 << 31), "ymi_conv2d (fp32): desc.zeros must lie within range of x and be 16-byte aligned relative to it");
    a.x_zero_off = (int)(dz / 4);
    YMI_REQUIRE((int64_t)a.n * a.h * a.w_in * a.x_cs < ((int64_t)1 << 31) && (int64_t)(a.cout_pad + 127) / 128 * 128 * a.k_pad < ((int64_t)1 << 31), "ymi_conv2d (fp32): tensor too large for 32-bit element offsets");
    return YMI_OK;
}

// grid, LDS size and operand form of one launch; `pick(mode)` returns the kernel of MODE 0 / 1 / 2
template <int BM, int BN, int STAGES, class Pick>
static int launch_f32_ring(const ConvArgs& a0, bool is1x1, hipStream_t s, const char* name, Pick pick) {
    ConvArgs a = a0;
    a.nblk_m = cdiv(a.M, BM);
    a.nblk_n = cdiv(a.cout_pad, BN);
    const bool utap = !is1x1 && (a.cin % FBK == 0) && (a.kh * a.kw <= 32);
    size_t lds = (size_t)STAGES * (BM + BN) * 64 + ((is1x1 || utap) ? 0 : (size_t)a.k_pad) + 16;
    if (lds < lds_floor_bytes()) lds = lds_floor_bytes();
    dim3 grid(a.nblk_m * a.nblk_n), block(256);
    void (*kfn)(const ConvArgs) = pick(is1x1 ? 1 : (utap ? 2 : 0));
    if (lds > 64 * 1024) { const int rc = allow_big_lds((const void*)kfn, (int)lds); if (rc != YMI_OK) return rc; }
    hipLaunchKernelGGL(kfn, grid, block, lds, s, a);
    return check_launch(name);
}

}  // namespace ymi
