// fp32 convolution, LDS-DMA pipelined (gfx950) -- the kernel family of the fp32 mode since round 5 (tiles 201-206).
//
// The fp32 mode (fp32 NHWC activations, fp32 folded weights, exact fp32 arithmetic on v_mfma_f32_32x32x2_f32 with two-level
// summation) is the mode in which the HIP path reproduces the reference's fp32 CPU path to rounding-order accuracy (north_star:
// boxes within 1e-3 IoU, equal labels).  Until round 4 it ran on ONE register-staged 128x64 tile with 8-deep steps
// (conv_f32.hip, kept as tile -100: the A/B and bisect partner): 30 % of the 157 TFLOP/s the f32-input MFMA delivers, because a
// step carried 512 cycles of matrix work per wave against a full global-load round trip.  Here:
//   * operands travel HBM/L2 -> LDS with global_load_lds_dwordx4 into a STAGES-deep ring (no VGPR round trip, counted vmcnt,
//     one s_barrier per step); a step is 16 floats deep = 64-byte LDS rows -- BYTE FOR BYTE the piece geometry of the 16-bit
//     kernels (conv_igemm_impl.hpp v2: 1 KiB pieces of 16 rows, XOR swizzle on the source side, conflict-free ds_read_b128);
//   * block tiles up to 128 x 128 (wave tile 64 x 64: 32 MFMAs = 2048 matrix-pipe cycles per wave and step against 8 ds_read_b128
//     and <= 4 DMA instructions), two blocks per CU;
//   * a lane's ds_read_b128 delivers four consecutive k of its row; lanes < 32 take k-chunks {0, 2}, lanes >= 32 chunks {1, 3} of a
//     step.  Two v_permlane32_swap per fragment then hand lanes < 32 the EVEN and lanes >= 32 the ODD k of every pair, so the MFMAs
//     see the k pairs (0, 1), (2, 3), ... in ascending order -- exactly the operands, in exactly the order, of conv_f32.hip;
//   * partial sums of 64 k go to `part` and are folded into `acc` every 4 steps (the summation conv_f32.hip introduced: a plain
//     chain of K FMAs rounds ~sqrt(K) ulp, and the synthetic test networks amplify every ulp on its way to the logits);
//   => every output is BIT-IDENTICAL to the register-staged kernel's, whatever the tile (tests/test_hipsim_kernels.py, tests/test_ops_gpu.py):
//      the detections the reference-made goldens were validated against in rounds 3-4 are reproduced to the last bit, 1.6x faster;
//   * epilogue: + bias, exact SiLU x / (1 + exp(-x)) (torch's CPU formula), + shortcut, 16-byte stores; channel split (C3.cv1 + cv2
//     in one launch) and the x2-upsampled second output (PAN: nn.Upsample folded into its producer) like the 16-bit kernels.
//
// Replaces yolort/v5/models/common.py:69-70 (Conv.forward), :115-116 (Bottleneck shortcut), :172-173 (C3.cv1 / cv2 on one input),
// yolort/models/path_aggregation_network.py:221-223 (1x1 Conv -> nn.Upsample) and yolort/models/box_head.py:36,74 (head conv) -- in
// fp32, like the reference's CPU path.
#include "conv_f32_ring.hpp"   // the ring, the operand forms, the two-level summation and the epilogue (shared with conv_f32_split.hip)

namespace ymi {

// f = {(k0 | k4), (k1 | k5), (k2 | k6), (k3 | k7)} (lanes < 32 | lanes >= 32)  ->  {(k0 | k1), (k4 | k5), (k2 | k3), (k6 | k7)}
__device__ __forceinline__ void pair_even_odd(f32x4& f) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[0]), __float_as_uint(f[1]), false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[2]), __float_as_uint(f[3]), false, false);
    f[0] = __uint_as_float(a[0]);
    f[1] = __uint_as_float(a[1]);
    f[2] = __uint_as_float(b[0]);
    f[3] = __uint_as_float(b[1]);
}

// one 16-deep step in exact fp32: 8 k pairs per tile on v_mfma_f32_32x32x2_f32, in ascending k
struct F32PairMath {
    struct Pos { int p0, p1; };   // byte offset of this lane's k-chunk within its row, ks = 0 / 1
    static __device__ __forceinline__ Pos positions(int hi, int swz) { return {((0 + hi) ^ swz) * 16, ((2 + hi) ^ swz) * 16}; }
    template <int TM, int TN>
    static __device__ __forceinline__ void step(const unsigned char* as, const unsigned char* ws, int frow, Pos p, f32x16 (&part)[TN][TM]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pos = ks == 0 ? p.p0 : p.p1;
            f32x4 af[TM], wf[TN];
#pragma unroll
            for (int j = 0; j < TM; ++j) af[j] = *reinterpret_cast<const f32x4*>(as + (j * 32 + frow) * 64 + pos);
#pragma unroll
            for (int i = 0; i < TN; ++i) wf[i] = *reinterpret_cast<const f32x4*>(ws + (i * 32 + frow) * 64 + pos);
            // (k | k + 4) pairs -> (k | k + 1) pairs: component 0 <-> 1 and 2 <-> 3 exchange their upper / lower lane halves
#pragma unroll
            for (int j = 0; j < TM; ++j) pair_even_odd(af[j]);
#pragma unroll
            for (int i = 0; i < TN; ++i) pair_even_odd(wf[i]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = (q & 1) * 2 + (q >> 1);   // components 0, 2, 1, 3 hold the k pairs (0, 1), (2, 3), (4, 5), (6, 7) of this half-step
#pragma unroll
                for (int i = 0; i < TN; ++i)
#pragma unroll
                    for (int j = 0; j < TM; ++j) part[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[i][e], af[j][e], part[i][j], 0, 0, 0);
            }
        }
    }
};

// What was tried on top of this loop in round 5 and measured on every convolution of the yolov5s bs-32 plan (profiles/r05c_f32_tile_sweep_pipelined_c2.txt,
// r05d_f32_tile_experiments_c2.txt, r05d_f32_one_block_per_cu_c2.txt) -- all bit-identical, none kept:
//   * a software-pipelined loop (next half-step's ds_read_b128 and the ring refill issued between the MFMAs): +-1 % on every layer -- the 64-cycle f32 MFMA leaves the
//     issue port idle anyway;
//   * a four-deep ring: +-1 % (the loop is not DMA-latency-bound);
//   * single-wave blocks of 64 x 64 (no s_barrier at all): 1.2-1.3 x SLOWER (twice the L2 -> LDS operand traffic per flop);
//   * one block per CU (LDS floor): 1.2-1.7 x slower -- a single block reaches ~0.6 of its matrix-pipe time, the second resident block fills the rest.
// SQ_VALU_MFMA_BUSY_CYCLES is 0.53 of the SIMD-cycles at an effective clock of 2.3 GHz (profiles/r05b_rocprof_summary_c2_fp32.csv): the remainder is block-count
// quantisation over 256 CUs (400-800 blocks per launch at 40 x 40 / 20 x 20), the LDS-DMA issue cost inside the MFMA stream and the exact-SiLU epilogue.
template <int BM, int BN, int WM, int WN, int STAGES>
static int launch_f32_pipe(const ConvArgs& a, bool is1x1, hipStream_t s) {
    return launch_f32_ring<BM, BN, STAGES>(a, is1x1, s, "conv_f32_pipe_kernel", [](int mode) -> void (*)(const ConvArgs) {
        if (mode == 1) return conv_f32_pipe_kernel<BM, BN, WM, WN, STAGES, 1, F32PairMath>;
        if (mode == 2) return conv_f32_pipe_kernel<BM, BN, WM, WN, STAGES, 2, F32PairMath>;
        return conv_f32_pipe_kernel<BM, BN, WM, WN, STAGES, 0, F32PairMath>;
    });
}

// Tile choice for tile id 0: a function of the shape only.
// Fitted to the measurement of every tile on every convolution of the yolov5s bs-32 plan (profiles/r05a_f32_tile_sweep_c2.txt): 128 x 64 (four waves per SIMD resident,
// twice the blocks of 128 x 128 to balance over 256 CUs) wins or ties within 3 % wherever cout >= 64, except for the 512-wide layers (128 x 128: 3-5 %); the 32-cout
// layers take 128 x 32.  Every tile produces the same bits, so the choice is a matter of time only.
int conv_f32_pick_tile(int M, int cout_pad) {
    if (cout_pad <= 32) return 206;
    if (cout_pad >= 512 && (long)cdiv(M, 128) * cdiv(cout_pad, 128) >= 256) return 201;
    return 202;
}

int conv_f32_pipe_launch(const ConvArgs& a0, bool is1x1, int tile, hipStream_t s) {
    ConvArgs a = a0;
    { const int rc = conv_f32_ring_prepare(a); if (rc != YMI_OK) return rc; }
    if (tile == 0) tile = conv_f32_pick_tile(a.M, a.cout_pad);
    switch (tile) {
        case 201: return launch_f32_pipe<128, 128, 64, 64, 3>(a, is1x1, s);
        case 202: return launch_f32_pipe<128, 64, 64, 32, 3>(a, is1x1, s);
        case 203: return launch_f32_pipe<64, 64, 32, 32, 3>(a, is1x1, s);
        case 204: return launch_f32_pipe<256, 64, 64, 64, 3>(a, is1x1, s);
        case 205: return launch_f32_pipe<256, 32, 64, 32, 3>(a, is1x1, s);
        case 206: return launch_f32_pipe<128, 32, 32, 32, 3>(a, is1x1, s);
        default: break;
    }
    set_error("ymi_conv2d (fp32): unknown tile id %d (201-206, 0 = by shape, negative = the register-staged kernel)", tile);
    return YMI_EINVAL;
}

}  // namespace ymi
