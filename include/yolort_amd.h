/*
 * yolort_amd.h -- C ABI of libyolort_amd.so, the MI355X (gfx950) YOLOv5 inference hot path.
 *
 * This is the drop-in boundary.  The reference (zhiqwang/yolort) has no C
 * plugin ABI of its own: its plug points are Python constructor injection and ATen/torchvision
 * operators.  Each entry point below therefore replaces one ATen/torchvision call site of the
 * reference's hot path and cites it (paths relative to the reference root).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + explicit sizes, no torch types; `stream` is a hipStream_t
 *     passed as void* (NULL = default stream).  The caller owns every buffer.
 *   - every function returns 0 on success or a negative YMI_E* code and never throws; the message
 *     of the last failure on the calling thread is available from ymi_last_error().
 *   - no hidden hipDeviceSynchronize / hipMalloc; thread-safe for distinct streams.
 *   - activations are NHWC ("pixel-major"): element (n,y,x,c) of a view lives at
 *       base + ((n*H + y)*W + x) * cstride + c        (cstride >= C lets a view be a channel slice
 *     of a wider concat buffer -- this is how torch.cat is eliminated).
 */
#ifndef YOLORT_AMD_H
#define YOLORT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YMI_ABI_VERSION 6

/* error codes */
#define YMI_OK 0
#define YMI_EINVAL -1   /* bad argument / unsupported shape */
#define YMI_EHIP -2     /* HIP runtime error (message has hipGetErrorString) */
#define YMI_ENOMEM -3   /* caller-provided capacity too small (retry with the reported size) */

/* element types */
#define YMI_F16 0
#define YMI_BF16 1
#define YMI_F32 2
#define YMI_U8 3
#define YMI_U8_HWC 4 /* ymi_letterbox input only: interleaved (h, w, 3) uint8, as image decoders deliver it */

/* activation after conv */
#define YMI_ACT_NONE 0
#define YMI_ACT_SILU 1
/* the activations of the legacy r3.1 blocks (common.py:64-65 `Conv(version="r3.1")`: Hardswish; common.py:140 `BottleneckCSP.act`: LeakyReLU(0.1)): NOT carried by the
 * convolution epilogues (ymi_conv2d refuses them) -- such a convolution runs with YMI_ACT_NONE and ymi_act rewrites its output in place */
#define YMI_ACT_HARDSWISH 2
#define YMI_ACT_LEAKY 3

int ymi_abi_version(void);
const char* ymi_last_error(void);
/* number of HIP devices visible, or a negative error; used by the loud "no GPU" check */
int ymi_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Letterbox: per-image aspect-preserving bilinear resize + centred constant pad + dtype cast +
 * CHW -> NHWC(c_out) layout change, one launch for the whole batch.
 * Replaces yolort/models/transform.py:53-97 (_resize_image_and_masks -> F.interpolate bilinear,
 * align_corners=False, recompute_scale_factor=True) and :297-330 (batch_images: new_full + copy_).
 * The host computes resized sizes / pad offsets with the reference's float recipe
 * (yolort_amd.models.transform) and passes them in `geom`.
 *   imgs[i]     device pointer to image i, planar CHW (3,h,w), contiguous, dtype in_dtype
 *               (YMI_F32 / YMI_F16 / YMI_BF16 in [0,1], or YMI_U8 in [0,255] which is scaled by 1/255);
 *               YMI_U8_HWC: interleaved (h,w,3) uint8 instead (the /255, the HWC -> CHW permute of
 *               yolov5.py:218-228 and the letterbox are then one kernel)
 *   geom[i*6..] {h_in, w_in, h_resized, w_resized, pad_top, pad_left}
 *   out         (n, hb, wb, c_out) NHWC, dtype out_dtype, channels 3..c_out-1 zero-filled
 *   fill        pad value (reference: 114/255, transform.py:141)
 * ---------------------------------------------------------------------------------------- */
int ymi_letterbox(const void* const* imgs, const int32_t* geom, int n, int in_dtype, void* out, int hb,
                  int wb, int c_out, int out_dtype, float fill, void* stream);

/* ------------------------------------------------------------------------------------------
 * View canvas of augmented inference (test-time augmentation): a scaled, optionally left-right mirrored copy of the
 * letterboxed NHWC4 canvas.  Replaces yolort/v5/utils/torch_utils.py:288-300 (scale_img: F.interpolate bilinear,
 * align_corners=False, then F.pad with 0.447) and the x.flip(3) of yolort/v5/models/yolo.py:158, in one launch.
 *   src   (n, h, w, 4) NHWC4 of `dtype` (YMI_F16 / YMI_BF16 / YMI_F32); channel 3 is not read
 *   dst   (n, dh, dw, 4) NHWC4 of the same dtype; channel 3 is written as zero (the layout the stem reads)
 *   sh,sw the resized size, 1 <= sh <= dh, 1 <= sw <= dw.  The host computes the sizes as the reference does, in Python
 *         floats: sh, sw = int(h * r), int(w * r); dh, dw = ceil(h * r / gs) * gs, ceil(w * r / gs) * gs (gs = largest stride)
 *   flip  != 0: column x of the source is column w - 1 - x of `src` (mirror first, then scale, as the reference does)
 * Pixels inside (sh, sw): ATen's upsample_bilinear2d -- source index (dst + 0.5) * (in / out) - 0.5 (in / out rounded to fp32, then ONE
 * fused multiply-add: the exact expression rounded once, as ATen's CPU kernel computes it) clamped at 0, second tap clamped at in - 1,
 * weights l1 = index - floor, l0 = 1 - l1, in fp32.  The value is mathematically h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11); it is
 * evaluated over the four tap weights w_ij = fl(h_i * w_j) as fma(w11, v11, fma(w10, v10, fma(w00, v00, fl(w01 * v01)))) -- the order in which
 * the result equals F.interpolate bit for bit when the weights are powers of two (ratio 0.5); the nested form is an ulp away from it there --
 * then ONE rounding to `dtype`.  Pixels outside: 0.447 rounded to `dtype`.
 * Nothing outside dst's n * dh * dw pixels is written.
 * ---------------------------------------------------------------------------------------- */
#define YMI_VIEW_PAD 0.447f
int ymi_scale_view(const void* src, int n, int h, int w, void* dst, int dh, int dw, int sh, int sw, int flip, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Detection crops: every detection of the slab cut out of its ORIGINAL image and resized to one fixed size, in one launch per batch -- the input of a
 * second-stage classifier, a re-identification or OCR net, or a dataset of cut-outs.  Replaces the host loops of save_one_box (yolort/v5/utils/plots.py:545-558,
 * reached from Detections.crop, yolort/v5/models/common.py:644) and of apply_classifier (yolort/v5/utils/general.py:691-723), one cv2.resize per box.
 *   imgs[i]   HOST array of n device pointers, the images as ymi_letterbox takes them: planar CHW (3, h, w) of in_dtype YMI_F32 / YMI_F16 / YMI_BF16 in [0, 1] or
 *             YMI_U8 (scaled by 1/255, a true division), or interleaved (h, w, 3) uint8 for YMI_U8_HWC
 *   hw        HOST array {h, w} per image
 *   boxes     device (n, k, 4) fp32 xyxy in original-image coordinates, counts device (n) int32: the slab exactly as the top-k kernel writes it.  Slots at or past
 *             a count are never read; a count below 0 or above k is clamped and sets YMI_CROP_STATUS_BAD_COUNT
 *   crops     device (cap, 3, out_h, out_w) planar NCHW of out_dtype (YMI_F16 / YMI_BF16 / YMI_F32); index device (cap, 6) int32; total device int32[2]
 * Rectangle of a detection, every operation a rounded fp32 one in the order torch evaluates save_one_box (plots.py:548-553 with general.py:397-400, :410-413, :507-510):
 *   cx = (x1 + x2) / 2, cy = (y1 + y2) / 2, w = x2 - x1, h = y2 - y1;  square != 0: w = h = max(w, h);  w = w * gain + pad, h = h * gain + pad (two roundings each);
 *   corners cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, each truncated toward zero (.long()), then x clamped into [0, W], y into [0, H] (clip_coords).
 * The crop is rows y1:y2 and columns x1:x2 of the image.  A non-finite coordinate (of the box or of a corner) gives the empty rectangle (0, 0, 0, 0); an empty
 * rectangle (x2 <= x1 or y2 <= y1) gives an all-zero crop (not normalised) and keeps its row, so crops stay aligned with the detections; its index row reports the
 * clipped corners as the reference computes them (e.g. {64, 0, 64, 14} for a box right of a 64-wide image).  gain / pad: save_one_box
 * has 1.02 / 10, apply_classifier square, 1.3 / 30 -- but the reference pads in canvas pixels before scale_coords, this pads in image pixels (no parity claimed).
 * Resize to (out_h, out_w): ymi_scale_view's arithmetic (ATen's upsample_bilinear2d, align_corners=False) INSIDE the rectangle -- scale = in / out rounded to fp32,
 * source index ONE fmaf(scale, dst + 0.5, -0.5) clamped at 0, second tap clamped at the rectangle's last row / column (not the image's), four tap weights
 * w_ij = fl(h_i * w_j), value fma(w11, v11, fma(w10, v10, fma(w00, v00, fl(w01 * v01)))) -- bit-identical to F.interpolate(mode="bilinear", align_corners=False) of
 * the cut-out wherever the weights are powers of two (a rectangle of the output's size or twice it).  normalize != 0: then (v - mean[c]) / std[c], a rounded
 * subtraction and a correctly rounded division.  ONE rounding to out_dtype.  (cv2.resize on uint8 uses fixed-point weights and differs in the last bit of a byte.)
 * Order: image-major, the slab's order inside an image: row offset[i] + j holds detection j of image i, offset = the exclusive prefix of min(counts[i], k), computed
 * on the device by every workgroup (crop_resize_kernel, csrc/preproc_pool.hip: a workgroup owns 256 x 4 adjacent pixels of one crop, 8- / 16-byte stores per plane
 * where out_w % 4 == 0, scalar stores else).  index row = {image, detection, x1, y1, x2, y2} (the rectangle); total[0] = crops written = min(sum of the clamped
 * counts, cap); total[1] = status: YMI_CROP_STATUS_CAPACITY when the sum exceeds cap (the first cap crops are written, the rest dropped),
 * YMI_CROP_STATUS_BAD_COUNT.  Both words are WRITTEN by every call.  Rows at or beyond total[0] are not written, in crops or in index; nothing outside the two
 * buffers and total is written.  More than 64 images go as several launches over image ranges that all read the whole counts array (offsets stay global).
 * YMI_EINVAL: a null buffer (crops / index may be null only with cap 0, the inputs only with n 0), out_h or out_w < 1, cap < 0, n or k < 0, an unsupported dtype, normalize with a std of 0,
 * gain / pad (or mean / std) not finite.  No allocation, no synchronisation: ordered on `stream`, may be captured.  ABI stays 6: one new struct, one new function.
 * ---------------------------------------------------------------------------------------- */
#define YMI_CROP_STATUS_CAPACITY 1  /* total[1] bit 0 */
#define YMI_CROP_STATUS_BAD_COUNT 2 /* total[1] bit 1 */
typedef struct ymi_crop_desc {
    const void* const* imgs;
    const int32_t* hw;
    const float* boxes;
    const int32_t* counts;
    void* crops;
    int32_t* index;
    int32_t* total;
    float mean[3], std[3];
    float gain, pad;
    int32_t n, k, cap;
    int32_t out_h, out_w;
    int32_t in_dtype, out_dtype;
    int32_t square, normalize;
    int32_t reserved;
} ymi_crop_desc;
int ymi_crop_resize(const ymi_crop_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Annotated images: every detection of the slab drawn into its ORIGINAL image -- outline, label background, label text -- IN PLACE, in one launch per batch.
 * Replaces the host loop of Detections.render() / show() / save() (yolort/v5/models/common.py:575-652): per detection one Annotator.box_label
 * (yolort/v5/utils/plots.py:98-159) = three drawing calls, with the images leaving the device and coming back around it.
 *   imgs[i]   HOST array of n device pointers, the images as ymi_letterbox / ymi_crop_resize take them, WRITTEN in place: planar CHW (3, h, w) of in_dtype YMI_F32 /
 *             YMI_F16 / YMI_BF16 in [0, 1] or YMI_U8, or interleaved (h, w, 3) uint8 for YMI_U8_HWC
 *   hw        HOST array {h, w} per image;  lw, fs: HOST arrays, per image the outline width and the integer font scale, each in [1, 65535]
 *   boxes     device (n, k, 4) fp32 xyxy in original-image coordinates, scores (n, k) fp32, labels (n, k) int64, counts (n) int32: the slab as ymi_eval_desc takes it
 *   names     device (num_classes, YMI_RENDER_NAME_STRIDE) uint8: a length byte in 0..27 (a larger one counts as 27), then the bytes; null: the class index in decimal
 *   colors    device (m, 3) uint8 RGB; a detection has colors[label % m];  txt_color: RGB of the text, each in 0..255
 * THE DRAWING RULE (integer arithmetic throughout; x, y are pixel indices of the image):
 *   Corners   X0, Y0, X1, Y1 = the box's x1, y1, x2, y2 truncated toward zero (the int(box[i]) of the reference's cv2 branch, the truncation ymi_crop_resize uses).
 *             A detection draws NOTHING when a coordinate is not finite or has magnitude >= 2^24, or X1 < X0, or Y1 < Y0.
 *   Outline   of width lw: the pixels with X0 <= x <= X1, Y0 <= y <= Y1 and (x < X0 + lw or x > X1 - lw or y < Y0 + lw or y > Y1 - lw), clipped to the image.  This is
 *             PIL.ImageDraw.rectangle(width=lw, outline=...) -- the call of the reference's PIL branch -- wherever 2 * lw <= min(X1 - X0, Y1 - Y0) + 1; for thicker
 *             outlines this rule fills the box, while PIL paints outside it: the rule is the contract there.
 *   Label     (draw_labels != 0) text = the class name, then (draw_conf != 0) ' ' and the score as %.2f; L characters, L == 0 draws no label.  Cells of 6 x 11 pixels
 *             magnified fs times by pixel replication: w = 6 * fs * L, h = 11 * fs.  Placement is box_label's PIL branch: outside = (Y0 - h >= 0), ty = Y0 - h if
 *             outside, else Y0.  Background: the inclusive rectangle [X0, ty, X0 + w + 1, ty + h + 1] in the box colour, clipped to the image.  Glyphs: pixel (x, y) of
 *             [X0, X0 + w) x [ty, ty + h) belongs to character (x - X0) / (6 * fs), column ((x - X0) % (6 * fs)) / fs, row (y - ty) / fs; a set bit gives txt_color.
 *   Pixel     the LOWEST slot whose outline or label background covers the pixel decides: txt_color where a glyph bit of THAT detection is set, its box colour
 *             elsewhere -- the result of the reference's draw order (reversed(pred); outline, background, text per box).  A pixel no detection covers is not written.
 *   Colour    uint8 images store the byte; float images store byte / 255, a true division rounded ONCE to the dtype (for all 256 bytes the fp32 quotient rounded to
 *             fp16 / bf16 equals the directly rounded one).
 *   Score     a finite score in [0, 1] prints as the exact value of the fp32 score times 100 rounded to nearest, ties to even, "d.dd" -- what Python's
 *             f"{float(score):.2f}" prints (0.125 -> 0.12, 0.375 -> 0.38); the product is exact in fp64 (24 + 7 bits).  -0.0 compares as 0 and prints "-0.00", as
 *             Python does.  Any other score (NaN, negative, above 1, infinite) prints "?.??".
 *   Names     a byte outside 32..126 draws as '?'.  ASCII only, at most 27 bytes.
 *   Font      95 cells of 6 x 11 bits from Pillow's built-in bitmap font, one getmask() per character (csrc/render_font.hpp, tools/make_render_font.py).  The TEXT HAS
 *             NO PARITY WITH THE REFERENCE: that needs a downloaded Arial.ttf or cv2's Hershey strokes; outline and background geometry are the reference's PIL branch.
 *   Counts    slots at or past a count are never read; a count above k is taken as k and sets YMI_RENDER_STATUS_BAD_COUNT; a negative count (a stale slab row,
 *             YMI_SLAB_STALE) skips the image and sets YMI_RENDER_STATUS_STALE_ROW; a label outside [0, num_classes) skips that detection and sets
 *             YMI_RENDER_STATUS_BAD_LABEL.  status is ONE int32 the kernel ORs bits into; the caller zeroes it.
 *   Writes    nothing outside the images' own h * w * 3 elements, and no pixel that no detection covers.
 * render_kernel (csrc/preproc_pool.hip) is a GATHER, no races and no atomics on pixels: a workgroup owns a tile of 64 x 16 pixels of one image, compacts the
 * detections whose drawing extent (outline united with label background) meets the tile into an LDS list in slot order (wave ballot + prefix), returns WITHOUT
 * touching the image when the list is empty, and otherwise lets every pixel take its colour from the first list entry that covers it.  A thread owns four adjacent
 * pixels (12 contiguous bytes interleaved, 4 / 8 / 16 bytes per plane; scalar stores where w % 4 != 0, the view is misaligned or only some of the four are covered).
 * Ragged sizes: the grid is the sum of the images' tiles, found from a by-value table; more than 64 images go as several launches.
 * YMI_EINVAL: a null buffer (names may be null; everything may be with n 0), k > YMI_RENDER_MAX_K, n or k < 0, an lw or fs outside [1, 65535], m < 1, num_classes < 1,
 * a txt_color outside 0..255, an unsupported dtype, a null image or a negative size.  No allocation, no synchronisation: ordered on `stream`, may be captured.
 * ABI stays 6: one new struct, one new function.
 * ---------------------------------------------------------------------------------------- */
#define YMI_RENDER_MAX_K 1024
#define YMI_RENDER_NAME_STRIDE 28
#define YMI_RENDER_STATUS_BAD_COUNT 1 /* status bit 0 */
#define YMI_RENDER_STATUS_STALE_ROW 2 /* status bit 1 */
#define YMI_RENDER_STATUS_BAD_LABEL 4 /* status bit 2 */
typedef struct ymi_render_desc {
    void* const* imgs;
    const int32_t* hw;
    const int32_t* lw;
    const int32_t* fs;
    const float* boxes;
    const float* scores;
    const int64_t* labels;
    const int32_t* counts;
    const uint8_t* names;
    const uint8_t* colors;
    int32_t* status;
    int32_t m;
    int32_t txt_color[3];
    int32_t num_classes, in_dtype;
    int32_t draw_labels, draw_conf;
    int32_t n, k;
    int32_t reserved;
} ymi_render_desc;
int ymi_render(const ymi_render_desc* d, void* stream);

/* NCHW (n,c,h,w) -> NHWC view and back (module-level API edges; not on the fused path). */
int ymi_nchw_to_nhwc(const void* x, int n, int c, int h, int w, int in_dtype, void* y, int y_cstride,
                     int c_pad, int out_dtype, void* stream);
int ymi_nhwc_to_nchw(const void* x, int x_cstride, int n, int c, int h, int w, int in_dtype, void* y,
                     int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused convolution: y = act(conv2d(x, W) + bias) (+ residual), implicit GEMM on MFMA.
 * Replaces yolort/v5/models/common.py:69-70 `Conv.forward` = SiLU(BN(conv2d(x))) with BatchNorm
 * folded into W/bias on the host (formula of yolort/v5/utils/torch_utils.py:238-245, eps 1e-3),
 * the residual add of common.py:115-116 (Bottleneck) and, with act=NONE and a real bias, the
 * biased 1x1 head conv of yolort/models/box_head.py:36,74.
 *   x        NHWC view (n,h,w,cin) with pixel stride x_cstride; cin % 8 == 0
 *   w        packed weights [cout_pad][k_pad], k index = (ky*kw + kx)*cin + c, dtype = `dtype`,
 *            zero padded; cout_pad % 32 == 0, k_pad % 32 == 0  (see ymi_conv_pack_dims)
 *   bias     fp32 [cout_pad]
 *   ktab     int32 [k_pad/8][2] im2col table: {element offset (dy*w + dx)*x_cstride + c, dy<<16|dx}
 *            for every 8-channel chunk (built by ymi_conv_build_ktab); entries past K are {0,-1}
 *   y        NHWC view (n,ho,wo,cout) with pixel stride y_cstride, dtype out_dtype (dtype or F32)
 *   res      optional residual view, same shape as y, dtype `dtype` (NULL = none); added AFTER act
 *            (not combinable with y2)
 * ---------------------------------------------------------------------------------------- */
typedef struct ymi_conv_desc {
    const void* x;
    const void* w;
    const float* bias;
    const int32_t* ktab;
    void* y;
    const void* res;
    int32_t n, h, w_in, cin, x_cstride;
    int32_t ho, wo, cout, cout_pad, y_cstride, res_cstride;
    int32_t kh, kw, sh, sw, ph, pw, k_pad;
    int32_t act, dtype, out_dtype;
    int32_t tile; /* 0 = auto, else forces a tile configuration (tuning / tests) */
    /* optional second output: output channels [cout_split, cout) go to view y2 (channel 0 of y2 =
     * channel cout_split); lets one launch serve two consumers of the same input (C3.cv1 + C3.cv2,
     * reference common.py:172-173).  cout_split == 0 disables; must be a multiple of 8. */
    void* y2;
    int32_t y2_cstride, cout_split;
    /* y2_mode 0: channel split as above.  y2_mode 1 (cout_split must be 0, cout % 32 == 0, output of the compute dtype): y2 is an
     * (n, 2*ho, 2*wo) view that receives ALL output channels nearest-neighbour upsampled x2, in addition to y --
     * the nn.Upsample(scale_factor=2) of path_aggregation_network.py:221-223 folded into its producer's epilogue. */
    int32_t y2_mode, reserved0;
    /* optional CHAINED 1x1 convolution (Bottleneck.cv1 after C3.cv1, reference common.py:115,172): with K1 = cout_split
     * (or cout when there is no split) a second fused conv t = SiLU(chain_w * y[:, 0:K1] + chain_bias) is evaluated in
     * the epilogue from the freshly rounded outputs still in registers -- one launch instead of two and no re-read of y.
     * chain_w: packed [round_up(chain_cout,128)][K1] like w (K1 in {32, 64, 128}), chain_bias fp32 [chain_cout],
     * chain_y an (n, ho, wo) view of chain_cout channels (chain_cout % 32 == 0, <= 128).  Needs act SILU, a 16-bit
     * output and a tile whose cout width equals K1 (auto tile selection takes care of it); NULL disables. */
    const void* chain_w;
    const float* chain_bias;
    void* chain_y;
    int32_t chain_cout, chain_y_cstride;
    /* chained conv over a CONCAT (C3.cv3 after the last Bottleneck, common.py:173): its input channels are the K1 fresh
     * outputs followed by chain_k2 channels read from the (n, ho, wo) view chain_x2 (the other half of the concat buffer);
     * chain_w rows then hold K1 + chain_k2 weights.  chain_k2 % 16 == 0, <= 128; 0 / NULL = fresh outputs only.  With a
     * second source the producing conv may carry a residual and may be a 3x3 (LDS-halo variants with pixel-major waves). */
    const void* chain_x2;
    int32_t chain_x2_cstride, chain_k2;
    /* >= 256 readable zero bytes in device memory within +-4 GiB of x (e.g. the tail of x's own
     * buffer): source of out-of-image / out-of-range activation chunks for the direct-to-LDS loads of
     * the pipelined kernel, which also requires the packed weight ROWS to be zero-padded to a
     * multiple of 128 (NULL selects the register-staged kernel, which needs neither) */
    const void* zeros;
} ymi_conv_desc;

int ymi_conv2d(const ymi_conv_desc* d, void* stream);
/* fills host array ktab[k_pad/8][2] for the geometry in d (x_cstride, w_in, cin, kh, kw) */
int ymi_conv_build_ktab(int cin, int kh, int kw, int w_in, int x_cstride, int k_pad, int32_t* ktab_host);
/* fp32 mode (dtype = out_dtype = YMI_F32: fp32 activations and weights, exact fp32 arithmetic on the f32-input MFMA -- the
 * arithmetic of the reference's CPU path, common.py:69-70 run in torch.float32): the tile ymi_conv2d takes for tile == 0,
 * a function of (n*ho*wo, cout_pad) only, so every process sums in the same order.  Tiles 201-206 are the LDS-DMA
 * pipelined kernels (need desc.zeros); a negative tile id selects the register-staged kernel of rounds 2-4. */
int ymi_conv_f32_pick_tile(int m_pixels, int cout_pad);

/* ------------------------------------------------------------------------------------------
 * A whole C3 block in one launch: y = cv3(cat(m(cv1(x)), cv2(x))), m = Bottleneck(s)
 * x1 + cv2(cv1(x1)) -- yolort/v5/models/common.py:172-173 (C3.forward) with :115-116
 * (Bottleneck.forward) inlined, every Conv being :69-70 with BatchNorm folded into W/bias.
 * Intermediates never reach memory; results are bit-identical to the separate ymi_conv2d launches.
 * Two instances:
 *   (1) c_in = 64, c_hidden = 32, c_out = 64, one shortcut Bottleneck (yolov5s backbone.body.2): resident weights,
 *       csrc/c3_fused32.hip; wblob = NULL, mode = 0.
 *   (2) ABI 6 -- c_hidden = 64 or 128, c_out = 2 * c_hidden, c_in % 32 == 0: the strip kernel of csrc/c3_tile.hip (strips of whole rows where a
 *       row fits the LDS patch -- 80 x 80 / 40 x 40 of yolov5s --, column tiles with a halo column either side on wider maps; ymi_c3_tile_supported says),
 *       weights streamed in MFMA fragment order from `wblob` (ymi_c3_blob_bytes / ymi_c3_pack build it from w12 .. b3).
 *       A C3 with n > 1 Bottlenecks is a chain of launches over the same descriptor fields (`mode`):
 *         0  whole block, one Bottleneck:   x -> y
 *         1  HEAD  cv1 | cv2 + Bottleneck 0:   x -> y1_out (the Bottleneck's output), y2 (cv2(x))
 *         2  MID   one Bottleneck:             y1_in -> y1_out     (wm1 / wm2 = THAT Bottleneck's weights; never in place)
 *         3  TAIL  last Bottleneck + cv3:      y1_in, y2 -> y
 * Anything else returns YMI_EINVAL.  The Python side emits (1) since round 3 and (2) since round 6
 * (YOLORT_AMD_FUSE_C3=0 / YOLORT_AMD_C3_TILE=0 restore the separate launches).
 *   x / y       NHWC views (n,h,w,c_in) / (n,h,w,c_out), 16-bit, pixel strides x_cstride / y_cstride
 *   w12, b12    cv1 and cv2 stacked along cout: packed [>= 2*c_hidden][k12_pad] like ymi_conv_desc.w
 *               (rows 0..c_hidden-1 = cv1), fp32 bias [2*c_hidden]
 *   wm1, bm1    Bottleneck.cv1 (1x1, c_hidden -> c_hidden);  wm2, bm2  Bottleneck.cv2 (3x3 pad 1,
 *               k = (ky*3 + kx)*c_hidden + c);  w3, b3  cv3 (1x1, 2*c_hidden -> c_out)
 *   shortcut    1: the Bottleneck adds its input (common.py:116 `self.add`)
 * ---------------------------------------------------------------------------------------- */
typedef struct ymi_c3_desc {
    const void* x;
    void* y;
    const void* w12;
    const float* b12;
    const void* wm1;
    const float* bm1;
    const void* wm2;
    const float* bm2;
    const void* w3;
    const float* b3;
    int32_t n, h, w, x_cstride, y_cstride, dtype;
    int32_t c_in, c_hidden, c_out, n_bottlenecks, shortcut;
    int32_t k12_pad, km1_pad, km2_pad, k3_pad;
    int32_t mode;            /* ABI 6 (was reserved0): 0 whole block, 1 HEAD, 2 MID, 3 TAIL */
    /* ABI 6 */
    const void* wblob;       /* instance (2): ymi_c3_pack's weight stream for THIS mode (device memory, 16-byte aligned); NULL for instance (1) */
    const void* y1_in;       /* modes 2, 3: (n,h,w,c_hidden) view, the Bottleneck's input */
    void* y1_out;            /* modes 1, 2: (n,h,w,c_hidden) view, the Bottleneck's output */
    void* y2;                /* mode 1: cv2(x) is written here; mode 3: read from here; (n,h,w,c_hidden) view */
    int32_t y1_in_cstride, y1_out_cstride, y2_cstride, reserved1;
} ymi_c3_desc;

int ymi_c3_fused(const ymi_c3_desc* d, void* stream);
/* instance (2): size of / builder for the fragment-ordered weight stream of descriptor d's (c_in, c_hidden, mode); reads w12 .. b3 (device
 * pointers, the ymi_conv_desc.w layout) and writes `blob` on `stream`.  Weights that a mode does not use (w12 in modes 2 / 3, w3 in 1 / 2) may be NULL. */
int64_t ymi_c3_blob_bytes(const ymi_c3_desc* d);
int ymi_c3_pack(const ymi_c3_desc* d, void* blob, void* stream);
/* 1 when a strip geometry exists for (n, h, w, c_hidden) of d, i.e. ymi_c3_fused would take instance (2) for it */
int ymi_c3_tile_supported(const ymi_c3_desc* d);
/* ... and which one: out6 = {rows per strip R, slot origin delta, column tiles per row band, output columns per tile, patch slots, tiles}; returns 0 (out6 untouched) when
 * none exists.  Column tiles == 1: full-width strips (the rows of the patch share one pad slot); > 1: maps wider than the patch holds, a halo column either side of a tile. */
int ymi_c3_tile_geometry(const ymi_c3_desc* d, int* out6);

/* ------------------------------------------------------------------------------------------
 * SPP max-pool pyramid: given x = channels [0,c) of a (n,h,w,4c) concat buffer, writes
 * maxpool5(x), maxpool9(x), maxpool13(x) (stride 1, "same", -inf padding) into channel slices
 * [c,2c) [2c,3c) [3c,4c).  Replaces common.py:183-187 (SPP.forward: cat([x]+[m(x) for m in self.m])).
 * ---------------------------------------------------------------------------------------- */
int ymi_spp_pool(void* buf, int n, int h, int w, int c, int cstride, int dtype, void* stream);

/* nearest x2 upsample of view x (n,h,w,c) into view y (n,2h,2w,c) -- nn.Upsample(scale_factor=2),
 * yolort/models/path_aggregation_network.py:123,131,134 -- written straight into its concat slot. */
int ymi_upsample2x(const void* x, int x_cstride, int n, int h, int w, int c, void* y, int y_cstride,
                   int dtype, void* stream);
/* y <- act(y) (+ res) in place over the view (npix, c): the legacy r3.1 activations YMI_ACT_HARDSWISH (common.py:64-65) / YMI_ACT_LEAKY (LeakyReLU(0.1), common.py:140)
 * after a convolution run with YMI_ACT_NONE; `res`: the Bottleneck shortcut, added after the activation (common.py:115-116).  c and the strides in multiples of one
 * 16-byte packet (8 halves / 4 floats). */
int ymi_act(void* y, int y_cstride, int npix, int c, int dtype, int act, const void* res, int res_cstride, void* stream);
/* strided channel-slice copy (only used where a producer cannot write into its concat slot) */
int ymi_copy_view(const void* x, int x_cstride, int npix, int c, void* y, int y_cstride, int dtype,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Post-process (yolort/models/box_head.py:328-360,414-427 + torchvision batched_nms).
 * ymi_postprocess runs, on `stream`, with no host sync:
 *   1. decode   sigmoid, xy=(s*2-0.5+grid)*stride, wh=(s*2)^2*anchor (yolort/models/_utils.py:59-60,
 *               grids/shifts of anchor_utils.py in closed form), score = cls*obj (box_head.py:357),
 *               strict threshold score > score_thresh over ALL (anchor,class) pairs (box_head.py:418)
 *   2. sort     candidates per image by score descending, ties by candidate index (anchor asc,
 *               class asc) -- the stable order of torchvision.ops.nms
 *   3. nms      class-aware greedy suppression, IoU > nms_thresh strict, fp32 (box_head.py:422)
 *   4. top-k    first detections_per_img kept (box_head.py:424) and box rescale to the original
 *               image (yolort/models/transform.py:354-367 scale_coords, no clipping)
 * Inputs: logits[l] = fp32 NHWC (n, H_l, W_l, lcstride) with channel a*K + k (K = num_classes+5).
 * Outputs (fixed slab, the reference TensorRT wire format of relay/trt_graphsurgeon.py:223-244):
 *   out_boxes (n, K, 4) fp32, out_scores (n, K) fp32, out_labels (n, K) int64, out_count (n) int32.
 * Workspace: `ws` of `ws_bytes` bytes (query with ymi_postprocess_ws_bytes); candidate capacity
 * `cand_cap` is the batch-wide maximum number of (anchor,class) candidates; on overflow nothing is
 * truncated silently: the needed count is left in status[0] and status[1] is set to 1.
 * ---------------------------------------------------------------------------------------- */
#define YMI_MAX_LEVELS 4
typedef struct ymi_post_desc {
    const float* logits[YMI_MAX_LEVELS];
    int32_t lh[YMI_MAX_LEVELS], lw[YMI_MAX_LEVELS], lcstride[YMI_MAX_LEVELS];
    float stride[YMI_MAX_LEVELS];
    float anchors[YMI_MAX_LEVELS][6]; /* 3 anchors x (w,h) in pixels */
    int32_t num_levels, n, num_classes;   /* n: images of the batch, at most 1024 (the ranking kernel's per-block table; larger batches are refused, not truncated) */
    float score_thresh, nms_thresh;
    int32_t detections_per_img;
    /* per-image rescale (transform.py:358-367): box = (box - pad) / gain; gain<=0 disables */
    const float* rescale; /* device (n,3) {gain, pad_x, pad_y} or NULL */
    float* out_boxes;
    float* out_scores;
    int64_t* out_labels;
    int32_t* out_count;
    int32_t* status; /* device int32[8] (ABI 5; was int32[4]): {records sorted (after the score-prefix selection), overflow bits, segments, largest raw
                      * per-image count on overflow, RAW candidates of the batch (every (anchor, class) pair above the threshold), blocks of the last
                      * kernel done, reserved x2} */
    void* ws;
    int64_t ws_bytes;
    int32_t cand_cap;
    int32_t flags; /* YMI_POST_* bits */
    /* ABI 5: optional packed WIRE SLAB (n, 6 * detections_per_img + 1) fp32, written by the top-k kernel itself next to the four output arrays: per image
     * [boxes 4K | scores K | labels K as float | count], slots past the count zeroed -- the fixed-shape format one all-gather per batch carries between
     * ranks (the reference's TensorRT wire format, relay/trt_graphsurgeon.py:223-244, in one buffer).  When the batch has to be re-run by the caller
     * (status[1] != 0: candidate capacity / score prefix) the LAST block of the kernel overwrites every row's count column with -1 (YMI_SLAB_STALE), so
     * the receivers of a collective enqueued right behind the post-process learn it from the data.  NULL: not written. */
    float* out_slab;
} ymi_post_desc;
#define YMI_SLAB_STALE (-1.0f)

/* ymi_post_desc.flags.
 * By default an image with many candidates is post-processed on a score-ordered PREFIX of them (at least
 * max(4096, 4 * detections_per_img) records): greedy NMS decisions depend only on higher-scored boxes, so once
 * the prefix alone yields detections_per_img kept boxes the result equals the full computation exactly.  If a
 * truncated image ends with fewer kept boxes, bit 1 of status[1] is set and the caller re-runs the batch with
 * YMI_POST_EXACT_FULL (the Python host does this transparently). */
#define YMI_POST_EXACT_FULL 1
/* Best-class mode: ONE label per anchor -- the contract of ultralytics' non_max_suppression(..., multi_label=False) (yolort/v5/utils/general.py:572-583, what AutoShape
 * uses) instead of yolort's multi-label PostProcess.  Per anchor: s_c = cls_c * obj (the very fp32 product of the default mode), conf = max_c s_c, label = the lowest
 * class index with s_c == conf (torch.max(1)); the anchor is a candidate iff conf > score_thresh (strict), so there are at most total_anchors records per image and
 * status[4] counts passing ANCHORS.  Sort (ties by anchor index), class-aware NMS, top-k, rescale, slab and status words are those of the default mode; with
 * num_classes == 1 the two modes are bit-identical; thresholds <= 0 keep their meaning (every anchor yields its best class).  Honoured by ymi_postprocess,
 * ymi_conv_head_decode, ymi_conv_head_decode_group, their ymi_plan_add_* forms and the replay of an exported plan (the descriptor travels with the plan).
 * Differences from ultralytics: the NMS is the true class-aware NMS of this library, not the 4096-pixel class offset; there is no max_nms = 30000 cut of the
 * candidates; scores stay fp32 (`agnostic=` is YMI_POST_AGNOSTIC, `classes=` is YMI_POST_CLASS_FILTER below). */
#define YMI_POST_BEST_CLASS 2
/* Class-agnostic NMS: ONE suppression over all candidates of an image, whatever their label -- ultralytics' non_max_suppression(..., agnostic=True), i.e.
 * torchvision.ops.nms on the unshifted boxes.  Combines with YMI_POST_BEST_CLASS and YMI_POST_EXACT_FULL.  Candidate generation (both modes), the sort (score
 * descending, ties by candidate index), top-k, rescale, slab, status words and the LABELS of the kept detections are unchanged; only the suppression changes: within
 * an image a candidate is suppressed by ANY kept higher-ranked candidate whose fp32 IoU with it is > nms_thresh (strict; NaN from 0/0 does not suppress).  In
 * multi-label mode the several classes of one anchor share a box (IoU 1), so only the best-scoring of them survives -- ultralytics behaves the same.  With
 * num_classes == 1 the flag changes nothing in the result.  The score-prefix protocol holds as it is (decisions depend on higher-scored boxes only); more
 * suppression makes YMI_STATUS_PREFIX_SHORT more frequent, and the re-run with YMI_POST_EXACT_FULL covers it.  Each image is walked by one workgroup
 * (nms_block_kernel, csrc/postprocess.hip).  Honoured wherever YMI_POST_BEST_CLASS is: ymi_postprocess, ymi_post_finish (the fused head's begin / finish), the
 * ymi_plan_add_* forms and the replay of an exported plan. */
#define YMI_POST_AGNOSTIC 4
/* Class filter: only detections of an allowed set of classes -- ultralytics' non_max_suppression(..., classes=[...]) (yolort/v5/utils/general.py:585-587: after the
 * candidates are generated, before NMS).  Combines with YMI_POST_EXACT_FULL, YMI_POST_BEST_CLASS and YMI_POST_AGNOSTIC.  The set is a bit set in the workspace
 * (uint32[128] at ymi_post_class_mask_offset: bit c & 31 of word c >> 5 set = class c allowed), written by ymi_post_set_classes / ymi_plan_set_classes or by the
 * consumer, and read by the candidate producers only -- so changing the SET needs no new descriptor, no re-record and no graph re-capture; only switching between
 * "no filter" and "filter" changes the flag.  The region is carved last (every other workspace offset is unchanged); ymi_post_begin never touches it, and a fresh
 * workspace holds no valid mask: write it before the first run.
 *   multi-label mode: an (anchor, class) pair is a candidate iff cls * obj > score_thresh (strict, as ever) AND the class is allowed.
 *   best-class mode:  the best class is taken over ALL classes exactly as without the filter; the anchor is a candidate iff that class passes the threshold AND is
 *                     allowed.  An anchor whose best class is not allowed yields nothing even if an allowed class passes (ultralytics filters after x[:, 5:].max(1)).
 *   agnostic:         the single suppression runs over the filtered candidates only (a box of an unwanted class suppresses nothing).
 * The empty set gives zero detections in every image; with num_classes == 1 the set {0} is bit-identical to no filter.  Records of allowed classes are bit-identical to
 * those of an unfiltered run; sort, NMS, top-k, rescale and slab are unchanged.  status[4] counts what was produced AFTER the filter (passing pairs of allowed classes /
 * passing anchors whose best class is allowed); the capacity and score-prefix protocols apply to the filtered records.  Honoured wherever YMI_POST_BEST_CLASS is:
 * ymi_postprocess, ymi_conv_head_decode, ymi_conv_head_decode_group, their ymi_plan_add_* forms and the replay of an exported plan. */
#define YMI_POST_CLASS_FILTER 8
/* Merge-NMS: every kept box becomes the score-weighted mean of the candidates it overlaps -- ultralytics' non_max_suppression with its local `merge = True`
 * (yolort/v5/utils/general.py:604-613).  Combines with YMI_POST_EXACT_FULL, YMI_POST_BEST_CLASS, YMI_POST_AGNOSTIC and YMI_POST_CLASS_FILTER.  Candidates, sort
 * and suppression (class-aware, or agnostic under YMI_POST_AGNOSTIC) are unchanged; per image, after the NMS:
 *   1. n = the image's candidate count (what the producers emitted for it after threshold, best-class mode and class filter).  The image is merged iff
 *      1 < n < YMI_MERGE_MAX_N (general.py:606); every other image comes out exactly as without the flag, bit for bit.  The score-prefix selection never cuts an
 *      image below 4096 records, so a merged image is never a truncated one and YMI_STATUS_PREFIX_SHORT keeps its protocol.
 *   2. The kept list is the first detections_per_img kept records in rank order, taken BEFORE the merge (general.py:604-605).
 *   3. The contributors of a kept record i are ALL candidates j of the image, kept or suppressed, i included, that carry its label (any label under
 *      YMI_POST_AGNOSTIC) and whose fp32 IoU with i is > nms_thresh (strict; the suppression's own expression, NaN never passes); m_i is their number.
 *   4. merged box = sum_j(score_j * box_j) / sum_j(score_j) per coordinate, in fp32 with every product, sum and the division rounded on its own (no fused
 *      multiply-add) over the unrescaled decoded boxes; the summation order is a fixed function of the candidates' ranks, so the result is the same on every
 *      run.  If the weight sum is not > 0 (all-zero scores under a non-positive score_thresh) the box keeps its NMS coordinates.  Score and label are unchanged.
 *   5. Without YMI_POST_MERGE_KEEP_SINGLE a kept record with m_i <= 1 -- a box nothing else agrees with, or a zero-area box whose IoU with itself is NaN -- is
 *      dropped (general.py:612-613, `redundant = True`); the survivors are compacted in rank order, slots are NOT refilled: out_count can be below
 *      detections_per_img although more boxes were kept, as in the reference.  With YMI_POST_MERGE_KEEP_SINGLE nothing is dropped.
 *   6. rescale ((b - pad) / gain) applies to the merged box; slab, zeroing past the count, YMI_SLAB_STALE and every status word are those of the default
 *      (status[4] still counts raw candidates).
 * YMI_POST_MERGE_KEEP_SINGLE is valid only together with YMI_POST_MERGE (alone: YMI_EINVAL).  One workgroup per image (merge_gather_kernel, csrc/postprocess.hip,
 * launched instead of the top-k gather; without the flag the launch sequence is unchanged).  Honoured wherever YMI_POST_AGNOSTIC is: ymi_postprocess,
 * ymi_post_finish (the fused head's begin / finish), the ymi_plan_add_* forms, the post-process graph and the replay of an exported plan; ymi_batched_nms and ymi_nms
 * return indices and are not affected.
 * Differences from ultralytics: the overlap test runs on the unshifted boxes of the same class, not on boxes offset by 4096 x class; there is no max_nms cut of
 * the candidates; a non-positive weight sum leaves the box as it is where the reference would emit NaN. */
#define YMI_POST_MERGE 16
#define YMI_POST_MERGE_KEEP_SINGLE 32
#define YMI_MERGE_MAX_N 3000 /* an image is merged iff 1 < candidates < YMI_MERGE_MAX_N */
#define YMI_STATUS_OVERFLOW_CAPACITY 1 /* status[1] bit 0: candidate capacity exceeded (grow cand_cap) */
#define YMI_STATUS_PREFIX_SHORT 2      /* status[1] bit 1: prefix too short, re-run with YMI_POST_EXACT_FULL */

/* Stem convolution fed straight from planar images (fixed-size streams): when every image of the batch already is the
 * (3, H, W) canvas -- the reference's resize is then the identity and batch_images pads nothing (transform.py:53-97,
 * 297-330) -- the letterbox pass and its NHWC4 round trip are skipped.  `d` is the stem in its super-pixel form exactly
 * as for ymi_conv2d (cin 8, 6x3, stride (2,1), pad (2,1), h = H, w_in = W/2; x is ignored), imgs[i] are device pointers
 * to contiguous (3, H, W) images of dtype d->dtype (16-byte aligned, W % 8 == 0).  Output is bit-identical to
 * ymi_letterbox + ymi_conv2d.  Replaces yolort/models/darknetv6.py:81 + common.py:69-70 on that input. */
int ymi_conv_stem_planar(const ymi_conv_desc* d, const void* const* imgs, int n_imgs, void* stream);

/* The first TWO layers of the r6.0 backbone in one launch, for the same fixed-size streams: `stem` as for ymi_conv_stem_planar
 * with 32 output channels (its y is not written), `body1` = Conv(32, 64, k=3, s=2, p=1) + BN + SiLU over the stem's output
 * (its x is not read) -- yolort/models/darknetv6.py:81 and :85-86 with common.py:69-70.  The stem's output, the largest
 * activation of the network, never reaches memory.  Output is bit-identical to ymi_conv_stem_planar + ymi_conv2d. */
int ymi_stem_body1_planar(const ymi_conv_desc* stem, const ymi_conv_desc* body1, const void* const* imgs, int n_imgs, void* stream);

/* The same pair fed from the letterboxed canvas (dynamic-shape streams: transform.py:53-97 resizes and pads first): `stem` exactly as
 * for ymi_conv2d on the NHWC4 canvas (x = ymi_letterbox's output, x_cstride 8), `body1` as above.  Bit-identical to two ymi_conv2d calls. */
int ymi_stem_body1(const ymi_conv_desc* stem, const ymi_conv_desc* body1, void* stream);

/* Measurement aid (bench.py): one wave spins for `spin_us` microseconds of the constant 100 MHz clock and writes
 * {shader-clock cycles, 100 MHz ticks} to out[0..1] (device memory) -- the shader clock the chip runs at while whatever else
 * is in flight on other streams executes.  Asynchronous on `stream`. */
int ymi_clock_probe(uint64_t* out, int spin_us, void* stream);

int64_t ymi_postprocess_ws_bytes(int n, int total_anchors, int cand_cap);
int ymi_postprocess(const ymi_post_desc* d, void* stream);

/* The same post-process in three stages, for the FUSED head (below):
 *   ymi_post_begin        resets the candidate counters of the descriptor's workspace
 *   <candidate producers> ymi_conv_head_decode once per pyramid level (any order, same or ordered streams)
 *   ymi_post_finish       sort + class-aware NMS + top-k + rescale from the appended records
 * ymi_postprocess == begin + decode of the fp32 logits + finish.  logits[] / lcstride[] are ignored by
 * begin / finish / ymi_conv_head_decode; lh / lw / stride / anchors describe the levels as before. */
int ymi_post_begin(const ymi_post_desc* d, void* stream);
int ymi_post_finish(const ymi_post_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Augmented inference (test-time augmentation): ultralytics' DetectionModel.forward(x, augment=True) -> _forward_augment
 * (yolort/v5/models/yolo.py:147-163), what AutoShape.forward(imgs, size, augment) exposes.  The letterboxed batch runs three
 * times -- scale 1, scale 0.83 mirrored left-right, scale 0.67 (ymi_scale_view makes the two smaller canvases) --, the
 * predictions of each view are brought back to the full canvas (_descale_pred, yolo.py:181-197), the views are concatenated
 * along the anchor axis without the "tails" (_clip_augmented, yolo.py:199-208) and ONE NMS runs over the union.
 *
 * ymi_post_decode_view is a candidate producer between ymi_post_begin and ymi_post_finish: decode_kernel's twin for ONE view.
 *   sink  an ordinary ymi_post_desc whose levels describe the CONCATENATED anchor axis of all views; begin / finish / this call
 *         use its geometry only for the anchor count A = sum 3 * lh * lw, so one pseudo-level of 1 x (A / 3) does (logits[],
 *         lcstride[], stride[] and anchors[] of the sink are ignored here).  Thresholds, num_classes, flags (best-class mode,
 *         class filter), capacity and workspace are the sink's: scores, the strict threshold, YMI_POST_BEST_CLASS and
 *         YMI_POST_CLASS_FILTER behave exactly as in ymi_postprocess.
 *   view  geometry, fp32 NHWC logits (n of the sink, channel a * K + k), strides and anchors of this view's pyramid, and
 *         skip_mask    bit l set: level l contributes nothing and occupies NO anchor indices (the clipped tail)
 *         anchor_base  index of the view's first kept anchor within an image of the sink; the kept levels follow each other from
 *                      there in level order, anchor index within a level = (a * lh + y) * lw + x as ever.  Records carry
 *                      anchor_base + index, so the sort's tie order is view-major, then anchor, then class -- torch.cat(y, 1)'s --
 *                      and the decoded box of every kept anchor is stored at that index.
 *         scale, flip_w  the decoded box (x1, y1, x2, y2) of ymi_postprocess's decode is mapped to the full canvas in explicitly
 *                      rounded fp32: y1' = y1 / scale, y2' = y2 / scale; flip_w == 0: x1' = x1 / scale, x2' = x2 / scale;
 *                      flip_w = W > 0 (the full canvas width, the view was mirrored): x1' = W - x2 / scale, x2' = W - x1 / scale.
 * Which levels to skip: view 0 every level but the coarsest, the last view every level but the finest, the others none --
 * since every view's sides are multiples of the largest stride this is exactly what _clip_augmented cuts, for 3 and 4 levels.
 * Differences from the reference: it applies / scale and W - x to the centre and the size (xywh) and converts to corners
 * afterwards; here the corners themselves are divided and mirrored -- the two differ in rounding only (a few fp32 ulps of the
 * coordinate).  The NMS is this library's (true class-aware, no 4096-pixel class offset, no max_nms cut), as for every mode above.
 * The view must cover the sink's range: anchor_base + kept anchors <= A, else YMI_EINVAL.  ABI stays 6: a new struct and new
 * functions only, no existing struct changed -- a caller built against the previous header keeps working.
 * ---------------------------------------------------------------------------------------- */
typedef struct ymi_post_view {
    const float* logits[YMI_MAX_LEVELS];
    int32_t lh[YMI_MAX_LEVELS], lw[YMI_MAX_LEVELS], lcstride[YMI_MAX_LEVELS];
    float stride[YMI_MAX_LEVELS];
    float anchors[YMI_MAX_LEVELS][6];
    int32_t num_levels;
    int32_t skip_mask;
    int32_t anchor_base;
    float scale;
    int32_t flip_w;
    int32_t reserved;
} ymi_post_view;
int ymi_post_decode_view(const ymi_post_desc* sink, const ymi_post_view* view, void* stream);

/* YMI_POST_CLASS_FILTER: byte offset of the class mask (uint32[128], 256-byte aligned) inside a workspace of ymi_postprocess_ws_bytes(n, total_anchors, cand_cap)
 * bytes, for consumers who write the mask themselves; negative for arguments that have no workspace. */
int64_t ymi_post_class_mask_offset(int n, int total_anchors, int cand_cap);
/* writes the mask of descriptor d's workspace on `stream`: classes[0 .. count) are the allowed class indices (any order, duplicates allowed, count == 0 = the empty
 * set), each 0 <= c < d->num_classes, else YMI_EINVAL and nothing is written.  The list is consumed before the call returns (the words travel by value in a kernel
 * argument), the write is ordered on `stream` like any launch and may be captured.  YMI_EINVAL when d->flags lacks YMI_POST_CLASS_FILTER. */
int ymi_post_set_classes(const ymi_post_desc* d, const int32_t* classes, int count, void* stream);

/* Detection head of pyramid level `level` (the biased 1x1 conv of yolort/models/box_head.py:36,74) with the
 * decode + sigmoid + multi-label threshold of box_head.py:345-360,414-418 and _utils.py:59-60 fused into the
 * convolution's epilogue: the fp32 logits never reach memory, boxes of every anchor and the candidate records go
 * straight into `post`'s workspace (bit-identical to what ymi_postprocess derives from stored logits).
 * conv: 1x1 stride 1, cin % 32 == 0, k_pad == cin, act NONE, zeros required, y ignored.  Weight rows / bias are
 * packed per anchor: anchor q's K = num_classes + 5 outputs occupy rows q*RA .. q*RA+K-1, RA = round_up(K, 32)
 * (<= 128), remaining rows zero; cout = cout_pad = 3*RA. */
int ymi_conv_head_decode(const ymi_conv_desc* conv, const ymi_post_desc* post, int level, void* stream);
/* the heads of ALL pyramid levels in one launch (convs[l] = level l, same dtype and class count): the levels are
 * independent and the coarse ones have few blocks, so one grouped launch fills the chip where three back-to-back
 * launches leave it mostly idle.  Same records as the per-level calls. */
int ymi_conv_head_decode_group(const ymi_conv_desc* convs, int n_levels, const ymi_post_desc* post, void* stream);

/* Stand-alone class-aware NMS on caller-provided candidates of ONE image (kept indices in
 * score-descending stable order, like torchvision.ops.batched_nms called at box_head.py:422).
 * boxes (n,4) fp32 xyxy, scores (n) fp32, labels (n) int32; keep_out (n) int32, count_out int32[1].
 * Scores may be any non-NaN floats (negative, +-0 -- a tie --, +-inf, subnormal); NaN scores / coordinates are outside
 * the contract.  n < 2^20. */
int64_t ymi_nms_ws_bytes(int n);
int ymi_batched_nms(const float* boxes, const float* scores, const int32_t* labels, int n, float nms_thresh,
                    int32_t* keep_out, int32_t* count_out, void* ws, int64_t ws_bytes, void* stream);
/* Stand-alone class-AGNOSTIC NMS of one image: torchvision.ops.nms -- ymi_batched_nms with every label equal, without the label array and the label sort, and with one
 * workgroup instead of one wave walking the candidates.  Same buffers, same score contract (any non-NaN float, +-0 tie, n < 2^20), same workspace (ymi_nms_ws_bytes). */
int ymi_nms(const float* boxes, const float* scores, int n, float nms_thresh, int32_t* keep_out, int32_t* count_out, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * COCO matching on the device: the greedy detection <-> ground-truth matching of the COCO detection protocol (pycocotools COCOeval.evaluateImg, restated on the host by
 * yolort_amd/utils/metrics.py coco_ap) for the detection slab, one launch for every (image, class, area range, IoU threshold).  Only the matching runs here: the
 * caller sorts the flags by score and accumulates precision / recall on the host (metrics.py GpuDetectionEvaluator).
 * Inputs (device, read-only): the slab boxes (n, k, 4) fp32 xyxy, scores (n, k) fp32, labels (n, k) int64, counts (n) int32 -- what the top-k kernel writes and the
 * ranks all-gather --; ground truth gt_boxes (n, g, 4) fp32 xyxy, gt_labels (n, g) int32, gt_counts (n) int32 (negative counts as 0).  Slots at or past a count are
 * never read; a counts[i] above k or a gt_counts[i] above g is taken as k / g (the slab holds no more) without a status bit.  Scores may be ANY fp32 values: negative,
 * +-0 (a tie), +-inf, subnormal, and NaN, which sorts behind every number, in slab order among NaNs -- the total order of the host's stable argsort of -score.  Box
 * coordinates must not be NaN: a NaN IoU never matches here, while the host loop's `iou < best` is false for it and takes the ground truth.  In the descriptor itself: thrs[num_thrs <= YMI_EVAL_MAX_THRS] IoU thresholds, each in (0, 1]; area_rng[num_rngs <= YMI_EVAL_MAX_RNGS] = {lo, hi};
 * max_dets (0: no cut); num_classes (<= 4096).  k, g <= YMI_EVAL_MAX_PER_IMAGE; anything larger is refused with YMI_EINVAL, not truncated.
 * Per (image, class, range r, threshold t):
 *   - the detections of the class are ordered by score descending, equal scores (-0.0 == +0.0) in slab order, NaN last (a stable sort; the slab need not be sorted); only the
 *     first max_dets of each (image, class) take part (COCO's maxDets, per category as pycocotools applies it);
 *   - a ground truth is IGNORED in range r when its area (x2 - x1) * (y2 - y1) (fp32) is < lo or > hi; ground truths are walked non-ignored first, each group in input
 *     order ({-inf, +inf} ignores nothing: the evaluator's "all" range);
 *   - IoU = inter / (((area_d + area_g) - inter) + 1e-12f), inter = max(x2 - x1, 0) * max(y2 - y1, 0) of the intersection, every operation a rounded fp32 one and the
 *     division correctly rounded (zero-area pairs give 0, inverted boxes a negative IoU that never matches);
 *   - each detection, in score order, takes the still unused ground truth of the largest IoU among those with (double)IoU >= min(t, 1 - 1e-10); among equal IoUs the
 *     one walked LAST wins; ignored ground truth is looked at only if no non-ignored one qualified;
 *   - tp = matched a non-ignored ground truth; ig = matched an ignored one or, unmatched, the detection's own area is outside the range.
 * Outputs (device): tp, ig (num_rngs, n, k) uint16 with bit t per threshold, written for EVERY slot below the image's count (0 for a slot that takes no part) and for
 * no other; rank (n, k) int32 = the detection's position in its (image, class) score order, -1 when cut by max_dets or skipped, slots at or past the count untouched;
 * n_gt (num_rngs, num_classes) int32 = non-ignored ground truths per class ADDED to what the buffer holds (integer atomics: the caller zeroes it once and
 * accumulates over launches), images without detections included; status int32[4], of which the kernel only ever ORs bits into status[1] (the caller zeroes it):
 * YMI_EVAL_STATUS_BAD_LABEL when a label below a count is outside [0, num_classes) -- that detection (rank -1, flags 0) or ground truth is skipped --,
 * YMI_EVAL_STATUS_STALE_ROW when a counts[i] is negative (a stale slab row, YMI_SLAB_STALE) -- that image is skipped altogether, its ground truth included.
 * One workgroup per (image, range) (eval_match_kernel, csrc/postprocess.hip); no workspace; the launch is ordered on `stream`, synchronises nothing and may be captured.
 * Differences from pycocotools (those of metrics.py): no crowd (iscrowd) ground truth, the 1e-12 in the IoU denominator, areas from the boxes.  ABI stays 6: a new
 * struct and a new function. */
#define YMI_EVAL_MAX_THRS 16
#define YMI_EVAL_MAX_RNGS 4
#define YMI_EVAL_MAX_PER_IMAGE 1024
#define YMI_EVAL_STATUS_BAD_LABEL 1 /* status[1] bit 0 */
#define YMI_EVAL_STATUS_STALE_ROW 2 /* status[1] bit 1 */
typedef struct ymi_eval_desc {
    const float* boxes;
    const float* scores;
    const int64_t* labels;
    const int32_t* counts;
    const float* gt_boxes;
    const int32_t* gt_labels;
    const int32_t* gt_counts;
    uint16_t* tp;
    uint16_t* ig;
    int32_t* rank;
    int32_t* n_gt;
    int32_t* status;
    double thrs[YMI_EVAL_MAX_THRS];
    float area_rng[YMI_EVAL_MAX_RNGS][2];
    int32_t n, k, g;
    int32_t num_thrs, num_rngs;
    int32_t max_dets, num_classes;
    int32_t reserved;
} ymi_eval_desc;
int ymi_eval_match(const ymi_eval_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Plan: a recorded sequence of the launches above for one (arch, N, H, W, dtype), replayed with a
 * single call (and optionally captured into a hipGraph).  Replaces the Python module-by-module
 * dispatch of yolort/models/yolo.py:159-175.  The plan copies descriptors; buffers stay owned by
 * the caller and must outlive the plan.
 * ---------------------------------------------------------------------------------------- */
typedef struct ymi_plan ymi_plan;
ymi_plan* ymi_plan_create(void);
void ymi_plan_destroy(ymi_plan* p);
int ymi_plan_add_conv(ymi_plan* p, const ymi_conv_desc* d);
int ymi_plan_add_c3_fused(ymi_plan* p, const ymi_c3_desc* d);
int ymi_plan_add_spp_pool(ymi_plan* p, void* buf, int n, int h, int w, int c, int cstride, int dtype);
int ymi_plan_add_upsample2x(ymi_plan* p, const void* x, int x_cstride, int n, int h, int w, int c, void* y,
                            int y_cstride, int dtype);
int ymi_plan_add_copy_view(ymi_plan* p, const void* x, int x_cstride, int npix, int c, void* y,
                           int y_cstride, int dtype);
int ymi_plan_add_act(ymi_plan* p, void* y, int y_cstride, int npix, int c, int dtype, int act, const void* res, int res_cstride);
int ymi_plan_add_postprocess(ymi_plan* p, const ymi_post_desc* d);
int ymi_plan_add_post_begin(ymi_plan* p, const ymi_post_desc* d);
int ymi_plan_add_head_decode(ymi_plan* p, const ymi_conv_desc* conv, const ymi_post_desc* d, int level);
int ymi_plan_add_head_decode_group(ymi_plan* p, const ymi_conv_desc* convs, int n_levels, const ymi_post_desc* d);
int ymi_plan_add_post_finish(ymi_plan* p, const ymi_post_desc* d);
/* augmented inference: ymi_scale_view / ymi_post_decode_view as recorded ops (the view's candidates belong to the post-process of `sink`:
 * ymi_plan_set_classes writes that workspace's mask once, and an exported plan carries both descriptors) */
int ymi_plan_add_scale_view(ymi_plan* p, const void* src, int n, int h, int w, void* dst, int dh, int dw, int sh, int sw, int flip, int dtype);
int ymi_plan_add_post_decode_view(ymi_plan* p, const ymi_post_desc* sink, const ymi_post_view* view);
int ymi_plan_num_ops(const ymi_plan* p);
/* ymi_post_set_classes for every post-process descriptor recorded in the plan that carries YMI_POST_CLASS_FILTER (YMI_EINVAL if none does).  The plan remembers the
 * list: ymi_plan_export stores it, and ymi_plan_import writes the masks again before it returns, so an imported plan filters as the exporting one did; the consumer
 * changes the set later with this call.  A plan exported without a list imports with the empty set (its workspace is zero-filled).  ymi_plan_import has no stream
 * of the caller's: it writes the masks on the NULL (legacy default) stream and calls hipStreamSynchronize on it before it returns -- a consumer whose other threads
 * use blocking streams sees that synchronisation; streams created with hipStreamNonBlocking are not waited for. */
int ymi_plan_set_classes(ymi_plan* p, const int32_t* classes, int count, void* stream);
/* on != 0: ops 0 and 1 (the stem over the letterboxed canvas and body.1 reading its output, see ymi_stem_body1) run as ONE launch whenever a
 * run covers both; op indices are unchanged, the stem's output buffer is then not written.  Fails unless ops 0 and 1 are such a pair. */
int ymi_plan_set_fuse_stem(ymi_plan* p, int on);
/* runs ops [first, last) on stream (last < 0 = all); use_graph != 0 replays a captured hipGraph */
int ymi_plan_run(ymi_plan* p, int first, int last, int use_graph, void* stream);
/* ---- one batch of a serving loop in two calls (the host side of yolo.py:141-183 per batch: YOLO._acquire / _submit_entry) ----
 * ymi_plan_begin: the next batch's inputs were produced on `caller_stream`; `main_stream` (the stream this plan instance launches its conv stack on) waits for
 *   them and for the plan's previous batch to have drained (its buffers are about to be overwritten).  No host synchronisation.
 * ymi_plan_submit: ops [first, n_conv) on `main_stream` (hipGraph replay when use_graph & 1), then ops [n_conv, end) -- the post-process -- on `side_stream`
 *   behind them (a second captured graph when use_graph & 2; a plan keeps two captured ranges), then `result_bytes` of `dev_result` copied to the PINNED `host_result` on `side_stream`, then the plan's completion event.  main_waits_done != 0
 *   additionally makes `main_stream` wait for that event (one batch in flight).  Neither call synchronises the host or allocates after the first use.
 * ymi_plan_done_query: 1 = the last submitted batch has completed (or none was submitted), 0 = still running.  ymi_plan_done_sync blocks the host on it. */
int ymi_plan_begin(ymi_plan* p, void* caller_stream, void* main_stream);
int ymi_plan_submit(ymi_plan* p, int first, int n_conv, int use_graph, void* main_stream, void* side_stream, const void* dev_result, void* host_result,
                    size_t result_bytes, int main_waits_done);
int ymi_plan_done_query(ymi_plan* p);
int ymi_plan_done_sync(ymi_plan* p);

/* ------------------------------------------------------------------------------------------
 * ABI 6 -- plan export / import: a recorded plan as a self-contained file, for consumers without Python (the role the
 * reference's TorchScript / ONNX artefacts of yolort/relay + yolort/runtime play).
 *   ymi_plan_export   `regions` lists every device allocation the plan's descriptors point into (base, bytes):
 *                     YMI_REGION_CONST  contents are saved (packed weights, biases, im2col tables, weight streams)
 *                     YMI_REGION_SCRATCH zero-filled at import (activation buffers with their zero tails, workspaces)
 *                     YMI_REGION_IO     zero-filled at import; the consumer finds it by `tag` (YMI_TAG_*)
 *                     Every non-NULL pointer of every recorded op must lie inside one region (else YMI_EINVAL, the op and
 *                     field named in ymi_last_error).  Synchronises `stream` and reads the constant regions back.
 *   ymi_plan_import   allocates the regions (hipMalloc), uploads the constants, rebuilds the ops; the plan owns the
 *                     memory (ymi_plan_destroy frees it).  regions_out[0 .. min(n, max_regions)) receives the new
 *                     bases with the sizes / kinds / tags of the file.  Run with ymi_plan_run as usual.
 * The file is tied to the ABI version and build it was written by (descriptor layouts, tile ids).
 * ---------------------------------------------------------------------------------------- */
#define YMI_REGION_CONST 1
#define YMI_REGION_SCRATCH 2
#define YMI_REGION_IO 3
#define YMI_TAG_NONE 0
#define YMI_TAG_INPUT 1      /* the letterboxed batch: NHWC4 canvas (n, h, w, 4) of the compute dtype, channel 3 zero (ymi_letterbox writes it) */
#define YMI_TAG_RESCALE 2    /* ymi_post_desc.rescale: fp32 (n, 3) {gain, pad_x, pad_y} per image, written by the consumer per batch (zeros: boxes stay in canvas coordinates) */
#define YMI_TAG_BOXES 3      /* fp32 (n, K, 4) */
#define YMI_TAG_SCORES 4     /* fp32 (n, K) */
#define YMI_TAG_LABELS 5     /* int64 (n, K) */
#define YMI_TAG_STATUS_COUNT 6 /* int32 [8 status words | n counts] (ymi_post_desc.status / out_count share it) */
#define YMI_TAG_SLAB 7       /* fp32 (n, 6K + 1) wire slab */
typedef struct ymi_plan_region {
    const void* base;
    int64_t bytes;
    int32_t kind, tag;
} ymi_plan_region;
int ymi_plan_export(const ymi_plan* p, const ymi_plan_region* regions, int n_regions, const char* path, void* stream);
int ymi_plan_import(const char* path, ymi_plan** out_plan, ymi_plan_region* regions_out, int max_regions, int* n_regions_out);
/* per-op timing with HIP events on `stream`: ms_out[num_ops], averaged over iters */
int ymi_plan_profile(ymi_plan* p, int iters, float* ms_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLORT_AMD_H */
