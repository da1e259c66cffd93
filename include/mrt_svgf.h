/* mrt_svgf.h — variance-guided filtering of accumulated path frames (SVGF, Schied et al. 2017), on
 * the device: the temporal accumulation of mrt_temporal.h with the luminance moments carried
 * along, and an a-trous filter whose colour weight is scaled by each pixel's own variance.
 *
 * The stream-taking exports of mrt.h are a closed table; these two live in a
 * header of their own with a table of their own (tests/test_svgf_table.py,
 * tests/test_gpu_svgf_stream.py) and keep the same promises: every launch goes to `stream` (a
 * hipStream_t, NULL = the null stream), nothing waits on the host, nothing is read back and nothing
 * is allocated. Error codes and MRT_OK are mrt.h's. All pointers are device pointers on the calling
 * thread's current device. The CPU statements are mrth_svgf_accumulate and mrth_svgf_filter
 * (mrt_host.h).
 *
 * All arithmetic is float32, one IEEE operation at a time in the order written here, with no fused
 * multiply-add, no flushed denormal, correctly rounded `/` and no libm call but floorf, which is
 * exact. Every weight is rational: there is no exp, no sqrt and no pow.
 *   dot(a, b) = ((0 + a.x * b.x) + a.y * b.y) + a.z * b.z
 *   lum(c)    = dot((0.2126f, 0.7152f, 0.0722f), c.rgb)
 *   pos(x)    = (x > 0) ? x : 0, so a NaN gives 0
 * Host and device agree bit for bit; only the bits of a NaN that an operation makes differ. */
#ifndef MRT_SVGF_H
#define MRT_SVGF_H

#include <stdint.h>

#include "mrt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mrt_svgf_accumulate: mrt_temporal_accumulate with the luminance moments carried along, in one
 * launch. The first 19 fields are mrt_temporal_params' with the same meaning; steps 1-5 are
 * mrt_temporal_accumulate's, word for word, so history, imageOut and pixels equal that export's bit
 * for bit on every input. moments and prevMoments hold 4 floats per pixel: (m1, m2, 0, N), the
 * running means of the demodulated luminance and of its square, and the history length.
 * In addition, with c the current colour of step 1 (at a miss: the image) and
 *     l = lum(c),  l2 = l * l:
 *  - At a miss, with havePrev == 0, and wherever step 3 finds no history:
 *         moments[p] = (l, l2, 0, 1).
 *  - Where step 3 finds a history: over the same taps in the same order, with the same bw and the
 *    same wsum,
 *         hm = sum / wsum per channel, sum += bw * prevMoments[q] (a multiply, then an add)
 *         moments[p] = (hm.x + (l - hm.x) * alpha, hm.y + (l2 - hm.y) * alpha, 0, N)
 *    with step 3's alpha and N (a subtract, a multiply, an add), so moments[p].w == history[p].w.
 * prevMoments is ignored, and may be NULL, where havePrev == 0.
 * Launch shapes and variant are mrt_temporal_accumulate's (variant 0: the linear shape).
 * Checks, in this order, nothing written where one fails: NULL params; the scalar checks and limits
 * of mrt_temporal_accumulate; then MRT_ERR_INVALID_ARG for a NULL image, guide, albedo, history or
 * moments, for a NULL prevGuide, prevHistory or prevMoments where havePrev != 0, for a given buffer
 * other than pixels that is not 16-byte aligned, or for history, moments, imageOut or pixels
 * overlapping an input or another of them (moments in particular is not prevMoments). */
typedef struct mrt_svgf_accumulate_params {
    int32_t width;
    int32_t height;
    int32_t havePrev;            /* 0: the first frame, nothing is reprojected */
    int32_t maxHistory;          /* 1..2^20 */
    float normalCos;
    float sigmaPlane;            /* in scene units */
    int32_t variant;             /* 0: the shipped launch shape; 1: linear; 2: 32 x 8 tiles */
    int32_t reserved;            /* 0 */
    float prevWorldToScreen[16]; /* column-major, of the previous frame */
    float prevSubpixel[2];
    const float* image;          /* mrt_path_resolve's float image */
    const void* guide;           /* mrt_denoise_features' of this frame */
    const float* albedo;
    const float* prevPosition;   /* mrt_temporal_motion's; may be NULL: static geometry */
    const void* prevGuide;       /* ignored, and may be NULL, where havePrev == 0 */
    const float* prevHistory;    /* likewise */
    float* history;
    float* imageOut;             /* may be NULL */
    uint32_t* pixels;            /* may be NULL */
    const float* prevMoments;    /* ignored, and may be NULL, where havePrev == 0 */
    float* moments;
} mrt_svgf_accumulate_params;
int  mrt_svgf_accumulate(const mrt_svgf_accumulate_params* params, void* stream);

/* mrt_svgf_filter over a width x height frame, pixel p = y * width + x, hit(p) = guide[p].w != 0
 * (n_p, x_p: the guide's normal and position). image (mrt_svgf_accumulate's imageOut), albedo,
 * moments, scratch and imageOut hold 4 floats per pixel, varianceOut one. The working image c_k
 * holds (r, g, b, v) per pixel: the demodulated colour and the variance of its luminance.
 * Two weights recur. For a pixel p and a tap q:
 *         a   = dot(n_p, n_q);  a = (a > 0) ? a : 0  (a NaN becomes 0);  then a = a * a,
 *               normalSquarings times
 *         dpl = dot(n_p, x_q - x_p) * invPlane  (the difference per component);  wz = 1 / (1 + dpl * dpl)
 * which are mrt_denoise_filter's. invPlane = 1 / sigmaPlane and sl2 = sigmaLuminance *
 * sigmaLuminance are computed once in float32.
 *  1. The variance launch: c_0(p).rgb is mrt_denoise_filter's step 1 (at a hit, per channel:
 *     (albedo > 0) ? image / albedo : 0; at a miss the image). With (m1, m2, -, N) = moments[p]:
 *      - at a miss: v = 0;
 *      - at a hit with N >= 4 (a NaN N does not pass, an infinite one does):
 *            v = pos(m2 - m1 * m1);
 *      - at a hit otherwise: s1 = s2 = wsum = 0; for dy = -3 .. 3 (outer) and dx = -3 .. 3 (inner),
 *        both ascending, the centre included, q = (x + dx, y + dy); a tap whose q lies outside the
 *        frame or with !hit(q) is skipped; otherwise, with (m1_q, m2_q) of moments[q],
 *            w = a * wz;  s1 += w * m1_q;  s2 += w * m2_q  (a multiply, then an add);  wsum += w.
 *        Where wsum > 0:  M1 = s1 / wsum;  M2 = s2 / wsum;  v = pos(M2 - M1 * M1) * (4 / N).
 *        Else (a zero normal, a NaN):  v = pos(m2 - m1 * m1) * (4 / N).  4 / N is one division.
 *  2. Iterations k = 0 .. iterations - 1 with step s = 1 << k. A miss pixel copies c_k to c_{k+1}.
 *     At a hit pixel p = (x, y), with (c_p, v_p) = c_k(p):
 *      - gs = gv = 0; for dy = -1 .. 1 (outer) and dx = -1 .. 1 (inner), both ascending, q = (x + dx,
 *        y + dy), the adjacent pixel at every step; a q outside the frame or with !hit(q) is skipped;
 *        otherwise g = {1/4, 1/8, 1/16} for |dx| + |dy| = 0, 1, 2;  gv += g * v_q;  gs += g.
 *        vt = (gs > 0) ? gv / gs : v_p.
 *      - invL = 1 / (sl2 * vt + 1e-8f);  lp = lum(c_p).
 *      - sum = (0, 0, 0), sv = 0, wsum = 0; for dy = -2 .. 2 (outer) and dx = -2 .. 2 (inner), both
 *        ascending, q = (x + dx * s, y + dy * s); a tap whose q lies outside the frame or with
 *        !hit(q) is skipped; otherwise, the centre tap included:
 *            hw = h[|dx|] * h[|dy|],  h = {0.375, 0.25, 0.0625}
 *            dl = lum(c_q) - lp;  wl = 1 / (1 + (dl * dl) * invL)
 *            w  = ((hw * a) * wz) * wl
 *            sum += w * c_q per channel r, g, b (a multiply, then an add)
 *            sv  += (w * w) * v_q;  wsum += w.
 *      - c_{k+1}(p) = (wsum > 0) ? (sum / wsum, sv / (wsum * wsum)) : c_k(p).
 *  3. The write, folded into the last launch (the variance launch where iterations == 0), with
 *     (c, v) = c_iterations(p): r = hit(p) ? c * albedo : c per channel; imageOut[p] = (r,
 *     image[p].w) where imageOut is given; pixels[p] = (r, 1) through the truncating device toABGR,
 *     as mrt_path_resolve's, where pixels is given; varianceOut[p] = v, the variance of the
 *     demodulated luminance, not remodulated, where varianceOut is given.
 * One variance launch and one launch per iteration, each reading one image and writing another, so
 * no workgroup waits on another and there are no atomics. The variance launch writes scratch[0];
 * iteration k < iterations - 1 writes scratch[(k + 1) & 1]. So scratch[0] is needed from 1
 * iteration on and scratch[1] from 2 on; scratch[2] is reserved and never touched; one that is not
 * needed is ignored and may be NULL. An iteration runs one of two kernels with the same arithmetic:
 * one loads every tap from global memory in 32 x 8 tiles, one stages a tile of 64 columns by 4 rows
 * a step apart, with its halo, in LDS (steps 1 .. 16) and reads only the nine adjacent variances
 * from global memory. variant 0 takes the shipped choice, 1 the direct kernel
 * everywhere, 2 the staged one wherever it fits; the results do not depend on it.
 * Checks, in this order, nothing written where one fails: NULL params; width or height < 1, a
 * negative iterations or normalSquarings, a variant outside 0..2, or a sigmaLuminance or sigmaPlane
 * that is not above 0 (a NaN included) is MRT_ERR_INVALID_ARG; width * height above 2^26, iterations
 * above 8 or normalSquarings above 10 MRT_ERR_TOO_LARGE; then MRT_ERR_INVALID_ARG for a NULL image,
 * guide, albedo, moments or needed scratch, for imageOut and pixels both NULL, for an image, guide,
 * albedo, moments, needed scratch or imageOut that is not 16-byte aligned, or for a needed scratch,
 * imageOut, pixels or varianceOut that overlaps an input or another of them. */
typedef struct mrt_svgf_filter_params {
    int32_t width;
    int32_t height;
    int32_t iterations;          /* 0..8 */
    int32_t normalSquarings;     /* 0..10 */
    float sigmaLuminance;        /* in standard deviations of the demodulated luminance */
    float sigmaPlane;            /* in scene units */
    int32_t variant;             /* 0: the shipped kernels; 1: direct loads; 2: LDS tiles */
    int32_t reserved;            /* 0 */
    const float* image;          /* mrt_svgf_accumulate's imageOut */
    const void* guide;           /* mrt_denoise_features' */
    const float* albedo;
    const float* moments;        /* mrt_svgf_accumulate's */
    float* scratch[3];
    float* imageOut;             /* may be NULL where pixels is given */
    uint32_t* pixels;            /* may be NULL where imageOut is given */
    float* varianceOut;          /* may be NULL */
} mrt_svgf_filter_params;
int  mrt_svgf_filter(const mrt_svgf_filter_params* params, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MRT_SVGF_H */
