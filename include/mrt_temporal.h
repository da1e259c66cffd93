/* mrt_temporal.h — temporal accumulation of path frames with reprojection, on the device.
 *
 * The stream-taking exports of mrt.h are a closed table; these two live in a
 * header of their own with a table of their own (tests/test_temporal_table.py,
 * tests/test_gpu_temporal_stream.py) and keep the same promises: every launch goes to `stream` (a
 * hipStream_t, NULL = the null stream), nothing waits on the host, nothing is read back and nothing
 * is allocated. Error codes and MRT_OK are mrt.h's. All pointers are device pointers on the calling
 * thread's current device. The CPU statements are mrth_temporal_motion and
 * mrth_temporal_accumulate (mrt_host.h).
 *
 * All arithmetic is float32, one IEEE operation at a time in the order written here, with no fused
 * multiply-add, no flushed denormal, correctly rounded `/` and no libm call but floorf, which is
 * exact. dot(a, b) = ((0 + a.x * b.x) + a.y * b.y) + a.z * b.z. Host and device agree bit for bit;
 * only the bits of a NaN that an operation makes differ. */
#ifndef MRT_TEMPORAL_H
#define MRT_TEMPORAL_H

#include <stdint.h>

#include "mrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mrt_temporal_motion: where every primary hit's surface point was in the previous frame. One lane
 * per primary slot i < numPrimary: p = primarySlotToId[i]; a slot whose p lies outside
 * [0, numPixels) is skipped, nothing is read or written for it. The slot's ray (o, d) =
 * primaryRays[i] and result (id, t) = primaryResults[i] are read as mrt_denoise_features reads them.
 * triangles holds three int32 vertex indices per triangle, vertices and prevVertices three floats
 * per vertex (the current and the previous frame's, numVertices each).
 *   - Miss: id outside [0, numTris), or any of the triangle's three vertex indices outside
 *     [0, numVertices) (no vertex is read then): prevPosition[p] = (0, 0, 0, 0).
 *   - Hit: x = o + d * t per component (one multiply, one add: the features' x). v0, v1, v2 are the
 *     triangle's current vertices, q0, q1, q2 its previous ones.
 *         e0 = v1 - v0,  e1 = v2 - v0,  r = x - v0
 *         d00 = dot(e0, e0),  d01 = dot(e0, e1),  d11 = dot(e1, e1),  d20 = dot(r, e0),  d21 = dot(r, e1)
 *         den = d00 * d11 - d01 * d01
 *     Where !(den > 0) (a degenerate triangle, a NaN): prevPosition[p] = (x, 1). Else
 *         b1 = (d11 * d20 - d01 * d21) / den
 *         b2 = (d00 * d21 - d01 * d20) / den
 *         b0 = (1 - b1) - b2
 *         prevPosition[p] = ((q0 * b0 + q1 * b1) + q2 * b2, 1)  per component.
 * Pixels no slot names keep what prevPosition held. prevPosition holds 4 floats per pixel.
 * Checks, in this order, nothing written where one fails: a negative numPrimary, numTris,
 * numVertices or numPixels is MRT_ERR_INVALID_ARG; more than 2^26 slots or pixels
 * MRT_ERR_TOO_LARGE; numPrimary == 0 or numPixels == 0 returns MRT_OK and launches nothing; then
 * MRT_ERR_INVALID_ARG for a NULL pointer (triangles may be NULL where numTris == 0, the two vertex
 * arrays where numTris == 0 or numVertices == 0), rays, results or prevPosition not 16-byte
 * aligned, or prevPosition overlapping an input. */
int  mrt_temporal_motion(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                         const void* primaryResults, const int32_t* triangles, int64_t numTris,
                         const float* vertices, const float* prevVertices, int64_t numVertices,
                         int32_t numPixels, float* prevPosition, void* stream);

/* mrt_temporal_accumulate over a width x height frame, pixel p = y * width + x, hit(p) =
 * guide[p].w != 0 (n_p, x_p: the guide's normal and position, mrt_denoise_features' record). Every
 * buffer holds 4 floats per pixel, except the guides, which hold 8.
 *  1. Current colour c: at a hit, per channel r, g, b: (albedo > 0) ? image / albedo : 0
 *     (mrt_denoise_filter's step 1); at a miss, image.
 *  2. At a miss: history[p] = (c, 1) and out = c.
 *  3. At a hit with havePrev != 0:
 *       xw = prevPosition ? prevPosition[p].xyz : x_p. Where prevPosition is given and its w == 0:
 *       no history.
 *       clip_i = sum over j of m[j * 4 + i] * v_j with v = (xw, 1) and m = prevWorldToScreen,
 *       column-major; the sum runs from 0, left to right, as mrt_raygen_primary's does.
 *       Where !(clip.w > 0): no history.
 *       sx = ((clip.x / clip.w + 1) * 0.5) * (float)width - prevSubpixel[0], sy likewise with
 *       clip.y, height and prevSubpixel[1]: the inverse of the primary ray's screen position, so a
 *       point that the previous frame saw through pixel (px, py) gives (px, py).
 *       Where !(sx > -1 && sx < width && sy > -1 && sy < height): no history (a NaN lands here).
 *       fx = floorf(sx), ix = (int)fx, ax = sx - fx; the same in y.
 *       sum = (0, 0, 0, 0), wsum = 0; taps j = 0, 1 (outer) and i = 0, 1 (inner), q = (ix + i, iy + j),
 *       bw = (i ? ax : 1 - ax) * (j ? ay : 1 - ay). A tap is skipped where q is outside the frame,
 *       bw == 0, prevGuide[q].w == 0, !(dot(n_p, n_q) >= normalCos), or
 *       !(fabs(dot(n_q, x_q - xw)) * invPlane <= 1) (n_q, x_q: prevGuide[q]'s; the difference per
 *       component: the previous frame's own plane through the previous point). Otherwise
 *       sum += bw * prevHistory[q] over all four channels (a multiply, then an add), wsum += bw.
 *       Where !(wsum > 0): no history. Else
 *         hst = sum / wsum per channel;  n1 = hst.w + 1;
 *         N = (n1 < (float)maxHistory) ? n1 : (float)maxHistory;  alpha = 1 / N;
 *         out = hst + (c - hst) * alpha per channel r, g, b (a subtract, a multiply, an add);
 *         history[p] = (out, N).
 *  4. With no history (havePrev == 0 included): history[p] = (c, 1) and out = c.
 *  5. r = hit(p) ? out * albedo : out; imageOut[p] = (r, image[p].w) where imageOut is given;
 *     pixels[p] = (r, 1) through the truncating device toABGR, as mrt_path_resolve's, where pixels
 *     is given.
 * invPlane = 1 / sigmaPlane, computed once in float32. imageOut is what mrt_denoise_filter takes as
 * its image; history is demodulated, its w the history length. One launch, one lane per pixel, in
 * one of two shapes with the same arithmetic: 256 consecutive pixels per workgroup, or 32 x 8
 * tiles. variant 0 takes the shipped one, 1 the linear one, 2 the tiled one; the
 * results do not depend on it.
 * Checks, in this order, nothing written where one fails: NULL params; width or height < 1,
 * maxHistory < 1, a variant outside 0..2, a sigmaPlane that is not above 0 (a NaN included) or a NaN
 * normalCos is MRT_ERR_INVALID_ARG; width * height above 2^26 or maxHistory above 2^20
 * MRT_ERR_TOO_LARGE; then MRT_ERR_INVALID_ARG for a NULL image, guide, albedo or history, for a NULL
 * prevGuide or prevHistory where havePrev != 0, for a given buffer other than pixels that is not
 * 16-byte aligned, or for history, imageOut or pixels overlapping an input or another of them
 * (history in particular is not prevHistory). */
typedef struct mrt_temporal_params {
    int32_t width;
    int32_t height;
    int32_t havePrev;            /* 0: the first frame, nothing is reprojected */
    int32_t maxHistory;          /* 1..2^20: the running mean's longest length */
    float normalCos;             /* a tap's normal is within this cosine of the pixel's */
    float sigmaPlane;            /* in scene units */
    int32_t variant;             /* 0: the shipped launch shape; 1: linear; 2: 32 x 8 tiles */
    int32_t reserved;            /* 0 */
    float prevWorldToScreen[16]; /* column-major, of the previous frame */
    float prevSubpixel[2];       /* the previous frame's sample position inside a pixel */
    const float* image;          /* mrt_path_resolve's float image */
    const void* guide;           /* mrt_denoise_features' of this frame */
    const float* albedo;
    const float* prevPosition;   /* mrt_temporal_motion's; may be NULL: static geometry */
    const void* prevGuide;       /* ignored, and may be NULL, where havePrev == 0 */
    const float* prevHistory;    /* likewise */
    float* history;
    float* imageOut;             /* may be NULL */
    uint32_t* pixels;            /* may be NULL */
} mrt_temporal_params;
int  mrt_temporal_accumulate(const mrt_temporal_params* params, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MRT_TEMPORAL_H */
