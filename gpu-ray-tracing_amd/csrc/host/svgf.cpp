// svgf.cpp — the variance-guided filter on the CPU: the statements mrt_svgf_accumulate /
// mrt_svgf_filter (csrc/svgf_kernel.hip) are checked against, term for term (csrc/svgf_common.hpp),
// with the device's plans (csrc/temporal_plan.cpp, csrc/svgf_plan.cpp: the same checks, limits and
// constants). The pixels are walked in order; a launch reads one image and writes another.
#include <cstring>

#include "../../../include/mrt_host.h"
#include "../svgf_common.hpp"
#include "../svgf_plan.hpp"
#include "../temporal_plan.hpp"
#include "host_error.hpp"
#include "records.hpp"

namespace mrt {
namespace {

using svgf::Color;
using svgf::Guide;

static_assert(sizeof(Guide) == 32 && sizeof(Color) == 16, "record sizes");

struct AccumulateHostSource {
    const mrth_svgf_accumulate_params& a;
    Color image(int p) const { return get_record<Color>(a.image, p); }
    Guide guide(int p) const { return get_record<Guide>(a.guide, p); }
    Color albedo(int p) const { return get_record<Color>(a.albedo, p); }
    Color prev_position(int p) const { return get_record<Color>(a.prevPosition, p); }
    Guide prev_guide(int q) const { return get_record<Guide>(a.prevGuide, q); }
    Color prev_history(int q) const { return get_record<Color>(a.prevHistory, q); }
    Color prev_moments(int q) const { return get_record<Color>(a.prevMoments, q); }
};

struct VarianceHostSource {
    const mrth_svgf_filter_params& a;
    Guide guide(int x, int y) const { return get_record<Guide>(a.guide, y * a.width + x); }
    Color image(int x, int y) const { return get_record<Color>(a.image, y * a.width + x); }
    Color albedo(int x, int y) const { return get_record<Color>(a.albedo, y * a.width + x); }
    Color moments(int x, int y) const { return get_record<Color>(a.moments, y * a.width + x); }
};

// c_k of a pixel, from host memory.
struct IterateHostSource {
    const float* in;
    const void* guides;
    int width;
    Guide guide(int x, int y) const { return get_record<Guide>(guides, y * width + x); }
    Color color(int x, int y) const { return get_record<Color>(in, y * width + x); }
    bool near_hit(int x, int y) const { return denoise::is_hit(guide(x, y)); }
    float near_variance(int x, int y) const { return color(x, y).a; }
};

void write_last(const mrth_svgf_filter_params& a, int p, const Color& c, bool hit) {
    const Color v{c.r, c.g, c.b, get_record<Color>(a.image, p).a};
    const Color r = hit ? denoise::remodulate(v, get_record<Color>(a.albedo, p), true) : v;
    if (a.imageOut) put_record(a.imageOut, p, r);
    if (a.pixels) a.pixels[p] = denoise::pixel_of(r);
    if (a.varianceOut) a.varianceOut[p] = c.a;
}

}  // namespace
}  // namespace mrt

extern "C" {

int mrth_svgf_accumulate(const mrth_svgf_accumulate_params* a) {
    if (!a) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "svgf_accumulate: null params");
    const mrt::TemporalPlan plan =
        mrt::plan_temporal_accumulate(a->width, a->height, a->maxHistory, a->normalCos, a->sigmaPlane, a->variant);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    const bool havePrev = a->havePrev != 0;
    if (!a->image || !a->guide || !a->albedo || !a->history || !a->moments ||
        (havePrev && (!a->prevGuide || !a->prevHistory || !a->prevMoments)))
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "svgf_accumulate: null argument");
    mrt::temporal::Constants k{};
    k.width = a->width;
    k.height = a->height;
    k.havePrev = havePrev ? 1 : 0;
    k.maxHistory = a->maxHistory;
    k.hasPrevPosition = a->prevPosition ? 1 : 0;
    k.normalCos = a->normalCos;
    k.invPlane = plan.invPlane;
    for (int i = 0; i < 16; i++) k.m[i] = a->prevWorldToScreen[i];
    k.subpixel[0] = a->prevSubpixel[0];
    k.subpixel[1] = a->prevSubpixel[1];
    const mrt::AccumulateHostSource src{*a};
    const int n = a->width * a->height;
    for (int p = 0; p < n; p++) {
        mrt::Color history, moments, result;
        mrt::svgf::accumulate_pixel(src, k, p, history, moments, result);
        mrt::put_record(a->history, p, history);
        mrt::put_record(a->moments, p, moments);
        if (a->imageOut) mrt::put_record(a->imageOut, p, result);
        if (a->pixels) a->pixels[p] = mrt::denoise::pixel_of(result);
    }
    return MRTH_OK;
}

int mrth_svgf_filter(const mrth_svgf_filter_params* a) {
    if (!a) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "svgf_filter: null params");
    const mrt::SvgfPlan plan = mrt::plan_svgf_filter(a->width, a->height, a->iterations, a->normalSquarings, a->sigmaLuminance,
                                                     a->sigmaPlane, a->variant);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    const int N = plan.iterations;
    if (!a->image || !a->guide || !a->albedo || !a->moments || (N >= 1 && !a->scratch[0]) || (N >= 2 && !a->scratch[1]))
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "svgf_filter: null argument");
    if (!a->imageOut && !a->pixels) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "svgf_filter: neither imageOut nor pixels");
    const int w = a->width, h = a->height;
    const mrt::VarianceHostSource first{*a};
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            const mrt::Color c = mrt::svgf::variance_pixel(first, x, y, w, h, plan.invPlane, a->normalSquarings);
            const int p = y * w + x;
            if (N == 0) mrt::write_last(*a, p, c, mrt::denoise::is_hit(first.guide(x, y)));
            else mrt::put_record(a->scratch[0], p, c);
        }
    }
    for (int k = 0; k < N; k++) {
        const mrt::IterateHostSource src{a->scratch[k & 1], a->guide, w};
        const bool last = k == N - 1;
        float* out = a->scratch[(k + 1) & 1];
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                const mrt::Color c =
                    mrt::svgf::filter_pixel(src, x, y, w, h, 1 << k, plan.invPlane, plan.sigmaLum2, a->normalSquarings);
                const int p = y * w + x;
                if (last) mrt::write_last(*a, p, c, mrt::denoise::is_hit(src.guide(x, y)));
                else mrt::put_record(out, p, c);
            }
        }
    }
    return MRTH_OK;
}

}  // extern "C"
