// denoise.cpp — the denoiser on the CPU: the statements mrt_denoise_features / mrt_denoise_filter
// (csrc/denoise_kernel.hip) are checked against, term for term (csrc/denoise_common.hpp), with the
// device's plan (csrc/denoise_plan.cpp: the same checks, limits and per-iteration constants). The
// pixels are walked in order; an iteration reads one image and writes another, as a launch does.
#include <cstring>

#include "../../../include/mrt_host.h"
#include "../denoise_common.hpp"
#include "../denoise_plan.hpp"
#include "host_error.hpp"
#include "records.hpp"

namespace mrt {
namespace {

static_assert(sizeof(rg::RayRec) == 32 && sizeof(denoise::Guide) == 32 && sizeof(denoise::Color) == 16, "record sizes");

// c_k of a pixel, from host memory: iteration 0 demodulates the frame's image on the way.
struct HostSource {
    const float* in;
    const void* guides;
    const float* albedo;
    int width;
    bool first;
    denoise::Guide guide(int x, int y) const { return get_record<denoise::Guide>(guides, y * width + x); }
    denoise::Color color(int x, int y, bool hit) const {
        const int q = y * width + x;
        const denoise::Color c = get_record<denoise::Color>(in, q);
        if (!first || !hit) return c;
        return denoise::demodulate(c, get_record<denoise::Color>(albedo, q), true);
    }
};

void write_last(const mrth_denoise_params& a, int p, const denoise::Color& c, bool hit) {
    const denoise::Color r = hit ? denoise::remodulate(c, get_record<denoise::Color>(a.albedo, p), true) : c;
    if (a.imageOut) put_record(a.imageOut, p, r);
    if (a.pixels) a.pixels[p] = denoise::pixel_of(r);
}

}  // namespace
}  // namespace mrt

extern "C" {

int mrth_denoise_features(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                          const void* primaryResults, const float* triNormals, const uint32_t* triMaterialColor,
                          int64_t numTris, int32_t numPixels, void* guide, float* albedo) {
    const mrt::DenoisePlan plan = mrt::plan_denoise_features(numPrimary, numTris, numPixels);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    if (plan.empty) return MRTH_OK;
    if (!primarySlotToId || !primaryRays || !primaryResults || !guide || !albedo || (numTris > 0 && (!triNormals || !triMaterialColor)))
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "denoise_features: null argument");
    for (int32_t i = 0; i < numPrimary; i++) {
        const int32_t p = primarySlotToId[i];
        if (p < 0 || p >= numPixels) continue;
        const mrt::RayResult res = mrt::get_record<mrt::RayResult>(primaryResults, i);
        mrt::denoise::Guide g;
        mrt::denoise::Color a;
        mrt::denoise::features_one(mrt::get_record<mrt::rg::RayRec>(primaryRays, i), res.id, res.t, triNormals, triMaterialColor,
                                   numTris, g, a);
        mrt::put_record(guide, p, g);
        mrt::put_record(albedo, p, a);
    }
    return MRTH_OK;
}

int mrth_denoise_filter(const mrth_denoise_params* a) {
    if (!a) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "denoise_filter: null params");
    const mrt::DenoisePlan plan =
        mrt::plan_denoise_filter(a->width, a->height, a->iterations, a->normalSquarings, a->sigmaColor, a->sigmaPlane, a->variant);
    if (plan.rc != 0) return mrt::host_fail(MRTH_ERR_INVALID_ARG, plan.why);
    const int N = a->iterations;
    if (!a->image || !a->guide || !a->albedo || (N >= 2 && !a->scratch[0]) || (N >= 3 && !a->scratch[1]))
        return mrt::host_fail(MRTH_ERR_INVALID_ARG, "denoise_filter: null argument");
    if (!a->imageOut && !a->pixels) return mrt::host_fail(MRTH_ERR_INVALID_ARG, "denoise_filter: neither imageOut nor pixels");
    const int w = a->width, h = a->height;
    if (N == 0) {
        const mrt::HostSource src{a->image, a->guide, a->albedo, w, true};
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                const bool hit = mrt::denoise::is_hit(src.guide(x, y));
                mrt::write_last(*a, y * w + x, src.color(x, y, hit), hit);
            }
        }
        return MRTH_OK;
    }
    const float* in = a->image;
    for (int k = 0; k < N; k++) {
        const mrt::HostSource src{in, a->guide, a->albedo, w, k == 0};
        const bool last = k == N - 1;
        float* out = a->scratch[k & 1];
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                const mrt::denoise::Color c =
                    mrt::denoise::filter_pixel(src, x, y, w, h, 1 << k, plan.invPlane, plan.at[k].invColor2, a->normalSquarings);
                const int p = y * w + x;
                if (last) mrt::write_last(*a, p, c, mrt::denoise::is_hit(src.guide(x, y)));
                else mrt::put_record(out, p, c);
            }
        }
        in = out;
    }
    return MRTH_OK;
}

}  // extern "C"
