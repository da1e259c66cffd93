/*
 * mrt_host.h — C-ABI of the host side around the hot path: scenes, the SBVH
 * builder, the Compact2 layout and its bvhcache .dat format, the camera and
 * ray generation. These are the producers of the trace kernel's inputs
 * (SURVEY.md §8f "next" rows), restating:
 *   src/rt/Scene.cc:35-101, src/framework/io/MeshWavefrontIO.cc:258-467   (scene, OBJ)
 *   src/rt/bvh/SplitBVHBuilder.cc:55-485, src/framework/base/Sort.cc:63-239 (SBVH)
 *   src/rt/cuda/CudaBVH.cc:79-116,270-380, Renderer.cc:157-217            (Compact2, cache)
 *   src/rt/ray/RayGen.cc:50-142, RayGenKernels.cu:79-227, PixelTable.cc    (ray generation)
 * All buffers here are HOST memory. Functions return 0 or an MRTH_ERR_* code.
 */
#ifndef MRT_HOST_H
#define MRT_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MRTH_OK = 0, MRTH_ERR_INVALID_ARG = 1, MRTH_ERR_IO = 2, MRTH_ERR_GENERATOR = 3 };

typedef struct mrth_scene mrth_scene;
typedef struct mrth_bvh mrth_bvh;

typedef struct mrth_camera {
    float position[3];
    float forward[3];
    float up[3];
    float fov_deg;      /* vertical field of view */
    float near_dist;
    float far_dist;
} mrth_camera;

typedef struct mrth_build_params {
    float sah_node_cost;      /* 1.0 */
    float sah_triangle_cost;  /* 1.0 */
    int32_t min_leaf_size;    /* 1   (Renderer.cc:54) */
    int32_t max_leaf_size;    /* 8   (Renderer.cc:54) */
    float split_alpha;        /* 1e-5 (BVH.hh BuildParams) */
    int32_t threads;          /* 0 = all cores; output is independent of it */
} mrth_build_params;

typedef struct mrth_bvh_stats {
    int64_t inner_nodes;
    int64_t leaf_nodes;
    int64_t tri_refs;
    int64_t max_depth;
    float sah_cost;
    double build_seconds;
} mrth_bvh_stats;

/* ---- scenes -------------------------------------------------------------- */
/* name: "mori" | "bunny" | "conference" | "sponza" | "hairball" (published
 * triangle counts; "hairball" with param > 0: that many tubes, unpadded), "sphere" (param = rings), "random" (param = triangles). */
int  mrth_scene_synthetic(const char* name, int64_t param, uint64_t seed, mrth_scene** out);
int  mrth_scene_load_obj(const char* path, mrth_scene** out);
/* Positions and indices taken as they are; the default material. The same mesh written as an .obj and
 * read by mrth_scene_load_obj is another scene to mrth_scene_hash (and so another bvhcache name) for
 * two reasons, and only these (tests/test_ref_host.py): the reference's importer parses decimals by
 * accumulating in float32 (String.cc:452-509), so the text of a float32 comes back up to a few ulps
 * off unless it is a short dyadic number, and it numbers vertices in order of first use by a face
 * (MeshWavefrontIO.cc:317-348), without welding equal positions. from_arrays of load_obj's own
 * positions and indices (mrth_scene_copy_arrays) hashes like load_obj. */
int  mrth_scene_from_arrays(const float* vertices, int64_t numVertices, const int32_t* triangles,
                            int64_t numTriangles, mrth_scene** out);
void mrth_scene_destroy(mrth_scene* s);
int64_t mrth_scene_num_triangles(const mrth_scene* s);
int64_t mrth_scene_num_vertices(const mrth_scene* s);
int  mrth_scene_copy_arrays(const mrth_scene* s, float* vertices /* 3*nv or NULL */,
                            int32_t* triangles /* 3*nt or NULL */, float* normals /* 3*nt or NULL */);
int  mrth_scene_camera(const mrth_scene* s, mrth_camera* cam, float* aoRadius);
/* Per-triangle ABGR colour tables of Scene::Scene (reference Scene.cc:47-80): the
 * material colour and the shaded colour diffuse * (dot(n, normalize(1,2,3)) / 2 + 1/2),
 * both through the host Vec4f::toABGR (Math.cc:45-52). A triangle's material is its OBJ
 * submesh's .mtl entry (Kd rgb, d alpha; MeshWavefrontIO.cc:114-200) or the default
 * (diffuse 0.75 grey, Mesh.hh:92; synthetic scenes). Either output may be NULL; each
 * holds num_triangles uint32. */
int  mrth_scene_tri_colors(const mrth_scene* s, uint32_t* material, uint32_t* shaded);
/* Each triangle's material diffuse colour, 4 floats (rgb, alpha) per triangle: what
 * mrth_scene_tri_colors shades, to hand to mrth_scene_attributes / mrt_scene_attributes as
 * triDiffuse. The default material (0.75, 0.75, 0.75, 1) where the scene has no .mtl. */
int  mrth_scene_tri_diffuse(const mrth_scene* s, float* out /* 4*nt */);
/* The scene's per-triangle tables over plain arrays (no scene object): the CPU statement of
 * mrt_scene_attributes (mrt.h), whose bits it gives (csrc/scene_common.hpp holds the arithmetic
 * of both, and of mrth_scene_copy_arrays' normals and mrth_scene_tri_colors). Same arguments,
 * outputs and rules: any output may be NULL but not all three; triDiffuse NULL = the default
 * material; a triangle with a vertex index outside [0, numVertices) reads no vertex, gets the
 * normal (0, 0, 0) and adds one to *skipped (may be NULL; added to, not reset). numTriangles == 0
 * is MRTH_OK; MRTH_ERR_INVALID_ARG where mrt_scene_attributes refuses (too many triangles included). */
int  mrth_scene_attributes(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                           const float* triDiffuse, float* triNormals, uint32_t* triShadedColor,
                           uint32_t* triMaterialColor, int64_t* skipped);

/* ---- BVH (SBVH build -> Compact2 host buffers) ---------------------------- */
void mrth_default_build_params(mrth_build_params* p);

/* hashBuffer (Hash.cc:34-76), the framework hash the two functions below are built on. */
uint32_t mrth_fw_hash_buffer(const void* ptr, int64_t size);
/* Scene::hash (Scene.cc:93-101): the framework hash (Hash.cc:34-76) of the scene's five
 * buffers — triangle vertex indices, face normals, material and shaded colours, positions. */
uint32_t mrth_scene_hash(const mrth_scene* s);
/* The reference's bvhcache file name for this scene and build (Renderer.cc:178-186):
 * "%08x.dat" of hashBits(scene hash, Platform("GPU") hash, BuildParams hash, BVHLayout_Compact2),
 * written to out (>= 13 bytes; 16 are touched). p NULL = defaults (mrth_default_build_params). */
int  mrth_bvh_cache_name(const mrth_scene* s, const mrth_build_params* p, char out[16]);
int  mrth_bvh_build(const mrth_scene* s, const mrth_build_params* p /* NULL = defaults */, mrth_bvh** out);
/* A linear BVH (no reference counterpart; the CPU statement of mrt_tracer_build, mrt.h, whose
 * bytes it reproduces): triangles sorted by the 63-bit Morton code of their box centres (a
 * stable sort, equal codes in index order), the Karras 2012 hierarchy over the sorted keys,
 * a node kept as a record iff it holds more than max_leaf_size triangles (1..8; 0 = the
 * default, MRTH_LBVH_DEFAULT_MAX_LEAF), boxes and Woop rows as mrth_bvh_refit computes them.
 * Single-threaded and deterministic. No spatial splits and no SAH: traces are slower than on
 * mrth_bvh_build's tree, the build is orders of magnitude faster. stats: inner_nodes =
 * records, leaf_nodes = leaves, tri_refs = triangles; the rest 0. */
enum { MRTH_LBVH_DEFAULT_MAX_LEAF = 4 };
int  mrth_bvh_build_lbvh(const mrth_scene* s, int32_t max_leaf_size, mrth_bvh** out);
int  mrth_bvh_load(const char* datPath, mrth_bvh** out);
int  mrth_bvh_save(const mrth_bvh* b, const char* datPath);
int  mrth_bvh_from_buffers(const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                           const int32_t* triIndex, int64_t triIndexBytes, mrth_bvh** out);
void mrth_bvh_destroy(mrth_bvh* b);
int  mrth_bvh_buffers(const mrth_bvh* b, const void** nodes, int64_t* nodeBytes, const void** woop,
                      int64_t* woopBytes, const int32_t** triIndex, int64_t* triIndexBytes);
int  mrth_bvh_get_stats(const mrth_bvh* b, mrth_bvh_stats* out);
/* Refit in place for moved vertices of the same topology (no reference counterpart; the
 * CPU statement of mrt_tracer_refit, mrt.h). triangles are the ones the BVH was built over
 * (triIndex refers to them), vertices their new positions. Every leaf is walked from its
 * first Woop slot in steps of three up to its terminator: its Woop rows are rewritten from
 * triIndex -> triangle -> vertices, its box becomes the min/max of its triangles' vertices
 * (the whole triangle also where the SBVH builder had clipped the reference, so a refitted
 * box may be looser than the built one, never tighter than the geometry); every inner box
 * becomes the union of its child's two boxes. Words 12-15 of the nodes, triIndex and the
 * terminators are untouched; an empty leaf keeps its box and adds nothing to its ancestors.
 * A triIndex entry >= numTriangles, or a vertex index outside [0, numVertices), is
 * MRTH_ERR_INVALID_ARG and nothing is written. */
int  mrth_bvh_refit(mrth_bvh* b, const float* vertices, int64_t numVertices, const int32_t* triangles,
                    int64_t numTriangles);
/* Re-optimise the topology in place by treelet restructuring (Karras & Aila 2013; no reference
 * counterpart; the CPU statement of mrt_tracer_optimize, mrt.h, whose bytes it reproduces).
 * rounds 1..MRTH_OPTIMIZE_MAX_ROUNDS passes (0 = the default, 1). A pass takes the height levels
 * of the tree as it stands (mrt_refit_plan's) and, level by level from height 1 up, forms below
 * every record a treelet of at most 7 leaves (the two child slots, then repeatedly the inner leaf
 * of largest float32 area dx*dy + dy*dz + dz*dx replaced by its two children, a tie to the earliest),
 * finds by exact dynamic programming over the leaf subsets the binary topology with the smallest
 * sum of inner-box areas, and rewrites the treelet's records when that sum is strictly below the
 * present one (csrc/treelet_common.hpp states every tie rule). Leaves are not regrouped: the
 * multiset of (leaf ref, leaf box) stays, as do the record count, words 14-15, Woop rows,
 * triIndex and terminators. A rewritten inner box is the union of its record's two boxes, so a
 * tree on which that held (every LBVH; a refitted SBVH) keeps it; boxes the SBVH builder clipped
 * stay as tight as they were where their record is not rewritten. A treelet with fewer than
 * 3 leaves, an inverted leaf box (lo > hi) or a subset area that is not finite is left bit for
 * bit, so NaN, infinite and empty boxes never steer a rewrite; so is one whose root would not get
 * back, bit for bit, the union of its two old boxes (another order of uniting can flip the sign
 * of a zero plane, and clipped boxes are not the unions of what lies below them): the slot above
 * the root is never recomputed, and stays what a refit would write. Nodes that are not a tree:
 * MRTH_ERR_INVALID_ARG, nothing written. info may be NULL. */
enum { MRTH_OPTIMIZE_MAX_ROUNDS = 8 };
typedef struct mrth_optimize_info {
    int32_t rounds;                                /* passes run                                     */
    int32_t levels;                                /* height levels after the last pass              */
    int64_t considered[MRTH_OPTIMIZE_MAX_ROUNDS];  /* per pass: records of height >= 1               */
    int64_t rewritten[MRTH_OPTIMIZE_MAX_ROUNDS];   /* per pass: treelets whose records were rewritten */
    double  wall_ms;
} mrth_optimize_info;
int  mrth_bvh_optimize(mrth_bvh* b, int32_t rounds, mrth_optimize_info* info);
/* The tree's area sums (the CPU statement of mrt_tracer_tree_cost, mrt.h; the layout is
 * mrt_tree_cost's): half surface areas dx*dy + dy*dz + dz*dx in double from the float32 planes,
 * every slot's term the device's bit for bit, added in record order, side 0 before side 1, the
 * root's term last. leaves and triangles count every leaf slot; a slot whose area is not finite
 * or whose box is inverted is counted in skipped and enters no sum, and so does the root union
 * (root_area 0 then). Child refs are counted, never followed. */
typedef struct mrth_tree_cost {
    double root_area;      /* area of the union of record 0's two boxes                    */
    double inner_area;     /* sum over child slots that refer to a record, + root_area     */
    double leaf_area;      /* sum over child slots that refer to a leaf                    */
    double leaf_tri_area;  /* the same, each times its leaf's triangle count               */
    int64_t records, leaves, triangles;
    int64_t skipped;
} mrth_tree_cost;
int  mrth_bvh_tree_cost(const mrth_bvh* b, mrth_tree_cost* out);
/* Woop rows (Z,U,V; 12 floats) of one triangle, CudaBVH::woopifyTri. */
void mrth_woopify(const float v0[3], const float v1[3], const float v2[3], float out[12]);

/* ---- rays (Ray = 8 floats, RayResult = 4 x 32 bit) ------------------------ */
int  mrth_pixel_table(int32_t w, int32_t h, int32_t* indexToPixel /* w*h */);
int  mrth_primary_rays(const mrth_camera* cam, int32_t w, int32_t h, void* rays /* w*h Ray */,
                       int32_t* slotToId /* w*h or NULL */);
/* Primary rays sampled at (jx, jy) in [0, 1)^2 inside each pixel (centre = 0.5, 0.5). */
int  mrth_primary_rays_subpixel(const mrth_camera* cam, int32_t w, int32_t h, float jx, float jy, void* rays,
                                int32_t* slotToId);
/* CameraControls::decodeSignature (CameraControls.cc:374-419, 502-554): the 6-bit text
 * camera of the reference App's --camera argument (grtcmdline.txt). Fills cam (position,
 * forward, up, fov, near, far) and, if non-NULL, the signature's speed and keepAligned.
 * MRTH_ERR_INVALID_ARG for a malformed signature ("CameraControls: Invalid signature!"). */
int  mrth_camera_decode_signature(const char* sig, mrth_camera* cam, float* speed, int32_t* keepAligned);

/* invert(fitToView(-1, 2, (w, h)) * worldToClip), column-major (Renderer.cc:126-129): the
 * matrix mrt_raygen_primary (mrt.h) takes. */
int  mrth_camera_nscreen_to_world(const mrth_camera* cam, int32_t w, int32_t h, float out[16]);
int  mrth_ao_rays(const void* primaryRays, const void* primaryResults, int64_t numPrimary,
                  const mrth_scene* s, int32_t numSamples, float maxDist, uint32_t seed,
                  void* outRays /* numPrimary * numSamples Ray */);
int64_t mrth_count_hits(const void* results, int64_t n);
/* The CPU statements of mrt_raygen_shadow and mrt_reconstruct_lit (mrt.h, which states the rays
 * and the pixels), with the same arguments over HOST memory and no stream, built from the same
 * header (csrc/light_common.hpp): the same bits. Ray index = the input ray's index within the call.
 * A count of 0 returns MRTH_OK and writes nothing; a negative count, numSamples < 1, more than
 * 2^31 - 1 output rays or a NULL required pointer is MRTH_ERR_INVALID_ARG. */
int  mrth_shadow_rays(const void* inRays, const void* inResults, int64_t numInputRays, int32_t numSamples,
                      const float light[3], float lightRadius, uint32_t seed,
                      void* outRays /* numInputRays * numSamples Ray */);
int  mrth_reconstruct_lit(int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                          const int32_t* primarySlotToId, const void* primaryRays, const void* primaryResults,
                          const int32_t* batchIdToSlot /* NULL = identity */, const void* batchResults,
                          const float* triNormals, const uint32_t* triMaterialColor, const float light[3],
                          uint32_t* pixels);

/* The CPU statements of mrt_path_extend, mrt_path_accumulate and mrt_path_resolve (mrt.h, which
 * states the arithmetic, the compaction and the checks), with the same arguments over HOST memory
 * and no stream, built from the same header (csrc/path_common.hpp): the same bits in every output,
 * the live count included. The struct is mrt_path_extend_params, field for field. Where mrt.h says
 * MRT_ERR_INVALID_ARG or MRT_ERR_TOO_LARGE these return MRTH_ERR_INVALID_ARG; alignment and overlap,
 * which matter to the device's 16-byte accesses and parallel lanes only, are not checked here. */
typedef struct mrth_path_extend_params {
    int32_t vertex;
    int32_t depth;
    int32_t numSamples;
    uint32_t seed;
    float lightPos[3];
    float lightRadius;
    float lightColor[3];
    float sky[3];
    float maxDist;
    int32_t compact;
    const float* triNormals;
    const uint32_t* triMaterialColor;
    int64_t numTris;
    int32_t numSlots;
    int32_t numPaths;
    const void* inRays;
    const void* inResults;
    const void* inState;
    void* outShadowRays;
    void* outPending;
    void* outRays;
    void* outState;
    float* radiance;
    int32_t* liveCount;
} mrth_path_extend_params;
int  mrth_path_extend(const mrth_path_extend_params* params);
int  mrth_path_accumulate(int32_t numSlots, int32_t numPaths, const void* state, const void* pending,
                          const void* shadowResults, float* radiance);
int  mrth_path_resolve(int32_t numSamples, int32_t firstPrimary, int32_t numPrimary, const int32_t* primarySlotToId,
                       const void* primaryResults, const float* radiance, uint32_t* pixels, float* image);

/* The CPU statements of mrt_denoise_features and mrt_denoise_filter (mrt.h, which states the
 * arithmetic and the checks), with the same arguments over HOST memory and no stream, built from
 * the same header (csrc/denoise_common.hpp) and the same plan: the same bits in every output. The
 * struct is mrt_denoise_params, field for field. Where mrt.h says MRT_ERR_INVALID_ARG or
 * MRT_ERR_TOO_LARGE these return MRTH_ERR_INVALID_ARG; alignment and overlap, which matter to the
 * device's 16-byte accesses and parallel lanes only, are not checked here. */
int  mrth_denoise_features(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                           const void* primaryResults, const float* triNormals, const uint32_t* triMaterialColor,
                           int64_t numTris, int32_t numPixels, void* guide, float* albedo);
typedef struct mrth_denoise_params {
    int32_t width;
    int32_t height;
    int32_t iterations;
    int32_t normalSquarings;
    float sigmaColor;
    float sigmaPlane;
    int32_t variant;             /* checked, otherwise ignored: the host has one statement */
    int32_t reserved;
    const float* image;
    const void* guide;
    const float* albedo;
    float* scratch[2];
    float* imageOut;
    uint32_t* pixels;
} mrth_denoise_params;
int  mrth_denoise_filter(const mrth_denoise_params* params);

/* The CPU statements of mrt_temporal_motion and mrt_temporal_accumulate (mrt_temporal.h, which
 * states the arithmetic and the checks), with the same arguments over HOST memory and no stream,
 * built from the same header (csrc/temporal_common.hpp) and the same plan: the same bits in every
 * output. The struct is mrt_temporal_params, field for field. Where mrt_temporal.h says
 * MRT_ERR_INVALID_ARG or MRT_ERR_TOO_LARGE these return MRTH_ERR_INVALID_ARG; alignment and
 * overlap, which matter to the device's 16-byte accesses and parallel lanes only, are not checked
 * here. */
int  mrth_temporal_motion(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                          const void* primaryResults, const int32_t* triangles, int64_t numTris,
                          const float* vertices, const float* prevVertices, int64_t numVertices,
                          int32_t numPixels, float* prevPosition);
typedef struct mrth_temporal_params {
    int32_t width;
    int32_t height;
    int32_t havePrev;
    int32_t maxHistory;
    float normalCos;
    float sigmaPlane;
    int32_t variant;             /* checked, otherwise ignored: the host has one statement */
    int32_t reserved;
    float prevWorldToScreen[16];
    float prevSubpixel[2];
    const float* image;
    const void* guide;
    const float* albedo;
    const float* prevPosition;
    const void* prevGuide;
    const float* prevHistory;
    float* history;
    float* imageOut;
    uint32_t* pixels;
} mrth_temporal_params;
int  mrth_temporal_accumulate(const mrth_temporal_params* params);

/* The CPU statements of mrt_svgf_accumulate and mrt_svgf_filter (mrt_svgf.h, which states the
 * arithmetic and the checks), with the same arguments over HOST memory and no stream, built from
 * the same header (csrc/svgf_common.hpp) and the same plans: the same bits in every output. The
 * structs are mrt_svgf_accumulate_params and mrt_svgf_filter_params, field for field. Where
 * mrt_svgf.h says MRT_ERR_INVALID_ARG or MRT_ERR_TOO_LARGE these return MRTH_ERR_INVALID_ARG;
 * alignment and overlap, which matter to the device's 16-byte accesses and parallel lanes only, are
 * not checked here. */
typedef struct mrth_svgf_accumulate_params {
    int32_t width;
    int32_t height;
    int32_t havePrev;
    int32_t maxHistory;
    float normalCos;
    float sigmaPlane;
    int32_t variant;             /* checked, otherwise ignored: the host has one statement */
    int32_t reserved;
    float prevWorldToScreen[16];
    float prevSubpixel[2];
    const float* image;
    const void* guide;
    const float* albedo;
    const float* prevPosition;
    const void* prevGuide;
    const float* prevHistory;
    float* history;
    float* imageOut;
    uint32_t* pixels;
    const float* prevMoments;
    float* moments;
} mrth_svgf_accumulate_params;
int  mrth_svgf_accumulate(const mrth_svgf_accumulate_params* params);
typedef struct mrth_svgf_filter_params {
    int32_t width;
    int32_t height;
    int32_t iterations;
    int32_t normalSquarings;
    float sigmaLuminance;
    float sigmaPlane;
    int32_t variant;             /* checked, otherwise ignored */
    int32_t reserved;
    const float* image;
    const void* guide;
    const float* albedo;
    const float* moments;
    float* scratch[3];
    float* imageOut;
    uint32_t* pixels;
    float* varianceOut;
} mrth_svgf_filter_params;
int  mrth_svgf_filter(const mrth_svgf_filter_params* params);

/* RayBuffer::mortonSort (RayBuffer.cc:256-324): the CPU statement of mrt_ray_sort (mrt.h, which
 * states the key and the order), with the same arguments over HOST memory and no stream. outBox
 * is six host floats (lo.xyz, hi.xyz). The box and the keys are csrc/raysort_common.hpp's on both
 * sides and the sort is std::stable_sort on key >> (6 * drop_levels), so keys, box values (up to
 * the sign of a zero), permutation, rays and both id maps equal the device's bit for bit.
 * MRTH_ERR_INVALID_ARG where mrt_ray_sort refuses (more than 2^30 rays included); numRays == 0
 * returns MRTH_OK and writes nothing. */
typedef struct mrth_ray_sort_params {
    int32_t drop_levels;  /* 0..24, 0 = the reference's full key */
    int32_t box;          /* 0 = origins and end points (reference), 1 = origins only */
} mrth_ray_sort_params;
int  mrth_ray_sort(const void* inRays, const int32_t* inSlotToId /* NULL = identity */, int32_t numRays,
                   const mrth_ray_sort_params* params /* NULL = defaults */, void* outRays,
                   int32_t* outIdToSlot /* may be NULL */, int32_t* outSlotToId /* may be NULL */,
                   uint32_t* outKeys /* may be NULL: 6 words per ray, in INPUT order */,
                   float* outBox /* may be NULL: lo.xyz, hi.xyz */);

const char* mrth_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MRT_HOST_H */
