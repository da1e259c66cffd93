/*
 * mrt.h — C-ABI of the MI355X BVH ray-traversal engine (the hot path).
 *
 * This is the drop-in boundary for the reference's tracing kernel module:
 *   reference  src/rt/kernels/CudaTracerKernels.hh:42-52   (extern "C" prototypes)
 *   reference  src/rt/kernels/kepler_dynamic_fetch.cu:417-479 (their implementations)
 *   caller     src/rt/cuda/CudaTracer.cc:119-177            (CudaTracer::traceBatch)
 *
 * Data formats are the reference's, byte for byte:
 *   - nodes    : CudaBVH BVHLayout_Compact2 node array, 64 B per inner node
 *                (reference src/rt/cuda/CudaBVH.hh:40-55, CudaBVH.cc:270-357)
 *   - woop     : Woop triangle rows (Z,U,V as float4) + one float4 terminator
 *                (x bits == 0x80000000) after every leaf
 *   - triIndex : one int32 per woop float4 slot (origIdx for the Z row)
 *   - rays     : Ray[n], 32 B = float4(orig.xyz, tmin) + float4(dir.xyz, tmax)
 *                (reference src/rt/Util.hh:64-73)
 *   - results  : RayResult[n], 16 B = int id, float t, int pad[2]; the trace
 *                writes only {id, t} (reference src/rt/Util.hh:79-89,
 *                CudaTracerKernels.hh:197 STORE_RESULT)
 *
 * All buffer pointers are DEVICE pointers owned by the caller (the library
 * borrows them; reference ownership model CudaBVH.cc:101-109, RayBuffer.cc:42-81).
 * Every function returns 0 on success or a positive MRT_ERR_* code; the
 * reference instead printed and exit(-1)'d (cutil_inline_runtime.h:32-42) —
 * the compat entry points at the bottom keep that behaviour.
 */
#ifndef MRT_H
#define MRT_H

#include <stdint.h>
#include <stddef.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------ */
enum {
    MRT_OK = 0,
    MRT_ERR_INVALID_ARG = 1,   /* null pointer / negative size / bad flag   */
    MRT_ERR_NOT_BOUND = 2,     /* trace before bind (CudaTracer.cc:129)      */
    MRT_ERR_HIP = 3,           /* a HIP runtime call failed                  */
    MRT_ERR_NO_DEVICE = 4,     /* no GPU visible                             */
    MRT_ERR_TOO_LARGE = 5,     /* buffer beyond the 4 GiB buffer-offset range, or > 2^30 rays per launch */
    MRT_ERR_STACK_OVERFLOW = 6 /* a ray needed more than the reference's 64 stack entries
                                  (kepler_dynamic_fetch.cu:47 STACK_SIZE): its result is incomplete */
};

/* ---- trace flags (bit set) -------------------------------------------- */
enum {
    MRT_TRACE_ANY_HIT = 1u << 0,  /* any-hit early out; reference anyHit=!needClosestHit (CudaTracer.cc:172) */
    MRT_TRACE_EXACT_RCP = 1u << 1,/* correctly rounded 1/x in the Woop test & ray setup (parity mode);
                                     default is the hardware v_rcp_f32 (the reference used rcp.approx)  */
    MRT_TRACE_LOCKSTEP_OFF = 1u << 2, /* per-lane (non-speculative) while-while: every lane follows the
                                     single-ray order exactly (deterministic any-hit, exact counters)  */
    MRT_TRACE_STATS = 1u << 3,    /* also write per-ray {inner nodes, tris tested, leaves, latency in 10 ns ticks} int4s */
    MRT_TRACE_SECONDARY = 1u << 4 /* tuning hint, no effect on results: the batch holds secondary rays (AO, diffuse,
                                     later bounces). The autotuner keeps their schedule apart from a primary batch
                                     of the same size and kernel variant (saved / exported with variant | 512) */
};

/* One per HIP device. Re-entrant: launches on different streams get separate
 * scratch (stack spill slab, queue heads, overflow counter), so traces on
 * several streams of one handle may run concurrently. */
typedef struct mrt_tracer mrt_tracer;

/* Tuning knobs of the persistent launch (0 = library default). */
typedef struct mrt_launch_cfg {
    int32_t waves_per_cu;      /* persistent waves per CU (grid = CUs * waves_per_cu); 0 = auto (by batch size).
                                  With num_queues, waves_per_cu, fetch_threshold and lane_groups all at their
                                  defaults, a batch over a BVH larger than the 256 MB Infinity Cache uses
                                  one global queue, refills at 48 live lanes, 12 waves/CU up to 3 rays per
                                  lane of a 16-wave grid, else 16 (mrt_trace_info reports what a launch used) */
    int32_t fetch_threshold;   /* queue modes (num_queues >= 1): refill a wave when fewer than this many of its
                                  64 lanes are live (0 = when all are done; reference DYNAMIC_FETCH_THRESHOLD
                                  20 of 32, kepler_dynamic_fetch.cu:48). Static strided rounds ignore it   */
    int32_t num_queues;        /* -1 (default) = static strided rounds, no atomics; 1..8 = the reference's
                                  dynamic fetch: a static first round, then one atomic per wave refill
                                  on the queue of the wave's XCD (xcc % num_queues), no stealing of rays
                                  from a served queue; a queue no wave has taken from when a wave's own
                                  queue is dry (an XCD without workgroups of the launch, e.g. a CPX/DPX
                                  partition) is adopted by that wave, so every ray is traced whatever
                                  the placement. The autotuner's per-XCD candidate uses one queue per
                                  XCD of the device (hipDeviceAttributeNumberOfXccs)                   */
    int32_t lds_stack;         /* traversal-stack entries per lane kept in LDS: 8, 16 or 32       */
    int32_t lane_groups;       /* strided mode: a wave's 64 lanes take rays from this many (1..64, power of
                                  two) distant sub-ranges of the batch instead of 64 consecutive rays */
    int32_t wide;              /* the speculative traversal reads 4-wide nodes derived from the bound
                                  Compact2 tree at bind time (half the dependent node fetches; closest hits
                                  equal the binary traversal's except exact-t ties): 1 = exact child boxes
                                  (128-B nodes), 2 = child boxes quantized outward to 8 bits per plane
                                  (64-B nodes; a superset of the binary traversal's leaves, falls back to 1
                                  when a box has no finite quantization); 0 = the Compact2 nodes
                                  themselves; -1 = library default. The per-lane
                                  (MRT_TRACE_LOCKSTEP_OFF) mode always walks the Compact2 nodes */
    int32_t spec_slack;        /* speculative mode: a wave turns from its inner nodes to its postponed leaves
                                  once at most this many of its lanes are still without a leaf (0..63; the
                                  reference waits for all, i.e. 0; default 2; -1 = library default) */
    int32_t static_rounds;     /* queue modes (num_queues >= 1): rays handed out in this many static strided
                                  rounds of the grid before the queues take over (1..64; 0 = default 1) */
    int32_t autotune;          /* 1 = with the distribution knobs above at their defaults, the first launches
                                  of each batch size (per kernel variant, up to 64 sizes) time eight ray-
                                  distribution schedules (static rounds at 20, 16, 12 or 8 waves/CU, per-XCD
                                  block-cyclic queues, the global queue at 20, 16 or 12 waves/CU), then
                                  the winner and the runner-up, each with spec_slack 4 and 6, without the
                                  frontier tail, with 16 lane groups, and with 2 lane groups at spec_slack 6 (each
                                  knob only when left at its default), then the best such modifier on the
                                  six other schedules (stage 3); each candidate runs four launches at a time
                                  (the first untimed) until it has eight timed samples, without blocking,
                                  after one untimed round; the median ranks them and a candidate
                                  replaces the fixed rule (stage 1) or the previous stage's winner only
                                  when 3 % faster. Settling costs 32 untimed launches, then per stage of
                                  n candidates (8, 10, 6) 4 * n * 3 - 1 launches (eight samples at three
                                  per run of four: three cycles, the last run one launch short): 246
                                  launches when no modifier clears the margin, 317 with stage 3, when each
                                  timing is read by the next launch (mrt_tracer_trace_timed); asynchronous
                                  launches add their in-flight lag at every stage end (256-328 measured).
                                  The policy is csrc/tune.cpp, run on the CPU by tests/test_tune.py.
                                  A new batch size within 1/32 of a settled one of the same variant
                                  and ray class (MRT_TRACE_SECONDARY batches are a class
                                  of their own) takes the nearest settled schedule without exploring —
                                  a schedule tuned on another ray distribution of that class; such
                                  inherited entries are not exported by mrt_tracer_tune_export (an
                                  imported schedule for the same key replaces one and is). A batch
                                  size launched on more than one stream is not explored: it runs its settled
                                  schedule if it has one, else the fixed rule; reset by bind and set_config (default 1; mrt_tracer_tune_export /
                                  _import save and restore the choices). 0 = the fixed rule only; -1 = default */
    int32_t tail_lanes;        /* exact 4-wide speculative traversal: a wave that cannot refill (its strided
                                  round, or its queue drained) and is down to at most this many tracing
                                  lanes finishes those rays in the frontier tail: 64/R lanes per ray for R
                                  rays (at least four), up to 16/R pending nodes or four-triangle leaf chunks
                                  per ray per memory round trip, regrouping as rays finish (0..16; 0 = off;
                                  default 16; -1 = default; the autotuner tries 0 when left at the default) */
    int32_t queue_shared;      /* num_queues > 1: this percentage of the batch's rays (its end) goes to one
                                  shared queue that a wave takes from once its XCD's queue is dry; the
                                  rest is dealt in per-XCD contiguous shares (0..100; default 0; -1 =
                                  default)                                                             */
    int32_t queue_block;       /* num_queues > 1: 0 = each queue's share is contiguous; a power of two >= 64 =
                                  the shares are this many rays' blocks dealt cyclically (block i to queue
                                  i mod num_queues), so every XCD samples the whole frame (default 0;
                                  -1 = default)                                                        */
    int32_t ray_sort;          /* 1 = a static launch whose batch fits one round of the grid (e.g. 307 200 rays
                                  at 20 waves/CU) deals each workgroup's 256 consecutive rays to its four
                                  waves by direction octant, degenerate (tmax < 0) rays last, instead of
                                  the strided deal (exact 4-wide traversal only); 0 = off (default; -1 =
                                  default). Results are unchanged: every ray is traced once either way.
                                  With ray_sort = 1 the strided deal ignores lane_groups (in every launch,
                                  also one whose batch needs several rounds, where the sort is skipped) */
    int32_t queue_xcc_mask;    /* test hook, 0 = off (default; -1 = default): 1..15 = a wave takes from queue
                                  (XCC_ID & mask) % num_queues, so with mask 3 and 8 queues, queues 4..7
                                  have no waves of their own (the unserved-queue sweep must trace them) */
    int32_t backfill;          /* static strided rounds only: 0 = the persistent grid (default; -1 = default):
                                  every workgroup is resident for the whole launch and takes numRays /
                                  grid lanes rounds. k = 1..64: the grid is sized from the batch so that
                                  every lane takes at most k rays (ceil(numRays / (256 k)) workgroups,
                                  rounded up to a multiple of 8); a workgroup ends after its rounds and the
                                  hardware dispatcher starts the next one in the freed slot. waves_per_cu
                                  then caps the workgroups resident per CU (dynamic LDS passed at launch,
                                  checked against the occupancy query; 0 = the static default, 20). A batch
                                  that fits the resident grid runs the persistent launch, and k is raised
                                  until the spill slab (one per launched lane) fits 256 MB; mrt_trace_info
                                  reports what a launch used. Refused with num_queues >= 1 and with
                                  ray_sort = 1 (MRT_ERR_INVALID_ARG); a tracer with it set is not autotuned.
                                  Results are unchanged: every ray is traced once either way           */
    int32_t oneshot;           /* 1 = a backfilled grid of one ray per lane (backfill = 1) runs the one-shot
                                  kernels: the lane's ray is computed once, in closed form, and the kernel
                                  holds no refill loop, queue code or ray sort (fewer registers, no
                                  spills). The exact 4-wide speculative traversal at lds_stack 16 has them;
                                  another variant, a batch that fits the resident grid and one whose spill
                                  slab asks for more than one ray per lane run the launch as without it
                                  (mrt_trace_info.oneshot reports which). The grid is 8 * ceil(c / 256)
                                  workgroups for c positions per XCD group (deal_block). 0 = off (default;
                                  -1 = default). Refused unless backfill = 1 (so also with queues and
                                  with ray_sort). Results are unchanged: every ray is traced once        */
    int32_t deal_block;        /* oneshot = 1: 0 = each XCD group (blockIdx % 8) traces one contiguous chunk
                                  of roundup64(ceil(numRays / 8)) rays, as the strided rounds deal them
                                  (default; -1 = default). b = 6..15: the batch's 2^b-ray blocks are dealt
                                  cyclically, block i to group i mod 8, so every XCD samples the whole
                                  Morton-ordered frame and the groups cost alike; c = ceil(ceil(numRays /
                                  2^b) / 8) * 2^b, which may exceed ceil(numRays / 8) (lanes past the batch
                                  trace nothing). Refused without oneshot = 1 and outside {0, 6..15}     */
} mrt_launch_cfg;

/* Per-launch statistics reported back to the host (optional). */
typedef struct mrt_trace_info {
    float   kernel_ms;         /* event-timed duration of the trace launch (if requested)        */
    int32_t grid_waves;        /* waves launched: all resident at once in a persistent launch; in a
                                  backfilled one (backfill > 0) blocks_per_cu workgroups per CU at a time */
    int32_t block_threads;     /* threads per workgroup                                           */
    int32_t lds_stack_entries; /* per-lane traversal-stack entries held in LDS                    */
    int32_t wide;              /* node width the launch traversed: 2 (Compact2) or 4              */
    int32_t num_queues;        /* ray queues the launch used (0 = static strided rounds)          */
    int32_t fetch_threshold;   /* live-lane refill threshold the launch used (0 for static strided rounds:
                                  the refill applies to the queue modes only)                        */
    int32_t stack_overflows;   /* entries pushed past stack_capacity in this launch (then the call returns
                                  MRT_ERR_STACK_OVERFLOW; 0 for any SBVH of depth <= 64)            */
    int32_t node_bytes;        /* bytes per node the launch read: 64 (Compact2 or quantized 4-wide), 128 */
    int32_t autotune_candidate; /* cfg.autotune: the schedule candidate this launch used, else -1 (the fixed
                                  rule): 0..7 a ray-distribution schedule; 8..12 a stage-2 modifier of
                                  the stage-1 schedule s, encoded as modifier | s << 8 (8/9: spec_slack
                                  4/6, 10: the frontier tail toggled, 11: 16 lane groups, 12: 2 lane
                                  groups at spec_slack 6; bench.py schedule_name spells them out)    */
    int32_t autotune_locked;   /* 1 once the batch size's schedule is chosen                      */
    int32_t stack_capacity;    /* stack entries (sentinel included) the launch had: 64 = the reference's
                                  for the binary order; the wide orders get the bound tree's worst case
                                  (never less than 64), so no ray of a tree overflows there          */
    int32_t backfill;          /* rays per lane the launched grid was sized for (cfg.backfill or a saved
                                  schedule's, raised where the spill slab asked for it); 0 = the persistent
                                  grid, also for a batch that fits the resident grid                  */
    int32_t blocks_per_cu;     /* workgroups resident per CU at once                                  */
    int32_t dyn_lds_bytes;     /* dynamic LDS per workgroup that caps the residency of a backfilled
                                  launch (0 = none needed, and in every persistent launch)            */
    int32_t oneshot;           /* 1 = the launch ran the one-shot kernel on its own grid (cfg.oneshot or a
                                  saved schedule's); 0 in every other launch, also where cfg.oneshot fell
                                  back (see mrt_launch_cfg.oneshot)                                     */
    int32_t deal_block;        /* log2 of the one-shot launch's deal blocks (0 = contiguous, and whenever
                                  oneshot is 0)                                                       */
} mrt_trace_info;

/* What the last bind derived (mrt_tracer_bind_info). */
typedef struct mrt_bind_info {
    double  bind_ms;           /* wall time of the last bind / set_config's wide-node derivation      */
    int64_t wide_bytes;        /* bytes of the derived 4-wide node array (0 = the Compact2 nodes)      */
    int32_t wide_format;       /* 0 = Compact2, 1 = exact 4-wide (128 B), 2 = quantized 4-wide (64 B)  */
    int32_t stack_capacity;    /* stack entries the wide traversal gets (see mrt_trace_info)          */
    int32_t stack_bound;       /* entries (sentinel excluded) a depth-first walk of the bound tree can hold:
                                  the wide tree's worst case (63 for the binary order). The frontier tail
                                  expands several entries per step only while this much room stays free,
                                  so it never needs more than stack_capacity either                     */
} mrt_bind_info;

/* One settled launch schedule of the autotuner (cfg.autotune): the candidate a batch
 * size and kernel variant chose. Opaque apart from num_rays; valid for the library
 * version MRT_TUNE_VERSION and the BVH it was tuned on (the caller keys a saved
 * table by the BVH, e.g. next to its .dat cache). */
typedef struct mrt_tuned_schedule {
    int32_t num_rays;
    int32_t variant;
    int32_t candidate;         /* bits 0-15: the autotuner's code (mrt_trace_info.autotune_candidate);
                                  bits 16-22: cfg.backfill of the schedule (static schedules only, 0..64);
                                  bit 23: cfg.oneshot (only with a backfill of 1);
                                  bits 24-26: its residency cap in workgroups per CU (0 = the schedule's
                                  own waves_per_cu); bits 27-30: cfg.deal_block (0 or 6..15, only with
                                  bit 23); bit 31 is zero                                          */
    int32_t version;          /* MRT_TUNE_VERSION when exported; others are refused on import */
} mrt_tuned_schedule;
enum { MRT_TUNE_VERSION = 11 };   /* 11: round 6 (schedules re-tuned on the round-6 library) */

/* What mrt_tracer_refit_info reports. */
typedef struct mrt_refit_info {
    int32_t levels;            /* height levels of the bound tree (level 0: nodes with two leaf children)  */
    int32_t launches;          /* kernel launches of the last refit: 1 for the leaves, 1 per level >= 1 of
                                  more than 1024 nodes, 1 for all smaller levels together, 1 for the exact
                                  4-wide array (cfg.wide 1)                                              */
    int64_t plan_bytes;        /* device bytes of the refit plan: 4 per node (the level order), 2 per node
                                  (scratch), 4 per level, and 16 per wide node (cfg.wide 1)              */
    int64_t skipped_refs;      /* leaf triangles the refits since the last call left out because their
                                  triIndex entry or one of their vertex indices was out of range        */
} mrt_refit_info;

/* ---- handle API -------------------------------------------------------- */
int  mrt_tracer_create(int device, mrt_tracer** out);
int  mrt_tracer_destroy(mrt_tracer* t);

/* Bind a Compact2 BVH (device pointers, borrowed). Replaces bind_CudaBVHTexture
 * (CudaTracerKernels.hh:44); unlike the reference it may be called again to
 * re-bind a new BVH (the reference never re-bound, CudaTracer.cc:142-146).
 * Tracing only reads the buffers; mrt_tracer_refit WRITES nodes and woop in place,
 * so a caller that refits must bind writable memory. */
int  mrt_tracer_bind(mrt_tracer* t,
                     const void* nodes, int64_t nodeBytes,
                     const void* woop, int64_t woopBytes,
                     const int32_t* triIndex, int64_t triIndexBytes);
int  mrt_tracer_unbind(mrt_tracer* t);

int  mrt_tracer_set_config(mrt_tracer* t, const mrt_launch_cfg* cfg);
int  mrt_tracer_get_config(const mrt_tracer* t, mrt_launch_cfg* cfg);
int  mrt_tracer_bind_info(const mrt_tracer* t, mrt_bind_info* info);

/* The autotuner's settled schedules (up to capacity; *count = how many exist), and
 * the reverse: schedules saved from an earlier run of the same BVH are locked at
 * once (no exploring launches, the same schedule every run). Import after bind
 * (bind and set_config forget every schedule). */
int  mrt_tracer_tune_export(const mrt_tracer* t, mrt_tuned_schedule* out, int32_t capacity, int32_t* count);
int  mrt_tracer_tune_import(mrt_tracer* t, const mrt_tuned_schedule* in, int32_t count);

/* Stream-ordered trace of numRays (<= 2^30) rays (device pointers). stream is a
 * hipStream_t (NULL = the null stream). stats may be NULL unless
 * MRT_TRACE_STATS is set (then: int32[4*numRays]). Asynchronous: a stack
 * overflow cannot be returned here; it accumulates in a sticky per-stream
 * counter that mrt_tracer_stack_overflows reads. */
int  mrt_tracer_trace(mrt_tracer* t, const void* rays, void* results, int32_t numRays,
                      uint32_t flags, int32_t* stats, void* stream);

/* Same, but blocking and event-timed around the launch only — the
 * reference's launch_tracingKernel contract (kepler_dynamic_fetch.cu:432-474).
 * Returns MRT_ERR_STACK_OVERFLOW (results written, info filled) when a ray of
 * this launch needed more than stack_capacity entries (64 in the binary order). */
int  mrt_tracer_trace_timed(mrt_tracer* t, const void* rays, void* results, int32_t numRays,
                            uint32_t flags, int32_t* stats, void* stream, mrt_trace_info* info);

/* Stack overflows of asynchronous launches since the last reset, summed over the
 * handle's streams (synchronises them). reset != 0 zeroes the counters. */
int  mrt_tracer_stack_overflows(mrt_tracer* t, int64_t* count, int32_t reset);

/* Which traversal kernel ran, and which exist (host only: neither call touches the device).
 * A kernel key is a bit field:
 *   bit 0 (1)    any-hit (MRT_TRACE_ANY_HIT)
 *   bit 1 (2)    speculative: the warp-wide postponement (MRT_TRACE_LOCKSTEP_OFF clear)
 *   bit 2 (4)    exact reciprocal (MRT_TRACE_EXACT_RCP)
 *   bit 3 (8)    per-ray counters (MRT_TRACE_STATS)
 *   bits 4-5     lds << 4: the LDS stack entries per lane, lds 0 / 1 / 2 = 8 / 16 / 32 (cfg.lds_stack)
 *   bits 6-7     nodes << 6: the node format read, 0 = Compact2, 1 = exact 4-wide, 2 = quantized 4-wide
 *   bit 8 (256)  the instantiation with the frontier tail (cfg.tail_lanes > 0; exact 4-wide only)
 *   bit 9 (512)  the one-shot sibling (cfg.oneshot; exact 4-wide at 16 LDS entries only)
 * The 4-wide formats exist in the speculative mode only.
 *
 * mrt_trace_kernel_keys returns how many kernels the library instantiates and writes the first
 * `capacity` of their keys, ascending, to keys (which may be NULL with capacity 0): a key is
 * listed if and only if a launch of that variant has a kernel of its own to run.
 * mrt_tracer_last_kernel_key returns the key of the kernel the handle's most recent trace
 * launched: after the autotuner's candidate, after the tail was settled for the bound tree and
 * after cfg.oneshot fell back where it had to; -1 before any launch (and for a NULL handle).
 * Both go by the kernel function itself, not by the variant that was asked for: were two
 * variants served by one function, only the smaller key would be listed and reported. */
int  mrt_trace_kernel_keys(int32_t* keys, int capacity);
int  mrt_tracer_last_kernel_key(const mrt_tracer* t);

/* Refit the bound BVH on the device for moved vertices of a FIXED topology (animated or
 * deforming meshes; no reference counterpart). vertices (3 floats each) and triangles (3
 * vertex indices each; the triangles the BVH was built over, triIndex refers to them) are
 * DEVICE pointers. The call rewrites, in the bound nodes and woop buffers (which must be
 * writable) and in the library's derived 4-wide array, exactly what depends on vertex
 * positions: every leaf is walked from its first Woop slot in steps of three up to its
 * terminator, its Woop rows recomputed (bit-identical to mrth_bvh_refit / a host build of
 * the same vertices), its box set to the min/max of its triangles' vertices; inner boxes are
 * unions of their child's two boxes, one launch per height level, bottom-up. Words 12-15 of
 * the nodes, triIndex and the terminators are untouched; an empty leaf keeps its box.
 *   - Limits: a leaf box covers the whole triangle also where the SBVH builder had clipped
 *     the reference to a spatial split, so refitted boxes are correct but may be looser than
 *     built ones (traces get slower, never wrong); the tree is not re-optimised, so large
 *     deformations degrade it (mrt_tracer_tree_cost below reports the tree's SAH terms; DESIGN
 *     §13 has how far they predict the trace). When that shows, rebuild on the device (mrt_tracer_build_device:
 *     1.65 ms for bunny) or, where the leaves must stay, restructure (mrt_tracer_optimize below:
 *     bunny displaced by 10 % of its size traced 0.93x after one round, 0.85x after three,
 *     0.77x after the rebuild); mrth_bvh_build + bind is the 20 s host route.
 *   - A triIndex entry outside [0, numTriangles) or a vertex index outside [0, numVertices)
 *     is never dereferenced: that triangle keeps its old rows, is left out of its leaf's
 *     box, and is counted (mrt_refit_info.skipped_refs). Nothing is reported here.
 *   - Ordering: stream-ordered on `stream` (a hipStream_t, NULL = the null stream) without a
 *     host sync, after the first refit following a bind or set_config, which builds the
 *     refit plan (synchronous; on the device, mrt_tracer_bind_device below, or from one copy
 *     of the nodes to the host for a tree of more than MRT_DERIVE_MAX_LEVELS depth levels;
 *     mrt_refit_info.plan_bytes on the device until the next bind, unbind or set_config).
 *     After mrt_tracer_bind_device / mrt_tracer_build_device the plan is already there. The refit runs after this
 *     handle's traces enqueued on `stream` before it, and traces enqueued on `stream` after
 *     it see the refitted tree. A trace on ANOTHER stream that overlaps a refit reads a
 *     half-updated tree: ordering those (events, synchronisation) is the caller's job.
 *   - Kept: the autotuner's schedules, the workspaces and the wide traversal's stack
 *     capacity and bound (the topology, and with it the worst-case stack, is unchanged).
 *   - cfg.wide 1 (default): the exact 4-wide array's planes are copied from the refitted
 *     Compact2 slots the bind-time collapse took them from (the collapse is not redone:
 *     refitted surface areas would choose other children). cfg.wide 2: the quantized array
 *     has no in-place update; it is derived again from the refitted nodes through the
 *     bind-time host path, which makes the call SYNCHRONOUS and slow (results are correct).
 *     Where a refitted box is not finite (an infinite vertex coordinate) the quantized form
 *     cannot hold it: the exact array is derived instead (mrt_bind_info.wide_format 1), and
 *     it stays, updated in place by later refits, until the next bind or set_config.
 *   - A NaN vertex coordinate enters no box (a NaN plane would cull the finite triangles
 *     beside it); that triangle's Woop rows are NaN and nothing hits it. An infinite
 *     coordinate makes its leaf's and every ancestor's box infinite on that side.
 * MRT_ERR_NOT_BOUND before a bind; MRT_ERR_INVALID_ARG when the bound nodes are not a tree
 * (a child ref outside the array, a record reached twice or never). */
int  mrt_tracer_refit(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                      int64_t numTriangles, void* stream);

/* Blocking (waits for the device): the plan's levels and bytes, the last refit's launches,
 * and the out-of-range references skipped since the previous call (reset by it). All zero
 * before the first refit after a bind / set_config (a device bind or build installs the plan:
 * levels and plan_bytes are reported at once). */
int  mrt_tracer_refit_info(mrt_tracer* t, mrt_refit_info* info);

/* Blocking debug copy-out of the derived 4-wide array (device -> host), e.g. after a
 * refit: *bytes = its size (0 with cfg.wide 0); copied to out when out != NULL and
 * capacity suffices (else MRT_ERR_TOO_LARGE). mrt_tracer_bind_info tells its format. */
int  mrt_tracer_copy_wide_nodes(mrt_tracer* t, void* out, int64_t capacity, int64_t* bytes);

/* ---- device build (linear BVH) ------------------------------------------- */
/* Parameters of mrt_tracer_build (NULL = defaults). */
typedef struct mrt_build_params {
    int32_t max_leaf_size;     /* triangles per leaf at most: 1..8; 0 = default (MRT_LBVH_DEFAULT_MAX_LEAF) */
} mrt_build_params;
enum { MRT_LBVH_DEFAULT_MAX_LEAF = 4 };

/* What mrt_tracer_build_info reports about the last successful build. */
typedef struct mrt_build_info {
    double  wall_ms;           /* the whole call                                                        */
    double  plan_ms;           /* host: the emitted nodes copied back, the level plan, its upload       */
    double  bind_ms;           /* host: the bind (the 4-wide collapse, cfg.wide)                        */
    float   sort_ms;           /* device (events): centroid bounds, keys, the sort                      */
    float   emit_ms;           /* device: hierarchy, flags, prefix sums, emission                       */
    float   fit_ms;            /* device: Woop rows and boxes (the refit launches)                      */
    int32_t levels;            /* height levels of the tree (mrt_refit_info.levels)                     */
    int64_t records;           /* 64-byte node records written                                          */
    int64_t leaves;            /* leaves (the one-record tree's empty leaf included)                    */
    int64_t slots;             /* Woop slots = triIndex entries written: 3 * triangles + leaves         */
    int64_t scratch_bytes;     /* stream-ordered scratch taken and returned by the call                 */
    int64_t skipped_refs;      /* triangles with a vertex index out of range: zeroed rows, in no box    */
    int32_t max_leaf_size;     /* the value the build used                                              */
} mrt_build_info;

/* Host-only: upper bounds of what a build of numTriangles writes, the capacities
 * mrt_tracer_build asks for: numTriangles - 1 node records (at least one) of 64 bytes,
 * 4 * numTriangles + 1 Woop slots of 16 bytes, one triIndex int per slot.
 * MRT_ERR_INVALID_ARG for numTriangles < 1 or a null output, MRT_ERR_TOO_LARGE above the
 * refit's limits (2^28 slots: 67 108 863 triangles). */
int  mrt_lbvh_sizes(int64_t numTriangles, int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes);

/* Build a linear BVH on the device from vertices (3 floats each) and triangles (3 vertex
 * indices each), both DEVICE pointers, straight into the caller's Compact2 buffers nodes /
 * woop / triIndex (DEVICE pointers, borrowed as with mrt_tracer_bind; capacities in bytes, at
 * least mrt_lbvh_sizes), fill boxes and Woop rows, and bind the result: later traces and
 * refits work as after mrt_tracer_bind. *nodeBytes / *woopBytes / *triIndexBytes (host) = the
 * bytes written and bound. No reference counterpart (the reference builds on the CPU).
 *   - The tree: triangles sorted (stable, equal keys in index order) by the 63-bit Morton
 *     code of their box centres quantized to 21 bits per axis over the centres' bounds; the
 *     Karras 2012 hierarchy over the sorted keys (equal codes split by the bits of their
 *     sorted positions); a node is kept as a record iff it holds more than max_leaf_size
 *     triangles, a smaller child range is a leaf. Records are numbered in Karras order (the
 *     root is record 0), leaves by sorted position: the leaf of rank r starting at sorted
 *     position p owns Woop slots 3p + r onwards, its terminator included. At most
 *     max_leaf_size triangles give one record whose second child is an empty leaf with the
 *     first child's box. Boxes and Woop rows are what mrt_tracer_refit computes; the bytes
 *     equal mrth_bvh_build_lbvh's (mrt_host.h) and do not vary between runs.
 *   - Limits: the quality is below the SBVH's (no spatial splits, no SAH): traces are slower
 *     than on a mrth_bvh_build tree (DESIGN §10 has the measured ratio). mrt_tracer_optimize
 *     below lowers the built tree's inner-area sum by 11-12 % per round-1 call, but the primary
 *     trace followed only on hairball (0.99x after 1 round, 0.95x after 2) and not on bunny
 *     (1.01-1.09x); DESIGN §11 has the run. Coincident centres
 *     split by index bits, so the depth can exceed 63: the per-lane binary order
 *     (MRT_TRACE_LOCKSTEP_OFF, cfg.wide 0) then reports MRT_ERR_STACK_OVERFLOW as for any deep
 *     tree, while the wide orders size their stack at bind.
 *   - A triangle with a vertex index outside [0, numVertices) gets key 0, its vertices are
 *     never read, its Woop rows stay zero (no ray hits it), it is in no box, and it is counted
 *     (mrt_build_info.skipped_refs).
 *   - SYNCHRONOUS: the launches run on `stream` (a hipStream_t, NULL = the null stream), but
 *     the level plan of the emitted nodes is made on the host and the bind collapses them
 *     there too, so the call returns after the device has finished. Scratch (about 75 bytes
 *     per triangle) is taken and returned on the stream (hipMallocAsync / hipFreeAsync; a
 *     failed allocation is MRT_ERR_HIP).
 * Scalar arguments are checked first: MRT_ERR_INVALID_ARG for numTriangles < 1, numVertices
 * < 0 or max_leaf_size outside 0..8; MRT_ERR_TOO_LARGE for more triangles than mrt_lbvh_sizes
 * takes; then MRT_ERR_INVALID_ARG for a null pointer and MRT_ERR_TOO_LARGE for a capacity
 * below mrt_lbvh_sizes. In all these cases nothing is written and the previous bind stands. */
int  mrt_tracer_build(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                      int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity,
                      void* woop, int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity,
                      int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes, void* stream);

/* The last successful mrt_tracer_build of this handle (all zero before one). */
int  mrt_tracer_build_info(mrt_tracer* t, mrt_build_info* info);

/* ---- the refit plan and the 4-wide array derived on the device -------------------------- */
/* A tree of more depth levels than this is derived on the host instead (every pass of the
 * device derivation is one launch per depth level, or per run of small levels). */
enum { MRT_DERIVE_MAX_LEVELS = 1024 };

/* What mrt_tracer_derive_info reports about the last mrt_tracer_bind_device, mrt_tracer_build_device
 * or device-made refit plan of this handle (all zero before one). */
typedef struct mrt_derive_info {
    int32_t on_device_plan;    /* 1: the refit plan (height levels) was derived on the device; 0: on the
                                  host (a tree of more than MRT_DERIVE_MAX_LEVELS depth levels)          */
    int32_t on_device_wide;    /* 1: the 4-wide array and its source map were; 0: on the host (cfg.wide 2,
                                  the host fallback above) or none was derived (cfg.wide 0, a stack bound
                                  above 1024 entries)                                                    */
    int32_t levels;            /* height levels (mrt_refit_info.levels)                                  */
    int32_t depth_levels;      /* depth levels: the launches of a pass are at most this many             */
    int64_t wide_nodes;        /* 128-byte wide nodes written on the device                              */
    int32_t launches;          /* kernel launches of the derivation (the sort counts as one)             */
    int32_t readbacks;         /* host waits for a copy from the device: one fixed-size summary per
                                  topology launch, then a few summaries and 4 bytes per level             */
    float   topo_ms;           /* device (events): topology, heights, the sort                           */
    float   collapse_ms;       /* device: wide roots, sizes, numbers and the stack bound                 */
    float   emit_ms;           /* device: the wide nodes and the source map                              */
    double  wall_ms;           /* host wall time of the derivation (of the whole bind in a bind)         */
    int64_t scratch_bytes;     /* stream-ordered scratch taken and returned (48 bytes per node and the sort's)    */
} mrt_derive_info;

/* mrt_tracer_bind with the derived data made on the device: the same argument checks and effects
 * (the autotuner's schedules and the refit plan are forgotten), but no node array crosses to the
 * host. The launches run on `stream` (a hipStream_t, NULL = the null stream); the call returns
 * after the device has finished (the wide array's size is read back to allocate it).
 *   - The refit plan is derived and installed in every case, so the first mrt_tracer_refit copies
 *     nothing to the host and mrt_tracer_refit_info reports the levels at once.
 *   - cfg.wide 1: the exact 4-wide array, its source map and stack bound, byte for byte what
 *     mrt_tracer_bind derives (one collapse arithmetic, csrc/wide_common.hpp). cfg.wide 0: the
 *     plan only. cfg.wide 2: the plan on the device, the quantized array through
 *     mrt_tracer_bind's host path (mrt_derive_info.on_device_wide 0). A stack bound above 1024
 *     entries keeps the binary traversal, as mrt_tracer_bind does.
 *   - Every ref is checked on the device before it is followed. A tree that is none (a child ref
 *     outside the array or not a record's first float4, a record reached twice, a cycle, a record
 *     not reachable from node 0) is MRT_ERR_INVALID_ARG with mrt_refit_plan's reason, and the
 *     tracer is left UNBOUND.
 *   - More than MRT_DERIVE_MAX_LEVELS depth levels: everything through mrt_tracer_bind's host
 *     path (mrt_derive_info.on_device_plan 0). */
int  mrt_tracer_bind_device(mrt_tracer* t, const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                            const int32_t* triIndex, int64_t triIndexBytes, void* stream);

/* mrt_tracer_build (same arguments, checks, outputs and bytes written) with the level plan and the
 * bind's derived data made on the device: topology pass on the emitted nodes, the refit launches
 * with that plan, the collapse and emission, the bind, the plan kept for later refits. Still
 * blocking (the byte counts are return values), but no node array crosses to the host.
 * mrt_build_info.plan_ms and bind_ms are the host wall time of those phases. */
int  mrt_tracer_build_device(mrt_tracer* t, const float* vertices, int64_t numVertices, const int32_t* triangles,
                             int64_t numTriangles, const mrt_build_params* params, void* nodes, int64_t nodeCapacity,
                             void* woop, int64_t woopCapacity, int32_t* triIndex, int64_t triIndexCapacity,
                             int64_t* nodeBytes, int64_t* woopBytes, int64_t* triIndexBytes, void* stream);

int  mrt_tracer_derive_info(mrt_tracer* t, mrt_derive_info* info);

/* Blocking copy-out of the installed refit plan (device -> host), for tests and tools, in
 * mrt_refit_plan's shapes: order (nodeBytes / 64 entries, may be NULL), levelOffsets
 * (*numLevels + 1 entries; levelCapacity = entries it holds, MRT_ERR_TOO_LARGE when too few; may
 * be NULL), wideSrc (may be NULL; *numWideSrc entries, 0 without an exact wide array).
 * *numLevels = 0 when no plan is installed (before the first refit after a host bind). */
int  mrt_tracer_copy_refit_plan(mrt_tracer* t, int32_t* order, int64_t* levelOffsets, int32_t levelCapacity,
                                int32_t* numLevels, int32_t* wideSrc, int64_t wideSrcCapacity, int64_t* numWideSrc);

/* Host-only (no device): the refit plan of a Compact2 node array (host memory), as the
 * tracer builds it (csrc/refit_plan.cpp). order (nodeBytes / 64 entries, may be NULL): every
 * node once, grouped by height — a node whose children are both leaves has height 0, any
 * other 1 + the largest height of its inner children — level h at [levelOffsets[h],
 * levelOffsets[h + 1]) (*numLevels + 1 entries; levelCapacity = entries levelOffsets holds,
 * MRT_ERR_TOO_LARGE when too few; may be NULL). wideSrc (may be NULL): for the exact 4-wide
 * form, four entries per wide node, binaryNode * 2 + side = the Compact2 slot whose box
 * that wide child copies, -1 for an absent child, from the same collapse as
 * mrt_derive_wide_nodes form 1; *numWideSrc (may be NULL: no map) = its entries. Any valid
 * tree is accepted, whatever its numbering; MRT_ERR_INVALID_ARG for a child ref outside the
 * array, a record reached twice or a record not reachable from node 0. */
int  mrt_refit_plan(const void* nodes, int64_t nodeBytes, int32_t* order, int64_t* levelOffsets, int32_t levelCapacity,
                    int32_t* numLevels, int32_t* wideSrc, int64_t wideSrcCapacity, int64_t* numWideSrc);

/* ---- re-optimising the bound tree on the device (treelet restructuring) ----------------- */
enum { MRT_OPTIMIZE_MAX_ROUNDS = 8 };

/* Parameters of mrt_tracer_optimize (NULL = defaults). */
typedef struct mrt_optimize_params {
    int32_t rounds;            /* passes over the tree: 1..MRT_OPTIMIZE_MAX_ROUNDS; 0 = default (1)        */
} mrt_optimize_params;

/* What mrt_tracer_optimize_info reports about the last successful mrt_tracer_optimize. */
typedef struct mrt_optimize_info {
    int32_t rounds;            /* passes run                                                             */
    int32_t levels;            /* height levels of the tree as installed (mrt_refit_info.levels)         */
    int32_t launches;          /* restructuring launches of all passes: one per level above 64 records,
                                  one for the run of smaller levels (the derivations' are in
                                  mrt_derive_info)                                                       */
    int64_t considered[MRT_OPTIMIZE_MAX_ROUNDS];   /* per pass: records of height >= 1, one treelet each  */
    int64_t rewritten[MRT_OPTIMIZE_MAX_ROUNDS];    /* per pass: treelets whose records were rewritten     */
    float   device_ms;         /* device (events): the restructuring launches of all passes              */
    double  wall_ms;           /* host wall time of the whole call, derivations and install included     */
    int64_t scratch_bytes;     /* stream-ordered scratch of one derivation (mrt_derive_info.scratch_bytes)
                                  + the counters' 32 bytes                                               */
} mrt_optimize_info;

/* Re-optimise the topology of the bound Compact2 tree in place, on the device, by treelet
 * restructuring (Karras & Aila 2013; no reference counterpart): the cure for a device-built
 * tree's quality and for a tree that refits have degraded, without a host rebuild. The bound
 * nodes buffer must be writable, as for mrt_tracer_refit; woop and triIndex are not touched.
 *   - A pass derives the height levels on the device (as mrt_tracer_bind_device does, which
 *     also checks that the nodes are a tree) and then, level by level from height 1 up, forms
 *     below every record a treelet of at most 7 leaves, finds by exact dynamic programming over
 *     its 128 leaf subsets the binary topology of smallest summed inner-box area, and rewrites
 *     the treelet's records when that sum is strictly below the present one. Every rule and
 *     tie is csrc/treelet_common.hpp's; the bytes equal mrth_bvh_optimize's (mrt_host.h, which
 *     states what stays and which treelets are skipped) and do not vary between runs. One wave
 *     per treelet; one launch per level, one workgroup for the run of small levels; records of
 *     one level have disjoint subtrees, so no workgroup reads what another wrote in a launch.
 *   - After the last pass the refit plan, the exact 4-wide array, its source map and the
 *     stack bound are derived and installed exactly as mrt_tracer_bind_device does on the same
 *     buffers (cfg.wide 0 and 2 as there; mrt_derive_info describes it), so the next refit
 *     and trace work with no further step. Kept: the bind and the autotuner's schedules
 *     (the batches and kernels are the same; a trace's time on the new tree differs, and a
 *     caller may re-tune with mrt_tracer_set_config). Workspaces grow with the next trace if
 *     the stack bound grew (mrt_bind_info.stack_capacity). A tree that has MORE than
 *     MRT_DERIVE_MAX_LEVELS depth levels after a pass (none observed: passes shorten trees)
 *     ends the passes there and is installed through mrt_tracer_bind's host path, which
 *     forgets the schedules.
 *   - BLOCKING, like mrt_tracer_bind_device: the launches run on `stream` (a hipStream_t, NULL
 *     = the null stream) and the call returns after the device has finished. It first waits
 *     for this handle's own launches; a trace or refit of ANOTHER handle or a raw kernel that
 *     overlaps it on another stream reads a half-written tree: ordering those is the caller's.
 *   - What it buys is measured, not promised (tools/optimize_probe.py): one round
 *     takes 3.8 ms on bunny (50 664 records) and 21 ms on hairball (2.4 M), 1.7 and 15 ms of
 *     it on the device, and lowers the inner-area sum of a fresh LBVH to 0.89 / 0.88. The
 *     1024x768 primary trace on that tree went to 1.01x (bunny) and 0.99x (hairball) of the
 *     un-optimized LBVH's, 2 and 3 rounds to 1.09x / 1.05x and 0.95x / 0.96x: within the
 *     spread between settled schedules on bunny, so the default stays 1 round. On bunny
 *     refitted to vertices displaced by 10 % of its size: 0.93x after 1 round, 0.85x after 3;
 *     a fresh mrt_tracer_build_device of the moved vertices took 1.65 ms and gave 0.77x.
 * MRT_ERR_NOT_BOUND before a bind; MRT_ERR_INVALID_ARG for rounds outside 0..8 or bound nodes
 * that are not a tree; MRT_ERR_TOO_LARGE for a bound tree of more than MRT_DERIVE_MAX_LEVELS
 * depth levels (rebuild it, or optimise it with mrth_bvh_optimize and bind again). In all
 * these cases no byte of the tree is written and the bind, its derived data and the
 * schedules stand. */
int  mrt_tracer_optimize(mrt_tracer* t, const mrt_optimize_params* params, void* stream);

/* The last successful mrt_tracer_optimize of this handle (all zero before one). */
int  mrt_tracer_optimize_info(mrt_tracer* t, mrt_optimize_info* info);

/* Host-only (no device): the 4-wide node array a tracer derives at bind time
 * from a Compact2 node array (host memory). form 1 = exact child boxes, 128 B per
 * node; form 2 = child boxes quantized outward, 64 B per node (layouts in
 * csrc/wide_bvh.cpp). With the Woop array (host memory, may be NULL) the leaf refs
 * carry their triangle counts, as the tracer's own array does when the woop
 * indices fit 27 bits. *outBytes = the array's size; it is copied to out when
 * out != NULL and outCapacity suffices (else MRT_ERR_TOO_LARGE). Form 2 returns
 * MRT_ERR_INVALID_ARG when some box has no finite quantization. */
int  mrt_derive_wide_nodes(const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes, int32_t form,
                           void* out, int64_t outCapacity, int64_t* outBytes);

/* Diagnostics: run the EXACT variants' reciprocal (v_rcp_f32 + one FMA Newton step)
 * against the correctly rounded 1.0f / x for all 2^32 inputs on the current device;
 * *mismatches = number of differing bit patterns (0 expected). Blocking. */
int  mrt_selftest_exact_rcp(uint64_t* mismatches);

/* ---- device ray generation and hit counting (the trace's producers and consumer) ----
 * Stream-ordered on the calling thread's current HIP device. Buffers are device
 * pointers; the camera matrix and origin are host values. Per-ray arithmetic is
 * the host generator's (mrt_host.h mrth_primary_rays / mrth_ao_rays): primary
 * rays are bit-identical to it (device denormals flush to zero), AO/diffuse
 * directions agree to a few ulp (device cosf/sinf). */

/* RayGen::primary + rayGenPrimaryKernel (RayGen.cc:50-72, RayGenKernels.cu:79-113).
 * nscreenToWorld: column-major 4x4 (mrth_camera_nscreen_to_world). indexToPixel:
 * w*h pixel ids in trace order (mrth_pixel_table). slotToId/idToSlot may be NULL. */
int  mrt_raygen_primary(const float nscreenToWorld[16], const float origin[3], float maxDist, int32_t w, int32_t h,
                        const int32_t* indexToPixel, void* rays, int32_t* slotToId, int32_t* idToSlot, void* stream);

/* The same rays sampled at (jx, jy) in [0, 1)^2 inside each pixel instead of its centre
 * (0.5, 0.5): distinct, equally coherent batches of one view, e.g. one sample per rank
 * when a frame's rays are sharded over GPUs (bench.py). */
int  mrt_raygen_primary_subpixel(const float nscreenToWorld[16], const float origin[3], float maxDist, int32_t w,
                                 int32_t h, float jx, float jy, const int32_t* indexToPixel, void* rays,
                                 int32_t* slotToId, int32_t* idToSlot, void* stream);

/* RayGen::ao + rayGenAOKernel (RayGen.cc:77-120, RayGenKernels.cu:117-227): numSamples
 * hemisphere rays per input ray (origin backed off 1e-4 along the input ray, Halton
 * (2,3) samples rotated by a Jenkins hash of seed + ray index, tmax = -1 for input
 * misses). triNormals: 3 floats per triangle. Closest-hit use (diffuse): maxDist = far.
 * Input ids: -1 is a miss (normal (1, 0, 0), tmax = -1). Any other id outside [0, numTris) —
 * which the reference reads out of bounds — takes the normal (1, 0, 0) too and keeps tmax =
 * maxDist; triNormals is never read outside its numTris entries. (launch_rayGenAOKernel has no
 * numTris to pass: there every id but -1 must index triNormals, as in the reference.)
 * Edge values follow the reference's operations: a NaN t backs off by 0 (fmaxf), a zero normal
 * gives zero directions (normalize is v * rcp(length), rcp(0) = 0), a NaN normal NaN directions. */
int  mrt_raygen_ao(const void* inRays, const void* inResults, int32_t numInputRays, const float* triNormals,
                   int64_t numTris, int32_t numSamples, float maxDist, uint32_t seed, void* outRays,
                   int32_t* outIdToSlot, int32_t* outSlotToId, void* stream);

/* A whole frame's AO/diffuse rays, generated for a list of blocks of the frame's ray order
 * instead of batch by batch: the frame's RayGen::batching sequence (RayGen.cc:124-142) —
 * batch k = input rays [k*batchInputRays, (k+1)*batchInputRays), seeded by batchSeeds[k]
 * (host array, one glibc rand() per batch, RayGen.cc:106), numSamples rays per input ray
 * — numbers its rays g = input * numSamples + sample; output ray j is ray
 * blocks[j / blockRays] * blockRays + j % blockRays of it, bit-identical to the ray the
 * batches hold there (mrt_raygen_ao of batch k). blocks: device int32[numBlocks], any
 * order (e.g. a rank's shard, its costly blocks first). Only the frame's last block can
 * be partial; when listed it must be the last entry, and numOutRays = the listed rays
 * ((numBlocks-1)*blockRays + its length; else numBlocks*blockRays). Any number of batches
 * (the frame holds at most INT32_MAX rays): up to 256 batches travel in the kernel's arguments;
 * above that the seeds are written to scratch taken and returned on the stream
 * (hipMallocAsync / hipFreeAsync; a failed allocation is MRT_ERR_HIP) by one small fill launch
 * per 256 batches. Either way batchSeeds may be freed when the call returns, and the call is
 * stream-ordered without a host sync.
 * A block id outside [0, blocks in the frame) is not checked on the host (the list is device
 * memory): its output rays are left unwritten. */
int  mrt_raygen_ao_blocks(const void* inRays, const void* inResults, int32_t numInputRays, const float* triNormals,
                          int64_t numTris, int32_t numSamples, float maxDist, const uint32_t* batchSeeds,
                          int32_t numBatches, int32_t batchInputRays, const int32_t* blocks, int32_t numBlocks,
                          int32_t blockRays, int64_t numOutRays, void* outRays, void* stream);

/* One rank's blocks of a frame's AO/diffuse ray order for mrt_raygen_ao_blocks (multi-GPU
 * sharding: no reference counterpart — the reference is single-GPU). The frame's
 * numPrimary*numSamples rays are cut into blockRays-ray blocks, block i to rank i % world;
 * order 0 lists the rank's blocks in frame order, order 1 live blocks first: decreasing
 * number of live rays (samples whose primary ray hit, read from primaryResults — the primary
 * pass's RayResult[numPrimary]; a missed primary's samples are degenerate, tmax = -1), ties in
 * frame order, the frame's partial last block last (live counts quantized to 12 bits when
 * blockRays > 4094). Any number of blocks per rank that blocks[] holds (the frame: at most
 * INT32_MAX rays): a list of at most 16384 blocks is sorted by one workgroup in LDS, two launches
 * and no scratch; a longer one in 16384-entry tiles, four launches and 5 bytes per listed block + 16
 * KB per tile of scratch taken and returned on the stream (hipMallocAsync / hipFreeAsync; a
 * failed allocation is MRT_ERR_HIP). Before a tiled sort takes or launches anything the runtime is
 * asked (two pointer queries on the host, no sync) whether device-addressable memory of the rank's
 * blocks lies behind blocks (else MRT_ERR_TOO_LARGE, like a capacity that is too small) and of
 * numPrimary results behind primaryResults (else MRT_ERR_INVALID_ARG). blocks: device int32[capacity] (NULL: only *numBlocks /
 * *numRays are set; capacity below the rank's blocks: MRT_ERR_TOO_LARGE, nothing written);
 * *numBlocks and *numRays (host) = the rank's blocks and the rays they hold, known without the
 * device. Stream-ordered, no host sync. */
int  mrt_shard_blocks(const void* primaryResults, int32_t numPrimary, int32_t numSamples, int32_t blockRays,
                      int32_t world, int32_t rank, int32_t order, int32_t* blocks, int32_t capacity,
                      int32_t* numBlocks, int64_t* numRays, void* stream);

/* Parameters of mrt_ray_sort (NULL = defaults). */
typedef struct mrt_ray_sort_params {
    int32_t drop_levels;  /* 0..24, 0 = the reference's full key */
    int32_t box;          /* 0 = origins and end points (reference), 1 = origins only */
} mrt_ray_sort_params;

/* RayBuffer::mortonSort (RayBuffer.cc:256-324; findAABBKernel, genMortonKeysKernel and
 * reorderRaysKernel, RayBufferKernels.cu:74-200) without its two copies and its CPU sort: the
 * batch is put in the order of the reference's Morton key on the device. perm being that order,
 * outRays[j] = inRays[perm[j]] moved as bits, id = inSlotToId ? inSlotToId[perm[j]] : perm[j],
 * outSlotToId[j] = id, and outIdToSlot[id] = j where 0 <= id < numRays (an id outside that range
 * is never used as an index; the caller's contract, as in the reference, is a permutation).
 * outIdToSlot is what mrt_reconstruct takes as batchIdToSlot for the sorted batch's results.
 *   - The key (csrc/raysort_common.hpp; mrth_ray_sort, mrt_host.h, gives the same bits): the box
 *     lo / hi starts at +-FLT_MAX and takes every origin o and, with box 0, every end point
 *     o + d * tmax (a NaN never enters). Per axis a = (o - lo) / (hi - lo) and
 *     b = (d / |d| + 1) / 2 in IEEE float32 (the reference compiles these under fast-math, so its
 *     own bits are not defined), q = a * 2^24 capped at 2^24, r = b * 2^21 capped at 2^21, NaN and
 *     negative to 0. Bit 6 i + c of the key is bit i of component c of q.x, q.y, q.z, r.x, r.y,
 *     r.z (collectBits); six 32-bit words, word 5 most significant (0 with the caps).
 *     box 1 leaves the end points out: a diffuse batch's tmax is the camera's far distance, and
 *     its end points stretch the box until the origins share a few key levels.
 *   - The order: ascending by key >> (6 * drop_levels), ties by ascending input slot. The
 *     reference leaves ties to an unstable quicksort; a stable order is one of its outcomes and
 *     does not vary between runs. drop_levels d leaves the bit levels i < d of all six components
 *     out. The sort is LSD over the 64-bit words of the shifted key: three radix-sort passes for
 *     d <= 3, two for d <= 14, one above, each over the bits that can be set.
 *   - outKeys (may be NULL): six words per ray in INPUT order. outBox (may be NULL): lo.xyz,
 *     hi.xyz in device memory; the sign of a zero there may differ from mrth_ray_sort's.
 *   - Stream-ordered on `stream` (a hipStream_t, NULL = the null stream): no host sync and no
 *     readback. Scratch (about 60 bytes per ray, 24 less with outKeys) is taken and returned on
 *     the stream (hipMallocAsync / hipFreeAsync; a failed allocation is MRT_ERR_HIP).
 * numRays == 0 returns MRT_OK and launches nothing. MRT_ERR_INVALID_ARG for a negative count, a
 * null inRays or outRays, outRays overlapping inRays, or parameters out of range;
 * MRT_ERR_TOO_LARGE above 2^30 rays. In these cases nothing is written.
 * Whether the sort pays for itself is measured, not promised (tools/raysort_probe.py). */
int  mrt_ray_sort(const void* inRays, const int32_t* inSlotToId /* NULL = identity */, int32_t numRays,
                  const mrt_ray_sort_params* params /* NULL = defaults */, void* outRays,
                  int32_t* outIdToSlot /* may be NULL */, int32_t* outSlotToId /* may be NULL */,
                  uint32_t* outKeys /* may be NULL: 6 words per ray, in INPUT order */,
                  float* outBox /* may be NULL: lo.xyz, hi.xyz, device */, void* stream);

/* countHitsKernel (RendererKernels.cu:112-162): *hitCount (device int32) = number of
 * results with id >= 0. */
int  mrt_count_hits(const void* results, int32_t numRays, int32_t* hitCount, void* stream);

/* ray types of a batch (reference RayType_Primary / _AO / _Diffuse, App.cc); MRT_RAY_SHADOW is
 * the frame type of mrt_raygen_shadow / mrt_reconstruct_lit below, MRT_RAY_PATH that of
 * mrt_path_extend / _accumulate / _resolve (mrt_reconstruct refuses both) */
enum { MRT_RAY_PRIMARY = 0, MRT_RAY_AO = 1, MRT_RAY_DIFFUSE = 2, MRT_RAY_SHADOW = 3, MRT_RAY_PATH = 4 };

/* reconstructKernel (RendererKernels.cu:60-108; ReconstructInput RendererKernels.hh:46-61,
 * filled by Renderer.cc:421-445): one ABGR pixel per primary ray of the batch, at
 * pixels[primarySlotToId[firstPrimary + i]], i < numPrimary. Primary: shaded colour of
 * the hit triangle or the background (0.2, 0.4, 0.8); AO: the fraction of unblocked
 * rays (background where the primary missed); diffuse: the average shaded colour of
 * the bounce hits (white for misses) times the primary hit's material colour. Batch
 * rays of primary task i are batchIdToSlot[i * numRaysPerPrimary + k] (primary:
 * batchIdToSlot[pixel id]); batchIdToSlot NULL = identity layout (mrt_raygen_ao's).
 * Results are RayResult (16 B); colour tables one ABGR uint32 per triangle
 * (mrth_scene_tri_colors). Colour arithmetic is the reference's device code: float
 * sums in ray order, truncating toABGR.
 * The caller's contract, as in the reference: every id in primaryResults and batchResults lies
 * in [-1, entries of the colour tables); the kernels index the tables with it unguarded. */
int  mrt_reconstruct(int32_t rayType, int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                     const int32_t* primarySlotToId, const void* primaryResults, const int32_t* batchIdToSlot,
                     const void* batchResults, const uint32_t* triMaterialColor, const uint32_t* triShadedColor,
                     uint32_t* pixels, void* stream);

/* ---- an area light: shadow rays and direct lighting ----
 * RayGen::shadow + rayGenShadowKernel (RayGen.cc:147-183, which the reference leaves commented
 * out, and RayGenKernels.cu:231-293): numSamples rays per input ray from the traced point towards
 * samples of a light, for an any-hit trace; each ray's tmax is the distance to its own sample.
 *   - origin = o + d * max(t - 1e-4, 0) (a NaN t backs off by 0), as in mrt_raygen_ao.
 *   - Sample i of n: (sobol2D(i), (i + 0.5) / n) shifted by a per-ray offset (jenkinsMix twice over
 *     (seed + ray index, 0x9e3779b9, 0x9e3779b9), each word times 2^-32 after a round-to-nearest
 *     conversion, so an offset of exactly 1 occurs), wrapped once (`if (p >= 1) p -= 1`) and mapped
 *     to [-1, 1)^3: pos. target = light + lightRadius * pos: the samples fill a CUBE of half-side
 *     lightRadius, as in the reference. The ray index is the input ray's index within the call.
 *   - direction = (target - origin) * rcp(length), rcp(0) = 0: a sample on the origin gives a zero
 *     direction and tmax 0; a length that overflows to infinity gives a zero direction and tmax inf.
 *     tmin = 0; tmax = -1 where the input id is -1. No table is read: every other id gives a live ray.
 *   - Parity: the arithmetic is csrc/light_common.hpp's on both sides and this part of the library
 *     is built like mrt_scene_attributes' (no denormal flushing, no contraction, correctly rounded
 *     division and square root), so the rays equal mrth_shadow_rays' (mrt_host.h) bit for bit; only
 *     the bits of a NaN that an operation makes differ.
 * inRays / outRays must be 16-byte aligned (rays move as two 16-byte halves). outIdToSlot /
 * outSlotToId (may be NULL) get the identity. numInputRays == 0 returns MRT_OK and launches nothing;
 * a negative count, numSamples < 1 or a NULL required pointer is MRT_ERR_INVALID_ARG, more than
 * INT32_MAX output rays MRT_ERR_TOO_LARGE, and nothing is written. Stream-ordered, no host sync. */
int  mrt_raygen_shadow(const void* inRays, const void* inResults, int32_t numInputRays, int32_t numSamples,
                       const float light[3], float lightRadius, uint32_t seed, void* outRays, int32_t* outIdToSlot,
                       int32_t* outSlotToId, void* stream);

/* A whole frame's shadow rays for a list of blocks of the frame's ray order: mrt_raygen_ao_blocks'
 * contract exactly (batches, seeds, blocks, the partial last block, numOutRays, the seed table
 * above 256 batches, the checks and their order), with mrt_raygen_shadow's rays: output ray j is
 * bit-identical to the ray the batches hold at blocks[j / blockRays] * blockRays + j % blockRays. */
int  mrt_raygen_shadow_blocks(const void* inRays, const void* inResults, int32_t numInputRays, int32_t numSamples,
                              const float light[3], float lightRadius, const uint32_t* batchSeeds,
                              int32_t numBatches, int32_t batchInputRays, const int32_t* blocks, int32_t numBlocks,
                              int32_t blockRays, int64_t numOutRays, void* outRays, void* stream);

/* A shadow batch's pixels: one ABGR pixel per primary ray of the batch, at
 * pixels[primarySlotToId[firstPrimary + i]], i < numPrimary. A primary miss (id -1) gets the
 * background (0.2, 0.4, 0.8). Otherwise, with u of the primary's numRaysPerPrimary batch results
 * (batchIdToSlot[i * numRaysPerPrimary + k]; NULL = identity, mrt_raygen_shadow's layout) having
 * id -1 — shadow rays that reached their light samples — v = u * (1 / numRaysPerPrimary),
 * k = max(dot(nf, l), 0) with l the unit vector from the backed-off hit point to the light's
 * centre and nf the hit triangle's normal turned against the primary ray (a NaN gives 0), and the
 * pixel is (material.xyz * (k * v), 1) through the reference's device fromABGR / truncating toABGR
 * (RendererKernels.cu:38-56). primaryRays (16-byte aligned) are the rays primaryResults belong to.
 * The caller's contract, as in mrt_reconstruct: every primary id lies in [-1, entries of triNormals
 * and triMaterialColor). The arithmetic is csrc/light_common.hpp's: mrth_reconstruct_lit (mrt_host.h)
 * gives the same pixels bit for bit. numPrimary == 0 returns MRT_OK and launches nothing; a bad
 * shape or a NULL pointer (all but batchIdToSlot are required) is MRT_ERR_INVALID_ARG and nothing
 * is written. Stream-ordered, no host sync. */
int  mrt_reconstruct_lit(int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                         const int32_t* primarySlotToId, const void* primaryRays, const void* primaryResults,
                         const int32_t* batchIdToSlot, const void* batchResults, const float* triNormals,
                         const uint32_t* triMaterialColor, const float light[3], uint32_t* pixels, void* stream);

/* ---- multi-bounce diffuse paths with light sampling at every vertex ----
 * A path frame (MRT_RAY_PATH) carries S paths per primary ray through vertices 0 (the primary hit)
 * to depth. A path is one record per buffer at its SLOT: its current ray (Ray, 32 B), that ray's
 * result (RayResult, 16 B), and a 16-byte state {float throughput[3]; int32 task}. task is the path's
 * index in its batch, input ray * S + sample s, and names its entry of `radiance` (4 floats per
 * path: r, g, b, one unused). The caller zeroes radiance before vertex 0 and drives, per vertex b:
 *     mrt_path_extend(b)  ->  an any-hit trace of the shadow rays  ->  mrt_path_accumulate
 *                         ->  (b < depth) a closest-hit trace of the bounce rays  ->  b + 1
 * over *liveCount slots each, then mrt_path_resolve. All three are stream-ordered with no host sync.
 *
 * mrt_path_extend, slot i < numSlots. At vertex 0 the path is started: ray and result are
 * inRays / inResults[i / S] (the batch's input rays; no replicated copy is made), throughput
 * (1, 1, 1), task i; inState is not read. At vertex >= 1 ray, result and state are entry i of
 * inRays / inResults / inState, and a state whose task lies outside [0, numPaths) is no path: the
 * slot is dead and adds nothing. With (id, t) the result:
 *   - Miss: id outside [0, numTris) (so id -1). At vertex >= 1 radiance[task] += throughput * sky,
 *     channel by channel; at vertex 0 nothing is added (mrt_path_resolve writes the background where
 *     the primary's id is -1). The path ends.
 *   - Hit: the path survives. x = o + d * max(t - 1e-4, 0) (mrt_raygen_shadow's origin); nf =
 *     triNormals[id] turned against the ray (negated where dot(n, d) > 0); albedo = the first three
 *     channels of triMaterialColor[id] through the device fromABGR (byte * (1 / 255));
 *     throughput *= albedo.
 *   - Hash words: (a, b, c) = jenkinsMix twice over (seed + vertex * 0x9e3779b9 + key, 0x9e3779b9,
 *     0x9e3779b9) in uint32, key = i / S (the input ray's index) at vertex 0, so that a pixel's S
 *     paths share the offset and stay stratified, and key = task at vertex >= 1. A third jenkinsMix
 *     of the same three words gives (a', b', .).
 *   - Light sample: the shadow ray is mrt_raygen_shadow's ray for origin x, sample s of S and the
 *     offset (a, b, c) * 2^-32 (converted round-to-nearest, so an offset of exactly 1 occurs),
 *     towards the cube of half-side lightRadius round lightPos; tmax = the distance to the sample.
 *     At vertex 0 it is bit for bit the ray mrt_raygen_shadow makes for that input, sample and seed.
 *     Its pending contribution is throughput * lightColor * k per channel (in that order), k =
 *     mrt_reconstruct_lit's max(dot(nf, l), 0) towards the light's CENTRE: as there, the centre
 *     stands for the light and there is no distance falloff.
 *   - Bounce ray, only where vertex < depth: (h1, h2) = the Halton (2, 3) point of index s as
 *     mrt_raygen_ao computes it (radical inverses of s + 1); u1 = h1 + a' * 2^-32, u2 = h2 + b' * 2^-32,
 *     each wrapped once (`if (p >= 1) p -= 1`). cos and sin of 2 pi u2 without libm: v = 4 * u2,
 *     q = (int)v, f = v - q; where f > 0.5: f = f - 1, q = q + 1 (all exact); with g = f * f,
 *       S = f * (s1 + g * (s3 + g * (s5 + g * (s7 + g * s9)))),
 *       C = 1 + g * (c2 + g * (c4 + g * (c6 + g * (c8 + g * c10)))),
 *     s1.. = 1.5707963267948966, -0.6459640975062462, 0.07969262624616703, -0.004681754135318687,
 *     0.00016044118478735975 and c2.. = -1.2337005501361697, 0.253669507901048, -0.020863480763352957,
 *     0.0009192602748394263, -2.5202042373060596e-05 (the Taylor terms (pi/2)^k / k!, rounded to
 *     float32), and (cos, sin) = (C, S), (-S, C), (-C, -S), (S, -C) for q & 3 = 0, 1, 2, 3; within
 *     1e-6 of the true values (measured: DESIGN section 15). r = sqrt(u1), x = r * cos, y = r * sin,
 *     z = sqrt(max(1 - x * x - y * y, 0)). The tangents are mrt_raygen_ao's perp / biperp of nf
 *     (perp = (nf.y, -nf.x, 0), or (0, nf.z, -nf.y) where |nf.z| is the largest component, else
 *     (-nf.z, 0, nf.x) where |nf.x| is; normalized; biperp = cross(nf, perp)) WITHOUT its hash rotation:
 *     the shift already rotates. direction = normalize(perp * x + biperp * y + nf * z), origin x,
 *     tmin 0, tmax maxDist.
 * Estimator: cosine-weighted sampling of a Lambertian surface cancels the cosine and the 1 / pi, so
 * a bounce leaves throughput *= albedo and nothing else. Light and sky are in the units of
 * mrt_reconstruct_lit's k * v and of the background colour, not radiometric ones.
 * Output. compact != 0: survivor i's shadow ray, pending contribution (4 floats: r, g, b, 0), bounce
 * ray and new state go to entry rank(i) of outShadowRays / outPending / outRays / outState, rank(i)
 * = the number of survivors before i: stable order, the same from run to run, dense batches for both
 * traces. compact == 0 (in-place): every slot keeps its place; a slot that holds no survivor gets
 * rays with tmax -1 (all else 0), the state {0, 0, 0, task -1} and a zero pending, stays dead at
 * later vertices, and the caller goes on with numSlots slots. Both modes do the same arithmetic per
 * path: the radiance bits are equal. *liveCount (device int32) = the survivors, in both modes. In
 * compact mode every state of a vertex >= 1 must be a path (as the previous call left them). outRays
 * may be NULL at vertex == depth, where no bounce ray is written. Three launches, none waiting on
 * another workgroup: a count per 256 slots, a one-workgroup scan of the counts, the step itself; the
 * counts are scratch taken and returned on the stream (hipMallocAsync / hipFreeAsync; a failed
 * allocation is MRT_ERR_HIP).
 * Parity: the arithmetic is csrc/path_common.hpp's on both sides and this part of the library is
 * built like mrt_raygen_shadow's, so every output equals mrth_path_extend's (mrt_host.h) bit for
 * bit; only the bits of a NaN that an operation makes differ.
 * Checks, in this order, nothing written where one fails: NULL params; a negative numSlots or
 * numPaths, numSamples < 1, depth < 0 or vertex outside [0, depth] is MRT_ERR_INVALID_ARG; depth
 * above 64 or more than 2^22 slots or paths MRT_ERR_TOO_LARGE; numPaths < numSlots at vertex 0
 * MRT_ERR_INVALID_ARG; numSlots == 0 returns MRT_OK and launches nothing; then
 * MRT_ERR_INVALID_ARG for a NULL required pointer (all but inState at vertex 0 and outRays at
 * vertex == depth), numTris < 0, a ray buffer, state or pending buffer that is not 16-byte aligned,
 * or an output buffer that overlaps an input buffer or another output. */
typedef struct mrt_path_extend_params {
    int32_t vertex;              /* 0..depth */
    int32_t depth;               /* 0..64 */
    int32_t numSamples;          /* S */
    uint32_t seed;               /* the batch's */
    float lightPos[3];
    float lightRadius;
    float lightColor[3];
    float sky[3];
    float maxDist;               /* a bounce ray's tmax */
    int32_t compact;
    const float* triNormals;     /* 3 floats per triangle */
    const uint32_t* triMaterialColor;
    int64_t numTris;
    int32_t numSlots;
    int32_t numPaths;            /* entries of radiance */
    const void* inRays;
    const void* inResults;
    const void* inState;
    void* outShadowRays;
    void* outPending;
    void* outRays;
    void* outState;
    float* radiance;
    int32_t* liveCount;
} mrt_path_extend_params;
int  mrt_path_extend(const mrt_path_extend_params* params, void* stream);

/* After the shadow batch of a vertex is traced: radiance[task] += pending[i], channel by channel,
 * for every slot i < numSlots whose state's task lies in [0, numPaths) and whose shadow result has
 * id -1 (the ray reached its light sample). A path's additions thus happen in vertex order, each by
 * the one lane that holds the path: no float atomics, whose order would not be defined. Equals
 * mrth_path_accumulate bit for bit. numSlots == 0 returns MRT_OK and launches nothing; a negative
 * count, a NULL pointer or a state / pending / radiance buffer that is not 16-byte aligned is
 * MRT_ERR_INVALID_ARG, more than 2^22 slots or paths MRT_ERR_TOO_LARGE, and nothing is written. */
int  mrt_path_accumulate(int32_t numSlots, int32_t numPaths, const void* state, const void* pending,
                         const void* shadowResults, float* radiance, void* stream);

/* A path batch's pixels: per primary ray i < numPrimary of the batch, at pixel =
 * primarySlotToId[firstPrimary + i]: value = (sum of radiance[i * numSamples + s] over s in sample
 * order, from 0) * (1 / numSamples) per channel, alpha 1; pixels[pixel] = the value through the
 * truncating device toABGR; image (may be NULL; 4 floats per pixel, 16-byte aligned) gets the
 * unclamped value. Where primaryResults[firstPrimary + i] has id -1 the value is the background
 * (0.2, 0.4, 0.8, 1). Equals mrth_path_resolve bit for bit. numPrimary == 0 returns MRT_OK and
 * launches nothing; a bad shape or a NULL required pointer is MRT_ERR_INVALID_ARG, more than 2^22
 * paths MRT_ERR_TOO_LARGE, and nothing is written. */
int  mrt_path_resolve(int32_t numSamples, int32_t firstPrimary, int32_t numPrimary, const int32_t* primarySlotToId,
                      const void* primaryResults, const float* radiance, uint32_t* pixels, float* image,
                      void* stream);

/* ---- an edge-avoiding wavelet denoiser for path frames ----
 * An a-trous filter (Dammertz et al. 2010) over the float image mrt_path_resolve writes, run on the
 * albedo-demodulated image and guided by the primary hit's normal and position. Two calls: the
 * features of a frame's traced primary batch, then the filter. All arithmetic is float32, one IEEE
 * operation at a time in the order written here, with no fused multiply-add, no flushed denormal,
 * correctly rounded `/` and no libm call. dot(a, b) = ((0 + a.x * b.x) + a.y * b.y) + a.z * b.z.
 *
 * mrt_denoise_features, one lane per primary slot i < numPrimary: p = primarySlotToId[i]; a slot
 * whose p lies outside [0, numPixels) is skipped, nothing is read or written for it. With the
 * slot's ray (o, d) = primaryRays[i] and result (id, t) = primaryResults[i]:
 *   - Miss (id outside [0, numTris)): guide[p] = {0, 0, 0, 0, 0, 0, 0, 0}, albedo[p] = (1, 1, 1, 1).
 *   - Hit: nf = triNormals[id], negated where dot(nf, d) > 0 (mrt_path_extend's rule); x = o + d * t
 *     per component (one multiply, one add, no back-off); guide[p] = {nf.x, nf.y, nf.z, 1, x.x, x.y,
 *     x.z, 0} (8 floats, 32 bytes); albedo[p] = the first three channels of triMaterialColor[id]
 *     through the device fromABGR (byte * (1 / 255)), w = 1.
 * Pixels no slot names keep what guide and albedo held. Two slots that name one pixel are the
 * caller's error: the result is one of the two. Equals mrth_denoise_features bit for bit.
 * Checks, in this order, nothing written where one fails: a negative numPrimary, numTris or
 * numPixels is MRT_ERR_INVALID_ARG; more than 2^26 slots or pixels MRT_ERR_TOO_LARGE; numPrimary == 0
 * or numPixels == 0 returns MRT_OK and launches nothing; then MRT_ERR_INVALID_ARG for a NULL pointer
 * (the two tables may be NULL where numTris == 0), rays, results, guide or albedo not 16-byte
 * aligned, or guide or albedo overlapping an input or each other. */
int  mrt_denoise_features(int32_t numPrimary, const int32_t* primarySlotToId, const void* primaryRays,
                          const void* primaryResults, const float* triNormals, const uint32_t* triMaterialColor,
                          int64_t numTris, int32_t numPixels, void* guide, float* albedo, void* stream);

/* mrt_denoise_filter over a width x height frame, pixel p = y * width + x, hit(p) = guide[p].w != 0
 * (n_p, x_p: the guide's normal and position; image, albedo, scratch, imageOut: 4 floats per pixel).
 *  1. Demodulate: where hit(p), per channel r, g, b: c0 = (albedo > 0) ? image / albedo : 0; at a
 *     miss c0 = image. Channel w is carried unchanged from image to imageOut and takes no part.
 *  2. Iterations k = 0 .. iterations - 1 with step s = 1 << k. A miss pixel copies c_k to c_{k+1}.
 *     At a hit pixel p = (x, y): sum = (0, 0, 0), wsum = 0; for dy = -2 .. 2 (outer) and dx = -2 .. 2
 *     (inner), both ascending, q = (x + dx * s, y + dy * s); a tap whose q lies outside the frame or
 *     with !hit(q) is skipped; otherwise, the centre tap (dx = dy = 0) included:
 *         hw  = h[|dx|] * h[|dy|],  h = {0.375, 0.25, 0.0625}
 *         a   = dot(n_p, n_q);  a = (a > 0) ? a : 0  (a NaN becomes 0);  then a = a * a,
 *               normalSquarings times (7: the exponent 128)
 *         dpl = dot(n_p, x_q - x_p) * invPlane  (the difference per component);  wz = 1 / (1 + dpl * dpl)
 *         e   = c_k(q) - c_k(p);  dc2 = (e.x * e.x + e.y * e.y) + e.z * e.z;  wc = 1 / (1 + dc2 * invColor2[k])
 *         w   = ((hw * a) * wz) * wc;  sum += w * c_k(q) per channel (a multiply, then an add);  wsum += w
 *     c_{k+1}(p) = (wsum > 0) ? sum / wsum : c_k(p). The guard covers a degenerate triangle's zero
 *     normal (every weight 0) and a NaN weight sum.
 *  3. Remodulate: r = hit(p) ? c_N * albedo : c_N per channel; imageOut[p] = (r, image[p].w) where
 *     imageOut is given; pixels[p] = (r, 1) through the truncating device toABGR, as
 *     mrt_path_resolve's, where pixels is given.
 * Constants, computed once in float32: invPlane = 1 / sigmaPlane; invColor2[k] = 1 / (s_k * s_k) with
 * s_k = sigmaColor * 2^-k. A sigmaColor whose square overflows gives invColor2 = 0 (wc = 1: colour
 * takes no part); one whose square underflows to 0 gives infinity, the centre tap's 0 * infinity a
 * NaN weight, and the pixel keeps c_k. There is no exp and no pow.
 * One launch per iteration, each reading one image and writing another, so no workgroup waits on
 * another and there are no float atomics; demodulation is folded into the first launch's loads,
 * remodulation and the pixel write into the last launch's stores; iterations == 0 is one launch
 * of steps 1 and 3. Iteration k < iterations - 1 writes scratch[k & 1]: scratch[0] is needed from 2
 * iterations on, scratch[1] from 3 on; one that is not needed is ignored and may be NULL. Both calls
 * are stream-ordered, with no host sync, no readback and no allocation. A launch runs one of two
 * kernels with the same arithmetic: one loads every tap from global memory, one stages a tile of 64
 * columns by 4 rows a step apart, with its halo, in LDS (steps 1 .. 16). variant 0 takes the one
 * measured faster at each step, 1 the direct one everywhere, 2 the staged one
 * wherever it fits; the results do not depend on it.
 * Parity: the arithmetic is csrc/denoise_common.hpp's on both sides and this part of the library is
 * built like mrt_path_extend's, so imageOut and pixels equal mrth_denoise_filter's (mrt_host.h) bit
 * for bit; only the bits of a NaN that an operation makes differ.
 * Checks, in this order, nothing written where one fails: NULL params; width or height < 1, a
 * negative iterations or normalSquarings, a variant outside 0..2, or a sigmaColor or sigmaPlane that
 * is not above 0 (a NaN included) is MRT_ERR_INVALID_ARG; width * height above 2^26, iterations above 8 or normalSquarings
 * above 10 MRT_ERR_TOO_LARGE; then MRT_ERR_INVALID_ARG for a NULL image, guide, albedo or needed
 * scratch, for imageOut and pixels both NULL, for an image, guide, albedo, needed scratch or
 * imageOut that is not 16-byte aligned, or for a needed scratch, imageOut or pixels that overlaps an
 * input or another of them. */
typedef struct mrt_denoise_params {
    int32_t width;
    int32_t height;
    int32_t iterations;          /* 0..8 */
    int32_t normalSquarings;     /* 0..10 */
    float sigmaColor;            /* in units of the demodulated image */
    float sigmaPlane;            /* in scene units */
    int32_t variant;             /* 0: the kernel measured faster at each step; 1: direct loads; 2: LDS tiles */
    int32_t reserved;            /* 0 */
    const float* image;          /* mrt_path_resolve's float image */
    const void* guide;           /* mrt_denoise_features' */
    const float* albedo;
    float* scratch[2];
    float* imageOut;             /* may be NULL where pixels is given */
    uint32_t* pixels;            /* may be NULL where imageOut is given */
} mrt_denoise_params;
int  mrt_denoise_filter(const mrt_denoise_params* params, void* stream);

/* ---- a moving scene: normals, colours and the tree's cost on the device ---- */
/* Scene::Scene's per-triangle tables (reference Scene.cc:37,66-80) from vertices in DEVICE
 * memory: what mrt_raygen_ao / _ao_blocks read as triNormals and mrt_reconstruct as
 * triShadedColor / triMaterialColor, kept current beside mrt_tracer_refit without the vertices
 * crossing to the host. All pointers are device pointers on the calling thread's current device.
 *   - triNormals: normalize(cross(v1 - v0, v2 - v0)), normalize being a * rcp(length(a)) with
 *     rcp(0) = 0: a zero-area triangle gets the normal (0, 0, 0).
 *   - triShadedColor: diffuse.xyz * (dot(n, normalize(1, 2, 3)) * 0.5 + 0.5), alpha 1, through the
 *     host Vec4f::toABGR (Math.cc:45-52: in double, fixed point, its clamp sends a NaN channel to 0).
 *     triMaterialColor: toABGR(diffuse). triDiffuse: 4 floats per triangle (mrth_scene_tri_diffuse),
 *     NULL = the default material (0.75, 0.75, 0.75, 1; Mesh.hh:92).
 *   - Parity: the arithmetic is csrc/scene_common.hpp's on both sides, and this part of the
 *     library is built WITHOUT denormal flushing, without contraction or fast-math and with
 *     correctly rounded division and square root (mrt_raygen_primary's part flushes; this one
 *     does not). So every output equals mrth_scene_attributes' (mrt_host.h) bit for bit, denormal
 *     coordinates, edges and normals included, and no input is excepted on account of the denormal
 *     mode. The one difference is not arithmetic: the bits of a NaN that an operation makes (x86
 *     0xFFC00000, gfx950 0x7FC00000), so a normal that is NaN on one side (a NaN or infinite
 *     coordinate, an overflowing cross product) is NaN on the other with possibly other bits. The
 *     colours are integers and equal in every case.
 *   - A triangle with a vertex index outside [0, numVertices) never has that vertex read: it
 *     gets the normal (0, 0, 0), is shaded accordingly, and *skipped (device int64, may be NULL)
 *     is increased by one. The count is added to, never reset: clear it yourself.
 *   - One launch, one lane per triangle, stream-ordered on `stream` (a hipStream_t, NULL = the null
 *     stream): no host sync, no scratch, no readback. Outputs may be the tables a previous call
 *     wrote; every entry is rewritten.
 * numTriangles == 0 returns MRT_OK and launches nothing. MRT_ERR_INVALID_ARG for a negative count,
 * all three outputs NULL, or NULL vertices / triangles with numTriangles > 0; MRT_ERR_TOO_LARGE
 * above 67108863 triangles (mrt_tracer_refit's limit). In these cases nothing is written. */
int  mrt_scene_attributes(const float* vertices, int64_t numVertices, const int32_t* triangles, int64_t numTriangles,
                          const float* triDiffuse /* 4 floats per triangle; NULL = the default material */,
                          float* triNormals /* 3 per triangle, may be NULL */,
                          uint32_t* triShadedColor /* may be NULL */, uint32_t* triMaterialColor /* may be NULL */,
                          int64_t* skipped /* device, may be NULL: added to, not reset */, void* stream);

/* The area sums of the bound Compact2 tree: the terms of its SAH cost, for deciding whether a
 * refitted tree has degraded enough to rebuild (mrt_tracer_refit's Limits). Areas are half
 * surface areas dx*dy + dy*dz + dz*dx, the differences and products taken in double from the
 * float32 planes of the bound Compact2 records (the array a refit writes, not the 4-wide copy).
 * With Cn and Ct a platform's node and triangle costs,
 * SAH = (Cn * inner_area + Ct * leaf_tri_area) / root_area. */
typedef struct mrt_tree_cost {
    double root_area;      /* area of the union of record 0's two boxes                    */
    double inner_area;     /* sum over child slots that refer to a record, + root_area     */
    double leaf_area;      /* sum over child slots that refer to a leaf                    */
    double leaf_tri_area;  /* the same, each times its leaf's triangle count               */
    int64_t records, leaves, triangles;
    int64_t skipped;       /* slots whose area is not finite or whose box is inverted: in no sum */
} mrt_tree_cost;

/* Sums over every record of the bound array, two child slots each (a leaf's triangles: the walk
 * from its first Woop slot in steps of three to its terminator, as in a refit; a leaf ref is
 * followed only inside the Woop array). leaves and triangles count every leaf slot, skipped or
 * not; a root union that is not finite or inverted gives root_area 0 and counts in skipped.
 * One lane per slot, a reduction per wave, one partial per workgroup and a last step that adds
 * the partials in index order: no floating-point atomics, so two calls on the same tree give the
 * same bits. mrth_bvh_tree_cost (mrt_host.h) computes every slot's term with the same bits and
 * adds them in record order: the counts are equal and each sum agrees within records * 2^-52
 * relative (non-negative terms, two summation orders).
 *   host != NULL: blocking, one readback of 64 bytes after the work enqueued on `stream`.
 *   host == NULL, device != NULL (sizeof(mrt_tree_cost) bytes of device memory): stream-ordered,
 *   no host sync. With both, the device copy is written and then read back.
 * Scratch (48 bytes per 128 records) is taken and returned on the stream (hipMallocAsync /
 * hipFreeAsync; a failed allocation is MRT_ERR_HIP). Ordered after a refit enqueued on `stream`
 * before it. MRT_ERR_NOT_BOUND before a bind; MRT_ERR_INVALID_ARG with both outputs NULL. The
 * records are not checked to form a tree: child refs to records are counted, never followed. */
int  mrt_tracer_tree_cost(mrt_tracer* t, mrt_tree_cost* host /* may be NULL */,
                          void* device /* sizeof(mrt_tree_cost) of device memory, may be NULL */, void* stream);

/* ---- per-device convenience API (one implicit tracer per device) -------- */
int  mrt_bind_bvh(const void* nodes, int64_t nodeBytes, const void* woop, int64_t woopBytes,
                  const int32_t* triIndex, int64_t triIndexBytes);
int  mrt_unbind_bvh(void);
int  mrt_trace(const void* rays, void* results, int32_t numRays, int32_t anyHit, void* stream,
               float* outMs /* may be NULL: then asynchronous */);

/* Host-side introspection. */
const char* mrt_error_string(int err);
const char* mrt_last_error_detail(void);     /* thread-local text of the last failure */
int  mrt_version(void);                      /* 100 * major + minor                     */
int  mrt_device_count(void);

/* ---- reference-compatible entry points (same names, same arguments) ----
 * CudaTracerKernels.hh:44-52. Errors print "[file,line] (HIP error N: msg)"
 * and exit(-1) like cutilSafeCall. float4/int4/RayResult are passed as void*
 * and Vec2i& as a pointer to two int32 (ABI-identical). */
void  bind_CudaBVHTexture(void* nodeBuf, int64_t nodeBufSize, void* triWoopBuf, int64_t triWoopSize,
                          int32_t* triIndexBuf, int64_t triIndexSize);
void  unbind_CudaBVHTexture(void);
float launch_tracingKernel(int32_t nthreads, int32_t* blockSize, int numRays, bool anyHit,
                           void* rays, void* results,
                           void* nodesA, void* nodesB, void* nodesC, void* nodesD,
                           void* trisA, void* trisB, void* trisC, int32_t* triIndices);
void  copy_tracing_results(void* result_host, void* result_dev, int32_t size);

/* RendererKernels.hh:46-69 input structs, field for field (same C layout: three int32,
 * three bools, then 8-byte-aligned pointers). The reference passes them by C++
 * reference, which is ABI-identical to a pointer. Both launchers synchronise like
 * the reference's (cudaDeviceSynchronize) and ignore its launch-shape arguments. */
typedef struct mrt_reconstruct_input {
    int32_t   numRaysPerPrimary, firstPrimary, numPrimary;
    bool      isPrimary, isAO, isDiffuse;
    int32_t*  primarySlotToID;
    void*     primaryResults;
    int32_t*  batchIDToSlot;
    void*     batchResults;
    uint32_t* triMaterialColor;
    uint32_t* triShadedColor;
    uint32_t* pixels;
} mrt_reconstruct_input;

typedef struct mrt_count_hits_input {
    int32_t numRays;
    void*   rayResults;
    int32_t raysPerThread;
} mrt_count_hits_input;

/* RayGenKernels.hh:40-68 input structs, field for field: Vec3f = 3 floats, Mat4f =
 * 16 floats column-major, then 8-byte-aligned pointers. */
typedef struct mrt_raygen_primary_input {
    float    origin[3];
    float    nscreenToWorld[16];
    int32_t  w, h;
    float    maxDist;
    void*    rays;
    int32_t* idToSlot;
    int32_t* slotToID;
    int32_t* indexToPixel;
} mrt_raygen_primary_input;

typedef struct mrt_raygen_ao_input {
    int32_t  firstInputSlot, numInputRays, numSamples;
    float    maxDist;
    uint32_t randomSeed;
    void*    inRays;
    void*    inResults;
    void*    outRays;
    int32_t* outIDToSlot;
    int32_t* outSlotToID;
    void*    normals;          /* const Vec3f*: one per triangle, unbounded like the reference's */
} mrt_raygen_ao_input;

/* launch_rayGenPrimaryKernel / launch_rayGenAOKernel (RayGenKernels.cu:295-330); blocking */
void    launch_rayGenPrimaryKernel(int32_t nthreads, mrt_raygen_primary_input* in);
void    launch_rayGenAOKernel(int32_t nthreads, mrt_raygen_ao_input* in);

/* launch_reconstructKernel (RendererKernels.cu:166-186) */
void    launch_reconstructKernel(int32_t nthreads, mrt_reconstruct_input* in);
/* launch_countHitsKernel (RendererKernels.cu:189-215): returns the hit count */
int32_t launch_countHitsKernel(int32_t threads, const int32_t* blockSize, mrt_count_hits_input* in);

/* RayBufferKernels.hh:46-91 structs, field for field: Vec3f = 3 floats, then 8-byte-aligned
 * pointers (device memory). What a reference build with Renderer's sortSecondary on needs at
 * link time; mrt_ray_sort does the whole of RayBuffer::mortonSort without its two copies of the
 * keys and its CPU sort. */
typedef struct mrt_morton_key {
    int32_t  oldSlot;
    uint32_t hash[6];          /* hash[5] most significant */
} mrt_morton_key;

typedef struct mrt_find_aabb_input {
    int32_t  numRays;
    int32_t  raysPerThread;
    void*    inRays;
} mrt_find_aabb_input;

typedef struct mrt_find_aabb_output {
    float    aabbLo[3];
    float    aabbHi[3];
} mrt_find_aabb_output;

typedef struct mrt_gen_morton_keys_input {
    int32_t  numRays;
    float    aabbLo[3];
    float    aabbHi[3];
    void*    inRays;
    mrt_morton_key* outKeys;
} mrt_gen_morton_keys_input;

typedef struct mrt_reorder_rays_input {
    int32_t  numRays;
    mrt_morton_key* inKeys;
    void*    inRays;
    int32_t* inSlotToID;
    void*    outRays;
    int32_t* outIDToSlot;
    int32_t* outSlotToID;
} mrt_reorder_rays_input;

/* launch_findAABBKernel / launch_genMortonKeysKernel / launch_reorderRaysKernel
 * (RayBufferKernels.cu:204-255; prototypes RayBufferKernels.hh:112-117): blocking, the launch-shape
 * arguments are ignored. findAABB folds the rays' box (origins and end points) into *out, a HOST
 * struct the caller starts at +-FLT_MAX; genMortonKeys takes the box from *in and writes
 * {oldSlot = index, key} per ray; reorderRays reads oldSlot from the (sorted) keys and moves
 * rays and ids as mrt_ray_sort does (an oldSlot or id outside [0, numRays) is skipped). */
void    launch_findAABBKernel(int32_t nthreads, const int32_t* blockSize, mrt_find_aabb_input* in,
                              mrt_find_aabb_output* out);
void    launch_genMortonKeysKernel(int32_t nthreads, const int32_t* blockSize, mrt_gen_morton_keys_input* in);
void    launch_reorderRaysKernel(int32_t nthreads, mrt_reorder_rays_input* in);

#ifdef __cplusplus
}
#endif

#endif /* MRT_H */
