/*
 * saccot.h — C ABI of libsaccot.so: the SAC-COT compatibility-triangle sample-consensus hot path
 * on AMD Instinct MI355X (gfx950).
 *
 * What this replaces in the reference
 * -----------------------------------
 * The upstream tree (ytuhzq/SAC-COT) is a single file, /root/reference/README.md:1-2, which names the
 * algorithm ("SAC-COT: Sample Consensus by Sampling Compatibility Triangles in Graphs for 3-D Point Cloud
 * Registration") and ships no code, no FFI and no tests.  There is therefore no reference interface to
 * cite beyond README.md:2; the boundary below is the one fixed by BASELINE.json `north_star`
 * ("correspondence-in / (R,t,inlier-mask)-out", "thin C-ABI layer") and SURVEY.md §8(b).
 * Every entry point says which SURVEY §8(a) row it implements.
 *
 * Conventions
 * -----------
 *  - plain C types only; no C++ exception crosses this boundary; every function returns an int status
 *    (0 = SC_OK, negative = error) unless stated otherwise;
 *  - "host" entry points take host pointers and do the H2D/D2H copies themselves; "_device" entry points
 *    take device pointers (hipMalloc / torch CUDA tensors) and enqueue on the context's stream;
 *  - a context (`sc_ctx`) is bound to ONE GPU and ONE stream (one process per GPU).  Calls on one context
 *    must be serialised by the caller; distinct contexts are independent; there is no global mutable state;
 *  - device workspace is owned by the context, grows on demand, is never shrunk, and is freed by
 *    sc_destroy();  the library never keeps a caller pointer past the return of the call;
 *  - there is NO CPU fallback in this library: without a usable HIP device sc_create() fails with SC_EHIP.
 */
#ifndef SACCOT_H
#define SACCOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_VERSION_MAJOR 0
#define SC_VERSION_MINOR 10  /* 0.10, lanes: a directly enqueued host-free sc_register_device_async frame on a caller's stream runs on a private lane of its context, ordered after that stream at the call and before it at sc_wait (below; no entry or struct of this header changed; saccot_debug.h: sc_debug.no_lane took the struct's tail padding, sc_debug_info.reserved2 became `lane`, sc_debug_info grew n_lane).  0.10 + SC_HAS_POLISH: sc_polish / sc_polish_device / sc_polish_default_params (refits iterated to a fixed point on a scored frame; the minor number stays, callers detect the entries by symbol or by SC_HAS_POLISH).  0.10: sc_match / sc_match_device / sc_register_features (descriptor matching on the GPU, feeding the registration).  0.9: sc_peel / sc_peel_device / sc_register_instances (further rigid motions from a scored frame).  0.8: sc_debug_info grew cumulative counters of how a context's frames ran (saccot_debug.h); every entry refuses a context with an outstanding call; a host-free enqueue that does not fit the workspace cap runs the waited way.  0.7: sc_finalize_gathered_device_async (+ sc_wait), sc_hypothesize_device with SC_FLAG_EST_BOUND host-free on a repeated shape.  0.6: SC_FLAG_EST_BOUND also on sc_hypothesize_device (SC_EBOUND from the finalize call); SC_FLAG_SHARD_AB (sc_register_multi replicates stages A and B on small graphs unless told otherwise); sc_debug / sc_debug_info grew (the Gram filter's frame and cut: saccot_debug.h).  0.5: sc_register_device_async / sc_wait (host-free enqueue), SC_FLAG_EST_BOUND / SC_EBOUND (sharded stage B pruned by an estimated bound), sc_stats.bytes_moved, the debug hooks moved to
                                saccot_debug.h; 0.4: sc_debug_last / sc_debug_info, sc_debug.filter_blind; 0.3: sc_set_debug (no environment variables), SC_FLAG_NO_DENSE_S, sc_shard_* (stages A and B sharded); 0.2: SC_FLAG_TIMING_HOT,
                                SC_STREAM_DEFAULT, sc_hypothesize_begin/end_device, sc_finalize_gathered_device */

#define SC_HAS_POLISH 1  /* this header declares sc_polish* (added within 0.10) */
#define SC_HAS_BATCH 1   /* this header declares sc_register_batch* (added within 0.10) */
#define SC_HAS_MATCH_BATCH 1  /* this header declares sc_match_batch* and sc_register_batch_features* (added within 0.10) */
#define SC_HAS_POLISH_BATCH 1  /* this header declares sc_polish_batch* (added within 0.10) */
#define SC_HAS_INSTANCES_BATCH 1  /* this header declares sc_register_instances_batch* (added within 0.10) */
#define SC_HAS_PAIRS 1  /* this header declares sc_match_pairs*, sc_register_pairs_features* and sc_polish_pairs_slots_device (added within 0.10) */
#define SC_HAS_POSE_INFO 1  /* this header declares sc_pose_info_batch* and sc_pose_info_pairs_slots_device (added within 0.10) */
#define SC_HAS_POSE_INFO_FRAME 1  /* this header declares sc_pose_info_frame* and sc_pose_info_default_params (added within 0.10) */
#define SC_HAS_POLISH_POSES 1  /* this header declares sc_polish_poses* (added within 0.10) */
#define SC_HAS_ASSIGN 1  /* this header declares sc_assign_poses* and sc_assign_default_params (added within 0.10) */
#define SC_HAS_SETTLE 1  /* this header declares sc_settle_poses* and sc_settle_default_params (added within 0.10) */
#define SC_HAS_MERGE 1  /* this header declares sc_merge_poses* and sc_merge_default_params (added within 0.10) */
#define SC_HAS_PAIRS_CYCLES 1  /* this header declares sc_pairs_cycles*, sc_cycles_default_params and sc_cycles_thresholds (added within 0.10) */
#define SC_HAS_PAIRS_SYNC 1  /* this header declares sc_pairs_sync*, sc_sync_default_params and sc_sync_thresholds (added within 0.10) */
#define SC_HAS_PAIRS_SOLVE 1  /* this header declares sc_pairs_solve*, sc_solve_default_params and sc_solve_thresholds (added within 0.10) */
#define SC_HAS_MATCH_GUIDED 1  /* this header declares sc_match_guided*, sc_register_guided_features and sc_guide_default_params (added within 0.10) */
#define SC_HAS_MATCH_GUIDED_POSES 1  /* this header declares sc_match_guided_poses*, sc_register_guided_poses_features and SC_GUIDE_MAX_POSES (added within 0.10) */
#define SC_HAS_MATCH_GUIDED_BATCH 1  /* this header declares sc_match_guided_batch*, sc_match_guided_pairs* and sc_register_guided_{batch,pairs}_features_device (added within 0.10) */

/* status codes */
#define SC_OK        0
#define SC_EINVAL   -1   /* bad argument: n < 3, null pointer, non-finite input, bad params.size ...        */
#define SC_ENOMEM   -2   /* device or host allocation failed / workspace cap exceeded                       */
#define SC_EHIP     -3   /* HIP runtime error (sc_last_error() has the string)                              */
#define SC_ERCCL    -4   /* RCCL error or librccl.so.1 not loadable (sc_create_multi / sc_register_multi)   */
#define SC_ENOHYP   -5   /* no compatibility triangle / every inlier count is 0: R = I, t = 0, mask = 0     */
#define SC_ETOOMANY -6   /* the graph has more triangles than the workspace cap can rank (see max_workspace),  */
                         /* or 2^32 or more edges (edge ids are 32-bit)                                      */

#define SC_EBOUND   -8   /* calls made with SC_FLAG_EST_BOUND only: the ESTIMATED pruning bound was too high (the merged           */
                        /* candidates hold fewer than T keys above it) — or, sc_hypothesize_device, a host-free enqueue did not */
                        /* cover this input's counts: nothing was returned; repeat the call(s) WITHOUT the flag                */
#define SC_ERETRY   -7   /* sharded stages A + B only: a rank's candidate blob was too small for this input (its    */
                         /* list was cut at a key the merged threshold does not clear).  Outputs are not valid;    */
                         /* repeat the call on every rank with sc_params.shard_cand_level raised by one (every     */
                         /* rank sees the same blobs, so every rank returns it together).  sc_register_multi does  */
                         /* this by itself.                                                                        */

/* Limits: 3 <= n <= 2^24; max_triangles <= 2^32 - 256; the compatibility graph must have fewer than 2^32 edges
 * (SC_ETOOMANY otherwise; with the default 64 GiB workspace cap a dense graph runs out of workspace long before). */

/* point layouts for `src` / `tgt` */
#define SC_AOS 0   /* N x 3 row-major: x0 y0 z0 x1 y1 z1 ...                                   */
#define SC_SOA 1   /* 3 planes of N: x[0..N) y[0..N) z[0..N)  (a MATLAB N x 3 column-major array) */

/* triangle ranking */
#define SC_RANK_WEIGHT 0   /* w = (s_ij + s_ik) + s_jk, fp32, descending                     */
#define SC_RANK_DEGREE 1   /* deg_i + deg_j + deg_k, u32, descending                         */

/* hypothesis scoring (SURVEY §8f-2 `score_mode`).  The winner is the hypothesis with the largest score, ties as before
 * (best ranking key, then lowest (i,j,k)); the inlier MASK is always the test |R p + t - q| < tau.  The truncated
 * scores are sums of per-correspondence integers (10 fractional bits), so they are exact, order-free sums:
 *   SC_SCORE_MSE:  sum over n of  floor(1024 * max(0, 1 - d2_n / tau^2))      (MSAC: truncated squared residual)
 *   SC_SCORE_MAE:  sum over n of  floor(1024 * max(0, 1 - d_n / tau)),  d_n = sqrt(d2_n)  (truncated absolute residual)
 * with d2_n the canonical squared residual, 1 / tau^2 and 1 / tau rounded once from fp64, the product by fma. */
#define SC_SCORE_COUNT 0   /* number of inliers (default)                                      */
#define SC_SCORE_MSE   1
#define SC_SCORE_MAE   2

/* flags */
#define SC_FLAG_TIMING       1u /* record a HIP event pair around every stage and fill sc_stats.us_* (each record  */
                                /* costs ~5 us of stream time: diagnostics, not for the timed loop)               */
#define SC_FLAG_TIMING_HOT  16u /* only the dominant kernel: us_score (2 records per call)                          */
#define SC_FLAG_TIMING_ONE  64u /* ONE stage bracket (2 records per call), chosen by SC_TIMING_STAGE(k) in the flags: the   */
                                /* call runs its hot path (speculative launches on), so per-stage times taken one stage per   */
                                /* pass are times of the code that is actually timed end to end                                */
#define SC_TIMING_STAGE(k)  (((uint32_t)(k) & 15u) << 8) /* k: 0 staging, 1 compat, 2 triangles, 3 kabsch, 4 score, 5 argmax, 6 mask */
#define SC_FLAG_EXACT_TOTAL  2u /* sc_stats.tri_total = 3-cliques of the WHOLE graph (one extra counting pass);  */
                                /* default: 3-cliques of the pruned graph the top-T search actually enumerated   */
#define SC_FLAG_REFINE       8u /* after C3, replace (R,t) by the fp64 least-squares refit over the winner's inlier  */
                                /* mask; the mask itself stays the fp32 winner's                   */
#define SC_FLAG_NO_PRUNE     4u /* disable the certified pruning of stage B (results are identical either way)    */
#define SC_FLAG_EST_BOUND  128u /* phase API sc_shard_* only (sc_register / sc_register_device / sc_register_multi do this by themselves): */
                                /* stage B prunes by a bound ESTIMATED from a 1-in-64 sample of the graph's triangles instead of a      */
                                /* certified one.  EVERY rank takes the whole (cheap) sample, so sc_shard_edges_device leaves the same    */
                                /* histogram on every rank and the all-reduce after it MUST BE SKIPPED — three collectives per call, not  */
                                /* four.  The merge verifies the bound; when it was too high the finalize call returns SC_EBOUND on every  */
                                /* rank (nothing returned): repeat the call without this flag.  Results are identical either way.         */
                                /* Also taken by sc_hypothesize_device (stages A and B replicated on every rank; NOT by the _begin / _end   */
                                /* pair, whose shared histogram is a certifying sample's): sc_finalize_device / _gathered_device then      */
                                /* returns SC_EBOUND when the select found the bound too high — on every rank alike (the estimate is a      */
                                /* function of the input).  A HOST-FREE enqueue that outgrew its covers comes back as SC_EBOUND too, and     */
                                /* whether a rank enqueues host-free, and what its launches cover, follows from the history of ITS context:  */
                                /* ranks whose contexts have seen the same calls in the same order (bench.py's, sc_register_multi's) fail    */
                                /* together; a caller whose ranks may differ (a context recreated or warmed up differently) must AGREE on   */
                                /* the status before it repeats — any rank's SC_EBOUND means every rank repeats (sc_register_multi does).    */
#define SC_FLAG_SHARD_AB 4096u /* sc_register_multi only: shard stages A and B over the devices at EVERY size.  By default it does so from   */
                                /* 8192 correspondences on; below, every device runs stages A and B for the whole job (pruned by the      */
                                /* estimated bound) and scores its share — one 16-byte exchange per call instead of three collectives.    */
                                /* Results are identical either way.                                                                    */
#define SC_FLAG_NO_DENSE_S  32u /* stage A writes only the adjacency bit rows, not the dense n x n weight matrix S:   */
                                /* nothing after stage A reads S (edge weights are recomputed from the points), so    */
                                /* every result is identical; sc_compat_host returns S only without this flag         */

typedef struct sc_ctx sc_ctx;

/* All tunables of the path (SURVEY §8a `sc_params`).  POD; `size` must be sizeof(sc_params).
 * Numeric domain: any finite coordinate, any positive finite sigma / tau, min_len >= 0, 0 < t_cmp < 1 is accepted and
 * computed as the CPU restatement computes it, bit for bit.  The units of length are free within limits: multiplying the coordinates
 * and sigma, tau, min_len by 2^k leaves the graph, the ranked list, R, the scores, the mask and the winner unchanged and multiplies t by
 * 2^k exactly, as long as the SQUARED lengths the path compares stay normal fp32 numbers — for pair lengths, tau and min_len between
 * ~1e-18 and ~4e18 and sigma above ~1e-15 they do (a scene of extent 1 with sigma = tau = min_len = 0.05: -46 <= k <= 62; adjacency and inlier counts alone
 * from k = -58; the Kabsch stage normalises its triangle and holds from -80 to 120).  Outside nothing fails: a pair whose squared
 * length overflows is no edge, so the graph thins out and in the end the call returns SC_ENOHYP; squared lengths that underflow lose
 * bits or vanish, and results drift from the scale-covariant ones. */
typedef struct sc_params {
  uint32_t size;            /* = sizeof(sc_params); versioning                                          */
  float    sigma;           /* rigidity scale: s_ij = exp(-d^2 / (2 sigma^2)), d = | |pi-pj| - |qi-qj| | */
  float    t_cmp;           /* edge iff s_ij >= t_cmp  <=>  d <= sigma*sqrt(-2 ln t_cmp); in (0,1)       */
  float    tau;             /* inlier distance: |R p + t - q| < tau                                     */
  float    min_len;         /* edge additionally needs |pi-pj| >= min_len and |qi-qj| >= min_len        */
  uint32_t max_triangles;   /* T: hypotheses scored = top-T ranked compatibility triangles              */
  int32_t  rank_mode;       /* SC_RANK_WEIGHT / SC_RANK_DEGREE                                          */
  int32_t  layout;          /* SC_AOS / SC_SOA                                                          */
  int32_t  shard_rank;      /* this GPU's rank in [0, shard_world)                                      */
  int32_t  shard_world;     /* number of GPUs sharing the T hypotheses (1 = no sharding)                */
  uint32_t shard_block;     /* ranked triangles are dealt round-robin in blocks of this many (0 -> 1024) */
  uint32_t flags;           /* SC_FLAG_*                                                                */
  uint64_t max_workspace;   /* cap in bytes on the device workspace (0 -> 64 GiB)                       */
  int32_t  score_mode;      /* SC_SCORE_COUNT / SC_SCORE_MSE / SC_SCORE_MAE                             */
  int32_t  shard_cand_level;/* sharded A + B: a candidate blob holds max(2T/world, 4096) << level entries (<= T):    */
                            /* 0, raised by one after SC_ERETRY; negative values shrink the blob (tests)             */
} sc_params;

/* Per-call statistics (all optional: pass NULL).  Times are device times from HIP events on the
 * context's stream (each bracket minus the cost of one event record, calibrated once per context and stream), only filled when SC_FLAG_TIMING / SC_FLAG_TIMING_HOT is set, and delivered by the call
 * that ends the path (sc_register, sc_register_device, sc_finalize_device): sc_hypothesize_device never waits
 * for the GPU at its end, so the us_* fields of ITS stats stay 0. */
typedef struct sc_stats {
  uint32_t size;            /* = sizeof(sc_stats)                                                       */
  uint32_t n;               /* correspondences                                                          */
  uint64_t edges;           /* undirected edges of the compatibility graph                              */
  uint64_t tri_total;       /* 3-cliques enumerated (whole graph with SC_FLAG_EXACT_TOTAL / NO_PRUNE)   */
  uint32_t tri_kept;        /* T_eff = min(T, tri_total)                                                */
  uint32_t tri_scored;      /* hypotheses scored by THIS rank                                           */
  uint32_t best_rank;       /* rank index (0-based) of the winning triangle in the ranked list          */
  uint32_t best_count;      /* its score: the inlier count, or the truncated score of params.score_mode   */
  float    us_stage;        /* input staging (layout -> padded planes, finiteness check)                */
  float    us_compat;       /* stage A: the compat_rows kernel alone                                    */
  float    us_triangles;    /* stage B: every kernel of it plus its two 8-byte read-backs               */
  float    us_trikeys;      /* stage B: the tri_keys kernel alone (part of us_triangles)                */
  float    us_kabsch;       /* stage C1                                                                 */
  float    us_score;        /* stage C2: the score kernel alone                                         */
  float    us_argmax;       /* stage C2: partial-count reduction + arg-max key                          */
  float    us_mask;         /* stage C3: winner re-solve + mask                                         */
  float    us_total;        /* sum of the above                                                         */
  uint64_t workspace_bytes; /* device bytes currently held by the context                               */
  uint64_t bytes_moved;     /* ALGORITHMIC bytes this call's kernels read and wrote in device memory, from the counts of   */
                            /* the call (SURVEY §5 / §8d formulas: stage A 4n^2 + n^2/8 + 24n (n^2/8 + 24n without S),   */
                            /* stage B n^2/8 + 20 E + 12 M + 16 T_eff, stage C 52 T_scored + 24 n + n): a yardstick for    */
                            /* achieved-bandwidth figures, not a hardware counter                                          */
} sc_stats;

/* ---- library ---------------------------------------------------------------------------------- */
int         sc_version(void);                 /* (major << 16) | minor                               */
const char* sc_strerror(int status);          /* static string, never NULL                           */
void        sc_default_params(sc_params* p);  /* size set, sigma = tau = min_len = 0.1, t_cmp = 0.9,
                                                 T = 50000, weight ranking, AOS, no sharding          */

/* ---- context ---------------------------------------------------------------------------------- */
int         sc_create(int device, sc_ctx** out);      /* binds `device`, creates a private stream    */
void        sc_destroy(sc_ctx* ctx);                   /* frees the workspace; NULL is a no-op        */
int         sc_set_stream(sc_ctx* ctx, void* hip_stream); /* enqueue on a caller stream (e.g. torch's
                                                 current stream) instead of the private one, so that the
                                                 caller's own work on that stream (an all-reduce of d_key,
                                                 a copy of d_mask) is ordered with the kernels.  NULL
                                                 restores the private stream, which is NON-blocking: nothing
                                                 orders it against other streams.  The device's default
                                                 (null) stream has no handle of its own: pass
                                                 SC_STREAM_DEFAULT for it (torch reports it as 0).
                                                 One kind of call is ordered with that stream at its two
                                                 ends only, not inside it: a frame of a direct
                                                 sc_register_device_async call (below) follows everything
                                                 enqueued on the stream before the call, precedes everything
                                                 enqueued after its sc_wait, and may run CONCURRENTLY with
                                                 what the caller enqueues there in between                */
#define SC_STREAM_DEFAULT ((void*)1)
const char* sc_last_error(const sc_ctx* ctx);          /* last HIP error text seen by this context    */

/* Test / tuning hooks (sc_set_debug, sc_debug_last) are NOT part of the drop-in surface: include/saccot_debug.h. */

/* ---- the drop-in entry point: correspondences in, (R, t, inlier mask) out ------------------------
 * north_star: "keeping the reference's correspondence-in / (R,t,inlier-mask)-out function signature".
 * Runs A (compat graph) -> B (ranked triangles) -> C1 (Kabsch) -> C2 (score, arg-max) -> C3 (mask) on the
 * GPU.  src/tgt: n points each, fp32, `params->layout`; row m of src corresponds to row m of tgt.
 * R: 3x3 row-major, t: 3, mask: n bytes (0/1), all caller-allocated HOST memory.  q ~ R p + t.
 * Requires shard_world == 1 (multi-GPU callers use the two-phase form below). */
int sc_register(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                float R[9], float t[3], uint8_t* mask, sc_stats* stats);

/* Same, with every buffer already resident in HBM (d_Rt: 12 floats = R row-major then t).  Output visibility as
 * for sc_finalize_device below: complete on return with the private stream, stream-ordered with a caller stream. */
int sc_register_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, int64_t n,
                       const sc_params* params, float* d_Rt, uint8_t* d_mask, sc_stats* stats);

/* The same call in two halves, for callers that register a STREAM of frames: sc_register_device_async enqueues the
 * whole path on the context's stream and returns without waiting for the GPU; sc_wait delivers the status and the
 * statistics of that call (and is where the host first looks at anything the GPU produced).  Between the two the host
 * is free — e.g. to enqueue the next frame on a SECOND context bound to the same stream (sc_set_stream): the GPU then
 * never waits for the host, and the two frames OVERLAP on it.  At most ONE call may be outstanding per context
 * (SC_EINVAL otherwise); d_src / d_tgt must stay valid and unchanged until sc_wait returns, d_Rt / d_mask are complete
 * when it does (as for sc_register_device).
 * Ordering on a caller's stream (sc_set_stream): the frame is ordered AFTER everything enqueued on that stream before
 * sc_register_device_async was called (the producers of d_src / d_tgt, earlier readers of d_Rt / d_mask) and BEFORE everything
 * enqueued on it after sc_wait has returned (copies of d_mask, sc_peel / sc_polish*, the next frame).  Between the two calls
 * its kernels do not sit in that stream: a host-free frame (below) runs on a private lane of the context beside it, and may run
 * concurrently with whatever the caller enqueues on the stream in that window — which therefore must not touch the four
 * buffers, as the rule above already says.  Work on the stream that has to FOLLOW the frame is enqueued after sc_wait.
 * How it can return early: a call whose shape (n, parameters) equals the previous call's on this context is enqueued
 * "host-free" — its launches are sized by what the previous call needed (plus slack) and read the two data-dependent
 * counts of stage B (edges, triangles of the pruned graph) from device memory instead of from the host.  sc_wait
 * validates: had a count outgrown what the launches covered (or had any other of the waiting path's fallbacks been
 * needed), it repeats the call the waiting way before it returns — results are identical either way, bit for bit.
 * The first call on a context, and every call whose shape differs from the one before, simply waits inside
 * sc_register_device_async as sc_register_device always did.  sc_register_device is async + wait. */
int sc_register_device_async(sc_ctx* ctx, const float* d_src, const float* d_tgt, int64_t n,
                             const sc_params* params, float* d_Rt, uint8_t* d_mask);
int sc_wait(sc_ctx* ctx, sc_stats* stats);

/* ---- many small registrations in one launch: sc_register_batch ---------------------------------------------
 * sc_register is a chain of about 35 dependent launches: well filled by 5000 correspondences, almost pure launch latency for a few
 * hundred.  Small problems arriving by the thousand — object-pose candidates of a camera frame, fragment pairs with 250 - 500
 * keypoints, the cluster pairs of a place-recognition back end — go through ONE launch here, a workgroup per problem, every stage
 * of the path inside it (sc_batch.hip).  No host read-back, no launch sized by the data, nothing shared between problems.
 *
 * Layout: the problems are PACKED.  Problem b owns rows [offset[b], offset[b + 1]) of src / tgt — params->layout SC_AOS: total x 3
 * row-major; SC_SOA: three planes of total, total = offset[n_problems] — and the same range of mask (total bytes).  offset is a HOST
 * array of n_problems + 1 words in BOTH forms (the caller knows its sizes); the library copies it and keeps no caller pointer.  One
 * sc_params serves the whole batch.  3 <= n_b = offset[b + 1] - offset[b] <= SC_BATCH_MAX_N.
 *
 * Semantics: for every problem b the record's status, Rt, edges, tri_total, tri_kept, best_rank, best_count and the mask range equal
 * what sc_register(ctx, problem b alone, n_b, the same params plus SC_FLAG_EXACT_TOTAL) returns, bit for bit, in either ranking mode
 * and all three score modes.
 *   - SC_ENOHYP (no triangle, or no hypothesis with a score): R = I, t = 0, mask zero, the counts as sc_register reports them.
 *   - A problem that holds a non-finite coordinate gets status SC_EINVAL, R = I, t = 0, mask zero, every count 0 (n stays n_b).  It is
 *     found on the device, does not disturb its neighbours and does not fail the call.
 *   - A problem's record is a function of its own points and the parameters only: not of its position in the batch, of n_problems, of
 *     the other problems, or of the context's history.
 *   - The CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument;
 *     n_problems == 0; an n_b < 3 or > SC_BATCH_MAX_N; offsets that decrease, or a total above 2^31; shard_world != 1; any flag other
 *     than SC_FLAG_NO_DENSE_S, SC_FLAG_NO_PRUNE, SC_FLAG_EXACT_TOTAL (result-neutral: accepted and ignored) — SC_FLAG_REFINE, the timing
 *     flags, SC_FLAG_EST_BOUND, SC_FLAG_SHARD_AB are refused: the fp64 refit is not part of a batch member's path (it is a launch of
 *     its own behind it: sc_polish_batch); the usual sc_params
 *     checks; a call outstanding on the context.
 *   - max_triangles may be anything sc_register accepts: nothing is materialised per hypothesis, so SC_ETOOMANY cannot occur.
 *   - sc_register_batch_device enqueues on the context's stream and returns without waiting, like sc_match_device: d_res and d_mask are
 *     complete in stream order.  (It may wait for the previous batch call's copy of ITS offsets out of the staging area the two share.)
 *     sc_register_batch copies in, enqueues, copies out and waits.
 *   - The call ends the frame a context may hold and leaves none: sc_peel / sc_polish after it return SC_EINVAL.
 *   - Workspace: the copy of offset, plus the host form's device copies of its arrays; allocated by the first batch call, counted in
 *     workspace_bytes and held against params->max_workspace (SC_ENOMEM).  A context that never batches allocates and runs nothing new.
 *     (The device copies of a host form — this one's and those of every host-array entry below — live in ONE pool the host forms
 *     of a context share: a host form returns with the stream idle, so nothing in the pool outlives it, and a context that uses
 *     several of them holds one copy of the largest arrays, not one per entry.  Whatever a host form returns, no copy from or
 *     into the caller's arrays is in flight.)
 * Cost: a problem occupies ONE compute unit's workgroup for (triangles of its graph) x (3 .. 10 enumeration passes) + (kept triangles)
 * x n_b.  The graphs of a few hundred putative correspondences hold 10^3 .. 10^5 triangles; a DENSE 512-point problem (2 x 10^7
 * triangles) keeps its workgroup busy for tens of milliseconds while the rest of the batch has long finished — such problems belong
 * to sc_register.  There is no balancing by problem size. */
#define SC_BATCH_MAX_N 512u
typedef struct sc_batch_result {   /* 80 bytes */
  float    Rt[12];      /* R row-major, then t; R = I, t = 0 unless status == SC_OK        */
  int32_t  status;      /* SC_OK, SC_ENOHYP, or SC_EINVAL (a non-finite coordinate)        */
  uint32_t n;           /* correspondences of this problem                                 */
  uint32_t edges;
  uint32_t tri_kept;    /* min(T, tri_total)                                               */
  uint64_t tri_total;   /* 3-cliques of the WHOLE graph (as with SC_FLAG_EXACT_TOTAL)      */
  uint32_t best_rank;
  uint32_t best_count;
} sc_batch_result;
/* every buffer but offset in HBM: d_src / d_tgt total x 3 floats, d_res n_problems records, d_mask total bytes */
int sc_register_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                             const sc_params* params, sc_batch_result* d_res, uint8_t* d_mask);
/* the same with host arrays; waits */
int sc_register_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                      const sc_params* params, sc_batch_result* res, uint8_t* mask);

/* ---- further rigid motions from a scored frame: sc_peel ---------------------------------------------
 * sc_register answers "which ONE rigid motion explains most correspondences".  The T scored hypotheses stay in the
 * context; a ROUND re-scores them over the correspondences no earlier winner has claimed — stages C2 + C3 only, a
 * fraction of a frame — and returns the next motion: a second instance, the background, or a runner-up that is
 * distinct from the winner (winner 236 inliers, next round 4: unambiguous; 236 then 210: a repeated structure).
 *
 * A FRAME is what an sc_register / sc_register_device / sc_register_device_async + sc_wait call that returned SC_OK
 * (shard_world == 1) leaves in its context.  Its mask is the claimed set C_0.  Round r >= 1:
 *   1. alive = correspondences not in C_{r-1};
 *   2. score_r(h) of every hypothesis h of the frame's selection = the frame's score_mode over the alive ones only
 *      (canonical fp32 chain; sums of integers, so independent of order);
 *   3. winner = largest score_r, ties by best ranking key, then lowest (i, j, k): the frame's own total order;
 *   4. every score_r == 0: SC_ENOHYP, R = I, t = 0, mask all zero, C_r = C_{r-1}; a further call returns the same;
 *   5. mask_r[m] = alive[m] and |R p_m + t - q_m|^2 < tau^2 (the winner's fp32 (R, t)), n bytes in the caller's
 *      ORIGINAL indexing; C_r = C_{r-1} u mask_r;
 *   6. with SC_FLAG_REFINE in the frame's parameters (R, t) is the fp64 refit over mask_r; mask_r stays the fp32 winner's;
 *   7. stats: n, edges, tri_total, tri_kept as the frame reported them, tri_scored = tri_kept, best_rank = the winner's
 *      index in the ranked list, best_count = score_r(winner) (inlier-count mode: == popcount(mask_r)).  A frame with
 *      SC_FLAG_TIMING: us_stage = the claim + compact launch, us_score, us_argmax, us_mask (with the refit), us_total.
 * A round's results are a function of the frame's input and r only — not of how the frame was enqueued (waited,
 * host-free, repeated), of which C2 kernel scored it, or of the context's history.
 * What ends a frame: any other computing entry on the context (sc_register*, sc_match*, sc_hypothesize*, sc_finalize*, sc_shard_*,
 * every sc_*_host hook), or a frame call that did not return SC_OK.  sc_peel* without a frame: SC_EINVAL (sc_last_error
 * says so); with a call outstanding: SC_EINVAL as everywhere.  d_src / d_tgt need not stay valid after the frame call:
 * rounds read the context's staged copy.  Rounds wait for their winner (there is no async form).  Sharded and multi-GPU
 * forms (sc_hypothesize*, sc_shard_*, sc_register_multi) leave no frame.
 * NOT "run the path again on the rest": the compatibility graph and the ranked list are the frame's.  A motion none of
 * whose triangles made the frame's top T cannot be found by peeling — for that case run a second sc_register on the
 * correspondences no round has claimed.
 * The first round allocates the rounds' workspace (a second set of planes, n claimed bytes; they count toward
 * workspace_bytes); a context that never peels allocates and runs nothing new. */
/* round r of the frame in ctx; outputs in HBM (d_Rt: 12 floats), visibility as for sc_register_device */
int sc_peel_device(sc_ctx* ctx, float* d_Rt, uint8_t* d_mask, sc_stats* stats);
/* the same, host outputs */
int sc_peel(sc_ctx* ctx, float R[9], float t[3], uint8_t* mask, sc_stats* stats);
/* frame + rounds in one call (host arrays): stops after max_instances motions (1 .. 65536), or at the first whose
 * best_count < min_score (that one is not returned), or at SC_ENOHYP.  Motion 0 is the frame's winner, motion k round k's.
 * Rt: max_instances x 12; score: max_instances; label: n x int32, the index of the motion that claimed correspondence m,
 * -1 for none (built on the device, copied out once); *n_found >= 0.  Returns the frame's status if the frame fails
 * (SC_ENOHYP: *n_found = 0, label all -1), else SC_OK.  stats: the frame's.  Rounds may follow (sc_peel). */
int sc_register_instances(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                          uint32_t max_instances, uint32_t min_score, float* Rt, uint32_t* score, int32_t* label,
                          uint32_t* n_found, sc_stats* stats);

/* ---- the last step of a sample-consensus registration: local optimisation of the best hypotheses: sc_polish ------------
 * What sc_register returns is the pose of ONE 3-point sample — the best of T Kabsch solutions, good to a fraction of a degree —
 * and SC_FLAG_REFINE adds exactly one least-squares refit over that winner's own mask.  sc_polish iterates "inliers of (R, t) ->
 * fp64 least-squares refit -> inliers again" to a fixed point, for the best `candidates` hypotheses of the frame, and returns the
 * one that scores best afterwards.  On the C1 scene (n = 2000, tau = 0.02) the pose error drops about five-fold (0.33 deg -> 0.06 deg).
 * It stays on the frame's correspondences: no dense clouds, no nearest-neighbour search, no tolerance.
 *
 * A FRAME is as defined for sc_peel.  sc_polish reads the frame and changes nothing in it: rounds before or after it are unaffected
 * and do not affect it, it may be repeated, and its result is a function of the frame's input and the polish parameters only —
 * not of how the frame was enqueued or of the context's history.
 *   1. Candidates: the K = min(candidates, number of hypotheses with frame score > 0) hypotheses that come first in the frame's
 *      total order — largest frame score over all n correspondences in the frame's score_mode, then lowest position in the ranked
 *      list (best ranking key, then lowest (i, j, k)).  K == 0: SC_ENOHYP, R = I, t = 0, mask all zero.
 *   2. Iteration, per candidate: Rt_0 = its fp32 (R, t) from the frame; for it = 1 .. max_iter:
 *          mask = the canonical inlier test |R p + t - q|^2 < tau^2 of Rt_{it-1} over all n;
 *          Rt_it = the fp64 least-squares refit over that mask, rounded to fp32 — SC_FLAG_REFINE's refit, in its canonical order
 *                  (chunks of 64 consecutive indices summed sequentially, the chunk sums added sequentially; pass 1 the centroids,
 *                  pass 2 H by fma; 10 Jacobi sweeps in fp64);
 *      stop when the refit is declined (fewer than 3 inliers, or a non-finite result) or when Rt_it equals Rt_{it-1} bit for bit.
 *      iters = the number of refits that changed (R, t); the candidate's result is its last iterate; score = the frame's
 *      score_mode score of that iterate over all n; score0 = its frame score.
 *   3. Winner: the candidate with the largest score, ties to the earlier candidate.  Outputs: its (R, t), and mask[m] = the
 *      canonical inlier test of that (R, t).  stats: n, edges, tri_total, tri_kept, tri_scored are the frame's; best_rank = the
 *      winner's position in the ranked list; best_count = its score.  With the frame's SC_FLAG_TIMING: us_stage = the candidate
 *      selection, us_score = the polish launch, us_mask = the winner / mask launch, us_total their sum.
 * best_count MAY BE BELOW the frame's (C1, inlier count: 394 -> 390).  The frame's winner is the 3-point pose that happens to
 * catch most correspondences inside tau; the least-squares pose over its inliers sits in the middle of them, and a few borderline
 * correspondences that the sample's tilt had caught fall outside.  The polished pose is the better one (0.06 deg against 0.33 deg
 * from the truth on that scene) although it counts fewer; in the truncated score modes, which weigh residuals instead of counting
 * them, the polished score is the higher one (275 300 -> 282 177).  A caller that wants the count to decide compares the two itself.
 * Errors as for sc_peel: no frame — also after sc_match, or after a frame call that returned SC_ENOHYP — SC_EINVAL (sc_last_error says
 * so); a call outstanding: SC_EINVAL; params->size, a range or a reserved field wrong: SC_EINVAL.  The first polish allocates the
 * workspace (the candidate list, candidates x ceil(n / 64) x 16 doubles of chunk sums; counted in workspace_bytes and held against the
 * frame's cap: SC_ENOMEM); a context that never polishes allocates and runs nothing new.  sc_polish waits for its winner (no async form). */
typedef struct sc_polish_params {
  uint32_t size;         /* = sizeof(sc_polish_params)                                                */
  uint32_t candidates;   /* hypotheses polished: 1 .. 64                                              */
  uint32_t max_iter;     /* refits per candidate at most: 1 .. 64                                     */
  uint32_t flags;        /* must be 0                                                                 */
  uint32_t reserved[4];  /* must be 0                                                                 */
} sc_polish_params;
typedef struct sc_polish_cand {  /* 64 bytes */
  float    Rt[12];       /* the candidate's last iterate: R row-major, then t                          */
  uint32_t rank;         /* its position in the ranked list                                            */
  uint32_t score0;       /* its frame score                                                            */
  uint32_t score;        /* the score of Rt over all n, frame's score_mode                             */
  uint16_t iters;        /* refits that changed (R, t)                                                 */
  uint16_t reserved;
} sc_polish_cand;
int sc_polish_default_params(sc_polish_params* pp);   /* size set, candidates 8, max_iter 16, no flags */
/* outputs in HBM (d_Rt: 12 floats, d_mask: n bytes; d_cand: `candidates` records, entries past K zeroed, NULL ok; d_ncand: K, NULL ok),
 * visibility as for sc_register_device */
int sc_polish_device(sc_ctx* ctx, const sc_polish_params* pp, float* d_Rt, uint8_t* d_mask, sc_polish_cand* d_cand, uint32_t* d_ncand,
                     sc_stats* stats);
/* the same, host outputs (cand: `candidates` records, NULL ok; n_cand: NULL ok) */
int sc_polish(sc_ctx* ctx, const sc_polish_params* pp, float R[9], float t[3], uint8_t* mask, sc_polish_cand* cand, uint32_t* n_cand,
              sc_stats* stats);

/* ---- descriptor matching: two sets of keypoint descriptors in, putative correspondences out --------------
 * What stands in front of sc_register in a caller's frame: source keypoint i has a descriptor fsrc[i] (FPFH 33-D, FCGF 32-D,
 * SHOT 352-D ...), target keypoint j has ftgt[j]; a correspondence is (i, the j whose descriptor is nearest).  Brute force, exact,
 * and a function of the input alone, bit for bit:
 *   fsrc: ns x dim, ftgt: nt x dim, fp32, row-major, finite; 1 <= dim <= 1024, 1 <= ns, nt <= 2^24.
 *   distance of row i and row j, fp32, every operation rounded to nearest, no fused multiply-add, c ascending:
 *       acc = 0;  for c in 0 .. dim-1:  d = a[c] - b[c];  acc = acc + d * d
 *   (symmetric bit for bit; a sum that overflows to +inf is legal and ordered like any other value).
 *   The candidates of source row i are ordered by the u64 key (bits(acc) << 32) | j, ascending: nearest first, ties to the lower
 *   index.  The reverse order, for target row j, is (bits(acc) << 32) | i.
 *   knn = k (1 .. 4): row i yields its k smallest keys in order (fewer if nt < k).
 *   SC_MATCH_MUTUAL (k = 1 only): (i, j) is kept iff j is i's minimum and i is j's minimum under the reverse order.
 *   ratio in (0, 1) (k = 1 only; 0 = off): (i, j) is kept iff acc1 < r2 * acc2, r2 = (float)((double)ratio * ratio), one fp32
 *   multiply, acc2 the distance of i's second-smallest key; kept when nt == 1.  Both tests may be combined.
 * Output: corr (n x 2 int32: i, j) in ascending (i, rank) order, d2 (n x fp32: acc), and the count n <= ns * knn.
 * A NaN or infinity among the descriptors is SC_EINVAL; it is found on the device by the pass that reads it.
 * Workspace (the slices' partial lists, the column minima) belongs to the context like every other buffer: allocated by the first
 * match, grown on demand, counted in workspace_bytes and held against the cap of the last sc_params the context saw (64 GiB before
 * any); a context that never matches allocates and runs nothing new.  sc_match* ends the frame a context may hold (sc_peel). */
#define SC_MATCH_MUTUAL 1u
typedef struct sc_match_params {
  uint32_t size;         /* = sizeof(sc_match_params)                                                  */
  uint32_t dim;          /* D: floats per descriptor, 1 .. 1024                                         */
  uint32_t knn;          /* k: 1 .. 4                                                                   */
  uint32_t flags;        /* SC_MATCH_*                                                                  */
  float    ratio;        /* 0 = off, else in (0, 1): the ratio test (k = 1)                             */
  uint32_t reserved[3];  /* must be 0                                                                   */
} sc_match_params;
int sc_match_default_params(sc_match_params* mp);   /* size set, dim 0 (the caller sets it), knn 1, no flags, ratio 0 */
/* Every buffer in HBM.  d_corr: ns * knn x 2 int32, d_d2: ns * knn floats, d_count: 2 x u32.  Enqueues on the context's stream and
 * returns without waiting: d_count[0] = n and the first n entries of d_corr / d_d2 are valid in stream order; d_count[1] = 1 if a
 * non-finite descriptor was read (then n = 0 and d_corr / d_d2 are unspecified).  Parameter errors return SC_EINVAL at once. */
int sc_match_device(sc_ctx* ctx, const float* d_fsrc, int64_t ns, const float* d_ftgt, int64_t nt, const sc_match_params* mp,
                    int32_t* d_corr, float* d_d2, uint32_t* d_count);
/* The same with host arrays (corr, d2: room for ns * knn entries; the first *n are written); waits.  A non-finite descriptor:
 * SC_EINVAL, *n = 0. */
int sc_match(sc_ctx* ctx, const float* fsrc, int64_t ns, const float* ftgt, int64_t nt, const sc_match_params* mp,
             int32_t* corr, float* d2, uint32_t* n);
/* Descriptors in, (R, t), correspondences and mask out (host arrays): sc_match on the descriptors, then sc_register on
 * (src_pts[corr[m][0]], tgt_pts[corr[m][1]]), m < n — the matched points are gathered on the device and nothing but the count
 * crosses the host in between (one wait).  src_pts: ns points, tgt_pts: nt points, params->layout; mask: room for ns * knn bytes,
 * mask[m] belongs to corr[m].  corr, d2, *n are valid whenever the match itself succeeded (every status but SC_EINVAL / SC_ENOMEM /
 * SC_EHIP); n < 3: SC_ENOHYP with R = I, t = 0 and the mask untouched; otherwise status, R, t, mask and stats are exactly those of
 * sc_register(ctx, gathered src, gathered tgt, n, params, ...), and the call leaves that frame: sc_peel may follow. */
int sc_register_features(sc_ctx* ctx, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts,
                         const float* ftgt, int64_t nt, const sc_match_params* mp, const sc_params* params, float R[9],
                         float t[3], int32_t* corr, float* d2, uint32_t* n, uint8_t* mask, sc_stats* stats);

/* ---- descriptor matching gated by a pose prior: sc_match_guided ("guided matching") ----------------------
 * Once a pose is known — a frame's winner, a motion of sc_peel, an external prior — a pipeline matches again under it: source
 * keypoint i may only pair with the target keypoints that lie within a radius of where the pose puts it, and among those the nearest
 * descriptor wins.  This is NOT sc_match filtered by the gate afterwards: a row whose pose-blind nearest neighbour lies outside the
 * gate is re-assigned here, not lost.  A function of the input alone, bit for bit:
 *   The pose: Rt is the library's record, R = Rt[0..8] row-major, t = Rt[9..11], mapping source onto target.
 *   src_pts: ns points, tgt_pts: nt points, fp32, in guide->layout (SC_AOS: n x 3 row-major; SC_SOA: three planes of n), finite;
 *   point i belongs to descriptor row i.  fsrc, ftgt, ns, nt and every rule of sc_match_params: as sc_match.
 *   The gate residual of (i, j), p = src_pts[i], q = tgt_pts[j] — the canonical residual of the masks' inlier test, every operation
 *   fp32 and rounded to nearest, fma = the fused multiply-add, c in x, y, z:
 *       e_c = t_c + fma(R_c2, pz, fma(R_c1, py, fma(R_c0, px, -q_c)));   g2 = fma(ez, ez, fma(ey, ey, ex * ex))
 *   The threshold: gate2 = (float)((double)gate * gate), as tau^2 is derived from tau.
 *   Admissibility: adm(i, j) <=> g2(i, j) < gate2, a float <: a NaN or infinite residual is never admissible (and raises no flag:
 *   only the INPUT is tested for finiteness, see below).
 *   The descriptor distance acc(i, j) and both u64 key orders are sc_match's, unchanged.
 *   Candidates: row i's candidates are its admissible j only, ordered by (bits(acc) << 32) | j.
 *     knn = k: the k smallest admissible keys in order, fewer if fewer are admissible; a row with no admissible j yields nothing.
 *     SC_MATCH_MUTUAL: target j's minimum runs over its admissible i only, under the reverse key (bits(acc) << 32) | i.
 *     ratio: acc1 < r2 * acc2 with acc2 the second-smallest ADMISSIBLE key; the match is kept when the row has fewer than two
 *     admissible candidates (the rule nt == 1 follows in sc_match).
 * Output: corr (n x 2 int32) and d2 (n x fp32: acc) as in sc_match, in ascending (i, rank) order; g2 (n x fp32, optional: NULL ok):
 * the gate residual of every output entry; count[0] = n, count[1] = 1 if any descriptor, any point or the pose is not finite — then
 * n = 0, and the host forms return SC_EINVAL with *n = 0.  That flag depends on the input alone: every element of both descriptor
 * arrays, both point arrays and the pose is tested, whatever the gate excludes.
 * Determinism: the whole output is a function of the inputs, bit for bit — not of launch geometry, of the context's history or of
 * which form was called.
 * Frames and workspace: like sc_match*, these entries end the frame the context may hold; the workspace is sc_match's (the host
 * forms add their device copies), counted in workspace_bytes and held against the cap; a context that never calls them allocates
 * nothing new.
 * Refused with SC_EINVAL on the host before anything is enqueued, sc_last_error naming which: every rule of sc_match_params; a NULL
 * argument (g2 / d_g2 excepted); guide->size wrong; a layout above SC_SOA; a gate that is not finite and > 0; a flag or reserved word
 * that is not 0; a call outstanding on the context.
 * Not here: batch and pairs forms (entries of their own: sc_match_guided_batch, below); several poses per call (entries of their own: sc_match_guided_poses, below); a gate on anything but the point residual (descriptor-space or scale
 * gates); soft weighting by g2. */
typedef struct sc_guide_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_guide_params)                                                  */
  uint32_t layout;       /* SC_AOS / SC_SOA: how src_pts and tgt_pts are laid out                      */
  float    gate;         /* radius, finite, > 0                                                        */
  uint32_t flags;        /* must be 0 (the sc_match_guided_batch entries: SC_GUIDE_POSE_STATUS or 0)   */
  uint32_t reserved[4];  /* must be 0                                                                  */
} sc_guide_params;
int sc_guide_default_params(sc_guide_params* gp);   /* size set, SC_AOS, gate 0 (the caller sets it), no flags */
/* Every buffer in HBM.  d_corr, d_d2, d_count as sc_match_device's; d_g2: ns * knn floats or NULL; d_Rt: 12 floats.  Exactly three
 * stream operations on the context's stream whatever the sizes (a memset and two launches), no host word; returns without waiting.
 * d_Rt is read in stream order: it may be the d_Rt that a preceding sc_register_device_async / sc_peel_device /
 * sc_polish_poses_device on the same stream wrote.  d_count[1] = 1: n = 0 and d_corr / d_d2 / d_g2 are unspecified. */
int sc_match_guided_device(sc_ctx* ctx, const float* d_src_pts, const float* d_fsrc, int64_t ns, const float* d_tgt_pts,
                           const float* d_ftgt, int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const float* d_Rt,
                           int32_t* d_corr, float* d_d2, float* d_g2, uint32_t* d_count);
/* The same with host arrays (corr, d2, g2: room for ns * knn entries, g2 may be NULL; the first *n are written); waits.  A
 * non-finite descriptor, point or pose entry: SC_EINVAL, *n = 0. */
int sc_match_guided(sc_ctx* ctx, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt,
                    int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const float Rt[12], int32_t* corr, float* d2,
                    float* g2, uint32_t* n);
/* sc_register_features with the guided match in front: the guided match under Rt_prior, the gather on the device, then the
 * unchanged sc_register_device on the gathered arrays, with one host wait (the count).  guide->layout must equal params->layout (the
 * keypoints are one pair of arrays); g2 may be NULL.  corr, d2, g2, *n are valid whenever the match itself succeeded; n < 3:
 * SC_ENOHYP with R = I, t = 0 and the mask untouched; otherwise status, R, t, mask and stats are exactly those of sc_register on
 * the gathered correspondences, and the call leaves that frame: sc_peel, sc_polish*, sc_pose_info_frame and sc_assign_poses_frame
 * may follow. */
int sc_register_guided_features(sc_ctx* ctx, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts,
                                const float* ftgt, int64_t nt, const sc_match_params* mp, const sc_guide_params* gp,
                                const float Rt_prior[12], const sc_params* params, float R[9], float t[3], int32_t* corr, float* d2,
                                float* g2, uint32_t* n, uint8_t* mask, sc_stats* stats);

/* ---- descriptor matching for a whole batch of small problems: sc_match_batch -----------------------------
 * What stands in front of sc_register_batch: its callers (pose candidates, fragment pairs of a few hundred keypoints, cluster pairs)
 * start from two sets of keypoints with descriptors PER PAIR.  Through sc_match_device that is three stream operations per pair and,
 * for a data-dependent count, a host read per pair before the packed batch can be laid out.  Here the whole batch is matched by two
 * launches, and sc_register_batch_features* runs sc_register_batch's kernel behind them without a word reaching the host.
 *
 * Layout: the problems are PACKED, as in sc_register_batch.  Problem b owns descriptor rows [src_off[b], src_off[b + 1]) of fsrc
 * (total_s x dim, row-major) and [tgt_off[b], tgt_off[b + 1]) of ftgt (total_t x dim); the same row ranges index src_pts / tgt_pts
 * (params->layout: SC_AOS total x 3; SC_SOA three planes of total_s, respectively total_t).  Both offset arrays are HOST arrays of
 * n_problems + 1 words in every form; the library copies them and keeps no caller pointer.  One sc_match_params and one sc_params
 * serve the whole batch.  1 <= ns_b, nt_b <= SC_MATCH_BATCH_MAX_N.
 * Outputs live in SLOTS, because the counts are data-dependent and nothing may wait for them: problem b's slot starts at entry
 * slot[b] = src_off[b] * knn and holds ns_b * knn entries of corr (pairs of int32), d2 and mask.  corr holds indices LOCAL to the
 * problem: 0 <= i < ns_b, 0 <= j < nt_b.  count: 2 x n_problems words; count[2b] = n_b, count[2b + 1] = 1 if the problem read a
 * non-finite descriptor (then n_b = 0).  Slot entries past n_b are unspecified.
 *
 * Semantics of the match: slot b and its count pair hold (corr, d2, n, flag) of sc_match on problem b alone with the same
 * sc_match_params, bit for bit — the canonical distance, the u64 key order, knn 1 .. 4 (fewer where nt_b < knn), SC_MATCH_MUTUAL
 * and ratio with knn == 1, a problem with nt_b == 1 kept under the ratio test, a sum that overflows to +inf legal.  A slot is a
 * function of its own descriptors and the parameters only: not of the problem's position in the batch, of n_problems, of its
 * neighbours, or of the context's history.  A non-finite descriptor is found on the device, flags only its own problem and does not
 * fail the call.
 * Semantics of sc_register_batch_features*: the match, then for every b
 *   - flag set: status SC_EINVAL, R = I, t = 0, n = 0, every count 0;
 *   - n_b < 3: status SC_ENOHYP, R = I, t = 0, n = n_b, every count 0, mask bytes [slot[b], slot[b] + n_b) zero;
 *   - otherwise the record and mask bytes [slot[b], slot[b] + n_b) are sc_register_batch's on the gathered correspondences
 *     (src_pts[src_off[b] + i_m], tgt_pts[tgt_off[b] + j_m]), m < n_b — hence sc_register's on them alone with SC_FLAG_EXACT_TOTAL; a
 *     non-finite point among the gathered ones: SC_EINVAL with n = n_b, as there.  Mask byte slot[b] + m belongs to correspondence m.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument;
 * n_problems == 0; an ns_b or nt_b of 0 or above SC_MATCH_BATCH_MAX_N; offsets that decrease; total_s * knn > 2^31; any rule of
 * sc_match_params (see sc_match); a call outstanding on the context.  The features entries also refuse ns_b * knn > SC_BATCH_MAX_N
 * and everything sc_register_batch refuses of sc_params (shard_world != 1, SC_FLAG_REFINE, the timing flags, SC_FLAG_EST_BOUND,
 * SC_FLAG_SHARD_AB).
 * All four entries end the frame a context may hold and leave none: sc_peel / sc_polish after them return SC_EINVAL.  The device
 * forms enqueue on the context's stream and return without waiting; no word of the GPU's reaches the host, and the number of stream
 * operations (one copy of the offsets and maps, one memset, two launches, sc_register_batch's one) depends neither on n_problems nor
 * on any size.  (Like sc_register_batch_device a device form may wait for the previous batch call's copy out of the offset staging
 * area they share: an event behind that copy, not behind its kernel.)
 * Workspace: the copies of the offsets, slot starts and tile map, the rows' lists between the two launches, the column minima when
 * mutual, the gathered points, and the host forms' device copies; allocated by the first such call, counted in workspace_bytes and
 * held against the cap (SC_ENOMEM).  A context that never calls these entries allocates and runs nothing new. */
#define SC_MATCH_BATCH_MAX_N 4096u
/* every buffer but the offsets in HBM: d_corr total_s * knn x 2 int32, d_d2 total_s * knn floats, d_count 2 * n_problems u32 */
int sc_match_batch_device(sc_ctx* ctx, const float* d_fsrc, const uint32_t* src_off, const float* d_ftgt, const uint32_t* tgt_off,
                          uint32_t n_problems, const sc_match_params* mp, int32_t* d_corr, float* d_d2, uint32_t* d_count);
/* the same with host arrays; waits */
int sc_match_batch(sc_ctx* ctx, const float* fsrc, const uint32_t* src_off, const float* ftgt, const uint32_t* tgt_off,
                   uint32_t n_problems, const sc_match_params* mp, int32_t* corr, float* d2, uint32_t* count);
/* match + registration; d_res: n_problems records, d_mask: total_s * knn bytes, the rest as above */
int sc_register_batch_features_device(sc_ctx* ctx, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                      const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                                      const sc_match_params* mp, const sc_params* params, sc_batch_result* d_res, int32_t* d_corr,
                                      float* d_d2, uint32_t* d_count, uint8_t* d_mask);
/* the same with host arrays; waits */
int sc_register_batch_features(sc_ctx* ctx, const float* src_pts, const float* fsrc, const uint32_t* src_off, const float* tgt_pts,
                               const float* ftgt, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                               const sc_params* params, sc_batch_result* res, int32_t* corr, float* d2, uint32_t* count,
                               uint8_t* mask);

/* ---- iterated fp64 refits for a batch's winners: sc_polish_batch ---------------------------------------------
 * What a frame's caller gets from SC_FLAG_REFINE and sc_polish, for the members of a batch: sc_register_batch* leaves the Kabsch pose
 * of ONE 3-point sample per problem; sc_polish_batch iterates "inliers of (R, t) -> fp64 least-squares refit -> inliers again" to a
 * fixed point for every problem of the batch in ONE launch, a workgroup per problem (sc_polish_batch.hip).  sc_register_batch_device
 * followed by sc_polish_batch_device on the same context is two launches and no host word.
 *
 * Layout: the packed problems of sc_register_batch — d_src, d_tgt, offset (a HOST array of n_problems + 1 words), params->layout —
 * plus d_res, n_problems records of sc_batch_result that hold the input pose and status of every problem.  d_res is READ, never
 * written, and need not come from sc_register_batch: only its status and Rt are looked at.  d_pol receives n_problems records of
 * sc_polish_batch_result, d_mask total bytes.
 *
 * sc_polish_params is reused: candidates MUST be 1 — a batch member keeps only its winner, nothing is materialised per hypothesis, so
 * more than one candidate per problem is out of scope —, max_iter 1 .. 64, flags and reserved 0.  sc_params is checked as
 * sc_register_batch checks it; only tau, score_mode and layout are read.
 *
 * Semantics, per problem b with input status SC_OK: Rt_0 = d_res[b].Rt, score0 = its score over all n_b in params->score_mode; then
 * step 2 of sc_polish, exactly: for it = 1 .. max_iter, mask = the canonical inlier test of Rt_{it-1}, Rt_it = the fp64 refit over
 * that mask in its canonical order, rounded to fp32; stop when the refit is declined (fewer than 3 inliers, or a non-finite result:
 * SC_POLISH_STOP_DECLINED), when Rt_it equals Rt_{it-1} bit for bit (SC_POLISH_STOP_FIXED), or after max_iter refits
 * (SC_POLISH_STOP_MAX_ITER).  iters = the refits that changed (R, t); Rt = the last iterate; score = its score over all n_b; mask byte
 * m = the canonical inlier test of Rt.  The record equals, bit for bit, what sc_register + sc_polish(candidates = 1, the same max_iter)
 * return for the problem alone, and with max_iter = 1 its Rt is sc_register's with SC_FLAG_REFINE.
 *   - A first refit that is declined: status SC_OK, Rt = the input's bits, iters 0, score = score0.
 *   - Input status != SC_OK: that status is passed through; R = I, t = 0, scores 0, iters 0, stop SC_POLISH_STOP_DECLINED, mask zero.
 *   - Input status SC_OK but a non-finite coordinate, or a non-finite input Rt: SC_EINVAL with the same output shape.  It is found on
 *     the device, affects only that problem and does not fail the call.
 *   - A record is a function of the problem's points, the input Rt, tau, score_mode and max_iter only: not of its position in the
 *     batch, of the neighbours, or of the context's history.
 *   - score MAY be below score0 in the inlier-count mode, as sc_polish's may be below the frame's (see there).
 * d_mask MAY be the buffer sc_register_batch_device wrote: the kernel never reads a mask.
 *
 * The slot form follows sc_register_batch_features_device: problem b's correspondences are (src_pts[src_off[b] + corr[slot[b] + m][0]],
 * tgt_pts[tgt_off[b] + corr[slot[b] + m][1]]), m < count[2b], slot[b] = src_off[b] * knn; d_res, d_pol and the mask bytes are positioned
 * as that entry positions them.  The kernel gathers while it stages and keeps no state from the features call.  A flagged problem or
 * one with count[2b] < 3 passes its input status through (SC_EINVAL if that status claims SC_OK); an index in corr outside the problem
 * is SC_EINVAL for that problem.  knn is the sc_match_params.knn the slots were laid out with (1 .. 4).
 *
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument;
 * everything sc_register_batch refuses (the slot form: everything sc_register_batch_features refuses of the offsets, ns_b * knn >
 * SC_BATCH_MAX_N included); pp->size wrong, candidates != 1, max_iter outside 1 .. 64, a non-zero flag or reserved word; a call
 * outstanding on the context.  The device forms enqueue on the context's stream and return without waiting: outputs are complete in
 * stream order.  (Like sc_register_batch_device they may wait for the previous batch call's copy out of the offset staging area they
 * share: an event behind that copy, not behind its kernel.)  All three entries end the frame a context may hold and leave none.
 * Workspace: the copies of the offsets, plus the host form's device copies of its arrays; allocated by the first such call, counted in
 * workspace_bytes and held against params->max_workspace (SC_ENOMEM).  A context that never calls these entries allocates and runs
 * nothing new.  There is no async / wait form and no balancing by problem size. */
#define SC_POLISH_STOP_FIXED    0   /* the refit returned the bits it started from               */
#define SC_POLISH_STOP_DECLINED 1   /* fewer than 3 inliers or a non-finite refit; or no pose    */
#define SC_POLISH_STOP_MAX_ITER 2   /* max_iter refits done, the last one still changed (R, t)  */
typedef struct sc_polish_batch_result {  /* 64 bytes */
  float    Rt[12];   /* the last iterate; R = I, t = 0 unless status == SC_OK                  */
  int32_t  status;   /* SC_OK, or why there is no pose: SC_ENOHYP / SC_EINVAL                  */
  uint32_t score0;   /* score of the input pose over all n, params->score_mode                 */
  uint32_t score;    /* score of Rt                                                            */
  uint16_t iters;    /* refits that changed (R, t)                                             */
  uint16_t stop;     /* SC_POLISH_STOP_*                                                       */
} sc_polish_batch_result;
/* every buffer but offset in HBM: d_src / d_tgt total x 3 floats, d_res / d_pol n_problems records, d_mask total bytes */
int sc_polish_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                           const sc_params* params, const sc_polish_params* pp, const sc_batch_result* d_res,
                           sc_polish_batch_result* d_pol, uint8_t* d_mask);
/* the same with host arrays; waits */
int sc_polish_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                    const sc_params* params, const sc_polish_params* pp, const sc_batch_result* res, sc_polish_batch_result* pol,
                    uint8_t* mask);
/* behind sc_register_batch_features_device: the points and both offset arrays as given there, its d_corr, d_count and d_res;
 * d_pol n_problems records, d_mask total_s * knn bytes */
int sc_polish_batch_slots_device(sc_ctx* ctx, const float* d_src_pts, const uint32_t* src_off, const float* d_tgt_pts,
                                 const uint32_t* tgt_off, uint32_t n_problems, uint32_t knn, const sc_params* params,
                                 const sc_polish_params* pp, const int32_t* d_corr, const uint32_t* d_count,
                                 const sc_batch_result* d_res, sc_polish_batch_result* d_pol, uint8_t* d_mask);

/* ---- several rigid motions per batch problem: sc_register_instances_batch ---------------------------------------------
 * What sc_register_instances answers for a frame — "which further rigid motions explain the rest?" — for the members of a batch:
 * a second instance of an object, or a background motion, is the normal case for sc_register_batch's callers.  ONE launch, a
 * workgroup per problem: it runs the frame exactly as sc_register_batch runs it and then, inside the same workgroup, up to
 * max_instances - 1 rounds of sc_peel on what the workgroup still holds (the points, the graph, K* and the cut).  No second launch,
 * no host word, no state in the context.
 *
 * Layout: the packed problems of sc_register_batch (d_src, d_tgt, offset a HOST array of n_problems + 1 words, params->layout,
 * 3 <= n_b <= SC_BATCH_MAX_N).  d_res holds max_instances x n_problems records, MOTION-MAJOR: motion k of problem b is
 * d_res[k * n_problems + b] — so that ONE PLANE, d_res + k * n_problems, is a valid d_res of sc_polish_batch_device.  d_label: total
 * int32, positioned like sc_register_batch's mask; d_nfound: n_problems words.  1 <= max_instances <= SC_INSTANCES_BATCH_MAX.
 *
 * Semantics, per problem b: sc_register_instances on the problem alone with SC_FLAG_EXACT_TOTAL.
 *   - Plane 0, d_res[b], is sc_register_batch's record of the problem, bit for bit, whatever min_score is.
 *   - Motion 0 is found iff plane 0 is SC_OK and its best_count >= min_score.
 *   - Motion k >= 1 is round k of sc_peel (steps 1 - 5 and 7 of its contract): the alive correspondences are those no earlier motion
 *     claimed; every KEPT triangle — the frame's selection, K* and the cut as the frame fixed them, triangles whose vertices are
 *     themselves claimed included — is scored over the alive ones in params->score_mode; the winner by score, then key, then lowest
 *     (i, j, k); mask_k = alive && the inlier test of the winner's fp32 (R, t).  A round in which every score is 0, or whose winner
 *     scores < min_score, stops the problem: that motion is not returned.
 *   - The record of motion k: status SC_OK, Rt the winner's; n, edges, tri_kept, tri_total plane 0's; best_rank the winner's position
 *     in the ranked list; best_count its score over the alive ones.
 *   - d_nfound[b] = the number of motions found.
 *   - Planes k >= max(nfound, 1): R = I, t = 0, the counts plane 0's, best_rank = best_count = 0, status SC_ENOHYP — or plane 0's
 *     status if that is SC_EINVAL.
 *   - d_label[offset[b] + m] = the motion that claimed correspondence m, -1 for none; every entry of the problem's range is written.
 *   - A problem's outputs are a function of its points, the parameters, max_instances and min_score only: not of its position, its
 *     neighbours, n_problems or the context's history.  A non-finite coordinate is found on the device and ends only its own problem
 *     (SC_EINVAL in every plane, nfound 0, labels -1).
 * As with sc_peel this is NOT "run the path again on the rest": a motion none of whose triangles made the frame's top T is not found.
 *
 * The features form is sc_register_batch_features_device with rounds: the match, then the kernel on the slots.  d_label holds
 * total_s * knn entries positioned like that entry's mask: entries [slot[b], slot[b] + n_b) are written, entries past n_b are
 * unspecified.  A flagged problem and one with n_b < 3 get the records sc_register_batch_features gives them, in every plane, and
 * nfound 0.
 *
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: everything
 * sc_register_batch (the features form: sc_register_batch_features) refuses — SC_FLAG_REFINE stays refused —, and max_instances
 * outside 1 .. SC_INSTANCES_BATCH_MAX.  The device forms enqueue on the context's stream and return without waiting (they may wait
 * for the previous batch call's copy out of the offset staging area, as the sibling entries do).  All three entries end the frame a
 * context may hold and leave none.  Workspace: the copy of the offsets (the features form: what sc_register_batch_features_device
 * holds), plus the host form's device copies of its arrays; allocated by the first such call, counted in workspace_bytes and held
 * against params->max_workspace (SC_ENOMEM).
 * Cost: a round is one scoring and one counting enumeration.  The scoring enumeration — (kept triangles) x (alive correspondences)
 * residuals — is what a frame mostly costs as well, so a round costs up to about a frame: measured, a call that finds two or three
 * motions costs 2.4 - 2.9 sc_register_batch_device calls.  max_instances and min_score bound it. */
#define SC_INSTANCES_BATCH_MAX 16u
/* every buffer but offset in HBM: d_res max_instances x n_problems records, d_label total int32, d_nfound n_problems u32 */
int sc_register_instances_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                       const sc_params* params, uint32_t max_instances, uint32_t min_score, sc_batch_result* d_res,
                                       int32_t* d_label, uint32_t* d_nfound);
/* the same with host arrays; waits */
int sc_register_instances_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                                const sc_params* params, uint32_t max_instances, uint32_t min_score, sc_batch_result* res,
                                int32_t* label, uint32_t* nfound);
/* match + instances; d_res max_instances x n_problems records, d_label total_s * knn int32, the rest as sc_register_batch_features_device */
int sc_register_instances_batch_features_device(sc_ctx* ctx, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                                const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off,
                                                uint32_t n_problems, const sc_match_params* mp, const sc_params* params,
                                                uint32_t max_instances, uint32_t min_score, sc_batch_result* d_res, int32_t* d_corr,
                                                float* d_d2, uint32_t* d_count, int32_t* d_label, uint32_t* d_nfound);

/* ---- listed pairs of shared keypoint sets: sc_match_pairs ------------------------------------------------------
 * The callers of sc_match_batch — fragment pairs, the cluster pairs of a place-recognition back end, object-pose candidates — do
 * not start from packed problems: they hold a TABLE of keypoint sets and a LIST of pairs drawn from it, and a set takes part in many
 * pairs.  A packed problem owns its rows, so such a caller had to copy every set's descriptors and points once per pair before the
 * call (64 sets of 256 keypoints, all 2016 pairs: 144 MB of copies of a 2.3 MB table).  These entries take the table and the list.
 *
 * Layout: ONE table of sets.  Set s owns rows [set_off[s], set_off[s + 1]) of feat (total x dim, row-major) and the same rows of
 * pts (params->layout: SC_AOS total x 3; SC_SOA three planes of total).  set_off is a HOST array of n_sets + 1 words.  pairs is a
 * HOST array of 2 * n_pairs words: pair p matches source set pairs[2p] against target set pairs[2p + 1].  Source and target come
 * from the same table (a caller with two collections concatenates them); pairs[2p] == pairs[2p + 1] is legal, a pair may occur
 * twice, and the list is in any order.  The library copies both host arrays and keeps no caller pointer.
 * Outputs live in SLOTS, as in sc_match_batch: slot[p] = knn x (the sum of ns_q over q < p), ns_q the rows of pair q's source set
 * (sc_pairs_layout computes them); corr holds indices LOCAL to the pair's two sets; the count pair sits at count[2p], count[2p + 1];
 * records at d_res[p], mask bytes at slot[p] + m.  This is what sc_match_batch produces for the same pairs expanded into packed
 * arrays in list order.
 *
 * Semantics: pair p's slot, count pair, record, mask bytes and polish record are, bit for bit, what sc_match_batch_device,
 * sc_register_batch_features_device and sc_polish_batch_slots_device return for problem p when the caller has expanded the pairs into
 * packed arrays in list order — and everything those contracts say holds per pair: the canonical distance and the u64 key order, knn
 * 1 .. 4, SC_MATCH_MUTUAL and ratio with knn == 1, a target set of one row kept under the ratio test, the records of flagged pairs and
 * of pairs with n_p < 3, entries past n_p unspecified, stream-ordered device forms with no host read.  In addition:
 *   - A pair's outputs are a function of its two sets and the parameters only: not of its position in the list, of the other pairs,
 *     of which other pairs share its sets, of n_pairs or of the context's history.  (Two pairs that share a target set do not share
 *     column minima.)
 *   - A non-finite descriptor in a set flags every pair that uses that set, and no other pair; the call returns SC_OK.
 *   - The number of stream operations is the packed form's: it depends neither on n_pairs nor on any size.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument;
 * n_sets == 0 or n_pairs == 0; set_off decreasing; a set index >= n_sets; a REFERENCED set with 0 rows or more than
 * SC_MATCH_BATCH_MAX_N (an unreferenced set may have any size); more than 2^31 output entries in all; every rule of sc_match_params /
 * sc_params / sc_polish_params that the packed entries apply; for the features and polish entries ns_p * knn > SC_BATCH_MAX_N; a call
 * outstanding on the context.  All entries with a context end the frame it may hold and leave none.  (A device form may wait for
 * the previous batch call's copy out of the staging area the batch entries share, as the packed forms do.)
 * Workspace: the pairs' records, slot starts and tile map; the rows' lists (the sum of ns_p x kp keys) and, when mutual, every
 * pair's own column minima (the sum of nt_p keys); the gathered points; the host forms' device copies of the table and the outputs.
 * They are the packed entries' buffers — a context that uses both forms holds one set —, allocated by the first such call, counted
 * in workspace_bytes and held against the cap (SC_ENOMEM).  A context that never calls these entries allocates and runs nothing new.
 * Not here: a pairs form of sc_register_instances_batch_features, balancing by pair size. */
/* host only, no context: slot[p] for p <= n_pairs (slot[n_pairs] = the entries in all); SC_EINVAL for a NULL argument, knn outside
 * 1 .. 4 and anything sc_match_pairs refuses of the table and the list */
int sc_pairs_layout(const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint32_t knn, uint32_t* slot);
/* every buffer but set_off and pairs in HBM: d_feat total x dim floats, d_corr slot[n_pairs] x 2 int32, d_d2 slot[n_pairs] floats,
 * d_count 2 * n_pairs u32 */
int sc_match_pairs_device(sc_ctx* ctx, const float* d_feat, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs,
                          uint32_t n_pairs, const sc_match_params* mp, int32_t* d_corr, float* d_d2, uint32_t* d_count);
/* the same with host arrays; waits */
int sc_match_pairs(sc_ctx* ctx, const float* feat, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs,
                   const sc_match_params* mp, int32_t* corr, float* d2, uint32_t* count);
/* match + registration; d_pts the table's points, d_res n_pairs records, d_mask slot[n_pairs] bytes, the rest as above */
int sc_register_pairs_features_device(sc_ctx* ctx, const float* d_pts, const float* d_feat, const uint32_t* set_off, uint32_t n_sets,
                                      const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_params* params,
                                      sc_batch_result* d_res, int32_t* d_corr, float* d_d2, uint32_t* d_count, uint8_t* d_mask);
/* the same with host arrays; waits */
int sc_register_pairs_features(sc_ctx* ctx, const float* pts, const float* feat, const uint32_t* set_off, uint32_t n_sets,
                               const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_params* params,
                               sc_batch_result* res, int32_t* corr, float* d2, uint32_t* count, uint8_t* mask);
/* behind sc_register_pairs_features_device, as sc_polish_batch_slots_device is behind sc_register_batch_features_device: the
 * table's points, set_off and pairs as given there, its d_corr, d_count and d_res; d_pol n_pairs records, d_mask slot[n_pairs] bytes */
int sc_polish_pairs_slots_device(sc_ctx* ctx, const float* d_pts, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs,
                                 uint32_t n_pairs, uint32_t knn, const sc_params* params, const sc_polish_params* pp,
                                 const int32_t* d_corr, const uint32_t* d_count, const sc_batch_result* d_res,
                                 sc_polish_batch_result* d_pol, uint8_t* d_mask);

/* ---- pose-gated matching for batches and pairs: sc_match_guided_batch -----------------------------------------
 * sc_match_guided for the callers of the batch and pairs entries: one pose PER PROBLEM (per pair), on the device, and the stream
 * operations of sc_match_batch / sc_match_pairs whatever the batch.  What it closes: sc_register_batch_features /
 * sc_register_pairs_features leave a pose per problem in d_res; re-matching under it through sc_match_guided_device was three stream
 * operations per problem (and, for pairs, the table expanded per pair again).
 *   Layout: offsets, slots, count pairs, local indices exactly those of sc_match_batch (sc_match_pairs).  The points — src_pts total_s
 *   and tgt_pts total_t rows (pairs: pts, the table's rows), point i of the array beside descriptor row i — are in guide->layout
 *   (SC_AOS: rows x 3; SC_SOA: three planes of ALL rows).  d_g2: optional (NULL ok), slot-positioned like d_d2.
 *   The pose input: d_pose holds one record per problem (pair), pose_stride bytes apart, float Rt[12] at byte 0; with
 *   SC_GUIDE_POSE_STATUS in guide->flags also an int32 status at byte 48.  pose_stride: a multiple of 4, >= 48, and >= 52 with the
 *   flag — so sc_batch_result (80, with the flag), sc_polish_batch_result (64, with the flag) and a plain array of 12-float poses
 *   (48) all serve unchanged.  d_pose is read in stream order and never written by the match.
 *   Semantics, per problem b: the slot, g2 and the count pair are, bit for bit, what sc_match_guided returns for that problem alone
 *   with pose record b, the same sc_match_params and the same gate; every rule of that contract holds per problem (admissibility is
 *   g2 < gate2, a float <; knn, mutual and ratio run over admissible cells only; a match is kept when its row has fewer than two
 *   admissible candidates; a hostile but finite pose admits nothing and raises no flag).
 *   count[2b + 1] = 1, and then n_b = 0, iff any descriptor, any point or the pose of problem b is not finite, whatever the gate
 *   excludes (pairs: of either set of the pair — a bad value in a set flags every pair that uses the set and no other).  It flags
 *   that problem only; the call — the host forms too — returns SC_OK.
 *   SC_GUIDE_POSE_STATUS and a status other than SC_OK: the problem is skipped — its count pair is (0, 0), nothing else of it is read
 *   or written, its neighbours are not disturbed.
 *   A problem's outputs are a function of its own inputs, its pose and the parameters only: not of its position, of n_problems, of
 *   the other problems, of shared sets or of the context's history.
 *   The features entries: the guided match, then the unchanged registration on the slots (sc_register_batch_features' second half,
 *   with its rules for flagged problems and n_b < 3; a skipped problem has n_b = 0, hence SC_ENOHYP).  guide->layout must equal
 *   params->layout; ns_b * knn > SC_BATCH_MAX_N is refused as there.  d_pose MAY be d_res: the registration launch that writes d_res
 *   is ordered behind both match launches, so the record of problem b is read before it is replaced.
 * Stream operations: those of the unguided form, independent of any size — one copy, one memset, two launches, plus the
 * registration's one; no host word.  Frames and workspace: the entries end the frame the context may hold; the workspace is the
 * batched match's (the host forms add their device copies), counted in workspace_bytes and held against the cap.
 * Refused with SC_EINVAL on the host before anything is enqueued, sc_last_error naming which: everything sc_match_batch
 * (sc_match_pairs) and their features entries refuse; every rule of sc_guide_params, but that guide->flags may be
 * SC_GUIDE_POSE_STATUS (any other bit is refused; sc_match_guided* and sc_register_guided_features keep refusing every flag); a
 * pose_stride that breaks the rule above; a NULL argument (g2 / d_g2 excepted); a call outstanding on the context.
 * Not here: host forms of the two features entries; one pose shared by all problems, and several poses per problem (several poses
 * in ONE problem are the frame form's: sc_match_guided_poses, below); an instances
 * form. */
#define SC_GUIDE_POSE_STATUS 1u   /* sc_guide_params.flags, these entries only: the pose records hold an int32 status at byte 48 */
/* Everything but the offsets in HBM; enqueues on the context's stream and returns without waiting. */
int sc_match_guided_batch_device(sc_ctx* ctx, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                 const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                                 const sc_match_params* mp, const sc_guide_params* gp, const void* d_pose, uint32_t pose_stride,
                                 int32_t* d_corr, float* d_d2, float* d_g2, uint32_t* d_count);
/* The same with host arrays (pose: n_problems * pose_stride bytes, copied as given; g2 may be NULL); waits.  A flagged problem is
 * its count pair's business: SC_OK. */
int sc_match_guided_batch(sc_ctx* ctx, const float* src_pts, const float* fsrc, const uint32_t* src_off, const float* tgt_pts,
                          const float* ftgt, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                          const sc_guide_params* gp, const void* pose, uint32_t pose_stride, int32_t* corr, float* d2, float* g2,
                          uint32_t* count);
/* The guided match, then sc_batch.hip's registration on the slots; d_res, d_mask as sc_register_batch_features_device's. */
int sc_register_guided_batch_features_device(sc_ctx* ctx, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                             const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off,
                                             uint32_t n_problems, const sc_match_params* mp, const sc_guide_params* gp,
                                             const void* d_pose, uint32_t pose_stride, const sc_params* params,
                                             sc_batch_result* d_res, int32_t* d_corr, float* d_d2, float* d_g2, uint32_t* d_count,
                                             uint8_t* d_mask);
/* The pairs forms: the table and the list of sc_match_pairs, d_pts the table's points, one pose record per PAIR. */
int sc_match_guided_pairs_device(sc_ctx* ctx, const float* d_pts, const float* d_feat, const uint32_t* set_off, uint32_t n_sets,
                                 const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_guide_params* gp,
                                 const void* d_pose, uint32_t pose_stride, int32_t* d_corr, float* d_d2, float* d_g2,
                                 uint32_t* d_count);
int sc_match_guided_pairs(sc_ctx* ctx, const float* pts, const float* feat, const uint32_t* set_off, uint32_t n_sets,
                          const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_guide_params* gp,
                          const void* pose, uint32_t pose_stride, int32_t* corr, float* d2, float* g2, uint32_t* count);
int sc_register_guided_pairs_features_device(sc_ctx* ctx, const float* d_pts, const float* d_feat, const uint32_t* set_off,
                                             uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp,
                                             const sc_guide_params* gp, const void* d_pose, uint32_t pose_stride,
                                             const sc_params* params, sc_batch_result* d_res, int32_t* d_corr, float* d_d2,
                                             float* d_g2, uint32_t* d_count, uint8_t* d_mask);

/* ---- loop consistency of a pair list's poses: sc_pairs_cycles ------------------------------------------------------
 * The pairs entries leave a relative pose per pair on the device, and their caller — a loop-closure or fragment-registration back
 * end — takes each as an edge of a pose graph.  A wrong pairwise registration (a repeated structure, a symmetric object) has a high
 * inlier count and a well-conditioned information matrix: nothing computed per pair tells it from a right one.  The other pairs do:
 * three pairs on three sets close a loop, and the composed motion round the loop is the identity or it is not.  These entries count,
 * for every pair, the loops of three it closes and the consistent ones among them, and prune the list to a fixed point: rigidity
 * triangles that vote, one level up — sets for points, poses for lengths.  On the device, stream-ordered behind the entries that
 * produce the poses, no host word in between.
 *
 * Inputs.  n_sets; pairs: a HOST array of 2 * n_pairs words, exactly the list of sc_match_pairs — pair p relates source set
 * pairs[2p] to target set pairs[2p + 1], in any order; self pairs and repeated pairs are legal, and (a, b) and (b, a) may both be
 * listed.  The library copies the list and keeps no pointer.  d_pose: n_pairs pose records, pose_stride bytes apart, under the rules
 * of every pose entry: float Rt[12] at byte 0 (R row-major, then t) maps the SOURCE set's coordinates onto the TARGET's; with
 * SC_CYCLES_STATUS an int32 status at byte 48; pose_stride a multiple of 4, at least 48, at least 52 with the flag; read, never
 * written.  sc_batch_result (80), sc_polish_batch_result (64) and plain 12-float records (48) all fit.  d_keep: n_pairs bytes or
 * NULL; a pair with keep[p] != 0 is never dropped (odometry edges) and still takes part in loops.
 * Thresholds, derived on the host in double: tr_min = 1.0 + 2.0 * cos((double)rot_tol), e2_max = (double)trans_tol *
 * (double)trans_tol.  sc_cycles_thresholds returns exactly the two values a call uses.
 *
 * Definitions.  The call is a function of the list, the poses, keep and the parameters alone, bit for bit.  All arithmetic is fp64
 * on the exactly widened fp32 entries; every operation is a plain rounded product or sum in the order written; nothing is fused.
 *   valid(p)   Rt is finite and, where a status is read, it is SC_OK.
 *   edge(p)    valid(p) and pairs[2p] != pairs[2p + 1].
 *   T(x->y)    from pair p: stored as (x, y): (R, t); stored as (y, x): (R^T, t') with
 *              t'_c = -((R_0c * t_0 + R_1c * t_1) + R_2c * t_2).
 *   M = B o A  M.R_ij = ((B.R_i0 * A.R_0j + B.R_i1 * A.R_1j) + B.R_i2 * A.R_2j)
 *              M.t_i  = ((B.R_i0 * A.t_0 + B.R_i1 * A.t_1) + B.R_i2 * A.t_2) + B.t_i
 *   triangle   three edges p, q, r on three distinct sets a < b < c, p on {a, b}, q on {b, c}, r on {a, c}.  Repeated pairs are edges
 *              of their own: two pairs on {a, b} give two triangles with the same q and r.  Its error is
 *              E = T_r(c->a) o (T_q(b->c) o T_p(a->b)), with tr = (E.R_00 + E.R_11) + E.R_22 and
 *              e2 = (E.t_0 * E.t_0 + E.t_1 * E.t_1) + E.t_2 * E.t_2.
 *   consistent tr >= tr_min && e2 <= e2_max, both cuts inclusive.  No NaN arises from finite fp32 poses, so there is none to order:
 *              tr cannot overflow (three factors below 2^128 each), and nothing is infinite before the squares of e2.  e2 itself
 *              may overflow to +inf with hostile finite poses — an inverted pose's t' carried through two more poses puts |E.t|
 *              near 2^517 —; +inf is then the largest max_e2 there is, and it is never consistent, trans_tol being finite.
 *              A loop off by exactly a half turn (tr = -1) is not consistent at any rot_tol: at the largest one accepted, the
 *              float nearest pi, tr_min = -1 + 7.5e-15, that float being 8.7e-8 away from pi.
 *   rounds     alive_0 = edge.  Round k = 1, 2, ...: ok_k(p) = the consistent triangles of p whose three pairs are all in
 *              alive_{k-1}; alive_k(p) = alive_{k-1}(p) && (ok_k(p) >= min_ok || keep[p]).  The rounds stop after the first round K
 *              with alive_K == alive_{K-1} (stable), or at K = max_rounds.  The stable result is the largest sub-list in which
 *              every unprotected pair closes at least min_ok consistent loops inside the sub-list; it does not depend on order.
 * Outputs.  sc_cycle_result (48 bytes) per pair at d_res[p]; an invalid pair or a self pair has every count 0, min_trace 3.0,
 * max_e2 0.0, is never alive and takes part in nothing: its neighbours are untouched.  sc_cycle_summary (32 bytes) at d_sum.
 * Forms.  sc_pairs_cycles_device: poses, keep and outputs in HBM; it enqueues and returns without waiting, reads no host word, and
 * its number of stream operations depends on max_rounds only, never on n_pairs or the graph (a copy, a memset, max_rounds + 2
 * launches; a round's launch returns at once when the list is already stable).  (It may wait for the previous batch call's copy
 * out of the staging area the batch entries share.)  sc_pairs_cycles: host arrays; waits.  Like every batch entry they end the
 * frame a context may hold.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument
 * other than d_keep (a NULL ctx: no text); n_sets == 0, n_pairs == 0 or n_pairs > SC_CYCLES_MAX_PAIRS; a set index >= n_sets; a set
 * named by more than SC_CYCLES_MAX_DEGREE listed pairs (a self pair names its set once) — then no uint32 count can overflow: a
 * pair's triangles are at most deg a * deg b; size wrong, max_rounds outside 1 .. 64, rot_tol not finite or outside [0, pi] (the
 * float nearest pi is accepted), trans_tol not finite or negative, an unknown flag or a non-zero reserved word; a pose_stride that
 * breaks the pose rule; a call outstanding on the context.
 * Workspace: the copied list with every set's sorted neighbour entries, the oriented fp64 poses (192 bytes a pair), two alive bytes
 * a pair and the round words; the host form adds device copies of its arrays, in the pool every host form shares
 * (sc_register_batch).  Allocated by the first such call, counted in
 * workspace_bytes and held against the cap (SC_ENOMEM, nothing enqueued).  A context that never calls these entries allocates and
 * runs nothing new.
 * Not here: solving the pose graph; loops longer than three; weighting a loop's test by the pairs' information matrices; a sharded
 * form. */
#define SC_CYCLES_STATUS     1u         /* flags: a pose record holds an int32 status at byte 48 */
#define SC_CYCLES_MAX_PAIRS  4194304u   /* 2^22 */
#define SC_CYCLES_MAX_DEGREE 65535u     /* listed pairs that may name one set */
typedef struct sc_cycle_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_cycle_params)                                  */
  uint32_t min_ok;       /* consistent loops an unprotected pair must close; default 1 */
  uint32_t max_rounds;   /* 1 .. 64; default 16                                        */
  uint32_t flags;        /* SC_CYCLES_STATUS or 0                                      */
  float    rot_tol;      /* radians, finite, in [0, pi]                                */
  float    trans_tol;    /* finite, >= 0, in the poses' unit                           */
  uint32_t reserved[2];  /* must be 0                                                  */
} sc_cycle_params;
typedef struct sc_cycle_result {   /* 48 bytes */
  int32_t  status;         /* SC_OK, the status passed through, or SC_EINVAL for a non-finite Rt */
  uint32_t cycles;         /* triangles of alive_0 that contain p                      */
  uint32_t ok;             /* the consistent ones among them                           */
  uint32_t ok_alive;       /* ok_K(p); 0 if p is not in alive_{K-1}                    */
  uint32_t alive;          /* alive_K(p)                                               */
  uint32_t dropped_round;  /* the k at which p left; 0 if it is alive or never was an edge */
  double   min_trace;      /* min tr over p's `cycles` triangles; 3.0 when cycles is 0 */
  double   max_e2;         /* max e2 over p's `cycles` triangles; 0.0 when cycles is 0 */
  uint32_t reserved[2];    /* written as 0                                             */
} sc_cycle_result;
typedef struct sc_cycle_summary {  /* 32 bytes */
  uint32_t rounds;         /* K                                                        */
  uint32_t stable;         /* 1: alive_K == alive_{K-1}                                */
  uint32_t alive;          /* pairs in alive_K                                         */
  uint32_t edges;          /* pairs in alive_0                                         */
  uint64_t triangles;      /* triangles of alive_0                                     */
  uint64_t consistent;     /* the consistent ones among them                           */
} sc_cycle_summary;
int sc_cycles_default_params(sc_cycle_params* cp);   /* size, min_ok 1, max_rounds 16; everything else 0: the tolerances are the caller's */
/* host only, no context: out[0] = tr_min, out[1] = e2_max; SC_EINVAL for a NULL argument, a wrong size or a tolerance out of range */
int sc_cycles_thresholds(const sc_cycle_params* cp, double out[2]);
/* pairs a HOST array; d_pose n_pairs records of pose_stride bytes, d_keep n_pairs bytes or NULL, d_res n_pairs records, d_sum one */
int sc_pairs_cycles_device(sc_ctx* ctx, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp,
                           const void* d_pose, uint32_t pose_stride, const uint8_t* d_keep, sc_cycle_result* d_res,
                           sc_cycle_summary* d_sum);
/* the same with host arrays (pose, keep, res, sum); waits */
int sc_pairs_cycles(sc_ctx* ctx, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp,
                    const void* pose, uint32_t pose_stride, const uint8_t* keep, sc_cycle_result* res, sc_cycle_summary* sum);

/* ---- descriptor matching gated by several poses: sc_match_guided_poses --------------------------------------------
 * The entrance of the multi-motion chain: sc_register_instances / sc_peel find K rigid motions, sc_polish_poses refits them,
 * sc_assign_poses_frame relabels, sc_pose_info_frame weighs — and the match that produces better correspondences once the poses are
 * known took one pose.  K calls of sc_match_guided are not this operation: each re-assigns every source keypoint under its own pose
 * alone, the K lists overlap and disagree, and each call's mutual and ratio tests see that pose's admissible set only.  Here ONE
 * match is gated by the union over the poses: target j is a candidate for source i if SOME pose puts i near it, the nearest
 * descriptor among all such candidates wins, and every output entry says which pose admitted it.  A function of the input alone,
 * bit for bit; everything not named here — the descriptor distance, both u64 key orders, knn 1 .. 4, mutual and ratio over the
 * admissible set, the output order, the layouts, the determinism, frames and workspace — is sc_match_guided's.
 *   The pose records are those of sc_assign_poses / sc_polish_poses: n_poses records pose_stride bytes apart, float Rt[12] at byte
 *   0 and, with SC_GUIDE_POSE_STATUS in guide->flags (these entries accept it; sc_match_guided* keeps refusing it), an int32 status
 *   at byte 48.  pose_stride: a multiple of 4, >= 48, and >= 52 with the flag.  1 <= n_poses <= SC_GUIDE_MAX_POSES.  The records
 *   are read, never written.
 *   g2_k(i, j): the gate residual of sc_match_guided under record k; gate2 as there.
 *   use(k): true without the flag; with it, status_k == SC_OK.  A record that is not used is skipped: its Rt is neither read for
 *   the gate nor tested for finiteness (failed records of sc_register_instances_batch hold the identity, which would admit pairs).
 *   adm(i, j) <=> there is a k with use(k) and g2_k(i, j) < gate2, a float <: a NaN or infinite residual never admits.
 *   Every output entry (i, j): label = the used k with the smallest g2_k(i, j), ties to the lowest k; g2 = that minimum; the entry
 *   is admissible, so g2 < gate2.  label is n x int32 — the array sc_polish_poses and sc_pose_info_frame accept as SEL_LABEL
 *   (label0 = 0) when a registration on these correspondences has left its frame.
 *   count[0] = n; count[1] = 1 iff a descriptor, a point or one of the 12 floats of a USED record is not finite — then n = 0, and
 *   the host forms return SC_EINVAL with *n = 0.  As in sc_match_guided the flag depends on the whole input, not on what the gate
 *   drops.  No record used: n = 0, and count[1] reports the descriptors and points only.
 *   n_poses == 1 without the flag: corr, d2, g2 and count equal sc_match_guided_device on that pose bit for bit; every label is 0.
 * Stream operations of the device form: those of sc_match_guided_device — a memset and two launches, no host word.  d_pose is read
 * in stream order: it may be what sc_polish_poses_device, or a copy on the same stream, just wrote.
 * Refused with SC_EINVAL on the host before anything is enqueued, sc_last_error naming which: everything sc_match_guided refuses
 * (but SC_GUIDE_POSE_STATUS); a NULL d_pose; n_poses out of range; a pose_stride that breaks the rule; any other flag.
 * Not here: batch and pairs forms of the several-pose gate; a gate radius per pose; per-pose tallies (sc_assign_poses_frame counts
 * them); soft weighting by the residuals. */
#define SC_GUIDE_MAX_POSES 64u
/* Every buffer in HBM.  d_corr, d_d2, d_g2, d_count as sc_match_guided_device's; d_label: ns * knn int32 or NULL. */
int sc_match_guided_poses_device(sc_ctx* ctx, const float* d_src_pts, const float* d_fsrc, int64_t ns, const float* d_tgt_pts,
                                 const float* d_ftgt, int64_t nt, const sc_match_params* mp, const sc_guide_params* gp,
                                 const void* d_pose, uint32_t pose_stride, uint32_t n_poses, int32_t* d_corr, float* d_d2,
                                 float* d_g2, int32_t* d_label, uint32_t* d_count);
/* The same with host arrays (pose: n_poses * pose_stride bytes, copied as given; corr, d2, g2, label: room for ns * knn entries,
 * g2 and label may be NULL; the first *n are written); waits.  A non-finite descriptor, point or used pose: SC_EINVAL, *n = 0. */
int sc_match_guided_poses(sc_ctx* ctx, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt,
                          int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const void* pose, uint32_t pose_stride,
                          uint32_t n_poses, int32_t* corr, float* d2, float* g2, int32_t* label, uint32_t* n);
/* sc_register_guided_features with the several-pose match in front: that match, the gather on the device, then the unchanged
 * sc_register_device on the gathered arrays, with one host wait (the count).  guide->layout must equal params->layout; g2 and label
 * may be NULL.  corr, d2, g2, label, *n are valid whenever the match itself succeeded; n < 3: SC_ENOHYP with R = I, t = 0 and the
 * mask untouched; otherwise status, R, t, mask and stats are exactly those of sc_register on the gathered correspondences, and the
 * call leaves that frame: sc_polish_poses / sc_pose_info_frame with SEL_LABEL and the returned labels may follow. */
int sc_register_guided_poses_features(sc_ctx* ctx, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts,
                                      const float* ftgt, int64_t nt, const sc_match_params* mp, const sc_guide_params* gp,
                                      const void* pose, uint32_t pose_stride, uint32_t n_poses, const sc_params* params, float R[9],
                                      float t[3], int32_t* corr, float* d2, float* g2, int32_t* label, uint32_t* n, uint8_t* mask,
                                      sc_stats* stats);

/* ---- the fp64 information matrix of a batch's poses: sc_pose_info_batch ------------------------------------------
 * The callers of the batch entries feed every pair's pose into a pose graph or a fusion step as an EDGE, and an edge needs a
 * weight: the 6 x 6 information matrix of the point-to-point least-squares problem at the pose, summed over the pose's inliers,
 * and usually the inliers' sum of squared residuals.  These entries compute both for every problem of a batch in ONE launch, a
 * workgroup per problem (sc_info_batch.hip), behind sc_register_batch* / sc_polish_batch* on the same context and without a host
 * word.  Three forms, as sc_polish_batch has them: packed, slots (behind sc_register_batch_features_device) and pairs (behind
 * sc_register_pairs_features_device).
 *
 * Layout: the problems as the sibling form takes them (packed: d_src, d_tgt, offset a HOST array of n_problems + 1 words,
 * params->layout, 3 <= n_b <= SC_BATCH_MAX_N; slots / pairs: the points, the offsets or the table and the list, knn, d_corr and
 * d_count exactly as sc_polish_batch_slots_device / sc_polish_pairs_slots_device take them).  d_info receives n_problems records of
 * sc_pose_info_result.
 * The pose input: d_pose is an array of records of pose_stride bytes; problem b's record starts at byte b * pose_stride and holds
 * float Rt[12] at byte 0 and int32 status at byte 48 — nothing else of it is read.  sc_batch_result (stride 80) and
 * sc_polish_batch_result (stride 64) are such records, and so is one plane of sc_register_instances_batch's d_res.  pose_stride must
 * be a multiple of 4 and at least 52; d_pose must be 4-byte aligned.  d_pose is READ, never written, and need not come from this
 * library.  Of sc_params only tau and layout are read; it is checked as sc_register_batch checks it.
 *
 * Semantics, per problem with input status SC_OK, finite points and a finite Rt (R = Rt[0 .. 8] row-major, t = Rt[9 .. 11]):
 *   - correspondence m is an inlier iff it passes the canonical fp32 inlier test of (R, t) that the masks use; inliers = their
 *     number c.
 *   - for every inlier, in fp64:  x_r = (((double)R[r][0] * p0 + (double)R[r][1] * p1) + (double)R[r][2] * p2) + (double)t_r,
 *     e_r = x_r - (double)q_r.  The products of two fp32 values are exact in fp64, every sum is rounded to nearest, and there is
 *     no fused multiply-add anywhere.
 *   - ten sums: s_r = sum x_r (3), m_rs = sum x_r * x_s for r <= s (6), sse = sum ((e0 * e0 + e1 * e1) + e2 * e2) (1); each in the
 *     library's canonical order: chunks of 64 consecutive indices summed sequentially from 0.0 in index order over the chunk's
 *     inliers, then the chunk sums added sequentially in chunk order.
 *   - the matrix is that of the residual e = x - q under pose' = exp([w, v]) * pose — the perturbation applied on the LEFT, in the
 *     target frame, rotation first —: J = [-[x]x | I], info = sum J^T J, assembled from the sums entry by entry:
 *       rotation block           (m00 + m11 + m22) I - M:  info[0] = m11 + m22, info[7] = m00 + m22, info[14] = m00 + m11 (one
 *                                rounded add each), off the diagonal -m_rs (an exact negation)
 *       rotation-translation     [s]x: rows (0, -s2, s1), (s2, 0, -s0), (-s1, s0, 0); the translation-rotation block is its transpose
 *       translation block        c I
 *     so info is symmetric bit for bit.
 *   - c == 0: status SC_OK, every byte of info and sse zero.  Nothing is declined for c < 3: a caller that wants a well-posed edge
 *     looks at inliers and at the matrix.
 *   - no fp64 chain can overflow for finite fp32 input, whatever Rt holds: |x_r| <= 3 FLT_MAX^2 + FLT_MAX < 2^258, a term is below
 *     3 * 2^518 and a sum has at most 512 of them: below 2^530, far from DBL_MAX.
 *   - Input status != SC_OK: that status is passed through with a zero record.
 *   - Input status SC_OK but a non-finite coordinate, or a non-finite Rt: SC_EINVAL with a zero record.  It is found on the device,
 *     affects only that problem and does not fail the call.
 *   - slots / pairs: the problem is gathered through corr while staging.  A flagged problem, or one with count[2b] < 3 or above its
 *     capacity, passes its input status through (SC_EINVAL if that status claims SC_OK); an index in corr outside the problem is
 *     SC_EINVAL for that problem.
 *   - A record is a function of the problem's points, its pose and tau only: not of its position in the batch, of the neighbours,
 *     of n_problems or of the context's history — bit for bit.
 *
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument;
 * a pose_stride below 52 or no multiple of 4; everything sc_polish_batch / _slots_device / sc_polish_pairs_slots_device refuses of
 * the offsets, sc_params, knn, the table and the list; a call outstanding on the context.  The device forms enqueue on the context's
 * stream and return without waiting: outputs are complete in stream order.  (They may wait for the previous batch call's copy out of
 * the offset staging area, as the sibling entries do.)  All entries end the frame a context may hold and leave none.
 * Workspace: the copy of the offsets (records), a buffer of these entries' own, plus the host form's device copies of its arrays,
 * in the pool every host form shares (sc_register_batch); allocated by the first such call, counted in workspace_bytes and held against params->max_workspace (SC_ENOMEM).  A context that
 * never calls these entries allocates and runs nothing new.
 * Not here: a mask output (sc_polish_batch writes it); weights per correspondence.  (The form for a scored frame is
 * sc_pose_info_frame, below.) */
typedef struct sc_pose_info_result {   /* 320 bytes */
  double   info[36];    /* 6 x 6 row-major, symmetric; order: rotation x y z, translation x y z */
  double   sse;         /* sum over the inliers of |R p + t - q|^2, fp64                        */
  int32_t  status;      /* SC_OK, or why there is no matrix: SC_ENOHYP / SC_EINVAL              */
  uint32_t inliers;     /* correspondences that pass the canonical inlier test of the pose      */
  uint32_t reserved[4]; /* written as 0                                                         */
} sc_pose_info_result;
/* every buffer but offset in HBM: d_src / d_tgt total x 3 floats, d_pose n_problems records of pose_stride bytes, d_info n_problems records */
int sc_pose_info_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                              const sc_params* params, const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info);
/* the same with host arrays; waits */
int sc_pose_info_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                       const sc_params* params, const void* pose, uint32_t pose_stride, sc_pose_info_result* info);
/* behind sc_register_batch_features_device (and sc_polish_batch_slots_device): the points and both offset arrays as given there, its
 * d_corr and d_count */
int sc_pose_info_batch_slots_device(sc_ctx* ctx, const float* d_src_pts, const uint32_t* src_off, const float* d_tgt_pts,
                                    const uint32_t* tgt_off, uint32_t n_problems, uint32_t knn, const sc_params* params,
                                    const int32_t* d_corr, const uint32_t* d_count, const void* d_pose, uint32_t pose_stride,
                                    sc_pose_info_result* d_info);
/* behind sc_register_pairs_features_device (and sc_polish_pairs_slots_device): the table's points, set_off and pairs as given there,
 * its d_corr and d_count; d_pose and d_info n_pairs records */
int sc_pose_info_pairs_slots_device(sc_ctx* ctx, const float* d_pts, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs,
                                    uint32_t n_pairs, uint32_t knn, const sc_params* params, const int32_t* d_corr,
                                    const uint32_t* d_count, const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info);

/* ---- the fp64 information matrix on a scored frame: sc_pose_info_frame ------------------------------------------
 * sc_pose_info_batch weighs the edges a batch produces.  The large single frame — sc_register*, sc_peel, sc_register_instances and
 * sc_polish on 5 000 to 2^24 correspondences — is where the poses multiply: its winner, up to 64 polished candidates and one motion
 * per round of sc_peel, each of them an edge of a fusion step.  These entries give every such pose its information matrix, the
 * inliers' sum of squared residuals and their count in ONE launch, a workgroup per pose (sc_info_frame.hip), on the frame the context
 * holds, without a host word.
 *
 * A FRAME is as defined for sc_peel.  The entries read the frame's staged points, its n and its tau, and change nothing in it:
 * rounds of sc_peel and calls of sc_polish before or after are unaffected and do not affect it, and the call may be repeated.  They
 * do NOT end the frame — peel a round, take its information matrix, peel the next.  Correspondences are in the caller's ORIGINAL
 * indexing (the staged planes are in that order: it is the order sc_peel's masks are written in).
 *
 * The pose input: d_pose is an array of n_poses records of pose_stride bytes; pose k's record starts at byte k * pose_stride and holds
 * float Rt[12] at byte 0 — R = Rt[0 .. 8] row-major, t = Rt[9 .. 11] — and, with SC_POSE_INFO_STATUS, an int32 status at byte 48.
 * Without that flag nothing past byte 47 is read.  d_pose is READ, never written, must be 4-byte aligned and need not come from this
 * library.  All of these serve:
 *     the 12 floats of sc_register_device / sc_peel_device      stride 48   no flag
 *     the Rt array of sc_register_instances                     stride 48   no flag
 *     sc_polish_cand (rank sits at byte 48)                     stride 64   no flag
 *     sc_batch_result                                           stride 80   SC_POSE_INFO_STATUS
 *     sc_polish_batch_result                                    stride 64   SC_POSE_INFO_STATUS
 * pose_stride is a multiple of 4 and at least 48, at least 52 with the flag.
 * The selection: which correspondences may be inliers at all.  SC_POSE_INFO_SEL_NONE: every one (d_sel is not read; NULL).
 * SC_POSE_INFO_SEL_MASK: d_sel holds n bytes, m takes part iff d_sel[m] != 0, the same set for every pose — sc_peel's mask_r: in the
 * inlier-count mode inliers == that round's best_count for the round's fp32 winner.  SC_POSE_INFO_SEL_LABEL: d_sel holds n int32; for
 * pose k, m takes part iff d_sel[m] == label0 + (int32)k — sc_register_instances' label with label0 = 0 and its Rt array: in the
 * inlier-count mode inliers == score[k].  d_sel is READ, never written.
 *
 * Semantics, per pose k with a finite Rt (and, with the flag, status SC_OK): sc_pose_info_batch's, word for word.
 *   - correspondence m is an inlier iff it takes part per sel_mode AND passes the canonical fp32 inlier test of (R, t) that the
 *     masks use; inliers = their number c.
 *   - for every inlier, in fp64:  x_r = (((double)R[r][0] * p0 + (double)R[r][1] * p1) + (double)R[r][2] * p2) + (double)t_r,
 *     e_r = x_r - (double)q_r.  The products of two fp32 values are exact in fp64, every sum is rounded to nearest, and there is
 *     no fused multiply-add anywhere.
 *   - ten sums: s_r = sum x_r (3), m_rs = sum x_r * x_s for r <= s (6), sse = sum ((e0 * e0 + e1 * e1) + e2 * e2) (1); each in the
 *     library's canonical order: chunks of 64 consecutive indices summed sequentially from 0.0 in index order over the chunk's
 *     inliers, then the chunk sums added sequentially in chunk order.
 *   - info = sum J^T J, J = [-[x]x | I], assembled from the sums entry by entry exactly as sc_pose_info_batch assembles it (see
 *     there: the rotation block one rounded add or an exact negation per entry, [s]x and its transpose, c I), so info is symmetric
 *     bit for bit.
 *   - c == 0: status SC_OK, every byte of info and sse zero.  Nothing is declined for c < 3.
 *   - no fp64 chain can overflow for finite fp32 input, whatever Rt holds: |x_r| <= 3 FLT_MAX^2 + FLT_MAX < 2^258, a term is below
 *     3 * 2^518 < 2^520 and a sum has at most 2^24 of them: below 2^(518 + 2 + 24) = 2^544, far from DBL_MAX.
 *   - Where both entries can see the same problem — n <= SC_BATCH_MAX_N, the same points, pose and tau, SC_POSE_INFO_SEL_NONE — the
 *     record equals sc_pose_info_batch's, bit for bit.
 *   - A record is a function of the frame's input, the pose, the selection and tau only: not of k (but through SEL_LABEL), of
 *     n_poses, of the other poses, of how the frame was enqueued or of the context's history — bit for bit.
 *   - With SC_POSE_INFO_STATUS a status other than SC_OK at byte 48 is passed through with a zero record.
 *   - A non-finite Rt: SC_EINVAL with a zero record, for that pose only.  It is found on the device and does not fail the call.
 *     (The frame's points are finite already: staging checked them.)
 *
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL ctx (no
 * text), ip, d_pose or d_info; ip->size wrong; sel_mode above 2; d_sel NULL with a mode that reads it; label0 != 0 outside
 * SC_POSE_INFO_SEL_LABEL; an unknown flag or a non-zero reserved word; n_poses 0 or above SC_POSE_INFO_MAX_POSES; a pose_stride
 * that breaks the rule above; no frame on the context — also after any batch, match or sharded entry, or after a frame call that
 * returned SC_ENOHYP: sc_peel's refusal, with its text —; a call outstanding on the context.  A refused call leaves the frame.
 * The device form enqueues on the context's stream and returns without waiting, and needs no host word: d_info is complete in
 * stream order.  The host form copies in, enqueues, copies out and waits.
 * Workspace: the chunk sums' scratch — n_poses x ceil(n / 64) x 16 doubles, a buffer of these entries' own — plus the host form's
 * device copies, in the pool every host form shares (sc_register_batch); allocated by the first such call, counted in workspace_bytes and held against the frame's cap (SC_ENOMEM, nothing
 * enqueued, the frame stays).  A context that never calls these entries allocates and runs nothing new.
 * Not here: weights per correspondence; a form for sharded / multi-GPU frames, which leave no frame. */
#define SC_POSE_INFO_MAX_POSES 1024u
#define SC_POSE_INFO_SEL_NONE  0u   /* every correspondence of the frame may be an inlier                          */
#define SC_POSE_INFO_SEL_MASK  1u   /* sel: n bytes; m takes part iff sel[m] != 0 (the same set for every pose)     */
#define SC_POSE_INFO_SEL_LABEL 2u   /* sel: n int32; for pose k, m takes part iff sel[m] == label0 + (int32)k       */
#define SC_POSE_INFO_STATUS    1u   /* flags: a pose record holds an int32 status at byte 48 (as in the batch form) */
typedef struct sc_pose_info_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_pose_info_params) */
  uint32_t sel_mode;     /* SC_POSE_INFO_SEL_*            */
  int32_t  label0;       /* SEL_LABEL only, else 0        */
  uint32_t flags;        /* SC_POSE_INFO_STATUS or 0      */
  uint32_t reserved[4];  /* must be 0                     */
} sc_pose_info_params;
int sc_pose_info_default_params(sc_pose_info_params* ip);   /* size set, everything else 0 */
/* d_pose: n_poses records of pose_stride bytes, float Rt[12] at byte 0; d_sel per sel_mode (NULL with SEL_NONE); d_info: n_poses records */
int sc_pose_info_frame_device(sc_ctx* ctx, const sc_pose_info_params* ip, const void* d_pose, uint32_t pose_stride,
                              uint32_t n_poses, const void* d_sel, sc_pose_info_result* d_info);
/* the same with host arrays (pose, sel, info); waits */
int sc_pose_info_frame(sc_ctx* ctx, const sc_pose_info_params* ip, const void* pose, uint32_t pose_stride,
                       uint32_t n_poses, const void* sel, sc_pose_info_result* info);

/* ---- caller-supplied poses refitted on a scored frame: sc_polish_poses ---------------------------------------------
 * A large frame produces many poses — its winner, one motion per round of sc_peel / sc_register_instances, and poses the caller
 * brings along: the previous frame's pose, an odometry prior, a pose composed along a loop.  sc_polish iterates only the top
 * candidates of the frame's own total order, which all belong to the dominant motion; motions 1, 2, ... stay at their 3-point Kabsch
 * pose (SC_FLAG_REFINE adds at most one refit), and an external pose cannot be polished on a frame at all.  These entries iterate
 * "inliers of (R, t) -> fp64 least-squares refit -> inliers again" to a fixed point for up to SC_POLISH_POSES_MAX poses of ANY origin
 * on the frame the context holds: ONE launch, a workgroup per pose (sc_polish_poses.hip), no host word.  It is what
 * sc_polish_batch_device does for any pose record of a batch, for the frame.
 *
 * A FRAME is as defined for sc_peel.  The entries read the frame's staged points, its n, tau and score_mode, and change nothing in
 * it: they do NOT end the frame, may be repeated, and may be interleaved with sc_peel, sc_polish and sc_pose_info_frame, which are
 * unaffected and do not affect them.  Correspondences are in the caller's ORIGINAL indexing.
 *
 * The pose input follows sc_pose_info_frame exactly: d_pose is an array of n_poses records of pose_stride bytes; pose k's record
 * starts at byte k * pose_stride and holds float Rt[12] at byte 0 and, with SC_POLISH_POSES_STATUS, an int32 status at byte 48;
 * without that flag nothing past byte 47 is read.  pose_stride is a multiple of 4 and at least 48, at least 52 with the flag.  d_pose
 * is READ, never written, must be 4-byte aligned and need not come from this library (see sc_pose_info_frame for the records that
 * serve).  The output record is sc_polish_batch_result (64 bytes): it is therefore itself a pose record for
 * sc_pose_info_frame_device (stride 64, SC_POSE_INFO_STATUS) and for a further sc_polish_poses_device (stride 64,
 * SC_POLISH_POSES_STATUS).  d_mask, if not NULL, receives n_poses x n bytes: pose k's mask is bytes [k * n, (k + 1) * n).
 *
 * The selection: which correspondences take part for pose k — part(m).  SC_POLISH_POSES_SEL_NONE: every one (d_sel is not read;
 * NULL).  _SEL_MASK: d_sel holds n bytes, part(m) iff d_sel[m] != 0, the same set for every pose (sc_peel's mask_r).  _SEL_LABEL:
 * d_sel holds n int32, part(m) iff d_sel[m] == label0 + k (what motion k of sc_register_instances claimed).  _SEL_ALIVE: d_sel holds
 * n int32, part(m) iff d_sel[m] < label0 or d_sel[m] >= label0 + k — with sc_register_instances' label and label0 = 0 the
 * correspondences that were alive in sc_peel's round k: claimed by no motion, or by motion k or a later one.  label0 + k is a
 * wrapping 32-bit add, compared as int32, as sc_pose_info_frame computes it.  d_sel is READ, never written.
 *
 * Semantics, per pose k with a finite Rt (and, with the flag, status SC_OK): step 2 of sc_polish with part ANDed into every inlier
 * set.  Rt_0 = the input; for it = 1 .. max_iter: mask = part(m) && the canonical inlier test of Rt_{it-1}; Rt_it = the fp64 refit
 * over that mask in its canonical order — chunks of 64 consecutive ORIGINAL indices — rounded to fp32; stop when the refit is
 * declined (fewer than 3 inliers, or a non-finite result: SC_POLISH_STOP_DECLINED), when Rt_it equals Rt_{it-1} bit for bit
 * (SC_POLISH_STOP_FIXED), or after max_iter refits (SC_POLISH_STOP_MAX_ITER).  iters = the refits that changed (R, t); Rt = the last
 * iterate; score0 / score = the frame's score_mode score of Rt_0 / of Rt over the correspondences that take part; mask byte m =
 * part(m) && the inlier test of Rt.
 *   - A first refit that is declined: status SC_OK, Rt = the input's bits, iters 0, score = score0.
 *   - With the flag, a status other than SC_OK is passed through; R = I, t = 0, scores 0, iters 0, stop SC_POLISH_STOP_DECLINED, mask
 *     zero.
 *   - A non-finite Rt: SC_EINVAL with the same output shape, for that pose only.  It is found on the device and does not fail the
 *     call.  (The frame's points are finite already: staging checked them.)
 *   - A record is a function of the frame's input, the pose, the selection, tau, score_mode and max_iter only, bit for bit: not of k
 *     (but through SEL_LABEL / SEL_ALIVE), of n_poses, of the other poses, of how the frame was enqueued or of the context's history.
 * Equalities, each bit for bit:
 *   1. SEL_NONE and the frame's fp32 winner as pose: Rt, score0, score, iters and the mask are those of
 *      sc_polish(candidates = 1, the same max_iter).
 *   2. SEL_NONE and a hypothesis of the ranked list as pose: the result is that hypothesis' sc_polish_cand record.
 *   3. n <= SC_BATCH_MAX_N, the same points, pose and parameters, SEL_NONE: the 64-byte record and the mask are sc_polish_batch's.
 *   4. SEL_ALIVE, label0 = 0, max_iter = 1, and the label and Rt arrays of sc_register_instances WITHOUT SC_FLAG_REFINE: Rt[k] is what
 *      the same call WITH SC_FLAG_REFINE returns for motion k — both are the refit over mask_k in original indexing — and score0[k]
 *      is that call's score[k], in every score mode.
 *   5. SEL_MASK with sc_peel's mask_r and max_iter = 1: Rt is that round's SC_FLAG_REFINE pose.
 *
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL ctx (no
 * text), params, d_pose or d_pol; params->size wrong; max_iter outside 1 .. 64; sel_mode above 3; d_sel NULL with a mode that reads
 * it; label0 != 0 with SEL_NONE or SEL_MASK; an unknown flag or a non-zero reserved word; n_poses 0 or above SC_POLISH_POSES_MAX; a
 * pose_stride that breaks the rule above; no frame on the context (sc_peel's refusal, with its text); a call outstanding on the
 * context.  A refused call leaves the frame.  The device form enqueues on the context's stream and returns without waiting, and
 * needs no host word: d_pol and d_mask are complete in stream order.  The host form copies in, enqueues, copies out and waits.
 * Workspace: the chunk sums' scratch — n_poses x ceil(n / 64) x 16 doubles, a buffer of these entries' own — plus the host form's
 * device copies (n_poses x n mask bytes among them when a mask is asked for), in the pool every host form shares; allocated by the first such call, counted in
 * workspace_bytes and held against the frame's cap (SC_ENOMEM, nothing enqueued, the frame stays).  A context that never calls these
 * entries allocates and runs nothing new.
 * Not here: a relabelled label output (sc_assign_poses_frame, below, writes it); a form for sharded frames; weights per correspondence; a batch form (sc_polish_batch takes
 * arbitrary poses already). */
#define SC_POLISH_POSES_MAX        1024u
#define SC_POLISH_POSES_SEL_NONE   0u  /* every correspondence takes part                                                    */
#define SC_POLISH_POSES_SEL_MASK   1u  /* sel: n bytes; m takes part iff sel[m] != 0 (the same set for every pose)            */
#define SC_POLISH_POSES_SEL_LABEL  2u  /* sel: n int32; pose k: m takes part iff sel[m] == label0 + k                         */
#define SC_POLISH_POSES_SEL_ALIVE  3u  /* sel: n int32; pose k: m takes part iff sel[m] < label0 or sel[m] >= label0 + k      */
#define SC_POLISH_POSES_STATUS     1u  /* flags: a pose record holds an int32 status at byte 48                               */
typedef struct sc_polish_poses_params {  /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_polish_poses_params)   */
  uint32_t max_iter;     /* refits per pose at most, 1 .. 64   */
  uint32_t sel_mode;     /* SC_POLISH_POSES_SEL_*              */
  int32_t  label0;       /* SEL_LABEL / SEL_ALIVE only, else 0 */
  uint32_t flags;        /* SC_POLISH_POSES_STATUS or 0        */
  uint32_t reserved[3];  /* must be 0                          */
} sc_polish_poses_params;
int sc_polish_poses_default_params(sc_polish_poses_params* qp);   /* size set, max_iter 16, everything else 0 */
/* d_pose: n_poses records of pose_stride bytes, float Rt[12] at byte 0; d_sel per sel_mode (NULL with SEL_NONE); d_pol: n_poses
 * records; d_mask: n_poses x n bytes, or NULL */
int sc_polish_poses_device(sc_ctx* ctx, const sc_polish_poses_params* qp, const void* d_pose, uint32_t pose_stride,
                           uint32_t n_poses, const void* d_sel, sc_polish_batch_result* d_pol, uint8_t* d_mask);
/* the same with host arrays (pose, sel, pol, mask); waits */
int sc_polish_poses(sc_ctx* ctx, const sc_polish_poses_params* qp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                    const void* sel, sc_polish_batch_result* pol, uint8_t* mask);

/* ---- correspondences labelled by the pose that fits best: sc_assign_poses ------------------------------------------
 * The library refits a list of poses (sc_polish_poses, sc_polish_batch), weighs it (sc_pose_info_frame, sc_pose_info_batch) and
 * restricts either to a label array (SEL_LABEL, SEL_ALIVE), but the only label array it produced was the greedy one of
 * sc_register_instances*: motion k owns what motions 0 .. k-1 left inside tau of its UNREFINED pose.  Once the motions are polished
 * that label is stale, and a pose a caller brings along has none.  These entries are the hard-assignment step of a multi-model fit:
 * K pose records in, every correspondence labelled with one pose or -1, and per pose how many correspondences it got and what they
 * score.  Two forms, where the poses multiply: on a scored frame (ONE kernel launch behind one memset, sc_assign_frame.hip) and on a
 * packed batch (ONE launch, a workgroup per problem, sc_assign_batch.hip).  No host word in either.
 *
 * Definitions, shared by both forms.  Pose records are those of sc_pose_info_frame / sc_polish_poses: float Rt[12] at byte 0 —
 * R = Rt[0 .. 8] row-major, t = Rt[9 .. 11] — and, where a status is read, an int32 at byte 48; read, never written; 4-byte aligned.
 *   valid(k)    Rt is finite and, where a status is read, it is SC_OK.
 *   d2_k(m)     the canonical fp32 squared residual of the masks' inlier test: e_c = t_c + fma(R_c2, pz, fma(R_c1, py, fma(R_c0, px,
 *               -q_c))), d2 = fma(ez, ez, fma(ey, ey, ex * ex)).
 *   part(m)     SC_ASSIGN_SEL_NONE: every m.  SC_ASSIGN_SEL_MASK: d_sel holds n bytes, m takes part iff d_sel[m] != 0.
 *   cand(k, m)  valid(k) && part(m) && d2_k(m) < tau^2 — tau^2 derived as the masks derive it, a float '<': a NaN residual (a finite
 *               pose with entries near FLT_MAX can produce one) is never a candidate.
 *   mode        SC_ASSIGN_BEST: label[m] = the candidate k with the smallest d2_k(m), ties to the lowest k; -1 without a candidate.
 *               SC_ASSIGN_FIRST: label[m] = the lowest candidate k, else -1 — the claim order of sc_peel: on the Rt array of
 *               sc_register_instances run without SC_FLAG_REFINE it returns that call's label.
 *   d2 output   optional (NULL): d2_label[m](m), or the bits 0x7F800000 (+inf) where the label is -1.
 *   record k    sc_assign_result: count = #{m : label[m] == k}; score = the sum over those m of the frame's (params->) score_mode term
 *               of pose k — in the inlier-count mode score == count —; status SC_OK for a valid pose; a status other than SC_OK at
 *               byte 48 is passed through and a non-finite Rt gives SC_EINVAL, both with count = score = 0: an invalid pose claims
 *               nothing, is found on the device and does not fail the call.  reserved is written 0.
 *   Every output is a function of the points, the poses in their order, the selection, tau and score_mode, bit for bit: not of how the
 *   frame was enqueued, of the context's history or of the launch geometry (the per-pose sums are sums of integers).
 *
 * The frame form.  A FRAME is as defined for sc_peel.  The entries read the frame's staged points, its n, tau and score_mode, change
 * nothing in it and do NOT end it: they may be repeated and interleaved with sc_peel, sc_polish* and sc_pose_info_frame.  d_label:
 * n int32 in the caller's ORIGINAL indexing; d_d2: n floats or NULL; d_asg: n_poses records.  SC_ASSIGN_STATUS: the record holds a
 * status at byte 48; without it nothing past byte 47 is read.  pose_stride is a multiple of 4 and at least 48, at least 52 with the
 * flag; 1 <= n_poses <= SC_ASSIGN_MAX_POSES.  The device form enqueues two stream operations whatever n and n_poses are — a memset of
 * d_asg and the kernel — and returns without waiting; the host form copies in, enqueues, copies out and waits.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL ctx (no
 * text), ap, d_pose, d_label or d_asg; ap->size wrong; mode above 1; sel_mode above 1; d_sel NULL with SC_ASSIGN_SEL_MASK; an
 * unknown flag or a non-zero reserved word; n_poses out of range; a pose_stride that breaks the rule; no frame on the context
 * (sc_peel's refusal, with its text); a call outstanding on the context.  A refused call leaves the frame.
 * Workspace: the device form needs none — the tallies are added into d_asg itself —; the host form's device copies are slots of the
 * pool every host form shares (sc_register_batch), allocated by the first such call, counted in workspace_bytes and held against the frame's cap (SC_ENOMEM,
 * nothing enqueued, the frame stays).  A context that never calls these entries allocates nothing new.
 * The loop this closes, every step stream-ordered: sc_register_instances -> sc_polish_poses_device(SEL_ALIVE) ->
 * sc_assign_poses_frame_device(BEST) -> sc_polish_poses_device(SEL_LABEL, max_iter = 1) -> sc_pose_info_frame_device(SEL_LABEL), so
 * that no correspondence is counted in two edges' matrices.
 *
 * The batch form, packed only.  The problems of sc_register_batch (d_src, d_tgt, offset a HOST array, params->layout, 3 <= n_b <=
 * SC_BATCH_MAX_N).  The poses motion-major, exactly as sc_register_instances_batch writes d_res: pose k of problem b starts at byte
 * (k * n_problems + b) * pose_stride; the status at byte 48 is always read (pose_stride at least 52; SC_ASSIGN_STATUS may be set or
 * not); 1 <= n_poses <= SC_ASSIGN_BATCH_MAX_POSES; sel_mode must be SC_ASSIGN_SEL_NONE.  d_label: total int32 positioned like
 * sc_register_batch's mask, every entry of a problem's range written; d_asg: n_poses x n_problems records, motion-major.  params is
 * checked as sc_register_batch checks it; only tau, score_mode and layout are read.  A problem holding a non-finite coordinate gets
 * label -1 throughout and SC_EINVAL in every one of its records; its neighbours are untouched.  A problem's outputs do not depend on
 * its position in the batch or on n_problems.  Like every batch entry it ends the frame a context may hold.  Refusals, workspace
 * (the copy of the offsets, the host form's device copies) and the offset staging wait are sc_pose_info_batch_device's.
 * Not here: slots and pairs forms; soft or weighted assignment; "relabel and refit until stable" (an entry of its own:
 * sc_settle_poses, below); merging or dropping poses (an entry of its own: sc_merge_poses, below); a form for sharded frames, which
 * leave no frame. */
#define SC_ASSIGN_MAX_POSES       1024u
#define SC_ASSIGN_BATCH_MAX_POSES 64u
#define SC_ASSIGN_BEST     0u   /* mode: the candidate with the smallest residual, ties to the lowest k */
#define SC_ASSIGN_FIRST    1u   /* mode: the lowest candidate k (sc_peel's claim order)                 */
#define SC_ASSIGN_SEL_NONE 0u   /* every correspondence takes part                                      */
#define SC_ASSIGN_SEL_MASK 1u   /* sel: n bytes; m takes part iff sel[m] != 0                           */
#define SC_ASSIGN_STATUS   1u   /* flags: a pose record holds an int32 status at byte 48                */
typedef struct sc_assign_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_assign_params)  */
  uint32_t mode;         /* SC_ASSIGN_BEST / _FIRST     */
  uint32_t sel_mode;     /* SC_ASSIGN_SEL_*             */
  uint32_t flags;        /* SC_ASSIGN_STATUS or 0       */
  uint32_t reserved[4];  /* must be 0                   */
} sc_assign_params;
typedef struct sc_assign_result {   /* 32 bytes */
  int32_t  status;       /* SC_OK, the status passed through, or SC_EINVAL   */
  uint32_t count;        /* correspondences labelled with this pose          */
  uint64_t score;        /* their score terms, summed (score_mode)           */
  uint32_t reserved[4];  /* written as 0                                     */
} sc_assign_result;
int sc_assign_default_params(sc_assign_params* ap);   /* size set, everything else 0 */
/* d_pose: n_poses records of pose_stride bytes; d_sel per sel_mode (NULL with SEL_NONE); d_label: n int32; d_d2: n floats or NULL;
 * d_asg: n_poses records */
int sc_assign_poses_frame_device(sc_ctx* ctx, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                 const uint8_t* d_sel, int32_t* d_label, float* d_d2, sc_assign_result* d_asg);
/* the same with host arrays (pose, sel, label, d2, asg); waits */
int sc_assign_poses_frame(sc_ctx* ctx, const sc_assign_params* ap, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          const uint8_t* sel, int32_t* label, float* d2, sc_assign_result* asg);
/* every buffer but offset in HBM: d_src / d_tgt total x 3 floats, d_pose n_poses x n_problems records of pose_stride bytes
 * (motion-major), d_label total int32, d_asg n_poses x n_problems records (motion-major) */
int sc_assign_poses_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                 const sc_params* params, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride,
                                 uint32_t n_poses, int32_t* d_label, sc_assign_result* d_asg);
/* the same with host arrays; waits */
int sc_assign_poses_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                          const sc_params* params, const sc_assign_params* ap, const void* pose, uint32_t pose_stride,
                          uint32_t n_poses, int32_t* label, sc_assign_result* asg);

/* ---- poses relabelled and refitted until stable: sc_settle_poses -----------------------------------------------------
 * The loop the entries above leave to the caller — sc_assign_poses(BEST), then sc_polish_poses(SEL_LABEL, max_iter 1) on its label,
 * again until no pose moves — has a stopping rule only the device knows.  A host-free caller enqueues max_iter rounds whether or not
 * the poses settled in the second; one who stops early pays a host round trip per round.  These entries run the loop to its fixed
 * point ON THE DEVICE, in ONE kernel launch without a grid barrier, and read nothing back.  Two forms: on a scored frame (ONE
 * workgroup owns the frame, sc_settle_frame.hip) and on a packed batch (a workgroup per problem, sc_settle_batch.hip).
 *
 * Definitions.  The pose records, valid(k), d2_k(m), part(m), cand(k, m) and the SC_ASSIGN_BEST rule are sc_assign_poses's, word for
 * word: float Rt[12] at byte 0 and, where a status is read, an int32 at byte 48; read, never written; 4-byte aligned.  The refit is
 * sc_polish_poses's single refit: the canonical fp64 refit over a set, in chunks of 64 consecutive ORIGINAL indices, chunk sums in
 * chunk order, rounded to fp32; declined with fewer than 3 members or a non-finite result.
 *   P_0         the input.  A pose that is invalid in P_0 stays invalid and claims nothing.
 *   round r     r = 1 .. max_iter.  L_r = the BEST labels under P_{r-1} and the selection.  For every valid k, P_r[k] = the refit over
 *               {m : L_r[m] == k}; a declined refit leaves P_r[k] = P_{r-1}[k], bit for bit.  If P_r equals P_{r-1} bit for bit in
 *               every pose the call stops with SC_POLISH_STOP_FIXED and this round is NOT counted; otherwise it is counted.
 *   stop        after max_iter counted rounds: SC_POLISH_STOP_MAX_ITER.
 *   d_label     n int32: the BEST labels under the FINAL poses (after FIXED the last round's; after MAX_ITER one more labelling
 *               pass); -1 without a candidate.  d_d2 (frame form, or NULL): their residuals, 0x7F800000 (+inf) where the label is -1.
 *   record k    sc_polish_batch_result: Rt = the final pose; score0 = pose k's tally — the frame's / params->score_mode term summed
 *               over its label — under P_0 and L_1; score = the tally under the final poses and labels; iters = the counted rounds
 *               in which pose k's bits changed; stop = SC_POLISH_STOP_DECLINED if pose k's refit was declined in the last executed
 *               round, else the call's stop; status SC_OK.  An invalid pose gets sc_polish_poses's record for it: the status
 *               passed through, or SC_EINVAL for a non-finite Rt; R = I, t = 0, scores 0, iters 0, SC_POLISH_STOP_DECLINED.  The
 *               records are therefore a pose list for sc_pose_info_frame_device, sc_polish_poses_device, sc_assign_poses_* and for
 *               this entry again (stride 64, with the status flag).
 *   d_rounds    two words (NULL: not wanted): [0] the counted rounds, [1] the call's stop.
 *   Every output is a function of the points, the poses in their order, the selection, tau, score_mode and max_iter only, bit for bit:
 *   not of the launch geometry, the context's history, how the frame was enqueued, or (batch) a problem's position or n_problems.
 * What the header promises, each bit for bit:
 *   (1) the composed loop.  With R = d_rounds[0], plus 1 after FIXED: R rounds of sc_assign_poses_frame_device(BEST, the same
 *       selection) followed by sc_polish_poses_device(SEL_LABEL, label0 0, max_iter 1, SC_POLISH_POSES_STATUS), each fed the round
 *       before's records at stride 64, end in the same Rt; one more sc_assign_poses_frame_device on them writes d_label, d_d2 and,
 *       as its scores, every record's score.
 *   (2) n_poses == 1 with SC_ASSIGN_SEL_NONE: the record is sc_polish_poses's (SEL_NONE, the same max_iter), label[m] == mask[m] - 1.
 *   (3) a batch problem's records, labels and rounds are the frame form's on that problem alone.
 *   (4) a list that came out with SC_POLISH_STOP_FIXED goes in again and comes out with 0 rounds and the same bytes.
 *
 * The frame form.  A FRAME is as defined for sc_peel.  The entries read the frame's staged points, its n, tau and score_mode, change
 * nothing in it and do NOT end it: they may be repeated and interleaved with sc_peel, sc_polish*, sc_pose_info_frame and
 * sc_assign_poses_frame.  Correspondences are in the caller's ORIGINAL indexing.  sel_mode SC_ASSIGN_SEL_NONE or SC_ASSIGN_SEL_MASK
 * (d_sel: n bytes).  SC_SETTLE_STATUS: the pose record holds a status at byte 48; without it nothing past byte 47 is read.
 * pose_stride is a multiple of 4 and at least 48, at least 52 with the flag; 1 <= n_poses <= SC_SETTLE_MAX_POSES.  The device form
 * enqueues ONE launch whatever n, n_poses and max_iter are and returns without waiting; the host form copies in, enqueues, copies
 * out and waits.
 * The batch form, packed only.  The problems of sc_register_batch (offset a HOST array, params->layout, 3 <= n_b <= SC_BATCH_MAX_N);
 * the poses and the records motion-major as sc_assign_poses_batch has them — one plane of sc_register_instances_batch's d_res per
 * pose, stride 80 —, the status at byte 48 always read (pose_stride at least 52); 1 <= n_poses <= SC_SETTLE_BATCH_MAX_POSES; sel_mode
 * must be SC_ASSIGN_SEL_NONE.  d_label: total int32 positioned like sc_register_batch's mask; d_rounds: two words per problem.  A
 * problem holding a non-finite coordinate gets label -1 throughout, SC_EINVAL in every one of its records (R = I, zeros,
 * SC_POLISH_STOP_DECLINED) and the words 0, SC_POLISH_STOP_DECLINED; its neighbours are untouched.  Like every batch entry it ends
 * the frame a context may hold.  params is checked as sc_register_batch checks it; only tau, score_mode and layout are read.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument
 * (a NULL ctx: no text; d_d2 and d_rounds may be NULL); sp->size wrong; max_iter outside 1 .. 64; sel_mode above 1 (batch: not 0);
 * d_sel NULL with SC_ASSIGN_SEL_MASK; an unknown flag or a non-zero reserved word; n_poses 0 or above the form's maximum; a
 * pose_stride that breaks the rule; no frame on the context (sc_peel's refusal, with its text); a call outstanding on the context;
 * the batch form's offsets and params as sc_assign_poses_batch refuses them.  A refused call leaves the frame.
 * Workspace: the frame form keeps the member bits and chunk sums of a round in n_poses x ceil(n / 64) x 16 doubles — the buffer
 * sc_polish_poses keeps, shared: the calls are stream-ordered, a context that uses both holds one —; the batch form the copy of the
 * offsets; the host forms device copies of their arrays, in the pool every host form shares
 * (sc_register_batch).  Everything is allocated by the first such call, counted in
 * workspace_bytes and held against the cap (SC_ENOMEM, nothing enqueued, the frame stays).  A context that never calls these entries
 * allocates and runs nothing new.
 * The loop this closes, every step stream-ordered and none read back: sc_register_instances -> sc_polish_poses_device(SEL_ALIVE) ->
 * sc_settle_poses_frame_device -> sc_pose_info_frame_device(SEL_LABEL, d_label, stride 64).
 * Not here: merging or dropping poses (an entry of its own: sc_merge_poses, below) (two copies of a pose split its inliers between
 * them by the tie rule: the lower k takes the ties, both stay in the list); soft assignment; slots and pairs forms; a form for sharded frames, which leave no frame. */
#define SC_SETTLE_MAX_POSES       64u   /* frame form */
#define SC_SETTLE_BATCH_MAX_POSES 16u   /* batch form: SC_INSTANCES_BATCH_MAX planes */
#define SC_SETTLE_STATUS 1u             /* flags: a pose record holds an int32 status at byte 48 */
typedef struct sc_settle_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_settle_params)                      */
  uint32_t max_iter;     /* counted rounds at most, 1 .. 64                 */
  uint32_t sel_mode;     /* SC_ASSIGN_SEL_NONE / _MASK; batch: _NONE        */
  uint32_t flags;        /* SC_SETTLE_STATUS or 0                           */
  uint32_t reserved[4];  /* must be 0                                       */
} sc_settle_params;
int sc_settle_default_params(sc_settle_params* sp);   /* size set, max_iter 16, everything else 0 */
/* d_pose: n_poses records of pose_stride bytes; d_sel per sel_mode (NULL with SEL_NONE); d_pol: n_poses records; d_label: n int32;
 * d_d2: n floats or NULL; d_rounds: 2 words or NULL */
int sc_settle_poses_frame_device(sc_ctx* ctx, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                 const uint8_t* d_sel, sc_polish_batch_result* d_pol, int32_t* d_label, float* d_d2, uint32_t* d_rounds);
/* the same with host arrays (pose, sel, pol, label, d2, rounds); waits */
int sc_settle_poses_frame(sc_ctx* ctx, const sc_settle_params* sp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          const uint8_t* sel, sc_polish_batch_result* pol, int32_t* label, float* d2, uint32_t* rounds);
/* every buffer but offset in HBM: d_src / d_tgt total x 3 floats, d_pose n_poses x n_problems records of pose_stride bytes
 * (motion-major), d_pol n_poses x n_problems records (motion-major), d_label total int32, d_rounds 2 x n_problems words or NULL */
int sc_settle_poses_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                 const sc_params* params, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride,
                                 uint32_t n_poses, sc_polish_batch_result* d_pol, int32_t* d_label, uint32_t* d_rounds);
/* the same with host arrays; waits */
int sc_settle_poses_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                          const sc_params* params, const sc_settle_params* sp, const void* pose, uint32_t pose_stride,
                          uint32_t n_poses, sc_polish_batch_result* pol, int32_t* label, uint32_t* rounds);

/* ---- duplicate poses found and folded: sc_merge_poses ----------------------------------------------------------------
 * A round of sc_peel scores over what the winner before left alive, so the next "motion" is often the same motion again, found on its
 * borderline correspondences; a pose a caller brings along (the previous frame's, an odometry prior) usually duplicates a motion of
 * the frame.  sc_settle_poses keeps both copies and splits the motion's inliers between them, and sc_pose_info_frame then sees two
 * weak edges where there is one strong edge.  "Are these two the same motion?" needs every pose's support set over all n
 * correspondences and the K x K table of their intersections: these entries build both ON THE DEVICE, decide there, and read nothing
 * back.  Two forms: on a scored frame (three launches behind one memset: sc_merge_frame.hip) and on a packed batch (ONE launch, a
 * workgroup per problem: sc_merge_batch.hip).
 *
 * Definitions, shared by both forms.  The pose records, valid(k), d2_k(m), part(m) and cand(k, m) are sc_assign_poses's, word for
 * word: float Rt[12] at byte 0 and, where a status is read (SC_MERGE_STATUS; the batch form always), an int32 at byte 48; read, never
 * written; 4-byte aligned.  An invalid pose is found on the device and does not fail the call.
 *   support     I_k = {m : cand(k, m)}: pose k's OWN inlier set — not an exclusive label: the sets of different poses overlap, and that
 *               is the point.  c_k = |I_k|.  s_k = the sum over I_k of the frame's (params->) score_mode term of pose k, as a uint32:
 *               the score0 sc_polish_poses reports for that pose under the same selection.  x_jk = |I_j & I_k|.
 *   strength    larger s_k first, ties to the lower k.
 *   same(j, k)  x_jk >= 1 and, in 64-bit unsigned integer arithmetic, SC_MERGE_OVER_MIN: x_jk * den >= num * min(c_j, c_k);
 *               SC_MERGE_OVER_UNION (Jaccard): x_jk * den >= num * (c_j + c_k - x_jk).  1 <= num <= den <= 65536.  No floating point
 *               enters the decision.
 *   the fold    greedy, the poses visited in strength order.  An invalid pose is out: parent -1.  A valid pose with c_k < min_count is
 *               dropped: parent -1.  Otherwise, if some pose j that is already kept has same(j, k), k is FOLDED into the strongest such
 *               j: parent[k] = j.  Otherwise k is KEPT: parent[k] = k.  Nothing is refitted: a kept pose keeps its input bits;
 *               sc_settle_poses or sc_polish_poses on the output does the refit over the united support.
 *   record      sc_merge_pose, 64 bytes, by the pose's fate:
 *                 kept     Rt = the input's bits, status SC_OK,     index = k,          count = c_k, score = s_k
 *                 folded   R = I, t = 0,          status SC_ENOHYP, index = its parent, count = c_k, score = s_k
 *                 dropped  R = I, t = 0,          status SC_ENOHYP, index = -1,         count = c_k, score = s_k
 *                 invalid  R = I, t = 0,          the status passed through, or SC_EINVAL for a non-finite Rt, index = -1, 0, 0
 *               The record is itself a pose record — Rt at byte 0, the status at byte 48 — for sc_settle_poses_*, sc_assign_poses_*,
 *               sc_polish_poses_device, sc_pose_info_frame_device and this entry again, read at stride 64 with their status flag: the
 *               dead records claim nothing.
 *   placement   without SC_MERGE_COMPACT the record of pose k sits at position k, so labels written by later entries keep the caller's
 *               pose numbers.  With it the list is stably partitioned: the kept poses first, in ascending k, then the others, in
 *               ascending k.  Either way there are n_poses records: a host-free caller passes the same n_poses on; one who waits
 *               reads the kept count and passes that on.
 *   d_parent    n_poses int32, by pose number (whatever the placement).
 *   d_count     two words (NULL: not wanted): [0] the kept poses, [1] the valid poses.  The batch form: two words per problem.
 *   d_overlap   the frame form only; NULL: not wanted.  n_poses x n_poses uint32, x_jk: symmetric, the diagonal is c_k, the rows and
 *               columns of invalid poses are 0.
 *   Every output is a function of the points, the poses in their order, the selection, tau, score_mode and sc_merge_params only, bit
 *   for bit: not of the launch geometry, the context's history, how the frame was enqueued, or (batch) a problem's position or
 *   n_problems.  Every sum is a sum of integers.
 * What the header promises, each bit for bit:
 *   (1) score[k] is sc_polish_poses's score0[k] under the same selection, in all three score modes; count[k] = #{m : part(m) and
 *       d2_k(m) < tau^2}.
 *   (2) a bit-identical copy of a valid pose with c_k >= 1 is folded into its lowest-numbered original (or that original's parent),
 *       for every num / den and either measure: it is never kept beside it.
 *   (3) the kept records, fed in again (stride 64, SC_MERGE_STATUS, the same parameters), are all kept again: d_count[0] and their
 *       bytes are unchanged.
 *   (4) a batch problem's outputs are the frame form's on that problem alone.
 *   (5) with num == den and SC_MERGE_OVER_MIN, k is folded into a kept j exactly when one support set contains the other.
 *
 * The frame form.  A FRAME is as defined for sc_peel.  The entries read the frame's staged points, its n, tau and score_mode, change
 * nothing in it and do NOT end it: they may be repeated and interleaved with sc_peel, sc_polish*, sc_pose_info_frame,
 * sc_assign_poses_frame and sc_settle_poses_frame.  Correspondences are in the caller's ORIGINAL indexing.  sel_mode
 * SC_ASSIGN_SEL_NONE or SC_ASSIGN_SEL_MASK (d_sel: n bytes).  pose_stride is a multiple of 4 and at least 48, at least 52 with
 * SC_MERGE_STATUS; 1 <= n_poses <= SC_MERGE_MAX_POSES.  The device form enqueues a fixed number of stream operations whatever n and
 * n_poses are — one memset (the tally words) and three launches: support, overlap, decide — reads no host word and returns without
 * waiting; the host form copies in, enqueues, copies out and waits.
 * The batch form, packed only.  The problems of sc_register_batch (offset a HOST array, params->layout, 3 <= n_b <= SC_BATCH_MAX_N);
 * the poses, the records and d_parent motion-major as sc_assign_poses_batch has them (pose k of problem b at (k * n_problems + b));
 * with SC_MERGE_COMPACT position p of problem b is record p * n_problems + b.  The status at byte 48 is always read (pose_stride at
 * least 52); 1 <= n_poses <= SC_MERGE_BATCH_MAX_POSES; sel_mode must be SC_ASSIGN_SEL_NONE.  A problem holding a non-finite
 * coordinate gets SC_EINVAL in every record (R = I, t = 0, index -1, 0, 0), parent -1 and the count words 0, 0; its neighbours are
 * untouched.  Like every batch entry it ends the frame a context may hold.  params is checked as sc_register_batch checks it; only
 * tau, score_mode and layout are read.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument
 * (a NULL ctx: no text; d_overlap and d_count may be NULL); mp->size wrong; a measure above 1; num or den outside 1 <= num <= den <=
 * 65536; sel_mode above 1 (batch: not 0); d_sel NULL with SC_ASSIGN_SEL_MASK; an unknown flag or a non-zero reserved word; n_poses 0
 * or above the form's maximum; a pose_stride that breaks the rule; no frame on the context (sc_peel's refusal, with its text); a
 * call outstanding on the context; the batch form's offsets and params as sc_assign_poses_batch refuses them.  A refused call leaves
 * the frame.
 * Workspace: the frame form keeps the support sets as bit rows, n_poses x ceil(n / 64) uint64, the tally words, and the overlap table
 * where the caller passes none; the batch form the copy of the offsets; the host forms device copies of their arrays, in the pool every host form shares
 * (sc_register_batch).  Everything is
 * allocated by the first such call, counted in workspace_bytes and held against the cap (SC_ENOMEM, nothing enqueued, the frame
 * stays).  A context that never calls these entries allocates and runs nothing new.
 * The loop this closes, every step stream-ordered and none read back: sc_register_instances -> sc_polish_poses_device(SEL_ALIVE) ->
 * sc_merge_poses_frame_device -> sc_settle_poses_frame_device(stride 64, SC_SETTLE_STATUS) -> sc_pose_info_frame_device(SEL_LABEL)
 * (INTEGRATION.md).
 * Not here: a refit of the kept poses (sc_settle_poses and sc_polish_poses do it); a relabelled label output (sc_assign_poses and
 * sc_settle_poses write it); merging by pose distance (angle, translation) rather than by support; slots and pairs forms; a form for
 * sharded frames, which leave no frame. */
#define SC_MERGE_MAX_POSES       1024u  /* frame form */
#define SC_MERGE_BATCH_MAX_POSES 64u    /* batch form */
#define SC_MERGE_OVER_MIN   0u          /* measure: the intersection over the smaller support */
#define SC_MERGE_OVER_UNION 1u          /* measure: the intersection over the union (Jaccard) */
#define SC_MERGE_STATUS  1u             /* flags: a pose record holds an int32 status at byte 48 */
#define SC_MERGE_COMPACT 2u             /* flags: the kept records first, then the others, each in ascending k */
typedef struct sc_merge_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_merge_params)                       */
  uint32_t measure;      /* SC_MERGE_OVER_MIN / _OVER_UNION                 */
  uint32_t num;          /* the fraction num / den: 1 <= num <= den         */
  uint32_t den;          /* ... <= 65536                                    */
  uint32_t min_count;    /* a valid pose with fewer inliers is dropped      */
  uint32_t sel_mode;     /* SC_ASSIGN_SEL_NONE / _MASK; batch: _NONE        */
  uint32_t flags;        /* SC_MERGE_STATUS, SC_MERGE_COMPACT or 0          */
  uint32_t reserved[1];  /* must be 0                                       */
} sc_merge_params;
typedef struct sc_merge_pose {     /* 64 bytes: a pose record, status at byte 48 */
  float    Rt[12];       /* kept: the input's bits; else R = I, t = 0        */
  int32_t  status;       /* SC_OK (kept), SC_ENOHYP (folded, dropped), or the invalid pose's status */
  int32_t  index;        /* kept: k; folded: its parent; else -1             */
  uint32_t count;        /* c_k (an invalid pose: 0)                         */
  uint32_t score;        /* s_k (an invalid pose: 0)                         */
} sc_merge_pose;
int sc_merge_default_params(sc_merge_params* mp);   /* size set, SC_MERGE_OVER_MIN, 1 / 2, everything else 0 */
/* d_pose: n_poses records of pose_stride bytes; d_sel per sel_mode (NULL with SEL_NONE); d_out: n_poses records; d_parent: n_poses
 * int32; d_overlap: n_poses x n_poses uint32 or NULL; d_count: 2 words or NULL */
int sc_merge_poses_frame_device(sc_ctx* ctx, const sc_merge_params* mp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                const uint8_t* d_sel, sc_merge_pose* d_out, int32_t* d_parent, uint32_t* d_overlap, uint32_t* d_count);
/* the same with host arrays (pose, sel, out, parent, overlap, count); waits */
int sc_merge_poses_frame(sc_ctx* ctx, const sc_merge_params* mp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                         const uint8_t* sel, sc_merge_pose* out, int32_t* parent, uint32_t* overlap, uint32_t* count);
/* every buffer but offset in HBM: d_src / d_tgt total x 3 floats, d_pose n_poses x n_problems records of pose_stride bytes
 * (motion-major), d_out n_poses x n_problems records (motion-major), d_parent n_poses x n_problems int32 (motion-major), d_count
 * 2 x n_problems words or NULL */
int sc_merge_poses_batch_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                const sc_params* params, const sc_merge_params* mp, const void* d_pose, uint32_t pose_stride,
                                uint32_t n_poses, sc_merge_pose* d_out, int32_t* d_parent, uint32_t* d_count);
/* the same with host arrays; waits */
int sc_merge_poses_batch(sc_ctx* ctx, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                         const sc_params* params, const sc_merge_params* mp, const void* pose, uint32_t pose_stride,
                         uint32_t n_poses, sc_merge_pose* out, int32_t* parent, uint32_t* count);

/* ---- absolute poses of a pair list's sets: sc_pairs_sync ----------------------------------------------------------------
 * The pairs chain leaves a relative pose per listed pair and, behind sc_pairs_cycles, a verdict on which pairs close consistent
 * loops.  What its caller — fragment registration, loop closure, multi-scan alignment — wants next is where the sets lie in ONE
 * frame.  These entries place every set that the list connects to an anchor set, on the device, stream-ordered behind
 * sc_pairs_cycles_device with no host word in between: the poses they leave are priors for sc_match_guided* as they stand
 * (where every component fits fp32: "Outputs" below).
 *
 * The method is anchored Jacobi averaging: breadth-first propagation and refinement in one rule.  X_s maps set s's coordinates
 * into the anchor's frame; pair p, stored (a, b) with pose T (a onto b), is the constraint X_a = X_b o T.  known_0 = {anchor},
 * X_0(anchor) = identity.  Round k recomputes every other set from the neighbours that were known after round k-1: the rotation
 * nearest the weighted sum of the predicted rotations (the chordal mean), the weighted mean of the predicted translations.  A round
 * reads X_{k-1} and writes every set of X_k (Jacobi, not Gauss-Seidel: nothing depends on scheduling), so a set first becomes known
 * in the round equal to its hop distance from the anchor.
 * The method's limits.  It is the synchronisation step a pose-graph solver is started from, and on well-connected lists also the
 * answer: 24 sets with all pairs stop in 4 - 5 rounds, 512 sets with 20 pairs a set in 9 - 14.  Along chains it DIFFUSES: a bare
 * ring of 40 sets needs 89 rounds at a tolerance of 1e-4 and 461 at 1e-6, an odometry strip of 200 sets with 40 closures 47 and 938
 * — more than max_rounds admits.  And "no set moved more than the tolerances in a round" is a STOPPING RULE, not an accuracy bound:
 * a slow mode moves every set by less than the tolerance a round, for many rounds.  Threshold the residuals (r2, e2 below) to judge
 * the result.
 *
 * Inputs.  n_sets, pairs (HOST), n_pairs, d_pose, pose_stride: exactly those of sc_pairs_cycles, under the same rules and limits
 * (SC_CYCLES_MAX_PAIRS, SC_CYCLES_MAX_DEGREE; SC_SYNC_STATUS for SC_CYCLES_STATUS).  d_use: NULL (every pair may be used) or a
 * uint32 read at byte p * use_stride, non-zero: pair p may be used; use_stride a multiple of 4, at least 4, ignored with NULL.
 * &d_res[0].alive of sc_pairs_cycles_device's records with use_stride 48 is the chain.  d_weight: NULL (every weight 1.0) or
 * n_pairs floats, widened to double; a pair whose weight is not finite or not greater than 0 is not used.  Nothing of the inputs is
 * written.
 * Thresholds, derived on the host in double: r2_max = 2.0 * (double)rot_tol * (double)rot_tol, e2_max = (double)trans_tol *
 * (double)trans_tol.  sc_sync_thresholds returns exactly the two values a call uses.  r2_max bounds the squared Frobenius distance
 * of two rotations, 2 theta^2 to first order; it is deliberately not a trace: 1 + 2 cos(rot_tol) is exactly 3.0 below 2e-8, and the
 * rounds would never stop.
 *
 * Definitions.  The call is a function of the list, the poses, use, weight and the parameters alone, bit for bit.  All arithmetic is
 * fp64 on the exactly widened fp32 entries; every operation is a plain rounded product, sum, quotient or square root in the order
 * written; nothing is fused.  valid(p), T(x->y) and M = B o A are those of sc_pairs_cycles.
 *   usable(p)  valid(p), pairs[2p] != pairs[2p + 1], use(p) != 0 (or d_use NULL), and w_p = (double)weight[p] (or 1.0) finite and
 *              > 0.
 *   sorted list  of set s: one entry for every listed pair that names s and another set n, in ascending order of (n, p).
 *   update     of set s != anchor in round k.  Its entries are taken in the order of its sorted list, i = 0, 1, ...  Entry i, on
 *              pair p to neighbour n, is LIVE if usable(p) and n is in known_{k-1}; then P = X_{k-1}(n) o T_p(s->n).  64 slots of
 *              13 doubles (acc[0 .. 11], accW), each +0.0.  Entry i adds into slot i mod 64, in increasing i:
 *              acc[c] = acc[c] + w_p * P[c] for the 12 components (P.R row-major, then P.t), accW = accW + w_p; an entry that is not
 *              live adds nothing.  The slots are folded: for h = 32, 16, 8, 4, 2, 1: slot[j] = slot[j] + slot[j + h] for j < h, every
 *              component.  With no live entry the set is unchanged.  Otherwise, from slot 0: M = acc[0 .. 8], c = acc[9 .. 11],
 *              W = accW; R' = rot(M), t'_i = c_i / W.  If any of the twelve is not finite (NaN or infinite) the set is unchanged —
 *              not known if it was not — and its `degenerate` grows by one.  Otherwise X_k(s) = (R', t') and s is in known_k.  The
 *              anchor is never recomputed.
 *   rot(M)     B_c = row c of M (c = 0, 1, 2), V_c = row c of the identity; dot(a, b) = (a_0 * b_0 + a_1 * b_1) + a_2 * b_2.
 *              Ten sweeps; a sweep takes (p, q) = (0, 1), (0, 2), (1, 2) in this order: alpha = dot(B_p, B_p), beta = dot(B_q, B_q),
 *              gamma = dot(B_p, B_q); if gamma != 0.0: zeta = (beta - alpha) / (gamma + gamma),
 *              tt = 1.0 / (|zeta| + sqrt(zeta * zeta + 1.0)), negated if zeta < 0.0, cs = 1.0 / sqrt(tt * tt + 1.0), sn = cs * tt;
 *              then for r = 0, 1, 2, with x = B_p[r], y = B_q[r]: B_p[r] = cs * x - sn * y, B_q[r] = sn * x + cs * y, and the same
 *              for V_p[r], V_q[r].  Then n_c = dot(B_c, B_c); i1 = the first c with the largest n_c (1 replaces 0 only if
 *              n_1 > n_0, 2 replaces that only if n_2 is greater still); i2 = the lower of the two other indices unless the
 *              higher one's n is greater.  s1 = sqrt(dot(B_i1, B_i1)), s2 = sqrt(dot(B_i2, B_i2)); u1 = B_i1 / s1, u2 = B_i2 / s2
 *              (component by component), v1 = V_i1, v2 = V_i2; u3 = u1 x u2, v3 = v1 x v2, with
 *              (a x b)_0 = a_1 * b_2 - a_2 * b_1, (a x b)_1 = a_2 * b_0 - a_0 * b_2, (a x b)_2 = a_0 * b_1 - a_1 * b_0;
 *              R'_rc = (v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c].  (The fp64 solve of the library's rigid refit applied to
 *              H = M^T, every fused multiply-add of it replaced by the rounded product followed by the rounded sum in the same
 *              nesting: the rotation nearest M in the Frobenius norm, a proper one whatever M's determinant.)
 *   changed    dR2 = the sum over the nine entries, row-major, of (R'_ij - R_ij) * (R'_ij - R_ij), added left to right; dt2
 *              likewise over the three of t.  Set s is changed in round k if it is in known_k and not in known_{k-1}, or
 *              dR2 > r2_max, or dt2 > e2_max: both cuts inclusive on the quiet side.
 *   rounds     K is the first round in which no set is changed (converged = 1), or max_rounds.  The outputs are X_K and known_K.
 *   residual   of pair p stored (a, b), when usable(p) and a and b are both in known_K: Q = X_K(b) o T_p(a->b) — the record
 *              itself —, r2 = the sum over the nine entries, row-major, of (X_K(a).R_ij - Q.R_ij) squared, added left to right,
 *              e2 = likewise over the three of t.
 * Outputs.  sc_sync_set (160 bytes) per set at d_set[s]: Rt is X_K(s) rounded once to fp32 and status SC_OK, so that d_set has the
 * layout of an array of pose records, with a status, of stride 160 for every pose entry — sc_pairs_sync itself among them; a set
 * that was never reached has Rt and X all zero and status SC_ENOHYP.  The rounding is the only one: a component of X_K whose
 * magnitude exceeds FLT_MAX becomes +-inf in Rt.  That can happen with finite inputs — translations add along a path, and records
 * that are no rotations multiply them: entries near FLT_MAX reach |X_K.t| of 1e76 within a few hops.  The status stays SC_OK and X
 * holds the finite value; every pose entry treats such a record as it treats any record that is not finite (fed back to
 * sc_pairs_sync: SC_EINVAL for that pair).  A caller that feeds d_set on looks at X, or lets the next entry's status say so.
 * sc_sync_pair (32 bytes) per pair at d_pair[p].  sc_sync_summary (32 bytes) at d_sum.
 * Forms.  sc_pairs_sync_device: poses, use, weight and outputs in HBM; it enqueues and returns without waiting, reads no host
 * word, and its number of stream operations depends on max_rounds only (a copy, a memset, max_rounds + 2 launches; a round's launch
 * returns at once when the round before changed no set).  (It may wait for the previous batch call's copy out of the staging area
 * the batch entries share.)  sc_pairs_sync: host arrays; waits.  Like every batch entry they end the frame a context may hold.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument
 * other than d_use and d_weight (a NULL ctx: no text); everything sc_pairs_cycles refuses of n_sets, n_pairs and the list; size
 * wrong, max_rounds outside 1 .. 256, rot_tol not finite or outside [0, pi], trans_tol not finite or negative, an unknown flag or a
 * non-zero reserved word; a pose_stride that breaks the pose rule; with d_use, a use_stride below 4 or no multiple of 4; an anchor
 * >= n_sets; a call outstanding on the context.
 * Workspace: the copied list with every set's sorted neighbour entries and the list starts, the oriented fp64 poses and a weight
 * (200 bytes a pair), two states and the tallies of a set (224 bytes a set) and the round words; the host form adds device copies
 * of its arrays, in the pool every host form shares.  Allocated by the first such call, counted in workspace_bytes and held against
 * the cap (SC_ENOMEM, nothing enqueued).  A context that never calls these entries allocates and runs nothing new.
 * Not here: a block solver — Gauss-Newton on the pairs' 6 x 6 information matrices, conjugate gradients on the graph Laplacian —
 * is sc_pairs_solve (below), which takes this entry's d_set as its start and is the answer where lists are chains: this entry
 * diffuses along them, as said above.  Not built: robust re-weighting between the rounds; several anchors; a sharded form. */
#define SC_SYNC_STATUS 1u   /* flags: a pose record holds an int32 status at byte 48 */
typedef struct sc_sync_params {    /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_sync_params)                                   */
  uint32_t anchor;       /* the set whose frame is the common one; < n_sets; default 0 */
  uint32_t max_rounds;   /* 1 .. 256; default 32                                       */
  uint32_t flags;        /* SC_SYNC_STATUS or 0                                        */
  float    rot_tol;      /* radians, finite, in [0, pi]                                */
  float    trans_tol;    /* finite, >= 0, in the poses' unit                           */
  uint32_t reserved[2];  /* must be 0                                                  */
} sc_sync_params;
typedef struct sc_sync_set {       /* 160 bytes */
  float    Rt[12];         /* X_K(s) rounded once: R row-major, then t; all 0 where s was never reached */
  int32_t  status;         /* SC_OK; SC_ENOHYP: never reached                                           */
  uint32_t known_round;    /* the k at which s became known; 0 for the anchor and for a set never reached */
  uint32_t used;           /* live entries of s in round K; 0 for the anchor                            */
  uint32_t degenerate;     /* rounds among 1 .. K in which s's sum gave no finite pose                   */
  double   X[12];          /* X_K(s); all 0 where s was never reached                                   */
} sc_sync_set;
typedef struct sc_sync_pair {      /* 32 bytes */
  int32_t  status;         /* SC_OK, the status passed through, or SC_EINVAL for a non-finite Rt        */
  uint32_t used;           /* 1: usable(p) and both of its sets are in known_K                          */
  double   r2;             /* the residual's rotation part; 0.0 where used is 0                         */
  double   e2;             /* the residual's translation part; 0.0 where used is 0                      */
  uint32_t reserved[2];    /* written as 0                                                              */
} sc_sync_pair;
typedef struct sc_sync_summary {   /* 32 bytes */
  uint32_t rounds;         /* K                                                        */
  uint32_t converged;      /* 1: no set changed in round K                             */
  uint32_t known;          /* sets in known_K, the anchor among them                   */
  uint32_t used;           /* pairs whose `used` is 1                                  */
  uint32_t changed_last;   /* sets changed in round K                                  */
  uint32_t reserved[3];    /* written as 0                                             */
} sc_sync_summary;
int sc_sync_default_params(sc_sync_params* sp);   /* size, anchor 0, max_rounds 32; everything else 0: the tolerances are the caller's */
/* host only, no context: out[0] = r2_max, out[1] = e2_max; SC_EINVAL for a NULL argument, a wrong size or a tolerance out of range */
int sc_sync_thresholds(const sc_sync_params* sp, double out[2]);
/* pairs a HOST array; d_pose n_pairs records of pose_stride bytes, d_use NULL or a word every use_stride bytes, d_weight NULL or
 * n_pairs floats, d_set n_sets records, d_pair n_pairs records, d_sum one */
int sc_pairs_sync_device(sc_ctx* ctx, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp,
                         const void* d_pose, uint32_t pose_stride, const void* d_use, uint32_t use_stride, const float* d_weight,
                         sc_sync_set* d_set, sc_sync_pair* d_pair, sc_sync_summary* d_sum);
/* the same with host arrays (pose, use, weight, set, pair, sum); waits */
int sc_pairs_sync(sc_ctx* ctx, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp,
                  const void* pose, uint32_t pose_stride, const void* use, uint32_t use_stride, const float* weight,
                  sc_sync_set* set, sc_sync_pair* pair, sc_sync_summary* sum);

/* ---- Gauss-Newton pose-graph solve of a pair list's sets: sc_pairs_solve --------------------------------------------------
 * sc_pairs_sync places the sets, and diffuses along chains; sc_pose_info_* leaves a 6 x 6 information matrix per pair that weighs
 * its pose.  These entries take both: from a start X_0 (sc_pairs_sync's d_set as it stands, or an earlier call's own d_set) they
 * minimise the sum over the usable pairs of xi_p^T info_p xi_p, xi_p the six-vector by which the pair's two sets miss its pose, by
 * Gauss-Newton steps whose linear systems are solved by block-Jacobi preconditioned conjugate gradients, all of it on the device,
 * stream-ordered behind sc_pairs_sync_device with no host word in between.
 * The method's limits.  No damping and no line search: a step that raises the cost is undone and ends the call (SC_SOLVE_STOP_ROSE),
 * so the start has to lie in the basin that sc_pairs_sync's result lies in.  The stopping rule is sc_pairs_sync's — no set moved
 * by more than the tolerances in a step — and here a step is a Newton step, not a diffusion round.  Measured on the reference
 * (tests/solve_ref.py), noise 0.01 rad / 0.02 units, info from 100 points a pair, tolerances 1e-6, cg_tol 1e-3: the bare ring of 40
 * sets, which sc_pairs_sync leaves unconverged after 256 rounds at 1e-6, stops CONVERGED from that result after 5 steps of 64 inner
 * iterations, cost 0.02326 -> 0.010395 (a dense solver's optimum: 0.010395); the odometry strip of 200 sets with 40 closures, which
 * sc_pairs_sync leaves unconverged likewise, keeps 4 steps of 64 at the defaults, cost 0.7261 -> 0.410234, and the fifth rises in
 * the last digits (ROSE); at max_inner 256 it stops CONVERGED after 4 steps and 510 iterations (dense optimum 0.410230: Gauss-Newton
 * drops a second-order term, and its fixed point is a relative 1e-5 above).  On chains the inner solve is the slow part: block
 * Jacobi does not shorten a chain, every step of the ring runs to max_inner.  A component of known
 * sets that no usable path joins to the anchor is legal and deterministic, and solved only up to its own gauge: its sets move
 * together by whatever rigid motion conjugate gradients from zero leave in the singular system.
 *
 * Inputs.  n_sets, pairs (HOST), n_pairs, d_pose, pose_stride, d_use, use_stride: exactly those of sc_pairs_sync, under the same
 * rules and limits (SC_CYCLES_MAX_PAIRS, SC_CYCLES_MAX_DEGREE; SC_SOLVE_STATUS for SC_SYNC_STATUS).  d_info: NULL (every matrix
 * the 6 x 6 identity) or n_pairs records of info_stride bytes: double info[36] at byte 0, row-major, order and meaning those of
 * sc_pose_info_result; with SC_SOLVE_INFO_STATUS an int32 status at byte 296.  info_stride is a multiple of 8 and at least 288
 * (300 with the flag): an array of sc_pose_info_result fits as it stands, stride 320.  d_init: n_sets records of init_stride
 * bytes, a multiple of 8 and at least 160: an int32 status at byte 48 and double X[12] at byte 64 — sc_sync_set and sc_solve_set
 * are such records.  A NULL d_info and an array of identity records give the same bytes.  Nothing of the inputs is written; d_set
 * may be d_init.
 * Thresholds, derived on the host in double: r2_max and e2_max exactly as sc_sync_thresholds derives them from rot_tol and
 * trans_tol, and cg2 = (double)cg_tol * (double)cg_tol.  sc_solve_thresholds returns exactly the three values a call uses.
 *
 * Definitions.  The call is a function of the list, the poses, use, info, init and the parameters alone, bit for bit.  All
 * arithmetic is fp64; every operation is a plain rounded product, sum, difference, quotient or square root in the order written;
 * nothing is fused; no sine, cosine or other library function appears.  "sum_k a_k, left to right" is ((a_0 + a_1) + a_2) + ...,
 * the first term taken as it is.  valid(p), T(x->y), the inverse and M = B o A are those of sc_pairs_cycles; rot(M), the sorted
 * list of a set, and "64 slots, folded" are those of sc_pairs_sync.
 *   known(s)   init status(s) == SC_OK and the twelve of init X(s) finite.  X_0(s) = init X(s), bit for bit, for every s.
 *   usable(p)  valid(p), pairs[2p] != pairs[2p + 1], use(p) != 0 (or d_use NULL), the 36 of info_p finite and its status SC_OK (or no
 *              flag; d_info NULL: info_p = the identity, 1.0 and +0.0), and both of its sets known.
 *   state(s)   SC_SOLVE_UNKNOWN if not known(s); else SC_SOLVE_ANCHOR if s == anchor; else SC_SOLVE_ISOLATED if no usable pair
 *              names s; else SC_SOLVE_FREE.  Only free sets ever move; every other set keeps X_0(s).
 *   error      of usable pair p stored (a, b) at state X: Xi = the inverse of X(b), D = Xi o X(a), E = D o T_p(b->a) (the inverse of
 *              the record, as sc_pairs_cycles orients it).  xi = (omega, v): omega_0 = (E.R_21 - E.R_12) / 2.0,
 *              omega_1 = (E.R_02 - E.R_20) / 2.0, omega_2 = (E.R_10 - E.R_01) / 2.0, v = E.t.  y_i = sum_j info[6 i + j] * xi_j,
 *              j = 0 .. 5 left to right; cost_p = sum_i xi_i * y_i, left to right; w2 = sum_i omega_i * omega_i,
 *              v2 = sum_i v_i * v_i, left to right.  A pair that is not usable has cost_p = w2 = v2 = +0.0.
 *   cost       of a state: chunks of 64 consecutive pairs (the last one shorter), each summed from +0.0 in increasing p,
 *              s = s + cost_p; then the chunk sums summed from +0.0 in increasing order.
 *   linearised under X'(s) = exp(delta_s) o X(s), the perturbation on the left, in the common frame, rotation first: with R, t of
 *              X(b), A is the 6 x 6 matrix Ad(X(b)^-1): A[i][j] = A[3 + i][3 + j] = R_ji, A[i][3 + j] = +0.0,
 *              A[3 + i][j] = -(c x t)_j with c = column i of R = (R_0i, R_1i, R_2i) and x sc_pairs_sync's cross product
 *              (i, j = 0 .. 2).  M[i][j] = sum_k info[6 i + k] * A[k][j]; W[i][j] = W[j][i] = sum_k A[k][i] * M[k][j] for i <= j;
 *              g_i = sum_k A[k][i] * y_k; every k = 0 .. 5 left to right, the zeros of A multiplied like any entry.  The dependence
 *              of xi's Jacobian on xi is dropped (Gauss-Newton).  The normal matrix is the graph Laplacian with the blocks W_p:
 *              H_aa += W_p, H_bb += W_p, H_ab = H_ba = -W_p; the right-hand side is -g, g_a += g_p, g_b -= g_p.
 *   row sums   of a free set s over its sorted list: entry i, on pair p to neighbour n, is LIVE if usable(p).  64 slots, each
 *              component +0.0; a live entry i adds into slot i mod 64 in increasing i, the slots are folded h = 32 .. 1, the sum
 *              is slot 0.  G(s): acc_c = acc_c + g_p[c] where s is the pair's stored first set, acc_c = acc_c - g_p[c] where it
 *              is the second.  Hd(s): acc_c = acc_c + W_p[c] for the 21 c with row <= column.  (H d)(s) for a vector d with a
 *              six-vector per set: e_j = d(s)_j - d(n)_j, u_c = sum_j W_p[c][j] * e_j left to right, acc_c = acc_c + u_c.
 *   factor     of Hd(s), H_ij = H_ji its entries, once per step: for j = 0 .. 5: u_k = L_jk * D_k (k < j); a = H_jj, then
 *              a = a - L_jk * u_k for k = 0 .. j-1; D_j = a; for i = j+1 .. 5: a = H_ij, then a = a - L_ik * u_k for
 *              k = 0 .. j-1; L_ij = a / D_j.  If any D_j is not > 0.0 or not finite, s is HELD for this step: it does not
 *              move, and its `degenerate` grows by one.  ACTIVE = free and not held.
 *   solve      z = Hd(s)^-1 r of an active s: y_i = r_i, then y_i = y_i - L_ik * y_k for k = 0 .. i-1 (i = 0 .. 5);
 *              w_i = y_i / D_i; for i = 5 .. 0: z_i = w_i, then z_i = z_i - L_ki * z_k for k = i+1 .. 5.  z = 0 where s is not
 *              active.
 *   grand sum  of a value per set (a.b = sum_c a_c * b_c, c = 0 .. 5 left to right, for an active set; +0.0 for every other):
 *              chunks of 64 consecutive sets, each summed from +0.0 in increasing s, then the chunk sums summed from +0.0 in
 *              increasing order.
 *   inner      the solve of step j, preconditioned conjugate gradients on the active sets (d = 0 elsewhere): x = 0, r = -G,
 *              z = solve(r), rz_0 = grand sum of r.z.  If rz_0 == 0.0 the solve ends with no iteration.  Iteration
 *              i = 1 .. max_inner: p = z if i == 1, else beta = rz_{i-1} / rz_{i-2}, p_c = z_c + beta * p_c; q = (H p); pq = grand
 *              sum of p.q; if pq is not > 0.0 or not finite the solve ends and this iteration is not applied.  alpha =
 *              rz_{i-1} / pq; x_c = x_c + alpha * p_c; r_c = r_c - alpha * q_c; z = solve(r); rz_i = grand sum of r.z; the solve
 *              ends if rz_i <= cg2 * rz_0, or at i == max_inner.  inner_j = the iterations applied.
 *   step       of an active set with x = (omega, v): Q = rot(I + [omega]x), the matrix rows (1.0, -omega_2, omega_1),
 *              (omega_2, 1.0, -omega_0), (-omega_1, omega_0, 1.0); R' = rot(Q R), Q R by the composition's rule; t'_i =
 *              ((Q_i0 * t_0 + Q_i1 * t_1) + Q_i2 * t_2) + v_i.  If any of the twelve is not finite the set is unchanged and its
 *              `degenerate` grows by one: no NaN is ever written into X.  A set is CHANGED in step j if it was stepped and
 *              dR2 > r2_max or dt2 > e2_max, dR2 and dt2 sc_pairs_sync's between X_j(s) and X_{j-1}(s).
 *   outer      c_0 = cost(X_0).  If no set is free: K = 0, SC_SOLVE_STOP_CONVERGED.  Step j = 1 .. max_outer: linearise at
 *              X_{j-1}, factor, inner solve, step, c_j = cost(X_j).  If !(c_j <= c_{j-1}) — a cost that is not finite
 *              included — the step is undone: K = j - 1, SC_SOLVE_STOP_ROSE.  Otherwise, if no set changed in step j or rz_0 was
 *              0.0: K = j, SC_SOLVE_STOP_CONVERGED; otherwise at j == max_outer: K = j, SC_SOLVE_STOP_MAX_OUTER.  J = the last
 *              step taken (K, or K + 1 after ROSE).  The outputs are X_K and the pairs' errors at X_K.
 * Outputs.  sc_solve_set (160 bytes, the layout of sc_sync_set) per set at d_set[s]: Rt is X_K(s) rounded once to fp32 (sc_pairs_sync's
 * remark on components past FLT_MAX holds), status the init status passed through, X = X_K(s); an unknown set's X is its init X.
 * sc_solve_pair (48 bytes) per pair at d_pair[p], sc_solve_summary (64 bytes) at d_sum.
 * Forms.  sc_pairs_solve_device: everything but pairs in HBM; it enqueues and returns without waiting, reads no host word, and the
 * number of its stream operations depends on max_outer and max_inner only: a copy, a memset and
 * 5 + max_outer * (4 + 2 * max_inner) launches (prepare, sets, linearise, decide; per step: factor, two per inner iteration —
 * the product, which forms p on the fly, and the update —, step, linearise, decide; finish).  Every stop is the device's: a
 * launch whose work is over returns at once on a word an earlier launch left.  A call with max_outer * max_inner > 2048 is
 * refused.  sc_pairs_solve: host arrays; waits.  Like every batch entry they end the frame a context may hold.
 * Errors: the CALL returns SC_EINVAL, decided on the host before anything is enqueued, sc_last_error naming which: a NULL argument
 * other than d_use and d_info (a NULL ctx: no text); everything sc_pairs_sync refuses of n_sets, n_pairs, the list, pose_stride and
 * use_stride; size wrong, max_outer outside 1 .. 32, max_inner outside 1 .. 256, their product above 2048, rot_tol or trans_tol
 * as sc_pairs_sync refuses them, cg_tol not finite or outside [0, 1), an unknown flag; with d_info, an info_stride that breaks the
 * rule above; an init_stride that does; an anchor >= n_sets; a call outstanding on the context.
 * Workspace: the copied list as sc_pairs_sync stages it, 584 bytes a pair (the oriented poses, W_p, g_p, the errors of two states),
 * 664 bytes a set (two states, the vectors of the inner solve with p twice, the factor, the tallies), the chunk sums and the
 * control words.  Allocated by the first such call, counted in workspace_bytes and held against the cap (SC_ENOMEM, nothing
 * enqueued); the host form adds device copies of its arrays, in the pool every host form shares.  A context that never calls
 * these entries allocates and runs nothing new.
 * Not here / not built: Levenberg-Marquardt damping; robust re-weighting or line processes; the exact point cost from the moments
 * sc_pose_info sums; a one-workgroup form for small graphs (a small list pays the launches: see DESIGN); several anchors; a
 * sharded form.  The ends of the fp32 range are the next, test-only change; the finite guards above are built and stated now. */
#define SC_SOLVE_STATUS 1u       /* flags: a pose record holds an int32 status at byte 48 */
#define SC_SOLVE_INFO_STATUS 2u  /* flags: an info record holds an int32 status at byte 296 */
#define SC_SOLVE_FREE 0u
#define SC_SOLVE_ANCHOR 1u
#define SC_SOLVE_UNKNOWN 2u
#define SC_SOLVE_ISOLATED 3u
#define SC_SOLVE_STOP_CONVERGED 1u
#define SC_SOLVE_STOP_ROSE 2u
#define SC_SOLVE_STOP_MAX_OUTER 3u
typedef struct sc_solve_params {   /* 32 bytes */
  uint32_t size;         /* = sizeof(sc_solve_params)                                  */
  uint32_t anchor;       /* the set that keeps its X; < n_sets; default 0              */
  uint32_t max_outer;    /* Gauss-Newton steps at most, 1 .. 32; default 8             */
  uint32_t max_inner;    /* iterations of a step's solve at most, 1 .. 256; default 64 */
  uint32_t flags;        /* SC_SOLVE_STATUS | SC_SOLVE_INFO_STATUS, or 0               */
  float    rot_tol;      /* radians, finite, in [0, pi]                                */
  float    trans_tol;    /* finite, >= 0, in the poses' unit                           */
  float    cg_tol;       /* finite, in [0, 1)                                          */
} sc_solve_params;
typedef struct sc_solve_set {      /* 160 bytes */
  float    Rt[12];         /* X_K(s) rounded once: R row-major, then t                                  */
  int32_t  status;         /* the init status, passed through                                           */
  uint32_t state;          /* SC_SOLVE_FREE / ANCHOR / UNKNOWN / ISOLATED                               */
  uint32_t degenerate;     /* steps among 1 .. J in which s was held, or stepped to no finite pose      */
  uint32_t reserved;       /* written as 0                                                              */
  double   X[12];          /* X_K(s)                                                                    */
} sc_solve_set;
typedef struct sc_solve_pair {     /* 48 bytes */
  int32_t  status;         /* SC_OK, the pose status passed through, or SC_EINVAL for a non-finite Rt   */
  uint32_t used;           /* 1: usable(p)                                                              */
  double   cost;           /* cost_p at X_K                                                             */
  double   w2;             /* omega.omega at X_K                                                        */
  double   v2;             /* v.v at X_K                                                                */
  uint32_t reserved[4];    /* written as 0                                                              */
} sc_solve_pair;
typedef struct sc_solve_summary {  /* 64 bytes */
  uint32_t outer;          /* K                                                        */
  uint32_t stop;           /* SC_SOLVE_STOP_*                                          */
  uint32_t inner_total;    /* inner_1 + ... + inner_J                                  */
  uint32_t inner_last;     /* inner_J; 0 where J is 0                                  */
  uint32_t free_sets;      /* sets whose state is SC_SOLVE_FREE                        */
  uint32_t used_pairs;     /* pairs whose `used` is 1                                  */
  uint32_t held_last;      /* sets held in step J                                      */
  uint32_t reserved;       /* written as 0                                             */
  double   cost0;          /* c_0                                                      */
  double   cost;           /* c_K                                                      */
  double   rz0;            /* rz_0 of step J; 0.0 where J is 0                         */
  double   reserved2;      /* written as 0.0                                           */
} sc_solve_summary;
int sc_solve_default_params(sc_solve_params* sp);   /* size, anchor 0, max_outer 8, max_inner 64; everything else 0: the tolerances are the caller's */
/* host only, no context: out[0] = r2_max, out[1] = e2_max, out[2] = cg2; SC_EINVAL for a NULL argument or parameters a call refuses
 * (the anchor apart) */
int sc_solve_thresholds(const sc_solve_params* sp, double out[3]);
/* pairs a HOST array; d_pose n_pairs records of pose_stride bytes, d_use NULL or a word every use_stride bytes, d_info NULL or
 * n_pairs records of info_stride bytes, d_init n_sets records of init_stride bytes, d_set n_sets records, d_pair n_pairs records,
 * d_sum one */
int sc_pairs_solve_device(sc_ctx* ctx, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp,
                          const void* d_pose, uint32_t pose_stride, const void* d_use, uint32_t use_stride,
                          const void* d_info, uint32_t info_stride, const void* d_init, uint32_t init_stride,
                          sc_solve_set* d_set, sc_solve_pair* d_pair, sc_solve_summary* d_sum);
/* the same with host arrays (pose, use, info, init, set, pair, sum); waits */
int sc_pairs_solve(sc_ctx* ctx, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp,
                   const void* pose, uint32_t pose_stride, const void* use, uint32_t use_stride,
                   const void* info, uint32_t info_stride, const void* init, uint32_t init_stride,
                   sc_solve_set* set, sc_solve_pair* pair, sc_solve_summary* sum);

/* ---- two-phase form for one-process-per-GPU sharding --------------------------------
 * Phase 1: A and B replicated, C1+C2 on this rank's blocks of the top-T list; writes this rank's winner key
 * PAIR to d_key (device, 2 x u64 = 16 bytes):
 *     d_key[0] = (inlier_count << 32) | ranking_key_of_the_triangle      (0 = no hypothesis with an inlier)
 *     d_key[1] = 0xFFFFFFFF - position of that triangle in the replicated top-T list, taking the LOWEST
 *                position among this rank's hypotheses that attain d_key[0]
 * The caller reduces over ranks in two steps (both 8-byte MAX all-reduces; RCCL through torch.distributed in
 * this repo's host layer, see sac-cot_amd/shard.py — any transport works):
 *     K0 = max_r d_key_r[0];   every rank whose own d_key[0] != K0 sets its d_key[1] = 0;   K1 = max_r d_key_r[1]
 * and stores (K0, K1) back into d_key.  The winner is thus: most inliers, then best ranking key, then lowest
 * (i,j,k) — "ties -> best-ranked triangle" of SURVEY §8a, decided without sorting the T hypotheses.
 * Phase 2: every rank decodes the same winner from the reduced pair, re-solves its (R,t) from its own
 * replicated list and builds the mask.  Returns SC_ENOHYP when d_key[0] is 0.
 * Synchronisation: sc_hypothesize_device returns with its last kernels still queued (d_key is valid in stream order:
 * enqueue the reduction on the same stream, or synchronise it).  sc_finalize_device returns once the winner is known
 * to the host (status, stats); on the context's private stream it also waits for d_Rt / d_mask, on a stream given
 * with sc_set_stream they are complete in THAT stream's order, like any other work the caller enqueues there. */
int sc_hypothesize_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, int64_t n,
                          const sc_params* params, uint64_t* d_key, sc_stats* stats);
int sc_finalize_device(sc_ctx* ctx, const uint64_t* d_key, float* d_Rt, uint8_t* d_mask, sc_stats* stats);

/* Phase 2 on the all-GATHERED key pairs: d_keys holds n_pairs pairs (rank r's pair at d_keys[2r], d_keys[2r+1]), e.g. the
 * output of ONE all-gather of the 16-byte pairs; the reduction described above (a lexicographic max) runs inside the
 * finalize kernel.  One collective per call instead of two dependent ones; sc_finalize_device is the n_pairs = 1 case. */
int sc_finalize_gathered_device(sc_ctx* ctx, const uint64_t* d_keys, int n_pairs, float* d_Rt, uint8_t* d_mask,
                                sc_stats* stats);
/* The same in two halves (0.7), for ranks that register a STREAM of frames: the finalize kernel is enqueued and the call returns;
 * sc_wait(ctx, stats) delivers what sc_finalize_gathered_device returns.  Between the two the rank's host thread is free — e.g. to
 * run sc_hypothesize_device, the exchange and this call for the job's NEXT frame on a second context bound to the same stream, so
 * that the GPU never waits for a winner's way to the host.  With SC_FLAG_EST_BOUND a sc_hypothesize_device call that repeats the
 * last call's shape on its context is itself enqueued without a host wait (as sc_register_device_async's calls are); its
 * validation happens in the finalize call / sc_wait, and a failed one is one more reason for SC_EBOUND — on every rank alike.
 * (The statistics sc_hypothesize_device itself returns are provisional for such a call — its counts are what the launches COVER;
 * the finalize call / sc_wait deliver the real ones.) */
int sc_finalize_gathered_device_async(sc_ctx* ctx, const uint64_t* d_keys, int n_pairs, float* d_Rt, uint8_t* d_mask);

/* Phase 1 in two halves, for large T_total over several GPUs: stage B's certificate (sc_tri_prune.hip 3b) samples ~5T/8
 * edges, which every rank would otherwise repeat (126 us at T_total = 400 k against 33 us at 50 k).  `begin` runs A,
 * the edge list and THIS rank's share of the sample (every shard_world-th sampled edge) into d_hist (device,
 * SC_HIST_WORDS x u32, zeroed here); the caller SUMS d_hist over the ranks (one 1 KiB all-reduce; any order: integer
 * sums) and passes the result to `end`, which prunes, enumerates, selects and scores exactly like
 * sc_hypothesize_device — the summed histogram counts distinct genuine triangles, so the bound it certifies is valid
 * and identical on every rank, and results equal the unsharded run's.  With shard_world == 1 the sum is the identity. */
#define SC_HIST_WORDS 256
int sc_hypothesize_begin_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, int64_t n,
                                const sc_params* params, uint32_t* d_hist, sc_stats* stats);
int sc_hypothesize_end_device(sc_ctx* ctx, const uint32_t* d_hist, uint64_t* d_key, sc_stats* stats);

/* ---- stages A and B sharded too: phase API, one context per GPU / rank ------------------
 * With the two-phase form above every rank repeats stages A and B.  Here rank r computes the row block
 * [r * rows_per_rank, ...) of the adjacency bit rows (and of S, kept local, unless SC_FLAG_NO_DENSE_S) and enumerates
 * the triangles of a contiguous, equally heavy range of rows; what the ranks exchange lives in CALLER buffers, and the
 * caller runs the collectives between the phases (RCCL through torch.distributed in this repo's host layer, RCCL
 * directly in sc_register_multi below; on one GPU the "ranks" of a test simply share the buffers):
 *     sc_shard_compat_device (d_bits_all)      -> all-gather, in place, of bits_bytes_per_rank per rank
 *     sc_shard_edges_device  (d_hist)          -> all-reduce SUM of SC_HIST_WORDS u32 (1 KiB)
 *     sc_shard_select_device (d_hist, d_mine)  -> all-gather of cand_bytes_per_rank per rank into d_cand_all
 *     sc_shard_score_device  (d_cand_all, d_key) -> all-gather of the 16-byte key pairs
 *     sc_finalize_gathered_device (d_keys, shard_world, ...)
 * d_bits_all: bits_bytes_total bytes; rank r's slice starts at r * bits_bytes_per_rank (its rows at their global
 * index).  A candidate blob holds a rank's own best triangles in (i,j,k) order — up to max(2T/world, 4096) <<
 * shard_cand_level of them, never more than T (a rank contributes ~T/world with equally heavy row ranges); the row
 * ranges ascend with the rank, so the concatenated blobs are in global (i,j,k) order and the merge is the same exact
 * select + compaction every rank runs on one GPU: winner, (R,t) and mask are bit-identical to the unsharded call.  If a
 * rank had to cut its list and the cut could have mattered, the finalize call returns SC_ERETRY on every rank.  Every rank must pass the
 * same n and parameters (shard_rank aside).  shard_world <= 64; shard_world == 1 works (no collective needed).
 * Each phase leaves its last kernels queued on the context's stream; enqueue the collective on the same stream. */
typedef struct sc_shard_plan {
  uint32_t size;                 /* = sizeof(sc_shard_plan), set by the caller                              */
  uint32_t rows_per_rank;        /* rows of the adjacency matrix rank r computes: [r * rows_per_rank, ...)   */
  uint32_t words_per_row;        /* u64 words per bit row                                                   */
  uint32_t reserved;
  uint64_t bits_bytes_per_rank;  /* rows_per_rank * words_per_row * 8                                       */
  uint64_t bits_bytes_total;     /* shard_world * bits_bytes_per_rank: size of d_bits_all                    */
  uint64_t cand_bytes_per_rank;  /* size of one candidate blob; d_cand_all holds shard_world of them         */
} sc_shard_plan;
int sc_shard_plan_query(const sc_params* params, int64_t n, sc_shard_plan* plan);
int sc_shard_compat_device(sc_ctx* ctx, const float* d_src, const float* d_tgt, int64_t n, const sc_params* params,
                           void* d_bits_all);
int sc_shard_edges_device(sc_ctx* ctx, uint32_t* d_hist);
int sc_shard_select_device(sc_ctx* ctx, const uint32_t* d_hist, void* d_cand_mine);
int sc_shard_score_device(sc_ctx* ctx, const void* d_cand_all, uint64_t* d_key, sc_stats* stats);

/* ---- native multi-device entry: one process, n_dev GPUs, RCCL inside the library ------------
 * For hosts without a collective layer of their own (C++, mex): host arrays in, (R, t, mask) out, like sc_register.
 * One context per device, stages A, B and C all sharded (the phase API above), the four collectives of a call issued
 * through RCCL on the devices' streams (all-gather of the bit rows, 1 KiB all-reduce, all-gather of the candidate
 * blobs, all-gather of the key pairs).  One worker thread per device drives its GPU (a call is ~35 launches and four
 * read-backs per device: from a single thread that is ~1 ms per step for eight GPUs); the calling convention stays
 * single-caller.  RCCL is opened at run time (librccl.so.1) only when n_dev > 1: n_dev == 1 is exactly sc_register
 * and makes no RCCL call.  device_ids must be distinct.  Results are bit-identical to sc_register for every n_dev.
 * params->shard_* must be left at no sharding (rank 0, world 1).  stats: rank 0's, with tri_scored and
 * workspace_bytes summed over the devices.  Errors: the first failing rank's status; sc_multi_last_error has its text.
 * sc_create_multi_loopback: n_ranks ranks on ONE device with device copies in place of RCCL — a test hook that runs
 * the whole orchestration on a one-GPU box; with n_ranks == 1 it runs the rank machinery over a real single-rank RCCL
 * communicator instead, which executes the RCCL calls themselves (N > 1 over RCCL is unmeasured on hardware: DESIGN.md §7). */
typedef struct sc_multi sc_multi;
int         sc_create_multi(const int* device_ids, int n_dev, sc_multi** out);
int         sc_create_multi_loopback(int device, int n_ranks, sc_multi** out);
void        sc_destroy_multi(sc_multi* m);
const char* sc_multi_last_error(const sc_multi* m);
int         sc_register_multi(sc_multi* m, const float* src, const float* tgt, int64_t n, const sc_params* params,
                              float R[9], float t[3], uint8_t* mask, sc_stats* stats);

/* ---- stage-level hooks (host pointers in and out) so every kernel is parity-testable alone --------
 * All take SoA or AoS input per params->layout and run ONLY the named stage(s) on the GPU. */

/* row A: S n x n fp32 row-major, bits n x ceil(n/64) u64 (bit j%64 of word j/64 of row i), deg n u32.
 * Any output pointer may be NULL. */
int sc_compat_host(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                   float* S, uint64_t* bits, uint32_t* deg);

/* rows A+B: ranked top-T triangles.  tri: T x 3 u32 (i<j<k, rank order), key: T u32 (fp32 bits of w for
 * SC_RANK_WEIGHT, the degree sum for SC_RANK_DEGREE), *t_eff = min(T, tri_total). */
int sc_triangles_host(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                      uint32_t* tri, uint32_t* key, uint32_t* t_eff, uint64_t* tri_total, uint64_t* edges);

/* row C1: Rt: T x 12 fp32 (R row-major, then t) for the given triangles. */
int sc_kabsch_host(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                   const uint32_t* tri, uint32_t n_tri, float* Rt);

/* row C2: inlier count of every hypothesis over all n correspondences, plus the arg-max key
 * (rank index = position in Rt).  cnt may be NULL. */
int sc_score_host(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                  const float* Rt, uint32_t n_hyp, uint32_t* cnt, uint64_t* key);

/* row C3: mask of one hypothesis. */
int sc_mask_host(sc_ctx* ctx, const float* src, const float* tgt, int64_t n, const sc_params* params,
                 const float Rt[12], uint8_t* mask);

#ifdef __cplusplus
}
#endif
#endif /* SACCOT_H */
