/* libpmce_hip.so — C ABI of the MI355X-native PMCE per-clip inference hot path.
 *
 * The reference (kasvii/PMCE) is pure Python/PyTorch and has no FFI; its boundary for this path is the
 * nn.Module API of lib/models (PMCE.py:15-26, PoseEstimation.py:95-120, CoevoDecoder.py:226-252) plus the
 * caller's J_regressor projection (lib/core/base.py:223-225).  The entry points below are what a binding of
 * that path needs; pmce_amd/_lib.py is the ctypes binding, pmce_amd/models/ the nn.Module-shaped host side,
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions (all functions):
 *   - return 0 on success, a negative PMCE_ERR_* otherwise; never throw, never exit; the message of the last
 *     error of the calling thread is pmce_last_error_string();
 *   - every pointer is a DEVICE pointer to contiguous row-major fp32 (int32 where noted), 16-byte aligned;
 *   - the caller owns every buffer: weights, activations, the workspace and - split_f16 mode - the arena that holds the f16
 *     planes of the large weights (pmce_model_split_bytes / pmce_model_set_split_arena).  What a model handle allocates for
 *     itself: 4 bytes of pinned host memory (the overflow word, pmce_model_overflowed), one internal HIP stream and a handful of
 *     events (two-stream execution inside a forward); and, ONLY when no arena was handed over, the planes by hipMalloc;
 *   - launches are asynchronous on the hipStream_t passed in.  The calls that synchronise: pmce_model_finalize[_on] and
 *     pmce_model_set_gemm_mode[_on] (they wait for their own packing kernels on the stream given; a mode change that drops
 *     existing planes first waits for the whole device - forwards in flight may read them - and is therefore not capturable),
 *     pmce_model_profile_read (waits for the recorded events);
 *   - mutable state outside the handles: the thread-local error string and, while a model entry point runs, the thread-local
 *     pointer to that model's overflow word - one process per GPU or several host threads with their own streams are both fine -
 *     and the process-wide TUNING AIDS pmce_gemm_set_tuning, pmce_gemm_split_set_tuning, pmce_gemm_set_max_workgroups (relaxed atomics
 *     read at launch time: meant for benchmarks and tests, not to be flipped while forwards are being enqueued elsewhere).
 * Fixed structural constants of the path: T = 16 frames, F = 2048 image-feature channels, V = 431 coarse
 * vertices, 6890 mesh vertices, D = 64 decoder channels, GRU hidden 1024, 8 lifter heads.  J <= 32,
 * C in {256, 512}.
 */
#ifndef PMCE_HIP_H
#define PMCE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* pmce_stream_t; /* == hipStream_t */

#define PMCE_OK 0
#define PMCE_ERR_ARG (-1)
#define PMCE_ERR_LAUNCH (-2)
#define PMCE_ERR_WORKSPACE (-3)
#define PMCE_ERR_OVERFLOW (-4) /* strict overflow policy only: an earlier call produced non-finite values (pmce_model_overflowed) */

int pmce_version(void);
/* identifies the sources the library was built from (16 hex digits; pmce_amd.build.source_id()): profiler summaries record it */
const char* pmce_build_id(void);
const char* pmce_last_error_string(void);

/* ---------------------------------------------------------------------------------------------------------
 * Whole-path model object (host-side descriptor only: it stores the pointers the caller registers).
 * Replaces: models.PMCE.get_model / PMCE.forward (PMCE.py:7-26), models.PoseEstimation.get_model /
 * GraphormerNet.forward (PoseEstimation.py:95-120), models.CoevoDecoder.get_model / Pose2Mesh.forward
 * (CoevoDecoder.py:226-252), and `J_regressor[None] @ (pred_mesh*1000)` (lib/core/base.py:223-225).
 * ------------------------------------------------------------------------------------------------------- */
typedef struct pmce_model pmce_model;

/* num_joint: J (17, or 19 for COCO-input checkpoints); embed_dim: C (a multiple of 128 from 128 to 512: 128|256|384|512); depth: lifter depth (3).
 * ENVIRONMENT: the library reads exactly five variables, all here, once per handle; each only sets the initial value of a setting that has an
 * API setter and a getter (tests/test_host_logic.py flips every one):
 *   PMCE_SPLIT_F16=0        initial gemm mode fp32 pipe           (pmce_model_set_gemm_mode / pmce_model_gemm_mode)
 *   PMCE_SPLIT_MIN_BATCH=n  calls below n clips stay on fp32 pipe (pmce_model_set_split_min_batch / _get_)
 *   PMCE_STRICT_OVERFLOW=1  strict overflow policy                (pmce_model_set_overflow_policy / _get_)
 *   PMCE_SINGLE_STREAM=1    no second stream inside a forward     (pmce_model_set_concurrency / _get_)
 *   PMCE_SPLIT_OVERLAP=0    diagnostic: the split mode strictly serial, one stream (pmce_model_get_split_overlap; Python's Pipeline reads it too)
 * (Rounds 2-4 carried 16 more A/B switches that kept superseded kernels reachable; round 5 removed them with those kernels.) */
int pmce_model_create(int num_joint, int embed_dim, int depth, pmce_model** out);
void pmce_model_destroy(pmce_model* m);
/* Register one packed tensor by name (names: pmce_model_tensor_name).  The pointer must stay valid. */
int pmce_model_set_tensor(pmce_model* m, const char* name, const void* dev_ptr);
/* Enumerate the packed-tensor names the model needs (i in [0, pmce_model_tensor_count)). */
int pmce_model_tensor_count(const pmce_model* m);
const char* pmce_model_tensor_name(const pmce_model* m, int i);
/* Optional caller-side projection (lib/core/base.py:196,225): register "jreg.indptr" (int32[R+1]), "jreg.indices"
 * (int32[nnz]), "jreg.data" (fp32[nnz]) with pmce_model_set_tensor and the row count R here. */
int pmce_model_set_regressor_rows(pmce_model* m, int rows);
/* Check that every tensor is registered and (split_f16 mode) pack the large weights as f16 planes (into the arena below, or memory of its own without one).
 * The packing kernels run on `stream` - pass the stream the registered tensors were produced on (they are read here) - and the
 * call returns when they are done (it synchronises that stream, nothing else).  pmce_model_finalize = ..._on(m, NULL): the null
 * stream, which is NOT ordered behind non-blocking streams (PyTorch's side streams). */
int pmce_model_finalize(pmce_model* m);
int pmce_model_finalize_on(pmce_model* m, pmce_stream_t stream);
/* The f16 planes (as many bytes again as the fp32 weights they mirror: 0.6 GB at C = 512) live in memory the CALLER provides:
 * pmce_model_split_bytes (after the last pmce_model_set_tensor; whatever the current mode; 0 for a handle that adopted another
 * one's planes) says how much, pmce_model_set_split_arena hands it over (256-byte aligned device memory that must outlive the model
 * and every handle sharing its planes) - before pmce_model_finalize[_on], and again before a pmce_model_set_gemm_mode[_on] that
 * switches a finalized model to split_f16.  Without an arena the library falls back to hipMalloc / hipFree of its own.
 * A handle in gemm mode 2 reports the larger arena that mode needs (the planes AND the lifter blocks' f16 weights): a caller with an arena
 * of its own selects mode 2 before it asks, i.e. before pmce_model_finalize[_on] (a finalized model is re-opened by registering a tensor
 * again). */
size_t pmce_model_split_bytes(const pmce_model* m);
int pmce_model_set_split_arena(pmce_model* m, void* arena, size_t bytes);
/* Arithmetic of the path's 30 large products per forward (the pose lifter's Linear layers, the GRU input projections, the
 * packed AdaLN and final products): split_f16 != 0 (the default; env PMCE_SPLIT_F16=0 at create for the other) = the three-product f16 form of pmce_gemm_nt_split_f16 on weights the
 * model packs for itself at finalize, 0 = the fp32 matrix pipe.  Both meet fp32 accuracy (tests/test_gpu_ops.py measures
 * each against an fp64 product); may be called at any time between forwards.  In split_f16 mode the GRU recurrence, the decoder's
 * FFNs and 431x431 self-attention and the lifter's attention (pmce_seq_attention_split_f16, for J = 17 / 19) use the same
 * three-product form.
 * split_f16 == 2: the opt-in SINGLE-PRODUCT f16 mode of the lifter.  Everything is mode 1 except the 8 * depth products of the lifter's
 * blocks (qkv, proj, fc1, fc2 of every spatial and temporal block): those run as ONE f16 product with fp32 accumulation
 * (pmce_gemm_nt_f16) on weights packed by pmce_gemm_pack_f16 beside the planes, their A operands plain f16 rows (the form value 2 of
 * pmce_ln_chain_f32 and the attention entries).  The residual stream, LayerNorm statistics, the attention's arithmetic, the feature
 * products, GRU, decoder, upsampler and regression head are mode 1's.  NOT fp32-grade: about 0.2 to 0.6 mm on pose3d with synthetic
 * weights, which the decoder can amplify beyond 1e-3 m on the mesh of a worst clip.  The LayerNorm-epilogue products (C = 256) and the fused qkv + attention
 * kernel (C = 512) are not taken in this mode.  pmce_model_set_split_min_batch and the overflow word work as in mode 1.  Any other value
 * returns PMCE_ERR_ARG. */
int pmce_model_set_gemm_mode(pmce_model* m, int split_f16);
/* The same with the packing (when the mode changes on a finalized model) on `stream`; it first waits for the whole device
 * (forwards in flight may read the planes it frees), so it must not be called during a stream capture. */
int pmce_model_set_gemm_mode_on(pmce_model* m, int split_f16, pmce_stream_t stream);
int pmce_model_gemm_mode(const pmce_model* m); /* 0, 1 or 2 */
/* A second handle on the SAME registered weights (a pipeline lane) takes the source's packed planes instead of packing its own copy:
 * call after the last pmce_model_set_tensor of `dst` and before its pmce_model_finalize; the planes live until the last handle goes. */
int pmce_model_share_split_weights(pmce_model* dst, const pmce_model* src);
/* Calls with fewer clips (windows) than this stay on the fp32 pipe even in split_f16 mode (default 1 = none do: the f16 form is
 * faster at every batch size; env PMCE_SPLIT_MIN_BATCH at create). */
int pmce_model_set_split_min_batch(pmce_model* m, int clips);
/* Range of the split_f16 form, and the word that reports leaving it.  The path's one RAW input that feeds products - img_feat -
 * is stored per call as row-scaled f16 planes (pmce_split_rows_scaled_f16), so ANY finite fp32 input is computed with fp32-grade
 * accuracy, exactly as the reference's Linear layers accept it (PoseEstimation.py:80, CoevoDecoder.py:228); every other product
 * operand is the output of a LayerNorm / attention / GELU / GRU gate / AdaLN, whose magnitude the weights bound.  What remains:
 * non-finite INPUTS (they propagate into the outputs of their own clip only, as in the reference) and intermediate activations
 * beyond f16's 65504 under exotic weights - these turn into inf / nan, never into a wrong finite value, and every non-finite value
 * of a forward reaches a product epilogue, which sets a word in pinned host memory the model owns (readable without
 * synchronisation; sticky until pmce_model_clear_overflow).  pmce_model_overflowed reflects the device work that has completed:
 * synchronise the stream first for a definite answer about a given call.  DEFAULT POLICY: the word only reports - calls are never
 * refused, the model behaves like the reference (a bad clip yields nan, the next call is unaffected); pmce_amd's Pipeline /
 * evaluator poll it when they drain and can re-run the offending batch on the fp32 pipe (pmce_model_set_gemm_mode(m, 0) /
 * pmce_model_set_split_min_batch), which has fp32's own range.  STRICT policy (pmce_model_set_overflow_policy(m, 1), env
 * PMCE_STRICT_OVERFLOW=1 at create): while the word is set every entry point returns PMCE_ERR_OVERFLOW before launching
 * anything.  Pipeline lanes created with pmce_model_share_split_weights share the source's word. */
int pmce_model_set_overflow_policy(pmce_model* m, int strict);
/* the values in force (defaults come from PMCE_STRICT_OVERFLOW / PMCE_SPLIT_MIN_BATCH at create; pmce_model_share_split_weights copies both to the lane) */
int pmce_model_get_overflow_policy(const pmce_model* m);
int pmce_model_get_split_min_batch(const pmce_model* m);
/* Measurement aid (bench.py), per MODEL: while set (null = off), every launch of the split GEMM made by an entry point of this model
 * adds, per workgroup, the shader clocks and the 100 MHz wall ticks its first wave was resident to device_two_words[0] / [1]: their
 * ratio x 0.1 is the shader clock in GHz the chip sustained under the kernel (MI355X is power-limited there: 1.6 - 1.8 GHz, not the
 * 2.4 GHz of the peak figures). */
int pmce_model_set_clock_probe(pmce_model* m, unsigned long long* device_two_words);
int pmce_model_overflowed(const pmce_model* m);
int pmce_model_clear_overflow(pmce_model* m);
/* Bytes of caller-provided workspace needed for a batch of B clips. */
size_t pmce_model_workspace_bytes(const pmce_model* m, int batch);

/* Byte offset inside the workspace of a named intermediate ("X","Y0","g","GB","VT0","VT1","VT2","F1","F2","JM"),
 * -1 if unknown — for parity tests of intermediates (after a forward VT1/VT2/VT0 hold the vertices after
 * coevoblock1/2/3, "g" the GRU feature y[8]). */
long long pmce_model_workspace_offset(const pmce_model* m, int batch, const char* name);

/* GraphormerNet.forward: pose2d[B,16,J,2], img_feat[B,16,2048] -> pose3d[B,J,3] (mm). */
int pmce_lifter_forward(pmce_model* m, const float* pose2d, const float* img_feat, float* pose3d, int batch, void* ws,
                        size_t ws_bytes, pmce_stream_t stream);
/* Pose2Mesh.forward: joints[B,J,3] (m), img_feat[B,16,2048] -> cam_pose[B,J,3], cam_mesh[B,6890,3] (m). */
int pmce_decoder_forward(pmce_model* m, const float* joints, const float* img_feat, float* cam_pose, float* cam_mesh,
                         int batch, void* ws, size_t ws_bytes, pmce_stream_t stream);
/* PMCE.forward: -> cam_mesh[B,6890,3] (m), cam_pose[B,J,3] (m), pose3d[B,J,3] (mm);
 * if pred_pose != NULL also the caller's projection pred_pose[B,R,3] = J_regressor @ (cam_mesh*1000) (mm). */
int pmce_forward(pmce_model* m, const float* pose2d, const float* img_feat, float* cam_mesh, float* cam_pose,
                 float* pose3d, float* pred_pose, int batch, void* ws, size_t ws_bytes, pmce_stream_t stream);

/* CoevoBlock.forward for ONE block k in 1..3 on explicit inputs (reference lib/models/CoevoDecoder.py:175-191):
 * joints[B,J,3] (m), vt_in[B,431,3], g[B,2048] (AdaLN conditioning = y[seqlen//2], :229) -> vt_out[B,431,3]; joint_out[B,J,3]
 * only for k == 3 (joints1/joints2 are discarded by Pose2Mesh.forward, :235-237), else NULL. */
int pmce_coevo_block_forward(pmce_model* m, int k, const float* joints, const float* vt_in, const float* g, float* vt_out,
                             float* joint_out, int batch, void* ws, size_t ws_bytes, pmce_stream_t stream);


/* Streaming (stride-1 windows of ONE long sequence, lib/_img_utils.py:27-57): the window-independent per-frame work
 * (embedding + SpatialBlocks[0] + norm_s of the lifter, PoseEstimation.py:78-85; GRU layer-0 input projections) is done
 * once per frame into x0[L,J,C] and gi0[L,6144]; pmce_stream_forward then serves W windows (int32 win[W,2], inclusive
 * [start,end], start == end repeats the frame) from those tables.  Results equal pmce_forward on the assembled windows.
 * Workspace: pmce_model_workspace_bytes(m, ceil(L/16)) for the precompute, (m, W) for the forward. */
int pmce_stream_precompute(pmce_model* m, const float* pose2d_frames, const float* feat_frames, int L, float* x0, float* gi0,
                           void* ws, size_t ws_bytes, pmce_stream_t stream);
int pmce_stream_forward(pmce_model* m, const float* x0, const float* gi0, const int* win, int W, int L, float* cam_mesh,
                        float* cam_pose, float* pose3d, float* pred_pose, void* ws, size_t ws_bytes, pmce_stream_t stream);
/* The same with the demo's middle-frame override (main/run_demo.py:340-344: j2d_processing overwrites frame 8 of every window in place
 * before normalize_screen_coordinates, so the model sees that frame's 500-px crop coordinates, screen-normalised).  x0_mid[L,J,C] is a
 * second window-independent token table: the x0 output of a pmce_stream_precompute over (the poses each frame has AS THE MIDDLE of its
 * window - pmce_demo_targets_f32's mid_pose2d ordered by frame -, feat_frames); token rows (w, 8, j) are taken from it, every other row
 * and the whole GRU branch from x0 / gi0.  x0_mid == x0 gives pmce_stream_forward's bits. */
int pmce_stream_forward_mid(pmce_model* m, const float* x0, const float* x0_mid, const float* gi0, const int* win, int W, int L,
                            float* cam_mesh, float* cam_pose, float* pose3d, float* pred_pose, void* ws, size_t ws_bytes,
                            pmce_stream_t stream);
/* building blocks of the above; xn_split 1: XN written pre-split, 2: as plain f16 rows (see pmce_ln_chain_f32) */
int pmce_window_tokens_f32(const float* x0, const int* win, const float* tpos, const float* w2, const float* b2, float eps2,
                           float* X, float* XN, int W, int L, int T, int J, int C, int xn_split, pmce_stream_t stream);
/* Rewrites the W * J rows (w, t_mid, j) of X / XN (filled by pmce_window_tokens_f32) from x0_mid: X = x0_mid[m(w),j,:] + tpos[t_mid,:],
 * XN = LN(X), m(w) = start + t_mid (start when start == end); the arithmetic of pmce_window_tokens_f32. */
int pmce_window_mid_tokens_f32(const float* x0_mid, const int* win, const float* tpos, const float* w2, const float* b2, float eps2,
                               float* X, float* XN, int W, int L, int T, int J, int C, int t_mid, int xn_split, pmce_stream_t stream);
int pmce_window_rows_f32(const float* src, const int* win, float* dst, int W, int L, int T, int ncols, pmce_stream_t stream);

/* enable != 0 (default): pmce_forward / pmce_decoder_forward run the image-feature branch (GRU, AdaLN parameters) and the
 * short joint-side kernels on a second, internally created HIP stream, forked from and joined back into the caller's
 * stream with events (hipGraph-capturable; results are identical).  0 keeps every launch on the caller's stream. */
int pmce_model_set_concurrency(pmce_model* m, int enable);
int pmce_model_get_concurrency(const pmce_model* m);
int pmce_model_get_split_overlap(const pmce_model* m);
/* Temporal lifter blocks at C = 512 in split-f16 mode: qkv product + attention as one kernel (pmce_qkv_attention_fused_split_f16) instead of two
 * launches with the fp32 [M,3C] tensor between them.  Bit-identical results either way.  mode 0 = never (A/B), 1 (default) = on grids where it is
 * faster (large batches; small ones keep the two launches), 2 = always.  No environment variable; pipeline lanes inherit the owner's setting
 * (pmce_model_share_split_weights). */
int pmce_model_set_qkv_attention_fused(pmce_model* m, int mode);
int pmce_model_get_qkv_attention_fused(const pmce_model* m);

/* Staggering of several forwards in flight (one handle per lane, shared weights): makes `stream` wait until the pose
 * lifter of the last pmce_forward enqueued on `m` has finished, so that the next batch's lifter (long matrix-bound GEMMs)
 * runs beside that batch's decoder (short latency-bound kernels) instead of beside its lifter.  No-op before m's first
 * forward.  Ordering only: results do not depend on it. */
int pmce_model_wait_lifter(pmce_model* m, pmce_stream_t stream);

/* Per-kernel-class timing of the forwards above (HIP events on the caller's stream).  enable != 0 starts
 * accumulating; pmce_model_profile_read synchronises the recorded events and returns, for class i, its
 * name, accumulated milliseconds and launch count; returns the number of classes. */
int pmce_model_profile(pmce_model* m, int enable);
int pmce_model_profile_read(pmce_model* m, int i, const char** name, double* ms, long long* launches);

/* ---------------------------------------------------------------------------------------------------------
 * Individual operators (what the model object launches; exported for the parity tests and for callers that
 * want one stage).  Shapes in comments; B = clips.
 * ------------------------------------------------------------------------------------------------------- */

/* C[m,n] = act(sum_k A[m,k] W[n,k] + bias[n]) + R[m,n]  — every nn.Linear / the packed GRU, AdaLN and upsample
 * products (timm Mlp/Attention Linear layers; CoevoDecoder.py:19-20,214-224).  K % 32 == 0.  act: 0 none,
 * 1 exact GELU.  Row maps: if a_div > 0 row r of A is at A + (r % a_div)*a_lo + (r / a_div)*a_hi, else r*lda;
 * same for C and R with c_*.  batch > 1 adds bs* element offsets per batch index (grid.z). */
int pmce_gemm_nt_f32(const float* A, const float* W, const float* bias, const float* R, float* C, int M, int N, int K,
                     long long lda, int ldw, long long ldc, int act, int a_div, long long a_lo, long long a_hi, int c_div,
                     long long c_lo, long long c_hi, int batch, long long bsA, long long bsW, long long bsBias,
                     long long bsC, pmce_stream_t stream);
/* Tuning aid only: force the tile configuration (0..3, -1 = automatic) and the persistent workgroups per CU (1..8, 0 =
 * automatic) of pmce_gemm_nt_f32 for the whole process (initially automatic; no environment variable sets it, see pmce_model_create). */
int pmce_gemm_set_tuning(int tile, int grid_per_cu);
/* Tuning aid only, process-wide like the one above: at most n workgroups (rounded up to a multiple of 8; 0 = automatic, the initial state) per
 * launch of the persistent kernels of pmce_gemm_nt_f32, pmce_gemm_nt_split_f16 and pmce_gemm_nt_split_f16_ln, so that a product of a few dozen
 * tiles makes every workgroup walk several (tests/test_gpu_gemm_split_exact.py, tests/test_gpu_gemm_f32_exact.py).  The split product's
 * small-grid kernel takes one tile per workgroup by design and ignores it.  Results do not depend on it. */
int pmce_gemm_set_max_workgroups(int n);
/* The same nn.Linear product on the f16 matrix pipe with fp32 operands, result and accuracy: W is split ONCE into f16
 * (hi, lo) planes of W[n] * 2^s(n) by pmce_gemm_pack_split_f16 (Wp: N*K floats of storage; wscale: N floats, 2^-s(n) - one power
 * of two per OUTPUT ROW n of W, chosen so that the row's largest |w| 2^s lies in [2^14, 2^15): an outlier row does not cost the
 * other rows' lo planes their bits), A is split into (hi, lo * 2^11) on the fly, C[m][n] = 2^-s(n) (Ahi Whi + Ahi Wlo + Alo Whi)
 * accumulated in fp32 - error at or below the fp32 product's own rounding.  A, bias, R, C stay fp32 and row-major (lda, ldc);
 * |A| must be below 65504 here (an element outside the f16 range yields inf/nan, never a silently wrong finite value; raw inputs
 * of arbitrary magnitude go through pmce_split_rows_scaled_f16 and rscale below; inside a model call a non-finite result also sets the
 * model's overflow word, pmce_model_overflowed).
 * MI355X: while a kernel that issues f16 matrix instructions runs, packed-fp32 vector arithmetic (v_pk_{fma,mul,add}_f32) of
 * any other wave on the same CU may return wrong results (scripts/microbench/libpmce_diag.so: pmce_dbg_victim reproduces it).  No kernel of this library contains
 * such instructions, so its entries may overlap each other freely; do not overlap these entries with foreign kernels that do.
 * blocked != 0 / w_blocked != 0: the BLOCKED weight layout (what the model packs and multiplies) - the same planes as
 * [ceil(N/64)][K/16][64 rows][16 hi | 16 lo] (Wp: ceil(N/64)*64*K floats of storage), so that what a tile fetches per k-tile is
 * contiguous 4 KB pieces instead of 64-byte pieces one weight row apart.  Results are bit-identical in both layouts (same arithmetic,
 * same k order).
 * a_packed != 0: A is not fp32 but already split, [M][K/16][hi 16 f16 | lo*2^11 16 f16] (the layout the lifter's own producers write;
 * pmce_split_rows_f16 makes it from fp32 rows; lda == K).  c_packed != 0 (packed A, GELU, no residual, N % 32 == 0, ldc == N): the result
 * is written pre-split as well - it is the A operand of the next product (the lifter's fc1 -> fc2).
 * c_div > 0 (no residual, ldc == N): mapped output rows, row r of C at C + (r % c_div)*c_lo + (r / c_div)*c_hi (the GRU layer-0 input
 * projection writes (b,t) rows time-major); c_div == 0: row r at r*ldc.
 * rscale != NULL: RAW inputs of any finite fp32 magnitude.  pmce_split_rows_scaled_f16 stores row m of A[M][lda] as f16 (hi, lo * 2^11)
 * planes of A[m] * 2^-e(m) (Ap: M*K floats of storage) and rscale[m] = 2^e(m), e(m) lifting the row's largest |a| into [2^14, 2^15) - the
 * per-row treatment pmce_gemm_pack_split_f16 gives W; A = Ap is then a packed A (whatever a_packed says; no activation, residual or packed
 * result) and C[m][n] = 2^e(m) 2^-s(n) (Ahi Whi + Ahi Wlo + Alo Whi) + bias[n].  Rows holding inf / nan keep e = 0 and yield non-finite
 * results in their own row only.  A row-scaled product needs K >= 128 (K = 32 .. 127 returns PMCE_ERR_ARG: the kernels read a tile's row
 * scales after its last k-tile while the LDS-DMA cursor runs up to three k-tile stages ahead; every row-scaled product of the path has
 * K = 2048). */
int pmce_gemm_pack_split_f16(const float* W, int N, int K, int ldw, float* Wp, float* wscale, int blocked, pmce_stream_t stream);
int pmce_gemm_nt_split_f16(const float* A, const float* rscale, const float* Wp, int w_blocked, const float* wscale, const float* bias,
                           const float* R, float* C, int M, int N, int K, long long lda, long long ldc, int act, int a_packed,
                           int c_packed, int c_div, long long c_lo, long long c_hi, pmce_stream_t stream);
int pmce_split_rows_f16(const float* A, long long M, int K, long long lda, float* Ap, pmce_stream_t stream);
int pmce_split_rows_scaled_f16(const float* A, long long M, int K, long long lda, float* Ap, float* rscale, pmce_stream_t stream);
/* A product with N = 256 and a residual, followed by the LayerNorm chain of its consumer, in ONE launch (round 4; proj -> norm2 and
 * fc2 -> norm_s / norm_t -> next norm1 of a C = 256 lifter block, reference PoseEstimation.py:26-28,84-85,91-92,101-106): with
 * x = Ap W^T + bias + R,   y1 = ln1_w ? LN(x; ln1_w, ln1_b, ln1_eps) : x,   out1 = y1 (fp32 [M,256]; may alias R; may be NULL),
 * out2 = LN(y1; ln2_w, ln2_b, ln2_eps) written pre-split (the next product's packed A; may be NULL).  Ap pre-split [M,K]; Wp from
 * pmce_gemm_pack_split_f16, w_blocked = its `blocked`.  The same as pmce_gemm_nt_split_f16 + pmce_ln_chain_f32 up to the
 * summation order of the row statistics (two-pass fp32 in both). */
int pmce_gemm_nt_split_f16_ln(const float* Ap, const float* Wp, int w_blocked, const float* wscale, const float* bias, const float* R,
                              int M, int K, const float* ln1_w, const float* ln1_b, float ln1_eps, float* out1, const float* ln2_w,
                              const float* ln2_b, float ln2_eps, float* out2, pmce_stream_t stream);
/* Tuning aid only: force the tile configuration of pmce_gemm_nt_split_f16 (0: 128x256, 1: 128x128, 2: 64x128; -1 automatic). */
int pmce_gemm_split_set_tuning(int tile);
/* Which kernel pmce_gemm_nt_split_f16 launches for this product under the current tuning (a query: nothing is launched; the launch decides
 * through the same function).  0 / 1 / 2: the persistent kernel with the 128x256 / 128x128 / 64x128 tile; 3: 64x128 with two k-tiles per
 * stage; 4 / 5: the small-grid kernel (one tile per workgroup) with the 64x64 / 64x128 tile.  row_scaled implies a packed A.  Sizes the
 * product refuses (K < 32, K % 16 != 0, a row-scaled A with K < 128) return PMCE_ERR_ARG. */
int pmce_gemm_split_path(int M, int N, int K, int act, int a_packed, int c_packed, int has_residual, int row_scaled);
/* PoseEstimation.py:78-81 — x[tok] = joint_embed(pose2d) + imgfeat_embed(img_feat)[b,t] + spatial_pos[j]. */
int pmce_embed_tokens_f32(const float* pose2d, const float* E, const float* Wje, const float* bje, const float* spos,
                          float* x, long long ntok, int J, int C, pmce_stream_t stream);
/* The same followed by LayerNorm(w2, b2, eps2) of every token row (SpatialBlocks[0].norm1, PoseEstimation.py:13-29 via :83) in ONE launch:
 * x = the tokens (fp32 [ntok, C]), xn = their LayerNorm - fp32, or pre-split [row][C/16][16 hi | 16 lo*2^11] f16 when xn_split is 1 (the operand of a
 * three-product f16 GEMM), or plain f16 [row][C] when it is 2 (see pmce_ln_chain_f32).  Bit-identical to pmce_embed_tokens_f32 + pmce_ln_chain_f32(out2).  C = 128, 256, 384 or 512. */
int pmce_embed_ln_f32(const float* pose2d, const float* E, const float* Wje, const float* bje, const float* spos, float* x,
                      long long ntok, int J, int C, const float* w2, const float* b2, float eps2, float* xn, int xn_split,
                      pmce_stream_t stream);
/* nn.LayerNorm chain over rows of C channels (C = 128, 256, 384 or 512, as for every row kernel of the lifter): y1 = (w1 ? LN(x;w1,b1,eps1) : x) + add[(row/add_div)%add_mod];
 * out1 = y1 (optional); out2 = LN(y1;w2,b2,eps2) (optional).  norm1/norm2/norm_s/norm_t (PoseEstimation.py:17,23,58-59).
 * out2_split (and out_split / xn_split of the entries below) != 0: out2 / out / XN written pre-split ([row][C/16][16 hi | 16 lo*2^11] f16
 * in the bytes of the fp32 row), i.e. directly as the A operand of pmce_gemm_nt_split_f16(a_packed = 1).
 * The value 2 of the same arguments: plain f16 [row][C], two bytes per channel in the first half of the buffer, every value rounded to
 * nearest even with |x| < 2^-14 flushed to zero (inf and NaN stay) - the A operand of pmce_gemm_nt_f16 (lda = C).  out1 stays fp32.
 * Any other value returns PMCE_ERR_ARG. */
int pmce_ln_chain_f32(const float* x, long long rows, int C, const float* w1, const float* b1, float eps1, const float* add,
                      int add_div, int add_mod, float* out1, const float* w2, const float* b2, float eps2, float* out2,
                      int out2_split, pmce_stream_t stream);
/* timm Attention core on qkv[tok][3C] for sequences of N <= 32 tokens, 8 heads of 32 or 64 channels (C = 256 or 512;
 * PoseEstimation.py:19 / CoevoDecoder.py:118-131).
 * sequence s, position i -> token (s % seq_div)*seq_lo + (s / seq_div)*seq_hi + i*tok_stride. */
int pmce_seq_attention_f32(const float* qkv, float* out, int nseq, int N, int C, int seq_div, long long seq_lo,
                           long long seq_hi, long long tok_stride, int out_split, pmce_stream_t stream);
/* The same for every width pmce_model_create accepts - what the model calls: C = 256 and 512 are pmce_seq_attention_f32's launches (the same
 * bits), C = 128 and 384 (heads of 16 and 48 channels) the same kernel at those head sizes.  Any other C returns PMCE_ERR_ARG before any launch. */
int pmce_lifter_attention_f32(const float* qkv, float* out, int nseq, int N, int C, int seq_div, long long seq_lo,
                              long long seq_hi, long long tok_stride, int out_split, pmce_stream_t stream);
/* The same attention (timm Attention of PoseEstimation.py:78-104) on the f16 matrix pipe in the three-product form: q, k, v read
 * as fp32 (split into f16 (hi, lo) planes inside the kernel), the result WRITTEN pre-split ([row][C/16][16 hi | 16 lo*2^11] f16 in
 * the bytes of the fp32 row) as the A operand of proj.  Sequence / token addressing as pmce_seq_attention_f32.  C = 256 or 512 (8 heads),
 * N = 16, 17 or 19 (pmce_seq_attention_split_supported tells); anything else returns PMCE_ERR_ARG - callers keep fp32 qkv and
 * pmce_seq_attention_f32 there.  A non-finite result sets the calling thread's overflow sink like the products do. */
int pmce_seq_attention_split_supported(int N, int C);
int pmce_seq_attention_split_f16(const float* qkv, float* out_planes, int nseq, int N, int C, int seq_div, long long seq_lo,
                                 long long seq_hi, long long tok_stride, pmce_stream_t stream);
/* The matrix-pipe attention for every width pmce_model_create accepts - what the model calls.  C = 256 and 512 are forwarded to pmce_seq_attention_split_f16 (the
 * same launch, the same bits); C = 128 and 384 (heads of 16 and 48 channels) run the same head stage (attention_head of
 * seq_attention_mfma.hip) on units of 512 / 768 bytes per row (lifter_attention_mfma.hip).  N = 16, 17 or 19; anything else returns PMCE_ERR_ARG before any launch. */
int pmce_lifter_attention_split_supported(int N, int C);
int pmce_lifter_attention_split_f16(const float* qkv, float* out_planes, int nseq, int N, int C, int seq_div, long long seq_lo,
                                    long long seq_hi, long long tok_stride, pmce_stream_t stream);
/* The same with the result's form as an argument: out_form 1 = pmce_lifter_attention_split_f16 (which forwards here: the same launch, the
 * same bits), 2 = plain f16 rows out[token][C] - the hi plane of form 1 with |x| < 2^-14 flushed to zero - the A operand of
 * pmce_gemm_nt_f16 (half the bytes written).  The arithmetic inside is the same. */
int pmce_lifter_attention_split_f16_form(const float* qkv, float* out, int nseq, int N, int C, int seq_div, long long seq_lo,
                                         long long seq_hi, long long tok_stride, int out_form, pmce_stream_t stream);
/* Temporal block, C = 512, split-f16 form: AO = attention(XN Wqkv^T + b) in ONE kernel - what pmce_gemm_nt_split_f16 (a_packed, blocked weight)
 * into fp32 qkv[M][3C] followed by pmce_seq_attention_split_f16(nseq = B*J, N = 16, seq_div = J, seq_lo = 1, seq_hi = 16*J, tok_stride = J) compute,
 * bit for bit, without the qkv tensor.  xn_planes / out_planes: pre-split rows [B*16*J][C/16][16 hi | 16 lo*2^11] f16; Wp / wscale: the [3C][C]
 * weight from pmce_gemm_pack_split_f16(blocked = 1); bias [3C] or NULL.  Sequences are the 16 frames of (clip, joint).  C must be 512.  A
 * non-finite result sets overflow_word (device-visible) to 1; NULL = the calling thread's overflow sink, as the products and the attention use. */
int pmce_qkv_attention_fused_split_f16(const float* xn_planes, const float* Wp, const float* wscale, const float* bias, float* out_planes, int B,
                                       int J, int C, unsigned* overflow_word, pmce_stream_t stream);
/* PoseEstimation.py:62-66,109-113 — LayerNorm(1e-5) + Linear(C->3) + Conv2d(T->1) frame fusion.
 * prew != NULL: x is the LAST TemporalBlock's output BEFORE its post-norm, and every row passes through LayerNorm(prew, preb, pre_eps) (norm_t,
 * PoseEstimation.py:92) on the way in - bit-identical to pmce_ln_chain_f32(out1) followed by the head on its result, without the launch and the
 * round trip. */
int pmce_lifter_head_f32(const float* x, const float* prew, const float* preb, float pre_eps, const float* lnw, const float* lnb,
                         const float* Wr, const float* br, const float* wf, const float* bf, float* pose3d, int B, int T, int J, int C,
                         pmce_stream_t stream);

/* Fused nn.GRU time step for ndir directions: gh = h_prev W_hh^T + b_hh on the matrix cores, then the gate update
 * (CoevoDecoder.py:216-221); gi = W_ih x + b_ih comes from pmce_gemm_nt_f32.  hp == NULL means h_prev = 0. */
int pmce_gru_step_f32(const float* gi0, const float* gi1, const float* whh0, const float* whh1, const float* bhh0,
                      const float* bhh1, const float* hp0, const float* hp1, float* ho0, float* ho1, long long gi_rs,
                      long long h_rs, int B, int H, int ndir, pmce_stream_t stream);
/* The same step with gh = h W_hh^T in the three-product f16 form (pmce_gemm_nt_split_f16's arithmetic): whh0p / whh1p are rows of
 * ONE weight packed by pmce_gemm_pack_split_f16 (K = H), wscale its scale pair, w_blocked its `blocked` (1 is what the model runs: the
 * 16 rows a DMA instruction fetches are 1 KB contiguous; whh0p / whh1p = the first row of each direction, a multiple of 64 rows apart).
 * B <= 64 runs a small-batch kernel (a workgroup per 8 hidden units: 256 workgroups whatever the batch), larger batches 64 rows x 32 units
 * per workgroup - same numbers, bit for bit, in both layouts, and for the same ROW INDEX at every batch size (this holds for pmce_gru_step_f32
 * too).  The rounding of a row does depend on its place in its 32-row tile: gh is summed in four K-quarters, and the quarter (row >> 3) & 3
 * adds the sum of the other three to its own.  Rows 32 apart get the same bits; the same clip at rows 0, 8, 16 and 24 gets results that agree
 * to fp32 rounding (each within 5e-6 of the fp64 step, tests/test_gpu_gru.py), not bit for bit. */
int pmce_gru_step_split_f32(const float* gi0, const float* gi1, const float* whh0p, const float* whh1p, const float* wscale,
                            const float* bhh0, const float* bhh1, const float* hp0, const float* hp1, float* ho0, float* ho1,
                            long long gi_rs, long long h_rs, int B, int H, int ndir, int w_blocked, pmce_stream_t stream);
/* y = x / denom (PMCE.py:18). */
int pmce_div_scalar_f32(const float* x, float* y, long long n, float denom, pmce_stream_t stream);

/* CoevoDecoder.py:232 — vertxs[b][v][:] = joints[b][vj[v]][:]; vj int32[431].  Bit-exact copy. */
int pmce_vertex_init_gather_f32(const float* joints, const int* vj, float* vt, int B, int J, pmce_stream_t stream);
/* Key/value side of the vertex<-joint CrossAttention (CoevoDecoder.py:47-62,83) with Wq / proj folded in:
 * GB[b][inst*128 + (gamma 0..63 | beta 64..127)] are the AdaLN parameters; Kf,Vf [B,64,64], s0 [B,64].
 * img != NULL (J <= 23): also writes the operands as the LDS image pmce_vertex_ca_mlp_f32's split_f16 form copies: per clip
 * pmce_ca_image_floats() floats - s0, two scales, Kf and Vf as (hi | lo) f16 fragment planes scaled by one power of two each.  Kf / s0 / Vf may
 * each be NULL when only the image is wanted. */
int pmce_ca_image_floats(void);
int pmce_ca_image_floats_written(int J); /* of a clip's row, the floats pmce_ca_fold_f32 writes at J joints (J <= 23) */
int pmce_ca_fold_f32(const float* xk, const float* xv, const float* GB, int gb_stride, int iq, int ik, int iv,
                     const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv, const float* bv,
                     const float* Wp, float* Kf, float* s0, float* Vf, float* img, int B, int J, pmce_stream_t stream);
/* The joint side of a CoevoBlock in ONE launch (what the model runs): the joint embedding of CoevoDecoder.py:177-180,184 -
 * jf = joint_proj(jt) + joint_pos_embed, xk = proj_j2v_dim(jf) + j2v_K_embed, xv = jf - followed by the fold above.  jf_out [B,J,64] may be
 * NULL (only the block-3 joint stream reads it). */
int pmce_joint_prep_f32(const float* jt, const float* Wj, const float* bj, const float* jpos, const float* Wj2v, const float* bj2v,
                        const float* j2vK, float* jf_out, const float* GB, int gb_stride, int iq, int ik, int iv, const float* Wq,
                        const float* bq, const float* Wk, const float* bk, const float* Wv, const float* bv, const float* Wp,
                        float* Kf, float* s0, float* Vf, float* img, int B, int J, pmce_stream_t stream);
/* THE north-star kernel: fused AdaLN + vertex<-joint cross-attention + residual for 431 query tokens
 * (first line of CrossAttentionBlock.forward, CoevoDecoder.py:83).  xq[B,431,64], or xq == NULL and
 * xq := Wv3*vt + Eq formed on the fly from vt[B,431,3]. */
int pmce_vertex_ca_f32(const float* xq, const float* vt, const float* Wv3, const float* Eq, const float* Kf,
                       const float* s0, const float* Vf, const float* bp, float* out, int B, int J, pmce_stream_t stream);
/* The FFN of the two kernels below: split_f16 != 0 runs the 64->256->64 FFN in the three-product f16 form (activations split in registers;
 * fp32 accumulate, fp32 results); ffn_img != NULL: every workgroup COPIES the FFN's f16 planes into LDS (LDS-DMA) from an image made once
 * (pmce_ffn_pack_f16 from the same W1 [256,64] / W2 [64,256]: pmce_ffn_image_floats() floats, 16-byte aligned) instead of converting
 * W1 / W2 itself - the same bits; pmce_model_finalize makes the six images. */
int pmce_ffn_image_floats(void);
int pmce_ffn_pack_f16(const float* W1, const float* W2, float* ffn_img, pmce_stream_t stream);
/* x + Mlp(AdaLN(x)) on [B,431,64] (CoevoDecoder.py:85-86,104); optional Linear(64->3)+coordinate residual (:189). */
int pmce_adaln_mlp_f32(const float* xin, const float* GB, int gb_stride, int inst, const float* W1, const float* b1,
                       const float* W2, const float* b2, float* yout, const float* Wc, const float* bc, const float* vt_in,
                       float* vt_out, int B, int split_f16, const float* ffn_img, pmce_stream_t stream);
/* The whole CrossAttentionBlock of the vertex stream in one launch (reference CoevoDecoder.py:82-87): vertex_ca followed by
 * its FFN (adaln_mlp with AdaLN instance `inst` of GB), the intermediate never leaving registers; arguments as those two.
 * Same arithmetic in the same order as pmce_vertex_ca_f32 + pmce_adaln_mlp_f32.  J <= 23 runs fused; beyond that one clip's
 * folded operands do not fit beside the FFN weights in LDS and the call runs the two kernels through `scratch` [B,431,64]
 * (may be NULL when J <= 23; fp32 attention from Kf / s0 / Vf).  split_f16 != 0 also runs the cross-attention's two contractions in the
 * three-product form and REQUIRES ca_img = the folded operands' image of pmce_ca_fold_f32 / pmce_joint_prep_f32 (Kf / s0 / Vf are then
 * not read). */
int pmce_vertex_ca_mlp_f32(const float* xq, const float* vt, const float* Wv3, const float* Eq, const float* Kf,
                           const float* s0, const float* Vf, const float* bp, const float* GB, int gb_stride, int inst,
                           const float* W1, const float* b1, const float* W2, const float* b2, float* yout, float* scratch,
                           int B, int J, int split_f16, const float* ffn_img, const float* ca_img, pmce_stream_t stream);

/* fp32 pipe: qkv = Linear(64->192)(AdaLN(x)) on [B,431,64] (CoevoDecoder.py:103,120), then
 * y = x + proj(softmax(q k^T/sqrt(32)) v), 2 heads, 431x431 per clip (CoevoDecoder.py:118-131,103). */
int pmce_adaln_qkv_f32(const float* xin, const float* GB, int gb_stride, int inst, const float* Wqkv, const float* bqkv,
                       float* qkv, int B, pmce_stream_t stream);
int pmce_vertex_sa_f32(const float* xin, const float* qkv, const float* Wp, const float* bp, float* yout, int B,
                       pmce_stream_t stream);
/* The qkv weight [192,64] as the f16 image pmce_vertex_sab_split_f32 copies into LDS: pmce_qkv_image_floats() floats, 16-byte aligned, made
 * once per weight. */
int pmce_qkv_image_floats(void);
int pmce_qkv_pack_f16(const float* Wqkv, float* qkv_img, pmce_stream_t stream);
/* The attention half of the vertex stream's AdaLN Block in ONE launch, three-product f16 form (what a model in split_f16 mode runs):
 *   y = x + proj(softmax(q k^T/sqrt(32)) v),  [q|k|v] = Linear(64->192)(AdaLN(x))   (CoevoDecoder.py:103,118-131)
 * without a [B,431,192] fp32 QKV round trip: q, k, v come out of the qkv product's accumulators in the attention's own operand
 * layouts (every contraction but the output projection as three f16 matrix products of (hi, lo) halves, fp32 accumulate); k and v pass through `scratch`
 * (pmce_vertex_sab_scratch_floats(B) floats, 16-byte aligned, caller-owned, contents meaningless outside the call) as f16 (hi | lo)
 * fragment planes.  qkv_img = pmce_qkv_pack_f16(Wqkv).  B > 128: one workgroup per clip; otherwise two. */
long long pmce_vertex_sab_scratch_floats(int B);
int pmce_vertex_sab_split_f32(const float* xin, const float* GB, int gb_stride, int inst, const float* qkv_img, const float* bqkv,
                              const float* Wp, const float* bp, float* scratch, float* yout, int B, pmce_stream_t stream);
/* k|v of the joint<-vertex CrossAttention for the 431 vertex tokens: kv[B,431,128] (CoevoDecoder.py:52-53,83,183).
 * tkv_img != NULL: its three 64 x 64 products (proj_v2j_dim, wk, wv) in the three-product f16 form (what a model in split_f16 mode runs):
 * tkv_img = pmce_tkv_pack_f16(Wv2j, Wk, Wv), pmce_tkv_image_floats() floats, 16-byte aligned, made once; NULL = the fp32 form. */
int pmce_tkv_image_floats(void);
int pmce_tkv_pack_f16(const float* Wv2j, const float* Wk, const float* Wv, float* tkv_img, pmce_stream_t stream);
int pmce_tokens_kv_f32(const float* xk, const float* xv, const float* vt, const float* Wv3, const float* Ev,
                       const float* Wv2j, const float* Ek, const float* GB, int gb_stride, int ik, int iv, const float* Wk,
                       const float* bk, const float* Wv, const float* bv, float* kv, int B, const float* tkv_img, pmce_stream_t stream);
/* Joint stream of a CoevoBlock (CoevoDecoder.py:183,187,189): stage 1 = joint<-vertex cross-attention +
 * residual only, 2 = + FFN, 3 = + self-attention block + coordinate head.  wptr: 18 weight pointers
 * (wq,bq,proj_w,proj_b,fc1_w,fc1_b,fc2_w,fc2_b,qkv_w,qkv_b,sproj_w,sproj_b,sfc1_w,sfc1_b,sfc2_w,sfc2_b,coor_w,coor_b);
 * inst: AdaLN instance ids (normq, norm2, SA.norm1, SA.norm2).  Stage 4 = the self-attention block alone (kv may be NULL).  y_out is
 * required at stages 1 and 2 and optional beyond; pose_out (stages 3, 4) needs jt. */
int pmce_joint_stream_f32(const float* xq, const float* jQ, const float* kv, const float* GB, int gb_stride,
                          const float* const* wptr, const int* inst, const float* jt, float* y_out, float* pose_out, int B,
                          int J, int stage, pmce_stream_t stream);
/* Operand of the packed upsample+residual product: A[b] = [relu(g[b]) | vt[b] flattened | 0-pad] (CoevoDecoder.py:238-244).
 * packed != 0 (KP % 16 == 0): the rows are written pre-split - the A operand of pmce_gemm_nt_split_f16(a_packed = 1); what the model runs. */
int pmce_build_final_operand_f32(const float* g, const float* vt, float* A, int B, int KP, int packed, pmce_stream_t stream);
/* lib/core/base.py:223-225 — out[b][r][:] = sum_nz data * (mesh[b][col][:] * scale); CSR regressor [R,6890]. */
int pmce_j_regress_f32(const float* mesh, const int* indptr, const int* indices, const float* data, float* out, int B,
                       int R, int NVF, float scale, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Evaluation metrics directly behind the path: replace the per-batch D2H + numpy of
 * compute_both_err (data/PW3D/dataset.py:269-282) and the per-sample loop of evaluate (:351-462).
 * ------------------------------------------------------------------------------------------------------- */
/* Per sample b: mpvpe[b] = mean_v ||(pm*scale - rp) - (gm*scale - rg)||; joints P = pj - rowsum*rp (if rowsum), minus
 * joint root_j, restricted to eval_idx (int32[n_eval]); mpjpe[b] = mean ||P-G||; pampjpe[b] after rigid_align
 * (lib/coord_utils.py:151-173, fp64).  rp/rg NULL -> mesh roots are the samples' own joint root_j (compute_both_err).
 * out_pe/out_ge (optional, [B,n_eval,3]) receive the aligned eval joints for pmce_accel_error_f32.
 * V == 0 (pm, gm, rp, rg, rowsum NULL): joints only - the pose-only flavours compute_joint_err / evaluate_joint
 * (data/Human36M/dataset.py:600-713: root 0, the 14 eval joints; data/PW3D/dataset.py:260-349: COCO set, root = joint J-2, every joint)
 * and MPII3D.evaluate (data/MPII3D/dataset.py:539-624: root 0, all 17 joints); mpvpe[b] = 0 then. */
int pmce_sample_errors_f32(const float* pm, const float* gm, float scale, int V, const float* rp, const float* rg,
                           const float* pj, const float* gj, int NJ, const float* rowsum, const int* eval_idx, int n_eval,
                           int root_j, float* out_mpvpe, float* out_mpjpe, float* out_pampjpe, float* out_pe, float* out_ge,
                           int B, pmce_stream_t stream);
/* Per-sample acceleration error (lib/coord_utils.py:218-245 as used at data/PW3D/dataset.py:415-429): 0 for the first and
 * last sample of each sequence (seq int32[N], samples of a sequence contiguous). */
int pmce_accel_error_f32(const float* pe, const float* ge, const int* seq, float* out, int N, int n_eval,
                         pmce_stream_t stream);

/* Sliding-window clip assembly on the GPU (lib/_img_utils.py:42-55; demo lib/utils/_dataset_demo.py:98-102):
 * per-frame tables pose[L,J,2], feat[L,2048] + windows int32[W,2] (inclusive [start,end]; start == end repeats the frame)
 * -> out_pose[W,16,J,2], out_feat[W,16,2048]. */
int pmce_assemble_windows_f32(const float* pose, const float* feat, const int* win, float* out_pose, float* out_feat, int W,
                              int L, int J, pmce_stream_t stream);

/* Detector keypoints -> model input, per frame (data/PW3D/dataset.py:185-204 add_pelvis_and_neck /
 * normalize_screen_coordinates, applied at :160-161 and :235-237): kp[L,J0,kp_stride] pixel coordinates (x, y first),
 * shape int32[L,2] = (height, width) -> out[L,J0+n_extra,2]; n_extra = 1 appends the pelvis (hip midpoint), 2 also the
 * neck (shoulder midpoint); x' = x/w*2 - 1, y' = y/w*2 - h/w. */
int pmce_prepare_pose2d_f32(const float* kp, int kp_stride, const int* shape, float* out, int L, int J0, int n_extra, int lhip,
                            int rhip, int lsho, int rsho, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's weak-perspective camera fit (main/run_demo.py:134-173 optimize_cam_param on lib/models/project_net.py:6-16
 * OptimzeCamLayer): per window, `steps` Adam steps (betas 0.9 / 0.999, eps 1e-8, moments zeroed per window) on cam = (s, tx, ty)
 * against the L1 loss mean_jc |(scale * joints3d[w][j][c] + cam[1 + c]) * cam[0] * crop_size/2 + crop_size/2 - target2d[w][j][c]|,
 * j < n_fit, c < 2.  _f32 / _f64: the compute type, which is also the type of EVERY floating-point buffer of the call.
 *   joints3d[W][n_fit][3], target2d[W][n_target][2] (n_target >= n_fit: the demo passes 19 rows and fits the first 17), n_fit in 1..32;
 *   step_table[steps][2] = (lr_t / (1 - 0.9^t), sqrt(1 - 0.999^t)) for t = 1..steps, computed by the caller in double (it carries the
 *     learning-rate schedule; pmce_amd.camera.step_table makes the demo's: 0.1, 0.05 after loop index 100, 0.001 after 200);
 *   chains: windows seq_offsets[s] .. seq_offsets[s + 1] - 1 (int32[S + 1], monotone, first 0, last W) form one chain - its first window
 *     starts from init[s] (init[S][3]), each later one from its predecessor's result, as the demo does along a tracklet (its project_net
 *     is created once, :245).  The table is given twice: seq_offsets_host is validated here, seq_offsets is the same table in device
 *     memory.  Both NULL (then S == W): every window is its own chain and starts from init[w];
 *   cam[W][3] = the camera after `steps` updates, loss[W] = the L1 loss at that camera;
 *   optional (all or none): bbox[W][4] = (x, y, w, h), img_w, img_h > 0 -> orig_cam[W][4] = (sx, sy, tx, ty), the demo's
 *     convert_crop_cam_to_orig_img (run_demo.py:49-67); otherwise NULL, NULL and img_w = img_h = 0.
 * One wave per chain, results bit-identical whatever W, S and the window's place in the batch.  fp64 follows the reference's fp64 run to
 * rounding; fp32 is the reference's dtype, where the loop is chaotic (sign gradients) and agrees as the reference's fp32 does with its fp64. */
int pmce_camfit_f32(const float* joints3d, const float* target2d, const float* init, const int* seq_offsets_host,
                    const int* seq_offsets, const float* step_table, float* cam, float* loss, const float* bbox, float* orig_cam, int W,
                    int S, int n_fit, int n_target, int steps, double scale, double crop_size, double img_w, double img_h,
                    pmce_stream_t stream);
int pmce_camfit_f64(const double* joints3d, const double* target2d, const double* init, const int* seq_offsets_host,
                    const int* seq_offsets, const double* step_table, double* cam, double* loss, const double* bbox, double* orig_cam,
                    int W, int S, int n_fit, int n_target, int steps, double scale, double crop_size, double img_w, double img_h,
                    pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's per-window target preparation (main/run_demo.py:340-344), one launch for a window table win[W,2] over per-frame pixel
 * keypoints kp[L,J0,kp_stride] (x, y first; COCO-17 in the demo).  With m = start + t_mid (start when start == end) the window's middle
 * frame: pelvis and neck are appended (run_demo.py:116-128), get_bbox and process_bbox(aspect_ratio = 1, scale = box_scale) give
 * bbox[W,4] = (x, y, w, h) in the reference's float32 operation order (lib/coord_utils.py:45-90), j2d_processing's rot = 0 affine gives
 * target2d[W,J0+2,2] in pixels of the crop_size x crop_size crop (lib/aug_utils.py:51-64), and mid_pose2d[W,J0+2,2] =
 * target2d / img_w * 2 - (1, img_h / img_w) is what the reference's in-place write leaves the model to see as that window's frame t_mid.
 * valid[W] (int32) is 0 where process_bbox returns None (w * h <= 0, or a box less than a pixel wide or high) or a keypoint is not finite:
 * bbox, target2d and mid_pose2d of such a window are NaN. */
int pmce_demo_targets_f32(const float* kp, int kp_stride, const int* win, float* bbox, float* target2d, float* mid_pose2d, int* valid,
                          int W, int L, int J0, int t_mid, float img_w, float img_h, float crop_size, float box_scale, int lhip, int rhip,
                          int lsho, int rsho, pmce_stream_t stream);
/* pose_windows[W,T,J,2] (pmce_assemble_windows_f32's out_pose): row t_mid of every window replaced by mid_pose2d[W,J,2]. */
int pmce_demo_override_mid_f32(float* pose_windows, const float* mid_pose2d, int W, int T, int J, int t_mid, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's mesh overlays (demo/renderer.py, main/run_demo.py:402-415): a batched triangle rasteriser with a z-buffer, smooth shading and
 * the demo's compositing rule.  A job is one person in one frame: verts[N][V][3] (fp32, metres, the model's frame), cams[N][4] =
 * (sx, sy, tx, ty) (pmce_camfit_*'s orig_cam), rotation[N][9] (row-major 3 x 3, applied to the reference's flipped mesh) or NULL.
 *     u = (sx (x + tx) + 1) width / 2,  v = (sy (y + ty) + 1) height / 2  (origin top-left, y down),  depth = z, smaller is nearer.
 * u, v are snapped to int32 with 8 sub-pixel bits; coverage is exact integer arithmetic on them: samples at pixel centres, top-left fill
 * rule.  A triangle with a vertex beyond +-2^14 px is dropped.  Fragments with z outside [-1, 1] are discarded; the nearest survivor
 * wins, equal z goes to the lowest face index; the result is the same bits every run.  Covered pixels of images[F][height][width][3]
 * (uint8, updated in place) take clamp(emissive + (ambient + intensity / pi * sum_l max(0, n . l)) * base) per channel, 8-bit value
 * floor(255 c + 0.5), n the interpolated, normalised vertex normal (area-weighted); every other pixel keeps its bits.
 *   faces[n_faces][3] int32 (device); vf_offsets[V + 1], vf_faces[3 n_faces]: the vertex -> incident faces CSR (device; the order of a
 *     vertex' list is the order its normal is summed in);
 *   job_frame[N]: the frame of each job.  The persons of a frame are drawn as LAYERS: sched[N] lists the jobs layer by layer
 *     (layer_offsets[n_layers + 1], first 0, last N), ascending distinct frames inside a layer.  depth_order = 0: a job paints over what
 *     the earlier layers left in its frame (the reference's order); 1: depth test across the jobs of a frame (layers * faces < 2^31).
 *     job_frame and sched are given twice, on the host (validated here) and on the device; layer_offsets on the host only;
 *   material (host) = (base[3], emissive, ambient, intensity); lights (host) [n_lights <= 8][3]: unit vectors towards the light, model frame;
 *   status[N] (device, out): bit 0 = a non-finite vertex, camera or rotation (the job draws nothing), bit 1 = a triangle dropped at the
 *     guard band;  optional outputs (NULL = not wanted): xy_fixed[N][V][2] int32 the snapped coordinates, face_id[F][height][width]
 *     int32 and depth[F][height][width] fp32, written where a pixel is drawn (the caller fills them beforehand);
 *   workspace: 16-byte aligned device memory of at least pmce_render_workspace_bytes(N, V, width, height, 1) bytes; the frames are
 *     processed in chunks of as many frames as fit (chunk_frames of the query = frames per chunk), with the same result whatever the chunk.
 *     Its content on entry does not matter.  width, height <= 8192.  A frame is read and written only inside the rectangles of its jobs.
 * The query returns 0 (and sets the error string) for arguments out of range. */
size_t pmce_render_workspace_bytes(int n_jobs, int n_verts, int width, int height, int chunk_frames);
int pmce_render_meshes(unsigned char* images, int n_frames, int width, int height, const float* verts, const float* cams,
                       const float* rotation, int n_jobs, int n_verts, const int* faces, int n_faces, const int* vf_offsets,
                       const int* vf_faces, const int* job_frame_host, const int* job_frame, const int* sched_host, const int* sched,
                       const int* layer_offsets_host, int n_layers, const float* material, const float* lights, int n_lights,
                       int cull_backfaces, int depth_order, int* status, int* xy_fixed, int* face_id, float* depth, void* workspace,
                       size_t workspace_bytes, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Batched SMPL forward (reference smplpytorch SMPL_Layer.forward with center_idx = None, fp32): the ground-truth meshes of the evaluation
 * from the datasets' SMPL fits.  Two launches on `stream` (pose kernel: one wave per sample; skinning kernel: 256 vertices x 16 samples
 * per workgroup), no atomics, no synchronisation; a sample's result does not depend on the batch it is in.
 *   model tables (device, prepared once by pmce_amd.smpl.SMPLModel):
 *     v_template_t[3][V]; dirs_t[220][3][V] = the 10 shape directions, the 207 pose directions, three zero rows;
 *     weights_t[24][V]; j_template[24][3] = J_regressor v_template and j_shapedirs[24][3][10] = J_regressor shapedirs (fp64 products
 *     rounded to fp32); parents_host[24] (host): the kinematic tree, entry i > 0 in [0, i), entry 0 not read; n_joints must be 24;
 *   pose[B][72] axis-angle, betas[B][10], trans[B][3] or NULL (zeros);
 *   optional camera form (both or neither), data/Human36M/dataset.py:354-398: cam_R[B][3][3], cam_t[B][3] in mm - the root rotation
 *     becomes cam_R R_0, betas are zeroed where any |beta| > 3, the translation becomes cam_R trans + cam_t / 1000 - J_0 + cam_R J_0.
 *     A zero root pose gives cam_R itself (the reference divides 0 by 0 there);
 *   sample_index[n] (device, int32, distinct entries in [0, B)) or NULL (then n == B): the rows this call computes, read and written
 *     in place - one call per gender of a mixed batch.  An entry outside [0, B) is ignored;
 *   verts_out[B][V][3], joints_out[B][24][3] = (x + trans) * scale - offset[b], offset[B][3] or NULL: scale = 1 without offset gives
 *     the layer's metres, scale = 1000 with the root joint in mm gives data/PW3D/dataset.py:86,240;
 *   workspace: 16-byte aligned device memory of at least pmce_smpl_workspace_bytes(B) bytes (rows indexed by sample).
 * The query returns 0 (and sets the error string) for B < 1. */
size_t pmce_smpl_workspace_bytes(int B);
int pmce_smpl_forward(const float* v_template_t, const float* dirs_t, const float* weights_t, const float* j_template,
                      const float* j_shapedirs, const int* parents_host, int n_joints, const float* pose, const float* betas,
                      const float* trans, const float* cam_R, const float* cam_t, const int* sample_index, int n, float scale,
                      const float* offset, float* verts_out, float* joints_out, void* workspace, size_t workspace_bytes, int B, int V,
                      pmce_stream_t stream);
/* The same layer on rotation matrices (smplx's pose2rot = False, what the HMR head calls: lib/models/spin.py:184-189):
 * rotmats[B][24][3][3] row-major replace `pose` and are used as they are - the pose map is R[1:] - I, no Rodrigues formula - and there is
 * no camera form.  betas is read at betas[b * betas_stride + 0..9], betas_stride >= 10 (the head's state rows hold the shape at a stride
 * of 157).  Everything else, the workspace included, is as for pmce_smpl_forward, whose pose kernel shares its body with this one. */
int pmce_smpl_forward_rotmat(const float* v_template_t, const float* dirs_t, const float* weights_t, const float* j_template,
                             const float* j_shapedirs, const int* parents_host, int n_joints, const float* rotmats,
                             const float* betas, int betas_stride, const float* trans, const int* sample_index, int n, float scale,
                             const float* offset, float* verts_out, float* joints_out, void* workspace, size_t workspace_bytes, int B,
                             int V, pmce_stream_t stream);
/* The layer's inverse: the SMPL pose, shape and translation nearest to meshes of SMPL's topology (csrc/smpl_fit.hip; the reference has no
 * such function, the algorithm is this project's and tests/smpl_fit_ref.py restates it).  On the GLOBAL rotations G_j the layer is
 * linear, v = trans + J_0 + sum_j G_j m_j; a sweep updates G_0..G_23 in index order, each by an orthogonal Procrustes step on the
 * current residual (3 x 3 SVD in fp64), then solves (betas, trans) by least squares through the 13 x 13 normal equations (fp64, Cholesky).
 * One launch on `stream`, one workgroup per sample, no atomics, no synchronisation; a sample's result does not depend on the batch it
 * is in.
 *   model tables as for pmce_smpl_forward, and subtree_weights_t[24][V]: row c = the sum of weights_t over the subtree of c (c included);
 *   verts[B][V][3]: the meshes, metres.  V in 1..pmce_smpl_fit_max_verts(): a sample's residual (12 V bytes) is kept in LDS;
 *   init_rotmats[B][24][3][3] (local, row-major), init_betas[B][10], init_trans[B][3]: the start, each or NULL - the cold start is the
 *     identity, zeros and mean(verts[b]) - mean(v_template);  fit_shape = 0 leaves the betas what they start as and solves trans alone;
 *   n_sweeps >= 1;  sample_index[n] or NULL (then n == B) as for pmce_smpl_forward: the rows this call fits, in place;
 *   rotmats[B][24][3][3] (local rotations), pose[B][72] (their axis-angle form by the rule of lib/geometry.py:84-249, as the HMR head's
 *     theta), betas[B][10], trans[B][3], residual[B] = mean_v |verts - layer(rotmats, betas, trans)| after the last sweep,
 *     history[B][n_sweeps] or NULL: the same after every sweep;
 *   status[B] (int32): PMCE_SMPL_FIT_DEGENERATE_JOINT - some step met sigma_1 == 0, sigma_2 <= 1e-6 sigma_1 or a non-finite sum and kept
 *     that joint's rotation; PMCE_SMPL_FIT_SINGULAR_SHAPE - a pivot of the factorisation was <= 0 or non-finite and that sweep kept
 *     (betas, trans); PMCE_SMPL_FIT_NONFINITE - verts[b] holds a non-finite number: the row's results are the identity, zeros, zeros,
 *     residual and history +inf;
 *   workspace: 16-byte aligned device memory of at least pmce_smpl_fit_workspace_bytes(B, V) bytes (rows indexed by sample).
 * The query returns 0 (and sets the error string) for B < 1 or V outside 1..pmce_smpl_fit_max_verts(). */
#define PMCE_SMPL_FIT_DEGENERATE_JOINT 1
#define PMCE_SMPL_FIT_SINGULAR_SHAPE 2
#define PMCE_SMPL_FIT_NONFINITE 4
int pmce_smpl_fit_max_verts(void);
size_t pmce_smpl_fit_workspace_bytes(int B, int V);
int pmce_smpl_fit(const float* v_template_t, const float* dirs_t, const float* weights_t, const float* subtree_weights_t,
                  const float* j_template, const float* j_shapedirs, const int* parents_host, int n_joints, const float* verts,
                  const float* init_rotmats, const float* init_betas, const float* init_trans, const int* sample_index, int n,
                  int n_sweeps, int fit_shape, float* rotmats, float* pose, float* betas, float* trans, float* residual, int* status,
                  float* history, void* workspace, size_t workspace_bytes, int B, int V, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's person crops (lib/utils/_dataset_demo.py:29-75 CropDataset) from frames that are already on the device.
 *
 * pmce_crop_boxes: keypoints[N][K][3] = (x, y, score), fp32, N >= 1 frames of one tracklet -> the box CropDataset crops each frame with,
 * computed and returned in fp64.  A frame is usable when some score exceeds vis_thresh and (max - min) of those keypoints has Euclidean
 * length >= 0.5 (lib/utils/smooth_bbox.py:36-59); it gets centre = (min + max) / 2 and scale = 150 / length.  An unusable frame between
 * two usable ones gets each of (cx, cy, scale) as np.linspace(prev, curr, n + 2)[1:-1] gives it: prev + k * ((curr - prev) / (n + 1)).
 *   boxes[N][4] (fp64) = (cx, cy, s, s), s = 150 / scale (the reference's second division, :49-50); NaN outside the span;
 *   usable[N] (int32); span[2] (int32) = (first usable frame, last usable frame + 1): the reference's [time_pt1:time_pt2]; (-1, 0) when
 *   no frame is usable.  One launch on `stream`, one wavefront per frame, no host wait.
 *
 * pmce_crop_patches: job n crops frames[frame_index[n]] (frames[n_frames][height][width][3], uint8) around boxes[n] = (cx, cy, w, h)
 * (fp64) to a side x side patch, side in 1..1024, width and height <= 16384.  The map is gen_trans_from_patch_cv's with rot = 0
 * (lib/utils/_img_utils.py:53-86), per axis and in fp64:
 *     c0 = f32(cx), half = f32(w * scale * 0.5), d = f32(cx + half) - c0, i = d / (side / 2), t = c0 - (side / 2) * i,  x_src = i x_dst + t.
 * Sampling is the fixed-point bilinear rule of cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) on 8-bit images: with rint = round half to
 * even, X = (rint(t_x * 1024) + 16 + rint(i_x * x * 1024)) >> 5 and Y = (rint((i_y * y + t_y) * 1024) + 16) >> 5 (arithmetic shifts), the
 * taps are columns X >> 5, (X >> 5) + 1 and rows Y >> 5, (Y >> 5) + 1 with fractions a = X & 31, b = Y & 31 and the integer weights
 * (32 - b)(32 - a) 32, (32 - b) a 32, b (32 - a) 32, b a 32; a tap outside the frame contributes 0; pixel = (sum + 16384) >> 15.
 *   norm_table[3][256] (device, fp32): the value output channel c takes for byte v - the caller builds ((v / 255) - mean[c]) / std[c]
 *     with the very fp32 operations it wants reproduced (pmce_amd.crops: torch's, on the CPU);
 *   swap_rb != 0: output channel c is the frame's byte 2 - c (BGR frames, RGB patches);
 *   patch_f32[N][3][side][side]; patch_u8[N][side][side][3] or NULL: the bytes before normalisation (the reference's raw_image);
 *   status[N] (int32): 0 fine; 1 the box is not finite or w * scale <= 0 or h * scale <= 0; 2 the map's source coordinates leave
 *     +-2^20 px (OpenCV's saturation is not reproduced); 3 frame_index[n] outside [0, n_frames) in a device table.  A job with status != 0
 *     gets the all-border patch (byte 0) and reads no frame;
 *   frame_index is given twice: frame_index_host (may be NULL: a table that exists only on the device is trusted) is validated here, an
 *     entry outside [0, n_frames) is PMCE_ERR_ARG; frame_index is the same table in device memory.
 * One launch, no atomics, integer arithmetic after the map: bit-identical from run to run and whatever N. */
int pmce_crop_boxes(const float* keypoints, int N, int K, double vis_thresh, double* boxes, int* usable, int* span, pmce_stream_t stream);
int pmce_crop_patches(const unsigned char* frames, int n_frames, int height, int width, const int* frame_index_host,
                      const int* frame_index, const double* boxes, int n_jobs, double scale, int side, int swap_rb,
                      const float* norm_table, float* patch_f32, unsigned char* patch_u8, int* status, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's 2D pose stage around the network (main/run_demo.py:264-286: inference_top_down_pose_model with the config
 * pose_detector/ViTPose_huge_coco_256x192.py): boxes to patches before pmce_vitpose_forward, heatmaps to keypoints after it
 * (csrc/pose2d.hip).  The formulas are written from mmpose 0.x's published text (TopDownAffine with use_udp, TopDown.forward_test,
 * keypoints_from_heatmaps with post_process='default', use_udp, kernel 11) and OpenCV's documented warpAffine rule; no value was
 * recorded from either.  f32(.) rounds to fp32, everything else is fp64.
 *
 * pmce_pose_patches: job n warps frames[frame_index[n]] (uint8 [n_frames][height][width][3]) around boxes[n] (fp64: (x, y, w, h) with
 * a top-left corner, or (cx, cy, w, h) when centred != 0: x = cx - 0.5 w, y = cy - 0.5 h) to a patch_h x patch_w patch, both in 2..1024.
 *   _box2cs: a = patch_w / patch_h; cx = f32(x + 0.5 w), cy = f32(y + 0.5 h); if w > a h: h = w / a, else if w < a h: w = h a;
 *     sx = f32(f32(w / 200) * f32(padding)), wt = f32(sx * 200f); sy, ht likewise from h.  centre_scale[n] = (cx, cy, wt, ht), fp32.
 *   The UDP map per axis (x shown): k = (patch_w - 1) / (double)wt, m00 = f32(k), m02 = f32(k * (double)f32(0.5f wt - cx)); inverted
 *     as OpenCV does: D = 1 / (m00 m11), ix = m11 D, iy = m00 D, tx = -ix m02, ty = -iy m12; x_src = ix x_dst + tx.
 *   From (ix, tx, iy, ty) on, the sampling, norm_table and swap_rb are those of pmce_crop_patches above.
 *   patch_f32[N][3][patch_h][patch_w]; patch_u8[N][patch_h][patch_w][3] or NULL.  mirror != 0: both hold 2 N patches, row N + n is
 *     row n mirrored in x (what the flip test feeds the network).
 *   status[N]: 0 fine; 1 the box is not finite or w <= 0 or h <= 0 (centre_scale[n] is then 0); 2 the source coordinates leave
 *     +-2^20 px (or the map is not finite); 3 frame_index[n] outside [0, n_frames) in a device table.  A job with status != 0 gets the
 *     all-border patch and reads no frame.  frame_index_host as for pmce_crop_patches.
 * One launch, no host wait, integer arithmetic after the map: bit-identical from run to run and whatever N.
 *
 * pmce_pose_decode: heatmaps heat[n][K][heat_h][heat_w] read through the element strides (sn, sk, sy, sx) - the network's NHWC
 * storage as it is - to keypoints[n][K][3] = (x, y, score) in image pixels.  K in 1..64, heat_h and heat_w in 6..4096.
 *   flip test: with heat_flipped (strides fn, fk, fy, fx; the network's heatmaps of the mirrored patches) and perm_host[K] (the
 *     flip pairs as a permutation, host memory), A[k][y][x] = f32(f32(h[k][y][x] + hf[perm[k]][y][heat_w - 1 - x]) * 0.5f); else A = h.
 *   maximum: score = max A[k], (px, py) its first position in row-major order.  score <= 0: the heatmap coordinates are (-1, -1) and
 *     are not refined (mmpose refines them at an index outside the map; that read is not reproduced).
 *   DARK (post_dark_udp, kernel 11): blur_host[11] (host memory) = f32(e_i / sum e), e_i = exp(-(i - 5)^2 / 8); B = g (x) g on A with
 *     BORDER_REFLECT_101, horizontal pass first, taps in ascending order, fp32; L = f32(log(min(max(B, 0.001f), 50f))) (the
 *     logarithm correctly rounded: taken in fp64), extended by edge replication; at (px, py) in
 *     fp32 dx = 0.5 (L[x+1] - L[x-1]), dxx = L[x+1] - 2 L + L[x-1], dy, dyy likewise, dxy = 0.5 (L[x+1,y+1] - L[x+1,y] - L[x,y+1] + L + L
 *     - L[x-1,y] - L[x,y-1] + L[x-1,y-1]); (ox, oy) = (Hess + 2^-23 I)^-1 (dx, dy) in fp64; hx = f32(px - ox), hy = f32(py - oy).
 *   transform_preds: x = f32(f32(f32(hx * f32(wt / (heat_w - 1))) + cx) - f32(0.5f wt)), y likewise, from centre_scale[n][4].
 *   status[n] (device, may be NULL) != 0: the image's keypoints are (0, 0, 0).
 *   coords[n][K][2] (fp32, may be NULL): (hx, hy); argmax[n][K][2] (int32, may be NULL): (px, py), (-1, -1) where score <= 0.
 * One launch, one workgroup per image, no atomics, no host wait: bit-identical from run to run and whatever n. */
int pmce_pose_patches(const unsigned char* frames, int n_frames, int height, int width, const int* frame_index_host,
                      const int* frame_index, const double* boxes, int n_jobs, int centred, double padding, int patch_h, int patch_w,
                      int swap_rb, int mirror, const float* norm_table, float* patch_f32, unsigned char* patch_u8, float* centre_scale,
                      int* status, pmce_stream_t stream);
int pmce_pose_decode(const float* heat, long long sn, long long sk, long long sy, long long sx, const float* heat_flipped,
                     long long fn, long long fk, long long fy, long long fx, int n, int K, int heat_h, int heat_w, const int* perm_host,
                     const float* blur_host, const float* centre_scale, const int* status, float* keypoints, float* coords,
                     int* argmax, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's feature extractor (reference lib/models/spin.py:18-143: Bottleneck, the HMR backbone, HMR.feature_extractor, called at
 * main/run_demo.py:247-252,315): convolutions on the f16 matrix pipe as three products of the exact two-term split, fp32 operands and
 * results, NHWC between the layers (csrc/conv.hip, csrc/extractor.cpp).
 *
 * pmce_conv_packed_floats: floats of storage of a packed weight = ceil(Cout / 64) * 64 * Kp, Kp = KH KW Cin rounded up to 32; 0 (and the
 *   error string) for a bad shape.
 * pmce_conv_pack_split_f16: W_oihw[Cout][Cin][KH][KW] fp32 (BatchNorm already folded) -> Wp = the blocked planes
 *   [ceil(Cout / 64)][Kp / 16][64][16 hi | 16 lo] f16 of W[n] * 2^s(n) with k = (ky, kx, cin), zero weights for k >= KH KW Cin and for the
 *   rows past Cout, and wscale[Cout] = 2^-s(n): one power of two per output channel, chosen as pmce_gemm_pack_split_f16 chooses it.
 * pmce_conv2d_split_f16: out[m][co] = relu?( wscale[co] * sum_k (xhi whi + xhi wlo + xlo whi) + bias[co] + R[m][co]? ), m = (image, oy, ox),
 *   OH = (H + 2 pad - KH) / stride + 1 (OW likewise); out and R are dense NHWC [n][OH][OW][Cout]; bias and R may be NULL.
 *   The input element (image i, channel c, row y, column x) is x[i sn + c sc + y sy + x sx] (element strides): NCHW and NHWC alike.  With
 *   sc == 1, Cin % 16 == 0 and sn, sy, sx multiples of 4 the gather is 16-byte loads; any other input takes the element-wise gather.
 *   Zero padding is a predicate of the load.  Activations are split while they are staged: a value that is not finite, or whose f16
 *   part is not (|x| > 65504), makes every output that reads it inf / NaN and no other; the ReLU keeps a NaN.  An output element's
 *   order of summation depends on nothing but its k index: results are bit-identical whatever n is.
 * pmce_maxpool3x3s2_nhwc_f32: nn.MaxPool2d(3, 2, 1) on x[n][H][W][C] -> y[n][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]; C % 4 == 0; the padding
 *   never wins, a NaN in the window is the result.
 * pmce_avgpool_nhwc_f32: y[n][C] = the mean of x[n][HW][C] over HW: one fp64 sum per element in pixel order, rounded once.
 * One launch each on `stream`, no atomics, no synchronisation.
 *
 * pmce_extractor: the [3, 4, 6, 3] bottleneck network (53 convolutions, the max pool, the average pool).  The handle owns the packed
 * weights (one hipMalloc in finalize); the caller owns everything else.
 *   pmce_extractor_conv_count / _conv_name / _conv_shape (Cout, Cin, KH, KW): the convolutions in the order of the forward, named as the
 *     reference's state dict names them ("conv1", "layer2.0.conv3", "layer3.0.downsample.0", ...);
 *   pmce_extractor_set_conv: the folded OIHW weight and the folded bias [Cout] of one convolution (device, fp32); they must stay valid
 *     until finalize returns;
 *   pmce_extractor_finalize_on: packs every convolution on `stream` and waits for it (the one call here that synchronises);
 *     PMCE_ERR_ARG names a convolution that was not set;
 *   pmce_extractor_workspace_bytes(n): 16-byte aligned device memory a forward of n patches needs (0 and the error string for n outside
 *     1..4096): three buffers of 112 * 112 * 64 and two of 56 * 56 * 128 floats per patch;
 *   pmce_extractor_forward: patches [n][3][224][224] through the element strides (sn, sc, sy, sx) -> feats[n][2048]; tap1..tap4, each
 *     optional, receive the outputs of layer1..layer4 as NHWC [n][56][56][256], [n][28][28][512], [n][14][14][1024], [n][7][7][2048].
 *     56 launches (and a copy per tap) on `stream`, no synchronisation; patch i's result does not depend on n. */
typedef struct pmce_extractor pmce_extractor;
long long pmce_conv_packed_floats(int Cout, int Cin, int KH, int KW);
int pmce_conv_pack_split_f16(const float* W_oihw, int Cout, int Cin, int KH, int KW, float* Wp, float* wscale, pmce_stream_t stream);
int pmce_conv2d_split_f16(const float* x, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H, int W,
                          const float* Wp, const float* wscale, const float* bias, const float* R, float* out, int Cout, int KH, int KW,
                          int stride, int pad, int relu, pmce_stream_t stream);
int pmce_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n, int H, int W, int C, pmce_stream_t stream);
int pmce_avgpool_nhwc_f32(const float* x, float* y, int n, int HW, int C, pmce_stream_t stream);
int pmce_extractor_create(pmce_extractor** out);
void pmce_extractor_destroy(pmce_extractor* e);
int pmce_extractor_conv_count(const pmce_extractor* e);
const char* pmce_extractor_conv_name(const pmce_extractor* e, int i);
int pmce_extractor_conv_shape(const pmce_extractor* e, int i, int* shape4);
int pmce_extractor_set_conv(pmce_extractor* e, const char* name, const float* folded_weight, const float* folded_bias);
int pmce_extractor_finalize_on(pmce_extractor* e, pmce_stream_t stream);
size_t pmce_extractor_workspace_bytes(int n);
int pmce_extractor_forward(const pmce_extractor* e, const float* patches, long long sn, long long sc, long long sy, long long sx,
                           float* feats, int n, float* tap1, float* tap2, float* tap3, float* tap4, void* workspace,
                           size_t workspace_bytes, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * SPIN's regression head (reference lib/models/spin.py:145-208 after the backbone = Regressor.forward :211-293, eval mode): features ->
 * the state (6D pose 144, shape 10, camera 3), rotation matrices, theta; then the 49 joints and their projection.
 *
 * pmce_hmr_head_f32: in eval mode n_iter iterations of fc1, fc2, decpose | decshape | deccam are one affine map of the initial state,
 *     state = Q features + cst [+ P init]      (pmce_amd.hmr.fold_regressor: Q [157][2048], P [157][157], c_n, fp64 rounded to fp32 once).
 *   features[n][2048]; q_t[2048][160] = Q transposed, each row padded with three zeros; cst[157] = c_n, or P s_0 + c_n when every sample
 *   starts from the same state; pmi_t[157][160] = (P - I) transposed and padded + init[n][157] (both or neither): per-sample initial
 *   states, computed as init + (cst + Q features + (P - I) init) - P is the identity plus a small correction, and the correction summed
 *   on its own loses less than 157 terms summed at the magnitude of the state.
 *   Outputs: state[n][157]; rotmat[n][24][3][3] = rot6d_to_rotmat of the state's first 144 numbers (lib/geometry.py:346-360: of each six
 *   a1 = elements 0, 2, 4 and a2 = elements 1, 3, 5, each normalised by max(norm, 1e-6), the vectors are the columns);
 *   theta[n][85] = (camera 3, rotation_matrix_to_angle_axis 72, shape 10) with geometry.py:84-249's four-branch quaternion (eps = 1e-6 on
 *   R22, R00 > R11, R00 < -R11), atan2 with the sign flip, k = 2 where sin^2 = 0, and NaN -> 0.
 *   One launch on `stream`, a batch tile of pmce_hmr_head_batch_tile() = 16 samples per workgroup, plain fp32 multiply-adds in a fixed
 *   order: a sample's result depends on its own row only and has the same bits whatever n and wherever it sits; with q_t = 0, P = I
 *   (pmi_t = 0), cst = 0 the state is `init` to the bit.  No atomics, no host wait.
 *
 * pmce_hmr_joints_f32: kp_3d[s][k] = joints[s][sel[k]] where sel[k] >= 0 (a posed SMPL joint, < 24), else row k of the CSR matrix
 *   (indptr[K + 1], indices, data; columns in [0, V)) times verts[s][V][3]; kp_2d[s][k] = 5000 (p.xy / p.z) / 112 with
 *   p = kp_3d + (cam1, cam2, 2 * 5000 / (224 cam0 + 1e-9)) (spin.py:309-353), cam read at cam[s * cam_stride + 0..2].
 *   joints[n][24][3], kp_3d[n][K][3], kp_2d[n][K][2], K in 1..256; sel, indptr, indices, data on the device.  One wave per sample.
 * Both return PMCE_ERR_ARG and set the error string for n < 1, a null pointer, P without init (or init without P), K out of range. */
int pmce_hmr_head_batch_tile(void);
int pmce_hmr_head_f32(const float* features, const float* q_t, const float* cst, const float* pmi_t, const float* init, int n,
                      float* state, float* rotmat, float* theta, pmce_stream_t stream);
int pmce_hmr_joints_f32(const float* joints, const float* verts, const int* sel, const int* indptr, const int* indices,
                        const float* data, const float* cam, int cam_stride, int n, int K, int V, float* kp_3d, float* kp_2d,
                        pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's 2D pose network, ViTPose (a ViT backbone + TopdownHeatmapSimpleHead; hyper-parameters of the reference's config
 * pose_detector/ViTPose_huge_coco_256x192.py): normalised person patches -> keypoint heatmaps (csrc/vit_attention.hip,
 * csrc/layernorm_rows.hip, csrc/deconv_gather.hip, csrc/vitpose.cpp).  Every nn.Linear is pmce_gemm_nt_split_f16, the patch
 * embedding pmce_conv2d_split_f16.
 *
 * pmce_vit_attention_split_f16: softmax(q k^T hd^-0.5) v per head on qkv[n N][3 C] fp32 (a row = q | k | v, each (heads, hd), as the
 *   qkv product writes it) -> out_planes[n N][C/16][16 hi | 16 lo*2^11] f16 in the bytes of an fp32 [n N][C], the A operand of proj.
 *   n images of N tokens, N in 1..192, hd = C / heads = 64 or 80 (pmce_vit_attention_supported tells; anything else PMCE_ERR_ARG).
 *   The three-product form on the f16 matrix pipe, fp32 accumulation, the exact two-pass softmax on the hardware 2^x; one workgroup
 *   per (image, head).  Keys at or beyond N are masked to -inf; no row outside [image N, image N + N) is read for an image.  A result
 *   row depends only on its own image: the same bits whatever n is and wherever the image sits.  A non-finite result sets the
 *   calling thread's overflow sink.  Buffers 16-byte aligned.
 * pmce_layernorm_rows_f32: y = x + add[row % add_mod] (add NULL: y = x); out1 = y (optional; may be x);
 *   out = LayerNorm(y; w, b, eps) as fp32 [rows][C] or, out_split != 0, as planes.  C % 16 == 0, C <= 2048, any rows >= 1;
 *   two-pass fp32 mean and (biased) variance, one wave per row.  A row whose variance overflows fp32 is NaN, not b.
 * pmce_deconv4x4s2_gather_f32: the gather half of ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + BatchNorm + ReLU.  With
 *   Y[n H W][16 Cout] = X[n H W][Cin] W'^T, W'[(ky, kx, co)][ci] = W[ci][co][ky][kx] s[co] (one pmce_gemm_nt_split_f16 on the packed W'),
 *   out[n][oy][ox][co] = relu(sum Y[n][iy][ix][(ky, kx, co)] + bias[co]) over the pairs with oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx, summed
 *   ky ascending, then kx ascending, the bias last; NHWC [n][2H][2W][Cout] fp32 or planes (out_split).  Cout % 16 == 0.  No atomics.
 *
 * pmce_vitpose: the network.  The handle owns the packed weights (one hipMalloc in finalize); the caller owns everything else.
 *   pmce_vitpose_create(H, W, C, depth, heads, F1, F2, K): image H x W in whole 16 x 16 patches, N = (H/16)(W/16) <= 192 tokens;
 *     C % 32 == 0; C / heads = 64 or 80; depth >= 1; F1, F2 % 32 == 0 (the deconvolutions' filters); K in 1..64 keypoints;
 *     PMCE_ERR_ARG names the offending value.
 *   pmce_vitpose_tensor_count / _tensor_name / _tensor_shape (fills shape4, returns the rank or a negative error): the tensors the
 *     handle reads, under their state-dict names, all fp32 on the device and 16-byte aligned.  Three of them are prepared by the
 *     host: "backbone.pos_embed" is the [N][C] table pos_embed[1:] + pos_embed[:1]; "keypoint_head.deconv_layers.{0,3}.weight" are
 *     the product forms W' [16 Cout][Cin] above (BatchNorm scale folded in fp64, rounded once) and
 *     "keypoint_head.deconv_layers.{1,4}.bias" the folded BatchNorm biases beta - mean s; "keypoint_head.final_layer.weight" is [K][F2].
 *   pmce_vitpose_set_tensor: one tensor; it must stay valid until finalize returns.
 *   pmce_vitpose_finalize_on: packs every matrix with pmce_gemm_pack_split_f16(blocked = 1) / pmce_conv_pack_split_f16 on `stream`
 *     and waits for it (the one call here that synchronises); PMCE_ERR_ARG names a tensor that was not set.
 *   pmce_vitpose_workspace_bytes(v, n): 16-byte aligned device memory a forward of n patches needs, n in 1..256 (0 and the error
 *     string otherwise; the second deconvolution's product result [768 n][16 F2] must stay below the product's 4 GiB operand limit).
 *   pmce_vitpose_forward: patches [n][3][H][W] through the element strides (sn, sc, sy, sx) -> heat NHWC [n][4 H/16][4 W/16][K];
 *     feat (optional) NHWC [n][H/16][W/16][C], the backbone's map after last_norm.  Per block: LayerNorm (planes), qkv product,
 *     attention (planes), proj with the residual, LayerNorm (planes), fc1 with GELU and a pre-split result, fc2 with the residual -
 *     seven launches; block 0's first LayerNorm also adds the position table.  Then last_norm, product + gather twice, the final
 *     product.  No synchronisation; patch i's result does not depend on n. */
typedef struct pmce_vitpose pmce_vitpose;
int pmce_vit_attention_supported(int N, int C, int heads);
int pmce_vit_attention_split_f16(const float* qkv, float* out_planes, int n, int N, int C, int heads, pmce_stream_t stream);
int pmce_layernorm_rows_f32(const float* x, long long rows, int C, const float* add, int add_mod, float* out1, const float* w,
                            const float* b, float eps, float* out, int out_split, pmce_stream_t stream);
int pmce_deconv4x4s2_gather_f32(const float* Y, const float* bias, float* out, int n, int H, int W, int Cout, int out_split,
                                pmce_stream_t stream);
int pmce_vitpose_create(int H, int W, int C, int depth, int heads, int F1, int F2, int K, pmce_vitpose** out);
void pmce_vitpose_destroy(pmce_vitpose* v);
int pmce_vitpose_tensor_count(const pmce_vitpose* v);
const char* pmce_vitpose_tensor_name(const pmce_vitpose* v, int i);
int pmce_vitpose_tensor_shape(const pmce_vitpose* v, int i, int* shape4);
int pmce_vitpose_set_tensor(pmce_vitpose* v, const char* name, const float* dev_ptr);
int pmce_vitpose_finalize_on(pmce_vitpose* v, pmce_stream_t stream);
size_t pmce_vitpose_workspace_bytes(const pmce_vitpose* v, int n);
int pmce_vitpose_forward(const pmce_vitpose* v, const float* patches, long long sn, long long sc, long long sy, long long sx, int n,
                         float* heat, float* feat, void* workspace, size_t workspace_bytes, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * ViTPose's opt-in single-product f16 mode (csrc/gemm_f16.hip, csrc/vit_attention.hip, csrc/layernorm_rows.hip): the four products
 * and the attention of every block as ONE f16 matrix product with fp32 accumulation, the operands between them stored as single f16.
 * r16(x) is round-to-nearest-even to f16 with every |x| < 2^-14 set to zero: every operand is rounded by it, none relies on f16
 * sub-normals.  The default mode's entries above keep their bits.
 *
 * pmce_gemm_pack_f16: W[N][ldw] fp32 -> W16 = r16(W[n] * 2^s(n)) as f16 in the blocked layout [ceil(N/64)][K/32][64][32]
 *   (pmce_gemm_packed_f16_halves(N, K) f16 of storage; rows past N are not written) and wscale[N] = 2^-s(n), the per-row power of two
 *   that pmce_gemm_pack_split_f16 chooses (the row's max |w| lifted into [2^14, 2^15)).  K % 32 == 0, ldw >= K.
 * pmce_gemm_nt_f16: C[M][N] = epi(A16[M][K] . W16[N][K]^T): A16 f16 [M][lda] (lda % 8 == 0), W16 / wscale from pmce_gemm_pack_f16,
 *   bias fp32 [N] or NULL, act 0 or 1 (exact GELU), R an optional fp32 residual [M][ldc] that MAY BE C itself, C fp32 [M][ldc] or
 *   (c_f16 = 1, no residual then) f16 [M][ldc] = r16 of the fp32 result.  K % 32 == 0, N % 32 == 0, any M >= 1; rows past M and columns
 *   past N are never read past the tensors and never stored.  v_mfma_f32_32x32x16_f16 with fp32 accumulators, k ascending; the epilogue
 *   (scale by 2^-s, bias, GELU, residual) in fp32.  A row of C has the same bits whatever M is and wherever the row sits.  A non-finite
 *   result, or an f16 result beyond 65504, sets *overflow_word (NULL: the calling thread's overflow sink) to 1.  Buffers 16-byte
 *   aligned; PMCE_ERR_ARG names the offending value.
 * pmce_gemm_f16_set_tuning (a process-wide TUNING AID like pmce_gemm_split_set_tuning): tile 0 = 128x256, 1 = 128x128, 2 = 64x128,
 *   anything else automatic; max_workgroups > 0 caps the persistent grid.  Results do not depend on either.
 * pmce_layernorm_rows_f16: pmce_layernorm_rows_f32's arithmetic, the result stored as r16(y), f16 [rows][C].  It does not touch the
 *   overflow word: a y beyond 65504 is stored as infinity and reported by the product that reads it.
 * pmce_vit_attention_f16: pmce_vit_attention_split_f16's kernel without the lo planes - its input, work split, bounds and shapes
 *   (pmce_vit_attention_supported answers for both); q, k, v rounded by r16, s = q.k hd^-0.5 in one accumulator, p~ = exp(s - max), out = (r16(p~) . r16(v)) / sum(p~) with
 *   the sum over the unrounded fp32 p~, stored as r16, f16 [n N][C].
 * pmce_vitpose_create_precision: pmce_vitpose_create with `precision` 0 (split, what pmce_vitpose_create passes) or 1 (f16; anything
 *   else PMCE_ERR_ARG naming the value).  The tensor table is the same in both.  In f16 mode the 4 x depth block weights are packed by
 *   pmce_gemm_pack_f16 (2 bytes per weight instead of 4) and pmce_vitpose_forward runs the same seven launches per block through the
 *   f16 entries; the patch embedding, the LayerNorm statistics, the fp32 residual stream, qkv's fp32 result, last_norm and the whole
 *   head are the default mode's.  pmce_vitpose_workspace_bytes is the same bound in both.  pmce_vitpose_precision reads the mode back
 *   (-1 for NULL). */
long long pmce_gemm_packed_f16_halves(int N, int K);
int pmce_gemm_pack_f16(const float* W, int N, int K, int ldw, void* W16, float* wscale, pmce_stream_t stream);
int pmce_gemm_nt_f16(const void* A16, const void* W16, const float* wscale, const float* bias, const float* R, void* C, int M, int N, int K,
                     long long lda, long long ldc, int act, int c_f16, unsigned* overflow_word, pmce_stream_t stream);
int pmce_gemm_f16_set_tuning(int tile, int max_workgroups);
int pmce_layernorm_rows_f16(const float* x, long long rows, int C, const float* add, int add_mod, float* out1, const float* w,
                            const float* b, float eps, void* out16, pmce_stream_t stream);
int pmce_vit_attention_f16(const float* qkv, void* out16, int n, int N, int C, int heads, pmce_stream_t stream);
int pmce_vitpose_create_precision(int H, int W, int C, int depth, int heads, int F1, int F2, int K, int precision, pmce_vitpose** out);
int pmce_vitpose_precision(const pmce_vitpose* v);

/* ---------------------------------------------------------------------------------------------------------
 * The feature extractor's single-product f16 mode (FeatureExtractor(..., precision="f16"); csrc/conv_f16.hpp, compiled with csrc/conv.hip):
 * the convolution with ONE f16 product per k-tile, fp32 accumulation, f16 maps between the layers.  Opt-in; the default mode keeps its bits.
 *
 * pmce_conv_packed_halves: f16 of storage of a packed weight = ceil(Cout / 64) * 64 * Kp, Kp = KH KW Cin rounded up to 64; 0 (and the
 *   error string) for a bad shape.
 * pmce_conv_pack_f16: W_oihw[Cout][Cin][KH][KW] fp32 (BatchNorm folded) -> Wp = the blocked layout [ceil(Cout / 64)][Kp / 32][64][32] f16 of
 *   r16(W[n] * 2^s(n)), k = (ky, kx, cin), zeros for k >= KH KW Cin and for the rows past Cout; wscale[Cout] = 2^-s(n) as
 *   pmce_conv_pack_split_f16 chooses it.  r16: round to nearest even, |x| < 2^-14 -> 0, beyond f16's range -> inf.
 * pmce_conv2d_act_f16: v = wscale[co] * sum_k a16[m][k] w16[co][k] + bias[co]; res_after_act == 0: y = act(v + R), 1: y = act(v) + R
 *   (act = 0 none, 1 ReLU, 2 leaky with slope in [0, 1]); out = y (out_dtype 0: fp32, pitch in floats) or r16(y) (out_dtype 1: f16, pitch
 *   in halves).  Every epilogue step is one fp32 rounding: the f16 result is r16 of the fp32 result, to the bit.
 *   x_dtype 1: f16 input taken as it is, x_dtype 0: fp32 input, each value rounded by r16 in the gather; both through the four element
 *   strides.  R (may be NULL) is f16, row m at R + m * res_pitch halves.  Pitches in Cout..2^24, M = n OH OW < 2^30, offsets < 2^40.
 *   No alignment is required: an f16 input with sc == 1, Cin % 32 == 0, sn, sy, sx multiples of 8 and a 16-byte aligned base is gathered
 *   by 16-byte loads, every other by element loads - to the same bits.  A result that is not finite (as f16 where f16 is written: a
 *   finite fp32 beyond 65504 becomes inf) is reported to the calling thread's overflow sink.  One accumulator per output element takes
 *   the k-tiles in order: bit-identical whatever n is.
 * pmce_maxpool3x3s2_nhwc_f16 / pmce_avgpool_nhwc_f16_f32 / pmce_upsample2x_nhwc_f16: the fp32 operators' rules on f16 maps (C and the
 *   pitches % 4 == 0, 8-byte aligned pointers for the pool and the upsample); the max and the copy are exact, the average is one fp64 sum
 *   in pixel order rounded once to fp32.  pmce_widen_f16_f32: y[i] = (float)x[i], exact.
 * pmce_extractor_create_precision: precision 0 (split_f16, what pmce_extractor_create passes) or 1 (f16; anything else PMCE_ERR_ARG naming
 *   the value).  In f16 mode the weights are packed by pmce_conv_pack_f16 (2 bytes per weight), every map between the layers is f16 and
 *   pmce_extractor_workspace_bytes_for(e, n) is half of the default's; the features and the taps stay fp32 (the taps widened exactly).
 *   pmce_extractor_precision reads the mode back (-1 for NULL). */
long long pmce_conv_packed_halves(int Cout, int Cin, int KH, int KW);
int pmce_conv_pack_f16(const float* W_oihw, int Cout, int Cin, int KH, int KW, void* Wp, float* wscale, pmce_stream_t stream);
int pmce_conv2d_act_f16(const void* x, int x_dtype, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H, int W,
                        const void* Wp, const float* wscale, const float* bias, const void* R, long long res_pitch, void* out,
                        long long out_pitch, int out_dtype, int Cout, int KH, int KW, int stride, int pad, int act, float slope,
                        int res_after_act, pmce_stream_t stream);
int pmce_maxpool3x3s2_nhwc_f16(const void* x, void* y, int n, int H, int W, int C, pmce_stream_t stream);
int pmce_avgpool_nhwc_f16_f32(const void* x, float* y, int n, int HW, int C, pmce_stream_t stream);
int pmce_upsample2x_nhwc_f16(const void* x, long long in_pitch, void* out, long long out_pitch, int n, int H, int W, int C,
                             pmce_stream_t stream);
int pmce_widen_f16_f32(const void* x, float* y, long long count, pmce_stream_t stream);
int pmce_extractor_create_precision(int precision, pmce_extractor** out);
int pmce_extractor_precision(const pmce_extractor* e);
size_t pmce_extractor_workspace_bytes_for(const pmce_extractor* e, int n);

/* ---------------------------------------------------------------------------------------------------------
 * The tracker's detector: YOLOv3 as the reference calls it (main/run_demo.py:199-215: MPT(detector_type='yolo', yolo_img_size=416)),
 * video frames -> box predictions (csrc/conv.hip, csrc/yolo.hip, csrc/yolo.cpp).  The structure is the published yolov3.cfg's and that of
 * the PyTorch-YOLOv3 lineage; no tensor was recorded from the yolov3 or multi_person_tracker packages.  Non-maximum suppression and SORT follow below
 * (csrc/tracker.hip).
 *
 * pmce_conv2d_act_split_f16: pmce_conv2d_split_f16 with
 *     v = wscale[co] * sum_k (...) + bias[co];   res_after_act == 0: out = act(v + R);   res_after_act == 1: out = act(v) + R
 *   act = 0 none, 1 ReLU, 2 leaky (v < 0 ? v * slope : v, slope in [0, 1]); row m of the result is out + m * out_pitch and of the residual
 *   R + m * res_pitch (floats; both >= Cout): a convolution writes into, and reads its residual from, a channel slice of a wider NHWC
 *   buffer.  The input is addressed by its four strides as before (a slice: sx = the pitch).  With act = 1, res_after_act = 0 and both
 *   pitches = Cout it is pmce_conv2d_split_f16 (relu = 1) to the bit - both are one launcher.  Same summation order: bit-identical whatever n.
 * pmce_upsample2x_nhwc_f32: nearest x2: out[i][2 y + dy][2 x + dx][c] = x[i][y][x][c], c < C; pixel rows of in_pitch / out_pitch floats
 *   (`out` points at the slice's first channel); C, the pitches % 4 == 0 and 16-byte aligned pointers: 16-byte accesses.
 * pmce_yolo_decode_f32: the three detection maps (NHWC [n][g_s][g_s][pitch_s], channel a (5 + nc) + c, a < 3) -> out[n][R][5 + nc],
 *   R = 3 (g_0^2 + g_1^2 + g_2^2), rows ordered scale, anchor, gy, gx.  With stride = (float)S / g, anchors_host[s][a] = (w, h) in input
 *   pixels and sigmoid, exp correctly rounded to fp32, every other operation one fp32 rounding (no contraction):
 *     x = (sigmoid(t0) + gx) * stride, y = (sigmoid(t1) + gy) * stride, w = (exp(t2) * (aw / stride)) * stride, h alike,
 *     conf = sigmoid(t4), cls_c = sigmoid(t5+c).     Boxes are (cx, cy, w, h) in pixels of the S x S input.  nc in 1..255, any g in 1..2048.
 *   pitches_host[3], grids_host[3], anchors_host[3][3][2] are host memory.  One launch, a thread per output float, no atomics.
 * pmce_letterbox_u8_f32: job j pads frames[frame_index[j]] (uint8 [n_frames][height][width][3]) to a square of side L = max(height,
 *   width) - d = |height - width|, d / 2 (rounded down) before and the rest after - and samples it at S x S as
 *   F.interpolate(mode="nearest") does: src = min((int)floorf(dst * scale), L - 1), scale = (float)L / S in fp32.
 *   out[j][c][y][x] = table[byte] (table[256], device: the caller's fp32 byte / 255) or pad_value outside the frame; swap_rb != 0: output
 *   channel c is the frame's byte 2 - c.  frame_index_host (may be NULL) is validated here; an entry of a device-only table outside
 *   [0, n_frames) gives the all-pad image and reads no frame.  One launch for all jobs.
 *
 * pmce_yolo: the network.  The handle owns the packed weights (one hipMalloc in finalize); the caller owns everything else.
 *   pmce_yolo_create: table[n_layers][9] = (kind, filters, size, stride, batch_normalize, leaky, source 0, source 1, anchor mask), one row
 *     per cfg section; kind 0 convolutional (pad = (size - 1) / 2), 1 shortcut (source 0 = the absolute index added to the layer before),
 *     2 route (absolute indices; source 1 = -1 for one source), 3 upsample (stride 2), 4 yolo (mask = bits of its three anchors).
 *     anchors18 = nine (w, h) in input pixels.  Supported: a shortcut right after the convolution it completes (out = from +
 *     act(conv): one launch); a two-source route [the upsample before it, a convolution's or shortcut's map]; three yolo layers, each
 *     after a linear convolution of 3 (5 + num_classes) filters; body convolutions with filters % 4 == 0.  PMCE_ERR_ARG names the layer.
 *   pmce_yolo_layer_plan: plan8 = (channels, input side / map side, buffer id (-1 none, -2 the caller's detection map), channel offset,
 *     pitch, buffer offset, buffer size, step of the buffer's last reader); offsets and sizes in units of n (S / 32)^2 floats.
 *   pmce_yolo_conv_shape (Cout, Cin, k, k) / pmce_yolo_set_conv: by layer index; folded OIHW weight and bias (device, fp32), valid until
 *     finalize returns.  pmce_yolo_finalize_on packs on `stream` and waits for it (the one call here that synchronises).
 *   pmce_yolo_workspace_bytes(y, n, S): n in 1..1024, S a multiple of 32 in 32..1024 (0 and the error string otherwise).
 *   pmce_yolo_forward: images [n][3][S][S] through the element strides -> map0..2 (NHWC [n][g][g][3 (5 + nc)], the raw detection maps in
 *     the order of the yolo layers) and rows[n][R][5 + nc] (NULL: no decoding).  One launch per convolution (a shortcut is an epilogue),
 *     per upsample and for the decoding, on `stream`, no synchronisation; image i's result does not depend on n. */
typedef struct pmce_yolo pmce_yolo;
int pmce_conv2d_act_split_f16(const float* x, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H, int W,
                              const float* Wp, const float* wscale, const float* bias, const float* R, long long res_pitch, float* out,
                              long long out_pitch, int Cout, int KH, int KW, int stride, int pad, int act, float slope, int res_after_act,
                              pmce_stream_t stream);
int pmce_upsample2x_nhwc_f32(const float* x, long long in_pitch, float* out, long long out_pitch, int n, int H, int W, int C,
                             pmce_stream_t stream);
int pmce_yolo_decode_f32(const float* map0, const float* map1, const float* map2, const long long* pitches_host, const int* grids_host,
                         const float* anchors_host, int n, int nc, int S, float* out, pmce_stream_t stream);
int pmce_letterbox_u8_f32(const unsigned char* frames, int n_frames, int height, int width, const int* frame_index_host,
                          const int* frame_index, int n_jobs, int S, int swap_rb, const float* table, float pad_value, float* out,
                          pmce_stream_t stream);
int pmce_yolo_create(const int* table, int n_layers, const float* anchors18, int num_classes, pmce_yolo** out);
/* pmce_yolo_create_precision: pmce_yolo_create with `precision` 0 (split_f16, what pmce_yolo_create passes) or 1 (f16; anything else
 *   PMCE_ERR_ARG naming the value).  In f16 mode the weights are packed by pmce_conv_pack_f16, every map of the workspace is f16 (the
 *   same plan, its units counted at 2 bytes: pmce_yolo_workspace_bytes is half of the default's), the stem rounds the fp32 images in its
 *   gather, shortcuts add an f16 residual and the upsample is pmce_upsample2x_nhwc_f16; the three detection maps are written in fp32 by
 *   their convolutions and decoded by pmce_yolo_decode_f32 as before.  pmce_yolo_precision reads the mode back (-1 for NULL). */
int pmce_yolo_create_precision(const int* table, int n_layers, const float* anchors18, int num_classes, int precision, pmce_yolo** out);
int pmce_yolo_precision(const pmce_yolo* y);
void pmce_yolo_destroy(pmce_yolo* y);
int pmce_yolo_layer_count(const pmce_yolo* y);
int pmce_yolo_conv_shape(const pmce_yolo* y, int i, int* shape4);
int pmce_yolo_layer_plan(const pmce_yolo* y, int i, long long* plan8);
long long pmce_yolo_workspace_units(const pmce_yolo* y);
int pmce_yolo_set_conv(pmce_yolo* y, int layer, const float* folded_weight, const float* folded_bias);
int pmce_yolo_finalize_on(pmce_yolo* y, pmce_stream_t stream);
size_t pmce_yolo_workspace_bytes(const pmce_yolo* y, int n, int S);
int pmce_yolo_forward(const pmce_yolo* y, const float* images, long long sn, long long sc, long long sy, long long sx, int n, int S,
                      float* map0, float* map1, float* map2, float* rows, void* workspace, size_t workspace_bytes, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The tracker's back half (csrc/tracker.hip): non-maximum suppression of the detector's rows, SORT over the frames of a video.  Written
 * from the published texts (the PyTorch-YOLOv3 lineage's non_max_suppression; Bewley's sort.py over filterpy's KalmanFilter formulas;
 * multi_person_tracker's run_tracker); no value was recorded from any of these packages.  tests/tracker_ref.py restates both.
 *
 * pmce_yolo_nms_f32: rows[n][R][5 + nc] = (cx, cy, w, h, conf, classes), R >= 1, nc in 1..255; one workgroup per image, one launch.
 *   fp32, one rounding per operation (no contraction), per image:
 *     candidates: conf >= conf_thres;  cls_conf = max of the class columns, cls = the FIRST maximum's index;  score = conf * cls_conf;
 *     corners (cx - w/2, cy - h/2, cx + w/2, cy + h/2);  order: score descending, ties by the lower row (the project's rule);
 *     while candidates remain: head = the first; invalid = the remaining ones of the head's cls with iou(head, .) > nms_thres,
 *       iou = inter / (a + b - inter + 1e-16), inter = max(x2 - x1 + 1, 0) max(y2 - y1 + 1, 0), areas (x2 - x1 + 1)(y2 - y1 + 1);
 *       kept box = sum(conf_i box_i) / sum(conf_i) over invalid, summed in sorted order; kept row = (x1, y1, x2, y2, conf, cls_conf,
 *       cls) with the head's confidences; invalid leave, and the head leaves ALWAYS (the lineage loops forever on a head whose
 *       self-IoU is not > nms_thres); heads are raw boxes: no IoU depends on a merged box.
 *   dets[n][max_keep][7] in keep order, rows past count[i] zero; status[i] = 0, 1 (more than max_candidates candidates) or 2 (more than
 *   max_keep kept) - then count[i] = 0 and the image's rows are zero, never a part.  max_candidates in 1..2048, max_keep in 1..64.
 *   src_row (may be NULL) [n][max_keep]: the row of every kept head, -1 past the count.
 *   people (may be NULL; with people_count) [n][max_keep][5] fp64 = (x1, y1, x2, y2, score), people_count[n]: the kept rows, in keep
 *   order, with cls == class_id, score > score_thres (score = conf, or the fp32 conf * cls_conf when score_product != 0) and a box that
 *   is finite with w > 0, h > 0 after the map to the frame x * ratio - pad_x, y * ratio - pad_y, evaluated in fp64 from the fp32 values
 *   (pmce_letterbox_u8_f32's geometry; the lineage's rescale_boxes is the same map up to the rounding of its pad // 2).
 *   The same bits whatever n; no atomics; validated on the host before the launch; no host wait.
 *
 * pmce_sort_track_f64: people[F][K][5], people_count[F] (clamped to 0..K, K <= 64) -> tracks[F][max_tracks][5] = (x1, y1, x2, y2,
 *   id + 1) in report order, track_count[F], status[F] (1: a new tracker did not fit into max_tracks <= 64 and its detection was
 *   dropped).  seq_offsets (host and device, or both NULL = one sequence) [S + 1] over frames: one 64-lane wave per sequence, ids from
 *   0 per sequence.  fp64, no contraction.  State (u, v, s, r, du, dv, ds), s = w h, r = w / h; F = I + ones at (0,4), (1,5), (2,6);
 *   H = [I4 | 0]; R = diag(1, 1, 10, 10); P0 = diag(10, 10, 10, 10, 1e4, 1e4, 1e4); Q = diag(1, 1, 1, 1, 0.01, 0.01, 0.0001).
 *   Per frame with a detection (update_on_empty != 0: per frame): frame_count += 1; every tracker predicts (x[6] = 0 if x[6] + x[2] <= 0;
 *   x = F x; P = F P F' + Q; hit_streak = 0 if time_since_update > 0; time_since_update += 1; box: w = sqrt(x2 x3), h = x2 / w) and is
 *   deleted when its box has a NaN; IoU = inter / (a + b - inter) (no +1) between every detection and every tracker; the assignment
 *   that maximises the total IoU (shortest augmenting paths with potentials; the newer sort.py's shortcut for one-to-one threshold
 *   matrices is not built); pairs below iou_threshold are unmatched; a matched tracker updates (time_since_update = 0, hit_streak += 1,
 *   y = z - H x, S = H P H' + R, K = P H' S^-1 by Gaussian elimination with partial pivoting, x += K y,
 *   P = (I - K H) P (I - K H)' + K R K'); unmatched detections found trackers in detection order; the list is walked from last to
 *   first: reported when time_since_update < 1 and (hit_streak >= min_hits or frame_count <= min_hits), deleted when
 *   time_since_update > max_age.  A sequence computes the same bits alone or beside others.
 *
 * pmce_sort_track_resume_f64: pmce_sort_track_f64 on a piece of each sequence, with the trackers carried in ``state``: S records of
 *   pmce_sort_state_bytes() bytes each (device memory, 8-byte aligned), record i for sequence i.  Each wave loads its record before its
 *   first frame and stores it, in place, after its last (after that frame's time_since_update > max_age deletion); the outputs are
 *   indexed by the frames of this call.  Feeding a video in pieces of any lengths gives, frame for frame, the bits of the one
 *   pmce_sort_track_f64 launch over the whole video.  A record, with t = tracker slot 0..63 the minor index everywhere:
 *     double x[7][64]       the filter state (u, v, s, r, du, dv, ds)
 *     double P[7][7][64]    its covariance, row-major
 *     int    alive[64], id[64] (from 0), time_since_update[64], hit_streak[64]
 *     int    frame_count, next_id
 *   An all-zero record is a fresh tracker (hipMemset makes one), and a slot that is not alive is stored as zeros, so equal histories
 *   give equal bytes.  A sequence without a frame in the call (seq_offsets[i] == seq_offsets[i + 1]) and a call with F == 0 leave the
 *   records untouched.  The rule: the same max_tracks, max_age, min_hits, iou_threshold and update_on_empty on every call of one state;
 *   the record does not store them and the kernel cannot tell.  K may differ between calls.
 *
 * pmce_tracklet_boxes_f64: multi_person_tracker's prepare_output_tracks for a gathered list of reported rows: row index[i] of
 *   tracks[total][5] (an index outside gives zeros) -> out[n][4] = (cx, cy, s, s), w = x2 - x1, h = y2 - y1, cx = x1 + w / 2,
 *   cy = y1 + h / 2, s = w if w / h > 1 else h, in fp64. */
int pmce_yolo_nms_f32(const float* rows, int n, int R, int nc, float conf_thres, float nms_thres, int max_candidates, int max_keep,
                      float* dets, int* count, int* status, int* src_row, double* people, int* people_count, int class_id,
                      double score_thres, int score_product, double pad_x, double pad_y, double ratio, pmce_stream_t stream);
int pmce_sort_track_f64(const double* people, const int* people_count, const int* seq_offsets_host, const int* seq_offsets, int F, int K,
                        int S, int max_age, int min_hits, double iou_threshold, int max_tracks, int update_on_empty, double* tracks,
                        int* track_count, int* status, pmce_stream_t stream);
size_t pmce_sort_state_bytes(void);
int pmce_sort_track_resume_f64(const double* people, const int* people_count, const int* seq_offsets_host, const int* seq_offsets, int F,
                               int K, int S, int max_age, int min_hits, double iou_threshold, int max_tracks, int update_on_empty,
                               double* tracks, int* track_count, int* status, void* state, pmce_stream_t stream);
int pmce_tracklet_boxes_f64(const double* tracks, const int* index, int total, int n, double* out, pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's frames from JPEG files (csrc/jpeg.hip, csrc/jpeg_entropy.hpp): baseline Huffman JPEG, 8 bit, grey or YCbCr 4:4:4 / 4:2:2 /
 * 4:2:0 in one interleaved scan, decoded to the bytes that libjpeg's default decoder (and with it cv2.imread) gives: jidctint "islow",
 * "fancy" chroma upsampling, jdcolor's fixed-point conversion.  Integer arithmetic, no atomics, no host wait; the same bits whatever
 * the batch.  pmce_amd/jpeg.py parses the markers on the host, refuses what is not served and writes the records below; all are
 * int32 unless stated, and one batch of files is one set of concatenated arrays.  An Exif orientation tag is not read.
 *
 * data[n_bytes]            the files' bytes, one after the other (n_bytes <= 2^31 - 129).
 * images[n][24]            0 width, 1 height, 2 components (1 or 3), 3 h, 4 v (luma sampling, 1 or 2; 1, 1 for a grey file),
 *                          5 mcus_x, 6 mcus_y, 7 restart interval (0: none), 8..10 quantisation table of component c (index into
 *                          quant), 11..13 its DC and 14..16 its AC Huffman table (index into huffman), 17 first block of the image in
 *                          the coefficient buffer, 18 first byte of its planes in the plane buffer (both relative to the round the image
 *                          is decoded in), 19 first segment, 20 segment count, 21 blocks per MCU (h v + 2, or 1), 22..23 zero.
 * quant[n][64]             uint16, in zigzag order as DQT stores them.
 * huffman[n][546]          0..16 maxcode[l]: the largest code of length l (-1: none; entry 0 unused); 17..33 valoff[l]: the index of a
 *                          length-l code's value is code + valoff[l]; 34..289 values; 290..545 lookahead by the next 8 bits:
 *                          (length << 8) | value for codes of at most 8 bits, 0 otherwise.
 * segments[n][5]           (image, first byte, end byte, first MCU, MCU count): one per restart interval, one per image without DRI;
 *                          bytes index `data`; [first, end) holds entropy-coded bytes only (it ends where the next marker begins).
 * coefficients             int16 [blocks][64] in natural order; blocks in scan order: MCU by MCU, inside an MCU the luma blocks (v rows
 *                          of h), then Cb, then Cr.
 * planes                   uint8; per image the luma plane (mcus_x h 8) x (mcus_y v 8), then Cb and Cr, (mcus_x 8) x (mcus_y 8) each.
 * status bits              PMCE_JPEG_STATUS_TRUNCATED 1: a segment consumed bits from beyond its end (zero bits are supplied there);
 *                          PMCE_JPEG_STATUS_CORRUPT 2: a code of no table, a run past coefficient 63 or a marker inside a segment;
 *                          PMCE_JPEG_STATUS_RECORD 4: a record that does not fit its arrays (the host never writes one).  A segment
 *                          with a bit set ends after the block at hand; what it did not decode stays zero.  No lane reads outside its
 *                          segment's bytes or writes outside its segment's blocks, whatever the bytes say (scripts/jpeg_entropy_host.cpp).
 *
 * pmce_jpeg_entropy: zeroes coefficients[n_blocks] (16-byte aligned) and decodes segments [first_segment, first_segment + n_segments),
 *   one lane each, into them; segment_status[s] for each of them (the array spans all segments).  lds_tables != 0 (the default of
 *   pmce_amd.jpeg): with at most 16 Huffman tables in the batch the lanes read them from LDS; 0: always from global memory (the same
 *   bits, slower; the form a batch with more tables takes).  lanes: segments per 64-lane wavefront, 1 .. 64, or 0: as few as still give
 *   every segment a lane within 4096 wavefronts (lanes of one wavefront take their branches in turn, wavefronts do not).
 * pmce_jpeg_idct: images [first_image, first_image + n_images): coefficient blocks -> planes; max_blocks: the largest block count of one
 *   of these images.
 * pmce_jpeg_colour: the same images: planes -> frames[image][height][width][3] (B, G, R; R, G, B with rgb != 0) and status[image] = the
 *   OR of the image's segment status words.  frames and status are indexed by the absolute image number. */
#define PMCE_JPEG_STATUS_TRUNCATED 1
#define PMCE_JPEG_STATUS_CORRUPT 2
#define PMCE_JPEG_STATUS_RECORD 4
int pmce_jpeg_entropy(const unsigned char* data, long long n_bytes, const int* segments, int first_segment, int n_segments,
                      const int* images, int n_images, const int* huffman, int n_huffman, short* coefficients, long long n_blocks,
                      int* segment_status, int lds_tables, int lanes, pmce_stream_t stream);
/* pmce_jpeg_entropy_parallel (csrc/jpeg_parallel.hip, csrc/jpeg_parallel.hpp): pmce_jpeg_entropy's result - the same coefficients and
 *   the same segment_status words for every byte string - with many lanes per segment, for files with few restart markers or none.
 *   A segment of n bytes is cut into max(1, ceil(n / subsequence)) subsequences of `subsequence` bytes (a multiple of 4 in 4 .. 65536),
 *   one lane each; pmce_jpeg_parallel_run() (256) consecutive ones of a segment are a run, one workgroup.  Lanes decode from guessed
 *   states and synchronise (Weissenberger and Schmidt, ICPP 2018): run by run in LDS, then twice across the runs' borders; a check
 *   of the fixed-point condition hands a segment that has not converged to the serial body, so the result is exact for every stream.
 *   offsets[segment][2]         int32, for every segment of the batch: its first subsequence and its first run, both counted from
 *                               the first segment of the round it is decoded in (pmce_amd.jpeg.subsequence_records).
 *   n_subsequences, n_runs      of the segments [first_segment, first_segment + n_segments) together.
 *   workspace                   8-byte aligned, 32 bytes per subsequence + 28 per run + 8 per segment, in this order: entry[n_subsequences]
 *                               and exit[n_subsequences] (64 bits each: byte position | bit << 32 | block in MCU << 35 | zigzag index
 *                               << 38, bit 63: ended), border[2][n_runs] (64 bits), then int32: rounds[3][n_runs] (per synchronising
 *                               launch, the rounds in which a lane of the run decoded again), per subsequence the blocks it completed,
 *                               its first block, its status and its DC extent, then serial[n_segments] (1: handed to the serial body)
 *                               and stop[n_segments] (the first lane with a code error: the lanes behind it write nothing).
 *   stage                       -1: everything (the coefficients' memset and pmce_jpeg_parallel_stages() launches); 0 .. stages - 1:
 *                               that launch alone, for timing - 0 sync (with the memset), 1 .. 2 join, 3 place, 4 write, 5 dc.
 *   No atomics, no host read or wait; the number of launches depends on nothing but `stage`. */
int pmce_jpeg_entropy_parallel(const unsigned char* data, long long n_bytes, const int* segments, int first_segment, int n_segments,
                               const int* images, int n_images, const int* huffman, int n_huffman, short* coefficients,
                               long long n_blocks, int* segment_status, int lds_tables, int subsequence, const int* offsets,
                               int n_subsequences, int n_runs, void* workspace, long long workspace_bytes, int stage,
                               pmce_stream_t stream);
int pmce_jpeg_parallel_run(void);
int pmce_jpeg_parallel_stages(void);
int pmce_jpeg_idct(const short* coefficients, const int* images, int first_image, int n_images, int max_blocks,
                   const unsigned short* quant, int n_quant, long long n_blocks, unsigned char* planes, long long plane_bytes,
                   pmce_stream_t stream);
int pmce_jpeg_colour(const unsigned char* planes, long long plane_bytes, const int* images, int first_image, int n_images,
                     const int* segment_status, int n_segments_total, int width, int height, int rgb, unsigned char* frames, int* status,
                     pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's frames written as JPEG files (csrc/jpeg_encode.hip, csrc/jpeg_encode.hpp): baseline Huffman JFIF, YCbCr 4:4:4 / 4:2:2 /
 * 4:2:0 in one interleaved scan, Annex K's Huffman tables, the bytes that libjpeg's default compressor (and with it cv2.imwrite) writes:
 * jccolor's fixed-point conversion, jcsample's box filter, jccoefct's dummy blocks, jfdctint "islow", the rounding quantiser.  Integer
 * arithmetic, no host wait; the same bytes whatever the batch.  pmce_amd/jpeg.py builds the header and the quantisation tables on the host.
 *
 * coefficients             int16 [frames][blocks][64] in ZIGZAG order; a frame's blocks in scan order: MCU by MCU, inside an MCU the
 *                          luma blocks (v rows of h), then Cb, then Cr; the dummy blocks of the right and bottom edge included.
 * workspace                16-byte aligned, pmce_jpeg_encode_workspace_bytes(): the unstuffed stream - per restart interval (per frame
 *                          without one) a slot of 208 bytes per block, rounded up to 256 - then per block its bits (int32) and its bit
 *                          offset in the slot (int64), per interval its bits (int64), per 256-byte piece of a slot its bytes in the file
 *                          (int32) and its place in the file (int64), per frame the scan's length (int64).
 * data, offsets, status    the files back to back: frame f is data[offsets[f] .. offsets[f + 1]); offsets int64 [all frames + 1],
 *                          status int32 [all frames], both indexed by the absolute frame number.  A frame whose file would be longer
 *                          than `capacity`, or end beyond data_bytes, has length 0 and PMCE_JPEG_ENCODE_STATUS_CAPACITY.
 *
 * pmce_jpeg_encode_coefficients: frames [first_frame, first_frame + n_frames) of uint8 frames[..][height][width][3] (B, G, R; R, G, B with
 *   rgb != 0) -> coefficients (16-byte aligned, room for n_blocks >= n_frames * blocks); quant: uint16 [2][64], natural order, luma then
 *   chroma, entries 1 .. 255; h, v: the luma sampling, 1x1, 2x1 or 2x2.
 * pmce_jpeg_encode_entropy: the entropy stages alone, on coefficients as above (n_frames of mcus_per_frame MCUs, luma_blocks = h v luma
 *   blocks each; values beyond +-2047 (DC difference) and +-1023 (AC) are clamped) -> data, offsets[first_frame + 1 ..], status[first_frame ..];
 *   offsets[first_frame] is read (written as 0 for first_frame 0), so calls follow each other on one stream.  header: the file's bytes up to
 *   the scan, on the device, the same for every frame; restart_interval in MCUs, 0: none.  stage: -1 everything; 0 .. pmce_jpeg_encode_stages()
 *   - 1: that launch alone, for timing - 0 lengths, 1 offsets, 2 bits (with the stream's memset), 3 count, 4 place, 5 frames, 6 write.
 * pmce_jpeg_encode_scan_pass(): entries per pass of the offset scan (an interval with more blocks takes several passes). */
#define PMCE_JPEG_ENCODE_STATUS_CAPACITY 1
int pmce_jpeg_encode_scan_pass(void);
int pmce_jpeg_encode_stages(void);
size_t pmce_jpeg_encode_workspace_bytes(int n_frames, long long mcus_per_frame, int luma_blocks, int restart_interval);
int pmce_jpeg_encode_coefficients(const unsigned char* frames, long long first_frame, int n_frames, int width, int height, int h, int v,
                                  int rgb, const unsigned short* quant, short* coefficients, long long n_blocks, pmce_stream_t stream);
int pmce_jpeg_encode_entropy(const short* coefficients, int n_frames, long long mcus_per_frame, int luma_blocks, int restart_interval,
                             const unsigned char* header, int header_bytes, long long capacity, void* workspace, size_t workspace_bytes,
                             unsigned char* data, long long data_bytes, long long* offsets, int* status, long long first_frame, int stage,
                             pmce_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The demo's debug overlay (csrc/overlay.hip, csrc/overlay_cover.hpp): the tracker's boxes and ids and the pose stage's 2D skeletons
 * drawn on uint8 frames[n_frames][height][width][3], in place.  A row is one person in one frame; rows of a frame are drawn in the
 * order given, inside a row the box's edges (top, right, bottom, left), the label, the limbs in the skeleton's order, the discs in
 * keypoint order; the last primitive that covers a pixel decides it, and the pixel is blended once:
 * (alpha colour + (255 - alpha) pixel + 127) / 255.  The rules are integer: a coordinate v becomes rint(16 v),
 * pixel (x, y) has its centre at (16 x + 8, 16 y + 8); a segment of thickness t covers the centres within 8 t units of it, a disc those
 * within 16 radius of the keypoint; the label is the id in decimal, a 5 x 7 font in 6 x 8 cells of label_scale-sized blocks (the glyph
 * at columns 1..5, rows 1..7 of its cell) in text_color on the person's colour, its left column floor(x1), its rows ending above
 * row floor(y1), clamped into the frame (none if it is larger than the frame).  Integer atomics only: the same bytes whatever the
 * launch order, the other rows and frames of the call, and the chunking.  No host wait.
 *   frame_index int32 [n_rows] (device); frame_index_host: NULL, or the same table on the host when it is ASCENDING (rows of a frame
 *     still in drawing order) - a chunk of frames then launches its own rows only, otherwise every chunk launches all rows and the
 *     kernel skips those of other chunks; boxes fp64 [n_rows][4] or NULL, box_format 0 (x1, y1, x2, y2), 1 (cx, cy, w, h), 2 (x, y, w, h);
 *   ids int64 [n_rows] or NULL, 0 <= id < 10^9: the label, and the colour palette[id % n_palette] (palette[0] without ids);
 *   keypoints fp64 [n_rows][n_keypoints][keypoint_dim = 2 or 3] or NULL; a keypoint is drawn when it is finite and, with a third
 *     component, that score is >= score_thresh; skeleton int32 [n_limbs][2] (device): a limb needs both its ends drawn;
 *   font uint8 [10][7] (device): a glyph's rows, bit 4 the left column; palette uint8 [n_palette][3] (device), stored channel order;
 *   text_color: three bytes on the HOST; thickness, radius 1..64; label_scale 1..64; alpha 0..255;
 *   status int32 [n_rows] (device, out): 1 = a non-finite box, a box with w <= 0 or h <= 0, a non-finite keypoint (that primitive, and a
 *     limb that names the keypoint, are skipped) or an id out of range (the row is skipped); 2 = a primitive with an endpoint beyond
 *     |v| > 2^14 px was dropped; 4 = frame_index outside 0 .. n_frames - 1 (the row is skipped);
 *   workspace: 4-byte aligned device memory of at least pmce_overlay_workspace_bytes(width, height, 1) bytes, one 32-bit key per pixel
 *     of a chunk; the frames are processed in chunks of as many as fit.  Its content on entry does not matter.  width, height <= 8192.
 * The query returns 0 (and sets the error string) for arguments out of range. */
size_t pmce_overlay_workspace_bytes(int width, int height, int chunk_frames);
int pmce_draw_overlays(unsigned char* frames, int n_frames, int width, int height, const int* frame_index_host, const int* frame_index,
                       const double* boxes, int box_format, const long long* ids, const double* keypoints, int n_keypoints, int keypoint_dim,
                       const int* skeleton, int n_limbs, double score_thresh, int thickness, int radius, int label_scale,
                       const unsigned char* font, const unsigned char* palette, int n_palette, const unsigned char* text_color, int alpha,
                       int n_rows, int* status, void* workspace, size_t workspace_bytes, pmce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PMCE_HIP_H */
