/*
 * mpcmax.h -- C ABI of libmpcmax.so: the contrast-maximisation (CMax) loss hot path of
 * tub-rip/MotionPriorCMax, hand-written for AMD MI355X (gfx950).
 *
 * The reference has no native code and therefore no FFI to mirror; each entry point below
 * replaces a stretch of the reference's PyTorch code (cited per function, paths relative to
 * the reference root).  The Python host side (motionpriorcmax_amd.losses) binds these with
 * ctypes -- see INTEGRATION.md for the stub a maintainer would add to the reference.
 *
 * Conventions
 *  - all tensor arguments are DEVICE pointers to densely packed fp32 / int32 arrays owned by
 *    the caller (PyTorch allocates them); the library never frees or retains them;
 *  - `ws` is a caller-provided scratch buffer of at least mpc_workspace_bytes() bytes; its
 *    content carries state from a *_fwd call to the matching *_bwd call;
 *  - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns without
 *    synchronising or allocating; the work consists of kernel launches only (no memset / memcpy nodes), so a
 *    sequence of calls can be captured into a HIP graph and replayed;
 *  - no mutable global state takes part in a result: the last-error string is thread local, and the only
 *    process-wide state is one-time, idempotent set-up (raising the dynamic-LDS limit of the kernels, tuning
 *    switches read once from the environment, listed in csrc/knn.hip);
 *  - return value: 0 ok, >0 a hipError_t, <0 an argument error (MPC_E_*).  No C++ exception
 *    crosses the ABI.
 *
 * Event record layout (one row of events[B][M][6], loader.py:156-161,360-364):
 *   0:y  1:x  2:t in [0,1]  3:polarity  4:bin index  5:valid (0 for padding rows)
 * Rows [0,Mp) are the positive block, rows [Mp,M) the negative block (loader.py:392-395); the
 * polarity split is by ROW INDEX as in focus.py:216-227.
 */
#ifndef MPCMAX_H
#define MPCMAX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_VERSION 107

/* flags (mpc_shape.flags) -- one bit per FocusLoss constructor switch (focus.py:28-45) */
#define MPC_F_SCALE_BY_DT     (1u << 0)  /* scale_iwe_by_dt        focus.py:204-206 */
#define MPC_F_MASK_BORDER     (1u << 1)  /* mask_image_border      focus.py:208-214 */
#define MPC_F_POLARITY_SPLIT  (1u << 2)  /* polarity_aware_batching focus.py:216-227 */
#define MPC_F_NORM_L2         (1u << 3)  /* focus_loss_norm == 'l2' (else 'l1') loss.py:22-25 */
#define MPC_F_OBJ_VARIANCE    (1u << 4)  /* loss_type == 'variance' loss.py:14-16 (else gradient magnitude) */
#define MPC_F_DIST_L1         (1u << 5)  /* dist_norm == 'l1' (else squared 'l2') focus.py:132-135 */
#define MPC_F_SCHEME_IWD      (1u << 6)  /* interpolation_scheme == 'iwd' (else 'mean') focus.py:155-163 */
#define MPC_F_WANT_NEXT       (1u << 7)  /* also build flow_to_next (smooth_type == 'on_flow_to_next') focus.py:170-178 */
#define MPC_F_NO_WARP         (1u << 8)  /* splat events at their own (y,x): imager.create_iwe on raw events, logging.py:76-79 */
#define MPC_F_UNIT_WEIGHT     (1u << 9)  /* weight = 1.0 for every row (create_iwe default weight) */
#define MPC_F_ATOMIC_PATH     (1u << 10) /* debugging: plain global-atomic kernels instead of the LDS-tiled ones */
#define MPC_F_NO_BWD_RECORDS  (1u << 11) /* forward only: mpc_event_splat_fwd need not keep records for _bwd */

/* argument errors */
#define MPC_E_NULL      (-1)
#define MPC_E_SHAPE     (-2)
#define MPC_E_WORKSPACE (-3)
#define MPC_E_UNSUPPORTED (-4)

typedef struct mpc_shape {
    int32_t B;      /* samples in the batch                                   */
    int32_t M;      /* padded events per sample                               */
    int32_t Mp;     /* num_pos_events: rows [0,Mp) positive, [Mp,M) negative  */
    int32_t nb;     /* num_bins                                               */
    int32_t T;      /* num_tref                                               */
    int32_t H, W;   /* image_shape                                            */
    int32_t sp;     /* lut_superpixel_size                                    */
    int32_t hq, wq; /* LUT grid = ceil(H/sp) x ceil(W/sp)                     */
    int32_t n;      /* trajectories per sample                                */
    int32_t K;      /* num_knn                                                */
    uint32_t flags; /* MPC_F_*                                                */
} mpc_shape;

/* scalars written by mpc_contrast_fwd / mpc_lut_smooth / mpc_finalize into `scal` (device,
 * MPC_SCAL_COUNT floats) */
#define MPC_SCAL_LOSS     0   /* focus + smooth                    focus.py:94      */
#define MPC_SCAL_FOCUS    1   /* 1 / val                           loss.py:12       */
#define MPC_SCAL_SMOOTH   2   /* smooth_weight * smoothness        focus.py:246     */
#define MPC_SCAL_VAL      3   /* contrast value                    loss.py:14-27    */
#define MPC_SCAL_GCOEF    4   /* d focus / d raw-IWE = GCOEF * grad_iwe_unscaled    */
#define MPC_SCAL_COUNT    8

int mpc_version(void);
const char *mpc_last_error_string(void);
/* Bounds-checked debug build (-DMPC_BOUNDS, csrc/bounds.h; the reference has no sanitizer hooks): waits for
 * the device, returns the number of out-of-range indices the checked accessors of the library's kernels recorded since the
 * last call (and clears the records; the first one's file:line, workgroup, index, extent -> mpc_last_error_string()).
 * 0 = clean; -1 = this library is the product build (the accessors compile to the bare index).                            */
int mpc_bounds_check(void);

/* Diagnostics (bench.py's instrumented pass; no reference counterpart): between mpc_profile_start() and mpc_profile_stop()
 * every kernel the library launches is bracketed by two HIP events on its launch stream.  mpc_profile_stop synchronises
 * on them and returns the number of launches recorded: their kernel names, newline separated, in `names` (names_cap
 * bytes) and their durations in milliseconds in `ms` (cap entries), in launch order.  Process-wide; not for use inside
 * a graph capture. */
int mpc_profile_start(void);
int mpc_profile_stop(char *names, int32_t names_cap, float *ms, int32_t cap);

/* Bytes of scratch needed by any call with this shape. */
int64_t mpc_workspace_bytes(const mpc_shape *s);

/* ---- A5: KNN flow look-up table (focus.py:115-180) --------------------------------------
 * traj      [B][T+nb][n][2]  (y,x); rows [0,T) are the reference times, [T,T+nb) the bin mids
 * flow_lut  [B][nb][hq][wq][T][2]                                   (out)
 * flow_next [B][nb-1][hq][wq][1][2]  or NULL unless MPC_F_WANT_NEXT (out)
 * knn_state mpc_knn_state_floats(s) floats = [3][B][nb][hq*wq] + [B][nb][ceil(hq/16)*ceil(wq/16)][5] : K-th distance
 *           (f32), K-th index (i32 bits; bit 30 set if a point at exactly the K-th distance was excluded by the index
 *           tie rule), iwd normaliser, then the largest K-th distance of every 16x16 cell tile per class of query
 *           (inner / within r+1 cells of the top, bottom, left, right border) (out; consumed by _bwd)
 * idx_out   [B][nb][hq*wq][K] int32, ascending by (distance, index), or NULL (debug/tests)  */
int mpc_knn_lut_fwd(const mpc_shape *s, const float *traj, float *flow_lut, float *flow_next,
                    float *knn_state, int32_t *idx_out, void *ws, void *stream);

/* Number of floats of the knn_state buffer of mpc_knn_lut_fwd / _bwd for this shape. */
int64_t mpc_knn_state_floats(const mpc_shape *s);

/* Diagnostics: byte offset, inside the workspace, of the list of queries that mpc_knn_lut_fwd's strip kernel handed to
 * its per-query fallback: int32 count, then count entries (query id = ((b*nb + bin)*hq + cy)*wq + cx in the low 30 bits,
 * reason in the top 2: 0 fewer than K candidates inside the first search square, 1 more candidate slots than the
 * fast path holds, 2 more keys at the K-th distance level than it ranks, 3 staging overflow).  Read it after
 * mpc_knn_lut_fwd (tests assert that the fast path serves nearly all queries of the benchmark shapes). */
int64_t mpc_knn_fail_list_offset(const mpc_shape *s);
/* Diagnostics: byte offsets of the other work lists of the KNN forward inside the workspace: out[0] strips searched again in
 * quarters, [1] strips with far queries or queries to search again, [2] / [3] the maps of such queries (bit per query; those
 * that need more rings), [4] far lists per (sample, bin), [5] tiles for the far queries' backward; -1: no such list. */
int mpc_knn_list_offsets(const mpc_shape *s, int64_t *out);
/* Diagnostics: byte offset of the counters of the KNN forward's tail launch inside the workspace (int32 each, read them after
 * mpc_knn_lut_fwd): +0 queries the main launch marked for the tail's strip workgroups (at most 1 024: the tail took them from the
 * marked list with its one-wavefront search and ran no far pass), +128 entries of the late list, +256 strip workgroups that counted
 * themselves done.  Tests assert which path a launch took. */
int64_t mpc_knn_tail_counters_offset(const mpc_shape *s);

/* Backward of the above w.r.t. traj (indices carry no gradient; 'iwd' weights are constants -- since version 107 the tile gather serves
 * 'iwd' too: a member's weight is one hardware reciprocal of (d + 1e-9), 1 ulp, on the query's gradient divided by its normaliser --,
 * focus.py:157-163).  grad_flow_next may be NULL.  grad_traj [B][T+nb][n][2] is overwritten. */
int mpc_knn_lut_bwd(const mpc_shape *s, const float *traj, const float *grad_flow_lut,
                    const float *grad_flow_next, const float *knn_state, float *grad_traj,
                    void *ws, void *stream);

/* ---- A5 for n >= 65536 (focus.py:129-178 has no limit on n; mpc_knn_lut_fwd's tables are 16 bit) -------------------------------
 * The caller searches contiguous index chunks of at most 65535 points with mpc_knn_lut_fwd (idx_out) and hands the C sorted lists
 * over; the K nearest of all n points are the K smallest of their union by (distance, global index) -- exact, same tie rule.
 * Limits: n <= 2^22, C <= 64, (2 * C' + 1) * K * 4 bytes <= 64 KB with C' = C rounded up to a power of two (else
 * MPC_E_UNSUPPORTED).  Additive: the version number is unchanged, the binding checks the three symbols by name. */

/* Bytes of the scratch buffer of mpc_knn_idx_bwd for this shape (focus.py:129-178: backward of the gather). */
int64_t mpc_knn_wide_workspace_bytes(const mpc_shape *s);

/* Merge + interpolation (focus.py:129-178).
 * traj        [B][T+nb][n][2], all n points
 * cand        [C][B][nb][hq*wq][K] int32: list c = idx_out of mpc_knn_lut_fwd on the points [chunk_start[c], chunk_start[c+1]),
 *             indices local to the chunk
 * chunk_start C + 1 ascending int32 in HOST memory, chunk_start[0] = 0, chunk_start[C] = n, every chunk K .. 65535 points
 * idx_out     [B][nb][hq*wq][K] int32 global indices, ascending by (distance, index)                            (out)
 * flow_lut    [B][nb][hq][wq][T][2] 'mean', or 'iwd' with MPC_F_SCHEME_IWD: weights 1 / (d + 1e-9) divided by their sum,
 *             summed over the K members in list order, in fp64 on the fp32 inputs and rounded once                (out)
 * flow_next   [B][nb-1][hq][wq][1][2] with MPC_F_WANT_NEXT (the same neighbours, mean), else NULL                 (out)  */
int mpc_knn_merge_fwd(const mpc_shape *s, const float *traj, const int32_t *cand, const int32_t *chunk_start,
                      int32_t num_chunks, int32_t *idx_out, float *flow_lut, float *flow_next, void *stream);

/* Backward of the interpolation over a saved index list (focus.py:129-178; 'iwd' weights are constants, recomputed from traj):
 * idx [B][nb][hq*wq][K] as mpc_knn_merge_fwd wrote it; grad_flow_next may be NULL; grad_traj [B][T+nb][n][2] is overwritten.
 * Sums are 64-bit fixed point: bitwise reproducible from run to run.  ws: mpc_knn_wide_workspace_bytes(s) bytes. */
int mpc_knn_idx_bwd(const mpc_shape *s, const float *traj, const int32_t *idx, const float *grad_flow_lut,
                    const float *grad_flow_next, float *grad_traj, void *ws, void *stream);

/* ---- A6-A8: warp + weights + bilinear vote (focus.py:182-230, event_image_converter.py:333-391)
 * events   [B][M][6], flow_lut [B][nb][hq][wq][T][2], t_ref [T] (device)
 * iwe_raw  [B*T][P][H][W]  P = 2 with MPC_F_POLARITY_SPLIT else 1     (out, overwritten)   */
int mpc_event_splat_fwd(const mpc_shape *s, const float *events, const float *flow_lut,
                        const float *t_ref, float *iwe_raw, void *ws, void *stream);

/* ---- event-axis sharding ("optional finer split": a batch smaller than the number of ranks; the reference
 * has batch DDP only, scripts/flow_training.py:125-128).  mpc_event_splat_fwd_fixed = mpc_event_splat_fwd on THIS rank's
 * rows of `events`, but the output is the image's Q33.30 fixed-point accumulators themselves (int64 [B*T][P][H][W]).
 * Integer partial images add up exactly and in any order: all-reduce(SUM) them across the ranks, then
 * mpc_iwe_from_fixed converts to the fp32 raw IWE -- bit for bit the image one rank computes from all the events.
 * The backward per rank is mpc_event_splat_bwd on its own rows (a partial dL/dLUT; summed across ranks in fp32). */
int mpc_event_splat_fwd_fixed(const mpc_shape *s, const float *events, const float *flow_lut, const float *t_ref,
                              int64_t *iwe_fixed, void *ws, void *stream);
int mpc_iwe_from_fixed(const int64_t *iwe_fixed, float *iwe_raw, int64_t count, void *stream);

/* ---- A8 blur + A9 objective (event_image_converter.py:170-175, loss.py:4-27,58-87)
 * iwe_blur [B*T][P][H][W] (out) ; grad_iwe [B*T][P][H][W] or NULL (out: UNSCALED adjoint image
 * Blur^T Sobel^T u, or Blur^T (x - mean) for the variance objective; multiply by
 * scal[MPC_SCAL_GCOEF] to get d focus_loss / d iwe_raw).  Partial sums go to ws; call
 * mpc_finalize afterwards.                                                                  */
int mpc_contrast_fwd(const mpc_shape *s, const float *iwe_raw, float *iwe_blur, float *grad_iwe,
                     void *ws, void *stream);

/* ---- A10: smoothness of a flow field (focus.py:232-246, loss.py:29-56)
 * field [nimg][hq][wq][C] (the LUT layout: nimg = B*nb, C = 2*T; or flow_next: nimg = B*(nb-1),
 * C = 2).  grad_field (same shape, or NULL) receives d smoothness_loss / d field INCLUDING
 * smooth_weight.  Partial sums go to ws; call mpc_finalize afterwards.                       */
int mpc_lut_smooth(const mpc_shape *s, const float *field, int32_t nimg, int32_t C,
                   float smooth_weight, float *grad_field, void *ws, void *stream);

/* Reduce the partial sums of mpc_contrast_fwd and (if smooth_nimg > 0: the nimg, C, weight of
 * the preceding mpc_lut_smooth call) in fp64 and write scal[MPC_SCAL_*] (device).            */
int mpc_finalize(const mpc_shape *s, int32_t smooth_nimg, int32_t smooth_C, float smooth_weight,
                 float *scal, void *ws, void *stream);

/* ---- A11: backward of A6-A8 into the LUT.
 * grad_flow_lut[b][bin][iy][ix][tref][:] = grad_out * (scal[GCOEF] * sum over the cell's events of
 * w * bilinear-gradient of grad_iwe at the warped position  +  add_term[...]).
 * add_term: same shape as the LUT or NULL (used to fold in the smoothness gradient of
 * mpc_lut_smooth).  grad_out: device scalar or NULL (= 1).  Must follow mpc_event_splat_fwd on the
 * same workspace (the LDS-tiled path reuses the records that call left there).                 */
/* ---- UNPINNED EXTENSION (no reference code: the reference gathers a binned flow LUT, focus.py:182-195): gradient of the
 * objective with respect to the warped position of every event, i.e. autograd of create_iwe (event_image_converter.py:333-391)
 * through `warped = differences + events[..., :2]` (focus.py:191), for rows whose (y, x) columns hold positions that are warped
 * already (s->flags must carry MPC_F_NO_WARP; num_tref == 1).  grad_pos[b][i][:] = grad_out * scal[GCOEF] * w * bilinear
 * gradient of grad_iwe at the row's position, 0 for rows of weight 0.  Follows mpc_event_splat_fwd / mpc_contrast_fwd /
 * mpc_finalize of the same rows.  Used by FocusLoss.calc_per_event_basis (per-event continuous-time basis warp).          */
int mpc_event_pos_grad(const mpc_shape *s, const float *events, const float *t_ref, const float *grad_iwe,
                       const float *scal, const float *grad_out, float *grad_pos, void *stream);
/* Same extension, fused: mpc_pe_warp writes the rows with the per-event continuous-time basis warp applied --
 *   rows_out[b][i] = (y + sum_j coef[cell][0][j] phi[b][i][j], x + sum_j coef[cell][1][j] phi[b][i][j], t, p, cell, valid),
 * cell = the LUT cell of the event's own position (focus.py:186-187), coef_rows [B*hq*wq][2][k] the tile coefficients
 * (trajectories.py:15-52), phi [B][M][k] = basis_j(t_ref) - basis_j(t_event) (basis.py:18-31), or phi = NULL: the polynomial basis
 * t^(j+1) (basis.py:26-27) worked out in the kernels from t_ref[0] and the rows' time column, k <= 8 -- for mpc_event_splat_fwd with
 * MPC_F_NO_WARP; mpc_pe_grad is its backward: grad_coef_rows (zeroed here) += phi * d objective / d warped position, with float
 * atomics (the gradient of this extension is not bitwise reproducible).                                                    */
int mpc_pe_warp(const mpc_shape *s, const float *events, const float *coef_rows, const float *phi, int32_t k,
                const float *t_ref, float *rows_out, void *stream);
int mpc_pe_grad(const mpc_shape *s, const float *rows, const float *phi, int32_t k, const float *t_ref, const float *grad_iwe,
                const float *scal, const float *grad_out, float *grad_coef_rows, void *stream);
/* mpc_pe_grad for bucket-ordered events (mpc_event_bucket_order / mpc_ingest_scatter_ordered and their `offsets` table): no
 * global atomics -- every LUT strip of a sample accumulates in LDS fixed point (bitwise reproducible) and is written once.
 * `split` workgroups share the row ranges of a strip and write partial results: grad_coef_rows is [split][B*hq*wq][2][k], to be
 * summed over its first axis.  MPC_E_UNSUPPORTED if a strip's [cell][2][k] accumulators exceed the LDS (then: mpc_pe_grad).  */
int mpc_pe_grad_ordered(const mpc_shape *s, const float *rows, const int32_t *offsets, const float *phi, int32_t k,
                        const float *t_ref, const float *grad_iwe, const float *scal, const float *grad_out,
                        float *grad_coef_rows, int32_t split, void *stream);
/* 1 where mpc_pe_grad_ordered serves (shape, k), 0 where the caller takes mpc_pe_grad: the rule lives in the library only. */
int32_t mpc_pe_grad_ordered_supported(const mpc_shape *s, int32_t k);
/* Same extension: the dense <-> per-tile operators around the two calls above (csrc/tiles.hip; version 107: kernels instead of two
 * dozen torch operators -- the per-event step was bound by the host).
 *   mpc_pe_tile_rows      coef_rows [B*hq*wq][c2] = sum over the S scales of grid [B][S][c2][H][W] at the tile centres
 *                         (y, x) = (iy * tile + tile / 2, ix * tile + tile / 2): get_optical_flow_tile_mask + coeffs_grid_to_list,
 *                         src/utils/trajectories.py:3-52, scales summed as compute_basis does (basis.py:29-31); hq = ceil(H / tile).
 *                         A tile without a centre -- 0 < H % tile <= tile / 2: the centre of the last row of cells lies outside the
 *                         image (W and the last column likewise) -- gets ZERO coefficients: its events are not warped and it enters
 *                         the smoothness field with zero flow
 *   mpc_pe_tile_rows_bwd  its adjoint: EVERY element of grad_grid [B][S][c2][H][W] is written (0 off the tile centres; the gradient
 *                         of a tile without a centre goes nowhere)
 *   mpc_pe_basis_field    field [B*nb][G][2] = sum_j coef_rows[(b, cell)][d][j] * phim[t][j] -- the flow from the bin mid-times to
 *                         t_ref per tile, the field the smoothness term takes (mpc_lut_smooth: nimg = B * nb, C = 2); k <= 8, nb <= 64
 *   mpc_pe_rows_grad_finish  grad_coef_rows [B*G][2][k] = sum over the `split` partial results of mpc_pe_grad_ordered (split = 1: of
 *                         mpc_pe_grad) + grad_out[0] * (adjoint of mpc_pe_basis_field applied to grad_field, or nothing if NULL)  */
int mpc_pe_tile_rows(const float *grid, float *coef_rows, int32_t B, int32_t S, int32_t c2, int32_t H, int32_t W, int32_t tile, void *stream);
int mpc_pe_tile_rows_bwd(const float *grad_rows, float *grad_grid, int32_t B, int32_t S, int32_t c2, int32_t H, int32_t W, int32_t tile, void *stream);
/* The same two calls on a coefficient grid in the network's own precision (see "element types of the network tensors" below):
 * grid / grad_grid [B][S][c2][H][W] of element type `dtype`; coef_rows and grad_rows stay fp32.  mpc_pe_tile_rows IS
 * mpc_pe_tile_rows_dt(MPC_DT_F32).  The 16-bit gradient is written with 16-byte stores of 8 elements where W is a multiple of 8 and
 * the row start is 16-byte aligned, element by element otherwise. */
int mpc_pe_tile_rows_dt(const void *grid, int32_t dtype, float *coef_rows, int32_t B, int32_t S, int32_t c2, int32_t H, int32_t W, int32_t tile,
                        void *stream);
int mpc_pe_tile_rows_bwd_dt(const float *grad_rows, void *grad_grid, int32_t dtype, int32_t B, int32_t S, int32_t c2, int32_t H, int32_t W,
                            int32_t tile, void *stream);
int mpc_pe_basis_field(const float *coef_rows, const float *phim, float *field, int32_t B, int32_t G, int32_t k, int32_t nb, void *stream);
int mpc_pe_rows_grad_finish(const float *grad_parts, int32_t split, const float *grad_field, const float *phim, const float *grad_out,
                            float *grad_coef_rows, int32_t B, int32_t G, int32_t k, int32_t nb, void *stream);
/* Same extension, a TABULATED basis (FocusLoss.calc_per_event_basis(basis_type='table'); additive, still version 107): the basis is a
 * table [S + 1][k] of fp32 samples at the knots i / S, interpolated linearly at every event's time, each line one fp32 operation:
 *   tc = min(max(t, 0), 1);  x = tc * (float)S;  i = min((int)floorf(x), S - 1);  f = x - (float)i;
 *   B_j(t) = table[i][j] + f * (table[i + 1][j] - table[i][j]);   phi_j(event) = B_j(t_ref) - B_j(t_event)
 * -- a basis the kernels can read AND differentiate: no [B][M][k] tensor exists in either direction.
 *   mpc_pe_table_supported   1 where these calls serve (shape, k, S): MPC_F_NO_WARP, num_tref == 1, k <= 8, num_bins <= 64 and
 *                            (S + 1) * k <= mpc_pe_table_limit() (the 64-bit accumulators of mpc_pe_table_basis_grad in LDS); 0
 *                            where the caller takes another route.  The rule lives in the library only.
 *   mpc_pe_table_warp        mpc_pe_warp with phi from the table
 *   mpc_pe_table_grad        mpc_pe_grad with phi from the table; grad_pos [B][M][2] or NULL: every row's UNSCALED position gradient
 *                            (gy, gx) -- without scal[GCOEF] and grad_out; zeros for rows of weight 0 --, kept for
 *                            mpc_pe_table_basis_grad so that the adjoint image is gathered once
 *   mpc_pe_table_grad_ordered  mpc_pe_grad_ordered likewise (grad_pos is zeroed here: rows outside the offsets table stay zero)
 *   mpc_pe_table_basis_grad  grad_table [S + 1][k] = scal[GCOEF] * grad_out * d objective / d table through the events: with
 *                            G_j = gy * coef[cell][0][j] + gx * coef[cell][1][j], grad[i][j] -= (1 - f) G_j, grad[i + 1][j] -= f G_j at
 *                            every row's (i, f), and + (1 - f_r) sum G_j, + f_r sum G_j at the two knots of t_ref.  Sums in 64-bit
 *                            fixed point (Q33.30): bitwise reproducible for any row order and either event layout.  acc: scratch of
 *                            (S + 2) * k int64 (zeroed here).  (The smoothness term reaches the table through phim: below.)
 *   mpc_pe_field_basis_grad  the adjoint of mpc_pe_basis_field w.r.t. phim: grad_phim [nb][k] = grad_out[0] * sum over (b, cell, d) of
 *                            grad_field[(b, t)][cell][d] * coef_rows[(b, cell)][d][j]; fp64 sums in a fixed order; part: scratch of
 *                            nb * 64 * k doubles; k <= 8, nb <= 64                                                                  */
int32_t mpc_pe_table_supported(const mpc_shape *s, int32_t k, int32_t S);
int32_t mpc_pe_table_limit(void);
int mpc_pe_table_warp(const mpc_shape *s, const float *events, const float *coef_rows, const float *table, int32_t S, int32_t k,
                      const float *t_ref, float *rows_out, void *stream);
int mpc_pe_table_grad(const mpc_shape *s, const float *rows, const float *table, int32_t S, int32_t k, const float *t_ref,
                      const float *grad_iwe, const float *scal, const float *grad_out, float *grad_coef_rows, float *grad_pos, void *stream);
int mpc_pe_table_grad_ordered(const mpc_shape *s, const float *rows, const int32_t *offsets, const float *table, int32_t S, int32_t k,
                              const float *t_ref, const float *grad_iwe, const float *scal, const float *grad_out,
                              float *grad_coef_rows, int32_t split, float *grad_pos, void *stream);
int mpc_pe_table_basis_grad(const mpc_shape *s, const float *rows, const float *grad_pos, const float *coef_rows, int32_t S, int32_t k,
                            const float *t_ref, const float *scal, const float *grad_out, int64_t *acc, float *grad_table, void *stream);
int mpc_pe_field_basis_grad(const float *grad_field, const float *coef_rows, const float *grad_out, double *part, float *grad_phim,
                            int32_t B, int32_t G, int32_t k, int32_t nb, void *stream);

/* ---- UNPINNED EXTENSION (FocusLoss.calc_per_event_curves; csrc/pe_curves.hip): the per-event continuous-time warp along RAFT-spline
 * curves -- control points 1..d (P0 = 0; reference curves/polynomial.py:60-61: x channels first) on the 1/8 grid with the convex-
 * upsampling mask (raft_spline/utils.py:30-45), or per tile already; every event moves along the curve of its LUT cell at ITS OWN time.
 * The basis is evaluated in the kernels, in fp32 with one rounding per line (utils.curve_event_basis: the same lines in torch):
 *   MPC_PEC_BEZIER      u = 1 - t;  tp_1 = t, tp_i = tp_{i-1} * t;  up_0 = 1, up_1 = u, up_i = up_{i-1} * u;  E_i = (C(d,i) * tp_i) * up_{d-i}
 *   MPC_PEC_POLYNOMIAL  E_1 = t, E_i = E_{i-1} * t
 *   MPC_PEC_TABLE       table [S + 1][d]:  tc = min(max(t, 0), 1);  x = tc * (float)S;  i = min((int)floorf(x), S - 1);  f = x - (float)i;
 *                       E_j = T[i][j] + f * (T[i+1][j] - T[i][j])
 *   MPC_PEC_BSPLINE     the clamped (open-uniform) cubic B-spline of d + 1 control points (P0 = 0), L = d - 2 spans, 3 <= d; no table:
 *                         tc = min(max(t, 0), 1);  x = tc * (float)L;  s = min((int)floorf(x), L - 1)
 *                         u(k) = (float)min(max(s + k, 0), L)          scaled knots, exact small integers, k = -2..3
 *                         N_0 = 1
 *                         for j = 1..3:  saved = 0
 *                             for r = 0..j-1:
 *                                 right = u(r+1) - x;   left = x - u(1-j+r);   den = u(r+1) - u(1-j+r)      (den is 1, 2 or 3, never 0)
 *                                 temp = N_r / den;     N_r = saved + right * temp;     saved = left * temp
 *                             N_j = saved
 *                         E_{s-1+q} = N_q, q = 0..3   (index -1 is P0 and is dropped);   every other E_j = +0
 *                       (the division correctly rounded.)  t = 0: every E_j is exactly 0; t = 1: E_d is exactly 1, the others exactly 0;
 *                       at most 4 of the d are non-zero: mpc_pec_warp reads only the coefficient pairs whose phi_j is not 0 (at most 8;
 *                       the same bits as the dense sum for finite coefficients), mpc_pec_rows_grad adds nothing for the others.
 *   phi_j = E_j(t_ref[0]) - E_j(t_event)
 * mpc_pec_supported     the one copy of the limits: 0 = not served; bit 0: (shape, d, basis, S) is served -- MPC_F_NO_WARP, num_tref == 1,
 *                       1 <= d <= 16 (MPC_PEC_BSPLINE: 3 <= d <= 16), num_bins <= 64, a table with (S + 1) * d <= mpc_pe_table_limit(); bit 1: mpc_pec_rows_grad also
 *                       serves an offsets table (one order of a LUT strip's accumulators fits the LDS)
 * mpc_pec_head_rows     rows [B*G][2][d]:  rows[(b, cell)][0][j] = scale * up_y[j],  rows[(b, cell)][1][j] = scale * up_x[j]  at the tile
 *                       centres (iy * tile + tile / 2, ix * tile + tile / 2) of the 8h x 8w image, up as for mpc_cvx_traj_fwd; the centre
 *                       is never added.  mask NULL: params [B][2d][h][w] are per tile already (h x w tiles; tile is ignored).
 *                       With a mask tile is 2, 4, 8 or 16 and divides 8h and 8w: G = (8h / tile) * (8w / tile).
 * mpc_pec_head_rows_bwd its adjoint applied to grad_rows: grad_params [B][2d][h][w] and the dense grad_mask [B][576][h][w], every element
 *                       written, gather form, no float atomics.  (The adjoint of "centre + v" is that of v: with a mask this is
 *                       mpc_cvx_traj_bwd with the identity as its matrix.)  ws: mpc_pec_head_rows_bwd_workspace_bytes(), with a mask only.
 * mpc_pec_warp          rows_out [B][M][6] = (y + fy, x + fx, t, p, cell bits, valid), the record of mpc_pe_warp, for mpc_event_splat_fwd
 *                       with MPC_F_NO_WARP:  cell = the LUT cell of the event's own position;  fy = fx = 0;  for j ascending:
 *                       fy += rows[cell][0][j] * phi_j,  fx += rows[cell][1][j] * phi_j
 * mpc_pec_rows_grad     grad_rows[(b, cell)][a][j] = coef * sum over the rows of the cell of phi_j * grad_pos[row][a],  coef = (scal ?
 *                       scal[MPC_SCAL_GCOEF] : 1) * (grad_out ? grad_out[0] : 1);  rows_warped: what mpc_pec_warp wrote (time and cell
 *                       are read), grad_pos [B][M][2]: mpc_event_pos_grad's.  offsets (mpc_event_bucket_order): one workgroup per (sample,
 *                       LUT strip, pass over orders_per_pass orders) sums in LDS in Q33.30 and writes every element once -- bitwise
 *                       reproducible, each sum below 2^33 / coef in magnitude; at most as many orders per pass as cstrip_rows * wq * 2 * 8
 *                       bytes per order allow in 150 KB (more: MPC_E_UNSUPPORTED); orders_per_pass 0: the library's choice, the
 *                       fewest whose workgroups fit the device in one round (the pass is bound by its LDS atomics; same bits).  offsets NULL: grad_rows is zeroed and every
 *                       row adds with float atomics (any row order; slow, not reproducible).
 * mpc_pec_rows_grad_passes  the passes that call makes (0: not served with offsets)
 * mpc_pec_field         field [B*nbm][G][2] = sum_j rows[(b, cell)][a][j] * phim[t][j], j ascending (d <= 16, nbm <= 64): what mpc_lut_smooth takes
 * mpc_pec_field_adjoint grad_rows[(b, cell)][a][j] += grad_out[0] * sum_t grad_field[(b, t)][cell][a] * phim[t][j]
 * A table that TRAINS (additive, still version 107; served wherever mpc_pec_supported answers bit 0 for MPC_PEC_TABLE):
 * mpc_pec_table_basis_grad  grad_table [S + 1][d] = scal[MPC_SCAL_GCOEF] * grad_out[0] * d objective / d table through the events.
 *                       rows_warped: what mpc_pec_warp wrote (time and cell bits are read); grad_pos [B][M][2]: the UNSCALED position
 *                       gradients of mpc_event_pos_grad (a scal of ones, no grad_out); rows: mpc_pec_head_rows'.  With
 *                       G_j = gy * rows[cell][0][j] + gx * rows[cell][1][j] and (i, f) of the row's time, (ir, fr) of t_ref[0]:
 *                       grad[i][j] -= (1 - f) G_j, grad[i + 1][j] -= f G_j, grad[ir][j] += (1 - fr) G_j, grad[ir + 1][j] += fr G_j; rows
 *                       with (gy, gx) == (0, 0) add nothing.  One streaming pass, sums in 64-bit fixed point (Q33.30) in LDS: bitwise
 *                       the same for any row order, any grid and either event layout; |G_j| < 2^31 and a knot's sum over the batch
 *                       below 2^33.  1 <= d <= 16, S >= 1, (S + 1) * d <= mpc_pe_table_limit() (beyond: MPC_E_UNSUPPORTED, no launch).
 *                       acc: scratch of (S + 2) * d int64 (zeroed here).  The kernel body is mpc_pe_table_basis_grad's.
 * mpc_pec_field_basis_grad  the adjoint of mpc_pec_field w.r.t. phim: grad_phim [nbm][d] = grad_out[0] * sum over (b, cell, a) of
 *                       grad_field[(b, t)][cell][a] * rows[(b, cell)][a][j]; fp64 sums in a fixed order, bitwise reproducible; part:
 *                       scratch of nbm * 64 * d doubles; d <= 16, nbm <= 64                                                        */
#define MPC_PEC_BEZIER     0
#define MPC_PEC_POLYNOMIAL 1
#define MPC_PEC_TABLE      2
#define MPC_PEC_BSPLINE    3
int32_t mpc_pec_supported(const mpc_shape *s, int32_t d, int32_t basis, int32_t S);
int mpc_pec_head_rows(const float *params, const float *mask, float scale, int32_t tile, float *rows,
                      int32_t B, int32_t d, int32_t h, int32_t w, void *stream);
int64_t mpc_pec_head_rows_bwd_workspace_bytes(int32_t B, int32_t d, int32_t h, int32_t w, int32_t tile);
/* The two head calls on a mask in the network's own precision: mask / grad_mask [B][576][h][w] of element type `dtype` (ignored where
 * mask is NULL, but still checked); params, rows and their gradients stay fp32, the workspace is the same.  mpc_pec_head_rows(_bwd) ARE
 * these with MPC_DT_F32; the backward forwards to mpc_cvx_traj_bwd_dt. */
int mpc_pec_head_rows_dt(const float *params, const void *mask, int32_t dtype, float scale, int32_t tile, float *rows,
                         int32_t B, int32_t d, int32_t h, int32_t w, void *stream);
int mpc_pec_head_rows_bwd_dt(const float *grad_rows, const float *params, const void *mask, int32_t dtype, float scale, int32_t tile,
                             float *grad_params, void *grad_mask, int32_t B, int32_t d, int32_t h, int32_t w, void *ws, void *stream);
int mpc_pec_head_rows_bwd(const float *grad_rows, const float *params, const float *mask, float scale, int32_t tile,
                          float *grad_params, float *grad_mask, int32_t B, int32_t d, int32_t h, int32_t w, void *ws, void *stream);
int mpc_pec_warp(const mpc_shape *s, const float *events, const float *rows, int32_t basis, int32_t d, const float *table, int32_t S,
                 const float *t_ref, float *rows_out, void *stream);
int mpc_pec_rows_grad(const mpc_shape *s, const float *rows_warped, const int32_t *offsets, const float *grad_pos, int32_t basis,
                      int32_t d, const float *table, int32_t S, const float *t_ref, const float *scal, const float *grad_out,
                      int32_t orders_per_pass, float *grad_rows, void *stream);
int32_t mpc_pec_rows_grad_passes(const mpc_shape *s, int32_t d, int32_t orders_per_pass);
int mpc_pec_field(const float *rows, const float *phim, float *field, int32_t B, int32_t G, int32_t d, int32_t nbm, void *stream);
int mpc_pec_field_adjoint(const float *grad_field, const float *phim, const float *grad_out, float *grad_rows,
                          int32_t B, int32_t G, int32_t d, int32_t nbm, void *stream);
int mpc_pec_table_basis_grad(const mpc_shape *s, const float *rows_warped, const float *grad_pos, const float *rows, int32_t d, int32_t S,
                             const float *t_ref, const float *scal, const float *grad_out, int64_t *acc, float *grad_table, void *stream);
int mpc_pec_field_basis_grad(const float *grad_field, const float *rows, const float *grad_out, double *part, float *grad_phim,
                             int32_t B, int32_t G, int32_t d, int32_t nbm, void *stream);

int mpc_event_splat_bwd(const mpc_shape *s, const float *events, const float *flow_lut,
                        const float *t_ref, const float *grad_iwe, const float *scal,
                        const float *grad_out, float *grad_flow_lut, const float *add_term,
                        void *ws, void *stream);

/* ---- A4: the whole of FocusLoss.calc (focus.py:66-113) and of its backward as ONE call each: the same launch
 * sequence the stage entry points above issue (KNN LUT -> smoothness -> warp + vote -> blur + objective -> scalars;
 * event backward -> [scale] -> KNN backward), from C, so that a step costs two host calls instead of sixteen.
 * All buffers are caller-owned device memory (shapes as documented at the stage entry points):
 *   flow_next / smooth_grad : NULL unless used (MPC_F_WANT_NEXT; smooth_weight > 0 and the backward is wanted)
 *   grad_iwe                : NULL for a forward-only call (then also set MPC_F_NO_BWD_RECORDS)
 * smooth_weight > 0 applies the smoothness term to flow_next when MPC_F_WANT_NEXT is set, else to flow_lut
 * (focus.py:232-246).  mpc_focus_bwd must follow mpc_focus_fwd on the same buffers and workspace;
 * grad_lut_scratch [like flow_lut] and grad_next_scratch [like flow_next, or NULL] are scratch (version 107: the tile gather and the far
 * backward multiply the saved smoothness gradient by grad_out as they read it; grad_next_scratch is only written where the general
 * gather serves the shape -- num_tref > 1 -- but must still be given with smoothness on flow_to_next and a grad_out). */
typedef struct mpc_focus_buffers {
    const float *traj;        /* [B][T+nb][n][2]                      in  */
    const float *events;      /* [B][M][6]                            in  */
    const float *t_ref;       /* [T]                                  in  */
    float *flow_lut;          /* [B][nb][hq][wq][T][2]                out */
    float *flow_next;         /* [B][nb-1][hq][wq][1][2] or NULL      out */
    float *knn_state;         /* mpc_knn_state_floats(s)              out */
    float *smooth_grad;       /* like the smoothed field, or NULL     out */
    float *iwe_raw;           /* [B*T][P][H][W]                       out */
    float *iwe_blur;          /* [B*T][P][H][W]                       out */
    float *grad_iwe;          /* [B*T][P][H][W] or NULL               out */
    float *scal;              /* [MPC_SCAL_COUNT]                     out */
    float smooth_weight;
    const int32_t *event_offsets;  /* offsets table of mpc_event_bucket_order if `events` is ordered, else NULL   in  */
    float *scal_out;          /* [3] loss, focus, smooth once more, or NULL: the copy a caller hands out while `scal` stays saved for
                                 the backward (round 5: spares the host a copy kernel per step)                  out */
} mpc_focus_buffers;
int mpc_focus_fwd(const mpc_shape *s, const mpc_focus_buffers *io, void *ws, void *stream);
int mpc_focus_bwd(const mpc_shape *s, const mpc_focus_buffers *io, const float *grad_out,
                  float *grad_lut_scratch, float *grad_next_scratch, float *grad_traj, void *ws, void *stream);

/* ---- next row, layout half: a bucketed event layout handed from ingest to the loss.
 * mpc_event_bucket_order orders the rows of every polarity block of events [B][M][6] by (time bin, LUT strip), the key
 * of the backward buckets (it does not depend on the flow); padding rows stay at the end of their block.  Row order
 * inside a polarity block does not change the loss -- bit for bit -- so events_out is a valid `events` tensor anywhere.
 *   offsets [B][2][nb * S + 1] int32 (out), S = mpc_event_lut_strips(s): first row of bucket bin * S + strip of the
 *   block (strip = LUT row / ceil(hq / S), LUT row = clamp(int(y // sp), 0, hq - 1)), last entry = first padding row;   ws: mpc_event_order_workspace_bytes(s) bytes.
 * With the offsets, mpc_event_splat_fwd may be called with MPC_F_NO_BWD_RECORDS (it then writes no record per event
 * for the backward) and mpc_event_splat_bwd_ordered reads the event rows themselves (mpc_focus_buffers.event_offsets
 * does both). */
int32_t mpc_event_lut_strips(const mpc_shape *s);
int64_t mpc_event_order_workspace_bytes(const mpc_shape *s);
int mpc_event_bucket_order(const mpc_shape *s, const float *events_in, float *events_out, int32_t *offsets,
                           void *ws, void *stream);
int mpc_event_splat_bwd_ordered(const mpc_shape *s, const float *events, const int32_t *offsets, const float *flow_lut,
                                const float *t_ref, const float *grad_iwe, const float *scal, const float *grad_out,
                                float *grad_flow_lut, const float *add_term, void *ws, void *stream);

/* UNPINNED EXTENSION, default off (FocusLoss(pyramid_levels > 1)): helpers of an IWE pyramid, which BASELINE.json's
 * configs[2] names and the reference does not have.  mpc_pool2_fwd: out [nimg][H/2][W/2] = 2x2 average of in [nimg][H][W].
 * mpc_pool2_bwd_add: big[y][x] += (coef_small[0] / coef_big[0]) * 0.25 * small[y/2][x/2] (the adjoint of the pooling applied
 * to adjoint images that are kept in units of their own level's MPC_SCAL_GCOEF; both coefficients are device scalars). */
int mpc_pool2_fwd(const float *in, float *out, int32_t nimg, int32_t H, int32_t W, void *stream);
int mpc_pool2_bwd_add(const float *small, const float *coef_small, float *big, const float *coef_big, int32_t nimg,
                      int32_t H, int32_t W, void *stream);

/* UNPINNED EXTENSION: the IWE pyramid as one pass behind ANY forward of the library (csrc/iwe_pyramid.hip).  Every route ends
 * its forward in the raw IWE, the unscaled adjoint image grad_iwe and `scal` with d focus / d iwe_raw = scal[MPC_SCAL_GCOEF] *
 * grad_iwe; this pass adds the coarse levels to the latter two, so the backward of the route runs unchanged.  The definition is
 * the one of the helpers above: level l + 1 = 2x2 average of the raw level l (0.25f * ((p[0] + p[1]) + (p[W] + p[W + 1]))), the
 * 3x3 reflect blur and the gradient-magnitude objective on every level's own elements, focus = sum over the levels of 1 / val_l.
 *   mpc_iwe_pyramid_supported        host only, no device: 0, or MPC_E_UNSUPPORTED (levels outside [2, 6], MPC_F_OBJ_VARIANCE,
 *                                    T != 1), MPC_E_SHAPE (H or W not divisible by 2^(levels - 1), a coarsest level below 3x3, a
 *                                    shape mpc_workspace_bytes refuses), MPC_E_NULL.  The other two refuse the same, before any launch.
 *   mpc_iwe_pyramid_workspace_bytes  bytes of `pws` (host only).  Layout, part of the ABI: with want_grad the unscaled adjoint
 *                                    images of levels 1 .. levels - 1, [nimg][H >> l][W >> l] floats each, level l at float offset
 *                                    sum_{1 <= j < l} roundup(nimg * (H >> j) * (W >> j), 64); then the band sums.  nimg = B * P.
 *   mpc_iwe_pyramid_fwd              iwe_raw [nimg][H][W] (16-byte aligned); grad_iwe in/out, or NULL: no gradient (two launches
 *                                    instead of three); scal [MPC_SCAL_COUNT] in/out: FOCUS and LOSS gain the coarse levels' 1 / val_l
 *                                    (fp32, level by level; LOSS = the new FOCUS + SMOOTH), VAL and GCOEF stay level 0's; scal_out
 *                                    (or NULL): loss and focus once more, as mpc_focus_buffers.scal_out; level_scal (out)
 *                                    [levels][MPC_SCAL_COUNT]: row l = the scalars of level l alone (row 0: `scal` as it came) and in
 *                                    [MPC_SCAL_PYR_RATIO] the ratio r_l the fold used: grad_iwe[y][x] += sum_{l >= 1} r_l *
 *                                    g_l[y >> l][x >> l], r_l = 4^-l GCOEF_l / GCOEF_0, or 0 where a coefficient of level 0 .. l is 0,
 *                                    inf or NaN (mpc_pool2_bwd_add's rule: a flat level passes nothing on).  pws: a workspace of its
 *                                    own -- the step's `ws` carries state to the backward and is not touched.  Kernels only, on
 *                                    `stream`: no memset / memcpy node, no atomics, no host synchronisation; bitwise reproducible. */
#define MPC_SCAL_PYR_RATIO 5
int mpc_iwe_pyramid_supported(const mpc_shape *s, int32_t levels);
int64_t mpc_iwe_pyramid_workspace_bytes(const mpc_shape *s, int32_t levels, int32_t want_grad);
int mpc_iwe_pyramid_fwd(const mpc_shape *s, int32_t levels, const float *iwe_raw, float *grad_iwe, float *scal, float *scal_out,
                        float *level_scal, void *pws, void *stream);

/* y[i] = a[0] * x[i] (device scalar a; used to scale the smoothness gradient by grad_out). */
int mpc_scale(const float *x, const float *a, float *y, int64_t count, void *stream);

/* ---- next row: voxel-grid builder, reference src/loader/dsec/utils.py:29-77
 * (VoxelGrid.convert) as called from src/loader/dsec/loader.py:133-139.
 * xytp   [B][N][4] : x, y, t, p per raw event (p in {0,1}; t increasing within a sample; rows beyond
 *                    counts[b] are ignored)                        counts [B] int32 (device)
 * grid   [B][C][H][W] (out, overwritten).  norm: 0 none, 1 'mean_std', 2 'max'; quantile clipping before the
 * normalisation as in the reference (config/exe/flow_training/dsec.yaml uses quantile: 0). */
typedef struct mpc_vox_shape {
    int32_t B, N, C, H, W, norm;
    float quantile;   /* 0 <= quantile < 0.15: clip at the (1 - quantile) quantile of |grid| per sample (utils.py:57-61); 0 = off */
    float keep;       /* fp32(1 - quantile) with the subtraction done in DOUBLE by the caller, as `torch.quantile(x, 1 - q)` receives
                         it in the reference (utils.py:58): fp32(1 - fp64(q)) and 1 - fp32(q) differ by an ulp for ~6 % of the q.
                         0 = derive it from `quantile` */
} mpc_vox_shape;
int64_t mpc_voxel_workspace_bytes(const mpc_vox_shape *s);
int mpc_voxel_grid(const mpc_vox_shape *s, const float *xytp, const int32_t *counts, float *grid,
                   void *ws, void *stream);

/* ---- centred voxel grid: the network input of the EVIMO2 and MultiFlow configurations, reference
 * src/loader/utils/representation.py:26-111 (VoxelGrid.convert) and :9-18 (norm_voxel_grid) as called from
 * src/loader/evimo2/datasubset.py:146-189 and src/loader/multiflow/sample.py:172-200, with the resize of datasubset.py:189
 * (F.interpolate(size=(Ho, Wo), mode='bilinear', align_corners=False)) applied after the normalisation.
 * x, y, pol [B][N] fp32 (pol in {0,1}; integer coordinates are exact in fp32), time [B][N] int64 (increasing within a sample;
 * rows beyond counts[b] are ignored), counts [B] int32, centres [B][2] int64 = (t0_center, t1_center) per sample or NULL = the
 * first and last valid timestamp of the sample (read on the device).  All pointers are device pointers.
 * t_norm = float(time - c0) / float(c1 - c0) * float(C - 1); floor for every index; int_xy = 1: two taps per event at [t, y, x]
 * (representation.py:85-94; an event outside the sensor or with a non-integer coordinate is DROPPED, where the reference's flat
 * index wraps or raises), int_xy = 0: eight taps (:96-109).  c1 == c0 (also: a sample of one event with default centres) gives
 * no time axis: such a sample's grid is zero.  norm = 1: mean / unbiased std over the non-zero entries, (v - mean) / std if
 * std > 0 else v - mean, zeros stay.  grid [B][C][Ho or H][Wo or W] (out, every element written); a sample with counts[b] == 0
 * is all zero.  Kernels only, on `stream`; no allocation, no host synchronisation: the call can be captured into a HIP graph.
 * MPC_E_UNSUPPORTED: C < 2, H < 2 or W < 2 (the reference's asserts), or sizes the LDS strips cannot hold.
 * ws: mpc_repr_workspace_bytes(s) bytes, sized for the worst case so that no event distribution can overflow it: record buckets of
 * four times the mean fill (128 B per event row of [B][N]), per-sample spill regions that hold every record a sample can produce
 * (64 B per row, 96 B with int_xy = 0) and their chunk lists (one 16-byte descriptor per binning workgroup and bucket it can
 * overflow, up to 64 B per row): about 260 B x B x N, 2.3 GB at B = 6, N = 1 500 000.  It is scratch: nothing is kept between calls. */
typedef struct mpc_repr_shape {
    int32_t B, N, C, H, W, int_xy, norm, Ho, Wo;   /* Ho = Wo = 0: no resize */
} mpc_repr_shape;
int64_t mpc_repr_workspace_bytes(const mpc_repr_shape *s);
int mpc_repr_grid(const mpc_repr_shape *s, const float *x, const float *y, const int64_t *time, const float *pol,
                  const int32_t *counts, const int64_t *centres, float *grid, void *ws, void *stream);
/* norm_voxel_grid (representation.py:9-18) of grids that already lie in device memory: grid [B][per_sample], each sample
 * normalised in place over its non-zero entries.  ws: mpc_repr_norm_workspace_bytes(B) bytes.  No host synchronisation (the
 * reference's `if std > 0` is one). */
int64_t mpc_repr_norm_workspace_bytes(int32_t B);
int mpc_repr_norm(float *grid, int32_t B, int64_t per_sample, void *ws, void *stream);

/* ---- next row: event ingest, reference src/loader/dsec/loader.py:152-167 (time
 * normalisation, bin index, in-image filter, polarity split) + :360-415 (pad_events, sequence_collate_fn).
 * x, y, p [B][N] float32, t_us [B][N] int64 (increasing within a sample), counts [B] int32 (device).
 * mpc_ingest_count  -> out_max[2] (device): largest number of valid positive / negative events of a sample;
 *                      the caller reads them to size `events`  = [B][max_pos + max_neg][6]
 * mpc_ingest_scatter-> events (zero padded, valid flag in column 5, positive block first) and, if xytp is
 *                      not NULL, [B][N][4] = (x, y, t, p) as loader.py:135-138 hands them to the voxel grid. */
typedef struct mpc_ingest_shape {
    int32_t B, N, H, W, nb;
} mpc_ingest_shape;
int64_t mpc_ingest_workspace_bytes(const mpc_ingest_shape *s);
int mpc_ingest_count(const mpc_ingest_shape *s, const float *x, const float *y, const int64_t *t_us,
                     const float *p, const int32_t *counts, int32_t *out_max, void *ws, void *stream);
int mpc_ingest_scatter(const mpc_ingest_shape *s, const float *x, const float *y, const int64_t *t_us,
                       const float *p, const int32_t *counts, int32_t max_pos, int32_t max_neg,
                       float *events, float *xytp, void *ws, void *stream);

/* Ingest straight into the bucket-ordered layout: the outputs of mpc_ingest_scatter followed by mpc_event_bucket_order for
 * the loss shape `loss` (its B, nb, H, W, sp, hq, wq, flags; M = max_pos + max_neg, Mp = max_pos), without the extra pass
 * over the event tensor -- the (time bin, LUT strip) of an event is known when its row is written.  offsets
 * [B][2][nb * S + 1] as documented at mpc_event_bucket_order.  ws: the workspace mpc_ingest_count used (unchanged since);
 * ws_order: mpc_ingest_ordered_workspace_bytes(s, loss) bytes. */
int64_t mpc_ingest_ordered_workspace_bytes(const mpc_ingest_shape *s, const mpc_shape *loss);
int mpc_ingest_scatter_ordered(const mpc_ingest_shape *s, const mpc_shape *loss, const float *x, const float *y,
                               const int64_t *t_us, const float *p, const int32_t *counts, int32_t max_pos, int32_t max_neg,
                               float *events, int32_t *offsets, float *xytp, void *ws, void *ws_order, void *stream);

/* The same three steps with the DSEC rectification inside the coordinate load: reference loader.py:153,187-189,
 * x_rect, y_rect = rectify_ev_map[y, x].T.  x, y [B][N] int32 are the raw sensor pixel indices, rectify_map [Hs][Ws][2] fp32
 * (contiguous, 8-byte aligned; last axis (x_rect, y_rect)); Hs, Ws need not equal s->H, s->W.  One 8-byte load per event after a
 * bounds test on the raw index; no [B][N] float arrays are written.  Everything behind the load is what the float entry points
 * compute on the gathered values (a NaN map entry fails 0 <= v and the row is dropped, as numpy's mask drops it); xytp carries the
 * rectified coordinates of all rows (loader.py:169).  UNPINNED: an index outside the map (x >= Ws, y >= Hs, negative) raises or
 * wraps in the reference; here the row is dropped from `events` and written to xytp as (-2, -2, t, p).  The workspace query and
 * the order of the calls are those of the float entry points (mpc_ingest_workspace_bytes, mpc_ingest_ordered_workspace_bytes). */
int mpc_ingest_rect_count(const mpc_ingest_shape *s, int32_t Hs, int32_t Ws, const float *rectify_map, const int32_t *x,
                          const int32_t *y, const int64_t *t_us, const float *p, const int32_t *counts, int32_t *out_max,
                          void *ws, void *stream);
int mpc_ingest_rect_scatter(const mpc_ingest_shape *s, int32_t Hs, int32_t Ws, const float *rectify_map, const int32_t *x,
                            const int32_t *y, const int64_t *t_us, const float *p, const int32_t *counts, int32_t max_pos,
                            int32_t max_neg, float *events, float *xytp, void *ws, void *stream);
int mpc_ingest_rect_scatter_ordered(const mpc_ingest_shape *s, const mpc_shape *loss, int32_t Hs, int32_t Ws,
                                    const float *rectify_map, const int32_t *x, const int32_t *y, const int64_t *t_us,
                                    const float *p, const int32_t *counts, int32_t max_pos, int32_t max_neg, float *events,
                                    int32_t *offsets, float *xytp, void *ws, void *ws_order, void *stream);

/* ---- event ingest for the EVIMO2 and MultiFlow configurations: the raw window -> the same `events` tensor, without the in-image
 * filter of the DSEC loader.  x, y [B][N] int32 (xy_int = 1) or fp32; p [B][N] int64 (p_int64 = 1) or fp32, in {0, 1} (for EVIMO2
 * the flipped polarity 1 - p of datasubset.py:154); t_us [B][N] int64, NON-DECREASING within a sample; counts [B] int32 (device;
 * rows beyond counts[b] are ignored).  The same padded arrays mpc_repr_grid takes.
 *   time_mode = MPC_WINDOW_TIME_FP32_SUFFIX: reference src/loader/evimo2/datasubset.py:206-215, whose arithmetic is FLOAT32 from
 *     the first subtraction on (f32() = round to nearest, n = counts[b]):
 *       ts_start = f32(t[n-1]) - duration_us          duration_us = f32(flow_duration_ms * 1e3), rounded by the caller
 *       kept     : f32(t[i]) > ts_start               (strict; a suffix of the window)
 *       t_i      = (f32(t[i]) - ts_start) / (f32(t[n-1]) - ts_start)          correctly rounded fp32 quotient
 *       bin_i    = max(#{k : edges[k] < t_i} - 1, 0)  edges [nb + 1] fp32 (device): the values of torch.linspace(0, 1, nb + 1) as
 *                                                     computed on the CPU (datasubset.py:77), handed in by the caller
 *   time_mode = MPC_WINDOW_TIME_MINMAX64: reference src/loader/multiflow/sample.py:224-236 -- (t - min) / (max - min) in float64
 *     over all counts[b] events, the float64 edges of np.linspace (as mpc_ingest_scatter), cast to fp32 last; edges is not read.
 *   row = (y * y_scale, x * x_scale, t, p, bin, 1) in fp32.  The scales (one fp32 multiply each; 1 = coordinates as they are) are
 *     UNPINNED: the reference hands X_SCALE / Y_SCALE along (datasubset.py:227-228) but ships no code that applies them.
 *   split = 1 (polarity_aware_batching; datasubset.py:217-221, multiflow/datasubset.py:149-154, src/modules/data_loading.py:14-47):
 *     rows with p == 1, zero padded to the batch maximum max_pos, then rows with p == 0 padded to max_neg; input order inside
 *     each block.  split = 0 (data_loading.py:35-37): one block of max_pos rows, max_neg = 0, p is copied and not looked at.
 *   counts[b] == 0 gives zero rows (the EVIMO2 reference raises on ts[-1]).
 * mpc_ingest_window_count   -> out_max[2] (device) = max_pos, max_neg: the caller reads them to size events [B][max_pos + max_neg][6]
 * mpc_ingest_window_scatter -> events, every element written.  ws: mpc_ingest_window_workspace_bytes(s) bytes, unchanged between
 * the two calls.  Kernels only, on `stream`.  MPC_E_UNSUPPORTED: nb + 1 > 4096 in the fp32 mode (the edges live in LDS). */
#define MPC_WINDOW_TIME_FP32_SUFFIX 0
#define MPC_WINDOW_TIME_MINMAX64 1
typedef struct mpc_window_shape {
    int32_t B, N, nb;
    int32_t time_mode;          /* MPC_WINDOW_TIME_* */
    int32_t xy_int;             /* x, y: 1 = int32, 0 = fp32 */
    int32_t p_int64;            /* p: 1 = int64, 0 = fp32 */
    int32_t split;              /* 1 = positive block then negative block, 0 = one block */
    float duration_us;          /* fp32 mode only */
    float x_scale, y_scale;
} mpc_window_shape;
int64_t mpc_ingest_window_workspace_bytes(const mpc_window_shape *s);
int mpc_ingest_window_count(const mpc_window_shape *s, const int64_t *t_us, const void *p, const int32_t *counts,
                            int32_t *out_max, void *ws, void *stream);
int mpc_ingest_window_scatter(const mpc_window_shape *s, const void *x, const void *y, const int64_t *t_us, const void *p,
                              const int32_t *counts, const float *edges, int32_t max_pos, int32_t max_neg, float *events,
                              void *ws, void *stream);

/* ---- next row: dense flow from tile trajectories and flow error metrics.
 * mpc_dense_flow = reference src/utils/flow.py:12-16 (dense_flow_from_traj): list_to_grid
 *   (src/utils/trajectories.py:54-76) at pixel_positions // patch, then the anti-aliased bicubic resize
 *   of src/utils/flow.py:9-10 to H x W.
 *   traj_flow [B][n][C], pixel_positions [n][2] int64 (y, x)
 *   patch_flow [B][C][H/patch][W/patch] (out), dense [B][C][H][W] (out)
 * mpc_flow_error = reference src/utils/flow.py:18-70 (calculate_flow_error).
 *   flow_gt, flow_pred [B][2][H][W]; event_mask [B][H][W] bytes (non-zero = true) or NULL;
 *   time_scale [B] or NULL; out[5] (device) = EPE, 1PE, 2PE, 3PE, AE (degrees). */
typedef struct mpc_flow_shape {
    int32_t B, C, n, patch, H, W;
} mpc_flow_shape;
int mpc_dense_flow(const mpc_flow_shape *s, const float *traj_flow, const int64_t *pixel_positions,
                   float *patch_flow, float *dense, void *stream);
typedef struct mpc_err_shape {
    int32_t B, H, W;
} mpc_err_shape;
int64_t mpc_flow_error_workspace_bytes(const mpc_err_shape *s);
int mpc_flow_error(const mpc_err_shape *s, const float *flow_gt, const float *flow_pred,
                   const uint8_t *event_mask, const float *time_scale, float *out, void *ws, void *stream);

/* ---- next row + BASELINE.json configs[3]: flow curves sampled at the tile centres as `trajectories` for the loss.
 * Reference: src/models/raft_spline/curves/base.py:88-123 (CurveBase.get_flow_from_reference: flow(t) = sum_k B_k(t) P_k, P_0 == 0),
 * bezier.py:92-113 (Bernstein basis, evaluated on the host in float64 as the reference does), polynomial.py:60-61 (dim 1 = (x, y)).
 *   params [B][2][d][n]  control points 1..d of every tile, channel 0 = x, channel 1 = y (the network's [B, 2d, h, w] output, n = h*w)
 *   basis  [T][d]        basis functions at the T reconstruction times (Bernstein: pinned by bezier.py; clamped cubic B-spline:
 *                        UNPINNED extension -- the reference has no such curve)
 *   pos    [n][2]        tile centres (y, x) (src/utils/trajectories.py:3-13)
 *   traj   [B][T][n][2]  (out)  (y, x) = pos + scale * sum_k basis[t][k] * (P_k.y, P_k.x)
 * mpc_curve_traj_bwd: grad_params [B][2][d][n] (out, overwritten) = the adjoint of the above applied to grad_traj [B][T][n][2].  */
int mpc_curve_traj_fwd(const float *params, const float *basis, const float *pos, float scale, float *traj,
                       int32_t B, int32_t d, int32_t T, int32_t n, void *stream);
int mpc_curve_traj_bwd(const float *grad_traj, const float *basis, float scale, float *grad_params,
                       int32_t B, int32_t d, int32_t T, int32_t n, void *stream);

/* ---- the RAFT-spline output head: control points on the 1/8 grid + convex-upsampling mask -> `trajectories` / dense flows.
 * Reference: src/models/raft_spline/curves/base.py:35-38 (create_upsampled), src/models/raft_spline/utils.py:30-45 (cvx_upsample:
 * softmax over the 9 neighbours, F.unfold's row-major 3 x 3 order, zero padding, the factor 8 of the change in resolution),
 * base.py:95-123 + bezier.py:92-113 (get_flow_from_reference), src/modules/raft_spline.py:122-154 (the flows validation evaluates).
 *   params [B][2][d][h][w]   control points 1..d on the 1/8 grid, channel 0 = x, channel 1 = y
 *   mask   [B][576][h][w]    logits, channel = k * 64 + sy * 8 + sx (k: neighbour, (sy, sx): position inside the 8 x 8 cell)
 *   basis  [T][d]            as for mpc_curve_traj_fwd
 *   up[c] at pixel (y, x) = sum_k softmax_k(mask[k][y % 8][x % 8][y / 8][x / 8]) * 8 * P0[c][y / 8 + k / 3 - 1][x / 8 + k % 3 - 1]
 *   traj   [B][T][n][2]      (out)  (y, x) = tile centre + scale * sum_j basis[t][j] * (up.y[j], up.x[j]) at the tile centres
 *                            (iy * tile + tile / 2, ix * tile + tile / 2) of the 8h x 8w image in row-major order (computed by the
 *                            kernel; src/utils/trajectories.py:3-13), n = their count
 *   flows  [T][B][2][8h][8w] (out)  scale * sum_j basis[t][j] * up[j] at every pixel, (x, y) order (forward only)
 * mpc_cvx_traj_bwd: the adjoint applied to grad_traj [B][T][n][2]: grad_params [B][2d][h][w] and the DENSE grad_mask [B][576][h][w]
 * (every element written, 0 off the channels the tile centres read), either may be NULL and is then not computed; gather form, no
 * float atomics: bitwise reproducible.  ws: mpc_cvx_traj_bwd_workspace_bytes() bytes, needed (non-NULL) only with grad_params.
 * Limits: d <= 16, T * d * 4 <= 48 KB (else MPC_E_UNSUPPORTED); tile >= 1.  B = 0 or an empty grid launches nothing.  */
int mpc_cvx_traj_fwd(const float *params, const float *mask, const float *basis, float scale, float *traj,
                     int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile, void *stream);
int64_t mpc_cvx_traj_bwd_workspace_bytes(int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile);
int mpc_cvx_traj_bwd(const float *grad_traj, const float *params, const float *mask, const float *basis, float scale,
                     float *grad_params, float *grad_mask, int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile,
                     void *ws, void *stream);
int mpc_cvx_flow_fwd(const float *params, const float *mask, const float *basis, float scale, float *flows,
                     int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, void *stream);

/* ---- element types of the network tensors (additive: the version number is unchanged, the binding checks the symbols by name).
 * The networks in front of these nodes run under autocast or as .half() / .bfloat16() models, so their two large outputs -- the
 * coefficient grid and the convex-upsampling mask -- arrive in 16 bits.  Every `_dt` entry point is the call of the same name with
 * `void *` for that tensor and for its gradient plus the element type; EVERYTHING else in the signature stays fp32 (traj, rows, basis,
 * dphi, params / grad_params, grad_traj, grad_dphi, workspaces), and the workspace-size queries are those of the fp32 calls.
 *   load    fp16 by the hardware convert, bf16 as bits << 16: exact, and the arithmetic behind the load is that of the fp32 kernels --
 *           every forward output equals, bit for bit, what the fp32 call returns for the upcast tensor
 *   store   each gradient element is computed in fp32 exactly as in the fp32 call and rounded ONCE to `dtype`, round to nearest even:
 *           bf16 by  NaN -> 0x7FC0, else u += 0x7FFF + ((u >> 16) & 1), u >>= 16  (the bits of torch.Tensor.to(torch.bfloat16)); fp16 by
 *           the hardware convert (overflow to +-inf, subnormals kept).  Elements off the tile centres are +0.
 * The fp32 entry points ARE the `_dt` ones with MPC_DT_F32: one copy of the host code, the same kernels and bits as before.  Any other
 * dtype code: MPC_E_UNSUPPORTED with an error string, no launch. */
#define MPC_DT_F32 0
#define MPC_DT_F16 1
#define MPC_DT_BF16 2
int mpc_cvx_traj_fwd_dt(const float *params, const void *mask, int32_t dtype, const float *basis, float scale, float *traj,
                        int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile, void *stream);
int mpc_cvx_flow_fwd_dt(const float *params, const void *mask, int32_t dtype, const float *basis, float scale, float *flows,
                        int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, void *stream);
/* grad_mask in `dtype`: the zero fill keeps its plane / chunk walk (1024 elements a chunk), 16-byte stores of 8 elements where the
 * ADDRESS of the 8 is 16-byte aligned (a plane of odd h * w starts at any even address), element by element otherwise. */
int mpc_cvx_traj_bwd_dt(const float *grad_traj, const float *params, const void *mask, int32_t dtype, const float *basis, float scale,
                        float *grad_params, void *grad_mask, int32_t B, int32_t d, int32_t T, int32_t h, int32_t w, int32_t tile,
                        void *ws, void *stream);

/* ---- row A3 of SURVEY.md 8(a): the network's coefficient grid -> `trajectories` for the loss, and back.
 * Reference: src/modules/trajectory_net.py:57-119 (compute_basis, calculate_coords, calculate_trajectories_at_t: the reference's
 * TrajectoryNet.step, :142-161), src/utils/trajectories.py:3-52 (tile mask, coeffs_grid_to_list), src/utils/basis.py:4-46.
 *   grid   [B][S][2k][H][W]  channels 0..k-1: y coefficients, k..2k-1: x; the S scales are summed
 *   tiles  (y, x) = (iy * tile + tile / 2, ix * tile + tile / 2), iy < hq = ceil((H - tile / 2) / tile), ix < wq likewise (the count of
 *          get_optical_flow_tile_mask's mask[s::tile, s::tile] -- NOT ceil(H / tile) as the LUT cells of mpc_pe_tile_rows); tile
 *          i = iy * wq + ix, n = hq * wq (the order of torch.nonzero)
 *   dphi[t][j] = phi_j(times[t]) - phi_j(anchor_time), j = 1..k:  MPC_BASIS_POLY t^j,  MPC_BASIS_DCT sqrt(2) cos(pi/2 (2t + 1) j) --
 *          evaluated by the kernels from the DEVICE array times [n_t] (never read by the host) -- or MPC_BASIS_MATRIX: the caller's
 *          dphi [n_t][k] (a learned basis: net(times) - net(anchor)); `times` may be NULL then, `dphi` is ignored otherwise
 *   traj   [B][n_t][n][2]  (out)  (y, x) = sum_j dphi[t][j] * (cy[j], cx[j]) (+ the tile centre if add_offsets)
 *   rows   [B*n][2k] (out, or NULL)  the scale-summed coefficients of every tile (what the backward needs for grad_dphi)
 * mpc_grid_traj_bwd: grad_grid [B][S][2k][H][W] (out) = the adjoint applied to grad_traj [B][n_t][n][2]: EVERY element is written (0 off
 * the tile centres; nothing to pre-zero).  grad_dphi [n_t][k] (out, or NULL; MPC_BASIS_MATRIX only, needs rows of the forward and
 * scratch of mpc_grid_traj_scratch_floats() floats) = sum over (b, i) of g.y * cy[j] + g.x * cx[j], summed in a fixed order.
 * Limits: k <= 16, n_t * k * 4 <= 16 KB (else MPC_E_UNSUPPORTED).  B = 0 or no tile: the forward launches nothing; the backward
 * still zero-fills a grid without tiles, and with B = 0 writes grad_dphi = 0 (if given); pointers to empty arrays may be NULL. */
#define MPC_BASIS_POLY 0
#define MPC_BASIS_DCT 1
#define MPC_BASIS_MATRIX 2
int64_t mpc_grid_traj_scratch_floats(int32_t B, int32_t k, int32_t H, int32_t W, int32_t tile, int32_t n_t);
int mpc_grid_traj_fwd(const float *grid, const float *times, const float *dphi, int32_t basis, float anchor_time, int32_t add_offsets,
                      float *traj, float *rows, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W, int32_t tile, int32_t n_t,
                      void *stream);
int mpc_grid_traj_bwd(const float *grad_traj, const float *times, const float *dphi, int32_t basis, float anchor_time, const float *rows,
                      float *grad_grid, float *grad_dphi, float *scratch, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W,
                      int32_t tile, int32_t n_t, void *stream);
/* The same two calls on a grid of element type `dtype` (MPC_DT_*, above): grid / grad_grid [B][S][2k][H][W]; traj, rows, dphi and
 * grad_dphi stay fp32.  The 16-bit gradient is written with 16-byte stores of 8 elements where W is a multiple of 8 and grad_grid is
 * 16-byte aligned, element by element otherwise. */
int mpc_grid_traj_fwd_dt(const void *grid, int32_t dtype, const float *times, const float *dphi, int32_t basis, float anchor_time,
                         int32_t add_offsets, float *traj, float *rows, int32_t B, int32_t S, int32_t k, int32_t H, int32_t W, int32_t tile,
                         int32_t n_t, void *stream);
int mpc_grid_traj_bwd_dt(const float *grad_traj, const float *times, const float *dphi, int32_t basis, float anchor_time, const float *rows,
                         void *grad_grid, int32_t dtype, float *grad_dphi, float *scratch, int32_t B, int32_t S, int32_t k, int32_t H,
                         int32_t W, int32_t tile, int32_t n_t, void *stream);

/* ---- the RAFT-spline validation step's flow metrics (what scripts/trajectory_inference.py logs) as one fused reduction.
 * Reference: src/modules/raft_spline.py:88-215 (validation_step: which metric sees which prediction and mask), src/modules/utils.py
 * :85-102 epe_masked, :104-126 epe_masked_multi, :128-184 ae_masked(_multi), :186-218 n_pixel_error_masked, :220-296
 * calculate_flow_error / calculate_trajectory_flow_error, :335-541 the Metric classes (when update() adds a value), :67-74 the
 * linear-motion baseline.
 *   predictions P_m, m < M, (x, y) order, from ONE of
 *     params [B][2][d][h][w] + up_mask [B][576][h][w] + basis [M][d] (d >= 1; H = 8h, W = 8w): the curves of mpc_cvx_flow_fwd evaluated
 *       in registers, never written (the same device functions: the same bits), or
 *     flows  [M][B][2][H][W] (d = 0; h, w ignored);
 *     both times `scale`
 *   timestamps [M] fp32 (device)   the baseline's prediction at step m is timestamps[m] * P_{M-1}
 *   flow_gt    [B][M][2][H][W]     finite (the loaders zero NaN; the reference itself yields NaN on inf)
 *   flow_valid [B][M][H][W] bytes (non-zero = true), or NULL: V_m
 *   ev_repr    [B][C][H][W] (E = any channel != 0, a NaN counts), or event_mask [B][H][W] bytes: exactly one of the two
 *   values [MPC_VAL_COUNT] fp32, updated [MPC_VAL_COUNT] int32 (out, device): the keys below; updated = 1 where the reference's
 *     Metric.update adds the value, 0 where it skips (the epe family with every mask empty: value NaN) or raises (NPE with an empty
 *     mask, utils.py:199: the five singles of that mask are NaN / 0 -- unpinned) and for the EPE_STEP slots >= M (value 0).
 * Per pixel, step and sample: e = |P - G|, a = acos(clamp((P.G + 1) / (|(P, 1)| |(G, 1)|))), r_k = e > k && e / max(|G|, 1e-6) >= 0.05
 * in fp32 (the angle as atan2(|u x v|, u.v), u = (P, 1), v = (G, 1): the same angle without the loss of acos near 1); every sum in
 * fp64, every count an integer; a fixed reduction order, no atomics: bitwise reproducible.
 *   epe = sum_K e / |K|, ae = sum_K a / |K| (degrees), kpe = 100 sum_K r_k / |K|     over the whole batch, step M - 1
 *   epe_multi = mean over the steps with |K_m| > 0 of epe_m; ae_multi = sum_m ae_m / M (0 / 0 = NaN, as the reference)
 *   TEPE / T3PE / TAE = mean over the M * B images of sum_F e, #_F(e > 3), sum_F a (degrees) / (|F| + 1e-5), F = K_m && Gx != 0 &&
 *     Gy != 0 && both finite; EPE_STEPmm = the mean over the B images of step m of the first
 * Kernels only on `stream` (no memset / memcpy nodes: capturable), nothing read back.  ws: mpc_val_metrics_workspace_bytes() bytes.
 * Limits: d <= 16, M <= 16 (else MPC_E_UNSUPPORTED).  B = 0 launches nothing (values / updated are left as they are).  */
#define MPC_VAL_MAX_STEPS 16
#define MPC_VAL_EPE 0                  /* val/epe ae 1pe 2pe 3pe: no mask, step M - 1 */
#define MPC_VAL_AE 1
#define MPC_VAL_1PE 2
#define MPC_VAL_2PE 3
#define MPC_VAL_3PE 4
#define MPC_VAL_MASKED_SINGLE 5        /* + the five above: val/masked_epe ..: mask E */
#define MPC_VAL_MULTI 10               /* val/<..>: no mask */
#define MPC_VAL_EV_MASKED_MULTI 31     /* val/ev_masked_<..>: E && V_m (E alone without flow_valid) */
#define MPC_VAL_MASKED_MULTI 52        /* val/masked_<..>: V_m (no mask without flow_valid) */
#define MPC_VAL_EPE_MULTI 0            /* offsets inside each of the three groups of 5 + MPC_VAL_MAX_STEPS */
#define MPC_VAL_AE_MULTI 1
#define MPC_VAL_T3PE 2
#define MPC_VAL_TEPE 3
#define MPC_VAL_TAE 4
#define MPC_VAL_EPE_STEP 5             /* + m */
#define MPC_VAL_EPE_MULTI_LIN 73
#define MPC_VAL_AE_MULTI_LIN 74
#define MPC_VAL_COUNT 75
typedef struct mpc_val_shape {
    int32_t B, M, d, h, w, H, W, C;    /* d = 0: predictions from `flows`; C = 0: E from `event_mask` */
} mpc_val_shape;
int64_t mpc_val_metrics_workspace_bytes(const mpc_val_shape *s);
int mpc_val_metrics(const mpc_val_shape *s, const float *params, const float *up_mask, const float *basis, const float *flows,
                    float scale, const float *timestamps, const float *flow_gt, const uint8_t *flow_valid, const float *ev_repr,
                    const uint8_t *event_mask, float *values, int32_t *updated, void *ws, void *stream);

/* ---- the RAFT-spline correlation lookup: the one gather inside the network's update loop, 12 times per forward.
 * Reference: src/models/raft_spline/corr.py:304-348 (CorrBlockParallelMultiTarget.__call__), raft_spline/utils.py:4-20
 * (bilinear_sampler: grid_sample, align_corners=True, zero padding), raft.py:165-189 (flows = bezier.get_flow_from_reference(times);
 * coords1 = coords0 + flows; corr_block(coords1)), corr.py:262-270, 106-123, 296-302 (the pyramid the lookup reads).
 *   level l (num_levels of them)  [n_l][B*h*w][h_l][w_l]  the correlation volume of the n_l targets that have more than l levels
 *                                 (level_target[l][0..n_l), ascending), avg-pooled l times: h_l = h >> l, w_l = w >> l
 *   entries e = (level, slot) in level-major order, E = sum_l n_l; K = 2 * radius + 1
 *   centre of (target t, sample b, pixel (y, x)):  coords [T][B][2][h][w] ((x, y) order), or -- coords == NULL -- the Bezier mode:
 *                                 (x, y) + sum_j basis[t][j] * params[b][(x: j, y: d + j)][y][x], params [B][2d][h][w], basis [T][d]
 *   out [B][E * K * K][h][w]      channel e * K * K + i * K + j = the bilinear sample (zero outside, per tap) of the query's OWN slice
 *                                 level[l][slot][b * h * w + y * w + x] at (centre.x / 2^l + j - radius, centre.y / 2^l + i - radius)
 * The offsets are integers: the K * K samples of one (query, entry) share one pair of fractions and read one (K + 1)^2 window.
 * mpc_corr_lookup_bwd: the adjoint applied to grad_out [B][E * K * K][h][w] -- grad_coords [T][B][2][h][w] (coords mode) or grad_params
 * [B][2d][h][w] (Bezier mode: the curve adjoint in the same launch), and for every level with desc->grad_level[l] != NULL the whole
 * of grad_level[l] (window cells in gather form, every other element 0: nothing to pre-zero).  A NULL gradient pointer drops its
 * part.  In the Bezier mode a non-NULL grad_coords is written too -- the coordinate gradient of every target, which the launch forms
 * before it contracts it with the matrix (what mpc_curve_basis_grad, below, sums the matrix' own gradient from); grad_params may
 * then be NULL.  A query's slice is read by that query alone: no atomics, every sum in a fixed order, bitwise reproducible.  One launch
 * each way; the descriptor travels by value as a kernel argument (no copy to the device).
 * MPC_CORR_F_GRAD_ACCUM (mpc_corr_lookup_bwd only): every non-NULL grad_level[l] holds a gradient already (a call without the flag
 * wrote it) and the window cells of this call are ADDED to it -- per in-slice window cell of each (slot, query) one read, one add of
 * the cell's gathered cotangent (formed first, the same up-to-four-term sum in the same order) and one store; every other element
 * is left untouched, a cell is visited once per launch, work and traffic follow the windows and not the slices.  grad_coords /
 * grad_params are written as without the flag; with every grad_level NULL the flag changes nothing.  The calls that share a buffer
 * must be ordered on one stream.
 * Limits: radius <= 4, d <= 16, T <= 16, num_levels <= 6 (else MPC_E_UNSUPPORTED); level sizes that are not (h >> l, w >> l), are
 * below 2 (the reference divides by w_l - 1), or a target list that is not ascending / nested: MPC_E_SHAPE.
 * mpc_corr_lookup_supported: the same checks on the host alone, 0 or the error code.  */
#define MPC_CORR_MAX_LEVELS 6
#define MPC_CORR_MAX_TARGETS 16
#define MPC_CORR_MAX_RADIUS 4
typedef struct mpc_corr_desc {
    int32_t B, h, w, T, d, radius, num_levels;     /* d: control points per axis (Bezier mode; ignored with coords) */
    int32_t flags;                                  /* MPC_CORR_F_LANE_PER_QUERY (diagnostics), MPC_CORR_F_GRAD_ACCUM */
    int32_t level_h[MPC_CORR_MAX_LEVELS], level_w[MPC_CORR_MAX_LEVELS], level_n[MPC_CORR_MAX_LEVELS];
    uint8_t level_target[MPC_CORR_MAX_LEVELS][MPC_CORR_MAX_TARGETS];
    const float *level[MPC_CORR_MAX_LEVELS];
    float *grad_level[MPC_CORR_MAX_LEVELS];         /* mpc_corr_lookup_bwd only */
} mpc_corr_desc;
#define MPC_CORR_F_LANE_PER_QUERY 1                    /* forward: one thread per (query, entry) instead of a wave per window (probe A/B) */
#define MPC_CORR_F_GRAD_ACCUM 2                        /* backward: add the window cells into grad_level, leave the rest of it untouched */
int mpc_corr_lookup_supported(const mpc_corr_desc *desc);
int mpc_corr_lookup_fwd(const mpc_corr_desc *desc, const float *coords, const float *params, const float *basis, float *out,
                        void *stream);
int mpc_corr_lookup_bwd(const mpc_corr_desc *desc, const float *coords, const float *params, const float *basis,
                        const float *grad_out, float *grad_coords, float *grad_params, void *stream);

/* ---- the gradient of the basis matrix of the three RAFT-spline nodes above (additive, still version 107): the reference's
 * curve_type LEARNED while its basis network trains (src/models/raft_spline/curves/learned.py:76-77).  The curve is linear in the
 * matrix, so one reduction serves mpc_curve_traj_bwd, mpc_cvx_traj_bwd and mpc_corr_lookup_bwd, run BEHIND them (their kernels are
 * unchanged).  With R[b][i][c][j] the control points that site i of sample b evaluates and G[t][b][i][c] the cotangent of the
 * displacement there (c: x, y):
 *   grad_basis [T][d] (out, overwritten) = scale * sum over (b, i) of (G[t][b][i].x * R[b][i].x[j] + G[t][b][i].y * R[b][i].y[j])
 *   MPC_CBG_PLAIN   the plain head:  R = params [B][2][d][sites] (x first), G = grad_traj [B][T][sites][2] ((y, x) order), sites = n
 *   MPC_CBG_ROWS    the convex-upsampling head:  R = rows [B * sites][2][d] (y first) of mpc_pec_head_rows(_dt) called with scale 1 --
 *                   the upsampled control points at the tile centres, in the mask's own dtype --, G = grad_traj as above
 *   MPC_CBG_LOOKUP  the lookup in the Bezier mode:  R = params [B][2d][h][w], G = grad_coords [T][B][2][h][w] as mpc_corr_lookup_bwd
 *                   writes it when it is given grad_coords in that mode -- beside grad_params, or alone with grad_params NULL
 *                   (params detached); sites = h * w, scale = 1.  A call that does not ask for grad_coords there launches what it
 *                   launched before.
 * Two kernels: per-workgroup partials [P][T][d] over 256 consecutive (sample, site) pairs each (a butterfly over the wavefront, the
 * waves in order), then the finishing pass of mpc_grid_traj_bwd's grad_dphi over the partials.  No float atomics, no host
 * synchronisation, nothing allocated: bitwise reproducible, independent of the scheduling.  scratch:
 * mpc_curve_basis_grad_scratch_floats() floats = ceil(B * sites / 256) * T * d.
 * Limits: those of the nodes, d <= 16 and T * d * 4 <= 48 KB (else MPC_E_UNSUPPORTED, also from the size query).  B = 0 or sites = 0:
 * grad_basis = 0 (one kernel); G, R and scratch may be NULL then. */
#define MPC_CBG_PLAIN 0
#define MPC_CBG_ROWS 1
#define MPC_CBG_LOOKUP 2
int64_t mpc_curve_basis_grad_scratch_floats(int32_t B, int32_t d, int32_t T, int32_t sites);
int mpc_curve_basis_grad(const float *G, const float *R, int32_t layout, float scale, float *grad_basis, float *scratch,
                         int32_t B, int32_t d, int32_t T, int32_t sites, void *stream);

/* ---- the RAFT-spline correlation pyramid the lookup reads, built from the two feature maps on the fp32 matrix cores.
 * Reference: src/models/raft_spline/corr.py:235-270 (CorrComputation._corr_dot_prod_1_to_N / get_correlation_volume:
 * fmap1^T fmap2 / sqrt(D)), corr.py:106-123 (CorrData.get_downsampled: avg_pool2d 2 x 2 stride 2 per level, an odd last row /
 * column dropped), corr.py:296-302 (level l holds the targets with more than l levels), raft.py:126 (fp32).
 *   fmap1 [B][D][h][w], fmap2 [T][B][D][h][w]; the descriptor gives B, h, w, T, num_levels, level_h / level_w / level_n /
 *   level_target as for the lookup; `radius`, `d` and `flags` are ignored.
 * mpc_corr_pyramid_fwd (replaces corr.py:262-270 and :106-123): writes desc->level[l] [n_l][B*h*w][h_l][w_l] for every level,
 *   level_l[slot][b*h*w + i][j] = (sum_c fmap1[b][c][i] * P_l(fmap2[t][b])[c][j]) / sqrt(D), P_l the 2 x 2 mean applied l times
 *   (pooling commutes with the product), c ascending in one fma chain (v_mfma_f32_32x32x2_f32): one GEMM launch over all levels
 *   after one small pooling launch per level >= 1; every level written once, none read back.
 * mpc_corr_pyramid_bwd (replaces the autograd of the same lines): cotangents desc->grad_level[l] (inputs; NULL = zero),
 *   grad_fmap1 [B][D][h][w] and / or grad_fmap2 [T][B][D][h][w] (NULL drops it and its launches); every element of a gradient is
 *   written by a kernel (nothing to pre-zero), no atomics, every sum in a fixed order: bitwise reproducible.  desc->level[] is not read.
 * mpc_corr_pyramid_workspace_bytes (>= 16; < 0: the error code): the caller owns `ws` (16-byte aligned); the forward's holds
 *   the pooled feature maps, the backward's (backward != 0) also the per-level feature-map gradients and the split-k partials.
 * Limits: D a multiple of 4 in [4, 512], T <= 16, num_levels <= 6 (else MPC_E_UNSUPPORTED); level sizes that are not
 * (h >> l, w >> l) or are empty, D < 1, or a target list that is not ascending / nested: MPC_E_SHAPE.
 * mpc_corr_pyramid_supported: these checks on the host alone, 0 or the error code.  B = 0 launches nothing.  */
long long mpc_corr_pyramid_workspace_bytes(const mpc_corr_desc *desc, int D, int backward);
int mpc_corr_pyramid_supported(const mpc_corr_desc *desc, int D);
int mpc_corr_pyramid_fwd(const mpc_corr_desc *desc, int D, const float *fmap1, const float *fmap2, void *ws, void *stream);
int mpc_corr_pyramid_bwd(const mpc_corr_desc *desc, int D, const float *fmap1, const float *fmap2, float *grad_fmap1,
                         float *grad_fmap2, void *ws, void *stream);

/* Same extension, several references (additive, still version 107): the events-plus-frames pyramid of the reference's default model.
 * Reference: corr.py:221-225 (CorrComputation.__add__: the flat target list is the concatenation of the references' targets, events
 * then frames in raft.py:131-144), corr.py:246-260 (_corr_dot_prod_M_to_N), corr.py:282-302 (the merged volume, pooled).
 *   reference r: fmap1[r] [B][D][h][w], fmap2[r] [n_r][B][D][h][w], n_r = first_target[r + 1] - first_target[r] >= 1; flat target
 *   t = first_target[r] + k is target k of reference r; first_target[0] = 0, first_target[R] = desc->T.  All references share B, D,
 *   h, w.  `desc` describes the merged pyramid exactly as above (within a level the slots of one reference are contiguous):
 *   level_l[slot][b*h*w + i][j] = (sum_c fmap1[ref(t)][b][c][i] * P_l(fmap2[ref(t)][k][b])[c][j]) / sqrt(D).
 * The feature maps are read where they lie (no concatenated copy on the device) and grad_fmap1[r] / grad_fmap2[r]
 * (mpc_corr_pyramid_multi_bwd only; NULL drops that gradient, a reference with both NULL launches nothing of its own) are written
 * straight into their own tensors, every element by a kernel.  Launches: those of the single-reference call of the merged target list -- the forward one
 * GEMM after the pools, the backward at most one grad_fmap1 GEMM (over reference, split, sample, tile), one reduce, one gP GEMM, one
 * gather.  Every reference keeps the k split of the single-reference problem of that reference alone: the call equals the R
 * single-reference calls bit for bit (levels sliced by slot range, gradients per reference).
 * mpc_corr_pyramid_multi_workspace_bytes: the sum of mpc_corr_pyramid_workspace_bytes over the references taken alone.
 * Limits: those above on the merged list, and R in [1, MPC_CORR_MAX_REFS] (else MPC_E_UNSUPPORTED; the per-reference plans travel
 * to the kernels by value); a first_target that does not rise from 0 to desc->T: MPC_E_SHAPE.
 * mpc_corr_pyramid_multi_supported: these checks on the host alone.  */
#define MPC_CORR_MAX_REFS 4
typedef struct mpc_corr_refs {
    int32_t R;
    int32_t first_target[MPC_CORR_MAX_REFS + 1];
    const float *fmap1[MPC_CORR_MAX_REFS], *fmap2[MPC_CORR_MAX_REFS];
    float *grad_fmap1[MPC_CORR_MAX_REFS], *grad_fmap2[MPC_CORR_MAX_REFS];      /* mpc_corr_pyramid_multi_bwd only */
} mpc_corr_refs;
long long mpc_corr_pyramid_multi_workspace_bytes(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int backward);
int mpc_corr_pyramid_multi_supported(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs);
int mpc_corr_pyramid_multi_fwd(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, void *ws, void *stream);
int mpc_corr_pyramid_multi_bwd(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, void *ws, void *stream);

/* The same four calls on feature maps of element type `dtype` (MPC_DT_*, additive, still version 107): what the RAFT-spline encoders
 * hand over under autocast, read in place instead of the reference's `.float()` copies (raft.py:126).  fmap1 / fmap2 and grad_fmap1 /
 * grad_fmap2 are of that type -- in the list form the pointers of mpc_corr_refs are READ AS that type, one dtype per call --; levels,
 * cotangents and the workspace stay fp32, and the workspace and `_supported` queries are those above.  The fp32 entry points ARE
 * these with MPC_DT_F32: the same kernels and bits as before.  Any other dtype code: MPC_E_UNSUPPORTED with an error string, no launch.
 * With MPC_DT_F16 / MPC_DT_BF16:
 *   level 0 of the forward runs on the 16-bit matrix cores (v_mfma_f32_32x32x16_f16 / _bf16, k_corr_pyr_gemm16): products of two
 *     16-bit values are exact in fp32 and the accumulation is fp32, so the element is the sum the fp32 call forms on the upcast
 *     tensors in another order (16 channels per instruction): equal where every partial sum is exact, otherwise within
 *     gamma(D) * sum |fmap1| |fmap2| / sqrt(D), gamma(n) = (n + 8) u / (1 - (n + 8) u) with u = 2^-23 (the rounding of the
 *     instruction's adder is not specified).  fp16 subnormal inputs are multiplied as the values they are, not flushed.
 *   everything else -- the pools, the forward levels >= 1, both backward products, the reduce and the gather -- converts the 16-bit
 *     element at the load (exact) and is the fp32 call's arithmetic on the upcast tensors bit for bit, on v_mfma_f32_32x32x2_f32
 *     with the same tiling, k splits and order of partials.  The forward is two GEMM launches (level 0, then the levels above).
 *   gradients are computed in fp32 as in the fp32 call and rounded ONCE to `dtype`, round to nearest even (as
 *     torch.Tensor.to(dtype)); grad_fmap2 with 16-byte stores of 8 elements where w is a multiple of 8 and the tensors are 16-byte
 *     aligned, element by element otherwise; the split-k partials and the per-level gradients in the workspace stay fp32.
 *   16-byte loads of 8 elements at level 0 where the map is 16-byte aligned and h * w is a multiple of 8, element loads otherwise
 *     (any 2-byte aligned view is served). */
int mpc_corr_pyramid_fwd_dt(const mpc_corr_desc *desc, int D, const void *fmap1, const void *fmap2, int32_t dtype, void *ws, void *stream);
int mpc_corr_pyramid_bwd_dt(const mpc_corr_desc *desc, int D, const void *fmap1, const void *fmap2, void *grad_fmap1, void *grad_fmap2,
                            int32_t dtype, void *ws, void *stream);
int mpc_corr_pyramid_multi_fwd_dt(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int32_t dtype, void *ws, void *stream);
int mpc_corr_pyramid_multi_bwd_dt(const mpc_corr_desc *desc, int D, const mpc_corr_refs *refs, int32_t dtype, void *ws, void *stream);

/* ---- the ground-truth flow targets of the EVIMO2 / MultiFlow configurations (what mpc_val_metrics takes as flow_gt / flow_valid)
 * from the raw multi-step flow, as one launch.
 * Reference: src/loader/evimo2/datasubset.py:171-188 (mode 0), src/loader/multiflow/sample.py:108-139 with downsample=True (mode 1).
 *   mode 0  raw_flow [B][S][2][H][W], (x, y) order, NaN = invalid pixel
 *           valid_src = neither channel NaN (:171); every NaN element -> 0 on its own (:173)
 *           flow [B][S][2][Ho][Wo] (out) = F.interpolate(bilinear, align_corners=False) of the zeroed field: source coordinate
 *             max(fp32(H / Ho) * (j + 0.5) - 0.5, 0), neighbour clamped to the last row, columns blended first, rows last (the
 *             arithmetic of mpc_repr_grid's resize: one shared device function); then channel 0 * fp32(Wo / W), channel 1 *
 *             fp32(Ho / H): one fp32 multiply after the blend (:185-188)
 *           flow_valid [B][S][Ho][Wo] bytes 0 / 1 (out) = F.interpolate(nearest) of valid_src: source index
 *             min(floor(j * fp32(H / Ho)), H - 1), likewise in x (:179-181)
 *           id_out [B][Ho][Wo] (out, has_id = 1) = the same nearest pick of id_mask [B][H][W] (fp32) (:182-184)
 *   mode 1  raw_flow [B][S][H][W][2], channels last as the h5 files hold it (the np.moveaxis of :133 is folded into the read)
 *           flow [B][S][2][Ho][Wo] (out) = F.interpolate(bilinear, align_corners=True): source coordinate fp32((H - 1) / (Ho - 1)) * j,
 *             the same blend order, then * 0.5 (:113, :137).  No NaN treatment (a NaN propagates as in the reference), no validity:
 *             flow_valid, id_mask and id_out are ignored and may be NULL; has_id = 1 is an error.
 * Every output element is written by the kernel (nothing to pre-zero); one kernel on `stream`, no workspace, no memset / memcpy
 * nodes (capturable), nothing read back.  flow must be 4-byte aligned, and flow_valid too (its bytes are stored four at a time);
 * with Wo % 4 == 0 and 16-byte aligned flow (and id_out) the rows are written in 16-byte stores.
 * Limits: B, S, H, W, Ho, Wo >= 1; Ho, Wo >= 2 in mode 1 (the reference divides by Ho - 1): MPC_E_SHAPE otherwise.
 * mpc_flow_targets_supported: the same checks on the host alone, 0 or the error code (+ mpc_last_error_string()).  */
typedef struct mpc_targets_shape { int32_t B, S, H, W, Ho, Wo, mode /* 0 evimo2, 1 multiflow */, has_id; } mpc_targets_shape;
int mpc_flow_targets_supported(const mpc_targets_shape *s);
int mpc_flow_targets(const mpc_targets_shape *s, const float *raw_flow, const float *id_mask,
                     float *flow, uint8_t *flow_valid, float *id_out, void *stream);

/* ---- the DSEC flow files on the device.  png16 [B][H][W][3] uint16 is the 16-bit PNG payload as imageio returns / takes it:
 * channel 0 = x, channel 1 = y, channel 2 = valid.  One kernel each on `stream` (the error: two), no memset / memcpy nodes, nothing
 * read back.  Four pixels (24 B) per thread in 8-byte payload accesses when H * W % 4 == 0 and png16 is 8-byte, the fp32 planes
 * 16-byte (and valid 4-byte) aligned; one pixel per thread otherwise.  B, H, W >= 1, B * H * W < 2^31.
 * mpc_dsec_flow_decode = reference src/loader/dsec/loader.py:174-180: flow [B][2][H][W] (out): channel 0 = (png[..., 1] - 2^15) / 128,
 *   channel 1 = (png[..., 0] - 2^15) / 128 (exact in fp32); valid [B][H][W] bytes 0 / 1 (out) = png[..., 2] != 0 (:178, astype(bool)).
 * mpc_dsec_flow_error = mpc_flow_error (src/utils/flow.py:18-70, src/utils/metrics.py:50-56) with flow_gt and event_mask decoded
 *   from png16 in the load: no fp32 target and no mask are written.  Same per-pixel arithmetic, the same pixels per thread and
 *   order of the sums as mpc_flow_error, hence the same bits.  flow_pred [B][2][H][W]; time_scale [B] or NULL; out[5] (device);
 *   ws: mpc_dsec_flow_error_workspace_bytes(s) bytes; B <= 65535.
 * mpc_dsec_flow_encode = scripts/dsec_inference.py:33-49 (scale_optical_flow + save_flow), flow [B][2][H][W] (y, x) -> png16 (out),
 *   every operation one correctly rounded fp32 operation, no contraction: mag = sqrt(u * u + v * v); where mag > max_magnitude
 *   (strict) u = (u / mag) * max_magnitude and likewise v, both with that one mag; q = u * 128 + 32768 truncated to uint16;
 *   png16[..., 0] = q(x), [..., 1] = q(y), [..., 2] = 0.  UNPINNED: a pixel with a NaN or infinite component gets payload 0 in
 *   both channels; a finite q outside [0, 65535] (only with max_magnitude >= 256) saturates. */
int mpc_dsec_flow_decode(const uint16_t *png16, float *flow, uint8_t *valid, int32_t B, int32_t H, int32_t W, void *stream);
int64_t mpc_dsec_flow_error_workspace_bytes(const mpc_err_shape *s);
int mpc_dsec_flow_error(const mpc_err_shape *s, const uint16_t *png16, const float *flow_pred, const float *time_scale,
                        float *out, void *ws, void *stream);
int mpc_dsec_flow_encode(const float *flow, float max_magnitude, uint16_t *png16, int32_t B, int32_t H, int32_t W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCMAX_H */
