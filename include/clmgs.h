/* clmgs.h -- C ABI of libclmgs_hip.so, the MI355X (gfx950) replacement for the
 * native operators the CLM-GS engines call.
 *
 * Conventions:
 *   - plain C types; every buffer is CALLER-ALLOCATED (device memory unless the
 *     name says host/pinned) and passed as raw pointer + extents;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return 0 on success, non-zero = hipError_t or a CLMGS_E* code; the message
 *     is available (thread-local) from clmgs_last_error();
 *   - no allocation inside, except explicit temp-storage queries: calling a
 *     `*_temp_bytes` function tells the caller how much scratch to pass;
 *   - re-entrant from two host threads on different streams (render thread and
 *     optimizer thread); nothing here holds the Python GIL.
 *
 * Each entry point cites the reference interface it replaces
 * (file:line under the reference tree).  The kernels themselves are absent
 * from the reference (empty submodules), see oracle/gs_oracle.py's header.
 */
#ifndef CLMGS_H
#define CLMGS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLMGS_EINVAL 10001
#define CLMGS_ENOMEM 10002

int clmgs_version(void);
const char* clmgs_last_error(void);

/* ---- gsplat.fully_fused_projection  (strategies/base_engine.py:36-47,139-151;
 *      strategies/no_offload/engine.py:49-60; strategies/clm_offload/engine.py:51-63)
 * means[N,3] quats[N,4] scales[N,3] viewmats[C,4,4] Ks[C,3,3] ->
 * radii[C,N] i32 (0 = culled), means2d[C,N,2], depths[C,N], conics[C,N,3].
 * Any of means2d/depths/conics may be NULL (visibility-only pass). */
int clmgs_projection_fwd(void* stream, int C, int N, const float* means, const float* quats,
                         const float* scales, const float* viewmats, const float* Ks, int width,
                         int height, float eps2d, float near_plane, float far_plane,
                         float radius_clip, int32_t* radii, float* means2d, float* depths,
                         float* conics);
/* The same cull from the RAW parameters (quaternions un-normalised, scales as logs), radii[C,N]
 * only: what calculate_filters (strategies/base_engine.py:18-76) needs, reading each Gaussian
 * once for all C cameras and skipping the exp / normalize passes over N. */
int clmgs_visibility_raw(void* stream, int C, int N, const float* means, const float* quats_raw,
                         const float* log_scales, const float* viewmats, const float* Ks, int width,
                         int height, float eps2d, float near_plane, float far_plane,
                         float radius_clip, int32_t* radii);

/* Visibility filters of a batch selected on the GPU (calculate_filters, base_engine.py:18-76, plus the
 * union "rows the batch touches"), same cull as clmgs_visibility_raw but nothing of size C*N leaves
 * the kernel: _count writes one ballot word + popcount per (camera, 64 Gaussians) into `temp`, scans
 * them and leaves cum_totals[C+1] (device, i64: set bits of cameras 0..r; row C = union over the
 * cameras); the caller reads cum_totals, allocates out[cum_totals[C]] i64 and calls _emit, which
 * writes the ascending Gaussian indices of camera 0, camera 1, ..., then of the union.  1 <= C <= 64
 * (the engines' largest batch); every pair first takes a conservative screen test, only the
 * survivors the exact projection -- the selected sets are the exact test's. */
size_t clmgs_visibility_select_temp_bytes(int C, int N);
int clmgs_visibility_select_count(void* stream, int C, int N, const float* means,
                                  const float* quats_raw, const float* log_scales,
                                  const float* viewmats, const float* Ks, int width, int height,
                                  float eps2d, float near_plane, float far_plane, float radius_clip,
                                  void* temp, size_t temp_bytes, int64_t* cum_totals);
/* The same with what the caller already knows about blocks of 256 consecutive rows: block_flags[ceil(N/256)], 0 = no row
 * of the block passes the cull in any camera (clmgs_adam_small_deferred computes such flags with a superset test).  The
 * flagged-off blocks are not read; the result is the unflagged call's, bit for bit.  NULL: as above. */
int clmgs_visibility_select_count_blocks(void* stream, int C, int N, const float* means, const float* quats_raw,
                                         const float* log_scales, const float* viewmats, const float* Ks, int width,
                                         int height, float eps2d, float near_plane, float far_plane, float radius_clip,
                                         void* temp, size_t temp_bytes, int64_t* cum_totals,
                                         const uint8_t* block_flags);
/* The same over a SELECTED set of blocks: with blk_sel_bits[ceil(N/256)] only the blocks with
 * ((blk_sel_bits[blk] & sel_mask) != 0) == sel_want (0 or 1) are read and get their words written.  scan == 0: the words
 * only (cum_totals may be NULL); a later call on the same `temp` takes the other blocks and, with scan != 0, runs the
 * scan over all words and leaves cum_totals.  Two such calls (sel_want 0, then 1 with scan) leave what one call of
 * clmgs_visibility_select_count_blocks leaves, bit for bit.  blk_sel_bits NULL (then scan must be set): that call. */
int clmgs_visibility_select_count_blocks_sel(void* stream, int C, int N, const float* means, const float* quats_raw,
                                             const float* log_scales, const float* viewmats, const float* Ks, int width,
                                             int height, float eps2d, float near_plane, float far_plane,
                                             float radius_clip, void* temp, size_t temp_bytes, int64_t* cum_totals,
                                             const uint8_t* block_flags, const uint64_t* blk_sel_bits,
                                             uint64_t sel_mask, int sel_want, int scan);
int clmgs_visibility_select_emit(void* stream, int C, int N, const void* temp, int64_t* out);
/* VJP of the above.  v_means[N,3], v_quats[N,4], v_scales[N,3] are overwritten
 * with the sum over the C cameras. */
int clmgs_projection_bwd(void* stream, int C, int N, const float* means, const float* quats,
                         const float* scales, const float* viewmats, const float* Ks, int width,
                         int height, float eps2d, const int32_t* radii, const float* v_means2d,
                         const float* v_depths, const float* v_conics, float* v_means,
                         float* v_quats, float* v_scales);

/* ---- gsplat.fully_fused_projection(calc_compensations=True): clmgs_projection_fwd plus the Mip-Splatting opacity
 * compensation of every pair, compensations[C,N] = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I))), 0 where culled; the
 * determinant of cov2d is formed from the un-blurred entries.  radii, means2d, depths and conics are clmgs_projection_fwd's
 * bit for bit; here every output is required. */
int clmgs_projection_aa_fwd(void* stream, int C, int N, const float* means, const float* quats,
                            const float* scales, const float* viewmats, const float* Ks, int width,
                            int height, float eps2d, float near_plane, float far_plane,
                            float radius_clip, int32_t* radii, float* means2d, float* depths,
                            float* conics, float* compensations);
/* Its VJP: clmgs_projection_bwd with one more cotangent, v_compensations[C,N] (NULL = zeros), in gsplat's guarded form:
 * the square root's derivative is taken as 0.5 / (compensation + 1e-6). */
int clmgs_projection_aa_bwd(void* stream, int C, int N, const float* means, const float* quats,
                            const float* scales, const float* viewmats, const float* Ks, int width,
                            int height, float eps2d, const int32_t* radii, const float* v_means2d,
                            const float* v_depths, const float* v_conics, const float* v_compensations,
                            float* v_means, float* v_quats, float* v_scales);

/* ---- gsplat.fully_fused_projection(camera_model="ortho") and rasterization(camera_model="ortho"): the orthographic
 * projection.  Ks[c] = [[sx,0,cx],[0,sy,cy],[0,0,1]] with sx, sy in pixels per world unit; with p = R m + t,
 * means2d = (sx p.x + cx, sy p.y + cy), depths = p.z, cov2d = J Sc J^T + eps2d I with the constant
 * J = [[sx,0,0],[0,sy,0]] (no perspective divide, no frustum clamp); near / far plane, radius, radius_clip, the
 * off-screen tests and the conic are clmgs_projection_fwd's.  The arguments are clmgs_projection_aa_fwd's; means2d,
 * depths, conics and compensations are each optional (all NULL: the cull alone, radii only -- visibility_radii).
 * Culled pairs: radius 0 and zero floats.  N == 0 returns 0 before any pointer check. */
int clmgs_projection_ortho_fwd(void* stream, int C, int N, const float* means, const float* quats,
                               const float* scales, const float* viewmats, const float* Ks, int width,
                               int height, float eps2d, float near_plane, float far_plane,
                               float radius_clip, int32_t* radii, float* means2d, float* depths,
                               float* conics, float* compensations);
/* Its VJP: the arguments of clmgs_projection_aa_bwd; v_depths and v_compensations optional (NULL = zeros), the
 * compensation's cotangent in gsplat's guarded form.  No view-matrix gradient exists for this model. */
int clmgs_projection_ortho_bwd(void* stream, int C, int N, const float* means, const float* quats,
                               const float* scales, const float* viewmats, const float* Ks, int width,
                               int height, float eps2d, const int32_t* radii, const float* v_means2d,
                               const float* v_depths, const float* v_conics, const float* v_compensations,
                               float* v_means, float* v_quats, float* v_scales);

/* ---- gsplat.spherical_harmonics  (base_engine.py:161-163; no_offload/engine.py:67-69;
 *      clm_offload/engine.py:73-76)
 * dirs[n,3] (un-normalised), coeffs[n,16,3], masks[n] u8 or NULL -> colors[n,3]. */
int clmgs_sh_fwd(void* stream, int n, int degree, const float* dirs, const float* coeffs,
                 const uint8_t* masks, float* colors);
/* v_coeffs[n,16,3]: accumulate != 0 adds into the buffer (this is
 * clm_kernels.spherical_harmonics_bwd_inplace, clm_offload/engine.py:709-716),
 * else overwrites (rows beyond the active degree = 0).  v_dirs[n,3] may be NULL. */
int clmgs_sh_bwd(void* stream, int n, int degree, const float* dirs, const float* coeffs,
                 const uint8_t* masks, const float* v_colors, float* v_coeffs, int accumulate,
                 float* v_dirs);

/* ---- gsplat.isect_tiles / isect_offset_encode  (base_engine.py:175-186)
 * Phase 1: tiles_per_gauss[C*N] i32 and its inclusive prefix sum cum[C*N] i64.
 * The caller reads cum[C*N-1] (= I) and allocates isect buffers. */
size_t clmgs_isect_count_temp_bytes(int CN);
int clmgs_isect_count(void* stream, int C, int N, const float* means2d, const int32_t* radii,
                      int tile_size, int tile_width, int tile_height, int32_t* tiles_per_gauss,
                      int64_t* cum, void* temp, size_t temp_bytes);
/* Phase 2: emit + sort.  isect_ids[I] i64 = (cam << tile_bits | tile) << 32 | depth bits,
 * flatten_ids[I] i32 = cam*N + gaussian, both sorted by key (stable). */
size_t clmgs_isect_sort_temp_bytes(int64_t n_isects);
int clmgs_isect_emit_sort(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                          const int32_t* radii, const float* depths, const int64_t* cum,
                          int tile_size, int tile_width, int tile_height, int64_t* isect_ids,
                          int32_t* flatten_ids, void* temp, size_t temp_bytes);
/* offsets[C*tile_h*tile_w] i32 = first sorted index of each (cam,tile). */
int clmgs_isect_offsets(void* stream, int64_t n_isects, const int64_t* isect_ids, int C,
                        int tile_width, int tile_height, int32_t* offsets);

/* ---- two-level binning (engine fast path; single camera).  Same (tile, depth, row) order as
 * clmgs_isect_emit_sort, ~1/4 of its traffic: A = stable depth sort of the V rows + tile counts
 * in that order (order[V] i32, cum[V] i64 inclusive; caller reads cum[V-1] = I);
 * B = emit in depth order + ONE stable sort on the tile-id bits -> flatten_ids[I] i32 (row ids),
 * offsets[tile_w*tile_h] i32, and isect_ids[I] i64 if non-NULL.
 * row_cum[V] (i64, optional, from order_count): inclusive counts of the EMITTED intersections in ROW
 * order; with it emit_sort also returns emit_slot[I] (i32): the slot of every sorted intersection,
 * row i owning the contiguous slots [row_cum[i-1], row_cum[i]) -- hand emit_slot to
 * clmgs_rasterize_bwd (which STORES one partial-gradient line per slot) and row_cum to whoever sums the
 * rows (clmgs_preprocess_bwd, or clmgs_rasterize_bwd's own row-sum pass): atomic-free, deterministic. */
size_t clmgs_isect2_order_temp_bytes(int V);
int clmgs_isect2_order_count(void* stream, int V, const float* means2d, const int32_t* radii,
                             const float* depths, int tile_size, int tile_width, int tile_height,
                             const void* packed, int32_t* order, int64_t* cum, uint64_t* boxes,
                             int64_t* totals, void* temp, size_t temp_bytes, int64_t* row_cum);
size_t clmgs_isect2_sort_temp_bytes(int64_t n_isects);
int clmgs_isect2_emit_sort(void* stream, int V, int64_t n_isects, const float* depths,
                           const int32_t* order, const int64_t* cum, const uint64_t* boxes,
                           int tile_width, int tile_height, int32_t* flatten_ids, int32_t* offsets,
                           int64_t* isect_ids, int32_t* emit_slot, void* temp, size_t temp_bytes,
                           const int64_t* row_cum);

/* ---- gsplat.rasterize_to_pixels  (base_engine.py:192-203)
 * means2d[C*N,2] conics[C*N,3] colors[C*N,3] opacities[C*N], backgrounds[C,3] or NULL ->
 * render_colors[C,H,W,3], render_alphas[C,H,W], last_ids[C,H,W] i32.  tile_size must be 16.
 * `packed` is caller scratch of clmgs_rasterize_pack_bytes(C,N) bytes (64 B aligned): fwd fills it
 * with one 64 B raster record per Gaussian and the tile kernels gather that one line; keep it for
 * the backward call.  means2d == NULL: `packed` already holds the records (clmgs_preprocess_fwd). */
size_t clmgs_rasterize_pack_bytes(int C, int N);
int clmgs_rasterize_fwd(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                        const float* conics, const float* colors, const float* opacities,
                        const float* backgrounds, int width, int height, int tile_size,
                        int tile_width, int tile_height, const int32_t* offsets,
                        const int32_t* flatten_ids, void* packed, float* render_colors,
                        float* render_alphas, int32_t* last_ids);
/* VJP.  packed = the forward's record buffer; packed_grad = scratch of the same size, one 64 B
 * gradient line per Gaussian (x y ca cb | cc r g b | o).  Two accumulation modes:
 *   - emit_slot == NULL: packed_grad is zeroed here and the per-(Gaussian,tile) sums are added
 *     with float atomics (any flatten_ids / offsets, C >= 1);
 *   - emit_slot from clmgs_isect2_emit_sort (C == 1) + `partials` scratch of
 *     clmgs_rasterize_partials_bytes(n_isects) bytes (64 B lines, 16 B aligned): every (Gaussian,tile) sum is
 *     STORED at its slot (every slot is written exactly once, zeros included) -- no atomics (they
 *     bound the kernel: 4.05 -> ~2 ms at 12 M intersections), bitwise reproducible gradients.  With
 *     packed_grad != NULL (+ row_cum from clmgs_isect2_order_count) a row-order pass then adds each row's
 *     contiguous slot range into packed_grad; with packed_grad == NULL the partial lines are the
 *     result and clmgs_preprocess_bwd(partials, row_cum) sums them on the fly (engine path).
 * v_means2d[C*N,2] v_conics[C*N,3] v_colors[C*N,3] v_opacities[C*N] are OVERWRITTEN;
 * v_means2d == NULL skips the unpack (the caller reads packed_grad / the partial lines). */
size_t clmgs_rasterize_partials_bytes(int64_t n_isects);
int clmgs_rasterize_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                        const float* backgrounds, int width, int height, int tile_size,
                        int tile_width, int tile_height, const int32_t* offsets,
                        const int32_t* flatten_ids, const float* render_alphas,
                        const int32_t* last_ids, const float* v_render_colors,
                        const float* v_render_alphas, void* packed_grad, float* v_means2d,
                        float* v_conics, float* v_colors, float* v_opacities,
                        const int32_t* emit_slot, const int64_t* row_cum, void* partials);

/* ---- per-Gaussian blend weights (contribution pruning; csrc/contrib.hip)
 * A forward-only walk of the same lists with the forward's blend rules, no colours.  means2d[C*N,2] conics[C*N,3]
 * opacities[C*N], offsets / flatten_ids as for clmgs_rasterize_fwd, C >= 1, tile_size 16.  For every (Gaussian, tile)
 * entry, over the in-image pixels at which clmgs_rasterize_fwd accumulates it, with w = alpha * T:
 *   wsum_q[r]    += round_to_nearest(2^28 * sum w)    uint64 fixed point, unit 2^-28
 *   wmax_bits[r]  = max(wmax_bits[r], bits(max w))     uint32: the bit pattern of a non-negative float
 *   pixels[r]    += number of those pixels             uint64
 * by integer atomics only: the arrays are bit-reproducible.  The entry ADDS: the caller zeroes the three arrays (n_out
 * elements each) once and may call camera after camera.  Destination row r of Gaussian g of camera cam: rows[g] with
 * `rows` (int64[N], one table for all C cameras), cam * N + g with rows == NULL (then n_out >= C*N).  A row outside
 * [0, n_out) is dropped.  Entries that are culled, never reached or valid at no pixel touch nothing.
 * `packed`: caller scratch of clmgs_rasterize_contrib_pack_bytes(C,N) bytes (32 B aligned), filled here with one 32 B
 * record per Gaussian.  Argument errors return CLMGS_EINVAL before anything is written; n_isects == 0 is accepted and
 * writes nothing. */
size_t clmgs_rasterize_contrib_pack_bytes(int C, int N);
int clmgs_rasterize_contrib(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                            const float* conics, const float* opacities, int width, int height,
                            int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                            const int32_t* flatten_ids, const int64_t* rows, int64_t n_out, void* packed,
                            uint64_t* wsum_q, uint32_t* wmax_bits, uint64_t* pixels);

/* ---- median depth (surface depth for mesh export; csrc/median.hip)
 * A forward-only walk of the same lists with the forward's blend rules, no colours, which stops where the transmittance
 * has fallen to one half.  means2d[C*N,2] conics[C*N,3] opacities[C*N] depths[C*N] (camera-space depth), offsets /
 * flatten_ids as for clmgs_rasterize_fwd, C >= 1, tile_size 16.  The median entry of a pixel is the last entry that
 * clmgs_rasterize_fwd accumulates there while the transmittance before it is > 0.5: the entry at which T crosses one
 * half, or the pixel's last contributor where the final T stays above it.
 *   median_depth[C,H,W]  depths[] of that entry, copied; 0.0 where nothing is accumulated
 *   median_id[C,H,W]     its row within its camera, flatten_id - cam * N; -1 where nothing is accumulated
 * Every pixel is written exactly once, nothing else is; no atomics: the maps are bit-reproducible.  A list entry whose
 * id is not a row of its camera reads and writes nothing.  Not differentiable.
 * `packed`: caller scratch of clmgs_rasterize_median_pack_bytes(C,N) bytes (32 B aligned), filled here with one 32 B
 * record per Gaussian.  Argument errors return CLMGS_EINVAL before anything is written; n_isects == 0 or N == 0 is
 * accepted and writes 0.0 / -1 to every pixel. */
size_t clmgs_rasterize_median_pack_bytes(int C, int N);
int clmgs_rasterize_median(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                           const float* conics, const float* opacities, const float* depths, int width, int height,
                           int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                           const int32_t* flatten_ids, void* packed, float* median_depth, int32_t* median_id);

/* ---- ray depth (csrc/ray_depth.hip, csrc/ray_math.h; DESIGN.md section 3, "Ray depth")
 * The ray-Gaussian intersection depth of RaDe-GS (Zhang et al. 2024, "Rasterizing Depth in Gaussian Splatting") and GOF
 * (Yu et al. 2024, "Gaussian Opacity Fields"): the depth of the point on a pixel's ray at which a Gaussian's 3-D density
 * exp(-0.5 (x - m)^T S^-1 (x - m)) is largest,  t* = d^T S^-1 (m - o) / d^T S^-1 d,  evaluated for the pixel's MEDIAN
 * Gaussian (clmgs_rasterize_median's median_id) instead of that Gaussian's centre depth.  Per pixel, not blended over
 * the pixel's contributors.  Forward-only, not differentiable.
 *   means[N,3] quats[N,4] (w,x,y,z; normalised here) scales[N,3] (ACTIVATED, as clmgs_projection_fwd takes
 *   them): the rows every camera indexes;  cams: DEVICE array [C,16] of doubles, per camera the top 3x4 of the view matrix
 *   (row-major) then fx, fy, cx, cy;  median_id int32 [C,H,W]: the row within its camera;  median_depth[C,H,W]: the
 *   depth returned where t* is unusable;  camera_model 0 = pinhole (origin 0, direction (u, v, 1)), 1 = orthographic
 *   (K in pixels per world unit: origin (u, v, 0), direction (0, 0, 1)), u = (x + 0.5 - cx) / fx, v = (y + 0.5 - cy) / fy.
 *   ray_depth[C,H,W] = (float) t* where t* is finite and > near_plane, else median_depth[] of the pixel, copied; 0.0 where
 *   the id lies outside [0, N): such a pixel reads no row.  float64 arithmetic without contraction (ray_math.h): bit-
 *   reproducible, every pixel written exactly once, no atomics.
 * Argument errors (a negative size, C H W or the grid beyond 2^31 - 1, camera_model outside 0..1, a null or misaligned
 * pointer) return CLMGS_EINVAL before anything is written; C H W == 0 is a no-op, N == 0 writes 0.0 to every pixel. */
int clmgs_ray_depth(void* stream, int C, int N, int height, int width, const float* means, const float* quats,
                    const float* scales, const double* cams, const int32_t* median_id, const float* median_depth,
                    double near_plane, int camera_model, float* ray_depth);

/* ---- gsplat.rasterize_to_pixels with colors[..., 4]  (what gsplat's rasterization(render_mode="RGB+D" / "RGB+ED")
 * calls: the camera-space depth rides as a fourth colour channel and is blended with the same weights)
 * Same contract as clmgs_rasterize_fwd / _bwd with rows of four: colors[C*N,4], backgrounds[C,4] or NULL ->
 * render_colors[C,H,W,4]; v_render_colors[C,H,W,4] -> v_colors[C*N,4].  `packed` / `packed_grad` have the same
 * sizes (clmgs_rasterize_pack_bytes): the fourth channel travels in the record's spare word next to blue, its
 * gradient in word 9 of the gradient line (x y ca cb | cc r g b | o d).  Channels 0..2, render_alphas and last_ids
 * are bit-identical to clmgs_rasterize_fwd on the same inputs.  means2d == NULL: `packed` already holds 4-channel
 * records (an earlier clmgs_rasterize4_fwd; clmgs_preprocess_fwd writes 3-channel ones, fourth word 0).
 * clmgs_rasterize4_bwd: the atomic route only -- emit_slot or partials != NULL returns CLMGS_EINVAL before anything is
 * written.  The slot route of four channels is clmgs_rasterize4_slot_bwd: clmgs_rasterize_bwd's slot contract (C == 1,
 * emit_slot, partials required; packed_grad + row_cum optional), the stored line is  x y ca cb | cc r g b | o d - -
 * (zero lines stay zero), and the optional per-row sum carries word 9.  Absgrad with four channels is not built. */
int clmgs_rasterize4_fwd(void* stream, int C, int N, int64_t n_isects, const float* means2d,
                         const float* conics, const float* colors, const float* opacities,
                         const float* backgrounds, int width, int height, int tile_size,
                         int tile_width, int tile_height, const int32_t* offsets,
                         const int32_t* flatten_ids, void* packed, float* render_colors,
                         float* render_alphas, int32_t* last_ids);
int clmgs_rasterize4_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                         const float* backgrounds, int width, int height, int tile_size,
                         int tile_width, int tile_height, const int32_t* offsets,
                         const int32_t* flatten_ids, const float* render_alphas,
                         const int32_t* last_ids, const float* v_render_colors,
                         const float* v_render_alphas, void* packed_grad, float* v_means2d,
                         float* v_conics, float* v_colors, float* v_opacities,
                         const int32_t* emit_slot, const int64_t* row_cum, void* partials);
int clmgs_rasterize4_slot_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                              const float* backgrounds, int width, int height, int tile_size,
                              int tile_width, int tile_height, const int32_t* offsets,
                              const int32_t* flatten_ids, const float* render_alphas,
                              const int32_t* last_ids, const float* v_render_colors,
                              const float* v_render_alphas, void* packed_grad, float* v_means2d,
                              float* v_conics, float* v_colors, float* v_opacities,
                              const int32_t* emit_slot, const int64_t* row_cum, void* partials);

/* ---- gsplat.rasterize_to_pixels(absgrad=True) -> means2d.absgrad  (AbsGS; consumed by gsplat's
 * DefaultStrategy(absgrad=True)): next to the signed screen-space gradient, the sum over the pixels p at which the
 * Gaussian contributes of the per-pixel magnitudes,  absgrad = sum_p ( |dL_p/dmean2d.x| , |dL_p/dmean2d.y| ).
 * Same contract and arguments as clmgs_rasterize_bwd, three channels, both accumulation modes.  The 64 B gradient line
 * and the slot route's partial line become   x y ca cb | cc r g b | o - ax ay   (words 10 and 11 hold the pair; word 9
 * stays the fourth channel's); every other word is what clmgs_rasterize_bwd writes.  v_means2d_abs[C*N,2] (optional,
 * needs v_means2d) is OVERWRITTEN with the unpack. */
int clmgs_rasterize_abs_bwd(void* stream, int C, int N, int64_t n_isects, const void* packed,
                            const float* backgrounds, int width, int height, int tile_size,
                            int tile_width, int tile_height, const int32_t* offsets,
                            const int32_t* flatten_ids, const float* render_alphas,
                            const int32_t* last_ids, const float* v_render_colors,
                            const float* v_render_alphas, void* packed_grad, float* v_means2d,
                            float* v_conics, float* v_colors, float* v_opacities,
                            const int32_t* emit_slot, const int64_t* row_cum, void* partials,
                            float* v_means2d_abs);

/* ---- device-count forms (engine fast path): the data-dependent size I of a camera need not reach the host
 * before the consumers of the list are enqueued.  The reference reads it back synchronously
 * (strategies/base_engine.py:64-69 `counts.cpu()`, gsplat.isect_tiles' cum[-1].item()); here `capacity` (a
 * prediction by the caller, >= the true count or the camera is redone) sizes every buffer and launch, and
 * the TRUE count is read ON THE DEVICE from n_isects_dev = totals[0] of clmgs_isect2_order_count.
 * Intersections beyond the capacity are dropped (never written out of bounds); the caller compares the count
 * with the capacity from its asynchronous readback and, if it was exceeded, repeats the camera with the exact
 * forms above before anything was accumulated.  Same results as the exact forms when count <= capacity
 * (tests/test_gpu_ops.py).  rasterize_*_dev: slot mode only (C == 1, records in `packed`, partial lines out). */
int clmgs_isect2_emit_sort_dev(void* stream, int V, int64_t capacity, const int64_t* n_isects_dev,
                               const float* depths, const int32_t* order, const int64_t* cum,
                               const uint64_t* boxes, int tile_width, int tile_height,
                               int32_t* flatten_ids, int32_t* offsets, int64_t* isect_ids,
                               int32_t* emit_slot, void* temp, size_t temp_bytes, const int64_t* row_cum);

/* Tile-major binning (round 5; the engine's default route): the same lists as clmgs_isect2_order_count +
 * clmgs_isect2_emit_sort -- gsplat.isect_tiles + isect_offset_encode of strategies/base_engine.py:175-186, sorted by
 * (tile, depth bits, row index) -- built without a global sort: per-tile counters, an exclusive scan (= offsets), a
 * scatter of 16 B records into the tiles' segments and one LDS sort per tile (csrc/isect3.hip).  8 kernel launches and one
 * clear instead of 23.
 *  - clmgs_isect3_front: per-row tile boxes / exact tile masks (packed != NULL), tile counters, row_cum[V] (inclusive
 *    emitted counts in ROW order = the slot ranges of clmgs_rasterize_bwd's slot mode), totals[2] on the device =
 *    {intersections to emit, un-culled count}.  `temp` (clmgs_isect3_front_temp_bytes) must stay alive until _bin ran.
 *  - clmgs_isect3_bin: offsets[tile_w*tile_h], flatten_ids[I], emit_slot[I] (optional), isect_ids[I] (optional) from the
 *    front half's temp; n_isects = totals[0] read back by the caller.
 *  - clmgs_isect3_bin_dev: device-count form (see clmgs_isect2_emit_sort_dev): buffers and launches sized for
 *    `capacity`, the true count read on the device; above the capacity the lists are memory-safe but incomplete and
 *    the caller redoes the camera. */
size_t clmgs_isect3_front_temp_bytes(int V, int n_tiles);
int clmgs_isect3_front(void* stream, int V, const float* means2d, const int32_t* radii, int tile_size, int tile_width,
                       int tile_height, const void* packed, int64_t* totals, int64_t* row_cum, void* temp,
                       size_t temp_bytes);
size_t clmgs_isect3_bin_temp_bytes(int64_t n_isects, int n_tiles);
int clmgs_isect3_bin(void* stream, int V, int64_t n_isects, const float* depths, int tile_width, int tile_height,
                     const int64_t* row_cum, const void* front_temp, int32_t* flatten_ids, int32_t* offsets,
                     int64_t* isect_ids, int32_t* emit_slot, void* temp, size_t temp_bytes);
int clmgs_isect3_bin_dev(void* stream, int V, int64_t capacity, const int64_t* n_isects_dev, const float* depths,
                         int tile_width, int tile_height, const int64_t* row_cum, const void* front_temp,
                         int32_t* flatten_ids, int32_t* offsets, int64_t* isect_ids, int32_t* emit_slot, void* temp,
                         size_t temp_bytes);
int clmgs_rasterize_fwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                            const float* backgrounds, int width, int height, int tile_size,
                            int tile_width, int tile_height, const int32_t* offsets,
                            const int32_t* flatten_ids, void* packed, float* render_colors,
                            float* render_alphas, int32_t* last_ids);
int clmgs_rasterize_bwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                            const void* packed, const float* backgrounds, int width, int height,
                            int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                            const int32_t* flatten_ids, const float* render_alphas,
                            const int32_t* last_ids, const float* v_render_colors,
                            const float* v_render_alphas, const int32_t* emit_slot,
                            const int64_t* row_cum, void* partials);

/* Four channels, device-count forms: the contracts of clmgs_rasterize_fwd_dev / _bwd_dev with render_colors /
 * v_render_colors rows of 4, backgrounds[C,4] or NULL, the fourth colour in word 9 of every record of `packed`
 * (clmgs_invdepth_pack) and its gradient in word 9 of every partial line. */
int clmgs_rasterize4_fwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                             const float* backgrounds, int width, int height, int tile_size,
                             int tile_width, int tile_height, const int32_t* offsets,
                             const int32_t* flatten_ids, void* packed, float* render_colors,
                             float* render_alphas, int32_t* last_ids);
int clmgs_rasterize4_bwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                             const void* packed, const float* backgrounds, int width, int height,
                             int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                             const int32_t* flatten_ids, const float* render_alphas,
                             const int32_t* last_ids, const float* v_render_colors,
                             const float* v_render_alphas, const int32_t* emit_slot,
                             const int64_t* row_cum, void* partials);

/* gsplat's absgrad, device-count form of the slot mode: clmgs_rasterize_bwd_dev whose partial lines carry the pair in
 * words 10 and 11 (x y ca cb | cc r g b | o - ax ay), for clmgs_preprocess_abs_bwd to sum. */
int clmgs_rasterize_abs_bwd_dev(void* stream, int C, int N, int64_t capacity, const int64_t* n_isects_dev,
                                const void* packed, const float* backgrounds, int width, int height,
                                int tile_size, int tile_width, int tile_height, const int32_t* offsets,
                                const int32_t* flatten_ids, const float* render_alphas,
                                const int32_t* last_ids, const float* v_render_colors,
                                const float* v_render_alphas, const int32_t* emit_slot,
                                const int64_t* row_cum, void* partials);

/* ---- fused per-camera front end (engine-internal fast path; same arithmetic as the op chain
 * strategies/clm_offload/engine.py:650-691 forward and :703-742 + densification.py:59-102 backward)
 * For i < V, row g = filter ? filter[i] : i of the RAW parameter tensors (xyz[N,3], opacity_raw[N],
 * scaling_raw[N,3], rotation_raw[N,4]); SH rows from sh_rows[g] (sh_by_filter) or sh_rows[i].
 * viewmat[16] (row-major world->camera), K[9], campos[3] are HOST pointers (copied into the launch).
 * fwd: exp / sigmoid, projection, SH colour, +0.5 clamp -> radii[V] means2d[V,2] depths[V]
 * conics[V,3] colors[V,3] opacities[V] and the packed raster records packed[V,16].
 * bwd: from packed_grad[V,16] -- or, packed_grad == NULL, from the partial lines `partials` of
 * clmgs_rasterize_bwd, row i summing the lines [row_cum[i-1], row_cum[i]) in ascending order --
 * ACCUMULATES into g_xyz[N,3] g_opacity[N] g_scaling[N,3]
 * g_rotation[N,4] (raw-parameter gradients) and g_sh_rows (indexed like sh_rows), and, if
 * max_radii2D != NULL, updates the densification statistics of every filter row (or, with
 * stats_only_visible, of the rows with radius > 0: densification.py:105-147). */
/* Packed small attributes: opacity_raw == scaling_raw == rotation_raw == NULL means `xyz` is the
 * 16 B-aligned [N,12] table  xyz 3 | opacity 1 | scaling 3 | rotation 4 | pad  (one 48 B row per
 * Gaussian instead of four scattered pieces, each of which costs a 64 B line); in the backward the
 * gradient outputs follow the same convention (g_opacity == g_scaling == g_rotation == NULL:
 * g_xyz is the packed [N,12] gradient table), and packed parameters go with packed gradients.
 * Statistics: grad_accum == denom == NULL with max_radii2D != NULL means max_radii2D is a 16 B-aligned
 * [N,4] table  max radius | grad accum | count | pad  (one row instead of three scattered floats).
 * sh_index[V] (i32, optional, with sh_by_filter = 1): position i reads SH row sh_rows[sh_index[i]] and
 * accumulates into g_sh_rows[sh_index[i]] -- sh_rows is then a staging table holding only the rows a
 * batch touches (host-resident mode: clm_offload/engine.py:494-508 moves rows host -> GPU per batch).
 * sh_stamp[N] (i32, optional, bwd with sh_by_filter = 1) + cur_step: FIRST-TOUCH stores.  sh_stamp[row]
 * is the optimizer step whose gradient g_sh_rows[row] holds; a row whose stamp differs from cur_step is
 * STORED (its previous content was consumed -- clmgs_adam_catch_up(keep_grad = 1) does not clear it) and
 * stamped cur_step, later cameras of the same step accumulate.  sh_stamp doubles as the deferred
 * optimizer's g_step table.  The reference clears the whole gradient buffer every batch
 * (clm_offload/engine.py:870-882) and accumulates (send_shs2cpu_grad_buffer_stream, accum = True).
 * At degree d < 3 both policies touch only the row's first ceil(3 (d+1)^2 / 4) float4s; the rest of the 48 floats
 * is neither read nor written ("Gradient rows are stored on first touch": why nothing stale waits there).
 * Both launches run min(ceil(V / 64), clmgs_preprocess_grid_cap()) one-wave workgroups of 64 rows; above 64 x the cap
 * a wave takes further chunks, grid-stride. */
int clmgs_preprocess_grid_cap(void);
int clmgs_preprocess_fwd(void* stream, int V, const int64_t* filter, const float* xyz,
                         const float* opacity_raw, const float* scaling_raw,
                         const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                         const float* viewmat_host, const float* K_host, const float* campos_host,
                         int width, int height, int degree, float eps2d, float near_plane,
                         float far_plane, float radius_clip, int32_t* radii, float* means2d,
                         float* depths, float* conics, float* colors, float* opacities, void* packed,
                         const int32_t* sh_index);
int clmgs_preprocess_bwd(void* stream, int V, const int64_t* filter, const float* xyz,
                         const float* opacity_raw, const float* scaling_raw,
                         const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                         const float* viewmat_host, const float* K_host, const float* campos_host,
                         int width, int height, int degree, float eps2d, const int32_t* radii,
                         const void* packed_grad, float* g_xyz, float* g_opacity, float* g_scaling,
                         float* g_rotation, float* g_sh_rows, float* max_radii2D, float* grad_accum,
                         float* denom, float* v_means2d_out, int stats_only_visible,
                         const void* partials, const int64_t* row_cum, const int32_t* sh_index,
                         int32_t* sh_stamp, int cur_step);

/* gsplat's absgrad (DefaultStrategy(absgrad=True); AbsGS): clmgs_preprocess_bwd on the lines of clmgs_rasterize_abs_bwd /
 * _abs_bwd_dev,  x y ca cb | cc r g b | o - ax ay  (packed_grad[V,16] or the partial lines).  Words 10 and 11 are summed
 * per row in the same ascending slot order as the rest of the line, and the densification statistic becomes
 *   grad_accum += sqrt((ax * width / 2)^2 + (ay * height / 2)^2)
 * in place of the same norm of the signed x y.  Every gradient, denom and max_radii2D are clmgs_preprocess_bwd's bit for
 * bit.  v_means2d_abs_out[V,2] (optional) mirrors v_means2d_out. */
int clmgs_preprocess_abs_bwd(void* stream, int V, const int64_t* filter, const float* xyz,
                             const float* opacity_raw, const float* scaling_raw,
                             const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                             const float* viewmat_host, const float* K_host, const float* campos_host,
                             int width, int height, int degree, float eps2d, const int32_t* radii,
                             const void* packed_grad, float* g_xyz, float* g_opacity, float* g_scaling,
                             float* g_rotation, float* g_sh_rows, float* max_radii2D, float* grad_accum,
                             float* denom, float* v_means2d_out, int stats_only_visible,
                             const void* partials, const int64_t* row_cum, const int32_t* sh_index,
                             int32_t* sh_stamp, int cur_step, float* v_means2d_abs_out);

/* gsplat's rasterization(rasterize_mode="antialiased") (Mip-Splatting): the fused front end with the opacity compensation
 * of clmgs_projection_aa_fwd.  Argument lists are those of the plain counterparts.
 * fwd: the opacity word of the record and opacities[V] are sigmoid(opacity_raw) * compensation (the binning's tile-mask
 * test reads the record, so it follows); radii, means2d, depths, conics and colours are clmgs_preprocess_fwd's bit for bit.
 * bwd (records written by _aa_fwd): with go the row's summed opacity word and op = sigmoid(opacity_raw),
 *   g_opacity += go * compensation * op (1 - op),   v_compensation = go * op
 * and v_compensation enters the projection VJP as in clmgs_projection_aa_bwd.  Statistics are the plain entry's.
 * _aa_abs_bwd: _aa_bwd's gradients bit for bit, the statistic from the abs pair as in clmgs_preprocess_abs_bwd. */
int clmgs_preprocess_aa_fwd(void* stream, int V, const int64_t* filter, const float* xyz,
                            const float* opacity_raw, const float* scaling_raw,
                            const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                            const float* viewmat_host, const float* K_host, const float* campos_host,
                            int width, int height, int degree, float eps2d, float near_plane,
                            float far_plane, float radius_clip, int32_t* radii, float* means2d,
                            float* depths, float* conics, float* colors, float* opacities, void* packed,
                            const int32_t* sh_index);
int clmgs_preprocess_aa_bwd(void* stream, int V, const int64_t* filter, const float* xyz,
                            const float* opacity_raw, const float* scaling_raw,
                            const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                            const float* viewmat_host, const float* K_host, const float* campos_host,
                            int width, int height, int degree, float eps2d, const int32_t* radii,
                            const void* packed_grad, float* g_xyz, float* g_opacity, float* g_scaling,
                            float* g_rotation, float* g_sh_rows, float* max_radii2D, float* grad_accum,
                            float* denom, float* v_means2d_out, int stats_only_visible,
                            const void* partials, const int64_t* row_cum, const int32_t* sh_index,
                            int32_t* sh_stamp, int cur_step);
int clmgs_preprocess_aa_abs_bwd(void* stream, int V, const int64_t* filter, const float* xyz,
                                const float* opacity_raw, const float* scaling_raw,
                                const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                                const float* viewmat_host, const float* K_host, const float* campos_host,
                                int width, int height, int degree, float eps2d, const int32_t* radii,
                                const void* packed_grad, float* g_xyz, float* g_opacity, float* g_scaling,
                                float* g_rotation, float* g_sh_rows, float* max_radii2D, float* grad_accum,
                                float* denom, float* v_means2d_out, int stats_only_visible,
                                const void* partials, const int64_t* row_cum, const int32_t* sh_index,
                                int32_t* sh_stamp, int cur_step, float* v_means2d_abs_out);

/* ---- clm_kernels.fused_ssim  (base_engine.py:5,93; definition utils/loss_utils.py:26-85)
 * img1,img2 [B,CH,H,W].  fwd adds per-block SSIM-map sums into ssim_sum[1024] (caller zeroes
 * it; mean = sum of the 1024 slots / (B*CH*H*W)) and, when the three dm_* maps are non-NULL, the
 * partial derivatives needed by bwd.  bwd writes v_img1 = v_mean[0] * inv_numel * dSSIM_sum/dimg1
 * (v_mean is a DEVICE scalar: the upstream cotangent never visits the host). */
int clmgs_ssim_fwd(void* stream, int B, int CH, int H, int W, const float* img1,
                   const float* img2, float* ssim_sum, float* dm_dmu1, float* dm_dsigma1_sq,
                   float* dm_dsigma12);
int clmgs_ssim_bwd(void* stream, int B, int CH, int H, int W, const float* img1,
                   const float* img2, const float* v_mean, float inv_numel, const float* dm_dmu1,
                   const float* dm_dsigma1_sq, const float* dm_dsigma12, float* v_img1);

/* ---- fused training loss  (strategies/base_engine.py:79-103: FusedCompiledLoss + loss_combined)
 * loss = (1 - lambda) * mean|img - gt| + lambda * (1 - SSIM(img, gt)), gt = clamp(gt_u8 / 255).
 * img is a [3,H,W] VIEW given by its element strides (so the rasterizer's [H,W,3] output is read
 * in place); gt_u8 is planar [3,H,W].  fwd adds per-block (sum|x-y|, sum SSIM) pairs into
 * partials[2 * clmgs_loss_slots()] (caller zeroes; total = column sums) and, if m1..m3 != NULL,
 * writes the three [3,H,W] derivative maps bwd needs.  bwd writes v_img with img's strides;
 * v_loss is a DEVICE scalar. */
int clmgs_loss_slots(void);
int clmgs_l1_ssim_loss_fwd(void* stream, int H, int W, const float* img, int64_t stride_c,
                           int64_t stride_y, int64_t stride_x, const uint8_t* gt_u8,
                           float* partials, float* m1, float* m2, float* m3);
int clmgs_l1_ssim_loss_bwd(void* stream, int H, int W, const float* img, int64_t stride_c,
                           int64_t stride_y, int64_t stride_x, const uint8_t* gt_u8,
                           const float* v_loss, float lambda_dssim, const float* m1,
                           const float* m2, const float* m3, float* v_img);
/* Masked forms: the same loss with a per-pixel ignore mask, mask[H,W] uint8 planar (0 = ignored, any other value =
 * counted; required non-NULL), shared by the three channels:
 *   loss = (1 - lambda) * sum m |img - gt| / (3 H W) + lambda * sum m (1 - ssim_map) / (3 H W).
 * The SSIM window statistics are those of the whole, unmasked images and the divisor stays 3 H W.  fwd adds the two
 * sums over COUNTED pixels only (the caller forms sum m (1 - ssim_map) as 3 * count - partial) and writes ZEROS into
 * m1..m3 at ignored pixels; bwd writes every element of v_img (exactly 0 farther than 5 pixels from any counted
 * pixel).  With an all-counted mask both compute what the unmasked entries compute. */
int clmgs_l1_ssim_loss_masked_fwd(void* stream, int H, int W, const float* img, int64_t stride_c,
                                  int64_t stride_y, int64_t stride_x, const uint8_t* gt_u8,
                                  float* partials, float* m1, float* m2, float* m3,
                                  const uint8_t* mask);
int clmgs_l1_ssim_loss_masked_bwd(void* stream, int H, int W, const float* img, int64_t stride_c,
                                  int64_t stride_y, int64_t stride_x, const uint8_t* gt_u8,
                                  const float* v_loss, float lambda_dssim, const float* m1,
                                  const float* m2, const float* m3, float* v_img,
                                  const uint8_t* mask);

/* ---- per-camera exposure compensation (csrc/exposure.hip; the convention of the INRIA 3DGS exposure.json)
 * E_dev: DEVICE pointer to float32 [3][4], row-major.  x, y, g, v_x are [3,H,W] VIEWS given by their element strides
 * (c, y, x), like img of the loss entries: the rasterizer's [H,W,3] buffer and a planar image alike.
 *   fwd:  y[c] = x[0] E[0][c] + x[1] E[1][c] + x[2] E[2][c] + E[c][3]            (y must not alias x)
 *   bwd:  v_x[k] = E[k][0] g[0] + E[k][1] g[1] + E[k][2] g[2], g = dL/dy; v_x MAY BE g itself (same pointer and
 *         strides: in place).  Each workgroup STORES one row of 12 floats, laid out like E, into
 *         partials[clmgs_exposure_partials_rows(H, W)][12] (every row is written; nothing to zero):
 *         their column sums are dL/dE[k][c] = sum_p x[k] g[c] (c < 3) and dL/dE[c][3] = sum_p g[c].
 *   grad_finish: one wave sums the `rows` rows of partials in a fixed order and ADDS the 12 sums into grad12.
 * No float atomics: the same inputs give the same bits on every run. */
int clmgs_exposure_partials_rows(int H, int W);
int clmgs_exposure_fwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                       int64_t stride_x, const float* E_dev, float* y, int64_t ystride_c, int64_t ystride_y,
                       int64_t ystride_x);
int clmgs_exposure_bwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                       int64_t stride_x, const float* E_dev, const float* g, int64_t gstride_c,
                       int64_t gstride_y, int64_t gstride_x, float* v_x, int64_t vstride_c, int64_t vstride_y,
                       int64_t vstride_x, float* partials);
int clmgs_exposure_grad_finish(void* stream, int rows, const float* partials, float* grad12);

/* ---- learnable sky (csrc/sky.hip): one equirectangular map sky[Hs,Ws,3] (DEVICE pointer, world axes) composited
 * behind the splats.  x, y, g are [3,H,W] VIEWS by element strides (c, y, x) like the exposure entries' (with an
 * [H,W,4] buffer the fourth word of a pixel is neither read nor written); alphas, v_alphas are contiguous [H,W];
 * viewmat_host[16] (row-major world->camera) and K_host[9] are HOST pointers, as clmgs_preprocess_fwd takes them.  With
 * R = viewmat[:3,:3], dc = ((px + .5 - cx) / fx, (py + .5 - cy) / fy, 1), d = R^T dc / |dc|,
 * u = (atan2(d.x, d.z) / 2pi + .5) Ws - .5 (columns wrap), v = (asin(d.y) / pi + .5) Hs - .5 (rows clamp),
 * s = the bilinear sample of the map at (u, v), weights w_k:
 *   fwd:  y[c] = x[c] + (1 - alphas) s[c]; y MAY BE x itself (same pointer and strides: in place).
 *   bwd:  v_alphas = -(g[0] s[0] + g[1] s[1] + g[2] s[2]) is STORED, and round(2^48 (1 - alphas) w_k g[c]) is ADDED
 *         into acc[Hs,Ws,3], signed 64-bit fixed point with unit 2^-48, by integer atomics only: acc holds the same
 *         bits whatever the order of pixels, workgroups, calls and cameras.  The caller zeroes acc once and may call
 *         camera after camera.  CONTRACT: every texel's sum stays below 2^15 in magnitude.
 *   acc_add:      dst[i] += src[i], i < n (int64).
 *   grad_convert: grad[i] += float(acc[i] * 2^-48) (through double), then acc[i] = 0.
 * A null pointer, H < 1, W < 1, Hs < 1, Ws < 1 or a zero focal length returns CLMGS_EINVAL before anything is written. */
int clmgs_sky_fwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                  const float* alphas, const float* viewmat_host, const float* K_host, const float* sky, int Hs,
                  int Ws, float* y, int64_t ystride_c, int64_t ystride_y, int64_t ystride_x);
int clmgs_sky_bwd(void* stream, int H, int W, const float* g, int64_t gstride_c, int64_t gstride_y, int64_t gstride_x,
                  const float* alphas, const float* viewmat_host, const float* K_host, const float* sky, int Hs,
                  int Ws, float* v_alphas, int64_t* acc);
int clmgs_sky_acc_add(void* stream, int64_t n, const int64_t* src, int64_t* dst);
int clmgs_sky_grad_convert(void* stream, int64_t n, int64_t* acc, float* grad);

/* ---- depth regularisation (csrc/invdepth.hip; the INRIA 3DGS convention: rendered inverse depth
 * I = sum_i w_i / z_i, the fourth blended channel with 1/z as fourth colour and background 0, against a uint16 prior
 * prior = raw / 65536 * scale + offset)
 *   pack:     word 9 (the fourth colour) of record i of packed[V,16] = radii[i] > 0 ? 1 / depths[i] : 0; no other word
 *             of the records clmgs_preprocess_fwd / _aa_fwd left is touched.
 *   l1_fwd_bwd: one pass over the H*W pixels.  I and v_I are [H,W] VIEWS given by their element strides (y, x): channel
 *             3 of an [H,W,4] buffer (strides 4W, 4) and a planar map alike.  prior_u16 [H,W] contiguous; mask uint8
 *             [H,W] contiguous or NULL (0 = ignored).  v_I = weight * m * sign(I - prior) / (H*W) (0 at I == prior) is
 *             STORED at every pixel -- that word only; each workgroup STORES one partial sum of m |I - prior| into
 *             partials[clmgs_invdepth_partials_rows(H, W)] (every row is written; nothing to zero).
 *   finish:   one wave sums the `rows` partial sums in a fixed order and STORES the total into sum_out[0]; the loss term
 *             is weight * sum_out[0] / (H*W).
 *   rows_bwd: for i < V with radii[i] > 0: g_d = the sum in ascending slot order of word 9 of the partial lines
 *             [row_cum[i-1], row_cum[i]) (partials != NULL) or word 9 of packed_grad[i] (packed_grad != NULL; exactly
 *             one of the two), and  g_xyz[g] += -g_d / depths[i]^2 * viewmat[2][0..2]  at row g = filter ? filter[i] : i
 *             of the [N,3] table (packed_grads = 0) or words 0..2 of the [N,12] table (packed_grads = 1); viewmat is a
 *             HOST pointer to the row-major world-to-camera matrix.  Other rows and words are not touched.  A plain
 *             read-modify-write: run it on the stream of, and after, the camera's clmgs_preprocess*_bwd.
 * No float atomics: the same inputs give the same bits on every run.  Bad arguments return CLMGS_EINVAL before
 * anything is written. */
int clmgs_invdepth_partials_rows(int H, int W);
int clmgs_invdepth_pack(void* stream, int V, const int32_t* radii, const float* depths, void* packed);
int clmgs_invdepth_l1_fwd_bwd(void* stream, int H, int W, const float* I, int64_t stride_y, int64_t stride_x,
                              const uint16_t* prior_u16, float scale, float offset, const uint8_t* mask,
                              float weight, float* v_I, int64_t vstride_y, int64_t vstride_x, float* partials);
int clmgs_invdepth_finish(void* stream, int rows, const float* partials, float* sum_out);
int clmgs_invdepth_rows_bwd(void* stream, int V, const int64_t* filter, const int32_t* radii, const float* depths,
                            const float* viewmat, const void* partials, const int64_t* row_cum,
                            const void* packed_grad, float* g_xyz, int packed_grads);

/* ---- MCMC densification (csrc/mcmc.hip; gsplat's MCMCStrategy, Kheradmand et al. 2024: a fixed Gaussian budget)
 *   relocation: for i < n, r = clamp(ratios[i], 1, 51), o = opacities[i] (ACTIVATED, in (0, 1)):
 *               new_opacities[i] = o' = 1 - (1 - o)^(1/r),
 *               D = sum_{i=1..r} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1),
 *               new_scales[i][0..2] = (o / D) * scales[i][0..2]   (ACTIVATED scales, [n,3]).
 *               Double arithmetic, each output rounded once to float.  Outputs must not alias inputs.
 *   reg_grad:   the gradients of w_o * mean(sigmoid(opacity_raw)) + w_s * mean(exp(scaling_raw)), ADDED: for i < n
 *               g_opacity[i * g_opacity_stride] += c_o * s (1 - s), s = sigmoid(opacity_raw[i * opacity_stride]);
 *               g_scaling[i * g_scaling_stride + j] += c_s * exp(scaling_raw[i * scaling_stride + j]), j = 0..2.
 *               Strides are in floats; the pointers address the first row's column: four separate tensors (strides 1
 *               and 3) and the packed [N,12] tables (stride 12, pointers at columns 3 and 4) alike.  The caller folds
 *               1/N, 1/3 and any batch scale into c_o / c_s.  Nothing but those four gradient columns is written.
 *   noise:      in place on xyz[n,3]: gate = 1 / (1 + exp(-100 ((1 - sigmoid(opacity_raw[i])) - 0.995))),
 *               Sigma = R diag(exp(scaling_raw[i]))^2 R^T with R of the NORMALISED rotation_raw[i] (w,x,y,z),
 *               xyz[i] += Sigma (noise[i] * gate * scaler).  A zero increment leaves the stored bits.  packed_mirror
 *               (optional, [n,12], 8 B aligned): columns 0..2 of row i receive the new xyz[i] in the same pass, columns
 *               3..11 are not written.
 * No atomics; the same inputs give the same bits on every run.  Bad arguments return CLMGS_EINVAL before anything is
 * written. */
int clmgs_mcmc_relocation(void* stream, int64_t n, const float* opacities, const float* scales, const int32_t* ratios,
                          float* new_opacities, float* new_scales);
int clmgs_mcmc_reg_grad(void* stream, int64_t n, const float* opacity_raw, int64_t opacity_stride,
                        const float* scaling_raw, int64_t scaling_stride, float* g_opacity, int64_t g_opacity_stride,
                        float* g_scaling, int64_t g_scaling_stride, float c_o, float c_s);
int clmgs_mcmc_noise(void* stream, int64_t n, float* xyz, const float* opacity_raw, const float* scaling_raw,
                     const float* rotation_raw, const float* noise, float scaler, float* packed_mirror);

/* ---- bilateral-grid colour correction (csrc/bilagrid.hip; gsplat's use_bilateral_grid operator)
 * grid_dev: DEVICE pointer to float32 [L][Hg][Wg][12], coefficient 4c + k = A[c][k]; 2 <= Wg, Hg <= 64, 2 <= L <= 32
 * (anything else: CLMGS_EINVAL).  x, y, g, v_x are [3,H,W] VIEWS given by their element strides (c, y, x), as for the
 * exposure entries.  With u = (px + .5) / W, v = (py + .5) / H, s = .299 x[0] + .587 x[1] + .114 x[2], A the trilinear
 * interpolation (align_corners, border) of the grid at (u, v, clamp(s, 0, 1)), every lerp fmaf(t, b - a, a):
 *   fwd:  y[c] = A[c][0] x[0] + A[c][1] x[1] + A[c][2] x[2] + A[c][3]             (y must not alias x)
 *   bwd:  v_x[k] = sum_c A[c][k] g[c] + lum[k] (L - 1) [0 < s < 1] sum_{c,k'} (A_hi - A_lo)[c][k'] g[c] x[k'] (x[3] = 1);
 *         v_x MAY BE g itself (same pointer and strides: in place).  Each workgroup STORES one row of L x 48 floats into
 *         partials[clmgs_bilagrid_partials_rows(H, W, Hg, Wg)][L * 48] (every row is written; nothing to zero).
 *   grad_finish: per grid element, the rows of its at most four cells summed in a fixed order and ADDED into
 *         grad[L][Hg][Wg][12]: dL/dG[node][4c + k] = sum_p w_node(p) g[c] x[k].  H, W as given to bwd.
 *   tv_grad: grad[n][L][Hg][Wg][12] += d(weight * tv)/dtable, tv = (1/n) sum_axis sum (G[i+1] - G[i])^2 / count_axis,
 *         count_axis = 12 x the differences along the axis in one grid.  16-byte aligned tables.
 * No float atomics: the same inputs give the same bits on every run. */
int clmgs_bilagrid_partials_rows(int H, int W, int Hg, int Wg);
int clmgs_bilagrid_fwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                       int64_t stride_x, const float* grid_dev, int L, int Hg, int Wg, float* y, int64_t ystride_c,
                       int64_t ystride_y, int64_t ystride_x);
int clmgs_bilagrid_bwd(void* stream, int H, int W, const float* x, int64_t stride_c, int64_t stride_y,
                       int64_t stride_x, const float* grid_dev, int L, int Hg, int Wg, const float* g,
                       int64_t gstride_c, int64_t gstride_y, int64_t gstride_x, float* v_x, int64_t vstride_c,
                       int64_t vstride_y, int64_t vstride_x, float* partials);
int clmgs_bilagrid_grad_finish(void* stream, int H, int W, int L, int Hg, int Wg, const float* partials, float* grad);
int clmgs_bilagrid_tv_grad(void* stream, const float* table, int64_t n, int L, int Hg, int Wg, float weight,
                           float* grad);

/* ---- camera pose refinement (csrc/pose.hip, csrc/pose_math.h; gsplat's pose_opt: the gradient of the loss with
 * respect to the camera).  For the world-to-camera matrix [Rv | t] and the camera centre c the front end was run
 * with, over the rows i with radii[i] > 0:
 *     v_R[9] = sum_i (vp_i m_i^T + 2 vS_i Rv Sigma_i)   v_t[3] = sum_i vp_i   v_campos[3] = -sum_i vd_i
 * vp_i / vS_i: the camera-space mean / covariance cotangents of the projection VJP; vd_i: the direction cotangent of
 * the SH VJP with the clamp mask applied (0 at degree 0).  c is NOT assumed to be -Rv^T t: the three stay apart and the
 * host composes them.
 *   pose_grad: replaces fully_fused_projection(viewmats_requires_grad=True)'s v_viewmats[:3, :4] (v_R | v_t) and the
 *             autograd of dirs = means - camtoworlds[:3, 3] (v_campos) of gsplat's rasterization() for ONE camera of the
 *             fused front end.  The inputs, and the argument checks, are those of clmgs_preprocess_bwd: rows, SH rows
 *             (not read at degree 0, may be NULL there), HOST camera constants, radii, and the cotangent lines either as
 *             packed_grad[V,16] or as partials + row_cum (exactly one; a row's lines are summed in ascending slot order,
 *             as clmgs_preprocess_bwd sums them).  antialiased != 0: for records of clmgs_preprocess_aa_fwd
 *             (v_compensation = go * op).  Each workgroup STORES one row of 16 floats  v_R | v_t | v_campos | 0  into
 *             partials_out[clmgs_pose_grad_partials_rows(V)][16] (every row is written; nothing to zero).
 *   pose_grad_finish: one wave sums the `rows` rows in ascending order and ADDS the 15 sums into grad15, once.
 *   projection_viewmat_bwd: replaces the v_viewmats output of gsplat's fully_fused_projection backward
 *             (viewmats_requires_grad=True), operator form: the arguments of clmgs_projection_aa_bwd (v_compensations
 *             NULL: the plain projection; v_depths optional, added to vp_i[2]), partials
 *             [C * clmgs_projection_viewmat_partials_rows(N)][16] scratch (one row per workgroup), and v_viewmats
 *             [C,16], STORED: rows 0..2 of the 4x4 = v_R | v_t, row 3 = 0.
 * No float atomics: the same inputs give the same bits on every run.  Bad arguments return CLMGS_EINVAL before
 * anything is written. */
int clmgs_pose_grad_partials_rows(int V);
int clmgs_pose_grad(void* stream, int V, const int64_t* filter, const float* xyz, const float* opacity_raw,
                    const float* scaling_raw, const float* rotation_raw, const float* sh_rows, int sh_by_filter,
                    const float* viewmat_host, const float* K_host, const float* campos_host, int width, int height,
                    int degree, float eps2d, const int32_t* radii, const void* packed_grad, const void* partials,
                    const int64_t* row_cum, const int32_t* sh_index, int antialiased, float* partials_out);
int clmgs_pose_grad_finish(void* stream, int rows, const float* partials, float* grad15);
int clmgs_projection_viewmat_partials_rows(int N);
int clmgs_projection_viewmat_bwd(void* stream, int C, int N, const float* means, const float* quats,
                                 const float* scales, const float* viewmats, const float* Ks, int width, int height,
                                 float eps2d, const int32_t* radii, const float* v_means2d, const float* v_depths,
                                 const float* v_conics, const float* v_compensations, float* partials,
                                 float* v_viewmats);

/* ---- clm_kernels row movers  (clm_offload/engine.py:499-505, 622-636, 789-802, 815-822)
 * dst/src may be device memory or pinned (mapped) host memory.
 * gather:      dst[dst_idx ? dst_idx[i] : i] = src[src_idx ? src_idx[i] : i]
 * scatter_add: dst[dst_idx ? dst_idx[i] : i] += src[src_idx ? src_idx[i] : i]
 * Index arrays are i32 or i64 (idx_is_64). cols floats per row; grid_blocks = 0 -> auto. */
int clmgs_rows_gather(void* stream, float* dst, const float* src, const void* dst_idx,
                      const void* src_idx, int idx_is_64, int64_t n_rows, int cols,
                      int grid_blocks);
int clmgs_rows_scatter_add(void* stream, float* dst, const float* src, const void* dst_idx,
                           const void* src_idx, int idx_is_64, int64_t n_rows, int cols,
                           int grid_blocks);

/* ---- clm_kernels bitmap helpers  (clm_offload/engine.py:152-153, 200-204, 227-232)
 * bitmap elements are elem_bytes in {1,2,4,8}. */
int clmgs_scatter_to_bit(void* stream, void* bitmap, int elem_bytes, const int64_t* filter,
                         int64_t n, int bit);
int clmgs_extract_ffs(void* stream, const void* bitmap, int elem_bytes, int64_t N, uint8_t* ffs);
/* cnt[bsz-1] i32 (caller zeroes): cnt[i] = #{g : bit(bsz-1-i) & bit(bsz-2-i)} i.e. the
 * number of Gaussians visible in both micro-batch i and i+1. */
int clmgs_pair_overlap_count(void* stream, const void* bitmap, int elem_bytes, int64_t N,
                             int bsz, int32_t* cnt);
/* clm_kernels.set_signal (clm_offload/engine.py:807,825): stream-ordered write of `value`
 * to pinned host flag signal[idx], visible to a polling host thread. */
int clmgs_set_signal(void* stream, int32_t* signal_pinned, int idx, int32_t value);

/* ---- Adam  (optimizer.py:6-184; clm_offload/gaussian_model.py:161-211)
 * Row-wise Adam over p,g,m,v [*, cols] with per-column learning rate col_lr[cols] (device).
 * rows: i32/i64 row list or NULL (all n_rows rows in order); mask: u8[n_rows] or NULL
 * (rows with mask==0 are skipped; this is clm_kernels.selective_adam_update).
 * g == NULL means an all-zero gradient (pure moment decay; nothing read or cleared).
 * g is multiplied by grad_scale; bias_correction uses the 1-based `step`; betas/eps are
 * doubles so 1-beta and beta^step are formed in double on the host;
 * zero_grad != 0 clears consumed gradient rows. */
int clmgs_adam_rows(void* stream, float* p, float* g, float* m, float* v, const void* rows,
                    int idx_is_64, const uint8_t* mask, int64_t n_rows, int cols,
                    const float* col_lr, double beta1, double beta2, double eps, int step,
                    int bias_correction, float grad_scale, int zero_grad);
/* Deferred dense Adam: replay, for the listed rows (NULL = rows 0..n_rows-1), the zero-gradient
 * updates of steps last_step[row]+1 .. to_step (moment decay + parameter step, same per-element
 * operations as clmgs_adam_rows with g == NULL, bias corrections from a running product).  The
 * caller then sets last_step[rows] = to_step.  Only the first max_replay missed steps are replayed
 * exactly; for the rest the moments are decayed analytically (the first moment has decayed by
 * beta1^max_replay by then, the parameter increments are below float resolution).  Elements whose
 * moments are both zero are left untouched (every replayed step is the identity for them).
 * g / g_step (both or neither): DEFERRED gradient step.  g_step[row] (i32) is the optimizer step whose
 * gradient waits in g[row, cols]; if it lies in (last_step, to_step] it is applied here at its own step
 * with grad_scale, between the replays before and after it, and the gradient row is zeroed: the same
 * operations in the same order as the eager update at the end of that batch (optimizer.py:130-144 /
 * clm_offload/engine.py:316-328), in one pass over the row instead of two.  keep_grad = 1: the consumed
 * row is not cleared (producers that STORE on first touch: clmgs_preprocess_bwd with sh_stamp).
 * With an explicit row list every table is addressed as base + row * cols and ONLY the listed rows are touched: m / v
 * may therefore be bases moved back by row0 rows in front of a shard that holds rows row0.. only (camera-DP: the moments
 * of a row live at its owner, clm_gs_amd/strategies/clm_offload/gaussian_model.py moments_sharded). */
/* The packed [N,12] mirror of the four GPU-resident parameter tensors, and their dense Adam when the
 * engine accumulates gradients in a packed [N,12] table: params / exp_avg / exp_avg_sq are HOST
 * arrays of 4 device pointers (xyz [N,3], opacity [N,1], scaling [N,3], rotation [N,4]), lr4 a
 * host array of their 4 learning rates.  One pass: grad * grad_scale -> Adam (torch.optim.Adam's
 * bias-corrected formula) -> p / m / v written back, mirror row refreshed, gradient row zeroed.
 * g_stamp (i32 [n], optional) + cur_step: the first-touch form -- only rows with g_stamp[row] == cur_step
 * carry a gradient of this step (clmgs_preprocess_bwd stamped them); the others are not read, and nothing
 * is zeroed. */
int clmgs_pack_small(void* stream, int64_t n, const float* xyz, const float* opacity,
                     const float* scaling, const float* rotation, void* packed_p);
int clmgs_adam_small_packed(void* stream, int64_t n, float* const* params, float* const* exp_avg,
                            float* const* exp_avg_sq, const double* lr4, void* packed_p,
                            void* packed_g, double beta1, double beta2, double eps, int step,
                            int bias_correction, float grad_scale, const int32_t* g_stamp, int cur_step);
int clmgs_adam_catch_up(void* stream, float* p, float* m, float* v, const int32_t* last_step,
                        const void* rows, int idx_is_64, int64_t n_rows, int cols,
                        const float* col_lr, double beta1, double beta2, double eps, int to_step,
                        int bias_correction, int max_replay, float* g, const int32_t* g_step,
                        float grad_scale, int keep_grad);
/* Host (OpenMP) variant on pinned/pageable host memory: cpu_adam.FusedCPUAdam row group
 * update (clm_offload/engine.py:316-328).  If signal != NULL, busy-waits until
 * *signal != 0 before touching the rows. */
int clmgs_host_adam_rows(float* p, float* g, float* m, float* v, const int32_t* rows,
                         int64_t n_rows, int cols, const float* col_lr, double beta1,
                         double beta2, double eps, int step, int bias_correction, float grad_scale,
                         int zero_grad, const volatile int32_t* signal, int n_threads);

/* Host-resident mode, this build's form of the cpu_adam worker (clm_offload/engine.py:301-335,
 * optimizer.py:130-144): a persistent pool of host threads and a DEFERRED row optimizer.  Per row two
 * int32 stamps: last_step (step p/m/v are current as of) and g_step (step whose gradient waits in g,
 * 0 = none).  clmgs_host_rows_prepare brings the listed rows (rows == NULL: rows 0..n_rows-1) to
 * `to_step` -- zero-gradient steps are replayed in registers, the waiting gradient is applied at its
 * own step with grad_scale -- sets last_step = to_step, g_step = next_g_step, and copies each
 * up-to-date parameter row into stage[k] (contiguous pinned staging for a hipMemcpyAsync; NULL to skip).
 * sparse != 0 (sparse_adam): rows are stepped only when they carry a gradient, nothing is replayed.
 * Arithmetic per element and step = clmgs_host_adam_rows'. */
int clmgs_host_pool_start(int n_threads);  /* <= 0: sized to the CPUs the process may use (cgroup quota aware) */
int clmgs_host_usable_cpus(void);
/* hipMemcpyAsync of `bytes` between pinned host memory and HBM on `stream` (SDMA engine; kind 1 = host
 * -> device, 2 = device -> host): how the host-resident mode moves its contiguous staging chunks
 * (replaces clm_kernels.send_shs2gpu_stream's zero-copy gather, clm_offload/engine.py:499-505). */
int clmgs_memcpy_async(void* stream, void* dst, const void* src, size_t bytes, int kind);
int clmgs_host_rows_prepare(float* p, const float* g, float* m, float* v, int32_t* last_step,
                            int32_t* g_step, const int32_t* rows, int64_t n_rows, int cols,
                            const float* col_lr, double beta1, double beta2, double eps, int to_step,
                            int next_g_step, int bias_correction, float grad_scale, int max_replay,
                            float* stage, int sparse);

/* ---- densification statistics  (clm_offload/gaussian_model.py:833-851;
 *      no_offload/gaussian_model.py:767-783; densification.py:59-147)
 * For i < n (only rows with radii[i] > 0 when only_visible != 0): g = filter ? filter[i] : i;
 * max_radii2D[g] = max(., radii[i]); accum[g] += |v_means2d[i] * (W/2, H/2)|; denom[g] += 1. */
int clmgs_densify_stats(void* stream, int64_t n, const int64_t* filter, const float* v_means2d,
                        const int32_t* radii, int only_visible, float half_w, float half_h,
                        float* max_radii2D,
                        float* xyz_gradient_accum, float* denom);

/* ---- storage order of the rows (no reference counterpart; clm_gs_amd/utils.py morton_order, trainer / densification):
 * order[i] = the row that comes i-th along the Z-order curve of (x, y), 16 bits per axis, ties in row order (stable):
 * code = spread(qx) | spread(qy) << 1 with q = rint((double(p) - lo) / max(hi - lo, 1e-30) * 65535); lo_hi (device) =
 * lo_x lo_y hi_x hi_y as doubles.  xyz [n,3] f32, order [n] i64, temp: clmgs_morton_order_temp_bytes(n); n < 2^31. */
size_t clmgs_morton_order_temp_bytes(int64_t n);
int clmgs_morton_order(void* stream, int64_t n, const float* xyz, const double* lo_hi, int64_t* order, void* temp,
                       size_t temp_bytes);

/* ---- fast_tsp.find_tour  (clm_offload/engine.py:179): open-tour heuristic on an n x n
 * integer distance matrix (greedy nearest neighbour + 2-opt until no improvement). */
int clmgs_tsp_tour(int n, const int64_t* dist, int32_t* tour);

/* ---- simple_knn._C.distCUDA2  (strategies/clm_offload/gaussian_model.py:60-63; init-time only)
 * pts_sorted[n,3]: points sorted by grid cell id ((z*gy + y)*gx + x, cell = floor((p - origin)/h)
 * clamped); cell_start[gx*gy*gz + 1] i32: first sorted index of every cell.  Writes the mean
 * squared distance to the 3 nearest neighbours, in sorted order.  Exact while the answer lies
 * within max_ring cells. */
int clmgs_knn3_mean_dist2(void* stream, int n, const float* pts_sorted, const int32_t* cell_start,
                          float ox, float oy, float oz, float h, int gx, int gy, int gz,
                          int max_ring, float* mean_d2_sorted);

/* Host-resident batch (sh_residency="host"): the rows a batch touches, grouped by the camera that uses them FIRST (slot
 * order of the rows that still have to be staged) and LAST (hand-back order of the gradient rows) -- what the reference
 * derives from its bitmap with ffs / sort / tolist (clm_offload/engine.py:137-260), as two stable one-digit radix sorts.
 * touched[n] ascending row ids; bitmap[N] of elem_bytes-wide words, bit bsz-1-i = camera i; staged (u8[N], optional):
 * rows already staged for this batch (not "late").  Out: late_sorted[<= n] (late rows by first camera), rows_by_last[n],
 * slot_of[row] = slot0 + position in late_sorted, counts[2*bsz+1] (device) = late rows per first camera | rows per
 * last camera | number of late rows. */
size_t clmgs_host_groups_temp_bytes(int64_t n);
int clmgs_host_groups(void* stream, int64_t n, const int64_t* touched, const void* bitmap, int elem_bytes, int bsz,
                      const uint8_t* staged, int slot0, int32_t* late_sorted, int32_t* rows_by_last, int32_t* slot_of,
                      int64_t* counts, void* temp, size_t temp_bytes);

/* Camera-DP, locality exchange, step F (clm_gs_amd/dp.py publish_rows; net-new, the reference is single GPU): packs
 * the message an owner all-gathers -- msg[0 .. chunk*cols) = the rows table[own_rows[i]] (zeros where stamp != NULL and
 * stamp[row] != step: the row's gradient line is not of this step), msg[chunk*cols + i] = the bits of
 * int32(own_rows[i] - lo).  cols % 4 == 0, msg / table 16 B aligned, chunk >= n_rows. */
int clmgs_publish_pack(void* stream, float* msg, const float* table, const int64_t* own_rows, const int32_t* stamp,
                       int step, int64_t lo, int64_t n_rows, int64_t chunk, int cols);

/* Camera-DP, the small attributes (xyz / opacity / scaling / rotation) computed by the OWNER of a row range (net-new:
 * the reference is single GPU; its SelectiveAdam, optimizer.py:6-88, is the sparse form on one device).  Between two
 * refreshes a rank's copies of the rows it does not own are stale by a bounded amount; three entries:
 *  - clmgs_visibility_candidates: mask[N] (u8) = 1 for every row OUTSIDE [own_lo, own_hi) that may pass the cull of
 *    clmgs_visibility_select_count in any of the C cameras if its stored mean is off by up to pos_margin (Euclidean) and
 *    its largest scale by a factor up to scale_gain -- a superset of the rows the exact cull keeps for the true values;
 *    the caller fetches the candidates' current lines from their owners before the exact pass.
 *  - clmgs_small_rows_scatter: packed [n_rows,12] lines (xyz 3 | opacity 1 | scaling 3 | rotation 4 | pad) written to
 *    the four parameter tensors and the packed mirror at the unique row ids `rows`.
 *  - clmgs_adam_small_packed_range: clmgs_adam_small_packed on the rows row_begin <= r < row_end only (row_end < 0:
 *    all rows); every other row of every table is left bit for bit as it was. */
int clmgs_visibility_candidates(void* stream, int C, int N, int own_lo, int own_hi, const float* means,
                                const float* log_scales, const float* viewmats, const float* Ks, int width,
                                int height, float eps2d, float near_plane, float far_plane, float pos_margin,
                                float scale_gain, uint8_t* mask);
int clmgs_small_rows_scatter(void* stream, int64_t n_rows, const int64_t* rows, const void* lines, float* xyz,
                             float* opacity, float* scaling, float* rotation, void* packed_p);
int clmgs_adam_small_packed_range(void* stream, int64_t n, int64_t row_begin, int64_t row_end, float* const* params,
                                  float* const* exp_avg, float* const* exp_avg_sq, const double* lr4, void* packed_p,
                                  void* packed_g, double beta1, double beta2, double eps, int step,
                                  int bias_correction, float grad_scale, const int32_t* g_stamp, int cur_step);

/* Single GPU, round 5: the dense Adam of the small attributes DEFERRED per block of 256 consecutive (Z-ordered) rows
 * (replaces the eager clmgs_adam_small_packed of a batch; the reference steps them eagerly with torch's Adam,
 * strategies/clm_offload/engine.py:870-882 / optimizer.py:91-184 -- same arithmetic per step, applied later).
 * blk_last[ceil(n/256)] holds the optimizer step each block is current as of.  A call brings up to `to_step` every
 * block that (a) may hold a row visible in one of the C cameras when its values are stale by the waiting steps'
 * worth of Adam's step bound (pos_margin[k], scale_gain[k] for k waiting steps), (b) is clmgs_small_deferred_kmax()
 * steps behind, or (c) any block at all when flush_all != 0 -- replaying the waiting steps one by one with the
 * constants of THEIR step (lr4_hist[j][4], step_index[j]: entry j describes step to_step - j; n_hist entries) and the
 * row's waiting gradient line (packed_g row, stamp g_stamp[row]) at the step it belongs to.  Bit-identical to the
 * eager sequence; the packed mirror is refreshed for the blocks processed. */
int clmgs_small_deferred_kmax(void);
int clmgs_adam_small_deferred(void* stream, int64_t n, float* const* params, float* const* exp_avg,
                              float* const* exp_avg_sq, void* packed_p, const void* packed_g, const int32_t* g_stamp,
                              int32_t* blk_last, int to_step, int n_hist, const double* lr4_hist,
                              const int32_t* step_index, const float* pos_margin, const float* scale_gain, double beta1,
                              double beta2, double eps, float grad_scale, int C, const float* viewmats, const float* Ks,
                              int width, int height, float eps2d, float near_plane, float far_plane, int flush_all,
                              uint8_t* blk_flag /* optional [ceil(n/256)] out: 0 = no row of the block can be visible in
                              any of the C cameras; input of clmgs_visibility_select_count_blocks */);
/* The same with a per-block camera word and / or a block selector.  blk_cams[ceil(n/256)] (optional out, needs blk_flag):
 * bit c = the candidate test admits camera c for some row of the block (blk_flag[blk] != 0 <=> blk_cams[blk] != 0).
 * blk_sel_bits[ceil(n/256)] (optional, not with flush_all): the call takes only the blocks with
 * ((blk_sel_bits[blk] & sel_mask) != 0) == sel_want (0 or 1); a block it does not take is neither read nor written, and
 * neither are its blk_flag / blk_last / blk_cams entries.  Two calls with sel_want 0 and 1 do what one call without a
 * selector does, bit for bit, so a caller that knows which blocks' inputs are final early can bring those up to date on
 * another stream.  Both NULL: clmgs_adam_small_deferred. */
int clmgs_adam_small_deferred_sel(void* stream, int64_t n, float* const* params, float* const* exp_avg,
                                  float* const* exp_avg_sq, void* packed_p, const void* packed_g, const int32_t* g_stamp,
                                  int32_t* blk_last, int to_step, int n_hist, const double* lr4_hist,
                                  const int32_t* step_index, const float* pos_margin, const float* scale_gain,
                                  double beta1, double beta2, double eps, float grad_scale, int C, const float* viewmats,
                                  const float* Ks, int width, int height, float eps2d, float near_plane, float far_plane,
                                  int flush_all, uint8_t* blk_flag, uint64_t* blk_cams, const uint64_t* blk_sel_bits,
                                  uint64_t sel_mask, int sel_want);

/* Device error word: kernels that meet a broken invariant of their caller raise a bit in one device word instead of
 * failing silently.  *bits: 4 = clmgs_adam_small_deferred met a block further behind than the step history it was given
 * (those rows' parameters are wrong).  1 and 2 are retired (they belonged to binning kernels that no longer exist) and
 * are never raised; any nonzero value is an error.  Synchronises the device; `reset` clears the word.  No reference
 * counterpart; callers check it where they synchronise anyway (evaluation, saving, the end of a benchmark). */
int clmgs_device_errors(uint32_t* bits, int reset);

/* ---- resolution schedule (csrc/resample.hip): exact integer area resampling to level L >= 1, f = 2^L,
 * Ho = ceil(H / f), Wo = ceil(W / f); the image extent is kept (pixel pitch W/Wo x H/Ho).  With
 *   wx(j,x) = max(0, min((x+1) Wo, (j+1) W) - max(x Wo, j W)),  wy(i,y) likewise from H, Ho,
 *   S(i,j) = sum_y sum_x wy(i,y) wx(j,x) p[y,x]:
 *   u8 / u16: out = (2 S + W H) / (2 W H) (round half up); u8 takes `planes` contiguous planes [planes,H,W], u16 one.
 *   mask:     p = [m != 0]; out = 255 where 2 S >= W H (at least half of the cell's area is counted), else 0; *count
 *             (device int64, 8-byte aligned) is zeroed on the stream and receives the number of 255s.
 * src and dst are contiguous and do not overlap; H, W <= 32768; 1 <= level <= 8 (level 0 is the input: no kernel).
 * Integer arithmetic only, the same bits on every run.  Bad arguments return CLMGS_EINVAL before anything is written. */
int clmgs_area_resample_u8(void* stream, int planes, int H, int W, int level, const uint8_t* src, uint8_t* dst);
int clmgs_area_resample_u16(void* stream, int H, int W, int level, const uint16_t* src, uint16_t* dst);
int clmgs_area_resample_mask(void* stream, int H, int W, int level, const uint8_t* src, uint8_t* dst, int64_t* count);

/* ---- lens distortion (csrc/undistort.hip, csrc/lens_math.h): inverse-map bilinear remap of a distorted source image
 * [planes,Hs,Ws] onto the ideal centred pinhole [planes,Ho,Wo] with focal lengths fxo, fyo and principal point
 * (Wo/2, Ho/2).  lens: HOST array of ten doubles fx, fy, cx, cy, k1, k2, k3, k4, p1, p2 -- intrinsics in pixels of the
 * source image, COLMAP's convention (the centre of the top-left pixel is at (0.5, 0.5)); `fisheye`: 0 or 1.  For output
 * pixel (i, j), all in float64, every product and sum rounded on its own in the order written:
 *   x = (j + 0.5 - Wo/2) / fxo,   y = (i + 0.5 - Ho/2) / fyo,   r2 = x*x + y*y
 *   perspective:  rad  = 1 + r2*(k1 + r2*k2)
 *                 mono = 1 + r2*(3*k1 + r2*5*k2)
 *                 xd = x*rad + 2*p1*x*y + p2*(r2 + 2*x*x)
 *                 yd = y*rad + p1*(r2 + 2*y*y) + 2*p2*x*y
 *   fisheye:      r = sqrt(r2),  th = atan(r),  t2 = th*th
 *                 rad  = 1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4)))
 *                 mono = 1 + t2*(3*k1 + t2*(5*k2 + t2*(7*k3 + t2*9*k4)))
 *                 s = th*rad/r  (s = 1 where r < 1e-12),  xd = x*s,  yd = y*s
 *   u = fx*xd + cx - 0.5,   v = fy*yd + cy - 0.5        (the source sample position, in pixel indices)
 * valid, with tau = 2^-20:  mono > 0  (the derivative of the distorted radius: where it is not positive a strongly
 *   negative k1 has folded the radial profile back and (u, v) is a second image of a ray that is not there),
 *   -tau <= u <= Ws-1+tau  and  -tau <= v <= Hs-1+tau;  with src_mask (uint8 [Hs,Ws]) also all four taps non-zero there.
 * sampling: u, v clamped into [0, Ws-1] x [0, Hs-1];  x0 = min(floor(u), max(Ws-2, 0)),  x1 = min(x0+1, Ws-1),
 *   a = u - x0;  y0, y1, b likewise from v;
 *   val = (1-b)*((1-a)*p[y0,x0] + a*p[y0,x1]) + b*((1-a)*p[y1,x0] + a*p[y1,x1]);  out = floor(val + 0.5) where valid, else 0.
 * u8: `planes` contiguous planes, one map for all of them; optional outputs `valid` (uint8 [Ho,Wo], 255 / 0) and `count`
 * (device int64, 8-byte aligned: zeroed on the stream, receives the number of valid pixels by integer atomics); optional
 * input src_mask.  u16: one plane, same map, same rounding, no mask.  What is written overlaps nothing that is read;
 * every side <= 32768.  The same inputs give the same bits on every run.  A size or `planes` below 1, a null src / dst /
 * lens, a non-finite or non-positive focal length or a non-finite lens term return CLMGS_EINVAL before anything is
 * written. */
int clmgs_undistort_u8(void* stream, int planes, int Hs, int Ws, int Ho, int Wo, const double* lens, int fisheye,
                       double fxo, double fyo, const uint8_t* src, const uint8_t* src_mask, uint8_t* dst, uint8_t* valid,
                       int64_t* count);
int clmgs_undistort_u16(void* stream, int Hs, int Ws, int Ho, int Wo, const double* lens, int fisheye, double fxo,
                        double fyo, const uint16_t* src, uint16_t* dst);

/* ---- compressed models (csrc/vq.hip; clm_gs_amd/compress.py): vector quantisation of the 45 higher-order SH
 * coefficients.  rows [n,48] and codebook [K,48] are float32 in the in-memory SH row layout (coefficient-major, DC in
 * columns 0..2), contiguous and 16-byte aligned; columns 0..2 of both are read and IGNORED (taken as zeros).
 * 1 <= n < 2^31, 1 <= K <= 65536; nothing is allocated.
 *  - clmgs_vq_assign: idx[n] (int32) = argmin_k sum_{j=3..47} (x_j - c_kj)^2, scored as |c_k|^2 - 2 x.c_k with x.c_k a
 *    column-ordered float32 fmaf chain (the exact f32 MFMA) and |c_k|^2 a column-ordered fmaf sum; the lowest k wins an
 *    exact tie of the scores.  dist (optional, float32 [n]) = sum_{j=3..47} (x_j - c_kj)^2 for the k chosen, summed
 *    directly from the winning centroid (exactly 0 for a row equal to its centroid), not as |x|^2 + score.  temp:
 *    clmgs_vq_assign_temp_bytes(K) bytes, 16-byte aligned (the |c_k|^2 of a pre-pass).  Rows and centroids outside
 *    [0,n) x [0,K) are neither read nor written.
 *  - clmgs_vq_accumulate: for every row, counts[idx[row]] += 1 and acc[idx[row], j-3] += rint(double(x_j) * scale) for
 *    j = 3..47, by 64-bit integer atomics only: acc int64 [K,45] and counts int64 [K] are the CALLER's and are added to
 *    (zero them before the first call; several calls sum several chunks of rows).  scale is a power of two with
 *    n_total * max|x| * scale < 2^62.  A row whose idx is outside [0,K) adds nothing.  The sums do not depend on the
 *    order of the rows: the same bits on every run.
 *  - clmgs_vq_finish: codebook[k, j] = float32(double(acc[k, j-3]) / double(counts[k]) / scale) for j = 3..47 where
 *    counts[k] > 0; a centroid with counts[k] == 0 keeps those columns; columns 0..2 of every centroid are written as 0. */
size_t clmgs_vq_assign_temp_bytes(int K);
int clmgs_vq_assign(void* stream, int64_t n, int K, const float* rows, const float* codebook, int32_t* idx, float* dist,
                    void* temp, size_t temp_bytes);
int clmgs_vq_accumulate(void* stream, int64_t n, int K, const float* rows, const int32_t* idx, double scale, int64_t* acc,
                        int64_t* counts);
int clmgs_vq_finish(void* stream, int K, const int64_t* acc, const int64_t* counts, double scale, float* codebook);

/* ---- mesh export (csrc/tsdf.hip, csrc/tsdf_math.h; clm_gs_amd/tsdf.py): TSDF fusion of depth maps into a dense grid and
 * naive Surface Nets.  The volume: nx x ny x nz voxels, x fastest, as ONE contiguous float32 tensor [6, nz, ny, nx] with the
 * planes tsum, wsum, cr, cg, cb, cw; every side >= 2 and nx ny nz < 2^31.  The kernels know nothing of the world frame.
 *  - clmgs_tsdf_integrate fuses B (1..16) cameras of one size H x W (each <= 32768): depth [B,H,W] (expected depth), alpha
 *    [B,H,W], rgb [B,3,H,W], float32 on the device; cams: HOST array [B,16] of doubles, per camera the 12 entries of the
 *    3x4 row-major matrix M that takes the grid point (i + 0.5, j + 0.5, k + 0.5, 1) of voxel (i, j, k) to camera space,
 *    then fx, fy, cx, cy.  Per voxel, for the cameras in the order given (float64, every operation rounded on its own):
 *      x, y, z = M p (each row ((m0 px + m1 py) + m2 pz) + m3);  skip unless z > near
 *      u = fx x / z + cx,  v = fy y / z + cy;  column floor(u), row floor(v) (pixel j covers [j, j + 1)); skip outside
 *      d, a = depth, alpha of that pixel;  skip unless a >= alpha_min and 0 < d <= depth_max
 *      sdf = d - (float) z  (float32);  skip if sdf < -trunc
 *      tsum += fminf(sdf * inv_trunc, 1.0f);  wsum += 1.0f
 *      if sdf <= trunc:  cr, cg, cb += the pixel's colour clamped to [0, 1];  cw += 1.0f
 *    A voxel that no camera of the call observed is neither read nor written.  The sums are sequential in camera order and
 *    a voxel has one owner (no atomics): splitting the cameras into calls differently gives the same bits.  cull: 1 = a
 *    workgroup first tests the box of its 64 x 4 x 8 voxels against every camera's frustum with a margin and skips the
 *    cameras that cannot observe it; 0 = no test; the result is the same, bit for bit.
 *  - extraction, with two inclusive int32 prefix sums taken by the caller in between.  A voxel is valid iff
 *    wsum >= min_weight (> 0) and inside iff tsum < 0; the cell at voxel (i, j, k) is that voxel and its +1 neighbours, and
 *    is active iff all eight are valid and their inside flags differ.  All arrays below have one entry per VOXEL:
 *      clmgs_tsdf_cells:      cell_count[v] = 1 if the cell at voxel v is active, else 0
 *      clmgs_tsdf_vertices:   cell_scan = inclusive prefix sum of cell_count, V = its last entry; vertex cell_scan[v] - 1 of
 *                             every active cell: the mean (float64) of the zero crossings of its sign-changing edges,
 *                             interpolated linearly on tsum / wsum, in grid coordinates, through grid_to_world (HOST, 12
 *                             doubles, 3x4 row-major) rounded to float32 -> verts [V,3]; the same mean of the corner colours
 *                             c / cw (0.5 where cw == 0) as floor(255 c + 0.5) -> colours uint8 [V,3]
 *      clmgs_tsdf_quad_count: quad_count[v] = how many of voxel v's +x, +y, +z grid edges carry a quad: both voxels valid,
 *                             different inside flags, and the four cells around the edge active
 *      clmgs_tsdf_quads:      quad_scan = inclusive prefix sum of quad_count, Q = its last entry (< 2^30); faces int32 [2Q,3]:
 *                             per quad, in (voxel, axis) order, the four cells around the edge right-handed about the axis
 *                             when the owner is inside, reversed otherwise, as two triangles along the diagonal q0 - q2.
 * Every entry returns CLMGS_EINVAL, before anything is launched, for a null or misaligned pointer, outputs that overlap
 * an input or each other, B outside 1..16, a non-finite or non-positive trunc, inv_trunc, fx, fy or min_weight, a
 * non-finite camera or grid_to_world entry, and sizes beyond the limits above. */
int clmgs_tsdf_integrate(void* stream, int nx, int ny, int nz, float* grid, int B, int H, int W, const float* depth,
                         const float* alpha, const float* rgb, const double* cams, float near, float depth_max,
                         float alpha_min, float trunc, float inv_trunc, int cull);
int clmgs_tsdf_cells(void* stream, int nx, int ny, int nz, const float* grid, float min_weight, int32_t* cell_count);
int clmgs_tsdf_vertices(void* stream, int nx, int ny, int nz, const float* grid, const int32_t* cell_scan, int V,
                        const double* grid_to_world, float* verts, uint8_t* colours);
int clmgs_tsdf_quad_count(void* stream, int nx, int ny, int nz, const float* grid, float min_weight,
                          const int32_t* cell_scan, int32_t* quad_count);
int clmgs_tsdf_quads(void* stream, int nx, int ny, int nz, const float* grid, float min_weight, const int32_t* cell_scan,
                     const int32_t* quad_scan, int V, int Q, int32_t* faces);

/* ---- mesh export, sparse volume (csrc/tsdf_sparse.hip, csrc/tsdf_fuse.h; clm_gs_amd/tsdf.py SparseTsdfVolume): the same
 * fusion and extraction on a brick-allocated volume; DESIGN.md section 3, "Sparse volume".  Bricks are 8 x 8 x 8 voxels
 * aligned to the grid origin; the brick grid is nbx x nby x nbz = ceil(n / 8) per axis, at most 2^30 bricks.  marks uint8
 * [nbz, nby, nbx]; table int32 [nbz, nby, nbx]: the slot of a brick or -1; bricks int32 [S]: the linear brick index of every
 * slot, ascending; pool float32 [S, 6, 8, 8, 8] (the six planes of a brick, z, y, x with x fastest); 1 <= S, S * 512 < 2^31.
 *  - clmgs_tsdf_mark stores 1 into marks[] for every brick that can hold a voxel some pixel of the B (1..16) cameras
 *    observes with -trunc <= sdf < 0, or a voxel within 1 voxel of one (a superset: the frustum piece of the pixel square
 *    between the depths max(d, near) (1 - 2^-20) and (d + trunc) (1 + 2^-20), cut into sub-slabs of at most 4 voxels, each
 *    as the bounding box of its eight corners widened by 1 + 2^-16 voxels).  cams: HOST array [B,16] of doubles, per camera
 *    the 12 entries of the 3x4 row-major matrix from camera space to grid coordinates (the inverse of clmgs_tsdf_integrate's
 *    M), then fx, fy, cx, cy, every entry finite and at most 1e30 in magnitude; voxel_cam: the length of a voxel in camera
 *    units, trunc / voxel_cam <= 4096.  Same-value byte stores: the result is a set, independent of the order and the
 *    split of the cameras.  marks is never cleared.
 *  - clmgs_tsdf_sparse_integrate: clmgs_tsdf_integrate on the voxels of the S bricks (one workgroup per brick, the same
 *    cull and camera loop); voxels of a border brick beyond the grid are not touched.
 *  - clmgs_tsdf_sparse_extract: the four extraction passes over the S * 512 slot voxels sv = slot * 512 + (z * 64 + y * 8 + x);
 *    count, cell_scan and quad_scan are int32 [S * 512] in that order.  pass 0: count = cells; pass 1: verts, colours and
 *    vert_keys int64 [V] (the dense linear index (k ny + j) nx + i of the vertex's cell); pass 2: count = quad counts (needs
 *    cell_scan); pass 3: faces int32 [2Q,3] and quad_keys int64 [Q] (3 * the owner's dense linear index + axis), face indices
 *    in the numbering of pass 1.  Sorted by the keys the vertices and quads are in the order of the dense entries.  The
 *    arguments a pass does not use may be null.  A neighbour whose brick is not stored counts as wsum = 0.
 * Every entry returns CLMGS_EINVAL, before anything is launched, for what the dense entries refuse and for a brick grid
 * above 2^30, S outside the limits above or above the brick grid, and a pass outside 0..3. */
int clmgs_tsdf_mark(void* stream, int nx, int ny, int nz, uint8_t* marks, int B, int H, int W, const float* depth,
                    const float* alpha, const double* cams, float near, float depth_max, float alpha_min, float trunc,
                    double voxel_cam);
int clmgs_tsdf_sparse_integrate(void* stream, int nx, int ny, int nz, int S, const int32_t* bricks, float* pool, int B, int H,
                                int W, const float* depth, const float* alpha, const float* rgb, const double* cams, float near,
                                float depth_max, float alpha_min, float trunc, float inv_trunc, int cull);
int clmgs_tsdf_sparse_extract(void* stream, int pass, int nx, int ny, int nz, int S, const int32_t* bricks, const int32_t* table,
                              const float* pool, float min_weight, int32_t* count, const int32_t* cell_scan,
                              const int32_t* quad_scan, int V, int Q, const double* grid_to_world, float* verts, uint8_t* colours,
                              int64_t* vert_keys, int32_t* faces, int64_t* quad_keys);

/* ---- mesh cleanup (csrc/mesh.hip; clm_gs_amd/mesh_clean.py): the connected components of a triangle list and their face
 * counts.  faces int32 [F,3] on the device, any triangle list over V vertices, 1 <= V < 2^31, 1 <= F < 2^31; two vertices
 * are connected when a face names both.  A face with an index outside [0, V) is skipped by every kernel.
 *  - clmgs_mesh_hook and clmgs_mesh_shortcut are the two halves of one labelling round over parent int32 [V], which the
 *    caller starts as 0, 1, .., V - 1: hook lowers, per face, the parents and grandparents of its three vertices to the
 *    smallest grandparent (integer atomic min); shortcut sets parent[v] = parent[parent[v]].  Either stores 1 to *flag
 *    (device int32) when it lowered an entry and leaves it alone otherwise.  The caller alternates them, each round with
 *    a zeroed flag, until a round leaves the flag zero: then parent[v] is the smallest vertex index of v's component (v
 *    itself for a vertex no face names), the same bits whatever the order of the faces.  Neither kernel waits for
 *    another workgroup; the number of rounds grows with the logarithm of a component's diameter.
 *  - clmgs_mesh_component_faces adds 1 to count[labels[faces[f,0]]] for every face (integer atomics, aggregated per run
 *    of equal labels inside a wave); count int32 [V] is zeroed by the caller.
 * Every entry returns CLMGS_EINVAL, before anything is launched, for V < 1 or F < 1, a null or misaligned pointer, and
 * outputs that overlap an input or each other. */
int clmgs_mesh_hook(void* stream, int V, int F, const int32_t* faces, int32_t* parent, int32_t* flag);
int clmgs_mesh_shortcut(void* stream, int V, int32_t* parent, int32_t* flag);
int clmgs_mesh_component_faces(void* stream, int V, int F, const int32_t* faces, const int32_t* labels, int32_t* count);

/* ---- mesh decimation (csrc/mesh_decimate.hip, csrc/decimate_math.h; clm_gs_amd/mesh_decimate.py): vertex clustering on a
 * world-aligned grid of `cell` units with quadric-error representatives; DESIGN.md section 3, "Mesh decimation".  verts
 * float32 [V,3], colours uint8 [V,3], faces int32 [F,3] on the device, 1 <= V < 2^31, 1 <= F < 2^31, cell > 0 and finite.
 * The sorts, prefix sums and compactions between the entries are the caller's.
 *  - clmgs_mesh_decimate_mark stores 1 to mark[v] (uint8 [V], zeroed by the caller) for every vertex a face names.
 *  - clmgs_mesh_decimate_keys writes keys int64 [V]: for a marked vertex ((i + 2^20) << 42) | ((j + 2^20) << 21) |
 *    (k + 2^20) with (i, j, k) = floor(double(x) / cell) per axis, -1 for an unmarked one.  A marked vertex with a
 *    non-finite coordinate ORs 1 into *flag (device int32, zeroed by the caller), one with an index outside
 *    [-2^20, 2^20) ORs 2; their keys are -1.
 *  - clmgs_mesh_decimate_faces maps every face through cluster int32 [V] (the rank of a vertex's key among the C distinct
 *    keys; unmarked vertices are never read): out_faces int32 [F,3] the three clusters rotated so that the smallest comes
 *    first, collapsed uint8 [F] 1 when two of them are equal, inc int64 [3F] one entry (cluster << 32 | face) per
 *    DISTINCT cluster among the corners and INT64_MAX in the unused slots.
 *  - clmgs_mesh_decimate_place, one lane per cluster, forms the output vertex of each of the C clusters.  lane_order int32
 *    [C] is a permutation of the clusters: lane t of the launch takes cluster lane_order[t].  Any permutation gives the
 *    same output; one that puts clusters whose vertices are neighbours in memory on neighbouring lanes is faster.
 *    cluster_keys int64 [C] ascending; vert_order int32 [n_members] the marked vertices ordered by cluster then index and
 *    vert_start int64 [C + 1] the segments of that list; inc int64 [n_inc] the used incidences sorted ascending
 *    (cluster, then face) and inc_start int64 [C + 1] their segments.  It sums in float64 without
 *    contraction, in list order, solves
 *    (A + mu I) x = r + mu m by the adjugate and writes out_verts float32 [C,3], out_colours uint8 [C,3] (the channel
 *    means, rounded half up, in integers) and code uint8 [C]: 0 the quadric's minimiser, 1 the mean because the quadric is
 *    degenerate, 2 the mean because the minimiser lies more than `cell` from the cell's centre along an axis.
 * Every entry returns CLMGS_EINVAL, before anything is launched, for a size outside its range, a bad cell, a null or
 * misaligned pointer, and outputs that overlap an input or each other.  An index read from memory that lies outside its
 * array is skipped by every kernel. */
int clmgs_mesh_decimate_mark(void* stream, int V, int F, const int32_t* faces, uint8_t* mark);
int clmgs_mesh_decimate_keys(void* stream, int V, const float* verts, const uint8_t* mark, double cell, int64_t* keys,
                             int32_t* flag);
int clmgs_mesh_decimate_faces(void* stream, int V, int F, int C, const int32_t* faces, const int32_t* cluster,
                              int32_t* out_faces, uint8_t* collapsed, int64_t* inc);
int clmgs_mesh_decimate_place(void* stream, int V, int F, int C, const float* verts, const uint8_t* colours,
                              const int32_t* faces, const int64_t* cluster_keys, const int32_t* vert_order,
                              const int64_t* vert_start, int64_t n_members, const int64_t* inc, const int64_t* inc_start,
                              int64_t n_inc, const int32_t* lane_order, double cell, float* out_verts, uint8_t* out_colours,
                              uint8_t* code);

/* ---- mesh smoothing and vertex normals (csrc/mesh_smooth.hip, csrc/mesh_vertex_math.h; clm_gs_amd/mesh_smooth.py):
 * DESIGN.md section 3, "Mesh smoothing and normals".  verts float32 [V,3] and faces int32 [F,3] on the device,
 * 1 <= V < 2^31, 1 <= F < 2^31.  order int64 [3F] holds the corner slots e = 3 f + k sorted by the vertex faces[f,k],
 * ascending e within a vertex (a stable sort); start int64 [V + 1] the segment boundaries.  Both lists are the caller's.
 * One lane per vertex walks its segment; all sums are float64, left to right, without contraction.
 *  - clmgs_mesh_smooth_step writes verts_out float32 [V,3], a buffer apart from verts_in: per entry s += p[faces[f,(k+1)%3]],
 *    then s += p[faces[f,(k+2)%3]], n += 2; out = float32(p + factor * (s / double(n) - p)), or p's own bits for n == 0.
 *    factor is finite.  A face that names a vertex twice is in its segment twice.
 *  - clmgs_mesh_vertex_normals writes normals float32 [V,3]: per entry a += (p1 - p0) x (p2 - p0) from the corners of f in
 *    stored order; q = (a0 a0 + a1 a1) + a2 a2; float32(a * (1.0 / sqrt(q))) for a finite q > 0, else (0, 0, 0).
 * Both return CLMGS_EINVAL, before anything is launched, for a size outside its range, a non-finite factor, a null or
 * misaligned pointer, and an output that overlaps an input.  An index read from memory that lies outside its array is
 * skipped by both kernels. */
int clmgs_mesh_smooth_step(void* stream, int V, int F, const float* verts_in, const int32_t* faces, const int64_t* order,
                           const int64_t* start, double factor, float* verts_out);
int clmgs_mesh_vertex_normals(void* stream, int V, int F, const float* verts, const int32_t* faces, const int64_t* order,
                              const int64_t* start, float* normals);

/* ---- mesh evaluation (csrc/mesh_distance.hip, csrc/mesh_distance_math.h; clm_gs_amd/mesh_eval.py): DESIGN.md section 3,
 * "Mesh evaluation".  verts float32 [V,3] and faces int32 [F,3] on the device, 1 <= V < 2^31, 1 <= F < 2^31.  All
 * arithmetic is float64 without contraction, in the order of csrc/mesh_distance_math.h.
 *  - clmgs_mesh_sample_count, one lane per face: area float64 [F] = 0.5 sqrt(|(b - a) x (c - a)|^2) and count int64 [F] =
 *    min(max(ceil(area / spacing^2), 1), 2^31), or 0 for a face whose area is zero or not finite (no primitive) or that
 *    names a vertex outside [0, V) (area 0).
 *  - clmgs_mesh_sample_emit, one lane per sample: offsets int64 [F+1] the exclusive prefix sum of count, sample_face
 *    int32 [S] the face of every sample (ascending), 1 <= S < 2^31.  Sample s of face f is number k = s - offsets[f] of
 *    n = offsets[f+1] - offsets[f]: u = frac(0.5 + (k+1) 0.7548776662466927), v = frac(0.5 + (k+1) 0.5698402909980532),
 *    both replaced by one minus themselves when u + v > 1; points float32 [S,3] = float32((a + u (b - a)) + v (c - a)),
 *    weight float64 [S] = area[f] / n.  A sample whose face or number is out of range gets zeros.
 *  - The primitive grid: origin (ox, oy, oz), cell size h > 0, gx x gy x gz cells, each at most 2^20 and at most 2^27 in
 *    all; the cell of a coordinate along an axis is clamp(floor((x - o) / h), 0, g - 1).  The primitives are the N = F
 *    triangles, or, with faces == NULL, the N = V points.  A face without a positive finite area and a point with a
 *    non-finite coordinate are not primitives.  clmgs_mesh_bin_count, one lane per primitive, writes count int64 [N]: the
 *    number of cells in the index range of its bounding box (0 for what is no primitive).  clmgs_mesh_bin_emit writes, at
 *    offsets[i] (int64 [N+1], the exclusive prefix sum), the pairs cell int64 [pairs] = (z gy + y) gx + x and prim int32
 *    [pairs] = i of that range, x fastest.
 *  - clmgs_mesh_distance, one lane per query: queries float32 [P,3]; cell_start int64 [gx gy gz + 1] and pair_prim int32
 *    [pairs] the pairs sorted by cell.  The lane walks growing Chebyshev shells of cells around the clamped cell of its
 *    query and keeps the smallest squared distance (md_closest_d2 / md_point_d2), ties to the smaller primitive index; it
 *    stops after shell R once best < (R h (1 - 2^-16))^2 or R h (1 - 2^-16) > max_distance.  dist float32 [P] =
 *    float32(sqrt(best)), prim int32 [P]; (+inf, -1) when sqrt(best) > max_distance, when there is no primitive, and for
 *    a query with a non-finite coordinate.  The result equals the minimum over ALL primitives for any h.  evaluated
 *    int32 [P] (or NULL): the number of primitives the lane evaluated.
 * Every entry returns CLMGS_EINVAL, before anything is launched, for a size outside its range, a spacing, cell size or
 * max_distance that is not positive (or NaN), a grid beyond the limits and a null or misaligned pointer.  An index read
 * from memory that lies outside its array is skipped by every kernel. */
int clmgs_mesh_sample_count(void* stream, int V, int F, const float* verts, const int32_t* faces, double spacing,
                            double* area, int64_t* count);
int clmgs_mesh_sample_emit(void* stream, int V, int F, const float* verts, const int32_t* faces, const double* area,
                           const int64_t* offsets, const int32_t* sample_face, int64_t S, float* points, double* weight);
int clmgs_mesh_bin_count(void* stream, int V, int N, const float* verts, const int32_t* faces, double ox, double oy,
                         double oz, double h, int gx, int gy, int gz, int64_t* count);
int clmgs_mesh_bin_emit(void* stream, int V, int N, const float* verts, const int32_t* faces, double ox, double oy, double oz,
                        double h, int gx, int gy, int gz, const int64_t* offsets, int64_t pairs, int64_t* cell,
                        int32_t* prim);
int clmgs_mesh_distance(void* stream, int64_t P, const float* queries, int V, int N, const float* verts,
                        const int32_t* faces, double ox, double oy, double oz, double h, int gx, int gy, int gz,
                        const int64_t* cell_start, const int32_t* pair_prim, int64_t pairs, double max_distance, float* dist,
                        int32_t* prim, int32_t* evaluated);

/* ---- pinned host memory  (numba.cuda.pinned_array at clm_offload/gaussian_model.py:34-44) */
void* clmgs_pinned_alloc(size_t bytes);
int clmgs_pinned_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* CLMGS_H */
