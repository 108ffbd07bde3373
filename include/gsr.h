/*
 * gsr.h -- C ABI of libgsr_hip.so, the MI355X (gfx950) differentiable Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary for ONE path of graphdeco-inria/gaussian-splatting: the native
 * operator behind `GaussianRasterizer` / `GaussianRasterizationSettings`
 * (reference call sites: gaussian_renderer/__init__.py:14, :36-52, :91-110; backward via
 * loss.backward() at train.py:142).  In the reference that operator lives in the un-vendored
 * submodule `submodules/diff-gaussian-rasterization` (.gitmodules:4-7) whose torch extension `_C`
 * exports `rasterize_gaussians`, `rasterize_gaussians_backward` and `mark_visible`; each entry point
 * below names the `_C` function it replaces.  A maintainer binds these with ctypes (see
 * INTEGRATION.md; gaussian-splatting_amd/diff_gaussian_rasterization/_lib.py is that binding).
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch / C++ types; every data pointer is a DEVICE pointer
 *     (tensor.data_ptr()) to contiguous fp32 / int32 data unless stated otherwise.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *     gsr_rasterize_forward learns num_rendered (it sizes the binning buffer) mid-pipeline like the reference, but
 *     without hipStreamSynchronize and -- since ABI 4 -- off the critical path: the count does not depend on the depth
 *     order, so the per-Gaussian preprocess kernel sums it and its last workgroup stores the 64-bit count + a sequence
 *     number into a mapped, pinned host word; the calling thread queues the depth sort, then polls the word (200 us of
 *     spinning, then sched_yield() between polls).
 *   - return value: GSR_OK (0) or a negative GsrStatus; gsr_last_error() gives the message for the
 *     calling thread.  No exception crosses the ABI.
 *   - no per-frame device allocation inside: scratch memory is caller-owned and obtained through the three
 *     resize callbacks (geometry / binning / image state), exactly like the reference's
 *     resizeFunctional lambdas; forward returns with the three buffers populated and the caller keeps
 *     them alive for gsr_rasterize_backward.  The library itself owns only a few 64-byte CONTROL BLOCKS per device,
 *     created the first time a device (or one more concurrent caller on it) is seen and kept for the life of the
 *     process: the mapped host word of the read-back above, a 64-byte device counter beside it, one mapped
 *     "oversized depth bucket" flag, and -- only when option fwd_bands > 1 -- one auxiliary HIP stream with five
 *     events.  Their creation (hipHostMalloc / hipMalloc / hipStreamCreate) synchronises the device once; do the
 *     first call outside a stream capture.
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_ABI_VERSION 4

typedef enum GsrStatus {
    GSR_OK = 0,
    GSR_ERR_INVALID_ARG = -1,   /* bad size / NULL pointer / inconsistent optional inputs */
    GSR_ERR_HIP = -2,           /* a HIP runtime call or kernel launch failed */
    GSR_ERR_ALLOC = -3,         /* a resize callback returned NULL */
    GSR_ERR_UNSUPPORTED = -4    /* e.g. more than 2^24 tiles, SH degree > 3 */
} GsrStatus;

/* Mirrors GaussianRasterizationSettings (gaussian_renderer/__init__.py:36-50), same field meaning.
 * bg / viewmatrix / projmatrix / campos are device pointers (they are CUDA tensors in the
 * reference).  viewmatrix / projmatrix are the row-major tensors the reference passes, i.e. the
 * TRANSPOSED math matrices (scene/cameras.py:86-88): flat index i + 4*j = math element (row i, col j). */
typedef struct GsrRasterSettings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    const float* bg;          /* [3] */
    float scale_modifier;
    const float* viewmatrix;  /* [16] */
    const float* projmatrix;  /* [16] */
    int32_t sh_degree;        /* active degree 0..3 */
    const float* campos;      /* [3] */
    int32_t prefiltered;      /* always 0 in the reference (gaussian_renderer/__init__.py:47) */
    int32_t debug;            /* 1: synchronise + check after every kernel */
    int32_t antialiasing;
    /* Extension for screen-tile sharding across GPUs (not in the reference):
     * only tile rows [tile_y0, tile_y1) are binned and rendered; pixels outside are left untouched.
     * tile_y1 <= 0 means "all rows". radii are unaffected by the band. */
    int32_t tile_y0;
    int32_t tile_y1;
    /* Extension: 1 = the caller will not run the backward for this forward (inference / torch.no_grad()): state that only
     * the backward reads (final_T, n_contrib, first-emission indices) is not written.  0 = reference behaviour. */
    int32_t no_backward;
    /* Extension -- the "separate_sh" call form the reference uses when its accelerated rasterizer is installed
     * (gaussian_renderer/__init__.py:82-100: rasterizer(dc = features_dc, shs = features_rest, ...)): when sh_dc is
     * non-NULL, SH coefficient 0 is read from sh_dc[P,1,3] and `shs` holds coefficients 1..M-1 as [P,M-1,3] (M still
     * counts ALL coefficients; supported for degree-3 storage, M == 16, with 16-byte aligned pointers -- else
     * GSR_ERR_UNSUPPORTED and the caller concatenates).  In the backward dL_dsh then receives [P,M-1,3] and dL_dsh_dc[P,1,3] the
     * gradient of the DC term.  This avoids the torch.cat of the two parameter tensors (scene/gaussian_model.py:121-125)
     * and the split of its gradient in every iteration.  Both NULL = fused [P,M,3] form. */
    const float* sh_dc;
    float* dL_dsh_dc;
} GsrRasterSettings;

/* Resize callback: make the buffer at least `bytes` long and return its (device) base address,
 * 128-byte aligned or better.  Mirrors the reference's std::function<char*(size_t)> lambdas that
 * call tensor.resize_(). */
typedef void* (*GsrResizeFn)(void* user, size_t bytes);

int gsr_abi_version(void);
const char* gsr_last_error(void);

/* Scratch sizes (bytes) -- mirrors the reference's required<GeometryState/BinningState/ImageState>(). */
size_t gsr_geometry_bytes(int P);
size_t gsr_binning_bytes(int64_t R, int n_tiles);
size_t gsr_image_bytes(int width, int height);
size_t gsr_backward_scratch_bytes(int P, int64_t R);

/*
 * Replaces _C.rasterize_gaussians.
 *   P            number of Gaussians; M = SH coefficients per channel in `shs` ((max_degree+1)^2).
 *   means3D[P,3], opacities[P], shs[P,M,3] XOR colors_precomp[P,3],
 *   (scales[P,3] AND rotations[P,4]) XOR cov3D_precomp[P,6]; absent inputs are NULL.
 *   out_color[3,H,W], out_invdepth[1,H,W] (may be NULL), radii[P] int32.
 *   *num_rendered receives R, the number of (Gaussian, tile) instances that were binned: the tiles of the snug rectangle of
 *   every Gaussian's alpha >= 1/255 ellipse (option snug_tiles), a subset of the reference's tile square -- the reference would
 *   report ~1.4x as many for the same frame; the rendered outputs are the same bits.
 * P == 0: out_color / out_invdepth are zero-filled, *num_rendered = 0, no callback is invoked.
 */
int gsr_rasterize_forward(const GsrRasterSettings* settings, int P, int M,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities, const float* scales, const float* rotations,
                          const float* cov3D_precomp,
                          GsrResizeFn geom_resize, void* geom_user,
                          GsrResizeFn binning_resize, void* binning_user,
                          GsrResizeFn image_resize, void* image_user,
                          float* out_color, float* out_invdepth, int32_t* radii,
                          int32_t* num_rendered, void* stream);

/*
 * Replaces _C.rasterize_gaussians_backward.
 *   geom/binning/image buffers: the three buffers forward filled (same P, R, settings, inputs).
 *   dL_dout_color[3,H,W]; dL_dout_invdepth[1,H,W] or NULL (treated as zero).
 * Outputs (every element is overwritten -- zeros for Gaussians with radii == 0 -- so the caller may pass
 * uninitialised memory; the reference's glue allocates them with torch::zeros):
 *   dL_dmeans2D[P,3]  (x,y in NDC-scaled units = pixel gradient * (0.5 W, 0.5 H); z = 0)
 *   dL_dcolors[P,3] (may be NULL unless colors_precomp was given: it is an intermediate otherwise), dL_dopacity[P],
 *   dL_dmeans3D[P,3], dL_dcov3D[P,6] (may be NULL unless cov3D_precomp was given), dL_dsh[P,M,3] (NULL if no shs),
 *   dL_dscales[P,3], dL_drotations[P,4] (NULL if cov3D_precomp was given).
 *   bwd_scratch: caller-owned scratch of gsr_backward_scratch_bytes(P, num_rendered) bytes (per-instance
 *   gradient records, the emission-order inverse map and the per-Gaussian 2-D gradient record).
 *   If splat_grads_out is non-NULL it receives the device address (inside bwd_scratch) of the per-Gaussian
 *   record [P,12] = [dpx,dpy,dA,dB,dC,dopacity,dr,dg,db,dinvdepth,0,0] (words 10, 11: gsr_backward_blend_abs) -- the 48-byte payload that is
 *   reduce-scattered between GPUs when the screen is sharded.
 */
int gsr_rasterize_backward(const GsrRasterSettings* settings, int P, int M, int32_t num_rendered,
                           const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, const float* rotations,
                           const float* cov3D_precomp, const int32_t* radii,
                           const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                           const float* dL_dout_color, const float* dL_dout_invdepth,
                           float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                           float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                           float* dL_dscales, float* dL_drotations, void* bwd_scratch,
                           float** splat_grads_out, void* stream);

/*
 * The two halves of gsr_rasterize_backward, exposed separately for screen-sharded multi-GPU training (SURVEY.md 8(e),
 * no reference counterpart): every rank runs gsr_backward_blend on its own band of tiles, the 48-byte per-Gaussian
 * records ([P,12], pointer returned in *splat_grads_out) are summed across ranks (RCCL all-reduce / reduce-scatter),
 * and gsr_backward_preprocess turns the summed records into the parameter gradients.
 * gsr_rasterize_backward == gsr_backward_blend followed by gsr_backward_preprocess on the same record array.
 */
int gsr_backward_blend(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                       const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                       const float* dL_dout_color, const float* dL_dout_invdepth,
                       void* bwd_scratch, float** splat_grads_out, void* stream);
int gsr_backward_preprocess(const GsrRasterSettings* settings, int P, int M,
                            const float* means3D, const float* shs, const float* colors_precomp,
                            const float* opacities, const float* scales, const float* rotations,
                            const float* cov3D_precomp, const int32_t* radii, const void* geom_buffer,
                            const float* splat_grads,
                            float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                            float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                            float* dL_dscales, float* dL_drotations, void* stream);

/*
 * Camera gradients (no reference counterpart): gsr_backward_preprocess that also returns dL/d(viewmatrix), dL/d(projmatrix) and
 * dL/d(campos).  Every other output is the same bits as gsr_backward_preprocess writes for the same inputs.
 * Contract: the gradient of the same function whose Gaussian gradients the backward returns, under the same conventions -- the
 * frustum-clamp stop-gradient, and no gradient through culling, radii, tile assignment, depth order or the alpha >= 1/255 and
 * transmittance cut-offs.  Per visible Gaussian (radii > 0), with p = (x, y, z, 1) and math matrices V, P:
 *   view rows 0-2:          dL/dV[r][j] += dt_r p_j   (dt = dL/d(view-space position), after the clamp masks), and for j < 3 the
 *                           covariance path through T = J W:  dW0j += J00 dT0j,  dW1j += J11 dT1j,  dW2j += J02 dT0j + J12 dT1j
 *   projection rows 0, 1, 3: dL/dP[0][j] += dhx p_j,  dL/dP[1][j] += dhy p_j,  dL/dP[3][j] += dhw p_j  (dh = dL/d(clip position))
 *   campos:                 dL/dcampos -= the SH backward's view-direction term of dL/dmean (zero with colors_precomp)
 *   View row 3 and projection row 2 are read by no kernel: their gradients are exactly 0.
 * The outputs are in the layout of viewmatrix / projmatrix (flat index i + 4*j = math element (row i, col j)), so a caller that
 * builds projmatrix = viewmatrix @ proj and campos = inverse(viewmatrix)[3, :3] chains through them with no further convention.
 * The three outputs are OVERWRITTEN (fp32, summed in fp64 in a fixed order: bit-reproducible); P == 0 writes zeros.
 * scratch: device memory of gsr_camera_grad_scratch_bytes(P) bytes, 8-byte aligned.  Every input form of gsr_backward_preprocess
 * is accepted (fused SH of any M, split sh_dc, colors_precomp, cov3D_precomp, antialiasing, with or without the inverse-depth
 * gradient in the records).  A screen-sharded caller gets its band's contribution from its own records.
 */
typedef struct GsrCameraGrads {
    float* dL_dviewmatrix;    /* [16] */
    float* dL_dprojmatrix;    /* [16] */
    float* dL_dcampos;        /* [3] */
    void* scratch;            /* gsr_camera_grad_scratch_bytes(P) */
} GsrCameraGrads;
size_t gsr_camera_grad_scratch_bytes(int P);
int gsr_backward_preprocess_camera(const GsrRasterSettings* settings, int P, int M,
                                   const float* means3D, const float* shs, const float* colors_precomp,
                                   const float* opacities, const float* scales, const float* rotations,
                                   const float* cov3D_precomp, const int32_t* radii, const void* geom_buffer,
                                   const float* splat_grads,
                                   float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                                   float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                   float* dL_dscales, float* dL_drotations, const GsrCameraGrads* camera, void* stream);

/*
 * Differentiable alpha image and per-pixel / learnable background (no reference counterpart): gsr_rasterize_forward and
 * gsr_backward_blend with one extra struct.  Per pixel, over the contributors i the forward blends (the same skip, 0.99 cap and
 * termination rules, nothing new):
 *   T_final = prod_i (1 - alpha_i)                          the transmittance the forward freezes at termination
 *   alpha   = 1 - T_final                                   out_alpha[1,H,W]
 *   color   = sum_i c_i alpha_i T_i + T_final * B(pixel)    B = settings->bg[3] broadcast, or bg_image[3,H,W] when given
 * Backward, in addition to what gsr_backward_blend computes:
 *   dL/dalpha_i            += (-T_final / (1 - alpha_i)) * (<B(pixel), dL/dC(pixel)> - dL/dalpha_image(pixel))
 *   dL_dbg_image[c][pixel]  = T_final(pixel) * dL/dC[c][pixel]     every pixel, also where no Gaussian contributes (T_final = 1)
 *   dL_dbg[c]               = sum over the pixels of the line above (fp64 products and sums in a fixed order, one rounding to fp32)
 * Conventions: those of the other gradients -- no gradient through culling, radii, tile assignment, depth order or the
 * alpha >= 1/255 and T < 1e-4 cut-offs; the 0.99 cap is passed straight through as for colour.  With a band of tile rows
 * (tile_y0 / tile_y1) out_alpha is written inside the band only (like out_color), and dL_dbg_image / dL_dbg are the band's
 * contribution: zero outside it.  P == 0: the composite forward writes alpha = 0 and color = B (gsr_rasterize_forward keeps the
 * reference's zero image), and the backward writes dL_dbg_image = dL/dC and its sum; it needs no state buffer then.
 * Every optional pointer may be NULL; with all of them NULL the two calls write the same bits as gsr_rasterize_forward /
 * gsr_backward_blend for P > 0, and a NULL `extra` itself is GSR_ERR_INVALID_ARG.  settings->bg must stay a valid pointer; it is not read
 * when bg_image is given.  The backward's bg_image must be the forward's.  dL_dbg_image and dL_dbg are OVERWRITTEN, bit-reproducible
 * (no atomics); dL_dbg needs `scratch`: device memory of gsr_composite_grad_scratch_bytes(width, height) bytes, 8-byte aligned.
 * The [P,12] records keep their layout, so gsr_backward_preprocess, gsr_backward_preprocess_camera and
 * gsr_backward_preprocess_sh_adam all follow gsr_backward_blend_composite unchanged.
 */
typedef struct GsrCompositeOut {
    float* out_alpha;             /* [1,H,W] or NULL */
    const float* bg_image;        /* [3,H,W] or NULL (then settings->bg) */
} GsrCompositeOut;
int gsr_rasterize_forward_composite(const GsrRasterSettings* settings, int P, int M,
                                    const float* means3D, const float* shs, const float* colors_precomp,
                                    const float* opacities, const float* scales, const float* rotations,
                                    const float* cov3D_precomp,
                                    GsrResizeFn geom_resize, void* geom_user,
                                    GsrResizeFn binning_resize, void* binning_user,
                                    GsrResizeFn image_resize, void* image_user,
                                    float* out_color, float* out_invdepth, int32_t* radii,
                                    int32_t* num_rendered, const GsrCompositeOut* extra, void* stream);
typedef struct GsrCompositeGrads {
    const float* dL_dout_alpha;   /* [1,H,W] or NULL (treated as zero) */
    const float* bg_image;        /* as in the forward */
    float* dL_dbg_image;          /* [3,H,W] or NULL */
    float* dL_dbg;                /* [3] or NULL */
    void* scratch;                /* gsr_composite_grad_scratch_bytes(width, height); needed for dL_dbg only */
} GsrCompositeGrads;
size_t gsr_composite_grad_scratch_bytes(int width, int height);
int gsr_backward_blend_composite(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                                 const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                 const float* dL_dout_color, const float* dL_dout_invdepth,
                                 void* bwd_scratch, float** splat_grads_out,
                                 const GsrCompositeGrads* extra, void* stream);

/*
 * Absolute screen-space gradients (no reference counterpart; the densification signal of AbsGS, gsplat's `absgrad`): the blend backward
 * that also returns, per Gaussian, the sum over pixels of the ABSOLUTE per-pixel gradient of its 2-D centre -- the signed sums of words
 * 0, 1 cancel where a large Gaussian covers fine detail, and density control then never splits it.
 * For Gaussian g and every pixel p of the rendered band at which the blend backward takes g -- the hard masks of the signed gradient,
 * nothing re-tested and nothing new: list position < n_contrib[p], power <= 0, alpha >= 1/255 -- with dx = mean2D.x - p.x,
 * dy = mean2D.y - p.y, the conic (A, B, C) and
 *   m_gp = opacity * G * dL/dalpha_gp      the backward's own m, straight through the 0.99 cap, including the background, alpha-image and
 *                                          inverse-depth terms when present,
 *   abs_x[g] = sum_p | m_gp (A dx + B dy) |        abs_y[g] = sum_p | m_gp (C dy + B dx) |
 * Products and sums are fp32, the summation order is fixed (two runs give the same bits), there are no atomics.
 * gsr_backward_blend_abs takes the arguments of gsr_backward_blend_composite, except that `extra` may be NULL (then it is gsr_backward_blend
 * with the two sums).  In the [P,12] records abs_x, abs_y are words 10, 11, in pixel units like words 0, 1; words 0 to 9 are the bits
 * gsr_backward_blend / gsr_backward_blend_composite write for the same inputs, and so is everything `extra` returns.  Rows without a
 * contributing pixel (culled Gaussians included) are zero.  With a band of tile rows the two words are the band's contribution; sums of
 * non-negative terms over disjoint bands add up to the full frame's, so the records stay correct under the all-reduce / reduce-scatter
 * of the sharded modes.  Every state gsr_backward_blend accepts is accepted (the record entry points' included); P == 0 or
 * num_rendered == 0 gives zero rows.  bwd_scratch is that of gsr_backward_blend (gsr_backward_scratch_bytes).  Builds with the
 * measurement variants (-DGSR_AB_VARIANTS) and a render_bwd_variant other than the default return GSR_ERR_UNSUPPORTED.
 * gsr_absgrad_from_records converts records into means2D_abs[P,3] = (0.5 W abs_x, 0.5 H abs_y, 0): the units and layout of
 * dL_dmeans2D, so it drops into gsr_density_stats unchanged.  Every row is overwritten; splat_grads must be 8-byte aligned.
 */
int gsr_backward_blend_abs(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                           const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                           const float* dL_dout_color, const float* dL_dout_invdepth,
                           void* bwd_scratch, float** splat_grads_out,
                           const GsrCompositeGrads* extra /* may be NULL */, void* stream);
int gsr_absgrad_from_records(const GsrRasterSettings* settings, int P, const float* splat_grads,
                             float* means2D_abs /* [P,3] */, void* stream);

/*
 * Per-Gaussian blend-weight statistics (no reference counterpart): what each Gaussian GAVE to the image of one forward -- the
 * importance scores of pruning (sum or max of alpha T), error-weighted densification scores and hit counts -- read from the state
 * that gsr_rasterize_forward / gsr_rasterize_forward_composite leave when run with no_backward == 0 (the same settings, the same
 * buffers, num_rendered as returned).  The states of the record entry points (from_splats / from_packed / from_segments) are not
 * supported.  Nothing is differentiable.
 * Gaussian i contributes to pixel p of the rendered band exactly when the forward blended it there: its entry is valid
 * (power <= 0 and alpha >= 1/255, alpha capped at 0.99) and its list position is <= n_contrib[p]; n_contrib is the authority on
 * termination (T < 1e-4 is not re-tested).  w_ip = alpha_ip * T_ip, T_ip the product of (1 - alpha) over the valid entries in
 * front of it: the forward's blend weight.  E = pixel_weight[H,W], NULL meaning 1 everywhere; a pixel with E(p) == 0 is excluded
 * from all three statistics, so E also serves as a mask.
 *   weight_sum[i]  = sum_p E(p) w_ip
 *   weight_max[i]  = max(0, max_p E(p) w_ip)
 *   pixel_count[i] = number of pixels p with E(p) != 0 that i contributes to
 * Every one of the P rows is written (zeros for culled and non-contributing Gaussians).  accumulate == 1 combines the frame's
 * finished per-Gaussian value with the stored one instead: sum <- sum + frame (one fp32 add), max <- max(max, frame),
 * count <- count + frame -- scores over many views build up in place.  P == 0 or num_rendered == 0: zeros with accumulate == 0,
 * the arrays left as they are with accumulate == 1.  With a band of tile rows (tile_y0 / tile_y1) the statistics are the band's
 * contribution.  Bit-reproducible: no atomics, every sum in a fixed order.  Each output pointer may be NULL.
 * `scratch`: device memory of gsr_contribution_scratch_bytes(P, num_rendered) bytes, 16-byte aligned, contents undefined before and
 * after.  A NULL `out`, or a NULL scratch with num_rendered > 0, is GSR_ERR_INVALID_ARG.
 */
typedef struct GsrContribOut {
    float*   weight_sum;    /* [P] or NULL */
    float*   weight_max;    /* [P] or NULL */
    int32_t* pixel_count;   /* [P] or NULL */
    int32_t  accumulate;    /* 0 overwrite, 1 combine as defined above */
    int32_t  reserved;
} GsrContribOut;
size_t gsr_contribution_scratch_bytes(int P, int64_t R);
int gsr_contribution_stats(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                           const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                           const float* pixel_weight /* [H,W] or NULL */, void* scratch,
                           const GsrContribOut* out, void* stream);

/*
 * Per-pixel probe (no reference counterpart): what one forward meant for every PIXEL beyond colour, inverse depth and alpha -- depth
 * maps that can be fused, the Gaussian under a pixel, the number of blended Gaussians -- read from the state of
 * gsr_contribution_stats: gsr_rasterize_forward / gsr_rasterize_forward_composite run with no_backward == 0, the same settings, the
 * same buffers, num_rendered as returned.  The states of the record entry points (from_splats / from_packed / from_segments) are not
 * supported.  Nothing is differentiable.
 * Conventions, those of gsr_contribution_stats: Gaussian g contributes to pixel p exactly when the forward blended it there -- its entry
 * is valid (power <= 0 and alpha >= 1/255, alpha capped at 0.99) and its list position is <= n_contrib[p]; n_contrib is the authority
 * on termination (T < 1e-4 is not re-tested).  Front to back, T is the product of (1 - alpha) over the contributors in front of an
 * entry, w = alpha * T its blend weight, T' = T (1 - alpha) the transmittance behind it, z its view-space depth (the preprocess's
 * depth, the 1/z of out_invdepth) and g the caller's Gaussian index.  Per pixel of the rendered band:
 *   expected_depth            = sum over contributors of w z, summed in fp32 in list order.  NOT normalised: divide by alpha
 *                               (1 - T_final) for the normalised form.  Complements out_invdepth = sum w / z.
 *   median_depth, median_id   = z and g of the FIRST contributor with T' < threshold (0.5: the median depth, where transmittance
 *                               crosses 1/2); 0.0f and -1 if the pixel has none.
 *   top_id, top_weight        = g and w of the contributor with the largest w; a later one replaces an earlier one on strict >
 *                               only, so the nearest wins exact ties; -1 and 0.0f without a contributor.
 *   count                     = number of contributors (n_contrib is a list position, not a count).
 * Every pixel of the band inside the image is written, pixels without a contributor with the defaults above (0.0f, 0.0f, -1, -1,
 * 0.0f, 0); with a band of tile rows (tile_y0 / tile_y1) pixels outside the band are not touched.  P == 0 or num_rendered == 0: the
 * defaults are written over the band and the state buffers are not read (they may be NULL).  Bit-reproducible: one lane per pixel,
 * fixed order, no atomics.  No scratch.  Each output pointer may be NULL.  A NULL `out`, a threshold outside (0,1) or NaN, negative
 * P / num_rendered, or NULL state buffers with P > 0 and num_rendered > 0 are GSR_ERR_INVALID_ARG.
 */
typedef struct GsrPixelProbeOut {
    float*   expected_depth;  /* [H,W] or NULL */
    float*   median_depth;    /* [H,W] or NULL */
    int32_t* median_id;       /* [H,W] or NULL */
    int32_t* top_id;          /* [H,W] or NULL */
    float*   top_weight;      /* [H,W] or NULL */
    int32_t* count;           /* [H,W] or NULL */
    float    threshold;       /* transmittance threshold of the median, 0 < t < 1 (0.5: the median) */
    int32_t  reserved;
} GsrPixelProbeOut;
int gsr_pixel_probe(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                    const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                    const GsrPixelProbeOut* out, void* stream);

/*
 * N-channel per-Gaussian features blended with the weights of a forward that has ALREADY run (no reference counterpart): language / semantic
 * feature fields, distillation heads, label lifting -- any number of channels on the geometry of one frame, without one forward and one blend
 * backward per three channels.  Read from the state of gsr_contribution_stats / gsr_pixel_probe: gsr_rasterize_forward /
 * gsr_rasterize_forward_composite run with no_backward == 0, the same settings, the same buffers, num_rendered as returned.  The states of the
 * record entry points (from_splats / from_packed / from_segments) are not supported.
 * Conventions, those two functions': Gaussian g contributes to pixel p exactly when the forward blended it there -- its entry is valid
 * (power <= 0 and alpha >= 1/255, alpha capped at 0.99) and its list position is <= n_contrib[p]; n_contrib is the authority on termination
 * (T < 1e-4 is not re-tested); w_gp = alpha_gp * T_gp is the forward's blend weight.
 *   gsr_render_features            out[c,p] = sum_g w_gp features[g,c], fp32 in list order.  NO background term and no normalisation: compose
 *                                  with the alpha image of gsr_rasterize_forward_composite (1 - alpha is the weight of a background).
 *   gsr_render_features_backward   dL_dfeatures[g,c] = sum_p w_gp dL_dout[c,p]: the gradient with respect to `features` ONLY.  Geometry and
 *                                  opacity are constants of the frame already rendered; gradients to them through `out` are the business
 *                                  of gsr_render_features_backward_geometry below.
 * features / dL_dfeatures are [P,C] row-major, out / dL_dout planar [C,H,W], 1 <= C <= GSR_MAX_FEATURE_CHANNELS.  Rows of `features` of
 * Gaussians that contribute nowhere (culled, hidden) are never multiplied into the image -- they may hold anything -- and their rows of
 * dL_dfeatures are exact zeros; every one of the P rows is written.  Every pixel of the band inside the image is written (zeros without a
 * contributor); with a band of tile rows (tile_y0 / tile_y1) pixels of `out` outside the band are not touched, dL_dout is read inside the band
 * only and dL_dfeatures is the band's contribution.  P == 0 or num_rendered == 0: zeros over the band / zero rows, and the state buffers are
 * not read (they may be NULL).  Bit-reproducible: no atomics, every sum in a fixed order; channel c of a C-channel call has the bits of a
 * 1-channel call on column c alone.
 * `scratch`: device memory of gsr_feature_grad_scratch_bytes(P, num_rendered, C) bytes, 16-byte aligned, contents undefined before and after;
 * one region reused by every channel group of a call: 68, 132 or 260 bytes per instance for C <= 4, <= 8 or more, whatever C is beyond that.  NULL settings, negative P / num_rendered, C outside the range, NULL features / out (dL_dout /
 * dL_dfeatures) with P > 0, a NULL scratch with num_rendered > 0, or NULL state buffers with P > 0 and num_rendered > 0 are
 * GSR_ERR_INVALID_ARG.
 */
#define GSR_MAX_FEATURE_CHANNELS 1024
int gsr_render_features(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                        const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                        const float* features /* [P,C] */, int C, float* out /* [C,H,W] */, void* stream);
size_t gsr_feature_grad_scratch_bytes(int P, int64_t R, int C);
int gsr_render_features_backward(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                                 const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                 const float* dL_dout /* [C,H,W] */, int C, void* scratch,
                                 float* dL_dfeatures /* [P,C] */, void* stream);
/*
 * Geometry and opacity gradients THROUGH the feature render (joint training of a field and its geometry; depth or normal supervision, where the
 * loss on a rendered z or normal column must move the Gaussians): the per-Gaussian [P,12] records of gsr_backward_blend for the loss
 * L(out), out = gsr_render_features(features).  Contributor rule as above.  Front to back over the contributors i of pixel p, with
 * T_i = prod_{j<i} (1 - alpha_j), w_i = alpha_i T_i and g_c = dL_dout[c,p]:
 *     s_i       = sum_c features[id_i,c] g_c
 *     dL/dalpha_i = T_i s_i - (sum_{j>i} w_j s_j) / (1 - alpha_i)        (no background / T_final term: `out` has none)
 *     m_i       = opacity_i G_i dL/dalpha_i                              (uncapped opacity * G, straight through the 0.99 cap, as for colour)
 * and per Gaussian, summed over the pixels of the band, (dx,dy) = mean2D - pixel, conic (A,B,C):
 *     word 0 dL/dpx = sum m (-A dx - B dy)   word 1 dL/dpy = sum m (-C dy - B dx)   (pixel units, like gsr_backward_blend)
 *     word 2 dL/dA = -1/2 sum m dx^2         word 3 dL/dB = -sum m dx dy            word 4 dL/dC = -1/2 sum m dy^2
 *     word 5 dL/dopacity = sum G dL/dalpha   words 6..11 = 0
 * i.e. words 0..5 and the layout of gsr_backward_blend's records: gsr_backward_preprocess follows unchanged and chains them to means3D /
 * scales / rotations / cov3D / opacity / means2D (its colour and SH gradients are zero).  No gradient through culling, radii, tile assignment,
 * depth order or the two cut-offs.  Rows of Gaussians without a contributing pixel are exact zeros, and their rows of `features` may hold
 * anything, NaN included: s_i is taken under the pair's predicate.  With a band of tile rows the records are the band's contribution.
 * P == 0 or num_rendered == 0: zero rows (P == 0: *splat_grads_out = NULL), and the state buffers are not read.  Fp32, no atomics, every sum
 * in a fixed order: two runs give the same bits.  The states of the record entry points are not supported.
 * `bwd_scratch`: gsr_backward_scratch_bytes(P, num_rendered) bytes, 16-byte aligned; *splat_grads_out points into it.  Argument checks as
 * gsr_render_features_backward; NULL features / dL_dout / bwd_scratch with P > 0 and a NULL splat_grads_out are GSR_ERR_INVALID_ARG.
 */
int gsr_render_features_backward_geometry(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                                          const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                                          const float* features /* [P,C] */, const float* dL_dout /* [C,H,W] */, int C,
                                          void* bwd_scratch /* gsr_backward_scratch_bytes(P, num_rendered) */,
                                          float** splat_grads_out, void* stream);

/*
 * Distortion loss on a rendered frame (no reference counterpart): the Mip-NeRF 360 regulariser that 2DGS / GOF / RaDe-GS train with,
 *     D(p) = sum_i sum_j w_i w_j |t_i - t_j|
 * which is quadratic in the blend weights and so beyond gsr_render_features.  Read from the state of gsr_pixel_probe / gsr_render_features
 * (a forward run with no_backward == 0, the same settings, the same buffers, num_rendered as returned); the states of the record entry points
 * (from_splats / from_packed / from_segments) are not supported.  Contributor rule, theirs: the entry is valid (power <= 0, alpha >= 1/255,
 * alpha capped at 0.99) and its list position is <= n_contrib[p]; n_contrib is the authority on termination; w_i = alpha_i T_i.
 * t_i is the Gaussian's view-space depth z (depth_mode 0) or 1/z (depth_mode 1, the bounded choice for unbounded scenes): the two values of
 * the splat record, those of out_invdepth and gsr_pixel_probe (which also deliver the depth maps themselves).
 * THE CONTRACT is the prefix form in list order -- equal to the pairwise form because t is monotone along a depth-sorted list --: front to
 * back over the contributors of p, with A_<i = sum_{j<i} w_j and B_<i = sum_{j<i} w_j t_j,
 *     D(p) = 2 sigma sum_i w_i (t_i A_<i - B_<i)                      sigma = +1 for z, -1 for 1/z
 * D is NOT normalised (divide by the square of the alpha image for the normalised form).  A pixel with fewer than two contributors has
 * D = 0 exactly.
 * `saved` [2,H,W] (may be NULL when no backward follows) is what the backward needs of the forward: plane 0 = sum_i w_i, plane 1 =
 * sum_i w_i (t_i - c), with c the t of LIST POSITION 0 OF THE PIXEL'S TILE (the first entry of the tile's range, whether or not it
 * contributes to p).  D and its derivatives are invariant under t -> t - c, and both kernels form every product of a t with a sum of weights
 * on t - c: t A - B would subtract two numbers of the size of the scene depth to get one of the size of a depth difference.
 * gsr_distortion_backward: the per-Gaussian [P,12] records of gsr_backward_blend for a loss L(D), g = dL_ddistortion[p], with the suffix
 * sums A_>i, B_>i:
 *     u_i = dD/dw_i = 2 sigma [t_i (A_<i - A_>i) - B_<i + B_>i]        v_i = dD/dt_i = 2 sigma w_i (A_<i - A_>i)
 *     s_i = g u_i
 *     dL/dalpha_i = T_i s_i - (sum_{j>i} w_j s_j) / (1 - alpha_i)       (gsr_render_features_backward_geometry's line, with this s)
 *     m_i = opacity_i G_i dL/dalpha_i
 * words 0..5 exactly as gsr_render_features_backward_geometry defines them from m (px, py, A, B, C, opacity), and
 *     word 9 = dL/d(1/z_g) = sum_p g v_ip (depth_mode 1),  = -z_g^2 sum_p g v_ip (depth_mode 0);       words 6, 7, 8, 10, 11 = 0
 * so that gsr_backward_preprocess follows unchanged: its inverse-depth term (dL/dz += -word9 / z^2) delivers the depth path to means3D.
 * No gradient through culling, radii, tile assignment, depth order or the two cut-offs; the 0.99 cap is passed straight through; the camera
 * is a constant; no gradient with respect to `saved`.  With a band of tile rows (tile_y0 / tile_y1) the maps are written inside the band
 * only (every pixel of the band inside the image, zeros included), dL_ddistortion / saved are read inside the band only and the records are
 * the band's contribution.  P == 0 or num_rendered == 0: zeros over the band / zero rows (P == 0: *splat_grads_out = NULL), and the state
 * buffers, dL_ddistortion and saved are not read.  Fp32, no atomics, every sum in a fixed order: two runs give the same bits.
 * `bwd_scratch`: gsr_backward_scratch_bytes(P, num_rendered) bytes, 16-byte aligned; *splat_grads_out points into it.  A NULL `out` or
 * `distortion`, a depth_mode outside {0, 1}, negative P / num_rendered, NULL state buffers / dL_ddistortion / saved with P > 0 and
 * num_rendered > 0, a NULL bwd_scratch with P > 0 and a NULL splat_grads_out are GSR_ERR_INVALID_ARG.
 */
typedef struct GsrDistortionOut {
    float*  distortion;     /* [H,W] */
    float*  saved;          /* [2,H,W] or NULL: (sum w, sum w (t - c)), for gsr_distortion_backward */
    int32_t depth_mode;     /* 0: t = z, 1: t = 1/z */
    int32_t reserved;
} GsrDistortionOut;
int gsr_distortion(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                   const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                   const GsrDistortionOut* out, void* stream);
int gsr_distortion_backward(const GsrRasterSettings* settings, int P, int32_t num_rendered,
                            const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                            const float* dL_ddistortion /* [H,W] */, const float* saved /* [2,H,W], the forward's */, int depth_mode,
                            void* bwd_scratch /* gsr_backward_scratch_bytes(P, num_rendered) */,
                            float** splat_grads_out, void* stream);

/*
 * Two-axis sharding (no reference counterpart): the per-Gaussian stages are sharded over the GAUSSIAN
 * axis (every rank owns P/G Gaussians, their parameters and optimizer state), binning + blending over the PIXEL axis
 * (bands of tile rows).  Forward: gsr_preprocess_forward on the own shard -> all-gather of the 64-byte splat records ->
 * gsr_rasterize_from_splats on the own band.  Backward: gsr_backward_blend on the own band (records of ALL Gaussians)
 * -> reduce-scatter (sum) of the 48-byte gradient records -> gsr_backward_preprocess on the own shard (geom_buffer may
 * be NULL there).  No parameter or parameter-gradient ever crosses ranks.
 *
 * gsr_preprocess_forward: projects the P Gaussians of the shard; writes radii[P] and splat_records[P,16] floats
 *   (x,y,conA,conB | conC,opacity,r,g | b,depth,tau,1/depth | rect.x,rect.y,0,tiles as bits) with the FULL-frame tile
 *   rectangle (tile_y0/tile_y1 of the settings are ignored).  geom_scratch: gsr_geometry_bytes(P) bytes.
 * gsr_rasterize_from_splats: bins and blends P gathered records inside the band the settings name; the records are
 *   copied into the geometry buffer (obtained through the callback), so the caller's array is not modified.  Buffers
 *   and outputs as gsr_rasterize_forward; a record whose tile count is 0 (culled, or a zero padding row) is ignored.
 */
int gsr_preprocess_forward(const GsrRasterSettings* settings, int P, int M,
                           const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, const float* rotations,
                           const float* cov3D_precomp, void* geom_scratch, int32_t* radii, float* splat_records,
                           void* stream);
int gsr_rasterize_from_splats(const GsrRasterSettings* settings, int P, const float* splat_records,
                              GsrResizeFn geom_resize, void* geom_user,
                              GsrResizeFn binning_resize, void* binning_user,
                              GsrResizeFn image_resize, void* image_user,
                              float* out_color, float* out_invdepth, int32_t* num_rendered, void* stream);

/*
 * Gaussian-sharded rendering (round 3; SURVEY.md 8(e), no reference counterpart): like the two-axis form, but the projected
 * splats are sent only where they are needed.  Rank g projects its P/G Gaussians (gsr_preprocess_forward), finds for every
 * band of tile rows [band_bounds[b], band_bounds[b+1]) the records whose tile rectangle touches it (gsr_route_count ->
 * band_counts, which the ranks exchange to size the buffers), packs them STABLY per band as 48-byte records
 * (x, y, conA, conB | conC, opacity, r, g | b, depth, rect.x bits, rect.y bits) together with their shard-local indices
 * (gsr_route_pack), and a variable-size all-to-all delivers segment b to rank b.  The receiver concatenates the segments in
 * rank order (= global Gaussian order when shards are contiguous index ranges, so depth ties resolve as on one GPU) and
 * calls gsr_rasterize_from_packed on its band: depth sort, scan, emission and tile sort then run on the band's Gaussians
 * only.  Backward: gsr_backward_blend on the received set -> reverse all-to-all of the [n,12] gradient rows ->
 * gsr_route_return adds the returned rows into splat_grads[P,12] of the shard (band order, no atomics, deterministic) ->
 * gsr_backward_preprocess.
 *   band_bounds : HOST array of n_bands + 1 tile-row indices (n_bands <= 64);  band_counts : DEVICE uint32[n_bands]
 *   band_offsets: HOST array of n_bands + 1 row offsets into packed / send_ids (exclusive scan of the counts)
 *   scratch     : gsr_route_scratch_bytes(P, n_bands) bytes, filled by gsr_route_count and read by gsr_route_pack
 */
size_t gsr_route_scratch_bytes(int P, int n_bands);
int gsr_route_count(int P, const float* splat_records, int n_bands, const int32_t* band_bounds, void* scratch,
                    uint32_t* band_counts, void* stream);
int gsr_route_pack(int P, const float* splat_records, int n_bands, const int32_t* band_bounds, const int64_t* band_offsets,
                   const void* scratch, float* packed, int32_t* send_ids, void* stream);
int gsr_rasterize_from_packed(const GsrRasterSettings* settings, int P, const float* packed_records,
                              GsrResizeFn geom_resize, void* geom_user,
                              GsrResizeFn binning_resize, void* binning_user,
                              GsrResizeFn image_resize, void* image_user,
                              float* out_color, float* out_invdepth, int32_t* num_rendered, void* stream);
int gsr_route_return(int P, int n_bands, const int64_t* band_offsets, const int32_t* send_ids, const float* returned,
                     float* splat_grads, void* stream);

/*
 * FIXED-CAPACITY form of the same exchange (round 4): no count matrix travels to the host before the records do.
 * gsr_route_pack_fixed lays the records of band b into a segment of capacity + 1 rows of `packed` (and of `send_ids`):
 *   row b*(capacity+1)            header: word 0 = band_counts[b] (may exceed capacity), word 1 = capacity, rest 0; send id -1
 *   rows .. + 1 .. + capacity     the first min(band_counts[b], capacity) records of the band, stable; unused rows: send id -1
 * Segment sizes do not depend on the counts, so the all-to-all has equal splits.  The receiver passes the n_segments segments it
 * got (rank order) to gsr_rasterize_from_segments: header rows and rows past a segment's count enter the frame as Gaussians
 * without tiles (P = n_segments * (capacity + 1) for gsr_backward_blend / gsr_backward_scratch_bytes), so depth ties still resolve
 * in (source rank, index) order.  The gradient rows go back in the same layout; gsr_route_return with band_offsets[b] =
 * b*(capacity+1) skips the rows whose send id is negative.  A segment whose count exceeds the capacity has lost records: the
 * caller compares band_counts with the capacity ON THE DEVICE, agrees on the outcome with the other ranks and repeats the frame
 * with the exact form (parallel.py does this without an extra host synchronisation).
 *   band_counts : DEVICE uint32[n_bands] as written by gsr_route_count;  scratch as for gsr_route_pack
 */
int gsr_route_pack_fixed(int P, const float* splat_records, int n_bands, const int32_t* band_bounds, int capacity,
                         const void* scratch, const uint32_t* band_counts, float* packed, int32_t* send_ids, void* stream);
int gsr_rasterize_from_segments(const GsrRasterSettings* settings, int n_segments, int capacity, const float* segments,
                                GsrResizeFn geom_resize, void* geom_user,
                                GsrResizeFn binning_resize, void* binning_user,
                                GsrResizeFn image_resize, void* image_user,
                                float* out_color, float* out_invdepth, int32_t* num_rendered, void* stream);

/*
 * OPT-IN fusion of the optimizer into the backward (no reference counterpart): gsr_backward_preprocess for the split-SH form
 * (settings->sh_dc = coefficient 0 [P,1,3], shs_rest = coefficients 1..15 [P,15,3], M = 16) that does NOT write the two SH
 * gradients but applies their Adam step in place, from the gradient tile in LDS: the gradient (204 B per Gaussian) never travels
 * to HBM and back.  settings->sh_dc and shs_rest are read (colour clamp) and then UPDATED; the moments likewise.
 *   sparse = 0: torch.optim.Adam on every row (rows without gradient take the g = 0 step), bias correction with step_dc / step_rest
 *   sparse = 1: SparseGaussianAdam on the rows with radii > 0, no bias correction
 * Every parameter comes out bit-identical to gsr_backward_preprocess followed by gsr_adam_step / gsr_sparse_adam_step on the two
 * tensors.  The caller owns the consequences: the step happens inside backward, once per call (no gradient accumulation).
 * All six SH arrays must be 16-byte aligned; colors_precomp is not supported in this form.
 */
typedef struct GsrShAdam {
    float* dc_exp_avg;
    float* dc_exp_avg_sq;
    float* rest_exp_avg;
    float* rest_exp_avg_sq;
    double lr_dc, lr_rest, beta1, beta2, eps;
    int32_t step_dc, step_rest;      /* 1-based, after incrementing; ignored when sparse */
    int32_t sparse;
    int32_t reserved;
} GsrShAdam;
int gsr_backward_preprocess_sh_adam(const GsrRasterSettings* settings, int P, int M, const float* means3D, float* shs_rest,
                                    const float* opacities, const float* scales, const float* rotations,
                                    const float* cov3D_precomp, const int32_t* radii, const void* geom_buffer,
                                    const float* splat_grads, float* dL_dmeans2D, float* dL_dopacity, float* dL_dmeans3D,
                                    float* dL_dcov3D, float* dL_dscales, float* dL_drotations, const GsrShAdam* adam,
                                    void* stream);

/*
 * Fused dense Adam step on one fp32 tensor of n elements (the optimizer step of train.py:177-186).
 * Same arithmetic as torch.optim.Adam(betas, eps) without weight decay / amsgrad; `step` is the 1-based step count
 * AFTER incrementing; state tensors exp_avg / exp_avg_sq are updated in place.
 */
int gsr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  double lr, double beta1, double beta2, double eps, int32_t step, void* stream);
/*
 * The same step for several tensors (a 3DGS model: positions, SH, opacities, scales, rotations -- one param group each,
 * scene/gaussian_model.py:178-211) in as few launches as possible: up to GSR_ADAM_MAX_TENSORS tensors share one kernel launch,
 * longer lists are split.  Results are bit-identical to gsr_adam_step on every tensor.
 */
#define GSR_ADAM_MAX_TENSORS 8
typedef struct GsrAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    double lr, beta1, beta2, eps;
    int32_t step;            /* 1-based, after incrementing */
    int32_t reserved;
} GsrAdamTensor;
int gsr_adam_step_multi(const GsrAdamTensor* tensors, int32_t count, void* stream);

/*
 * Sparse Adam step: replaces `_C.adamUpdate` behind `SparseGaussianAdam.step(visibility, N)` of the
 * reference's accelerated rasterizer (imported at train.py:37-41 and scene/gaussian_model.py:24-27, stepped at
 * train.py:180-183).  The tensor is N rows of M elements; rows with visible[row] == 0 are skipped entirely (parameter and
 * both moments untouched).  [RECALLED -- the source is an un-vendored submodule] no bias correction:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr m / (sqrt(v) + eps).   visible is uint8 / bool [N].
 */
int gsr_sparse_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* visible,
                         int64_t N, int64_t M, double lr, double beta1, double beta2, double eps, void* stream);
/* The same step for all parameter groups of one `SparseGaussianAdam.step(visibility, N)` call (the six tensors of
 * scene/gaussian_model.py:183-190, one group each) in ONE launch: tensor i is N rows of tensors[i].M elements with its own lr / eps;
 * visibility, N and the betas are shared.  Up to GSR_ADAM_MAX_TENSORS tensors per launch, longer lists are split.  Bit-identical to
 * gsr_sparse_adam_step on every tensor.  (Added in round 5; additive, the ABI version stays 4.) */
typedef struct GsrSparseAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t M;               /* elements per row (Gaussian) */
    double lr, eps;
} GsrSparseAdamTensor;
int gsr_sparse_adam_step_multi(const GsrSparseAdamTensor* tensors, int32_t count, const uint8_t* visible, int64_t N, double beta1,
                               double beta2, void* stream);

/*
 * Per-iteration statistics of adaptive density control: GaussianModel.add_densification_stats
 * (scene/gaussian_model.py:471-473, called at train.py:167) and the max_radii2D update of train.py:166, as ONE pass instead of
 * boolean-mask torch ops (three host synchronisations per training iteration):
 *   for visible i:  grad_accum[i] += sqrt(g[i,0]^2 + g[i,1]^2);  denom[i] += 1;  max_radii2D[i] = max(max_radii2D[i], radii[i])
 * viewspace_grad[P,3] = the operator's dL/dmeans2D; visible uint8/bool [P] or NULL (= radii > 0, what
 * gaussian_renderer/__init__.py:123 passes); radii int32 [P] or NULL (then max_radii2D is not touched).
 */
int gsr_density_stats(int P, const float* viewspace_grad, const uint8_t* visible, const int32_t* radii, float* grad_accum,
                      float* denom, float* max_radii2D, void* stream);

/*
 * 3DGS-MCMC density control (Kheradmand et al. 2024; gsplat's MCMCStrategy): the two native pieces.  gsr_scene/mcmc.py holds the
 * sampling and the optimizer bookkeeping around them.  (Additive, the ABI version stays 4.)
 *
 * Noise on the means, once per training iteration after the optimizer step, in place, one streaming pass:
 *   s = activated ? scales[i] : exp(scales[i]);   o = activated ? opacities[i] : sigmoid(opacities[i]);   q = rotations[i] / |rotations[i]|
 *   g = 1 / (1 + exp(-gate_k ((1 - o) - gate_x0)))                         (upstream: gate_k 100, gate_x0 0.995; evaluated in fp64)
 *   d = R(q) diag(s^2) R(q)^T noise[i] * g * noise_scale;                  xyz[i] += d
 * xyz, scales, noise are [P,3]; rotations [P,4] (w, x, y, z; the rasterizer's convention); opacities [P]; noise is standard-normal and comes
 * from the caller (no generator in the library); noise_scale is upstream's noise_lr * xyz_lr.  A row whose d is not finite in all three
 * components -- a NaN / inf scale, a zero quaternion, a NaN opacity, a non-finite noise value -- keeps its xyz bit for bit.  Pointers that are
 * all 16-byte aligned take 16-byte accesses (four Gaussians per lane); any other alignment is accepted and computes the same values.
 */
int gsr_mcmc_inject_noise(int P, float* xyz, const float* scales, const float* rotations, const float* opacities, const float* noise,
                          int activated, float noise_scale, float gate_k, float gate_x0, void* stream);
/*
 * Opacity and scale of a Gaussian that is replaced by N = clamp(ratios[i], 1, 51) copies of itself so that the rendered image is unchanged
 * (upstream's `compute_relocation`), on ACTIVATED opacities [n] and scales [n,3], evaluated in fp64 and rounded once:
 *   new_opacities[i] = 1 - (1 - o)^(1/N)  (as -expm1(log1p(-o) / N));
 *   new_scales[i]    = scales[i] o / D,   D = sum_{k=0}^{N-1} (-1)^k C(N, k+1) new_o^(k+1) / sqrt(k+1)
 * (upstream's double sum over a binomial table, collapsed by the hockey-stick identity).  o == 0: opacity 0, scale unchanged.  o outside
 * [0, 1) or not finite: both outputs are the inputs.  Clamping to a minimum opacity and the inverse activations are the caller's.
 */
int gsr_mcmc_relocation(int n, const float* opacities, const float* scales, const int32_t* ratios, float* new_opacities, float* new_scales,
                        void* stream);

/*
 * Bilateral-grid appearance model ("Bilateral Guided Radiance Field Processing"; gsplat's lib_bilagrid / fused_bilagrid): per-image colour
 * compensation by a low-resolution grid of 3x4 affine maps, sliced at (pixel position, pixel luminance).  (Additive, the ABI version stays 4.)
 *
 * A grid is A[12, L, Gh, Gw] fp32: channel 4 i + j is entry (i, j) of the map, i the output colour, j indexing (r, g, b, 1).  Images are planar
 * [3, H, W] fp32; values outside [0, 1] are expected.  For pixel (x, y) with colour (r, g, b):
 *   fx = (x + 0.5) / W (Gw - 1);   fy = (y + 0.5) / H (Gh - 1);   fz = (0.299 r + 0.587 g + 0.114 b) (L - 1), clamped to [0, L - 1]
 *   cell i0 = min(floor(f), n - 2), fraction t = f - i0 per axis;  A(p) = the trilinear blend of the 8 corners
 *   out_i = sum_{j<3} A_ij(p) rgb_j + A_i3(p)
 * (torch's grid_sample with align_corners=True and border padding).  Gradients go to the grid and to the image; the image gradient is the direct
 * term sum_i dL/dout_i A_ij plus the guidance term w_j (L - 1) sum_i dL/dout_i sum_j' dA_ij'/dfz [rgb, 1]_j', w = (0.299, 0.587, 0.114), where
 * dA/dfz is the slope of cell i0 when the UNCLAMPED fz lies in [0, L - 1] (at fz == L - 1 exactly: the slope of the last cell) and 0 outside.
 * Sizes: 2 <= L, Gh, Gw <= 64; H, W >= 1 (an image may be smaller than the grid).  Anything else is refused before any launch.
 *
 * Non-finite pixels: indices are taken from the clamped guidance value and a NaN guidance lands in cell 0, so nothing outside the buffers is
 * read or written.  That pixel's outputs and image gradient may be non-finite, and so may the grid gradient of the vertices it touches; every
 * other pixel's output and image gradient keeps its value bit for bit.
 *
 * The backward uses no floating-point atomics: per-workgroup partial sums in `scratch` (gsr_bilagrid_scratch_bytes bytes, 4-byte aligned; a
 * smaller scratch_bytes is refused) are added in a fixed order, so two runs give the same bits.  dL_dimage may be NULL; dL_dgrid is the same
 * bits either way, and every element of it is written.
 */
size_t gsr_bilagrid_scratch_bytes(int H, int W, int L, int Gh, int Gw);      /* 0: unsupported sizes */
int gsr_bilagrid_slice(int H, int W, int L, int Gh, int Gw, const float* grid, const float* image, float* out, void* stream);
int gsr_bilagrid_slice_backward(int H, int W, int L, int Gh, int Gw, const float* grid, const float* image, const float* dL_dout,
                                float* dL_dgrid, float* dL_dimage, void* scratch, size_t scratch_bytes, void* stream);
/*
 * Total variation of a set of grids X[N, 12, L, Gh, Gw]:
 *   tv = (1 / N) sum_{axis in L, Gh, Gw} sum (X[.. k + 1 ..] - X[.. k ..])^2 / count_axis,   count_axis = 12 (n_axis - 1) (the other two sizes)
 * evaluated in fp64 and rounded once.  The forward writes one fp64 partial sum per workgroup into `partials` (gsr_bilagrid_tv_partial_count
 * doubles, 8-byte aligned) and their sum, added in index order, into tv_out[1]; the backward takes dL/dtv as ONE device scalar.
 */
int64_t gsr_bilagrid_tv_partial_count(int N, int L, int Gh, int Gw);          /* 0: unsupported sizes */
int gsr_bilagrid_tv(int N, int L, int Gh, int Gw, const float* grids, double* partials, float* tv_out, void* stream);
int gsr_bilagrid_tv_backward(int N, int L, int Gh, int Gw, const float* grids, const float* dL_dtv, float* dL_dgrids, void* stream);

/*
 * Normal-consistency regulariser (2DGS, GOF, RaDe-GS, PGSR): per-Gaussian normals, the normals of a depth map, and the fused loss
 *   loss = (1 / (H W)) sum_p [1 - w(p) <normals(p), Nd(p)>].                                  (Additive, the ABI version stays 4.)
 *
 * Per-Gaussian normals, camera space, normals_out[P,3].  For row g: s = scales[g] (activated), q = rotations[g] (w first) AS GIVEN -- R(q) is
 * the matrix the rasterizer builds from q and is not normalised; k = the index of the smallest s (lowest index on exact ties); a = column k of
 * R(q); v_i = vm[i] a0 + vm[4 + i] a1 + vm[8 + i] a2 (the rotation part of `viewmatrix`, the flat 16 floats of the rasterizer's settings, a
 * device pointer); n = v / |v|; with p the view-space mean of means3D[g], n = -n when <n, p> > 0 (normals face the camera).  The backward
 * writes dL_drotations[P,4] through a(q) and the normalisation; k and the sign are constants, recomputed from the inputs (no saved state); no
 * gradient goes to scales, means3D or the camera.  A row with a non-finite input, or with |v| zero or non-finite, gets n = 0 and a zero
 * gradient row.  P == 0 is a no-op.
 *
 * NUMERICS CONTRACT of the depth normals.  depth is [H,W] fp32 (the z of the camera-space point seen by the pixel), normals are planar [3,H,W].
 * Pixel (x, y) has nx = (2 x + 1) / W - 1, ny = (2 y + 1) / H - 1 and the point p = (nx tanfovx z, ny tanfovy z, z): the rasterizer's pixel
 * centres (pix = ((ndc + 1) W - 1) / 2, centred principal point).  For an interior pixel (1 <= x <= W - 2, 1 <= y <= H - 2), with
 *   dz = z(x+1, y) - z(x-1, y),  sz = their sum;   dz' = z(x, y+1) - z(x, y-1),  sz' = their sum:
 *   du = (tanfovx (nx dz + (2 / W) sz),  ny tanfovy dz,  dz)          (= p(x+1, y) - p(x-1, y))
 *   dv = (nx tanfovx dz',  tanfovy (ny dz' + (2 / H) sz'),  dz')      (= p(x, y+1) - p(x, y-1))
 *   c = dv x du,   Nd = c / |c|.
 * A fronto-parallel plane gives (0, 0, -1): normals face the camera (2DGS's orientation, in camera space).  The depth differences are formed
 * BEFORE any multiplication by the ray -- differencing back-projected points cancels in fp32 with an error that grows with the resolution;
 * this form stays at a few 1e-7 at every size.  (The kernels evaluate c in the algebraically identical closed form in which the products
 * dz dz' of the two tangents, which cancel identically, are never formed.)
 * Nd = 0 at border pixels, where any of the five stencil depths (centre included) is not a finite positive number, and where |c| is zero or
 * not finite.  A poisoned depth pixel therefore changes Nd at itself and its four neighbours only, and dL/ddepth within Manhattan distance 2
 * only; every other output keeps its bits.  The gradient of the normalisation is (g - N <N, g>) / |c|; validity and the border carry none.
 * H or W below 3 is valid: every pixel is border, the map is zero and the loss is exactly 1.  tanfovx, tanfovy must be positive and finite.
 *
 * The loss: `weight` [H,W] is optional (NULL: 1) and a constant (2DGS passes the detached alpha).  Nd is never written to memory.  A pixel with
 * Nd = 0 or weight 0 contributes exactly 1 and exact zero gradients whatever `normals` holds there, NaN included.  The forward writes one fp64
 * partial sum per workgroup into `partials` (gsr_normal_loss_partial_count doubles, 8-byte aligned) and their sum, added in index order and
 * divided by H W, into loss_out[1].  The backward takes dL/dloss as ONE device scalar and writes dL_dnormals [3,H,W] and / or dL_ddepth [H,W]
 * (either may be NULL; each has the same bits whether or not the other is asked for).  No floating-point atomics anywhere: two runs give the
 * same bits.
 */
int gsr_gaussian_normals(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix, float* normals_out,
                         void* stream);
int gsr_gaussian_normals_backward(int P, const float* scales, const float* rotations, const float* means3D, const float* viewmatrix,
                                  const float* dL_dnormals, float* dL_drotations, void* stream);
int gsr_depth_normals(int H, int W, float tanfovx, float tanfovy, const float* depth, float* normals_out, void* stream);
int gsr_depth_normals_backward(int H, int W, float tanfovx, float tanfovy, const float* depth, const float* dL_dnormals, float* dL_ddepth,
                               void* stream);
int64_t gsr_normal_loss_partial_count(int H, int W);                          /* 0: unsupported sizes */
int gsr_normal_loss(int H, int W, float tanfovx, float tanfovy, const float* depth, const float* normals, const float* weight_or_null,
                    double* partials, float* loss_out, void* stream);
int gsr_normal_loss_backward(int H, int W, float tanfovx, float tanfovy, const float* depth, const float* normals, const float* weight_or_null,
                             const float* dL_dloss, float* dL_dnormals_or_null, float* dL_ddepth_or_null, void* stream);

/*
 * 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024; trained with by Gaussian Opacity Fields and RaDe-GS as well): every Gaussian is
 * low-passed in world space to the finest sampling rate any training camera sees it at.  The 2D half of the paper is `antialiasing` of the
 * rasterizer's settings.  gsr_scene/mip.py is the package side.  (Additive, the ABI version stays 4.)
 *
 * The camera sweep, upstream's `compute_3D_filter` in one call without a host synchronisation.  means3D is [P,3]; a camera record is 16 floats
 * (64 bytes), cameras is [C,16]:
 *   [0..8] R, row-major, and [9..11] T such that cam = xyz R + T (upstream's camera.R, camera.T: cam_j = sum_i xyz_i R[3 i + j] + T[j]);
 *   [12] focal_x, [13] focal_y, [14] image width W, [15] image height H (as floats).
 * For each Gaussian, distance = 100000; for each camera with z = cam.z: the camera SEES the Gaussian when z > 0.2 and
 *   -0.15 W <= cam.x / z focal_x + W / 2 <= 1.15 W,   -0.15 H <= cam.y / z focal_y + H / 2 <= 1.15 H,
 * and then distance = min(distance, z).  After all cameras a Gaussian that no camera saw takes the largest distance over those that were
 * seen, and filter_3D[i] = distance / max_c focal_x * sqrt(0.2), the maximum over ALL cameras, those that see nothing included.  seen (uint8
 * [P], upstream's valid_points) is optional: NULL costs nothing and changes no bit of filter_3D.
 * The screen test is evaluated as |cam.x focal_x| <= 0.65 W z (the same set for z > 0): a decision within rounding of a threshold may differ
 * from upstream's division.  Two departures from upstream: (1) when no Gaussian is seen at all, every distance stays 100000 (upstream raises on
 * the empty max); (2) a mean with a NaN / inf component fails every comparison: it is unseen and takes the fill value, and no other Gaussian's
 * value changes by a bit (upstream: an inf depth that passes the tests becomes everybody's fill value).  Two runs give the same bits: the
 * maximum is an integer maximum on the bits of positive floats.  scratch: gsr_mip_filter_scratch_bytes(P) bytes, 4-byte aligned, caller-owned;
 * its contents need not be initialised.  P == 0 succeeds without a launch; C < 1 is refused.
 *
 * The activations that the filter changes, one streaming pass each way; raw_scales [P,3] (log), raw_opacity [P] (logit), filter_3D [P]:
 *   s_i = exp(raw_scales[i]);   scales_out[i] = s'_i = sqrt(s_i^2 + f^2);   opacity_out = sigmoid(raw_opacity) c_0 c_1 c_2,   c_i = s_i / s'_i
 * NUMERICS CONTRACT.  The opacity factor is the product of the three per-axis ratios.  Upstream's sqrt(prod s_i^2 / prod (s_i^2 + f^2)) forms
 * products of six scales, which leave fp32's normal range for scales near 1e-7 (0/0 where both underflow); here nothing smaller than s_i^2 is
 * ever formed, so every scale down to 1e-18 is handled at full relative accuracy.
 * The backward takes dL/dscales' [P,3] and / or dL/dopacity' [P] (either may be NULL: a zero gradient, evaluated through the same arithmetic,
 * so the results are the bits of a call that passes zeros) and writes both dL_draw_scales [P,3] and dL_draw_opacity [P]:
 *   dL/dr_i = g_i s_i c_i + g_o o' (f / s'_i)^2;      dL/dr_o = g_o c_0 c_1 c_2 sigma (1 - sigma).        filter_3D is a constant (a buffer upstream).
 * Non-finite rows (they never spread): a row's outputs are what the arithmetic gives for its own inputs -- NaN for a NaN,
 * inf / NaN for a scale that overflows, the limits for the saturating infinities -- and no other row changes by a bit.  The gradient row (all
 * four values) is zero whenever a raw value or f of the row is not finite, or one of its four outputs is not.
 * Pointers that are all 16-byte aligned take 16-byte accesses (four Gaussians per lane); any other alignment computes the same bits.
 */
size_t gsr_mip_filter_scratch_bytes(int P);                                  /* 0: P < 0 */
int gsr_mip_filter_3d(int P, const float* means3D, int C, const float* cameras, float* filter_3D, uint8_t* seen_or_null, void* scratch,
                      void* stream);
int gsr_mip_activations(int P, const float* raw_scales, const float* raw_opacity, const float* filter_3D, float* scales_out, float* opacity_out,
                        void* stream);
int gsr_mip_activations_backward(int P, const float* raw_scales, const float* raw_opacity, const float* filter_3D,
                                 const float* dL_dscales_or_null, const float* dL_dopacity_or_null, float* dL_draw_scales,
                                 float* dL_draw_opacity, void* stream);

/*
 * Vector quantisation of per-Gaussian parameters: the two steps of a Lloyd (k-means) iteration over rows [P,D] and a codebook [K,D], what
 * "Compressed 3D Gaussian Splatting" (Niedermayr et al., CVPR 2024), Compact3D, LightGaussian and gsplat's PngCompression run over the SH
 * coefficients, scales and rotations of a trained scene.  gsr_scene/compress.py is the package side.  (Additive, the ABI version stays 4.)
 * Limits: 0 <= P, 1 <= D <= 64, 1 <= K <= 65536; anything else is GSR_ERR_INVALID_ARG (gsr_vq_scratch_bytes: 0).  scratch:
 * gsr_vq_scratch_bytes(P, D, K) bytes, 16-byte aligned, caller-owned, shared by both calls; its contents need not be initialised.
 *
 * gsr_vq_assign: idx[p] = argmin_k |x_p - c_k|^2, evaluated as argmin_k (|c_k|^2 - 2 x_p . c_k) in fp32 on the matrix pipe, never writing a
 * P x K block.  NUMERICS CONTRACT.  The score of (p, k) is the chain s = |c_k|^2; s = fmaf(-2 x_pi, c_ki, s) for ascending i, with
 * |c_k|^2 = fmaf(c_ki, c_ki, .) ascending from 0: the chosen centroid is within (D + 4) 2^-23 (|x|^2 + |c_got|^2 + |c_best|^2) of the best
 * squared distance.  The form cancels when |x| is large against the distances: centre the rows first (the argmin is translation-invariant;
 * gsr_scene.compress.kmeans does).  An exact fp32 tie of scores goes to the LOWEST index.  dist2[p] is recomputed for the winner directly,
 * d = 0; d = fmaf(x_i - c_i, x_i - c_i, d) ascending -- not from the score.  Containment: a row with a NaN / inf component
 * gets idx -1 and dist2 0 and changes no other row; a centroid with a NaN / inf component (or whose norm overflows) never wins; when no
 * centroid is finite (or every score of a row overflows) idx is -1.  P == 0 succeeds without a launch.
 *
 * gsr_vq_update: codebook[k] = (float)(sum w_p x_p / sum w_p) and mass[k] = (float) sum w_p over the rows with idx[p] == k, the sums in fp64 in
 * a fixed order (stable sort by idx, rows of a cluster in ascending p, segments cut into chunks of 256 rows that are added in chunk order): no
 * floating-point atomics, two runs give the same bits.  idx outside [0, K) (-1 of the assignment) belongs to nobody.  A cluster whose weights
 * sum to zero KEEPS its centroid, bit for bit, and reports mass 0.  weights NULL: 1; a negative, NaN or inf weight counts as 0, and a row of
 * weight 0 adds nothing whatever it holds.  P == 0: every mass is 0.
 */
size_t gsr_vq_scratch_bytes(int P, int D, int K);                            /* 0: unsupported sizes */
int gsr_vq_assign(int P, int D, int K, const float* rows, const float* codebook, int32_t* idx, float* dist2, void* scratch, void* stream);
int gsr_vq_update(int P, int D, int K, const float* rows, const float* weights_or_null, const int32_t* idx,
                  float* codebook /* in: kept where a cluster is empty; out */, float* mass /* [K] */, void* scratch, void* stream);

/*
 * TSDF fusion of rendered depth maps and mesh extraction: the step 2DGS, Gaussian Opacity Fields, RaDe-GS and PGSR end with.
 * gsr_scene/mesh.py is the package side.  (Additive, the ABI version stays 4.)
 *
 * The volume is dense, nx x ny x nz voxels stored [nz,ny,nx] (x fastest); voxel (ix,iy,iz) sits at origin + voxel_size (ix,iy,iz).  State:
 * tsdf (fp32, the running weighted mean, in [-1,1]), weight (fp32, a count of observations) and optionally rgb [3,nz,ny,nx].  A fresh volume
 * is tsdf = 1, weight = 0, rgb = 0.  nx ny nz >= 2^31 is refused.
 *
 * gsr_tsdf_integrate folds V views into the volume in ONE kernel (the volume is read and written at most once per call).  A camera record
 * is the 16 floats of gsr_mip_filter_3d; the principal point is (W / 2, H / 2) of the call's W and H (the package checks that every record
 * carries the same two numbers).  depth [V,H,W] is view-space z; color [V,3,H,W] goes with rgb (both or neither is used).  For a voxel at
 * xyz and view v, in view order, with cam = xyz R + T and z = cam.z:
 *   skip unless z > near;   px = floor(focal_x cam.x / z + W / 2), py = floor(focal_y cam.y / z + H / 2)  (the nearest pixel centre under the
 *   rasterizer's pixel convention);   skip unless 0 <= px < W and 0 <= py < H;   d = depth[v,py,px];   skip unless d is finite and d > 0;
 *   sdf = d - z;   skip when sdf < -sdf_trunc;   otherwise s += min(1, sdf / sdf_trunc), n += 1, c += color[v,:,py,px].
 * After all views, when n > 0:  tsdf' = (tsdf weight + s) / (weight + n), rgb likewise, weight' = weight + n.  A voxel with n == 0 is not
 * written.  This is Curless-Levoy's (and Open3D's) update with weight 1 per observation, folded over the call's views.
 * NUMERICS CONTRACT.  cam is three fmaf chains, fmaf(x, R0j, fmaf(y, R1j, fmaf(z, R2j, Tj))); every product, quotient, sum and comparison
 * named above is one correctly rounded fp32 operation, the sums run in view order, and there are no atomics: two runs give the same bits.
 * Non-finite input: a NaN / inf depth pixel is an invalid pixel; a record with a non-finite entry contributes to no
 * voxel; nothing spreads.  Limits: nx, ny, nz >= 0, V >= 0, H, W >= 1 (H W < 2^31), voxel_size > 0, sdf_trunc > 0, near >= 0, all finite;
 * anything else is GSR_ERR_INVALID_ARG.  V == 0 or an empty volume succeeds without a launch.
 *
 * The mesh is INDEXED and comes from marching tetrahedra: each cell (ix..ix+1, iy..iy+1, iz..iz+1) is cut into the six Kuhn tetrahedra, for
 * the axis permutation pi (in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx) the corners v0 = (0,0,0), v1 = v0 + e_pi(1),
 * v2 = v1 + e_pi(2), v3 = (1,1,1).  Every tetrahedron edge runs from a grid point in one of seven directions, numbered (1,0,0), (0,1,0),
 * (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1), and is owned by its lower grid point: a mesh vertex IS (owner voxel, direction).
 *   A voxel is observed when weight >= min_weight and its tsdf is finite; a cell is valid when its eight corners are observed; only valid
 *   cells emit faces.  A corner is inside when tsdf < 0, outside otherwise.  A vertex exists on an edge iff its ends differ in that and at
 *   least one valid cell contains the edge; it sits at p0 + s0 / (s0 - s1) (p1 - p0), its colour interpolated with the same ratio.  A
 *   tetrahedron emits 1 face for 1 or 3 inside corners, 2 for 2.  The winding comes from the case and the tetrahedron's orientation, never
 *   from the computed geometry: face normals point to the outside (positive tsdf), zero-area faces included, which are kept.
 *   With e_pq the vertex on the edge of tetrahedron corners p and q: one inside corner a (or one outside corner a) and the others b < c < d
 *   give the face (e_ab, e_ac, e_ad) or (e_ab, e_ad, e_ac); inside corners a < b and outside corners c < d give the quad (e_ac, e_ad, e_bd, e_bc)
 *   or (e_ac, e_bc, e_bd, e_ad), emitted as (q0, q1, q2), (q0, q2, q3) -- in each case the winding that faces outside.
 *   Order: vertices by (owner voxel index, direction), faces by (cell index, tetrahedron, face).
 * gsr_mesh_count classifies, counts and scans (fixed order, integers only) and leaves {vertices, faces} in counts_out (int32 [2], device);
 * the caller reads the two numbers -- the one synchronisation -- allocates, and gsr_mesh_emit writes vertices [nv,3], colors [nv,3]
 * (with rgb; both or neither) and faces [nf,3] from the SAME scratch, volume and min_weight's classification.  Nothing is written past nv
 * vertices or nf faces.  nv == 0 succeeds without a launch, as does a volume without a cell.  scratch: gsr_mesh_scratch_bytes bytes,
 * 128-byte aligned, caller-owned; its contents need not be initialised.  Extraction is limited to nx ny nz <= 178956970 (12 faces per
 * cell fit int32); gsr_mesh_scratch_bytes returns 0 beyond.
 */
int gsr_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float sdf_trunc, float near_z, int V,
                       const float* cameras, int H, int W, const float* depth, const float* color_or_null, float* tsdf, float* weight,
                       float* rgb_or_null, void* stream);
size_t gsr_mesh_scratch_bytes(int nx, int ny, int nz);                       /* 0: unsupported sizes */
int gsr_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float min_weight, void* scratch, int32_t* counts_out,
                   void* stream);
int gsr_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf, const float* rgb_or_null,
                  void* scratch, int nv, int nf, float* vertices, float* colors_or_null, int32_t* faces, void* stream);

/*
 * Mesh clean-up on an indexed triangle mesh -- what 2DGS's post_process_mesh(cluster_to_keep) and its kin in GOF, RaDe-GS and PGSR run before a
 * mesh is saved or evaluated: connected components, removal of small clusters, vertex normals, Taubin smoothing.  gsr_scene/mesh.py is the
 * package side (components, compact, filter_components, vertex_normals, smooth).  (Additive, the ABI version stays 4.)
 *
 * THE RULE every call shares: row f of faces [nf,3] (int32) is a FACE iff its three indices are in [0, nv) and pairwise different.  Any other
 * row is not there: no kernel reads a vertex through it, it joins nothing, it counts nowhere and it survives no compaction.
 * Sizes: 0 <= nv < 2^31, 0 <= 3 nf < 2^31, anything else is GSR_ERR_INVALID_ARG; empty inputs are valid calls that write nothing
 * (gsr_mesh_compact_count writes the two zeros).  scratch: gsr_meshops_scratch_bytes(nv, nf) bytes, 128-byte aligned, caller-owned, one
 * layout for all five operations; its contents need not be initialised, and a call reads only what it (or, for the emit, the count before
 * it) wrote.  No floating-point atomics anywhere: two runs give the same bits.
 *
 * gsr_mesh_components: two vertices are connected when a face holds both (connectivity is by VERTEX: two closed surfaces that share one
 * vertex are one component, where Open3D's cluster_connected_triangles, which joins triangles across shared edges, reports two).
 * vertex_label[v] (int32 [nv]) = the smallest vertex index of v's component; a vertex no face uses is its own component.  face_count[r]
 * (int32 [nv]) = the number of faces of the component whose label is r, 0 at every v that is no label.  Rounds of hook (per face and edge,
 * an integer atomicMin of the smaller of the two ends' current labels into the slot of the larger) and compress (every vertex points at its
 * root); labels only fall and stay inside the component, so the fixpoint is the component's minimum whatever the schedule.  The host reads
 * one word per round and stops at a round that hooked nothing: THE CALL SYNCHRONISES THE STREAM.  More than 2 ceil(log2(nv + 1)) + 8 rounds
 * is GSR_ERR_UNSUPPORTED (the call never spins); gsr_mesh_components_rounds() returns the rounds of the most recent call.
 *
 * gsr_mesh_compact_count / _emit: keep_face [nf] (uint8, non-zero = keep; NULL = keep every face) selects faces; a vertex is kept iff a kept
 * face uses it.  The count leaves {nv', nf'} in counts_out (int32 [2], device); the caller reads them -- the one synchronisation --
 * allocates, and the emit writes vertices' [nv',3], colors' [nv',3] (with colors; both or neither) and faces' [nf',3] from the SAME
 * scratch, faces and keep_face.  Kept vertices and kept faces stay in their original relative order and the indices are remapped: the
 * output is faces[keep] with new index = (number of kept vertices before it), values copied bit for bit.  Nothing is written past nv_out
 * vertices or nf_out faces; nv_out == 0 succeeds without a launch.
 *
 * gsr_mesh_vertex_normals: area-weighted.  N_i = sum over the faces f that hold vertex i, in ascending f, of (b - a) x (c - a) with
 * (a, b, c) the face's own corner order; every operand is converted to fp64 first, the cross product is (uy wz - uz wy, uz wx - ux wz,
 * ux wy - uy wx) and the sum runs in fp64.  n_i = N_i / sqrt((Nx Nx + Ny Ny) + Nz Nz) in fp64, rounded once to fp32; N_i == 0 exactly, or
 * no face, gives (0,0,0).  With gsr_mesh_emit's winding the normal points to positive tsdf (outside).  Non-finite positions give whatever
 * IEEE arithmetic yields, and only at the vertices of the faces that hold them.
 *
 * gsr_mesh_smooth: Taubin smoothing, `iterations` times a step with weight lambda followed by a step with weight mu (Taubin 1995: lambda > 0,
 * mu < -lambda; 0.5 / -0.53 are the customary pair).  One step with weight w, F_i the faces that hold vertex i in ascending order:
 *   S = sum over f in F_i of (p_j + p_k), j, k the two corners after i in f's cyclic order;   m = S / (2 |F_i|);   p_i' = p_i + w (m - p_i),
 * all in fp64 on operands converted first, rounded once to fp32; a vertex with |F_i| = 0 keeps its bits.  The weight of a neighbour in m is
 * therefore the number of faces on the edge to it: 2 on closed manifold regions, where every neighbour weighs the same and the step is
 * exactly the uniform umbrella operator, and 1 across a boundary edge.  All 2 iterations launches go out in one call, ping-pong between the
 * scratch and vertices_out; the input is never written (vertices_out must be another buffer).  iterations == 0 copies.  A non-finite
 * position reaches only vertices within 2 iterations edges of it.  NaN weights and iterations < 0 are GSR_ERR_INVALID_ARG.
 * The incident-face lists of the last two calls are the corners (vertex id, 3 f + k) sorted by vertex with the stable pair sort of the
 * binning chain, so a vertex's corners come out in ascending face order.
 */
size_t gsr_meshops_scratch_bytes(int nv, int nf);            /* 0: unsupported sizes */
int gsr_mesh_components(int nv, int nf, const int32_t* faces, int32_t* vertex_label, int32_t* face_count, void* scratch,
                        void* stream);                       /* synchronises the stream */
int gsr_mesh_components_rounds(void);                        /* hook + compress rounds of the most recent gsr_mesh_components */
int gsr_mesh_compact_count(int nv, int nf, const int32_t* faces, const uint8_t* keep_face_or_null, void* scratch,
                           int32_t* counts_out /*[2]: nv', nf'*/, void* stream);
int gsr_mesh_compact_emit(int nv, int nf, const float* vertices, const float* colors_or_null, const int32_t* faces,
                          const uint8_t* keep_face_or_null, void* scratch, int nv_out, int nf_out, float* vertices_out,
                          float* colors_out_or_null, int32_t* faces_out, void* stream);
int gsr_mesh_vertex_normals(int nv, int nf, const float* vertices, const int32_t* faces, float* normals_out, void* scratch, void* stream);
int gsr_mesh_smooth(int nv, int nf, const float* vertices, const int32_t* faces, int iterations, float lambda, float mu,
                    float* vertices_out, void* scratch, void* stream);

/*
 * Replaces `simple_knn._C.distCUDA2` (un-vendored submodule submodules/simple-knn, .gitmodules:1-3; called once per
 * scene at scene/gaussian_model.py:159): mean_dist2[i] = mean of the squared Euclidean distances
 * from points[i] to its 3 nearest OTHER points (exact; coincident points count with distance 0; fewer than 4 points
 * leaves FLT_MAX terms in the mean, as in the reference).  points[N,3] fp32, scratch of gsr_knn_scratch_bytes(N) bytes.
 */
size_t gsr_knn_scratch_bytes(int N);
int gsr_knn_mean_dist2(int N, const float* points, float* mean_dist2, void* scratch, void* stream);

/*
 * Fused SSIM map: replaces the un-vendored `fused_ssim` extension (train.py:31-35,122; its
 * `fusedssim` / `fusedssim_backward`), same numerics as utils/loss_utils.py:56-87 (11x11 Gaussian window, sigma 1.5,
 * zero padding 5, C1 = 0.01^2, C2 = 0.03^2).  Images are [planes, H, W] fp32 (planes = batch x channels).
 * forward writes the SSIM map and -- when the three derivative maps are non-NULL (training) -- dm/dmu1, dm/dE[x^2],
 * dm/dE[xy]; backward turns dL/dmap into dL/dimg1.
 */
int gsr_ssim_forward(int planes, int H, int W, const float* img1, const float* img2, float* ssim_map,
                     float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream);
int gsr_ssim_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmap,
                      const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                      float* dL_dimg1, void* stream);

/*
 * Mean-SSIM form of the same kernels -- what `fused_ssim(img1, img2)` returns (train.py:122): the forward writes one
 * partial sum per wave (per tile in the LDS-tiled A/B form) into `partials` -- gsr_ssim_partial_count floats is room for
 * either form -- and their mean, added in fixed order, into mean_out[1]; the backward takes dL/dmean as ONE device scalar.  Saves the SSIM-map round trip and the framework's
 * reduction / broadcast kernels; results equal gsr_ssim_forward + mean up to fp32 summation order.
 */
int64_t gsr_ssim_partial_count(int planes, int H, int W);
int gsr_ssim_mean_forward(int planes, int H, int W, const float* img1, const float* img2, float* partials, float* mean_out,
                          float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream);
int gsr_ssim_mean_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmean,
                           const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1,
                           void* stream);

/*
 * The whole training loss of train.py:119-126 in the same two kernels (round 3, SURVEY.md 8(f) N1 "fused SSIM + L1"):
 *     loss = (1 - lambda_dssim) * mean|img1 - img2| + lambda_dssim * (1 - mean SSIM(img1, img2))
 * (utils/loss_utils.py:40-41 for the L1 term).  The forward reads both images once (the L1 sum comes from the pixels the
 * SSIM window already staged) and writes loss_out[3] = (loss, L1, SSIM) -- the two parts for the progress bar of
 * train.py:147-151; the backward takes dL/dloss as ONE device scalar and writes dL/dimg1 = -lambda dSSIM/dimg1 +
 * (1 - lambda) sign(img1 - img2) / count once.  partials: 2 * gsr_ssim_partial_count(planes, H, W) floats.
 */
int gsr_train_loss_forward(int planes, int H, int W, const float* img1, const float* img2, float lambda_dssim, float* partials,
                           float* loss_out, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream);
int gsr_train_loss_backward(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dloss,
                            float lambda_dssim, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                            float* dL_dimg1, void* stream);

/* Replaces _C.mark_visible: present[i] = 1 iff Gaussian i is in front of the 0.2 near plane. */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/*
 * Introspection for tests and bench (no reference counterpart).  Views into the buffers forward filled.
 * Pointers are device pointers valid while the buffers live.
 */
typedef struct GsrForwardViews {
    const float* splats;          /* [P,16] x,y,conA,conB | conC,opacity,r,g | b,depth,tau,1/depth | rect,goffset,tiles (bits) */
    const uint32_t* tiles_touched;/* [P] */
    const uint32_t* depth_order;  /* [P] Gaussian ids in (depth, id) order; culled ones last */
    const uint32_t* point_list;   /* [R] Gaussian ids sorted by (tile, depth, id) */
    const uint32_t* ranges;       /* [n_tiles,2] start,end */
    const float* final_T;         /* [H*W] */
    const uint32_t* n_contrib;    /* [H*W] */
    const uint32_t* tile_scan;    /* [P] inclusive scan of tiles_touched in depth order (ABI 4) */
} GsrForwardViews;
int gsr_forward_views(int P, int64_t R, int width, int height,
                      const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                      GsrForwardViews* out);

/* Per-stage GPU timing (HIP events on `stream`, recorded around each kernel group when enabled).
 * Stage ids index GSR_STAGE_*; times accumulate until reset.  Used by bench.py for roofline.achieved. */
enum {
    GSR_STAGE_PREPROCESS = 0,
    GSR_STAGE_DEPTH_SORT = 1,
    GSR_STAGE_SCAN = 2,
    GSR_STAGE_EMIT = 3,
    GSR_STAGE_TILE_SORT = 4,
    GSR_STAGE_RANGES = 5,
    GSR_STAGE_RENDER = 6,
    GSR_STAGE_RENDER_BWD = 7,
    GSR_STAGE_PREPROCESS_BWD = 8,
    GSR_STAGE_GATHER_BWD = 9,
    GSR_STAGE_COLOR = 10,            /* (unused since ABI 4: the split preprocess was removed) */
    GSR_STAGE_R_WAIT = 11,           /* GPU idle between the depth sort and the first kernel the host launches after reading R */
    GSR_STAGE_COUNT = 12
};
int gsr_profile_enable(int on);      /* bit 0: per-stage events; bit 1: work counters (slow the blend kernels: count in a separate pass);
                                      * bit 2: per-wave trace of the blend kernels instead of the counters (gsr_profile_trace) */
int gsr_profile_reset(void);
/* Resolves pending events (synchronises them) and returns accumulated ms and launch counts per stage. */
int gsr_profile_read(float* ms_out, int32_t* count_out, int n);
/* Work counters of the blend kernels, accumulated over the launches made while profiling is enabled (bench.py turns them
 * into achieved FLOP/s): [0] forward (8x8 pixel block, list entry) pairs blended by a whole wave, [1] forward batches of
 * 64 entries box-tested, [2] / [3] the same for the blend backward.  reset != 0 clears them after reading.
 * [4] / [5]: steps of the HEAVIEST wave of the forward / backward launches (max, not sum): with the wave counts this gives the
 * tail of a launch, slowest wave / mean wave, which is what clustered scenes stress. */
#define GSR_COUNTER_COUNT 6
int gsr_profile_counters(uint64_t* out, int n, int reset);
/* Per-wave trace of the two blend kernels (measurement only; gsr_profile_enable(4)): entry w of the most recent launch's wave w is four
 * 64-bit words -- start and end time (100 MHz constant clock, s_memrealtime), placement (HW_ID bits 0-31, XCC id bits 32-35,
 * kernel bits 40-41: 1 forward, 2 backward) and the wave's blend steps.  Waves that left early (nothing to blend) keep a zero entry.
 * Copies min(max_waves, GSR_TRACE_WAVES) entries to `out`, clears the device copy, returns the number copied (negative: error).
 * This is how the tail of a blend launch was measured (tools/gpu_wave_trace.py). */
#define GSR_TRACE_WAVES 65536
int gsr_profile_trace(uint64_t* out, int max_waves);

/* Switches.  The product library accepts the tuning knobs sort_small_block_threshold, sort_mid_block_threshold,
 * sort_items_large, tile_sort_mode (0 fused two-level sort, 1 legacy LSD passes) and
 *   depth_sort_mode   0 = automatic: the bucket depth sort (4 launches, csrc/depthsort.hip) up to 3 M Gaussians, the LSD radix
 *                     passes beyond and for 64 frames after a frame whose depths crowded one bucket; 1 = always LSD; 2 = always
 *                     the bucket sort (all three give bit-identical bins)
 *   level2_scan_mode  0 = automatic, 1 = the tile sort's level-2 scan as its own launch, 2 = folded into the scatter
 * The measurement build (GSR_AB=1 python build.py -> lib_ab/, sources in tools/ab_variants/) also compiles render_fwd_variant 1 / 3,
 * render_bwd_variant 1 / 4 / 5 and the round-5 options fwd_bands (level-2 sort + blend band by band on two HIP streams) and
 * render_fwd_lds_pad (resident waves of the forward blend capped through LDS) -- all measured and rejected
 * (profiles/r05_ab_fwd_bands_occupancy.json); the product accepts only the defaults.  (ABI 4 removed the options of experiments
 * whose code left the sources: onesweep depth sort, color_overlap, first_hist_in_preprocess, sh_dma.)  Unknown names /
 * unavailable values return an error.
 * Switches of the product library (every setting gives the same results; 0 is the form they replaced):
 *   snug_tiles       1 = a Gaussian is binned into the tiles its alpha >= 1/255 ellipse can reach, 0 = into the reference's square
 *                    of radius 3 sqrt(lambda_max) (same outputs, ~1.4x the instances)
 *   bwd_heavy_first  launch order of the blend backward, planned from the forward's per-block step counts: 2 (default) = tiles by
 *                    their heaviest half, 1 = tiles by the sum of their four blocks (round 3), 3 = every half tile on its own,
 *                    0 = index order; scheduling only -- the gradients are the same bits in every order
 * and ssim_variant (0 = marching-wave SSIM / training-loss kernels, 1 = the LDS-tiled form), ssim_target_waves (launch shape of
 * the marching form: the waves a launch aims for, forward and backward alike, at least 256; 0 = back to the defaults of 4096
 * forward / 2048 backward, which no single value expresses), preprocess_grid_cap.
 *   preprocess_generic  0 (default) = the forward per-Gaussian kernel runs the instantiation compiled for the call form (scales + rotations,
 *                    16-coefficient SH fused or dc / rest, band of a quarter of the frame or more: no dead paths), 1 = always the generic one
 *                    (A/B and tests; the same bits either way)
 *   preprocess_hot_grid workgroups of those instantiations: 0 (default) = one resident round, from the occupancy the runtime reports; 1..2047
 *   ranking_generic  0 (default) = the stable-ranking kernels of the binning chain (emit_scatter, bucket_scatter, ds_segsort) run the
 *                    instantiation compiled for the frame's digit width (tile-id halves of 5..8 bits, bucket digit 5..7: 640x360 up to 4K), 1 = always the
 *                    run-time-width one (A/B and tests; the same bits either way)
 *   ranking_pad_last 1 (default) = emit_scatter and bucket_scatter rank the slots that a partial block lacks as ordinary items of the highest digit,
 *                    which the stable ranking leaves behind every real item and the final store drops, 0 = every item carries a validity predicate
 *                    through the ranking (the earlier form; A/B and tests; the same bits either way)
 * Test hook: debug_last_preprocess_path = 1 (generic) / 2 (hot) changes nothing and succeeds iff the most recent forward took that instantiation.
 * Test hook: debug_last_ranking_widths = hb << 4 | lb changes nothing and succeeds iff the most recent tile sort ran emit_scatter instantiated for
 * hb bits and bucket_scatter for lb bits (0: the run-time-width kernel).
 * Test hook: debug_dirty_control_block = t preloads t tickets into the frame counter of the NEXT forward call, once (a counter that is
 * not zero when a frame begins, csrc/gsr_frame.h): that frame is wrong or refused, the ones after it must be right again. */
int gsr_set_option(const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
