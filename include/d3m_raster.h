/*
 * d3m_raster.h -- C ABI of libd3m_raster.so, the MI355X (gfx950) differentiable mesh rasterizer.
 *
 * This is the drop-in boundary for the rasterization hot path of achao2013/deep3dmap.  Plain
 * pointers and sizes only: every pointer is a DEVICE pointer unless it says "host"; `stream` is a
 * hipStream_t passed as void* (NULL = the legacy default stream, which is what the reference's
 * `<<<blocks, threads>>>` launches use, rasterize_cuda_kernel.cu:615).  No ATen / torch types.
 *
 * Conventions kept from the reference extension (pnpmodules/neural_renderer/neural_renderer/cuda/
 * rasterize_cuda.cpp, "KCPP" below; kernels in rasterize_cuda_kernel.cu, "KCU"):
 *   - the caller allocates AND pre-fills every output (face_index -1, weight 0, depth = far, rgb 0,
 *     sampling maps 0, face_inv 0, grad buffers 0: neural_renderer/rasterize.py:50-69,111-115);
 *     entry points mutate in place;
 *   - tensors are contiguous f32 / i32 in the layouts named per argument;
 *   - disabled outputs may be NULL (the reference passes 1-element dummies, rasterize.py:46,59-69);
 *   - nothing here synchronises the device; errors detected on the host are returned at once,
 *     launch failures surface as D3M_ERR_LAUNCH with hipGetLastError() kept in d3m_last_hip_error().
 *
 * Return value of every int function: 0 on success, one of the D3M_ERR_* codes otherwise.
 */
#ifndef D3M_RASTER_H
#define D3M_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* d3m_stream_t; /* hipStream_t */

enum {
    D3M_OK = 0,
    D3M_ERR_INVALID = 1,   /* bad size / NULL where data is required / unsupported value */
    D3M_ERR_WORKSPACE = 2, /* workspace missing or smaller than d3m_*_workspace_bytes() */
    D3M_ERR_LAUNCH = 3     /* a HIP call failed; see d3m_last_hip_error() */
};

/* camera_mode values of d3m_camera_* (neural_renderer/renderer.py:88-112) */
enum { D3M_CAMERA_NONE = 0, D3M_CAMERA_LOOK_AT = 1, D3M_CAMERA_LOOK = 2, D3M_CAMERA_PROJECTION = 3 };

const char* d3m_version(void);
int d3m_last_hip_error(void);         /* hipError_t of the most recent failed HIP call, 0 if none */
/* Zero-fill up to six device ranges with ONE kernel launch (host arrays of `count` device pointers / byte counts; every
 * range 4-byte aligned and a multiple of 4 bytes, NULL / 0 entries skipped).  The library never uses memset nodes (a
 * captured hipMemsetAsync was not ordered reliably against the next kernel node on ROCm 7.2); callers that clear several
 * small scratch buffers per step (the reference does the same with torch.zeros, NR/rasterize.py:111-115) save a launch
 * per buffer. */
int d3m_zero_ranges(void* const* ptrs, const size_t* bytes, int count, d3m_stream_t stream);
/* CLEARS.  An operator that needs zeroed scratch (counters, arrival tickets, accumulators) clears it itself with one fill
 * launch in front of its kernels.  A caller that runs a whole step may do all of a step's clears in ONE launch instead --
 * d3m_lit_front, the step's first kernel, takes a list of ranges beside the camera and the light -- : it asks every operator
 * for what that operator would clear (d3m_forward_clear_bytes, d3m_edge_plan_clear_bytes, d3m_render_fit_scratch_clear_range,
 * d3m_backward_textures_lit_clear_ranges), zeroes those ranges, and passes D3M_PRECLEARED in the operator's `flags`. */
#define D3M_PRECLEARED 1
const char* d3m_error_string(int code);

/* Per-kernel timing with HIP events recorded on each launch's own stream (used by bench.py for the
 * live roofline figure; off by default).  d3m_timing_collect synchronises the device, returns one row
 * per kernel name (static strings) with its launch count and summed duration, and clears the record. */
void d3m_timing_enable(int on);
int d3m_timing_collect(const char** names, int* counts, float* total_ms, int max_entries);

/* ------------------------------------------------------------------------------------------------
 * A. The five operators of `neural_renderer.cuda.rasterize` (KCPP:193-199), same argument order.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of scratch d3m_forward_face_index_map(_mesh) needs for (batch_size, num_faces, image_size):
 * per-tile face lists built on the device -- or, for the meshes and batch sizes where d3m_forward_face_index_map_mesh
 * covers by bidding instead of binning, a 64-bit z-buffer and a list of big faces: the larger of the two.
 * A smaller buffer is accepted down to d3m_forward_workspace_min_bytes(); it lowers the size above which a face is handled
 * as "large" (scanned by every tile of its view) and rules the bidding form out.  Contents need no initialisation. */
size_t d3m_forward_workspace_bytes(int batch_size, int num_faces, int image_size);
size_t d3m_forward_workspace_min_bytes(int batch_size, int num_faces, int image_size);

/* Which of the two forms of coverage d3m_forward_face_index_map(_mesh) runs (both replace KCU:70-169 and
 * produce the same maps bit for bit): -1 = chosen per launch by mesh density and batch size (the default), 0 = per-tile
 * face lists only (k_bin_* -> k_raster_tiles), 1 = bidding into a 64-bit z-buffer wherever its workspace fits
 * (k_bid_faces -> k_bid_big -> k_bid_resolve).  Process-wide, read at every launch; the environment variable D3M_BID=0/1
 * sets the initial value.  Returns D3M_ERR_INVALID for any other value. */
int d3m_set_coverage_form(int form);
int d3m_get_coverage_form(void);

/* Run-to-run reproducibility (no reference counterpart: the reference's float atomics, KCU:533-538,586-589, are unordered
 * too).  on = 1: d3m_visibility (and the list a forward launch leaves) is built in ASCENDING face order by three launches
 * -- count, scan, compact -- instead of one whose chunks land in arrival order, so that every pass over the list issues its
 * float atomics from the same workgroups, in the same list order, in every run; the gathered passes of
 * d3m_backward_textures_lit and d3m_backward_depth_map take faces of ANY size (no per-pixel atomic fallback for boxes beyond
 * 4096 pixels), so that a face's sums are its own lanes'.  Process-wide, read at every launch; the
 * environment variable D3M_DETERMINISTIC=1 sets the initial value.  Returns D3M_ERR_INVALID for values other than 0 / 1. */
int d3m_set_deterministic(int on);
int d3m_get_deterministic(void);
/* Which form of the edge plan (d3m_edge_plan, and the plan d3m_backward_pixel_map builds itself) a blob takes: 0 = by its
 * size and the batch (the one-pass form where every line's fixed slice holds at least one crossing per pixel of the line,
 * the counted form otherwise), 1 = always the counted form, 2 = the one-pass form wherever it can run at all.  Process-wide,
 * read at every launch: a plan must be built and used under the same setting.  The environment variable
 * D3M_EG_PLAN_FORM=0/1/2 sets the initial value.  Returns D3M_ERR_INVALID for any other value. */
int d3m_set_edge_plan_form(int form);
int d3m_get_edge_plan_form(void);
/* The per-vertex sums of the deterministic mode (deep3dmap_amd/neural_renderer/rasterize.py, "DETERMINISTIC"): the adjoint
 * of vertices_to_faces + fill_back (NR/vertices_to_faces.py:16-22, NR/renderer.py:86) GATHERED per vertex in a fixed order
 * instead of scattered with float atomics.  adj_offsets [V+1], adj_items [3 F]: CSR adjacency of ONE index tensor tri [F,3]
 * -- item = 3 f + c for "corner c of triangle f", the items of a vertex in ascending order.
 * d3m_vertex_gather: grad_vertices [B,V,3] (WRITTEN) = the sum over a vertex's items of grad_faces_a[b,f,c,:] +
 * grad_faces_b[b,f,c,:] (either array may be NULL; both [B,F',3,3]) and, with fill_back, of the copy's [b,F+f,2-c,:];
 * `visibility` (optional): the d3m_visibility blob of the forward result -- faces that own no pixel are skipped unread.
 * d3m_face_light_backward_gather: d3m_face_light_backward for ONE shared mesh (vertices [V,3], grad_light [F',3]), the same
 * per-face terms gathered per vertex: grad_vertices [V,3] is WRITTEN. */
int d3m_vertex_gather(const float* grad_faces_a, const float* grad_faces_b, const int32_t* adj_offsets,
                      const int32_t* adj_items, float* grad_vertices, int batch_size, int num_vertices, int num_tri,
                      int fill_back, const void* visibility, d3m_stream_t stream);
int d3m_face_light_backward_gather(const float* vertices, const int32_t* tri, const int32_t* adj_offsets,
                                   const int32_t* adj_items, const float* grad_light, float* grad_vertices,
                                   float intensity_ambient, float intensity_directional, const float* color_ambient,
                                   const float* color_directional, const float* direction, int num_vertices, int num_tri,
                                   int fill_back, d3m_stream_t stream);
/* The form (0 | 1) a launch of d3m_forward_face_index_map_mesh on `batch_size` views of a mesh of `num_triangles` triangles
 * (before fill_back) at `image_size` takes with a workspace of d3m_forward_workspace_bytes(); -1 for invalid sizes.  The
 * automatic choice: bidding for sub-pixel triangles (more than two per three raster pixels) whatever the batch; per-tile
 * lists for big batches (d3m_forward_big_batch) and for coarse meshes (more than 10 raster pixels per triangle; with at
 * least 65 536 (view, triangle) pairs in the batch more than 10 + 2 (views - 1), at most 32); bidding otherwise. */
int d3m_forward_coverage_form(int batch_size, int num_triangles, int image_size);
/* 1 when the launch is a BIG BATCH of an ordinary mesh (more than 65 536 blocks of 8 x 8 pixels, triangles not sub-pixel):
 * every kernel of a step fills the chip by itself.  (Rounds 4-5 ran such a step's branches on one stream; since round 6
 * they run beside each other at every size.  The camera-sharded fit still keys its split exchange on it.) */
int d3m_forward_big_batch(int batch_size, int num_triangles, int image_size);

/* Replaces forward_face_index_map (KCPP:70-95 -> KCU:24-169: kernels 1 and 2).
 *   faces          [B,F,3,3] f32 in   NDC x,y in [-1,1] (+y up), z = depth
 *   face_index_map [B,S,S]   i32 out  index of the nearest covering face, -1 where uncovered
 *   weight_map     [B,S,S,3] f32 out  clamped+renormalised barycentrics of that face, 0 where uncovered
 *   depth_map      [B,S,S]   f32 out  perspective-correct depth, `far` where uncovered
 *   face_inv_map   [B,S,S,3,3] f32 out, written only if return_depth != 0 (may be NULL otherwise), 0 where uncovered
 *   (the uncovered values are the reference's pre-fill, rasterize.py:50-58: every pixel is written, so a caller
 *   that pre-fills as the reference does and one that passes uninitialised memory get the same maps)
 *   faces_inv      [B,F,3,3] f32 i/o  scratch the reference fills for front-facing faces (may be NULL)
 * Row 0 of the maps is the BOTTOM of the image (the flip happens in Python, rasterize.py:305-317). */
int d3m_forward_face_index_map(const float* faces, int32_t* face_index_map, float* weight_map,
                               float* depth_map, float* face_inv_map, float* faces_inv, int batch_size,
                               int num_faces, int image_size, float near, float far, int return_rgb,
                               int return_alpha, int return_depth, void* workspace, size_t workspace_bytes,
                               d3m_stream_t stream);

/* d3m_forward_face_index_map on an INDEXED mesh (an addition): vertices [B,V,3] (screen space), tri [Bt,Ft,3]
 * (Bt = 1: shared), fill_back appends the reversed-winding copies (renderer.py:86), i.e. num_faces =
 * (fill_back ? 2 : 1) * num_tri.  The faces are read through the indices and faces_out [B,num_faces,3,3] receives
 * the dense copy of the faces that CAN OWN A PIXEL -- front-facing, and with a pixel centre inside their (dilated) box:
 * what vertices_to_faces would have produced for the faces any later operator can touch -- so the gather needs no
 * pass of its own.  Every other entry of faces_out is left UNDEFINED (whatever the buffer held: it may be NaN); a
 * caller that sweeps the whole array must fill it first, or use d3m_gather_faces.  Workspace as
 * d3m_forward_workspace_bytes(B, num_faces, S). */
int d3m_forward_face_index_map_mesh(const float* vertices, const int32_t* tri, int tri_batch, int num_vertices,
                                    int num_tri, int fill_back, float* faces_out, int32_t* face_index_map,
                                    float* weight_map, float* depth_map, float* face_inv_map, int batch_size,
                                    int image_size, float near, float far, void* workspace, size_t workspace_bytes,
                                    void* visibility, size_t visibility_size, int flags, d3m_stream_t stream);
/* The same, also writing -- in its last pass -- the output images of the renderer's silhouette / depth modes WITHOUT
 * anti-aliasing (NR/renderer.py:114-183; what d3m_output_epilogue makes of the maps in a pass of its own): alpha_map [B,S,S]
 * (1 where covered; internal layout, row 0 = bottom: what the edge gradient reads), alpha_out and depth_out [B,S,S] (the
 * same and depth_map with the rows reversed, rasterize.py:311-317).  Any of the three may be NULL; face_inv_map must be
 * NULL when one is given (D3M_ERR_INVALID otherwise). */
int d3m_forward_face_index_map_mesh_modes(const float* vertices, const int32_t* tri, int tri_batch, int num_vertices,
                                          int num_tri, int fill_back, float* faces_out, int32_t* face_index_map,
                                          float* weight_map, float* depth_map, float* face_inv_map, int batch_size,
                                          int image_size, float near, float far, void* workspace, size_t workspace_bytes,
                                          void* visibility, size_t visibility_size, float* alpha_map, float* alpha_out,
                                          float* depth_out, int flags, d3m_stream_t stream);
/* flags: D3M_PRECLEARED -- the caller has zeroed the first d3m_forward_clear_bytes(...) bytes of `workspace` (the tile
 * counters and arrival tickets of the per-tile lists, or the z-buffer of the bidding form: whichever form a launch with
 * THIS workspace size takes); 0: the operator clears them itself. */
size_t d3m_forward_clear_bytes(int batch_size, int num_tri, int fill_back, int image_size, size_t workspace_bytes);
/* tri == NULL with tri_batch = -W (here, in d3m_face_light(_backward) and in d3m_vertex_target): the IMPLICIT topology of
 * a depth map's grid mesh with W vertices per row (deep3dmap/core/renderer/utils.py:74-78: num_vertices = H*W, num_tri =
 * 2 (H-1)(W-1), cell (y, x) carries (tl, bl, tr) in the first half of the list and (tr, bl, br) in the second) -- NrRenderer's
 * meshes need no index tensor.
 * `visibility` (NULL, or a blob of d3m_visibility_bytes(B, num_faces)): the tile pass then also leaves the first step
 * of d3m_visibility -- which faces own a pixel -- in the blob, and d3m_visibility(NULL, blob, ...) finishes it without a
 * pass over face_index_map. */

/* Replaces forward_texture_sampling (KCPP:97-124 -> KCU:172-242).
 *   textures [B,F,ts,ts,ts,3] f32 in; rgb_map [B,S,S,3] f32 i/o; sampling_index_map [B,S,S,8] i32 i/o;
 *   sampling_weight_map [B,S,S,8] f32 i/o (the last two may be NULL: they are recomputable). */
int d3m_forward_texture_sampling(const float* faces, const float* textures, const int32_t* face_index_map,
                                 const float* weight_map, const float* depth_map, float* rgb_map,
                                 int32_t* sampling_index_map, float* sampling_weight_map, int batch_size,
                                 int num_faces, int image_size, int texture_size, float eps,
                                 d3m_stream_t stream);

/* Replaces backward_pixel_map (KCPP:126-150 -> KCU:245-503).  Writes (not accumulates) the 9 entries of
 * every face that owns at least one pixel in grad_faces [B,F,3,3] (x,y carry the gradient, z is set to
 * 0).  grad_faces must arrive zero-initialised, as RasterizeFunction.backward provides it
 * (rasterize.py:111): the reference also stores zeros for front-facing faces without pixels and leaves
 * culled faces untouched, which is then identical.  rgb_map/grad_rgb_map may be NULL when return_rgb == 0, alpha
 * likewise.  workspace: d3m_backward_pixel_map_workspace_bytes() bytes of scratch (no init needed); with less -- down to
 * d3m_backward_pixel_map_workspace_min_bytes() -- the crossings that find no room are walked one thread each (slow,
 * same result); below that D3M_ERR_WORKSPACE. */
size_t d3m_backward_pixel_map_workspace_bytes(int batch_size, int num_faces, int image_size);
size_t d3m_backward_pixel_map_workspace_min_bytes(int batch_size, int num_faces, int image_size);
/* Optional destination of face gradients (an ADDITION to the reference's interface; NULL = the dense grad_faces):
 * when `faces` was gathered from vertices (vertices_to_faces + fill_back, renderer.py:86 / vertices_to_faces.py),
 * the gradient of each face corner is accumulated straight into grad_vertices [B,num_vertices,3] (+=, float
 * atomics) - the composition with the adjoint of that gather - and grad_faces may be NULL. */
typedef struct {
    float* grad_vertices;
    const int32_t* tri;     /* [tri_batch, num_tri, 3]; num_faces = (fill_back ? 2 : 1) * num_tri */
    int num_vertices, num_tri, tri_batch, fill_back;
} d3m_vertex_target;
/* `unscaled` (NULL = the gradient maps are final): the maps are the unscaled ones a fused fit objective left
 * (d3m_render_lit_epilogue with fit->grad_*_map, see struct d3m_fit_targets below); their scalar factors are applied
 * as the maps are read.
 * Alpha only (return_alpha, not return_rgb) with FINAL gradients takes no pass over the pixels to pack them: the walks read
 * grad_alpha_map and face_index_map as they are.  The same for the gradient of the OUTPUT image instead of the internal map:
 * `unscaled` with only grad_alpha_map = that image's gradient [B,s,s] and flags = D3M_GRAD_OF_OUTPUT_IMAGE (s = image_size:
 * the image is the alpha map with its rows reversed) or D3M_GRAD_OF_OUTPUT_IMAGE | D3M_FIT_POOLED (s = image_size / 2: its 2x2
 * average); the argument grad_alpha_map is then not read (NULL).  Any other `unscaled` without scratch or records: D3M_ERR_INVALID. */
typedef struct d3m_fit_targets d3m_fit_targets;
int d3m_backward_pixel_map(const float* faces, const int32_t* face_index_map, const float* rgb_map,
                           const float* alpha_map, const float* grad_rgb_map, const float* grad_alpha_map,
                           float* grad_faces, int batch_size, int num_faces, int image_size, float eps,
                           int return_rgb, int return_alpha, void* workspace, size_t workspace_bytes,
                           const d3m_vertex_target* vertex_target, void* visibility, void* edge_plan,
                           size_t edge_plan_size, const d3m_fit_targets* unscaled, d3m_stream_t stream);

/* Which faces own a pixel depends on face_index_map only.  d3m_visibility builds, once per forward result, the
 * flags and the compacted list of those faces in a caller-owned blob of d3m_visibility_bytes(); backward operators
 * that are handed the blob (`visibility`, NULL = each builds its own) skip that work and run over the list.
 * face_index_map NULL: the blob went through d3m_forward_face_index_map_mesh, which left the first step in it (the
 * marks) and cleared the list's counter -- ONE finishing call per forward: the list is appended under that counter, so a
 * second d3m_visibility(NULL, ...) on the same blob without a new forward would append the list a second time (call with
 * the face_index_map instead, which clears first).  The list is ascending within chunks of 8192 faces; the chunks land in
 * arrival order, so the ORDER of the list -- and with it the order of the float atomics of the passes that run over it
 * -- may differ from run to run (the sums agree to rounding; the flags and the set of listed faces do not vary). */
size_t d3m_visibility_bytes(int batch_size, int num_faces);
int d3m_visibility(const int32_t* face_index_map, void* visibility, size_t visibility_size, int batch_size,
                   int num_faces, int image_size, d3m_stream_t stream);
/* Where the edges of the visible faces cross the pixel grid -- every walk of KCU:312-362 / :417-431 starts at such a
 * crossing -- depends on `faces` and face_index_map only, not on the gradient maps.  d3m_edge_plan builds, once per
 * forward result, the crossings' records (position, the in-pixel and whether the face owns it, the inward walk's end,
 * the first factors of KCU:404/:409's `dist`) grouped by image line in a caller-owned blob of d3m_edge_plan_bytes() (less is
 * accepted down to d3m_edge_plan_min_bytes(): crossings without room are then walked the slow way);
 * d3m_backward_pixel_map handed the blob (`edge_plan`, NULL = it builds its own in its workspace) starts with the
 * line walk.  `visibility`: the d3m_visibility blob of the same forward result (required). */
size_t d3m_edge_plan_bytes(int batch_size, int num_faces, int image_size);
/* Two arrays of [B,2,S] ints inside the plan blob's zeroed prefix, at the returned byte offset and *bytes_each behind it,
 * which d3m_edge_plan clears together with its own counters: a caller that builds the plan BEFORE it renders with a fused
 * fit objective on the same stream may use them as d3m_fit_targets.edge_nz_lo_inv / edge_nz_hi1 ("zeroed by the caller")
 * and saves the launch that clears them.  The plan itself does not use them. */
size_t d3m_edge_plan_extents_offset(int batch_size, int num_faces, int image_size, size_t* bytes_each);
size_t d3m_edge_plan_min_bytes(int batch_size, int num_faces, int image_size);
/* flags: D3M_PRECLEARED -- the caller has zeroed the blob's first d3m_edge_plan_clear_bytes() bytes (line counters,
 * cursors, arrival tickets and the extents above). */
size_t d3m_edge_plan_clear_bytes(int batch_size, int num_faces, int image_size);
int d3m_edge_plan(const float* faces, const int32_t* face_index_map, void* visibility, void* edge_plan,
                  size_t edge_plan_size, int batch_size, int num_faces, int image_size, int flags, d3m_stream_t stream);

/* Scratch for the two entry points below: one int per face.  With it the sums are GATHERED per visible
 * face (no atomics; faces with a very large bounding box still use the per-pixel atomic kernel);
 * without it (NULL) the reference's per-pixel float atomics are used throughout. */
size_t d3m_backward_faces_workspace_bytes(int batch_size, int num_faces);

/* Replaces backward_textures (KCPP:152-168 -> KCU:506-540): grad_textures [B,F,ts,ts,ts,3] += .
 * `faces` [B,F,3,3] is an ADDITION to the reference's argument list (needed to gather per face; pass
 * NULL to force the atomic form). */
int d3m_backward_textures(const float* faces, const int32_t* face_index_map, const float* sampling_weight_map,
                          const int32_t* sampling_index_map, const float* grad_rgb_map, float* grad_textures,
                          int batch_size, int num_faces, int image_size, int texture_size, void* workspace,
                          size_t workspace_bytes, d3m_stream_t stream);

/* Replaces backward_depth_map (KCPP:170-191 -> KCU:543-592): grad_faces += (after backward_pixel_map).
 * face_inv_map may be NULL: the face inverse is then recomputed from `faces` (bit-identical values). */
int d3m_backward_depth_map(const float* faces, const float* depth_map, const int32_t* face_index_map,
                           const float* face_inv_map, const float* weight_map, const float* grad_depth_map,
                           float* grad_faces, int batch_size, int num_faces, int image_size, void* workspace,
                           size_t workspace_bytes, d3m_stream_t stream);

/* d3m_backward_depth_map for a mesh pipeline (faces = the dense copy d3m_forward_face_index_map_mesh left, visibility = the
 * blob it marked and d3m_visibility finished): runs over the listed faces only and ADDS its sums straight into
 * vertex_target->grad_vertices (float atomics) -- no dense grad_faces, no scatter-add pass behind it.  large_counter: 256
 * bytes, zero when the kernels start (cleared here unless flags & D3M_PRECLEARED).  flags & D3M_GRAD_OF_OUTPUT_IMAGE:
 * grad_depth_map is the gradient of the OUTPUT depth image [B,S,S] of a render without anti-aliasing (rows top to bottom,
 * rasterize.py:311-317) -- read with the flip undone, so the adjoint of the output epilogue needs no pass of its own. */
#define D3M_GRAD_OF_OUTPUT_IMAGE 32
int d3m_backward_depth_map_mesh(const float* faces, const float* depth_map, const int32_t* face_index_map,
                                const float* weight_map, const float* grad_depth_map, int batch_size, int num_faces,
                                int image_size, const d3m_vertex_target* vertex_target, void* visibility,
                                void* large_counter, int flags, d3m_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * B. The eager-torch steps either side of those operators, as single HIP passes.
 * ---------------------------------------------------------------------------------------------- */

/* Camera parameter block, HOST memory, copied by value into the launch.
 *   LOOK_AT / LOOK : rot = rows (x_axis, y_axis, z_axis) per view, eye per view
 *                    (neural_renderer/look_at.py:48-60, look.py:39-51), then, if perspective != 0,
 *                    x,y /= z * tan(viewing_angle) (perspective.py:13-20; `inv_width`= 1/tan is NOT
 *                    used: the divisions are kept as the reference writes them).
 *   PROJECTION     : v*R^T + t, x/(z+1e-9), distortion (k1,k2,p1,p2,k3), K, v = orig-v, map to
 *                    [-1,1] (projection.py:19-42).
 * Per-view arrays live on the DEVICE: rot [Bc,3,3], eye_or_t [Bc,3], K [Bc,3,3], dist [Bc,5]; Bc is
 * either 1 (broadcast) or batch_size. */
typedef struct d3m_camera {
    int mode;              /* D3M_CAMERA_* */
    int perspective;       /* look / look_at only */
    float tan_half_width;  /* tan(viewing_angle), look / look_at only */
    float orig_size;       /* projection only */
    const float* rot;      /* device: look/look_at basis rows, or projection R */
    const float* eye_or_t; /* device: look/look_at eye, or projection t */
    const float* K;        /* device: projection only */
    const float* dist;     /* device: projection only */
    int rot_batch, eye_batch, K_batch, dist_batch; /* 1 or batch_size each */
} d3m_camera;

/* look_at / look basis on the device (look_at.py:48-53, look.py:39-44): rot_out [B,3,3] rows
 * (x_axis, y_axis, z_axis); eye/at_or_direction/up are [n,3] device arrays with n = 1 or B.
 * is_look_at != 0: z = normalise(at - eye); else z = normalise(direction). */
int d3m_camera_basis(const float* eye, int eye_batch, const float* at_or_direction, int at_batch, const float* up,
                     int up_batch, int is_look_at, float* rot_out, int batch_size, d3m_stream_t stream);

/* vertices [Bv,V,3] (Bv = 1 broadcasts one mesh to every view) -> out [B,V,3] in NDC + depth. */
/* d3m_lit_front -- the FIRST launch of a lit render step, three jobs in one grid (each optional):
 *   camera   screen_out [B,V,3] = camera(vertices) as d3m_camera_forward (cam NULL: none).  `basis` (look_at / look only,
 *            NULL: cam->rot holds the basis): the basis is computed here from eye / at_or_direction / up exactly as
 *            d3m_camera_basis does and ALSO stored to cam->rot ([rot_batch,3,3], writable) for d3m_camera_backward;
 *   light    light [light_batch, F', 3] as d3m_face_light (light NULL: none);
 *   clears   up to 10 (pointer, bytes) ranges zeroed (4-byte multiples, 4-byte aligned) -- see "Clears" above.
 * (NR/look_at.py:48-60 + NR/lighting.py:33-56 + the torch.zeros of NR/rasterize.py:50-58,111-115, as one kernel.) */
typedef struct d3m_basis {
    const float* eye;             /* [eye_batch,3] */
    const float* at_or_direction; /* [at_batch,3]: `at` (look_at) or the viewing direction (look) */
    const float* up;              /* [up_batch,3] */
    int eye_batch, at_batch, up_batch, is_look_at;
} d3m_basis;
int d3m_lit_front(const float* vertices, int vertices_batch, const d3m_camera* cam, const d3m_basis* basis, float* screen_out,
                  int batch_size, int num_vertices, const int32_t* tri, int tri_batch, int num_tri, int fill_back,
                  float* light, int light_batch, float intensity_ambient, float intensity_directional,
                  const float* color_ambient, const float* color_directional, const float* direction,
                  void* const* zero_ptrs, const size_t* zero_bytes, int zero_count, d3m_stream_t stream);
/* d3m_lit_back -- the LAST launch of such a step: grad_vertices [vertices_batch,V,3] += the camera's adjoint of grad_screen
 * [B,V,3] (d3m_camera_backward) + the light's adjoint of grad_light [light_batch,F',3] (d3m_face_light_backward), both with
 * float atomics in one grid: grad_vertices must hold zeros (or other contributions) when the launch starts. */
int d3m_lit_back(const float* vertices, int vertices_batch, const d3m_camera* cam, const float* grad_screen,
                 float* grad_vertices, int batch_size, int num_vertices, const int32_t* tri, int tri_batch, int num_tri,
                 int fill_back, const float* grad_light, int light_batch, float intensity_ambient,
                 float intensity_directional, const float* color_ambient, const float* color_directional,
                 const float* direction, d3m_stream_t stream);
int d3m_camera_forward(const float* vertices, int vertices_batch, const d3m_camera* cam, float* out,
                       int batch_size, int num_vertices, d3m_stream_t stream);
/* grad_vertices [Bv,V,3] = d(out)/d(vertices)^T grad_out; with Bv == 1 the B views are summed. */
int d3m_camera_backward(const float* vertices, int vertices_batch, const d3m_camera* cam,
                        const float* grad_out, float* grad_vertices, int batch_size, int num_vertices,
                        d3m_stream_t stream);
/* the same, ADDED to grad_vertices (which then already holds another path's share, e.g. d3m_face_light_backward's: the two
 * gradients of a mesh that is both projected and lit need no separate sum) */
int d3m_camera_backward_add(const float* vertices, int vertices_batch, const d3m_camera* cam,
                            const float* grad_out, float* grad_vertices, int batch_size, int num_vertices,
                            d3m_stream_t stream);
/* d3m_camera_params_backward -- the gradient of the camera's PARAMETERS from grad_screen [B,V,3] (what d3m_camera_backward
 * takes to the vertices) on vertices [vertices_batch,V,3].  The camera block is read when the kernels run (a captured graph
 * reads in-place updates of the parameters at replay).  look / look_at: the gradient of the rows (x, y, z) of cam->rot and
 * of the translation; with `basis` (the vectors cam->rot was made of, as d3m_lit_front takes them) the rows' gradient goes
 * on through the basis (F.normalize(eps=1e-5): in the clamped branch not through the norm) to eye, at_or_direction and up.
 * projection: R, t, K (row 3 gets zeros, as in the reference) and dist.  `grad` fields are WRITTEN in the shape of the
 * matching parameter (the batch of cam / basis; batch 1: the sum over the views in view order); a NULL field is skipped;
 * at_or_direction / up need `basis`, K / dist a projection.  Fixed-order two-stage reduction (per-(view, vertex chunk)
 * partials in `workspace`, then one ordered pass; no float atomics): bit-reproducible for a given grad_screen. */
typedef struct d3m_camera_grad {      /* each field: device, written in the shape of the matching parameter; NULL = skipped */
    float* eye_or_t;                  /* look_at / look: eye [eye_batch,3];  projection: t [eye_batch,3] */
    float* at_or_direction;           /* look_at: at;  look: direction  [at_batch,3] (needs the d3m_basis) */
    float* up;                        /* [up_batch,3] (needs the d3m_basis) */
    float* rot;                       /* projection: R [rot_batch,3,3];  look / look_at: the basis rows [rot_batch,3,3] */
    float* K;                         /* projection only: K [K_batch,3,3] (row 3 gets zeros, as in the reference) */
    float* dist;                      /* projection only: [dist_batch,5] */
} d3m_camera_grad;
size_t d3m_camera_params_backward_workspace_bytes(int batch_size, int num_vertices, int mode);
int d3m_camera_params_backward(const float* vertices, int vertices_batch, const d3m_camera* cam, const d3m_basis* basis,
                               const float* grad_screen, const d3m_camera_grad* grad, int batch_size, int num_vertices,
                               void* workspace, size_t workspace_bytes, d3m_stream_t stream);

/* vertices_to_faces (neural_renderer/vertices_to_faces.py:16-22) with the fill_back copy made on the
 * fly (renderer.py:86): faces_out [B,F',3,3], F' = 2F if fill_back else F; face F+f is face f with
 * vertex order reversed.  tri [Bt,F,3] i32, Bt = 1 or B. */
int d3m_gather_faces(const float* vertices, const int32_t* tri, int tri_batch, float* faces_out,
                     int batch_size, int num_vertices, int num_tri, int fill_back, d3m_stream_t stream);
/* Its backward: the per-vertex scatter-add.  grad_vertices [B,V,3] += ; wave-level pre-reduction of
 * lanes that hit the same vertex, then float atomics. */
int d3m_scatter_face_grads(const float* grad_faces, const int32_t* tri, int tri_batch, float* grad_vertices,
                           int batch_size, int num_vertices, int num_tri, int fill_back,
                           d3m_stream_t stream);

/* lighting (neural_renderer/lighting.py:33-56): light = ia*ca + id*cd*relu(normal . direction) per face,
 * normal = normalise(cross(v0-v1, v2-v1)) with F.normalize's eps 1e-5, on WORLD-space faces
 * (renderer.py:159); textures_out = textures_in * light (may alias for the reference's in-place form).
 *   faces [N,3,3], textures [N,ts,ts,ts,3] with N = num_faces_total (= B*F'); the three colour /
 *   direction vectors are HOST arrays of 3 floats. */
int d3m_lighting_forward(const float* faces, const float* textures_in, float* textures_out,
                         float intensity_ambient, float intensity_directional, const float* color_ambient,
                         const float* color_directional, const float* direction, long num_faces_total,
                         int texture_size, d3m_stream_t stream);
/* grad_textures [N,ts,ts,ts,3] = grad_out*light (NULL to skip); grad_faces [N,3,3] = gradient through
 * the face normal (NULL to skip; written, not accumulated). */
int d3m_lighting_backward(const float* faces, const float* textures_in, const float* grad_out,
                          float* grad_textures, float* grad_faces, float intensity_ambient,
                          float intensity_directional, const float* color_ambient, const float* color_directional,
                          const float* direction, long num_faces_total, int texture_size, d3m_stream_t stream);

/* get_transform_matrices (deep3dmap/core/renderer/utils.py:34-71): view [B,n] = (rx, ry, rz[, tx, ty[, tz]]), n = 3, 5
 * or 6 -> rot [B,3,3] = Rz Ry Rx and trans [B,3] (missing components 0), and its adjoint (grad_rot / grad_trans may be
 * NULL = zero).  One launch each way instead of ~35 eager kernels. */
int d3m_view_transform(const float* view, int num_components, float* rot, float* trans, int batch_size,
                       d3m_stream_t stream);
int d3m_view_transform_backward(const float* view, int num_components, const float* grad_rot, const float* grad_trans,
                                float* grad_view, int batch_size, d3m_stream_t stream);
/* NrRenderer's depth map -> warped pixel grid (deep3dmap/core/renderer/renderer_nr.py:74-114,141-158): every
 * "depth_to_3d_grid, then rigid transforms, then maybe grid_3d_to_2d" of the class in one pass.
 *   P = depth * inv_K (x, y, 1)^T;   Q = rot_b (P - c) + c + trans_b,  c = (0, 0, rot_center_depth)
 *   K == NULL: out [B,H*W,3] = Q;    K [1|B,3,3]: out [B,H,W,2] = ((K (Q / Q.z)).xy / (W-1, H-1)) * 2 - 1, the sampling
 *   grid of F.grid_sample (renderer_nr.py:82-88).
 * crop (NULL or {top, bottom, left, right}: render_yaw's crop_mesh, renderer_nr.py:145-158): border rows / columns take
 * the y,z / x,z of the first kept row / column.  Inverse warps and chains of transforms are composed into (rot, trans)
 * by the caller.  The adjoint (no crop) WRITES grad_depth [B,H,W], grad_rot [B,3,3], grad_trans [B,3] (each may be NULL). */
int d3m_grid_warp(const float* depth, const float* inv_K, int inv_K_batch, const float* rot, const float* trans,
                  float rot_center_depth, const float* K, int K_batch, const int* crop, float* out, int batch_size,
                  int height, int width, d3m_stream_t stream);
int d3m_grid_warp_backward(const float* depth, const float* inv_K, int inv_K_batch, const float* rot, const float* trans,
                           float rot_center_depth, const float* K, int K_batch, const float* grad_out, float* grad_depth,
                           float* grad_rot, float* grad_trans, int batch_size, int height, int width, d3m_stream_t stream);
/* NrRenderer.get_normal_from_depth (renderer_nr.py:127-139): normal [B,H,W,3] of the back-projected depth map, central
 * differences, (0,0,1) on the one-pixel border, normalised with EPS = 1e-7; and its adjoint (grad_depth WRITTEN). */
int d3m_depth_normals(const float* depth, const float* inv_K, int inv_K_batch, float* normal, int batch_size, int height,
                      int width, d3m_stream_t stream);
int d3m_depth_normals_backward(const float* depth, const float* inv_K, int inv_K_batch, const float* grad_normal,
                               float* grad_depth, int batch_size, int height, int width, d3m_stream_t stream);
/* get_textures_from_im (deep3dmap/core/renderer/utils.py:81-107): textures [B, 2(H-1)(W-1), ts^3, C] of the implicit
 * grid mesh from im [B,C,H,W], ts = 1 or 2 (anything else: D3M_ERR_INVALID, as utils.py:106 raises); and its adjoint
 * (grad_im WRITTEN). */
int d3m_textures_from_im(const float* im, float* textures, int batch_size, int channels, int height, int width,
                         int texture_size, d3m_stream_t stream);
int d3m_textures_from_im_backward(const float* grad_textures, float* grad_im, int batch_size, int channels, int height,
                                  int width, int texture_size, d3m_stream_t stream);

/* Pt3dRenderer.sample's per-pixel pass (deep3dmap/core/renderer/renderer_pt3d.py:75-97; the reference runs it through
 * pytorch3d 0.6.1's TexturesUV + SoftPhongShader): for the template mesh rasterized in UV space -- face_index_map /
 * weight_map [coverage_batch = 1|B, T,T(,3)] of d3m_forward_face_index_map on its fill_back faces -- every covered pixel samples
 * imgs [B,C<=3,H,W] bilinearly (align_corners, border padding, v up) at the barycentric mix of its face's per-vertex
 * image coordinates uvs [B,V,2] and shades it with pytorch3d's Phong model against the interpolated vertex normals
 * vnormals [V,3] at the interpolated position verts [V,3]:
 *     colour = (ambient + diffuse * relu(n.l)) * texel + specular * relu(v.r)^shininess [n.l > 0]
 * `light` = HOST array of 10 floats: light location (3), camera centre (3), ambient, diffuse, specular, shininess (the
 * products light colour x material colour; the reference's shader is built without lights / materials, so pytorch3d's
 * defaults apply: (0,1,0), (0,0,2.7), 0.5, 0.3, 0.2, 64).  out_img / out_mask [B,T,T,4] (row 0 = top): rgb = the colour
 * above / the same with texel = 1, alpha = coverage; zeros where nothing covers or used[b] == 0.
 * The adjoint ADDS into grad_imgs [B,C,H,W] and grad_uvs [B,V,2] (either may be NULL; caller zeroes). */
int d3m_uv_unwrap(const int32_t* face_index_map, const float* weight_map, const int32_t* tri, const float* verts,
                  const float* vnormals, const float* uvs, const float* imgs, const int32_t* used, const float* light,
                  float* out_img, float* out_mask, int batch_size, int coverage_batch, int texture_size, int num_tri,
                  int num_vertices, int channels, int height, int width, d3m_stream_t stream);
int d3m_uv_unwrap_backward(const int32_t* face_index_map, const float* weight_map, const int32_t* tri, const float* verts,
                           const float* vnormals, const float* uvs, const float* imgs, const int32_t* used,
                           const float* light, const float* grad_img, float* grad_imgs, float* grad_uvs, int batch_size,
                           int coverage_batch, int texture_size, int num_tri, int num_vertices, int channels, int height,
                           int width, d3m_stream_t stream);

/* --- lighting and fill_back applied on the fly (instead of renderer.py:155-167,203-215 materialising
 * cat(textures, textures.permute(0,1,4,3,2,5)) * light per view) ---------------------------------------
 * light [Bl,F',3]: per-face light of the fill_back'd face array on WORLD vertices [Bv,V,3] / tri [Bt,F,3];
 * Bl = 1 when one mesh is shared by every view, else the batch size. */
int d3m_face_light(const float* vertices, int vertices_batch, const int32_t* tri, int tri_batch, float* light,
                   float intensity_ambient, float intensity_directional, const float* color_ambient,
                   const float* color_directional, const float* direction, int light_batch, int num_vertices,
                   int num_tri, int fill_back, d3m_stream_t stream);
/* grad_light [Bl,F',3] -> grad_vertices [Bv,V,3] += (through the face normals; float atomics). */
int d3m_face_light_backward(const float* vertices, int vertices_batch, const int32_t* tri, int tri_batch,
                            const float* grad_light, float* grad_vertices, float intensity_ambient,
                            float intensity_directional, const float* color_ambient, const float* color_directional,
                            const float* direction, int light_batch, int num_vertices, int num_tri, int fill_back,
                            d3m_stream_t stream);
/* --- lights read from DEVICE memory (learnable lights, one light per view) ----------------------------------------------
 * d3m_light: the five light parameters as device arrays, each of batch 1 (every view) or light_batch (row b for light row
 * b, i.e. view b):  intensity_ambient [n], intensity_directional [n], color_ambient [n,3], color_directional [n,3],
 * direction [n,3].  The *_dev entry points read the rows when their kernels run (a captured graph reads the light at
 * replay, nothing of it is baked into kernel arguments) and evaluate the by-value forms' expression on them: a light that
 * is the same in every view gives the bits of d3m_face_light / d3m_lit_front.  light_batch is B whenever any parameter is
 * given per view, even for a shared mesh.  d3m_light_params_backward WRITES a gradient laid out the same way. */
typedef struct d3m_light {
    float* intensity_ambient;     /* [ia_batch] */
    float* intensity_directional; /* [id_batch] */
    float* color_ambient;         /* [ca_batch,3] */
    float* color_directional;     /* [cd_batch,3] */
    float* direction;             /* [dir_batch,3] */
    int ia_batch, id_batch, ca_batch, cd_batch, dir_batch; /* 1 or light_batch each */
} d3m_light;
/* d3m_face_light / d3m_face_light_backward with the light of d3m_light */
int d3m_face_light_dev(const float* vertices, int vertices_batch, const int32_t* tri, int tri_batch, float* light,
                       const d3m_light* params, int light_batch, int num_vertices, int num_tri, int fill_back,
                       d3m_stream_t stream);
int d3m_face_light_backward_dev(const float* vertices, int vertices_batch, const int32_t* tri, int tri_batch,
                                const float* grad_light, float* grad_vertices, const d3m_light* params, int light_batch,
                                int num_vertices, int num_tri, int fill_back, d3m_stream_t stream);
/* d3m_face_light_backward_gather with the light of d3m_light (every parameter of batch 1: one shared mesh) */
int d3m_face_light_backward_gather_dev(const float* vertices, const int32_t* tri, const int32_t* adj_offsets,
                                       const int32_t* adj_items, const float* grad_light, float* grad_vertices,
                                       const d3m_light* params, int num_vertices, int num_tri, int fill_back,
                                       d3m_stream_t stream);
/* d3m_lit_front / d3m_lit_back with the light of d3m_light (light_batch 1 or batch_size) */
int d3m_lit_front_dev(const float* vertices, int vertices_batch, const d3m_camera* cam, const d3m_basis* basis,
                      float* screen_out, int batch_size, int num_vertices, const int32_t* tri, int tri_batch, int num_tri,
                      int fill_back, float* light, int light_batch, const d3m_light* params, void* const* zero_ptrs,
                      const size_t* zero_bytes, int zero_count, d3m_stream_t stream);
int d3m_lit_back_dev(const float* vertices, int vertices_batch, const d3m_camera* cam, const float* grad_screen,
                     float* grad_vertices, int batch_size, int num_vertices, const int32_t* tri, int tri_batch, int num_tri,
                     int fill_back, const float* grad_light, int light_batch, const d3m_light* params, d3m_stream_t stream);
/* d3m_light_params_backward -- the gradient of the light's parameters from grad_light [light_batch,F',3] (the per-face
 * light's gradient, d3m_backward_textures_lit) on WORLD vertices [vertices_batch,V,3] / tri [tri_batch,F,3], the normals
 * recomputed as d3m_face_light does.  With r = relu(n . dir), G = grad_light, summed over the faces of a row:
 *   d ia = sum G . ca,  d ca = ia sum G,  d id = sum r (G . cd),  d cd = id sum r G,  d dir = id sum [n . dir > 0] (G . cd) n;
 * a term whose intensity is 0 gives zeros (NR/lighting.py:36,40).  `grad` fields are WRITTEN in the shape of the matching
 * `light` parameter (the same batch; batch 1: the sum over the rows); a NULL field is skipped.  Fixed-order two-stage
 * reduction (per-workgroup partials in `workspace`, then one ordered pass; no float atomics): bit-reproducible. */
size_t d3m_light_params_backward_workspace_bytes(int light_batch, int num_tri, int fill_back);
int d3m_light_params_backward(const float* vertices, int vertices_batch, const int32_t* tri, int tri_batch,
                              const float* grad_light, int light_batch, const d3m_light* light, const d3m_light* grad,
                              int num_vertices, int num_tri, int fill_back, void* workspace, size_t workspace_bytes,
                              d3m_stream_t stream);
/* forward_texture_sampling on the VIRTUAL lit array: faces [B,F',3,3] (F' = 2*num_tri if fill_back),
 * textures [Bx,num_tri,ts,ts,ts,3] (Bx = 1: shared), light [Bl,F',3]; writes rgb_map [B,S,S,3] for covered
 * pixels.  Colours are bit-identical to sampling the materialised array (same f32 products). */
int d3m_forward_texture_sampling_lit(const float* faces, const float* textures, int textures_batch, const float* light,
                                     int light_batch, const int32_t* face_index_map, const float* weight_map,
                                     const float* depth_map, float* rgb_map, int batch_size, int num_tri,
                                     int fill_back, int image_size, int texture_size, float eps, d3m_stream_t stream);
/* (forward sampling entry points only) textures_batch = -W, W >= 2: `textures` is an IMAGE [B,3,H,W] and the 2x2x2 cubes of
 * the grid mesh's faces (num_tri = 2 (H-1)(W-1), texture_size 2) are evaluated from it where they are sampled --
 * get_textures_from_im (deep3dmap/core/renderer/utils.py:81-107) without its [B,F,2,2,2,3] array; same bits.
 * d3m_forward_texture_sampling_lit followed by d3m_output_epilogue in one pass, without the intermediate
 * rgb_map: writes the blended internal-resolution rgb_blended [B,S,S,3] (covered ? sampled : background) and
 * alpha_map [B,S,S] (NULL to skip) that the backward pass reads, and the output images rgb_out [B,3,s,s],
 * alpha_out / depth_out [B,s,s] (NULL to skip; s = S/2 when anti_aliasing), flipped as rasterize.py:305-326.
 *
 * `fit` (NULL = none; an ADDITION to the reference's structure, not its interface): the multi-view fit objective
 *     photometric_loss(rgb, rgb_target, mask) + sum((alpha - alpha_target)^2) / (s*s) + photometric_loss(depth, ...)
 * (deep3dmap/core/utils/utils.py:105-114 composed as d3m_fit_loss_forward does) evaluated in the same pass, where
 * the images are produced: *fit->loss receives the value, the images themselves need not be written (rgb_out NULL)
 * and are not read again.  alpha_map is required.  With anti_aliasing the targets are at the output size s = S/2 and the
 * objective is that of the pooled images (the records form below then carries D3M_FIT_POOLED).
 * With fit->grad_*_map set the pass also leaves the objective's gradient wrt the internal-resolution maps
 * (rgb_blended, alpha_map, depth_map) there, WITHOUT the scalar factors that are only known later - sign(rgb - target)
 * * mask, 2 (alpha - target), sign(depth - target) * mask - so that backward needs no pass over the pixels of its
 * own: d3m_backward_pixel_map / d3m_backward_textures_lit handed these maps AND the same struct as `unscaled` (with
 * grad_loss filled in; NULL = 1) multiply by grad_loss / (3 sum(mask)), grad_loss / (s*s), grad_loss / sum(mask)
 * as they read them.  (d3m_fit_loss_backward followed by d3m_output_epilogue_backward, without either.) */
struct d3m_fit_targets {
    const float* rgb_target;     /* [B,3,S,S]  output image layout (flipped, channel-major) */
    const float* depth_target;   /* [B,S,S] */
    const float* alpha_target;   /* [B,S,S] */
    const float* mask;           /* [B,S,S] */
    float* scratch;              /* d3m_render_fit_scratch_floats() floats, kept from forward to backward */
    float* loss;                 /* [1] */
    float* grad_rgb_map;         /* [B,S,S,3] \                                                        */
    float* grad_alpha_map;       /* [B,S,S]    > unscaled gradient maps, written by the epilogue; all or none */
    float* grad_depth_map;       /* [B,S,S]   /                                                         */
    const float* grad_loss;      /* [1] device scalar, read by the backward operators; NULL = 1 */
    const float* mask_sum;       /* [1] device scalar or NULL.  NULL: the photometric terms are normalised by the sum of
                                  * `mask` over THIS batch.  When the batch is one rank's shard of a larger objective
                                  * (camera-sharded fit), the sum of the mask over ALL shards: the shard's value is then
                                  * its additive part of the global objective and gradients add up across ranks. */
    /* The gradient wrt rgb_blended / alpha_map in the form the edge gradient reads it (all four or none; needs mask_sum
     * and grad_depth_map; grad_rgb_map / grad_alpha_map are then not written and may be NULL): per pixel
     *   edge_grad = (2 (alpha - target) / (S*S), sign(rgb - target) mask / (3 mask_sum))      float4 [B,S,S]
     *   edge_dot  = (<(alpha, rgb), edge_grad>, face index bits)                               float2 [B,S,S]
     * and per image line (b*2 + axis)*S + d0 the extent of its non-zero records (caller-zeroed int [B,2,S] each:
     * S - first, last + 1).  Everything but grad_loss is in there; d3m_backward_pixel_map / d3m_backward_textures_lit
     * handed the struct as `unscaled` read the records instead of packing the maps (no pass over the pixels).
     * With anti_aliasing (flags & D3M_FIT_POOLED, required then and only then) the records stay per INTERNAL pixel: each of
     * an output pixel's four gets a quarter of its gradient -- (2 (alpha_o - target) / (S*S), sign(rgb_o - target) mask / 4 /
     * (3 mask_sum)) -- and grad_depth_map sign(depth_o - target) mask / 4. */
    void* edge_grad;
    void* edge_dot;
    int* edge_nz_lo_inv;
    int* edge_nz_hi1;
    int flags;                   /* D3M_PRECLEARED: the caller has zeroed the scratch's ticket word
                                  * (d3m_render_fit_scratch_clear_range) -- see "Clears" above; else the pass does it.
                                  * D3M_FIT_FINISH_DEFERRED (records form of d3m_render_lit_epilogue only): the pass leaves
                                  * its partial sums in `scratch` and does NOT complete *loss; d3m_backward_textures_lit,
                                  * handed this struct (same flag) as `unscaled`, completes it in a kernel it launches anyway --
                                  * for callers that run the backward pass right behind the forward pass: no finishing launch
                                  * D3M_FIT_POOLED: the records belong to an objective on the 2x2-pooled images (see above) */
    /* VOID TILES (optional; NULL = exactly the behaviour without it).  The summary d3m_fit_target_summary made of THESE
     * targets: one byte per (view, 16 x 16 tile of the output image), 1 = alpha_target == 0, mask == 0 and finite rgb /
     * depth targets at every pixel of the tile.  Records form without anti-aliasing only (ignored otherwise): a tile of the
     * pass whose targets are void and which no face covers stores its zero partial sums and one byte in `scratch`, reads
     * face_index_map alone (and depth_map where depth_out is given: the tile's depth_out is copied from it) and writes
     * neither rgb_blended, alpha_map, the records nor grad_depth_map there (rgb_out / alpha_out / depth_out, when given,
     * are written everywhere).  The summary must describe the targets AS THE KERNEL READS THEM: targets rewritten in place
     * need a new summary.  d3m_backward_pixel_map handed the SAME struct as `unscaled` (same
     * tile_void, scratch, batch and image size; return_rgb and return_alpha) stages those tiles' pixels as the constants the
     * pass would have stored; d3m_backward_textures_lit reads records only at pixels a face owns.  Nothing is carried from
     * one launch to the next: every tile writes its byte in every launch.  d3m_fit_loss_records writes every record and
     * refuses a struct with tile_void set. */
    const unsigned char* tile_void;
};
#define D3M_FIT_FINISH_DEFERRED 2
#define D3M_FIT_POOLED 4
/* ... or, should the backward pass not come that way after all, by this call (the ticket must still be zero: one finish). */
/* tile_void of a set of targets (see struct d3m_fit_targets): batch_size * ceil(image_size / 16)^2 bytes, written. */
int d3m_fit_target_summary(const float* rgb_target, const float* depth_target, const float* alpha_target, const float* mask,
                           unsigned char* tile_void, int batch_size, int image_size, d3m_stream_t stream);
/* Tile edge of the records form of the objective's pass (A/B runs and tests): -1 = by the launch's size (16 up to 4 M
 * pixels, 32 above), 0 = always 16, 1 = always 32.  Anything else: D3M_ERR_INVALID, no change.  The forward and the
 * backward pass of a step must run under the same setting. */
int d3m_set_fit_tile_form(int form);
int d3m_get_fit_tile_form(void);
int d3m_fit_finish(const d3m_fit_targets* fit, int batch_size, int image_size, d3m_stream_t stream);
/* scratch: totals | partial sums | group sums | ticket | void tiles: the views' backgrounds and one byte per tile. */
size_t d3m_render_fit_scratch_floats(int batch_size, int image_size);
size_t d3m_render_fit_scratch_clear_range(int batch_size, int image_size, size_t* offset_floats);   /* returns a count of floats */
/* offset (in floats) of the void-tile flags a records-form pass with fit->tile_void leaves in the scratch: one byte per tile */
size_t d3m_render_fit_scratch_tile_void_offset(int batch_size, int image_size);
/* The same objective evaluated on FINISHED images -- rgb [B,3,S,S], depth / alpha [B,S,S], row 0 = top: what
 * d3m_render_lit_epilogue wrote as rgb_out / depth_out / alpha_out without anti-aliasing -- with its gradient left as the
 * edge gradient's per-pixel records, exactly as the fused pass leaves them (fit->edge_grad, edge_dot, edge_nz_* zeroed by
 * the caller, grad_depth_map, mask_sum; *fit->loss is complete on return of the stream).  face_index_map [B,S,S] (row 0 =
 * bottom) supplies the records' owner.  This is how the reference-shaped composition  loss(*renderer.render(...))
 * (NR/renderer.py:200-246 + the caller's loss) reaches the records route of d3m_backward_pixel_map /
 * d3m_backward_textures_lit without gradient images. */
int d3m_fit_loss_records(const float* rgb, const float* depth, const float* alpha, const int32_t* face_index_map,
                         const d3m_fit_targets* fit, int batch_size, int image_size, d3m_stream_t stream);
int d3m_render_lit_epilogue(const float* faces, const float* textures, int textures_batch, const float* light,
                            int light_batch, const int32_t* face_index_map, const float* weight_map,
                            const float* depth_map, const float* background, int background_batch,
                            float* rgb_blended, float* alpha_map, float* rgb_out, float* alpha_out, float* depth_out,
                            int batch_size, int num_tri, int fill_back, int image_size, int texture_size, float eps,
                            int anti_aliasing, const d3m_fit_targets* fit, d3m_stream_t stream);
/* Its backward (replaces backward_textures + the adjoint of lighting and of the fill_back cat):
 * grad_textures [Bx,num_tri,ts^3,3] is WRITTEN (summed over views when Bx = 1); grad_light [Bl,F',3] is
 * written when not NULL.  Sampling weights are recomputed from weight_map / depth_map (no 64 B/pixel
 * sampling maps).  Gathered per visible face for ts = 2, per-pixel float atomics otherwise.
 * grad_depth_map [B,S,S] / grad_faces [B,F',3,3] (both or neither): when given, the depth gradient of
 * backward_depth_map (KCU:543-592) is ADDED to grad_faces in the same pass over the faces' pixels, i.e. this one
 * call then stands for backward_textures + backward_depth_map of rasterize.py:146-151.  With vertex_target the
 * depth gradient goes to grad_vertices instead and grad_faces may be NULL. */
size_t d3m_backward_textures_lit_workspace_bytes(int batch_size, int num_tri, int fill_back, int texture_size);
int d3m_backward_textures_lit(const float* faces, const float* textures, int textures_batch, const float* light,
                              int light_batch, const int32_t* face_index_map, const float* weight_map,
                              const float* depth_map, const float* grad_rgb_map, float* grad_textures, float* grad_light,
                              const float* grad_depth_map, float* grad_faces, int batch_size, int num_tri, int fill_back,
                              int image_size, int texture_size, float eps, void* workspace, size_t workspace_bytes,
                              const d3m_vertex_target* vertex_target, void* visibility,
                              const d3m_fit_targets* unscaled, int flags, d3m_stream_t stream);
/* flags: D3M_PRECLEARED -- the caller has zeroed the (up to four) ranges d3m_backward_textures_lit_clear_ranges reports for
 * the same arguments: grad_light, the workspace's view masks / counter / arrival tickets (and, where they apply, the
 * per-view gradients and the flags).  Returns the number of ranges written to ptrs / bytes (room for four). */
int d3m_backward_textures_lit_clear_ranges(float* grad_textures, int textures_batch, float* grad_light, int light_batch,
                                           int batch_size, int num_tri, int fill_back, int texture_size, void* workspace,
                                           int has_visibility, void** ptrs, size_t* bytes);

/* Output epilogue of rasterize_rgbad (rasterize.py:305-326) in one pass: background blend + alpha
 * (rasterize.py:181-195), HWC->CHW, vertical flip, optional 2x2 average pool.
 *   in : face_index_map [B,S,S], rgb_map [B,S,S,3] (sampled, NOT yet blended; NULL if !rgb),
 *        depth_map [B,S,S] (NULL if !depth); background [Bb,3] device, Bb = 1 or B.
 *   out: rgb_out [B,3,s,s], alpha_out [B,s,s], depth_out [B,s,s]  (s = S/2 if anti_aliasing else S);
 *        rgb_blended [B,S,S,3] and alpha_map [B,S,S] are the internal-resolution maps the backward
 *        needs (either may be NULL when the mode does not use it). */
int d3m_output_epilogue(const int32_t* face_index_map, const float* rgb_map, const float* depth_map,
                        const float* background, int background_batch, float* rgb_blended, float* alpha_map,
                        float* rgb_out, float* alpha_out, float* depth_out, int batch_size, int image_size,
                        int anti_aliasing, d3m_stream_t stream);
/* Its adjoint: output-resolution grads -> internal maps grad_rgb_map [B,S,S,3], grad_alpha_map [B,S,S],
 * grad_depth_map [B,S,S] (un-pool, un-flip, CHW->HWC).  No coverage mask is applied: the reference
 * blends the background inside RasterizeFunction.forward, so its backward kernels receive the
 * gradient wrt the blended image at every pixel (rasterize.py:83,141-147).  NULL pairs are skipped. */
int d3m_output_epilogue_backward(const float* grad_rgb_out, const float* grad_alpha_out,
                                 const float* grad_depth_out, float* grad_rgb_map, float* grad_alpha_map,
                                 float* grad_depth_map, int batch_size, int image_size, int anti_aliasing,
                                 d3m_stream_t stream);
/* The same adjoint, with the rgb / alpha gradients leaving as the per-pixel records the edge gradient walks over
 * (edge_grad [B,S,S] float4, edge_dot [B,S,S] float2, the lines' non-zero extents edge_nz_* [B,2,S] i32: see
 * d3m_fit_targets) instead of gradient maps; the depth gradient still leaves as a map.  d3m_backward_pixel_map and
 * d3m_backward_textures_lit take the records through `unscaled` with scratch = grad_loss = mask_sum = NULL (final). */
int d3m_output_epilogue_backward_records(const float* grad_rgb_out, const float* grad_alpha_out,
                                         const float* grad_depth_out, const int32_t* face_index_map,
                                         const float* rgb_map, const float* alpha_map, void* edge_grad, void* edge_dot,
                                         int* edge_nz_lo_inv, int* edge_nz_hi1, float* grad_depth_map, int batch_size,
                                         int image_size, int anti_aliasing, d3m_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * C. Losses on the path (deep3dmap/core/utils/utils.py:82-114; examples/example2.py:43-47).
 *    Each writes ONE f32 to `loss` (device) and, if grad_* != NULL, the gradient for d(loss) = 1.
 * ---------------------------------------------------------------------------------------------- */
/* photometric_loss(im1, im2, mask, conf_sigma): im [B,C,H,W]; mask/conf_sigma [B,1,H,W] or NULL.
 * scratch: 2048 floats of device memory (per-workgroup partial sums; no initialisation needed);
 * batch_size * channels must not exceed 1024. */
int d3m_photometric_loss(const float* im1, const float* im2, const float* mask, const float* conf_sigma,
                         float* loss, float* grad_im1, float* scratch, int batch_size, int channels,
                         int height, int width, d3m_stream_t stream);
/* sum((a-b)^2) over n elements (silhouette loss of the examples).  scratch: 1024 floats. */
int d3m_sum_squared_error(const float* a, const float* b, float* loss, float* grad_a, float* scratch, long n,
                          d3m_stream_t stream);

/* smooth_loss of ONE map pred [B,H,W] (deep3dmap/core/utils/utils.py:82-102, one pyramid level, weight 1):
 * mean|dxx| + mean|dxy| + mean|dyx| + mean|dyy| of the nested first differences; H, W >= 3.  scratch: 4096 floats.
 * backward: grad_pred = *grad_loss * d loss / d pred (grad_loss is a device scalar). */
int d3m_smooth_loss_forward(const float* pred, float* loss, float* scratch, int batch_size, int height, int width,
                            d3m_stream_t stream);
int d3m_smooth_loss_backward(const float* pred, const float* grad_loss, float* grad_pred, int batch_size, int height,
                             int width, d3m_stream_t stream);

/* The multi-view fit objective in one reduction + one finish launch, and its gradients in one
 * more:  loss = photometric_loss(rgb, rgb_target, mask) + sum((alpha - alpha_target)^2) / (H*W)
 *             + photometric_loss(depth, depth_target, mask)
 * with rgb [B,3,H,W], depth / alpha / mask [B,H,W].  Same value and gradients as composing the three operators
 * above.  scratch: 4104 floats, written by forward and read by backward (it keeps the reduction totals).
 * grad_loss: device scalar (NULL = 1).  Any of the grad_* outputs may be NULL.
 * mask_sum: device scalar replacing sum(mask) as the photometric terms' normaliser (NULL = sum over this batch; see
 * struct d3m_fit_targets). */
int d3m_fit_loss_forward(const float* rgb, const float* rgb_target, const float* depth, const float* depth_target,
                         const float* alpha, const float* alpha_target, const float* mask, float* loss, float* scratch,
                         const float* mask_sum, int batch_size, int height, int width, d3m_stream_t stream);
int d3m_fit_loss_backward(const float* rgb, const float* rgb_target, const float* depth, const float* depth_target,
                          const float* alpha, const float* alpha_target, const float* mask, const float* scratch,
                          const float* grad_loss, float* grad_rgb, float* grad_depth, float* grad_alpha, int batch_size,
                          int height, int width, d3m_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * D. The renderer block of the gan2shape training step as fused passes (deep3dmap/models/frameworks/gan2shape.py:444,
 *    463-497 through NrRenderer, deep3dmap/core/renderer/renderer_nr.py:61-139):
 *
 *      rot, trans      = get_transform_matrices(view)   (when `view` is given; else rot / trans are inputs)   utils.py:54-71
 *      normal          = get_normal_from_depth(depth)                                           renderer_nr.py:127-139
 *      diffuse_shading = clamp((normal . light_d), min=0);  shading = light_a + light_b * diffuse_shading
 *      texture         = (albedo / 2 + 0.5) * shading * 2 - 1                                   gan2shape.py:463-466
 *      recon_depth     = warp_canon_depth(depth)    the depth map's grid mesh (implicit topology, fill_back) moved by
 *                        (rot, trans), projected by `camera`, rasterized in depth mode, clamped  renderer_nr.py:116-125
 *      recon_im_mask   = (recon_depth < depth_max) [* the other half's with `flip`] [* extra_mask]   gan2shape.py:476-482
 *      recon_im        = clamp(grid_sample(texture, get_inv_warped_2d_grid(recon_depth)), -1, 1)  gan2shape.py:475,483
 *      losses[0]       = photometric_loss(recon_im[:b], target, mask[:b])    (b = batch_size, or half of it with flip)
 *      losses[1]       = photometric_loss(recon_im[b:], target, mask[b:])    (flip only, else 0)    gan2shape.py:486,489
 *      losses[2]       = smooth_loss(depth) + smooth_loss(diffuse_shading)   (with_smooth)          gan2shape.py:493-494
 *      losses[3]       = losses[0] + losses[1] + lam_smooth * losses[2]
 *
 *    d3m_g2s_forward: 4 launches; d3m_g2s_backward: 5 (gradients for depth, albedo, light_a, light_b, light_d and the
 *    view -- as rot / trans and, with `view`, the view vector -- from the gradients of recon_im and of the four loss
 *    values).  The mesh is rasterized by bidding (depth, face) into a 64-bit z-buffer (its triangles are a few pixels
 *    each): same coverage, depth and tie rule as d3m_forward_face_index_map.  Device pointers unless marked. */
typedef struct d3m_g2s_block {
    int batch_size, height, width;       /* canonical maps: depth [B,H,W], albedo [B,3,H,W] */
    int image_size, anti_aliasing;       /* output images [B,.,s,s]; the mesh is rasterized at 2s with anti-aliasing */
    int flip;                            /* entries (b, b + B/2) are an image and its mirror: shared mask product */
    const float* inv_K; int inv_K_batch; /* NrRenderer.inv_K / K, [1|B,3,3] */
    const float* K; int K_batch;
    float rot_center_depth;
    float depth_min, depth_max;          /* recon_depth is clamped to [depth_min, depth_max] (= min_depth - margin,
                                          * max_depth + margin of renderer_nr.py:122-124) */
    float near, far;                     /* of the depth rasterization (the rasterizer's defaults, NR/renderer.py:149) */
    const d3m_camera* camera;            /* HOST: the mesh renderer's camera (renderer_nr.py:47-54) */
    /* inputs */
    const float* view; int view_components;   /* [B, 3|5|6] view vectors, or NULL */
    float *rot, *trans;                  /* [B,3,3], [B,3]: inputs when view == NULL, else written (set_transform_matrices) */
    const float *depth, *albedo;
    const float *light_a, *light_b;      /* [B] */
    const float* light_d;                /* [B,3] */
    const float* target;                 /* [b,3,s,s] input_im, or NULL (no photometric terms) */
    const float* extra_mask;             /* [B,s,s] multiplied into recon_im_mask (gan2shape.py:672), or NULL */
    /* forward outputs (normal, recon_depth may be NULL) */
    float* normal;                       /* [B,H,W,3] */
    float* diffuse_shading;              /* [B,H,W] */
    float* texture;                      /* [B,3,H,W] */
    float* recon_depth;                  /* [B,s,s] */
    float* recon_im;                     /* [B,3,s,s] */
    float* recon_im_mask;                /* [B,s,s] */
    float* losses;                       /* [4] */
    float lam_smooth; int with_smooth;
    /* kept from forward to backward (caller-allocated, no initialisation) */
    float* screen_vertices;              /* [B,H*W,3] */
    uint64_t* zbuffer;                   /* [B,S,S], S = image_size * (anti_aliasing ? 2 : 1) */
    float* scratch;                      /* d3m_g2s_scratch_floats() */
    /* backward inputs: gradient of recon_im [B,3,s,s] and of the four loss values (device scalars); NULL = zero */
    const float *grad_recon_im, *grad_l1, *grad_l1_flip, *grad_smooth, *grad_total;
    /* backward scratch; grad_texture must already be handed to d3m_g2s_forward, which clears it; d3m_g2s_backward
     * hands it back zeroed, so any number of backward passes may follow one forward */
    float* grad_texture;                 /* [B,3,H,W] */
    float* grad_tri;                     /* [B, 2 (H-1)(W-1), 3, 3] */
    float* grad_depth_map;               /* [B,S,S] */
    float* grad_normal;                  /* [B,H,W,3] */
    float* grad_depth_mesh;              /* [B,H,W] */
    /* backward outputs (WRITTEN; any of light / rot / trans / view may be NULL) */
    float *grad_depth, *grad_albedo, *grad_light_a, *grad_light_b, *grad_light_d, *grad_rot, *grad_trans, *grad_view;
} d3m_g2s_block;
size_t d3m_g2s_scratch_floats(int batch_size, int height, int width, int image_size);
int d3m_g2s_forward(const d3m_g2s_block* block, d3m_stream_t stream);
int d3m_g2s_backward(const d3m_g2s_block* block, d3m_stream_t stream);

/* NrRenderer's grid_sample frames (renderer_nr.py:180-184, 219-222, 263-267) in one pass:
 *   grid = ((K (Q / Q.z)).xy / (w-1, h-1)) * 2 - 1,  Q = rot_b (depth * inv_K (x, y, 1) - c) + c + trans_b        (as d3m_grid_warp)
 *   out [B,C,h,w] = F.grid_sample(src [B,C,H,W], grid, mode='bilinear');  out_nearest [B,Cn,h,w] = F.grid_sample(src_nearest,
 *   grid, mode='nearest') (src_nearest may be NULL) -- zeros padding, align_corners = False.  depth [B,h,w] is the target
 *   view's depth (recon_depth), (rot, trans) [B,3,3] / [B,3] the composed rigid motion (the inverse view for the frames).
 * The adjoint ADDS into grad_src [B,C,H,W] (float atomics; caller zeroes; may be NULL) and WRITES grad_depth [B,h,w] (may be
 * NULL) and, per workgroup, the partial sums of the gradient of (rot, trans): partials [B, d3m_warp_resample_partials(h, w), 12]
 * (9 + 3; the caller adds them up). */
int d3m_warp_resample(const float* depth, const float* inv_K, int inv_K_batch, const float* K, int K_batch, const float* rot,
                      const float* trans, float rot_center_depth, const float* src, int channels, const float* src_nearest,
                      int channels_nearest, float* out, float* out_nearest, int batch_size, int height, int width,
                      int src_height, int src_width, d3m_stream_t stream);
int d3m_warp_resample_partials(int height, int width);
int d3m_warp_resample_backward(const float* depth, const float* inv_K, int inv_K_batch, const float* K, int K_batch,
                               const float* rot, const float* trans, float rot_center_depth, const float* src, int channels,
                               const float* grad_out, float* grad_src, float* grad_depth, float* partials, int batch_size,
                               int height, int width, int src_height, int src_width, d3m_stream_t stream);

/* ---- texture assets ----------------------------------------------------------------------------------------- */
/* Replaces load_textures_cuda (NR/cuda/load_textures_cuda.cpp:6-37, kernel load_textures_cuda_kernel.cu:23-114):
 * fills textures [F, ts, ts, ts, 3] of every face with is_update[f] != 0 by sampling image [H, W, 3] at
 * barycentric combinations of the face's uv corners faces_uv [F, 3, 2].  texture_wrapping: 0 REPEAT,
 * 1 MIRRORED_REPEAT, 2 CLAMP_TO_EDGE, 3 CLAMP_TO_BORDER (writes zeros, like the reference).  faces_uv is
 * read-only here (the reference wraps it in place; see DESIGN.md for the one case where that matters). */
int d3m_load_textures(const float* image, const int32_t* is_update, const float* faces_uv, float* textures,
                      int num_faces, int texture_size, int image_height, int image_width, int texture_wrapping,
                      int use_bilinear, d3m_stream_t stream);
/* Learnable uv images: the map image -> cubes of d3m_load_textures as a function of the image, and its adjoint.
 * image [image_batch, H, W, 3] (row 0 = bottom, texture space), faces_uv [F, 3, 2], face_mask [F] i32 (NULL: every
 * face), base [base_batch, F, ts, ts, ts, 3] (base_batch 1 or image_batch; NULL: zeros).  WRITES textures
 * [image_batch, F, ts, ts, ts, 3]: the faces with face_mask != 0 sample view b's image with the arithmetic of
 * d3m_load_textures (the same bits), the others copy base.  D3M_ERR_INVALID: NULL image / faces_uv / textures, a size
 * <= 0, texture_size < 2, image_batch > 65535, texture_wrapping outside 0..3, base_batch neither 1 nor image_batch. */
int d3m_textures_from_image(const float* image, int image_batch, const float* faces_uv, const int32_t* face_mask,
                            const float* base, int base_batch, float* textures, int num_faces, int texture_size,
                            int image_height, int image_width, int texture_wrapping, int use_bilinear, d3m_stream_t stream);
/* The device part of the transpose's build: texel i = f * ts^3 + r writes its taps (4 bilinear, 1 nearest) as entries
 * e = i * taps + j: pixel [F*ts^3*taps] i32 = y * W + x, weight [F*ts^3*taps] f32 -- texture[i][k] = sum over j of
 * image[pixel][k] * weight, accumulated in j order.  Entries that add nothing (zero weight, face_mask[f] == 0,
 * CLAMP_TO_BORDER) get pixel = H * W and weight 0.  A stable sort by pixel gives the CSR d3m_uv_texture_adjoint walks.
 * D3M_ERR_INVALID: NULL faces_uv / pixel / weight, a size <= 0, texture_size < 2, texture_wrapping outside 0..3,
 * F*ts^3*taps or H*W beyond int32. */
int d3m_uv_texture_taps(const float* faces_uv, const int32_t* face_mask, int num_faces, int texture_size, int image_height,
                        int image_width, int texture_wrapping, int use_bilinear, int32_t* pixel, float* weight,
                        d3m_stream_t stream);
/* A gathered CSR with its long-row tables: what every fixed-order adjoint below walks (device arrays of i32, built once by
 * the caller; every index in range: the caller checks).  Row r owns items[offsets[r] .. offsets[r+1]) in the node's item
 * layout.  A row of up to long_row items is summed by its own lane(s) in item order.  A longer row (a hub) is listed in
 * long_rows (ascending) and cut into chunks, item ranges [start, end) i32x2 of at most 1024 items in row order; long row l
 * owns chunks[long_chunk_ptr[l] .. long_chunk_ptr[l+1]).  Each chunk is reduced by one workgroup in a fixed order
 * (csrc/d3m_row_gather.h states it) into the entry point's partials (scratch, plainly stored), and the row adds its chunks'
 * sums in chunk order.
 * Every entry point that takes one returns D3M_ERR_INVALID for: a NULL d3m_csr, NULL offsets, num_rows that is not the row
 * count it walks, a negative count, long_row < 0, long rows without chunks or chunks without long rows, chunks with a NULL
 * items / chunks / long_rows / long_chunk_ptr or without partials. */
typedef struct d3m_csr {
    const int32_t *offsets;         /* [num_rows + 1] */
    const int32_t *items;           /* the node's item layout (adjacency: 3 f + c; uv: (texel, weight bits) pairs) */
    const int32_t *chunks;          /* [num_chunks, 2] or NULL */
    const int32_t *long_rows;       /* [num_long_rows] ascending, or NULL */
    const int32_t *long_chunk_ptr;  /* [num_long_rows + 1] or NULL */
    int num_rows, num_chunks, num_long_rows, long_row;
} d3m_csr;
/* The adjoint (no float atomics, the same bits on every run): WRITES grad_image [batch_size, H, W, 3] from grad_textures
 * [batch_size, num_texels, 3] through the transpose: a d3m_csr of H*W rows whose items [nnz, 2] are (texel, weight's f32
 * bits), each row in ascending texel order (NULL where nnz = 0); partials [batch_size, num_chunks, 3] f32.  The rows that
 * are not long are walked by lanes_per_row (1, 2, 4, 8 or 16) lanes each: lane s sums entries s, s + lanes_per_row, ... and
 * the lanes' sums are combined by a butterfly -- a fixed order for a given lanes_per_row.
 * D3M_ERR_INVALID: what d3m_csr lists, NULL grad_textures / grad_image, a size <= 0, batch_size > 65535, lanes_per_row not a
 * listed value. */
int d3m_uv_texture_adjoint(const d3m_csr* transpose, int lanes_per_row, const float* grad_textures, float* partials,
                           float* grad_image, int batch_size, long num_texels, int image_height, int image_width,
                           d3m_stream_t stream);
/* Learnable per-vertex colours of an indexed mesh: the map colours -> 2x2x2 cubes and its adjoint.
 * colors [color_batch, V, 3], tri [F, 3] i32 (every index in [0, V): the caller checks).  WRITES textures
 * [color_batch, F, 2, 2, 2, 3]: texel idx of face f, channel k, is (C[idx][0] c0 + C[idx][1] c1) + C[idx][2] c2 with
 * cj = colors[b, tri[f][j], k] and C the 8x3 table of vcolor_to_texture_cube (deep3dmap/core/renderer/utils.py:84-94) --
 * the association of d3m_textures_from_im, the same bits on the grid mesh of an image.
 * D3M_ERR_INVALID: NULL colors / tri / textures, a size <= 0, color_batch > 65535. */
int d3m_vertex_color_textures(const float* colors, int color_batch, const int32_t* tri, float* textures, int num_vertices,
                              int num_tri, d3m_stream_t stream);
/* The adjoint (no float atomics, the same bits on every run): WRITES every element of grad_colors [batch_size, V, 3] from
 * grad_textures [batch_size, F, 2, 2, 2, 3] through the faces' adjacency: a d3m_csr of V rows, the one d3m_vertex_gather
 * walks (items [3 F], item = 3 f + c ascending per vertex): the sum, in item order, of each item's term t = sum over idx
 * ascending of C[idx][c] * grad_textures[b, f, idx, k]; a vertex of no face gets 0.  partials [batch_size, num_chunks, 3] f32.
 * D3M_ERR_INVALID: what d3m_csr lists, NULL grad_textures / items / grad_colors, a size <= 0, batch_size > 65535, 3 F beyond
 * int32. */
int d3m_vertex_color_textures_backward(const float* grad_textures, const d3m_csr* adjacency, float* partials,
                                       float* grad_colors, int batch_size, int num_vertices, int num_tri,
                                       d3m_stream_t stream);
/* Shape regularisers of an indexed mesh (no float atomics, the same bits on every run).  The topology of the faces, built
 * once by the caller (neural_renderer/mesh_regularizers.py; every index in range: the caller checks), two d3m_csr of V rows
 * each and the wing records: nbr, the E unique edges as a neighbour CSR (items [2E]: the distinct neighbours of a vertex,
 * ascending; NULL where E = 0); wings [P,4] i32 = (a, b, c, d): an edge a < b and the third vertices c, d of two faces on it;
 * wing, the wing CSR (items [4P]: item = 4 p + role, role 0..3 for a, b, c, d, ascending per vertex).  The vertex count is
 * nbr.num_rows, and wing.num_rows equals it. */
typedef struct d3m_mesh_topology {
    d3m_csr nbr, wing;
    const int32_t* wings;
    int num_edges, num_wings;
} d3m_mesh_topology;
/* Floats of scratch d3m_mesh_regularizer needs for batch_size vertex sets (0 for an invalid argument). */
size_t d3m_mesh_regularizer_scratch_floats(int batch_size, const d3m_mesh_topology* topology);
/* loss[b] = w_laplacian L_lap + w_edge L_edge + w_normal L_nc of vertices [batch_size, V, 3], and its gradient:
 *   L_lap  = (1/V) sum_v |x_v - mean of v's neighbours|^2 (a vertex without neighbours adds 0),
 *   L_edge = (1/E) sum_e (|x_a - x_b| - edge_target)^2 (the gradient of an edge of length 0 is 0),
 *   L_nc   = (1/P) sum_p (1 - cos(n0, n1)), n0 = (b-a) x (c-a), n1 = -(b-a) x (d-a) (a record with a zero normal adds 0).
 * A term of weight 0 is not evaluated; a term whose count (E, P) is 0 is 0.  WRITES loss_out [batch_size] and every element
 * of grad_vertices [batch_size, V, 3] (times grad_scale[b], a device array of batch_size floats; NULL: 1); with
 * accumulate != 0 both are ADDED to what is there.  grad_vertices NULL: the value only.  scratch: 16-byte aligned,
 * scratch_floats >= d3m_mesh_regularizer_scratch_floats().  At most 3 launches (k_mesh_reg_delta, k_mesh_reg_rows,
 * k_mesh_reg_finish), 2 more on a mesh with long rows (k_mesh_reg_mean_chunks, k_mesh_reg_row_chunks).
 * D3M_ERR_INVALID, before any launch: what d3m_csr lists of either CSR (V = nbr.num_rows rows; the partials are in scratch),
 * NULL vertices / topology / loss_out / scratch / items or wings that the enabled terms read, E or P < 0, batch_size outside
 * [1, 65535], a negative (or NaN) weight or edge_target, 2E or 4P beyond int32, a scratch that is too small or misaligned. */
int d3m_mesh_regularizer(const float* vertices, int batch_size, const d3m_mesh_topology* topology, float w_laplacian,
                         float w_edge, float edge_target, float w_normal, float* scratch, size_t scratch_floats,
                         const float* grad_scale, float* loss_out, float* grad_vertices, int accumulate,
                         d3m_stream_t stream);
/* The vertices of a linear morphable model and the adjoint of that map (no float atomics, the same bits on every run; f32
 * VALU with explicit fused multiply-adds).  basis [num_rows, num_components] row-major (num_rows = 3 V from Python),
 * coeffs [batch_size, num_components]; mean [num_rows] and scale [num_components] may be NULL (0 and 1).
 * WRITES every element of out [batch_size, num_rows]:  out[b, r] = mean[r] + sum_k basis[r, k] * (scale[k] * coeffs[b, k]).
 * One launch (k_morphable_forward); the basis is read once per 16 coefficient sets, with 16-byte loads when
 * num_components % 4 == 0 and basis is 16-byte aligned.  The sum: a row's components in runs of 64, wave w of the workgroup
 * adding components 16 w .. 16 w + 15 of every run in ascending order, then the four waves' sums in wave order, then mean.
 * D3M_ERR_INVALID, before any launch: NULL basis / coeffs / out, a pointer that is not 4-byte aligned, batch_size outside
 * [1, 4096], num_components outside [1, 1024], num_rows < 1, num_rows * num_components >= 2^31. */
int d3m_morphable_forward(const float* basis, const float* coeffs, const float* mean, const float* scale, float* out,
                          int batch_size, int num_rows, int num_components, d3m_stream_t stream);
/* Floats of scratch d3m_morphable_backward needs: ceil(num_rows / 256) * batch_size * num_components (0 for sizes the
 * entry points refuse). */
size_t d3m_morphable_scratch_floats(int batch_size, int num_rows, int num_components);
/* grad_coeffs[b, k] = grad_scale[b] * (scale[k] * sum_r basis[r, k] * grad_out[b, r]), grad_out [batch_size, num_rows];
 * scale and grad_scale (device arrays) may be NULL (1).  WRITES every element of grad_coeffs [batch_size, num_components];
 * with accumulate != 0 ADDS to what is there.  Two launches.  k_morphable_adjoint_chunks: a workgroup per chunk of 256
 * consecutive rows and 64 components, a lane per component; wave w adds rows 64 w .. 64 w + 63 of the chunk in ascending
 * order, the four waves' sums are added in wave order and stored with plain stores in scratch [chunks, batch_size,
 * num_components].  k_morphable_adjoint_finish: 16 groups of ceil(chunks / 16) consecutive chunks each, added in ascending
 * order, then the groups' sums in group order.  The basis is read once per 16 sets.  scratch: 16-byte aligned,
 * scratch_floats >= d3m_morphable_scratch_floats().
 * D3M_ERR_INVALID, before any launch: NULL basis / grad_out / grad_coeffs / scratch, a pointer that is not 4-byte aligned
 * (scratch: 16), the sizes d3m_morphable_forward refuses, a scratch that is too small. */
int d3m_morphable_backward(const float* basis, const float* grad_out, const float* scale, const float* grad_scale,
                           float* scratch, size_t scratch_floats, float* grad_coeffs, int batch_size, int num_rows,
                           int num_components, int accumulate, d3m_stream_t stream);
/* The weak-perspective pose of a point set, and its adjoint (no float atomics, the same bits on every run; plain f32).
 * vertices [vertices_batch, num_vertices, 3] with vertices_batch 1 (shared by all sets) or batch_size; pose: batch_size rows
 * of 7 floats (s, three angles, t), pose_stride floats apart (>= 7; read in place).  With a = clamp(angles, -angle_limit,
 * +angle_limit) (angle_limit <= 0: no clamp) and R = Rx(a0) Ry(a1) Rz(a2):
 *   posed[b, v] = s_b (R_b x[v]) + translation_scale t_b                           [batch_size, num_vertices, 3]
 *   uv[b, v]    = (posed_x / uv_size, 1 - posed_y / uv_size)                        [batch_size, num_vertices, 2]
 *   landmark_points[b, l] = posed[b, landmarks[l]]                                  [batch_size, num_landmarks, 3]
 * Each of the three outputs may be NULL (not computed), not all three; with only landmark_points the launch is
 * O(batch_size * num_landmarks).  landmarks: int32 indices in [0, num_vertices) -- NOT checked here -- and may repeat.
 * One launch (k_pose_forward); R_b is computed once per workgroup.
 * D3M_ERR_INVALID, before any launch: NULL vertices / pose, all outputs NULL, uv with uv_size <= 0, landmark_points with
 * num_landmarks 0, num_landmarks outside [0, 1024] or > 0 with NULL landmarks, batch_size outside [1, 4096], num_vertices
 * < 1, batch_size * num_vertices * 3 >= 2^31, vertices_batch neither 1 nor batch_size, pose_stride < 7, a pointer that is
 * not 4-byte aligned. */
int d3m_pose_forward(const float* vertices, int vertices_batch, const float* pose, int pose_stride, float translation_scale,
                     float angle_limit, float uv_size, const int32_t* landmarks, int num_landmarks, float* posed, float* uv,
                     float* landmark_points, int batch_size, int num_vertices, d3m_stream_t stream);
/* The constants that fix d3m_pose_backward's summation tree: out4 = (vertices per chunk, the cap of parts per set, sets per
 * finish workgroup, sums per set). */
void d3m_pose_tree_constants(int* out4);
/* Floats of scratch d3m_pose_backward needs: batch_size * min(ceil(num_vertices / 256), 64) * 12 (0 for sizes the entry
 * points refuse). */
size_t d3m_pose_scratch_floats(int batch_size, int num_vertices);
/* The adjoint of d3m_pose_forward.  grad_posed / grad_uv / grad_landmark_points (shapes of the outputs) may each be NULL
 * (zeros); G[b, v] = grad_posed + (grad_uv.x / uv_size, -grad_uv.y / uv_size, 0) + the landmark gradients pointing at v.
 * WRITES every element of grad_vertices [vertices_batch, num_vertices, 3] = s_b R_b^T G[b, v] (vertices_batch 1: summed over
 * the sets in ascending order) and of grad_pose [batch_size, 7] (dense) = (<M_b, R_b>, s_b <M_b, dR_b/da_k> where
 * -angle_limit <= angle_k <= angle_limit and 0 elsewhere, translation_scale n_b) with M_b = sum_v G (x) x, n_b = sum_v G;
 * either may be NULL (not computed), not both.  At most two launches.  k_pose_backward_chunks: workgroup p of a set's
 * min(ceil(num_vertices / 256), 64) takes the vertices 256 p + lane, + 256 parts, ... in ascending order per lane, adds the
 * lanes of a wave, then the four waves in order, and stores one partial per (set, p) in scratch; it writes grad_vertices
 * from the same read.  k_pose_backward_finish: a lane per set adds the partials in ascending p, then the landmark terms in
 * ascending l, and applies the Euler adjoint; the landmark gradients are added to grad_vertices by one lane per (set,
 * coordinate) walking l in ascending order (vertices_batch 1: summed over the sets in ascending order first).
 * scratch_floats >= d3m_pose_scratch_floats() when grad_pose is given together with grad_posed or grad_uv.
 * D3M_ERR_INVALID, before any launch: what d3m_pose_forward refuses of the inputs, grad_uv with uv_size <= 0,
 * grad_landmark_points with num_landmarks 0, both outputs NULL, a scratch that is needed and NULL or too small. */
int d3m_pose_backward(const float* vertices, int vertices_batch, const float* pose, int pose_stride, float translation_scale,
                      float angle_limit, float uv_size, const int32_t* landmarks, int num_landmarks, const float* grad_posed,
                      const float* grad_uv, const float* grad_landmark_points, float* scratch, size_t scratch_floats,
                      float* grad_vertices, float* grad_pose, int batch_size, int num_vertices, d3m_stream_t stream);
/* Smooth per-vertex normals of an indexed mesh and a 9-term spherical-harmonic light on per-vertex albedo, with the adjoint
 * (no float atomics, the same bits on every run; plain f32; csrc/d3m_smooth_shade.h states the order of every sum).
 * vertices [vertices_batch, V, 3], colors [colors_batch, V, 3], sh [sh_batch, 3, 9]: each batch is 1 (shared by all sets) or
 * batch_size.  tri [F, 3] i32 and the adjacency (a d3m_csr of V rows, item = 3 f + c) are those of
 * d3m_vertex_color_textures_backward (every index in range: the caller checks); the partials are in scratch.
 *   N_f = (x1 - x0) x (x2 - x0);  s[b,v] = the sum of N_f over v's items in ascending order;  r = |s|;  n = s / max(r, 1e-6)
 *   H(n) = (a0, a1 nx, a1 ny, a1 nz, a2 (2 nz^2 - nx^2 - ny^2), a3 ny nz, a3 nx nz, a3 nx ny, a4 (nx^2 - ny^2)) with
 *   a0 = sqrt(1/4pi), a1 = sqrt(3/4pi), a2 = a1 / 2, a3 = 3 sqrt(5/12pi), a4 = a3 / 2
 *   shaded[b,v,k] = colors[b,v,k] * sum_j sh[b,k,j] H_j(n[b,v])
 * WRITES every element of normals [vertices_batch, V, 3] (a vertex of no face: 0), lengths [vertices_batch, V] (r) and shaded
 * [batch_size, V, 3].  colors NULL: the normals only (shaded NULL, batch_size == vertices_batch; sh is not read).  At most
 * three launches (k_smooth_shade_face_normals, k_smooth_shade_normal_chunks on a mesh with long rows, k_smooth_shade_vertices).
 * scratch_floats >= d3m_smooth_shade_scratch_floats().
 * D3M_ERR_INVALID, before any launch: what d3m_csr lists, NULL vertices / tri / items / scratch / normals / lengths, colors
 * without sh or shaded, shaded without colors, batch_size outside [1, 65535], a batch that is neither 1 nor batch_size, a
 * size <= 0, 3 F beyond int32, batch_size * V * 3 >= 2^31, a scratch that is too small, a pointer that is not 4-byte
 * aligned. */
int d3m_smooth_shade_forward(const float* vertices, int vertices_batch, const float* colors, int colors_batch,
                             const float* sh, int sh_batch, const int32_t* tri, const d3m_csr* adjacency, float* scratch,
                             size_t scratch_floats, float* shaded, float* normals, float* lengths, int batch_size,
                             int num_vertices, int num_tri, d3m_stream_t stream);
/* Floats of scratch the two entry points need (0 for sizes they refuse): vertices_batch * (3 V + 9 F + 3 num_chunks) +
 * batch_size * min(ceil(V / 256), 64) * 27. */
size_t d3m_smooth_shade_scratch_floats(int batch_size, int vertices_batch, int num_vertices, int num_tri, int num_chunks);
/* The adjoint of d3m_smooth_shade_forward, from its inputs and its outputs normals and lengths.  grad_shaded [batch_size, V,
 * 3] and grad_normals [vertices_batch, V, 3] may each be NULL (zeros).  WRITES every element of grad_vertices
 * [vertices_batch, V, 3], grad_colors [colors_batch, V, 3] and grad_sh [sh_batch, 3, 9]; each may be NULL (not computed), not
 * all three; the gradient of a shared input is summed over the sets in ascending order.  grad_colors and grad_sh need
 * grad_shaded.  At most five launches (k_smooth_shade_backward_vertices, k_smooth_shade_backward_finish for grad_sh, and for
 * grad_vertices k_smooth_shade_backward_faces, k_smooth_shade_term_chunks on a mesh with long rows, k_smooth_shade_backward_rows).
 * D3M_ERR_INVALID, before any launch: what d3m_smooth_shade_forward refuses of the inputs, NULL normals / lengths, all three
 * outputs NULL, grad_colors or grad_sh without grad_shaded, grad_shaded without colors. */
int d3m_smooth_shade_backward(const float* vertices, int vertices_batch, const float* colors, int colors_batch,
                              const float* sh, int sh_batch, const float* normals, const float* lengths,
                              const float* grad_shaded, const float* grad_normals, const int32_t* tri,
                              const d3m_csr* adjacency, float* scratch, size_t scratch_floats, float* grad_vertices,
                              float* grad_colors, float* grad_sh, int batch_size, int num_vertices, int num_tri,
                              d3m_stream_t stream);
/* Per-vertex attribute images (an addition; csrc/d3m_attributes.h states the semantics and the order of every sum): C
 * channels of per-vertex data interpolated over a COVERAGE RECORD with the sampler's perspective-correct weights.  The record
 * is what d3m_forward_face_index_map_mesh left for batch_size views of ONE shared topology at the raster size S = image_size
 * (anti_aliasing == 0) or 2 image_size: face_index_map [B,S,S] (every entry in [-1, F'), F' = (fill_back ? 2 : 1) num_tri),
 * weight_map [B,S,S,3], depth_map [B,S,S], faces [B,F',3,3] (the dense copy: only owners' entries are read), tri [num_tri,3]
 * i32 (every index in [0, num_vertices): the caller checks, where it builds the adjacency), and the visibility blob that
 * d3m_visibility finished (visibility_size >= d3m_visibility_bytes(B, F'); read by the adjoint only, may be NULL forward). */
typedef struct d3m_fragments {
    const int32_t* face_index_map;
    const float* weight_map;
    const float* depth_map;
    const float* faces;
    const int32_t* tri;
    const void* visibility;
    size_t visibility_size;
    int batch_size, num_tri, fill_back, image_size, anti_aliasing;
} d3m_fragments;
/* attributes [attributes_batch, V, C] f32, attributes_batch 1 (shared by the views) or B; background [C] or NULL (zeros).
 * WRITES every element of images [B, C, image_size, image_size] and alpha [B, image_size, image_size] (rows top to bottom;
 * with anti-aliasing the mean of the 2x2 internal pixels, background included).  One launch (k_vertex_attribute_images).
 * D3M_ERR_INVALID, before any launch: a NULL record or a NULL map / faces / tri in it, NULL attributes / images / alpha,
 * batch_size not in [1, 65535], num_tri or image_size <= 0, image_size beyond 16384, B F' beyond 2^31 - 1, attributes_batch
 * neither 1 nor B, num_vertices <= 0, num_channels not in [1, 1024]. */
int d3m_vertex_attribute_images(const d3m_fragments* fragments, const float* attributes, int attributes_batch,
                                int num_vertices, int num_channels, const float* background, float* images, float* alpha,
                                d3m_stream_t stream);
/* Floats of scratch the adjoint needs: B F' 3 C per-face sums and B num_chunks C chunk sums of the adjacency's long rows
 * (0 for sizes the adjoint refuses). */
size_t d3m_vertex_attribute_scratch_floats(int batch_size, int num_faces, int num_channels, const d3m_csr* adjacency);
/* The adjoint with respect to the attributes: grad_images [B, C, image_size, image_size] -> grad_attributes
 * [attributes_batch, V, C], every element WRITTEN (a vertex of no visible face gets +0; shared attributes: summed over the
 * views in ascending order).  adjacency: the faces' d3m_csr of V rows (item = 3 f + c).  scratch needs no initialisation.  No
 * float atomics, nothing cleared; three launches (k_vertex_attribute_face_sums, k_vertex_attribute_large_face_sums,
 * k_vertex_attribute_adjoint_rows) and k_vertex_attribute_adjoint_chunks on a mesh with long rows.
 * D3M_ERR_INVALID, before any launch: what d3m_vertex_attribute_images refuses of the record and the sizes, a NULL or too
 * small visibility blob, what d3m_csr lists (num_rows = num_vertices), NULL items / grad_images / scratch / grad_attributes,
 * 3 num_tri beyond 2^31 - 1; D3M_ERR_WORKSPACE: scratch_floats below d3m_vertex_attribute_scratch_floats(). */
int d3m_vertex_attribute_images_backward(const d3m_fragments* fragments, const float* grad_images,
                                         const d3m_csr* adjacency, float* scratch, size_t scratch_floats,
                                         float* grad_attributes, int attributes_batch, int num_vertices, int num_channels,
                                         d3m_stream_t stream);
/* Per-pixel uv texture images (an addition; csrc/d3m_uv_texture.h states the semantics): image [image_batch, H, W, C] f32
 * (channels last; image_batch 1 -- shared by the views -- or B) looked up bilinearly at the interpolated uv of every pixel of
 * a coverage record; faces_uv [num_tri, 3, 2] f32 is the per-corner uv of d3m_load_textures, wrapped per corner with
 * texture_wrapping 0 REPEAT, 1 MIRRORED_REPEAT or 2 CLAMP_TO_EDGE; background [C] or NULL (zeros).  WRITES every element of
 * images [B, C, image_size, image_size] and alpha [B, image_size, image_size] (alpha: the bits of
 * d3m_vertex_attribute_images').  One launch (k_uv_texture_images).
 * D3M_ERR_INVALID, before any launch: what d3m_vertex_attribute_images refuses of the record, a NULL or misaligned faces_uv /
 * image / images / alpha, image_batch neither 1 nor B, H or W not in [1, 32768], C not in [1, 64], texture_wrapping 3
 * (CLAMP_TO_BORDER) or outside 0..2. */
int d3m_uv_texture_images(const d3m_fragments* fragments, const float* faces_uv, const float* image, int image_batch,
                          int image_height, int image_width, int num_channels, int texture_wrapping,
                          const float* background, float* images, float* alpha, d3m_stream_t stream);
/* Bytes of scratch the adjoint needs for a record of batch_size views at the raster size S: image_batch H W C int64
 * accumulators and 1024 block maxima.  0 for sizes the adjoint refuses, batch_size S S beyond 2^32 among them. */
size_t d3m_uv_texture_images_scratch_bytes(int image_batch, int image_height, int image_width, int num_channels,
                                           int batch_size, int raster_size);
/* The adjoint with respect to the image: grad_images [B, C, image_size, image_size] -> grad_image [image_batch, H, W, C],
 * every element WRITTEN, the same bits whatever the order of arrival: each term is rounded to a multiple of the quantum
 * 2^(ilogb(max |scale g|) + 1 - frac), frac = 62 - ceil(log2(B S S)), and added to an int64 accumulator with an integer
 * atomic; no float atomics, nothing read back.  A texel no sample reaches, and every texel when grad_images is all zeros,
 * gets +0; an Inf or NaN anywhere in grad_images makes every element NaN (no error status).  scratch (8-byte aligned) needs no
 * initialisation.  Three launches (k_uv_texture_images_clear_max, k_uv_texture_images_scatter, k_uv_texture_images_convert).
 * D3M_ERR_INVALID, before any launch: what d3m_uv_texture_images refuses, NULL grad_images / scratch / grad_image, a
 * misaligned scratch, B S S beyond 2^32; D3M_ERR_WORKSPACE: scratch_bytes below d3m_uv_texture_images_scratch_bytes(). */
int d3m_uv_texture_images_backward(const d3m_fragments* fragments, const float* faces_uv, const float* grad_images,
                                   int image_batch, int image_height, int image_width, int num_channels,
                                   int texture_wrapping, void* scratch, size_t scratch_bytes, float* grad_image,
                                   d3m_stream_t stream);
/* Mip-mapped per-pixel uv texture images (an addition; csrc/d3m_uv_texture_mip.h states the semantics).  `levels` = L, the
 * number of levels above level 0, 1 <= L <= 15, image_height and image_width divisible by 2^L; T = sum over l = 0..L of
 * (H >> l)(W >> l) texels per image.
 * d3m_texture_mip_pyramid WRITES every element of pyramid [image_batch, T, C]: level 0 is the image, a texel of level l + 1 is
 * (((a00 + a01) + a10) + a11) * 0.25 of its four children.  One launch (k_texture_mip_tile), two when L > 5
 * (k_texture_mip_tail).  D3M_ERR_INVALID, before any launch: a NULL or misaligned image / pyramid, image_batch not in
 * [1, 65535], H or W not in [1, 32768] or not divisible by 2^L, C not in [1, 64], L not in [1, 15]. */
int d3m_texture_mip_pyramid(const float* image, int image_batch, int image_height, int image_width, int num_channels,
                            int levels, float* pyramid, d3m_stream_t stream);
/* The level of detail lambda_c of every internal pixel of the record, lod [B, S, S] in map orientation (S the raster size), 0
 * where uncovered; every element WRITTEN.  One launch (k_uv_texture_lod).  D3M_ERR_INVALID, before any launch: what
 * d3m_uv_texture_images refuses of the record, faces_uv, the sizes and the wrapping, what d3m_texture_mip_pyramid refuses of
 * H, W and L, a lod_bias that is not finite, a NULL or misaligned lod. */
int d3m_uv_texture_lod(const d3m_fragments* fragments, const float* faces_uv, int image_height, int image_width,
                       int texture_wrapping, int levels, float lod_bias, float* lod, d3m_stream_t stream);
/* d3m_uv_texture_images with a trilinear lookup in `pyramid` (d3m_texture_mip_pyramid's, [image_batch, T, C]) at the level
 * lambda_c.  WRITES every element of images and alpha.  One launch (k_uv_texture_mip_images).  D3M_ERR_INVALID, before any
 * launch: what d3m_uv_texture_images and d3m_uv_texture_lod refuse. */
int d3m_uv_texture_mip_images(const d3m_fragments* fragments, const float* faces_uv, const float* pyramid, int image_batch,
                              int image_height, int image_width, int num_channels, int texture_wrapping, int levels,
                              float lod_bias, const float* background, float* images, float* alpha, d3m_stream_t stream);
/* Bytes of scratch the mip-mapped adjoint needs: image_batch T C int64 accumulators (one per element of every level) and
 * 1024 block maxima.  0 for sizes the adjoint refuses. */
size_t d3m_uv_texture_mip_images_scratch_bytes(int image_batch, int image_height, int image_width, int num_channels,
                                               int levels, int batch_size, int raster_size);
/* The adjoint with respect to the image (level 0): grad_images -> grad_image [image_batch, H, W, C], every element WRITTEN,
 * the same bits whatever the order of arrival: d3m_uv_texture_images_backward's number format with accumulators on every
 * level; the conversion gathers an element's accumulator and its ancestors' in level order, in double.  The pyramid is not
 * read.  Three launches (k_uv_texture_images_clear_max, k_uv_texture_mip_images_scatter, k_uv_texture_mip_images_convert).
 * D3M_ERR_INVALID, before any launch: what d3m_uv_texture_mip_images refuses, NULL grad_images / scratch / grad_image, a
 * misaligned scratch, B S S beyond 2^32, scratch_bytes below d3m_uv_texture_mip_images_scratch_bytes(). */
int d3m_uv_texture_mip_images_backward(const d3m_fragments* fragments, const float* faces_uv, const float* grad_images,
                                       int image_batch, int image_height, int image_width, int num_channels,
                                       int texture_wrapping, int levels, float lod_bias, void* scratch, size_t scratch_bytes,
                                       float* grad_image, d3m_stream_t stream);
/* The interior geometry gradient of what is drawn over a coverage record (an addition; csrc/d3m_fragment_geometry.h states the
 * function that is differentiated and the order of every sum): the derivative of the perspective-correct weights u_c of every
 * owned pixel with respect to the owner's three screen-space corners.  Coverage is a constant; the silhouette gradient is the
 * render nodes'.  The record must be the one d3m_forward_face_index_map_mesh made from the vertices the gradient is for.
 * d3m_fragment_weights WRITES every element of weights [B, S, S, 3] (S the raster size, map orientation): u_c =
 * weight_map * (depth_map / z_c), +0 where uncovered.  One launch (k_fragment_weights).  D3M_ERR_INVALID, before any launch:
 * what d3m_vertex_attribute_images refuses of the record, B S S beyond 2^32, a NULL or misaligned weights. */
int d3m_fragment_weights(const d3m_fragments* fragments, float* weights, d3m_stream_t stream);
/* Floats of scratch of d3m_fragment_geometry_backward: B F' 9 per-face sums and 3 B num_chunks chunk sums of the adjacency's
 * long rows; with_pixel_grads != 0: and 3 B S S more, room for a pixel_grads map (raster_size = S).  0 for sizes that are
 * refused. */
size_t d3m_fragment_geometry_scratch_floats(int batch_size, int num_faces, int raster_size, const d3m_csr* adjacency,
                                            int with_pixel_grads);
/* pixel_grads [B, S, S, 3] = dL/du_c of the attribute images for the image gradient grad_images [B, C, image_size,
 * image_size]: h_c = sum_k scale g[k] a_c[k], every element WRITTEN (+0 where uncovered).  One launch
 * (k_vertex_attribute_pixel_grads).  D3M_ERR_INVALID, before any launch: what d3m_vertex_attribute_images refuses of the
 * record, the attributes and the sizes, B S S beyond 2^32, NULL grad_images / pixel_grads. */
int d3m_vertex_attribute_pixel_grads(const d3m_fragments* fragments, const float* attributes, int attributes_batch,
                                     int num_vertices, int num_channels, const float* grad_images, float* pixel_grads,
                                     d3m_stream_t stream);
/* pixel_grads [B, S, S, 3] = dL/du_c of the plain bilinear uv texture images (d3m_uv_texture_images; not the mip-mapped
 * lookup, whose level of detail depends on the geometry): h_c = (W - 1) uv_c.x Dx + (H - 1) uv_c.y Dy, Dx / Dy the image
 * gradient's derivative along the lookup position from the four taps, 0 where that axis sits at a clamp limit.  faces_uv is a
 * constant.  Every element WRITTEN.  One launch (k_uv_texture_pixel_grads).  D3M_ERR_INVALID, before any launch: what
 * d3m_uv_texture_images refuses of the record, faces_uv, the image and the sizes, B S S beyond 2^32, a NULL or misaligned
 * grad_images / pixel_grads. */
int d3m_uv_texture_pixel_grads(const d3m_fragments* fragments, const float* faces_uv, const float* image, int image_batch,
                               int image_height, int image_width, int num_channels, int texture_wrapping,
                               const float* grad_images, float* pixel_grads, d3m_stream_t stream);
/* The shared adjoint: pixel_grads [B, S, S, 3] (read at owned pixels only) -> grad_screen_vertices [B, V, 3], every element
 * WRITTEN (a vertex of no visible face gets +0).  adjacency: the faces' d3m_csr of V rows (item = 3 f + c).  scratch needs no
 * initialisation.  No float atomics, nothing cleared; three launches (k_fragment_geometry_face_sums,
 * k_fragment_geometry_large_face_sums, k_vertex_attribute_adjoint_rows) and k_vertex_attribute_adjoint_chunks on a mesh with
 * long rows.  D3M_ERR_INVALID, before any launch: what d3m_fragment_weights refuses of the record, num_vertices <= 0, a NULL
 * or too small visibility blob, what d3m_csr lists (num_rows = num_vertices), NULL items, a NULL or misaligned pixel_grads /
 * scratch / grad_screen_vertices, 3 num_tri beyond 2^31 - 1; D3M_ERR_WORKSPACE: scratch_floats below
 * d3m_fragment_geometry_scratch_floats(..., 0). */
int d3m_fragment_geometry_backward(const d3m_fragments* fragments, const float* pixel_grads, const d3m_csr* adjacency,
                                   float* scratch, size_t scratch_floats, float* grad_screen_vertices, int num_vertices,
                                   d3m_stream_t stream);
/* Per-pixel spherical-harmonic shading over a coverage record (an addition; csrc/d3m_sh_fragments.h states the function and
 * the order of every sum): normals [normals_batch, V, 3] and, optionally, colors [colors_batch, V, 3] (NULL: none) are
 * interpolated at every pixel with the weights of d3m_vertex_attribute_images, the normal is normalised per pixel (m / max(|m|,
 * 1e-6)) and lit by sh [sh_batch, 3, 9] (channel, basis term; the basis of d3m_smooth_shade_forward): value_k = a_k sum_j
 * sh[k,j] H_j(n).  Each batch is 1 (shared by the views) or B.  background [3] or NULL (zeros).  WRITES every element of images
 * [B, 3, image_size, image_size] and alpha [B, image_size, image_size] (alpha: the bits of d3m_vertex_attribute_images').  One
 * launch (k_sh_fragment_images).  D3M_ERR_INVALID, before any launch: what d3m_vertex_attribute_images refuses of the record,
 * B S S beyond 2^32, NULL or misaligned normals / sh / images / alpha, misaligned colors / background, a batch neither 1 nor B,
 * num_vertices <= 0. */
int d3m_sh_fragment_images(const d3m_fragments* fragments, const float* normals, int normals_batch, const float* sh,
                           int sh_batch, const float* colors, int colors_batch, int num_vertices, const float* background,
                           float* images, float* alpha, d3m_stream_t stream);
/* Floats of scratch of d3m_sh_fragment_images_backward, with C = 6 (with_colors != 0) or 3 and S = raster_size:
 * d3m_vertex_attribute_scratch_floats(batch_size, num_faces, C, adjacency), then the gradient image B C S S, then the light's
 * partial sums B * min(ceil(S S / 1024), 256) * 27.  0 for sizes that are refused. */
size_t d3m_sh_fragment_scratch_floats(int batch_size, int num_faces, int raster_size, int with_colors,
                                      const d3m_csr* adjacency);
/* The adjoint: grad_images [B, 3, image_size, image_size] -> grad_sh [sh_batch, 3, 9], grad_vertex and pixel_grads [B, S, S, 3]
 * (d3m_sh_fragment_pixel_grads' map, written by the same per-pixel launch); each may be NULL (not computed), not all three;
 * every element of what is given is WRITTEN, the gradient of a shared input summed over the views in ascending order.
 * vertex_grads says what grad_vertex holds: 0 nothing (grad_vertex NULL), 1 the normals' gradient [normals_batch, V, 3], 2 the
 * colours' [colors_batch, V, 3], 3 both: with colors of the normals' batch [normals_batch, V, 6] (normals in channels 0..2,
 * colours in 3..5: one gather), with colors of another batch [normals_batch, V, 3] followed by [colors_batch, V, 3] (two
 * gathers).  scratch needs no initialisation.  No float atomics, nothing cleared.  Launches: k_sh_fragment_backward_pixels;
 * k_sh_fragment_finish for grad_sh; per gather k_vertex_attribute_face_sums, k_vertex_attribute_large_face_sums,
 * k_vertex_attribute_adjoint_rows, and k_vertex_attribute_adjoint_chunks on a mesh with long rows.  D3M_ERR_INVALID, before any
 * launch: what d3m_sh_fragment_images refuses of the record and the inputs, a NULL or too small visibility blob, what d3m_csr
 * lists (num_rows = num_vertices), NULL items, a NULL or misaligned grad_images / scratch, all three results NULL, a misaligned
 * result, vertex_grads outside 0..3, 0 with a grad_vertex or not 0 without, the colours' bit without colors, 3 num_tri beyond
 * 2^31 - 1; D3M_ERR_WORKSPACE: scratch_floats below d3m_sh_fragment_scratch_floats(). */
int d3m_sh_fragment_images_backward(const d3m_fragments* fragments, const float* normals, int normals_batch, const float* sh,
                                    int sh_batch, const float* colors, int colors_batch, int num_vertices,
                                    const float* grad_images, const d3m_csr* adjacency, float* scratch, size_t scratch_floats,
                                    float* grad_vertex, int vertex_grads, float* grad_sh, float* pixel_grads,
                                    d3m_stream_t stream);
/* pixel_grads [B, S, S, 3] = dL/du_c of the shaded images for d3m_fragment_geometry_backward: h_c = dL/dm . n_c + dL/da . c_c,
 * every element WRITTEN (+0 where uncovered) -- for a caller who wants nothing else of the adjoint.  One launch
 * (k_sh_fragment_backward_pixels).  D3M_ERR_INVALID, before any launch:
 * what d3m_sh_fragment_images refuses of the record and the inputs, a NULL or misaligned grad_images / pixel_grads. */
int d3m_sh_fragment_pixel_grads(const d3m_fragments* fragments, const float* normals, int normals_batch, const float* sh,
                                int sh_batch, const float* colors, int colors_batch, int num_vertices,
                                const float* grad_images, float* pixel_grads, d3m_stream_t stream);
/* Per-pixel spherical-harmonic shading of a UV albedo texture over a coverage record (an addition;
 * csrc/d3m_sh_uv_fragments.h states the function and the order of every sum): image [image_batch, H, W, 3] is looked up at
 * every internal pixel as d3m_uv_texture_images looks it up (faces_uv [num_tri, 3, 2], wrapped per corner by texture_wrapping:
 * REPEAT, MIRRORED_REPEAT or CLAMP_TO_EDGE) and multiplied THERE, before the pooling of a supersampled record, with the light
 * of d3m_sh_fragment_images (normals [normals_batch, V, 3], sh [sh_batch, 3, 9], no per-vertex colours): value_k = a_k sum_j
 * sh[k,j] H_j(n).  Each batch is 1 (shared by the views) or B.  background [3] or NULL (zeros).  WRITES every element of images
 * [B, 3, image_size, image_size] and alpha [B, image_size, image_size] (alpha: the bits of d3m_vertex_attribute_images').  One
 * launch (k_sh_uv_fragment_images).  D3M_ERR_INVALID, before any launch: what d3m_sh_fragment_images refuses of the record,
 * normals, sh and num_vertices; what d3m_uv_texture_images refuses of faces_uv, the image's sizes and batch (with three
 * channels) and the wrapping; a NULL or misaligned image / images / alpha, a misaligned background. */
int d3m_sh_uv_fragment_images(const d3m_fragments* fragments, const float* normals, int normals_batch, const float* sh,
                              int sh_batch, int num_vertices, const float* faces_uv, const float* image, int image_batch,
                              int image_height, int image_width, int texture_wrapping, const float* background, float* images,
                              float* alpha, d3m_stream_t stream);
/* Bytes of scratch of d3m_sh_uv_fragment_images_backward, with S = raster_size: d3m_uv_texture_images_scratch_bytes(image_batch,
 * H, W, 3, batch_size, S) rounded up to 8, then floats: d3m_vertex_attribute_scratch_floats(batch_size, num_faces, 3,
 * adjacency), the two gradient images 2 B 3 S S, the light's partial sums B * min(ceil(S S / 1024), 256) * 27.  0 for sizes
 * that are refused. */
size_t d3m_sh_uv_fragment_scratch_bytes(int batch_size, int num_faces, int raster_size, int image_batch, int image_height,
                                        int image_width, const d3m_csr* adjacency);
/* The adjoint: grad_images [B, 3, image_size, image_size] -> grad_normals [normals_batch, V, 3], grad_sh [sh_batch, 3, 9],
 * grad_image [image_batch, H, W, 3] and pixel_grads [B, S, S, 3] (d3m_sh_uv_fragment_pixel_grads' map, written by the same
 * per-pixel launch); each may be NULL (not computed), not all four; every element of what is given is WRITTEN, the gradient of
 * a shared input summed over the views (normals, sh: in ascending order; the image: in 64-bit fixed point, independent of
 * order, with d3m_uv_texture_images_backward's rules for a zero, an Inf or a NaN gradient and an untouched texel).  scratch (8-byte
 * aligned) needs no initialisation.  No float atomics.  Launches: k_sh_uv_fragment_backward_pixels; k_sh_fragment_finish for
 * grad_sh; for grad_image k_uv_texture_images_clear_max, k_uv_texture_images_scatter, k_uv_texture_images_convert; for
 * grad_normals k_vertex_attribute_face_sums, k_vertex_attribute_large_face_sums, k_vertex_attribute_adjoint_rows, and
 * k_vertex_attribute_adjoint_chunks on a mesh with long rows.  D3M_ERR_INVALID, before any launch: what
 * d3m_sh_uv_fragment_images refuses of the record and the inputs, a NULL or too small visibility blob, what d3m_csr lists
 * (num_rows = num_vertices), NULL items, a NULL or misaligned grad_images / scratch, all four results NULL, a misaligned
 * result, 3 num_tri beyond 2^31 - 1; D3M_ERR_WORKSPACE: scratch_bytes below d3m_sh_uv_fragment_scratch_bytes(). */
int d3m_sh_uv_fragment_images_backward(const d3m_fragments* fragments, const float* normals, int normals_batch, const float* sh,
                                       int sh_batch, int num_vertices, const float* faces_uv, const float* image,
                                       int image_batch, int image_height, int image_width, int texture_wrapping,
                                       const float* grad_images, const d3m_csr* adjacency, void* scratch, size_t scratch_bytes,
                                       float* grad_normals, float* grad_sh, float* grad_image, float* pixel_grads,
                                       d3m_stream_t stream);
/* pixel_grads [B, S, S, 3] = dL/du_c of the shaded images for d3m_fragment_geometry_backward: h_c = dL/dm . n_c + the lookup's
 * slopes along pos times the corner's wrapped uv, every element WRITTEN (+0 where uncovered) -- for a caller who wants nothing
 * else of the adjoint.  One launch (k_sh_uv_fragment_backward_pixels).  D3M_ERR_INVALID, before any launch: what
 * d3m_sh_uv_fragment_images refuses of the record and the inputs, a NULL or misaligned grad_images / pixel_grads. */
int d3m_sh_uv_fragment_pixel_grads(const d3m_fragments* fragments, const float* normals, int normals_batch, const float* sh,
                                   int sh_batch, int num_vertices, const float* faces_uv, const float* image, int image_batch,
                                   int image_height, int image_width, int texture_wrapping, const float* grad_images,
                                   float* pixel_grads, d3m_stream_t stream);
/* Analytic edge antialiasing of an image drawn over a coverage record, and its silhouette gradient (an addition;
 * csrc/d3m_antialias.h states the function, the pair decision and the order of every sum).  The record must be one without
 * anti-aliasing (S = image_size) that d3m_forward_face_index_map_mesh made from screen_vertices [B, V, 3];  side_opposite
 * [num_tri, 3] i32: per side j (corner j to j + 1) of a triangle the third vertex of the one other triangle on that undirected
 * edge, -1 for a boundary side, -2 for a side the node leaves alone (three or more triangles on it, a triangle that repeats an
 * index); an entry outside [-1, V) counts as -2.  images [B, C, S, S] in output orientation (row 0 = top).
 * d3m_antialias_images WRITES every element of images_out [B, C, S, S]: the image with the two pixels on either side of
 * every silhouette edge blended by the edge's position between their centres; a pixel of no such pair keeps its bits.  One
 * launch (k_antialias_images).  D3M_ERR_INVALID, before any launch: what d3m_vertex_attribute_images refuses of the record
 * and of num_vertices / num_channels, a record with anti_aliasing, B S S beyond 2^32, a NULL or misaligned images /
 * screen_vertices / side_opposite / images_out, images_out == images. */
int d3m_antialias_images(const d3m_fragments* fragments, const float* images, int num_channels, const float* screen_vertices,
                         int num_vertices, const int32_t* side_opposite, float* images_out, d3m_stream_t stream);
/* The adjoint with respect to the image and the derivative with respect to every pair's edge position, for grad_out [B, C,
 * S, S]: grad_images [B, C, S, S] (NULL: not formed), every element WRITTEN, and pair_grads [B, S, S, 4] in map orientation
 * (NULL: not formed), every element WRITTEN: slot -x, +x, -y, +y of a pixel holds dL/dt of that pair when the pixel is the
 * pair's near pixel, else +0.  A gather: no atomics, nothing cleared.  One launch (k_antialias_images_backward).
 * D3M_ERR_INVALID, before any launch: what d3m_antialias_images refuses (images_out aside), a NULL or misaligned grad_out,
 * both results NULL, a misaligned result, grad_images == images or grad_out. */
int d3m_antialias_images_backward(const d3m_fragments* fragments, const float* images, int num_channels,
                                  const float* screen_vertices, int num_vertices, const int32_t* side_opposite,
                                  const float* grad_out, float* grad_images, float* pair_grads, d3m_stream_t stream);
/* Floats of scratch of d3m_antialias_geometry_backward: d3m_fragment_geometry_scratch_floats(..., 0)'s B F' 9 per-face sums
 * and 3 B num_chunks chunk sums; with_pair_grads != 0: and 4 B S S more, room for a pair_grads map.  0 for sizes that are
 * refused. */
size_t d3m_antialias_scratch_floats(int batch_size, int num_faces, int raster_size, const d3m_csr* adjacency,
                                    int with_pair_grads);
/* pair_grads [B, S, S, 4] (d3m_antialias_images_backward's) -> grad_screen_vertices [B, V, 3], every element WRITTEN: x and y
 * of the two end vertices of every silhouette edge a pair chose; the z column, and a vertex on no such edge, get +0.
 * adjacency: the faces' d3m_csr of V rows (item = 3 f + c).  scratch needs no initialisation.  No float atomics, nothing
 * cleared; three launches (k_antialias_face_sums, k_antialias_large_face_sums, k_vertex_attribute_adjoint_rows) and
 * k_vertex_attribute_adjoint_chunks on a mesh with long rows.  D3M_ERR_INVALID, before any launch: what
 * d3m_fragment_geometry_backward refuses (pair_grads in the place of pixel_grads), a record with anti_aliasing;
 * D3M_ERR_WORKSPACE: scratch_floats below d3m_antialias_scratch_floats(..., 0). */
int d3m_antialias_geometry_backward(const d3m_fragments* fragments, const float* pair_grads, const d3m_csr* adjacency,
                                    float* scratch, size_t scratch_floats, float* grad_screen_vertices, int num_vertices,
                                    d3m_stream_t stream);
/* View images baked into a uv texture, the inverse of d3m_uv_texture_images (an addition; csrc/d3m_uv_bake.h states the
 * function, the visibility decision and the order of every sum).  layout: the record of the faces_uv layout -- batch_size 1,
 * no anti-aliasing, raster size T, every vertex at z = 1, so that its weight_map holds a texel's barycentrics in its owner --;
 * view: the record of B views that d3m_forward_face_index_map_mesh made from screen_vertices [B, V, 3]; both of num_tri
 * triangles.  images [B, C, H, W] in output orientation (row 0 = top), 1 <= C <= 64, H, W <= 32768.
 * d3m_uv_bake_texture WRITES every element of texture [B, T, T, C] (a visible texel: the four bilinear taps at its surface
 * point in the view; else background [C], NULL = zeros) and of mask [B, T, T] (1 or 0).  One launch (k_uv_bake_texture).
 * D3M_ERR_INVALID, before any launch: what d3m_vertex_attribute_images refuses of either record, a layout record with
 * batch_size != 1 or with anti_aliasing, records of different num_tri, sizes outside the ranges above, a depth_tolerance
 * that is negative or not finite, a NULL or misaligned images / screen_vertices / texture / mask, a misaligned background. */
int d3m_uv_bake_texture(const d3m_fragments* layout, const d3m_fragments* view, const float* images, int num_channels,
                        int image_height, int image_width, const float* screen_vertices, int num_vertices, int perspective,
                        float depth_tolerance, const float* background, float* texture, float* mask, d3m_stream_t stream);
/* Bytes of scratch of d3m_uv_bake_images_backward: B C H W int64 accumulators and 1024 block maxima; 0 for sizes that are
 * refused. */
size_t d3m_uv_bake_images_scratch_bytes(int batch_size, int num_channels, int image_height, int image_width);
/* grad_texture [B, T, T, C] -> grad_images [B, C, H, W], every element WRITTEN: the order-independent fixed-point scatter of
 * d3m_uv_texture_images_backward (frac = 62 - ceil(log2(T T)); an all-zero gradient gives +0 everywhere, a non-finite one NaN
 * everywhere).  scratch needs no initialisation.  No float atomics; three launches (k_uv_texture_images_clear_max,
 * k_uv_bake_images_scatter, k_uv_texture_images_convert).  D3M_ERR_INVALID, before any launch: what d3m_uv_bake_texture
 * refuses of the records, sizes, tolerance and screen_vertices, a NULL or misaligned grad_texture / grad_images, a NULL
 * scratch or one not aligned to 8 bytes; D3M_ERR_WORKSPACE: scratch_bytes below d3m_uv_bake_images_scratch_bytes(). */
int d3m_uv_bake_images_backward(const d3m_fragments* layout, const d3m_fragments* view, int num_channels, int image_height,
                                int image_width, const float* screen_vertices, int num_vertices, int perspective,
                                float depth_tolerance, const float* grad_texture, void* scratch, size_t scratch_bytes,
                                float* grad_images, d3m_stream_t stream);
/* Floats of scratch of d3m_uv_bake_vertices_backward: d3m_vertex_attribute_scratch_floats(B, F', 3, adjacency) -- the B F' 9
 * per-face sums and 3 B num_chunks chunk sums, F' = num_layout_faces the layout record's faces with its fill_back copies --
 * and B F' words of per-view flags.  0 for sizes that are refused. */
size_t d3m_uv_bake_scratch_floats(int batch_size, int num_layout_faces, const d3m_csr* adjacency);
/* grad_texture [B, T, T, C] -> grad_screen_vertices [B, V, 3] (x, y and z), every element WRITTEN; visibility and the choice
 * of taps are constants.  adjacency: the MESH faces' d3m_csr of V rows (item = 3 f + c).  scratch needs no initialisation.
 * No float atomics, nothing cleared; four launches (k_uv_bake_view_flags, k_uv_bake_face_sums, k_uv_bake_large_face_sums,
 * k_vertex_attribute_adjoint_rows) and k_vertex_attribute_adjoint_chunks on a mesh with long rows.  D3M_ERR_INVALID, before
 * any launch: what d3m_uv_bake_texture refuses (texture, mask and background aside), a NULL or misaligned grad_texture /
 * scratch / grad_screen_vertices, a layout record without a finished visibility blob, a malformed adjacency;
 * D3M_ERR_WORKSPACE: scratch_floats below d3m_uv_bake_scratch_floats(). */
int d3m_uv_bake_vertices_backward(const d3m_fragments* layout, const d3m_fragments* view, const float* images,
                                  int num_channels, int image_height, int image_width, const float* screen_vertices,
                                  int num_vertices, int perspective, float depth_tolerance, const float* grad_texture,
                                  const d3m_csr* adjacency, float* scratch, size_t scratch_floats,
                                  float* grad_screen_vertices, d3m_stream_t stream);
/* Fused view textures with their unseen texels filled by push-pull (an addition; csrc/d3m_uv_fill.h states the fusion, the
 * pull, the push and the order of every sum).  textures [B, H, W, C] and weights [B, H, W], 1 <= B <= 65535, 1 <= C <= 64,
 * H, W <= 32768 (any H, W).  The pyramids hold levels 1..L, level l of ceil(H / 2^l) x ceil(W / 2^l) texels, L the 1 x 1
 * level: d3m_uv_fill_pyramid_texels texels in all (0 for a 1 x 1 image and for sizes that are refused). */
size_t d3m_uv_fill_pyramid_texels(int image_height, int image_width);
/* Bytes of scratch of d3m_uv_fill_textures with fill != 0: C floats per pyramid texel (the sums) and per texel of levels
 * min(L, 5)..L (the pushed values).  0 for sizes that are refused. */
size_t d3m_uv_fill_scratch_bytes(int image_height, int image_width, int num_channels);
/* Bytes of scratch of d3m_uv_fill_textures_backward with fill != 0: C floats per pyramid texel.  0 for refused sizes. */
size_t d3m_uv_fill_backward_scratch_bytes(int image_height, int image_width, int num_channels);
/* WRITES every element of texture [H, W, C] and of valid [H, W] (1 or 0: some view's weight is > 0).  fill == 0: the weighted
 * mean of the views at valid texels, background [C] (NULL = zeros) elsewhere; one launch (k_uv_fill_fuse_tile), scratch and
 * counts unused.  fill != 0: the invalid texels are filled by push-pull; counts [count_texels] int32 receives the valid
 * texels under every pyramid texel (the backward reads it); three launches (k_uv_fill_fuse_tile, k_uv_fill_top,
 * k_uv_fill_push_tile).  scratch and counts need no initialisation.  D3M_ERR_INVALID, before any launch: sizes outside the
 * ranges above, a NULL or misaligned textures / weights / texture / valid, a misaligned background, with fill a NULL or
 * misaligned scratch or (beyond 1 x 1) counts; D3M_ERR_WORKSPACE: scratch_bytes below d3m_uv_fill_scratch_bytes() or
 * count_texels below d3m_uv_fill_pyramid_texels(). */
int d3m_uv_fill_textures(const float* textures, const float* weights, int batch_size, int image_height, int image_width,
                         int num_channels, int fill, const float* background, void* scratch, size_t scratch_bytes,
                         int32_t* counts, size_t count_texels, float* texture, float* valid, d3m_stream_t stream);
/* grad_texture [H, W, C] -> grad_textures [B, H, W, C], every element WRITTEN (exactly +0 where a view does not count);
 * weights, valid and counts: the forward's.  Gathers in a fixed order: no atomics, nothing cleared.  fill != 0:
 * k_uv_fill_adjoint_tile once per three levels while a level exceeds 32 x 32 and once for the levels above, then
 * k_uv_fill_adjoint_views -- 2 launches up to 32 x 32, 3 up to 256 x 256, 4 up to 2048 x 2048 --; fill == 0: one launch,
 * scratch and counts unused.  D3M_ERR_INVALID, before any launch: refused sizes, a NULL or misaligned weights / valid /
 * grad_texture / grad_textures, with fill beyond 1 x 1 a NULL or misaligned scratch or counts; D3M_ERR_WORKSPACE:
 * scratch_bytes below d3m_uv_fill_backward_scratch_bytes() or count_texels below d3m_uv_fill_pyramid_texels(). */
int d3m_uv_fill_textures_backward(const float* weights, const float* valid, const int32_t* counts, size_t count_texels,
                                  const float* grad_texture, int batch_size, int image_height, int image_width,
                                  int num_channels, int fill, void* scratch, size_t scratch_bytes, float* grad_textures,
                                  d3m_stream_t stream);
/* Regularisers of a UV texture (an addition; csrc/d3m_uv_texture_reg.h states the four terms, their counts and the order of
 * every sum): smoothness over the 4-neighbour pairs, left-right symmetry (u -> 1 - u), flatness and an anchor to a reference
 * texture, per image.  texture [B, H, W, C], 1 <= B <= 65535, 1 <= C <= 4, H, W <= 32768 (any H, W); mask [mask_batch, H, W],
 * mask_batch 1 or B, or NULL (every texel active; mask_batch ignored): a texel is active iff its mask is > 0; reference
 * [reference_batch, H, W, C], reference_batch 1 or B; reference_weights [reference_weights_batch, H, W], batch 1 or B, or NULL
 * (1).  w_* >= 0, not all 0; a term of weight 0 is not evaluated and its inputs are not read (reference and
 * reference_weights may be NULL with w_anchor == 0).  smooth_eps: D3M_UV_TEXTURE_REG_NO_EPS for the squared difference, else
 * > 0 (Charbonnier).  What every entry point refuses with D3M_ERR_INVALID before any launch: sizes, batches or C outside these
 * ranges, a negative or NaN weight, all weights 0, another smooth_eps <= 0 or NaN, w_anchor > 0 without a reference, a NULL
 * texture, a texture / reference / gradient not aligned to 16 bytes with C = 4, 8 with C = 2 and 4 otherwise, another
 * misaligned pointer. */
#define D3M_UV_TEXTURE_REG_NO_EPS (-1.0f)
/* Bytes of scratch of the two entry points below; 0 for sizes that are refused. */
size_t d3m_uv_texture_regularizer_scratch_bytes(int batch_size, int image_height, int image_width);
/* WRITES value [B] and stats [B, 4 + C]: the per-image coefficients weight / (count C) of the four terms (0 where the
 * count is 0) and the C channel means of the active texels, which d3m_uv_texture_regularizer_grad reads.  The counts are
 * taken on the device on every call.  Four launches (k_uv_texture_reg_stats, k_uv_texture_reg_stats_finish,
 * k_uv_texture_reg_terms, k_uv_texture_reg_value_finish), whatever B, H, W, C and the weights.  scratch needs no
 * initialisation.  D3M_ERR_INVALID also for a NULL value or stats, a NULL or misaligned scratch; D3M_ERR_WORKSPACE:
 * scratch_bytes below d3m_uv_texture_regularizer_scratch_bytes(). */
int d3m_uv_texture_regularizer(const float* texture, int batch_size, int image_height, int image_width, int num_channels,
                               const float* mask, int mask_batch, float w_smooth, float smooth_eps, float w_symmetry,
                               float w_flat, float w_anchor, const float* reference, int reference_batch,
                               const float* reference_weights, int reference_weights_batch, void* scratch, size_t scratch_bytes,
                               float* stats, float* value, d3m_stream_t stream);
/* Value and gradient.  grad_texture [B, H, W, C] (NULL: not wanted): every element WRITTEN, the gradient of image b times
 * grad_scale[b] (device memory; NULL: 1); exactly +0 at inactive texels and where grad_scale[b] == 0.  value [B] (NULL: not
 * wanted).  stats: the forward's [B, 4 + C], or NULL: they are computed here into scratch.  A gather per texel: no float
 * atomics, nothing cleared.  Launches: k_uv_texture_reg_terms alone with stats and without value; + k_uv_texture_reg_value_finish
 * with value; + k_uv_texture_reg_stats and k_uv_texture_reg_stats_finish without stats: at most four.  D3M_ERR_INVALID also
 * for value and grad_texture both NULL, a NULL or misaligned scratch where one is needed (without stats, with value);
 * D3M_ERR_WORKSPACE as above. */
int d3m_uv_texture_regularizer_grad(const float* texture, int batch_size, int image_height, int image_width, int num_channels,
                                    const float* mask, int mask_batch, float w_smooth, float smooth_eps, float w_symmetry,
                                    float w_flat, float w_anchor, const float* reference, int reference_batch,
                                    const float* reference_weights, int reference_weights_batch, const float* stats,
                                    const float* grad_scale, void* scratch, size_t scratch_bytes, float* value,
                                    float* grad_texture, d3m_stream_t stream);
/* Nearest points and chamfer distances between point sets (an addition; csrc/d3m_point_sets.h states the distance, the tie
 * rule, the order of every sum and the fixed-point scatter of the adjoint).  a [B, N, 3] and b [B, M, 3] in f32, 1 <= B <= 65535,
 * 1 <= N, M <= 2^30; lengths_a [B], lengths_b [B]: int32 in device memory, the ragged set sizes (clamped to 0 .. N and 0 .. M), or
 * NULL: N and M.  splits: the number of workgroups the targets' tiles of d3m_point_set_tile() points are split over per query
 * block, 0: d3m_point_set_splits() of the shapes; no result depends on it by a bit.  scratch: d3m_chamfer_distance_scratch_bytes()
 * bytes aligned to 8, no initialisation needed.  What every entry point refuses with D3M_ERR_INVALID before any launch: sizes
 * outside these ranges, a NULL a, b or scratch, a negative splits, a misaligned pointer, a NULL output that it writes;
 * D3M_ERR_WORKSPACE: scratch_bytes below the query's answer. */
/* Bytes of scratch of the three entry points below; 0 for sizes that are refused. */
size_t d3m_chamfer_distance_scratch_bytes(int batch_size, int num_points_a, int num_points_b);
/* The kernel's tile of targets, its queries per lane (a workgroup takes 256 times as many), and the split count it chooses for
 * B sets of num_queries queries against num_targets targets (0 for sizes that are refused). */
int d3m_point_set_tile(void);
int d3m_point_set_queries_per_lane(void);
int d3m_point_set_splits(int batch_size, int num_queries, int num_targets);
/* WRITES every element of index [B, N] (int32) and dist2 [B, N]: for every point its nearest target (the lowest index among equal
 * f32 distances) and the squared distance; -1 and +0 for a point at or beyond its set's length and for every point of an element
 * without targets; -1 and NaN where every candidate distance is NaN.  Three launches (k_pset_init, k_pset_nearest, k_pset_resolve). */
int d3m_nearest_points(const float* points, const float* targets, int batch_size, int num_points, int num_targets,
                       const int* lengths, const int* target_lengths, int splits, void* scratch, size_t scratch_bytes, int* index,
                       float* dist2, d3m_stream_t stream);
/* WRITES value [B] = weight_ab L_ab + weight_ba L_ba, L_ab the mean over a's points of rho(dist2 to the nearest point of b), rho
 * the identity (squared != 0) or the square root; truncate >= 0: a term with dist2 > truncate^2 contributes rho(truncate^2),
 * truncate < 0: none.  Also WRITES the searches' index_ab, dist2_ab [B, N] and index_ba, dist2_ba [B, M] and coef [B, 2] =
 * weight / set length (0 for an empty set), which d3m_chamfer_distance_backward reads.  A direction of weight 0 is not evaluated:
 * its index and dist2 may be NULL and are not written.  Four launches (k_pset_init, k_pset_nearest, k_pset_resolve,
 * k_pset_value_finish).  D3M_ERR_INVALID also for a negative or non-finite weight, both weights 0, a non-finite truncate. */
int d3m_chamfer_distance(const float* a, const float* b, int batch_size, int num_points_a, int num_points_b, const int* lengths_a,
                         const int* lengths_b, int squared, float truncate, float weight_ab, float weight_ba, int splits,
                         void* scratch, size_t scratch_bytes, int* index_ab, float* dist2_ab, int* index_ba, float* dist2_ba,
                         float* coef, float* value, d3m_stream_t stream);
/* WRITES every element of grad_a [B, N, 3] and grad_b [B, M, 3], the argmin held constant: a point's direct term as a query plus
 * minus the terms of the points whose nearest neighbour it is, summed in 64-bit fixed point (no float atomics; the same bits on
 * every run).  index_* / dist2_* / coef: the forward's; a direction whose index is NULL is off.  upstream [B] in device memory,
 * the gradient of value; or, with upstream_per_query != 0, upstream [B, N], the gradient of d3m_nearest_points' dist2 (coef and
 * index_ba NULL).  Exactly +0 at truncated terms' direct gradients, beyond the sets' lengths and everywhere when every term is
 * 0; NaN everywhere when a term is not finite.  Three launches (k_pset_direct, k_pset_scatter, k_pset_convert). */
int d3m_chamfer_distance_backward(const float* a, const float* b, int batch_size, int num_points_a, int num_points_b,
                                  const int* lengths_a, const int* lengths_b, const int* index_ab, const float* dist2_ab,
                                  const int* index_ba, const float* dist2_ba, const float* coef, const float* upstream,
                                  int upstream_per_query, int squared, float truncate, void* scratch, size_t scratch_bytes,
                                  float* grad_a, float* grad_b, d3m_stream_t stream);
/* Replaces create_texture_image_cuda (NR/cuda/create_texture_image_cuda.cpp:6-30, kernels
 * create_texture_image_cuda_kernel.cu:10-115, both launches in one pass): renders textures
 * [F, tsi, tsi, tsi, 3] into the atlas image [image_height, image_width, 3] of tile_width tiles per row
 * (tile edge = image_width / tile_width); vertices_all [F, 3, 2] are the tile-space corners.  Tiles beyond
 * num_faces are zero-filled. */
int d3m_create_texture_image(const float* vertices_all, const float* textures, float* image, int num_faces,
                             int texture_size_in, int image_height, int image_width, int tile_width, float eps,
                             d3m_stream_t stream);

/* ---- the face3d utility rasterizer family (f64) ----------------------------------------------------------------
 * Replace the C++ cores of deep3dmap/core/renderer/renderer_demo/mesh_cython/render.cpp (MC) that render_cython.pyx
 * exposes (:55-161) and render.py drives (:124-299); same argument order and array layouts (vertices [3,nver],
 * triangles [3,ntri] coordinate-major, images [h,w,c], everything double / int32), device pointers, plus a workspace
 * of d3m_mesh_workspace_bytes(nver, ntri, h, w) bytes (no initialisation needed; pass 0 for the dimensions a
 * function does not have) and a stream.  In/out buffers (image, depth_buffer, depth_tmp, vis, triangle_buffer, norm,
 * uv) are pre-filled by the caller as render.py does and updated exactly as the reference's sequential loops would. */
size_t d3m_mesh_workspace_bytes(int nver, int ntri, int h, int w);
/* _render_colors_core, MC:27-91 */
int d3m_mesh_render_colors(double* image, const double* vertices, const int32_t* triangles, const double* tri_depth,
                           const double* tri_tex, double* depth_buffer, int nver, int ntri, int h, int w, int c,
                           void* workspace, size_t workspace_bytes, d3m_stream_t stream);
/* _render_texture_core, MC:94-185 (mapping_type 0 nearest, 1 bilinear; texel indices are clamped) */
int d3m_mesh_render_texture(double* image, const double* vertices, const int32_t* triangles, const double* texture,
                            const double* tex_coords, const int32_t* tex_triangles, const double* tri_depth,
                            double* depth_buffer, int nver, int tex_nver, int ntri, int h, int w, int c, int tex_h,
                            int tex_w, int tex_c, int mapping_type, void* workspace, size_t workspace_bytes,
                            d3m_stream_t stream);
/* _map_texture_core, MC:188-250 */
int d3m_mesh_map_texture(double* dst_image, const double* src_image, const double* dst_vertices,
                         const double* src_vertices, const int32_t* dst_triangle_buffer, const int32_t* triangles,
                         int nver, int ntri, int sh, int sw, int sc, int h, int w, int c, d3m_stream_t stream);
/* _vis_of_vertices_core, MC:253-318 */
int d3m_mesh_vis_of_vertices(double* vis, const double* vertices, const int32_t* triangles, const double* tri_depth,
                             double* depth_buffer, double* depth_tmp, int nver, int ntri, int h, int w, void* workspace,
                             size_t workspace_bytes, d3m_stream_t stream);
/* _get_triangle_buffer_core, MC:321-365 */
int d3m_mesh_get_triangle_buffer(int32_t* triangle_buffer, const double* vertices, const int32_t* triangles,
                                 const double* tri_depth, double* depth_buffer, int nver, int ntri, int h, int w,
                                 void* workspace, size_t workspace_bytes, d3m_stream_t stream);
/* _get_norm_direction_core, MC:4-24 (sums in triangle-index order, as the reference's loop) */
int d3m_mesh_get_norm_direction(double* norm, const double* tri_norm, const int32_t* triangles, int nver, int ntri,
                                void* workspace, size_t workspace_bytes, d3m_stream_t stream);
/* The numpy statements render.py wraps around the cores, with numpy's roundings (no fused multiply-add, true
 * division): per-triangle mean of per-vertex values [channels, nver] -> [channels, ntri] (render.py:141-142),
 * cross(pt0 - pt1, pt0 - pt2) per triangle (:6-9), and the unit-length step with the zero-normal rule (:19-26). */
int d3m_mesh_triangle_mean(const double* values, const int32_t* triangles, double* out, int channels, int nver, int ntri,
                           d3m_stream_t stream);
int d3m_mesh_triangle_normals(const double* vertices, const int32_t* triangles, double* tri_norm, int nver, int ntri,
                              d3m_stream_t stream);
int d3m_mesh_normalize(double* norm, int nver, d3m_stream_t stream);
/* _get_correspondence_core, MC:441-488 */
int d3m_mesh_get_correspondence(const double* image, const double* pncc_code, double* uv, int nver, int h, int w, int c,
                                void* workspace, size_t workspace_bytes, d3m_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* D3M_RASTER_H */
