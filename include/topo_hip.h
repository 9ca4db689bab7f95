/*
 * topo_hip.h -- C ABI of libtopo_hip.so: the MI355X-native terrain render path of krzyz/topo-renderer.
 *
 * The reference has no FFI or plugin interface; the seam this library plugs into is the inherent-method
 * surface of `TerrainRenderer` (topo-renderer/src/render/terrain_renderer.rs), called only from
 * `RenderEngine` (render_engine.rs:143,160-166,183-189,212-214,276-284).  Each entry point below names the
 * reference method it replaces; INTEGRATION.md shows the Rust `extern "C"` shim that binds them.
 *
 * Conventions: every function returns TOPO_OK (0) or a negative topo_status; topo_last_error() gives the
 * text.  No exception crosses the boundary.  A context is thread-affine like the reference (all calls from
 * the one event-loop thread; the reference keeps its shared mesh buffers in thread_local!,
 * render_buffer.rs:12-15).  The caller keeps ownership of every input pointer; outputs are caller-allocated.
 * There is no CPU fallback: with no HIP device every compute call fails with TOPO_ERR_HIP.
 */
#ifndef TOPO_HIP_H
#define TOPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct topo_ctx topo_ctx;

typedef enum topo_status {
    TOPO_OK = 0,
    TOPO_ERR_INVALID = -1,     /* bad argument (null pointer, zero size, mixed tile sizes, ...) */
    TOPO_ERR_UNSUPPORTED = -2, /* valid in the reference but outside this path (pixelize_n < 99.99999, format) */
    TOPO_ERR_HIP = -3,         /* a HIP runtime call failed (no device, out of memory, launch failure) */
    TOPO_ERR_NOT_FOUND = -4,   /* no such tile */
    TOPO_ERR_CAPACITY = -5     /* draw-order id space exhausted (too many / too large tiles), or a frame overflowed its
                                * rare-triangle queue and is incomplete (see topo_join) */
} topo_status;

/* The surface format the reference picks: `surface_caps.formats[0]`, with the sRGB suffix when the surface also offers
 * that variant (render_engine.rs:77-84); render target and final target share it (terrain_renderer.rs:88-93).  The *Srgb
 * formats encode linear -> sRGB8 on store and decode on sample (so the pipeline encodes twice and decodes once in
 * between); the plain formats store round(clamp(v) * 255) and sample c / 255.  Bgra differs from Rgba
 * only in the byte order of the output texels (B G R A in memory). */
#define TOPO_FORMAT_RGBA8_UNORM_SRGB 1u
#define TOPO_FORMAT_BGRA8_UNORM_SRGB 2u
#define TOPO_FORMAT_RGBA8_UNORM 3u
#define TOPO_FORMAT_BGRA8_UNORM 4u

/* `Uniforms`, #[repr(C)], 160 bytes: topo-renderer/src/render/data.rs:33-41 (WGSL mirror render_shader.wgsl:3-9).
 * Matrices are glam column-major. */
typedef struct topo_uniforms {
    float camera_proj[16]; /* projection * view (camera.rs:122-128) */
    float normal_proj[16]; /* uploaded by the reference, read by no shader */
    float camera_pos[4];   /* eye, w = 0; only .xy reaches the output (dither seed) */
    float sun_direction[3];
    int32_t view_mode;     /* 0 lit + dither, 1 lit, 2 normals (render_shader.wgsl:108-114) */
} topo_uniforms;

/* `PostprocessingUniforms`, 16 bytes: render/data.rs:74-80 */
typedef struct topo_post_uniforms {
    float viewport[2];
    float pixelize_n; /* the reference always passes 100.0 (application_data.rs:31); < 99.99999 is rejected */
    float _padding;
} topo_post_uniforms;

/* ---- the TerrainRenderer surface ---------------------------------------------------------------------- */

/* TerrainRenderer::new(device, format, target_size)                        terrain_renderer.rs:37-69 */
int topo_create(topo_ctx** out, int hip_device, uint32_t width, uint32_t height, uint32_t color_format);
void topo_destroy(topo_ctx* ctx);

/* TerrainRenderer::add_terrain(.., location, height_map_data, coordinate_transform, size, ..)
 *                                                                           terrain_renderer.rs:173-350
 * heights: w*h little-endian f32, row-major, row 0 = north (RenderBuffer::new, render_buffer.rs:76-90), host
 * memory, borrowed for the call.  raster_point/model_point/pixel_scale: CoordinateTransform
 * (common/coordinate_transform.rs:16-20).  Uploads, computes the interior normals and the seam/corner normals
 * against the already loaded neighbours exactly as the reference orchestrates them.  Returns when the copy of
 * `heights` is complete (work stays queued on the context's stream). */
int topo_add_terrain(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg, const float* heights, uint32_t w, uint32_t h,
                     const float raster_point[2], const float model_point[2], const float pixel_scale[2]);

/* TerrainRenderer::unload_terrain(&location)                                terrain_renderer.rs:361-363 */
int topo_unload_terrain(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg);

/* TerrainRenderer::update(device, queue, target_size, &uniforms, &postprocessing_uniforms)
 *                                                                           terrain_renderer.rs:151-171 */
int topo_update(topo_ctx* ctx, uint32_t width, uint32_t height, const topo_uniforms* uniforms,
                const topo_post_uniforms* post);

/* TerrainRenderer::render(target, encoder, viewport) + the depth copy of RenderEngine::render
 *                                               terrain_renderer.rs:365-452, render_engine.rs:219-249
 * rgba_out: height rows of width RGBA8 (sRGB-encoded) texels, rgba_pitch bytes apart.  depth_out (nullable):
 * Depth32Float rows depth_pitch bytes apart; the reference uses pad_256(4*width) (data/mod.rs:9-11).
 * Host pointers; synchronous.  A frame whose rare-triangle queue overflowed is rendered again with a grown queue (with an
 * explicit topo_debug_set_queue_caps capacity: TOPO_ERR_CAPACITY instead); only the frame handed out counts for
 * topo_frame_status.  An overflow of a frame queued earlier through the asynchronous entry points is not this call's error:
 * it stays for the next topo_join / topo_synchronize. */
int topo_render(topo_ctx* ctx, uint8_t* rgba_out, size_t rgba_pitch, float* depth_out, size_t depth_pitch);
/* The way out to host memory.  The reference presents its frame without a read-back and maps the depth buffer only when the
 * camera moved (render_engine.rs:219-252); a host that asks topo_render for host images gets them at the link's rate if it
 * pins the buffers it reuses frame after frame (hipHostRegister under the hood; unpin before freeing them):
 * topo_render then copies straight into them.  Any other buffer is filled through a pinned staging image of the context's
 * own, slice by slice (the device copies slice k + 1 while host threads move slice k to the caller's rows) -- several times
 * the rate of a plain copy into pageable memory, below the pinned one.  depth_out == NULL skips the depth copy. */
int topo_pin_host_buffer(topo_ctx* ctx, void* buffer, size_t bytes);
int topo_unpin_host_buffer(topo_ctx* ctx, void* buffer);

const char* topo_last_error(topo_ctx* ctx);

/* ---- additive entry points (no reference counterpart) ------------------------------------------------- */

/* topo_render with device outputs: the frame of the last topo_update into rgba_dev / depth_dev (depth nullable), in stream
 * order on the context's stream; no host copy.  Asynchronous: the frame's status is reported by the call that waits
 * for it (topo_join / topo_synchronize, or topo_frame_status). */
int topo_render_device(topo_ctx* ctx, uint8_t* rgba_dev, size_t rgba_pitch, float* depth_dev, size_t depth_pitch);
/* As topo_add_terrain with `heights` already in device memory (device-to-device copy). */
int topo_add_terrain_device(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg, const float* heights_dev, uint32_t w,
                            uint32_t h, const float raster_point[2], const float model_point[2],
                            const float pixel_scale[2]);

/* Re-runs the whole load phase (interior, seam and corner normals) over the resident heights, replaying the
 * original insertion order.  Used to time the load phase without PCIe. */
int topo_recompute_normals(topo_ctx* ctx);

/* n_views complete reference frames (one per `views[i]`) of width x height over the loaded tiles, in one
 * submission.  View i's image starts at rgba_dev + i*rgba_view_stride (bytes), rows rgba_pitch apart; same for
 * depth_dev (nullable).  Device pointers; asynchronous on the context's stream.  A 360-degree panorama is
 * 8 views of 45 degrees; with rgba_view_stride = 4*width and rgba_pitch = 4*n_views*width the
 * views land side by side in one row-major strip. */
int topo_render_views_device(topo_ctx* ctx, uint32_t n_views, const topo_uniforms* views, uint32_t width,
                             uint32_t height, uint8_t* rgba_dev, size_t rgba_view_stride, size_t rgba_pitch,
                             float* depth_dev, size_t depth_view_stride, size_t depth_pitch);

/* ---- multi-GPU: the 360-degree strip sharded by azimuth sector, and the viewpoint batch ---------------------------
 * (no reference counterpart: the reference renders one perspective view on one GPU.)
 * One process per GPU, each with its own topo_ctx over the same tiles (the DEM is replicated: 1.15 GB of 288 GB).  The
 * strip is TOPO_PANORAMA_SECTORS = 8 fixed sectors of sector_w x sector_h (the cameras of topo_panorama_uniforms), stored
 * SECTOR-MAJOR -- uint8 strip[8][sector_h][sector_w][4], float depth[8][sector_h][sector_w] -- so that the share of rank g,
 * sectors [8g/N, 8(g+1)/N), is one contiguous block.  topo_render_panorama renders this rank's sectors into their place in
 * strip_dev / depth_dev (device pointers, caller-owned, the same size on every rank) -- ONE cull / raster submission for all of
 * them -- and exchanges them over RCCL (xGMI) so that after topo_synchronize every rank holds the whole strip, bit-identical
 * for every N.  The exchange is overlapped: the frame is resolved in slots (topo_panorama_slots: a sector of the rank's range
 * and a band of its rows, ~8 MiB of RGBA each, the same plan on every rank), and behind each slot's resolve kernel the slot
 * is shipped on a second stream -- every rank sends its part to every other rank and receives theirs straight into place
 * (grouped ncclSend / ncclRecv: all seven xGMI links of a fully connected node carry a slot at once) -- while the next slot
 * is being resolved; the context's stream waits for the last exchange.  comm == NULL (or a world of 1): all 8 sectors, no
 * exchange.  RCCL is bound at run time (dlopen of librccl.so); nothing else in this library needs it.
 *
 * Call sequence for N ranks: rank 0 calls topo_comm_unique_id and hands the 128 bytes to the other ranks through the
 * host's own channel (a file, a socket, MPI, ...); every rank calls topo_comm_init(&comm, its_device, id, rank, N)
 * (collective: returns when all N have joined), loads the same tiles, then calls topo_render_panorama with the same
 * arguments; topo_comm_destroy at the end.  A host that already owns an ncclComm_t (e.g. one created by PyTorch) wraps it
 * with topo_comm_from_nccl instead; it is borrowed, not destroyed. */
#define TOPO_PANORAMA_SECTORS 8u
#define TOPO_COMM_ID_BYTES 128u
typedef struct topo_comm topo_comm;
int topo_comm_unique_id(uint8_t out_id[TOPO_COMM_ID_BYTES]);
int topo_comm_init(topo_comm** out, int hip_device, const uint8_t id[TOPO_COMM_ID_BYTES], int rank, int world);
int topo_comm_from_nccl(topo_comm** out, void* nccl_comm, int rank, int world);
void topo_comm_destroy(topo_comm* comm);
/* The sectors rank `rank` of `world` renders: [*first, *first + *count). */
void topo_panorama_sector_range(int rank, int world, uint32_t* first, uint32_t* count);
typedef struct topo_panorama_slot {
    uint32_t sector;       /* index within the rank's sector range: sector (first + sector) of the strip */
    uint32_t row0, rows;   /* the band of pixel rows [row0, row0 + rows) of that sector */
} topo_panorama_slot;
/* The resolve / exchange slots of one panorama for a world of `world` ranks, in the order every rank goes through them;
 * writes up to `cap` of them to `out` (nullable) and returns their number.  Slot i of rank g is bytes
 * [((g * 8 / world + sector) * sector_h + row0) * sector_w * 4, + rows * sector_w * 4) of the strip. */
uint32_t topo_panorama_slots(int world, uint32_t sector_w, uint32_t sector_h, topo_panorama_slot* out, uint32_t cap);
int topo_render_panorama(topo_ctx* ctx, topo_comm* comm, const float eye[3], float yaw0, float pitch, uint32_t sector_w,
                         uint32_t sector_h, float sun_theta_deg, float sun_phi_deg, int32_t view_mode, uint8_t* strip_dev,
                         float* depth_dev /* nullable */);
/* BASELINE config 5 (throughput mode): n_viewpoints independent panoramas -- viewpoint v has eye eyes_xyz[3v..], first
 * sector yaw yaw0[v], sun (sun_theta_phi_deg[2v], [2v+1]) -- into rgba_dev[v][8][sector_h][sector_w][4] (and depth_dev
 * likewise, nullable).  Eight viewpoints (64 views) go into one submission and, with topo_set_pipeline_depth(d), d
 * submissions are in flight; asynchronous (topo_join / topo_synchronize).  Viewpoints are independent: a multi-GPU host
 * gives each rank its own share of the batch, there is no collective. */
int topo_render_batch(topo_ctx* ctx, uint32_t n_viewpoints, const float* eyes_xyz, const float* yaw0,
                      const float* sun_theta_phi_deg, float pitch, uint32_t sector_w, uint32_t sector_h, int32_t view_mode,
                      uint8_t* rgba_dev, float* depth_dev /* nullable */);

/* RenderEngine::get_visible_labels(peaks, projection, size, depth_state, depth_buffer_view)   render_engine.rs:338-396
 * (the immediate consumer of the depth output, kept on the device so the pad_256 read-back
 * disappears).  For each peak (ECEF f32 xyz, PeakInstance.position): project_point3 through `camera_proj`; inside
 * the open NDC cube (|x| < 1, |y| < 1, z < 1) it maps to pixel (x_pos, y_pos) = ((0.5*(x+1)*w) as u32,
 * (-0.5*(y-1)*h) as u32) and is visible iff dist_from_depth(z) - 10 < dist_from_depth(depth[y_pos][x_pos]).
 * visible_out[i] = 0/1; xy_out[2i], xy_out[2i+1] = pixel (0 when not visible).  Host pointers; uses the uniforms of
 * the last topo_update and the depth of the last topo_render (which must have been called with depth_out). */
int topo_visible_peaks(topo_ctx* ctx, uint32_t n_peaks, const float* peaks_xyz, uint8_t* visible_out, uint32_t* xy_out);
/* Same over caller-owned device memory (any view of a topo_render_views_device submission); asynchronous. */
int topo_visible_peaks_device(topo_ctx* ctx, const topo_uniforms* view, uint32_t width, uint32_t height,
                              const float* depth_dev, size_t depth_pitch, uint32_t n_peaks, const float* peaks_xyz_dev,
                              uint8_t* visible_dev, uint32_t* xy_dev);

/* ---- overlay pass -------------------------------------------------------------------------
 * LineRenderer::render (line_renderer.rs:200-212, resources/shaders/line_shader.wgsl): the label leader lines and label
 * backgrounds, tessellated on the CPU (lyon, on the host's side) into a triangle list of `GpuVertex` (line_renderer.rs:18-25),
 * drawn INTO the post pass: opaque, counter-clockwise front faces, back faces culled, depth test Greater with write against
 * the post pass's depth attachment, which the post quad has filled with 1/4096 -- so z_index 2 (strokes) lies under 3
 * (fills) under 100 (the text renderer's layer, text_renderer.rs:291), an equal z keeps the earlier triangle, and z_index
 * <= 1 is never visible.  vs_main: z = z_index / 4096, p = (position + normal * line_width) * (1, -1),
 * clip = (2 p.x / width - 1, 2 p.y / height + 1, z, 1); positions are pixels, y down.  The image is the context's
 * width x height in its colour format (what topo_render / topo_render_device produced). */
typedef struct topo_overlay_vertex {
    float position[2];
    float normal[2];
    float color[3];      /* linear RGB; alpha is 1 */
    int32_t z_index;
} topo_overlay_vertex;   /* 32 bytes, = GpuVertex */
int topo_overlay_lines(topo_ctx* ctx, const topo_overlay_vertex* vertices, uint32_t n_vertices, const uint32_t* indices,
                       uint32_t n_indices, float line_width /* Primitive.width: 0.5 in the reference */, uint8_t* rgba /* host, in/out */,
                       size_t rgba_pitch);
int topo_overlay_lines_device(topo_ctx* ctx, const topo_overlay_vertex* vertices, uint32_t n_vertices, const uint32_t* indices,
                              uint32_t n_indices, float line_width, uint8_t* rgba_dev /* device, in/out */, size_t rgba_pitch);

/* TextRenderer::render (text_renderer.rs:198-204, :259-291): the label text, drawn into the same pass after the lines by
 * glyphon 0.10.0 (third-party; Cargo.lock).  The host keeps what is the host's -- shaping and glyph rasterisation (cosmic-text,
 * swash) into an R8 mask atlas -- and hands over what glyphon's own vertex buffer holds: one `GlyphToRender` per glyph (28
 * bytes: quad pos .. pos + dim in pixels showing the atlas texels uv .. uv + dim 1 : 1, color = a << 24 | r << 16 | g << 8 | b,
 * content_type_with_srgb = {1 = mask atlas, 1 = decode r, g, b from sRGB (ColorMode::Accurate on an *Srgb surface)}).  The
 * fragment is (color.rgb, color.a * mask) under BlendState::ALPHA_BLENDING -- in linear light on an *Srgb surface -- with the
 * pass's depth state: Greater with write, every glyph at `depth` (the reference: 100/4096, above the lines), so where quads
 * overlap the one drawn first keeps its pixels.  Colour glyphs (content type 0) are rejected with TOPO_ERR_UNSUPPORTED. */
typedef struct topo_glyph {
    int32_t pos[2];
    uint16_t dim[2];
    uint16_t uv[2];
    uint32_t color;
    uint16_t content_type_with_srgb[2];
    float depth;         /* not read: `depth` of the call applies to every glyph */
} topo_glyph;            /* 28 bytes, = glyphon's GlyphToRender */
int topo_overlay_glyphs(topo_ctx* ctx, const topo_glyph* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas_mask /* host, R8 */,
                        uint32_t atlas_w, uint32_t atlas_h, uint8_t* rgba /* host, in/out */, size_t rgba_pitch);
int topo_overlay_glyphs_device(topo_ctx* ctx, const topo_glyph* glyphs /* host */, uint32_t n_glyphs, float depth, const uint8_t* atlas_mask /* host */,
                               uint32_t atlas_w, uint32_t atlas_h, uint8_t* rgba_dev /* device, in/out */, size_t rgba_pitch);

/* Run the context's work on an existing hipStream_t (e.g. PyTorch's current stream); NULL restores the
 * context's own stream. */
int topo_set_stream(topo_ctx* ctx, void* hip_stream);
int topo_synchronize(topo_ctx* ctx);
/* Throughput mode for topo_render_views_device: with depth d > 1 (max 4) consecutive submissions rotate through d frame
 * contexts, each with its own buffers and HIP stream, so that the memory-latency-bound cull/raster phases of one frame run
 * under the ALU-bound resolve pass of the previous one (c4: 1.27 -> 1.08 ms per panorama at depth 2).  Each submission is
 * ordered after the work queued so far on the context's stream (topo_set_stream), but NOT the other way round: outputs are
 * complete after topo_join (waits for the frames in flight) or topo_synchronize.  Depth 1 (default): everything runs
 * in order on the context's stream.  topo_render (host outputs) always waits for its frame. */
int topo_set_pipeline_depth(topo_ctx* ctx, int32_t depth);
/* Waits for every frame in flight, on whichever stream it was queued (a slot-by-slot topo_render_panorama runs on the
 * context's stream at any depth).  A frame's status word is per frame; if one or more of the frames waited for overflowed
 * its rare-triangle queue (triangles were dropped: its outputs are incomplete) topo_join -- and likewise topo_synchronize --
 * returns TOPO_ERR_CAPACITY once: the next call reports only frames that finish after this one.  The frames after an
 * overflowed one are unaffected.  (topo_render, the synchronous entry point, never hands out such a frame: it grows the
 * queue and renders the frame again.) */
int topo_join(topo_ctx* ctx);
/* Status bits of the frames that have completed since the previous call (waits for the frames in flight first; the bits
 * of all of them OR-ed together, so a burst of frames cannot hide an earlier frame's overflow behind a clean last frame; an
 * attempt topo_render threw away and rendered again is not one of them; the call clears them): out[0] = status bits (bit 0 big-triangle queue overflowed: handled exactly, slower; bit 1 rare-triangle queue overflowed:
 * frame incomplete; bit 2 bounds violation, only ever set by the TOPO_BOUNDS_CHECK build libtopo_hip_check.so),
 * out[1] = site tag and out[2], out[3] = low/high word of the offending value of the first bounds violation. */
int topo_frame_status(topo_ctx* ctx, uint32_t out[4]);

/* Form of the interior-normals kernel: 4, 8, 16, 32 or 64 = staged through an LDS tile of that many output rows per
 * workgroup (BASELINE config 3's sweep knob); 0 (the default: the sweep's optimum on MI355X) = without an LDS tile -- four
 * texels per lane, the rows above and below kept in registers, neighbours by wave shifts -- for tile widths that are a
 * multiple of four (other widths take the LDS form with 32 rows).  Same bytes either way. */
int topo_set_normals_lds_rows(topo_ctx* ctx, int rows);

/* Two-phase occlusion filter: blocks whose nearest possible view depth exceeds `metres` are rastered only if some
 * pixel of their conservative footprint is not already covered by nearer terrain (exact: a dropped block cannot
 * win a pixel).  Default 90 000 m; 0 turns the filter off (one phase, every frustum-surviving block rastered). */
int topo_set_occlusion_split(topo_ctx* ctx, float metres);

/* Per-kernel durations (ms, HIP events on the context's stream) of the last topo_render* call:
 * [0] clear  [1] cull  [2] raster (both phases)  [3] occlusion test  [4] raster_rare + raster_big (both phases)
 * [5] resolve+post  [6] total; of the last topo_recompute_normals: [7] the load phase -- every load-time kernel of the
 * resident tiles: the per-tile tables of the frame phase (block min/max, cull bounds, sin/cos tables) and the normals K1-K3 --
 * and [8] its tables part alone.  Synchronises. */
#define TOPO_TIMING_SLOTS 9
int topo_get_timings(topo_ctx* ctx, float out_ms[TOPO_TIMING_SLOTS]);
/* The same durations of the last `n_frames` frames (each context keeps the events of its last 32), oldest first:
 * out_ms[7 * i + k] = slot [k] (k = 0..6) of frame i, *n_out = frames written.  Waits for the frames in flight, so it is
 * called AFTER a timed region: nothing inside the region has to wait for a frame just to learn its kernels' durations. */
int topo_get_timing_history(topo_ctx* ctx, uint32_t n_frames, float* out_ms, uint32_t* n_out);
/* Which of the slots [0]..[5] to measure (bit i = slot i; default all).  Every timing event between two kernels leaves the
 * GPU idle for ~6 us while the marker completes -- 4 % of a c4 frame, a third of a c1 frame with all nine events -- so a
 * caller that only wants one kernel's duration (bench.py: the dominant one) or none selects just that; unselected slots
 * read 0.  The total [6] (an event in front of the frame's first kernel and one behind its last) is measured unless
 * TOPO_TIMING_NO_TOTAL is or'ed into the mask (then it reads 0 too; slot_mask = TOPO_TIMING_NO_TOTAL: no events at all). */
#define TOPO_TIMING_NO_TOTAL 0x80u
int topo_set_timing_slots(topo_ctx* ctx, uint32_t slot_mask);

/* Counters of the last topo_render* call, its own (waits for that frame on the stream it was queued on): [0] near blocks rastered, [1] big-triangle items, [2] that frame's status bits
 * (bit 0: big-triangle queue overflowed -- handled in-lane, slower, still exact; bit 1: rare-triangle queue
 * overflowed -- triangles dropped, frame incomplete: see topo_join), [3] rare triangles
 * (>= 64 px across or near-clipped), [4] far blocks occlusion-tested, [5] far blocks that survived the test. */
int topo_get_counters(topo_ctx* ctx, uint32_t out[6]);

/* ---- viewshed: which ground the rendered frames show ------------------------------------------------------------
 * A tile of w x h texels has (w-1) x (h-1) cells; cell (x, y) is the quad between texels (x, y) and (x+1, y+1), row 0
 * north.  With accumulation on, every frame the context renders afterwards (topo_render, topo_render_device, every view of
 * topo_render_views_device, topo_render_batch, topo_render_panorama) marks each cell one of whose two triangles owns at least
 * one pixel of the frame, OR-ed into a mask per tile that persists until topo_viewshed_reset: eight panorama sectors give the
 * 360-degree viewshed, a batch of viewpoints what is seen from any of them.  A frame whose rare-triangle queue overflowed
 * (incomplete: see topo_join) marks nothing.  A tile added while the masks exist starts empty, also when it replaces one;
 * topo_unload_terrain frees its mask; the masks of tiles that stay survive topo_change_location.  Multi-GPU: each rank's
 * masks cover the sectors that rank rendered; combining them across ranks is the caller's job. */
/* on != 0: every later frame ORs the cells that won >= 1 pixel into per-tile masks (allocated on first use, 1 bit per
 * cell); 0: stop accumulating (the masks are kept). */
int topo_viewshed_enable(topo_ctx* ctx, int32_t on);
/* Empties every tile's mask (waits for the frames in flight). */
int topo_viewshed_reset(topo_ctx* ctx);
/* The tile's mask as (h-1) rows of (w-1) bytes, 0/1, row 0 north, into host memory with the given row pitch (waits for the
 * frames in flight); *n_visible_out (may be NULL) = the number of marked cells.  TOPO_ERR_NOT_FOUND for a tile that is not
 * loaded, TOPO_ERR_INVALID if accumulation was never enabled. */
int topo_viewshed_read(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg, uint8_t* mask_out, size_t pitch, uint64_t* n_visible_out);

/* ---- horizon: where the terrain meets the sky in the latest submission, column by column -----------------------------------
 * The latest submission is that of the last topo_render / topo_render_device / topo_render_views_device / topo_render_panorama (this
 * rank's sectors) / topo_render_batch call; a batch of more than 8 viewpoints is several submissions, and only its last one stays
 * queryable.  For every view v and column x of it the query reports the topmost terrain pixel: the smallest row whose pixel a
 * triangle won.  Row 0 means the terrain reaches the top edge: the true horizon may lie above the view.  The tile and cell are those
 * of the viewshed (cell (x, y) = the quad between texels (x, y) and (x+1, y+1), row 0 north); fan = the piece of a near-clipped
 * triangle.  Errors: TOPO_ERR_INVALID when nothing was rendered yet, for views outside the submission, and once tiles were added,
 * replaced or unloaded after it (its draw order is gone); TOPO_ERR_CAPACITY from the host read when the submission overflowed its
 * rare-triangle queue (incomplete: see topo_join; the next topo_join does not report it again).  Multi-GPU: each rank answers for
 * its own sectors. */
typedef struct topo_horizon_point {      /* 32 bytes */
    int32_t row;                         /* topmost terrain row; -1 all sky; -2 frame incomplete (device variant) */
    float depth;                         /* depth output at (row, column); 1.0 for sky */
    int32_t lat_deg, lon_deg;            /* tile of the winning triangle (0, 0 for sky) */
    uint32_t cell_x, cell_y, fan;        /* the triangle: viewshed cell numbering, row 0 north */
    uint32_t _reserved;
} topo_horizon_point;
#define TOPO_HORIZON_SKY (-1)
#define TOPO_HORIZON_INCOMPLETE (-2)
/* n_views / width / height of the latest submission (what the horizon calls read). */
int topo_horizon_shape(topo_ctx* ctx, uint32_t* n_views, uint32_t* width, uint32_t* height);
/* Host memory; waits for that submission.  Views [first_view, first_view + n_views), view i's `width` records at
 * out + i * view_stride (records, >= width). */
int topo_horizon_read(topo_ctx* ctx, uint32_t first_view, uint32_t n_views, topo_horizon_point* out, size_t view_stride);
/* Device memory (16-byte aligned); asynchronous: queued on the stream that submission ran on, behind it.  An incomplete frame
 * writes row TOPO_HORIZON_INCOMPLETE into every record. */
int topo_horizon_device(topo_ctx* ctx, uint32_t first_view, uint32_t n_views, topo_horizon_point* out_dev, size_t view_stride);
/* Host helper, f64: azimuth (degrees clockwise from true north at the eye, [0, 360)) and elevation (degrees above the plane normal
 * to the eye's geocentric radius) of the pixel-space points (x, y) = xy[2i], xy[2i+1] of the view `view` of width x height, into
 * az_el_out[2i], [2i+1].  The ray is obtained by inverting view->camera_proj; the eye is view->camera_pos.  With
 * (x, y) = (column + 0.5, row + 0.5) a horizon record becomes the skyline's azimuth and elevation. */
void topo_pixel_angles(const topo_uniforms* view, uint32_t width, uint32_t height, uint32_t n, const float* xy, double* az_el_out);

/* ---- ground: the terrain point under a pixel of the latest submission ------------------------------------------------------------
 * "What am I pointing at?"  For pixel (x, y) of view `view` of the latest submission (as the horizon calls define it) the query takes
 * the triangle that won the pixel, reads its three vertex heights from the tile's resident DEM and reports the point of that
 * triangle's plane which the view's camera_proj maps to the pixel centre (x + 0.5, y + 0.5): longitude and latitude (degrees,
 * lon = atan2(Y, X), lat = asin(Z / |p|)), height = |p| - R0 (R0 = 6 371 000 m, the reference's sphere), range = |p - camera_pos|.
 * The arithmetic is f64 throughout -- the f32 tile transform, height, camera_proj and camera_pos are widened and taken as exact --
 * so the answer does not share the frame depth's error (topo_dist_from_depth(depth) is only good to about 2 / w: hundreds of metres
 * of range at 20 km).  The point may lie marginally outside its triangle (the rasteriser snaps vertices to 1/256 px); a piece of a
 * near-clipped triangle (fan) answers with its original triangle's plane.  w1, w2: the plane's barycentric weights of the
 * triangle's second and third vertex (index-buffer order).  Errors, stream order and tile changes are those of the horizon calls:
 * TOPO_ERR_INVALID when nothing was rendered yet, for a view or pixel outside the submission and once tiles were added, replaced or
 * unloaded after it; TOPO_ERR_CAPACITY, once, from the host read of a submission that overflowed its rare-triangle queue.  The
 * queries write nothing but their outputs. */
typedef struct topo_ground_point {       /* 64 bytes; written as 16-byte stores */
    double lon_deg, lat_deg;
    float height_m, range_m;             /* the f64 values rounded once */
    float depth;                         /* the key's depth = the frame's depth output at the pixel; 1.0 for sky */
    int32_t kind;                        /* TOPO_GROUND_*; every other field of a sky / incomplete / outside record is 0 (sky: depth 1.0) */
    int32_t tile_lat_deg, tile_lon_deg;  /* tile of the winning triangle */
    uint32_t cell_x, cell_y;             /* its cell: viewshed / horizon numbering */
    uint32_t tri, fan;                   /* tri = triangle & 1 (index-buffer order within the cell); fan = piece of a near-clipped triangle */
    float w1, w2;
} topo_ground_point;
#define TOPO_GROUND_TERRAIN 1
#define TOPO_GROUND_SKY 0
#define TOPO_GROUND_OUTSIDE (-1)         /* device list only: the query names a view or pixel outside the submission (nothing was read) */
#define TOPO_GROUND_INCOMPLETE (-2)      /* device list only: the submission overflowed its rare-triangle queue */
#define TOPO_GROUND_DEGENERATE (-3)      /* no finite point: a void (non-finite) vertex height or a vanishing determinant; the tile, cell,
                                          * triangle and depth are still reported, the position and weights are 0 */
typedef struct topo_ground_query { uint32_t view, x, y, _reserved; } topo_ground_query;
/* Host memory, n queries -> n records; waits for the submission. */
int topo_ground_read(topo_ctx* ctx, uint32_t n, const topo_ground_query* queries, topo_ground_point* out);
/* Device memory (both 16-byte aligned); asynchronous: queued on the stream that submission ran on, behind it. */
int topo_ground_device(topo_ctx* ctx, uint32_t n, const topo_ground_query* queries_dev, topo_ground_point* out_dev);
/* The dense form: for every pixel of views [first_view, first_view + n_views) a float4 (lon_deg, lat_deg, height_m, range_m), each the
 * f64 result rounded once to f32 -- bit for bit (float) of what the list calls report -- view i at out_dev + i * view_stride_bytes,
 * rows pitch_bytes apart (device memory; pointer and strides multiples of 16; bytes between rows and views are left alone).  Pixels
 * without a terrain point (sky, degenerate, incomplete submission) get four quiet NaNs.  f32 longitude is good to about 0.85 m on
 * the ground at |lon| >= 128 degrees (half that below 128, and so on); the list calls give f64.  Asynchronous, as topo_ground_device. */
int topo_ground_map_device(topo_ctx* ctx, uint32_t first_view, uint32_t n_views, float* out_dev, size_t view_stride_bytes, size_t pitch_bytes);

/* ---- rays: line of sight over the resident tiles -------------------------------------------------------------------------------
 * "Can the summit at B be seen from the hut at A?"  A ray p(t) = origin + t * dir (f64 ECEF metres, the frame of
 * topo_geometry_transform; dir need not be unit: with dir = B - A, t in [0, 1] is the segment from A to B) against every triangle of
 * every resident tile -- the triangles the renderer draws: the vertices of the ground queries (the f32 tile transform and height
 * widened, f64 from there on), the index-buffer topology, both faces.  A triangle with a non-finite vertex height does not exist;
 * finite sentinel heights are geometry, as in the frame.  The test is Moeller-Trumbore in f64 on vertices translated by the origin:
 * hit iff u >= 0, v >= 0, u + v <= 1, t_min <= t <= t_max and t finite.  The hit reported is the one with the smallest t; on equal t
 * the tile that comes first in draw order, then the lower triangle index.  front = 1 when the ray meets the side the renderer
 * draws (N . dir < 0 with N = (v1 - v0) x (v2 - v0)).  A ray with a non-finite origin or direction component, a zero dir or
 * !(t_min <= t_max) is TOPO_RAY_INVALID; infinite bounds are allowed.  An endpoint that lies ON the terrain touches its own triangle
 * at t = 0 (or 1) within rounding: for "is B visible from A" lift the endpoints off the ground or keep t_min / t_max short of them.
 * The calls read the resident tiles only and need no submission; they run on the context's stream (topo_set_stream) behind whatever
 * was queued there, and write nothing but their outputs.  With no tiles every valid ray misses; n = 0 is a no-op.
 * TOPO_ERR_INVALID for null or misaligned pointers. */
typedef struct topo_ray { double origin[3]; double dir[3]; double t_min, t_max; } topo_ray;      /* 64 bytes */
typedef struct topo_ray_hit {            /* 64 bytes; written as 16-byte stores */
    double t;                            /* hit point = origin + t * dir */
    double lon_deg, lat_deg;             /* of the hit point, as topo_ground_point defines them */
    float height_m;                      /* |p| - R0, the f64 value rounded once */
    int32_t kind;                        /* TOPO_RAY_*; every other field is 0 unless TOPO_RAY_HIT */
    int32_t tile_lat_deg, tile_lon_deg;  /* tile of the triangle hit */
    uint32_t cell_x, cell_y;             /* its cell: viewshed / horizon / ground numbering */
    uint32_t tri, front;                 /* tri = triangle & 1 (index-buffer order within the cell) */
    float w1, w2;                        /* Moeller-Trumbore u, v: the weights of the triangle's second and third vertex */
} topo_ray_hit;
#define TOPO_RAY_HIT 1
#define TOPO_RAY_MISS 0
#define TOPO_RAY_INVALID (-1)
/* Host memory, n rays -> n records; waits. */
int topo_raycast_read(topo_ctx* ctx, uint32_t n, const topo_ray* rays, topo_ray_hit* out);
/* Device memory (both 16-byte aligned); asynchronous on the context's stream. */
int topo_raycast_device(topo_ctx* ctx, uint32_t n, const topo_ray* rays_dev, topo_ray_hit* out_dev);
/* The first application: a lit / shadowed layer for views [first_view, first_view + n_views) of the latest submission (as the
 * horizon and ground calls define it; their errors, stream order and handling of an overflowed submission), one byte per pixel:
 * view i at out_dev + i * view_stride_bytes, rows pitch_bytes apart (device memory; pitch >= width, bytes between width and the
 * pitch are left alone).  sun_dir points TOWARDS the sun (topo_uniforms.sun_direction widened, or topo_sun_direction) and is
 * normalised in f64; zero or non-finite: TOPO_ERR_INVALID.  Per pixel: the ground point exactly as topo_ground_map_device finds it,
 * its three barycentric weights clamped to >= 0 and renormalised so that it lies on the pixel's own triangle T0 (a piece of a
 * near-clipped triangle answers with its original triangle); TOPO_SUN_AWAY if N(T0) . sun <= 0; otherwise the ray from that point
 * along sun against every triangle except T0, a hit counting for 1e-3 m < t <= 1e6 m: any hit TOPO_SUN_SHADOW, none TOPO_SUN_LIT.
 * The frame path shades with sun_direction but casts no shadows; this layer is what it leaves out.  Asynchronous. */
#define TOPO_SUN_NONE 0     /* no terrain point: sky, degenerate, incomplete submission */
#define TOPO_SUN_LIT 1
#define TOPO_SUN_AWAY 2     /* the pixel's own triangle faces away from the sun: N . sun <= 0 */
#define TOPO_SUN_SHADOW 3   /* faces the sun, other terrain is in the way */
int topo_sunlit_map_device(topo_ctx* ctx, uint32_t first_view, uint32_t n_views, const double sun_dir[3], uint8_t* out_dev, size_t view_stride_bytes,
                           size_t pitch_bytes);
/* Host helper, f64, no GPU: the unit ECEF direction at azimuth az_deg (clockwise from true north) and elevation el_deg over the
 * horizontal plane of the point at (lon_deg, lat_deg), in the east / north / up frame of topo_pixel_angles and topo_unwrap_device
 * (up = the geocentric radius).  The direction towards the sun for a ray from the ground, for one. */
void topo_sun_direction(double lon_deg, double lat_deg, double az_deg, double el_deg, double dir_out[3]);

/* ---- surface: the drawn terrain under a longitude and latitude -- points, grids and profiles -----------------------------------
 * "How high is the drawn terrain at this longitude and latitude?"  The mesh is that of the rays.  A triangle exists for these
 * queries iff each of its three vertex heights is finite, < 1e9 and > -R0 (only then does every vertex lie over its own longitude
 * and latitude); finite sentinel heights are geometry, as in the frame.  For the unit direction u of (lon, lat) the line is
 * origin R0 u, direction u, so that t is the height over the sphere.  The test is that of the rays on vertices translated by the
 * origin, with TOLERANT edges: hit iff u >= -e, v >= -e, u + v <= 1 + e with e = 2^-30, t finite and -R0 < t < 1e9 -- interior
 * edges and vertices are watertight, and a point at an exact DEM post on the mesh border has terrain.  Among all triangles of all
 * resident tiles the LARGEST t is reported (the surface seen from above); on equal t the tile that comes first in draw order, then
 * the lower triangle index.  Tiles may overlap or leave gaps; the columns of a tile are taken to lie within 180 degrees of its
 * model point, and a tile whose pixel scale is zero or not finite in x or y has no surface.  slope_deg is the angle between the triangle's normal n = (v1 - v0) x (v2 - v0), turned to the side of u, and u;
 * aspect_deg the azimuth, clockwise from true north in [0, 360), of the horizontal part of that normal -- the downslope direction
 * -- in the east / north / up frame of topo_sun_direction at the point, 0 where it vanishes.
 * A point is valid iff lon and lat are finite and |lat| <= 90; any finite lon wraps, and at |lat| = 90 the given lon picks the
 * column.  An invalid point is TOPO_SURFACE_INVALID; a valid point outside every tile, in a gap or over a void is TOPO_SURFACE_NONE.
 * The calls read the resident tiles only and need no submission; they run on the context's stream (topo_set_stream) behind whatever
 * was queued there, and write nothing but their outputs.  With no tiles every valid point is NONE; n = 0 is a no-op.
 * TOPO_ERR_INVALID for null or misaligned pointers. */
typedef struct topo_surface_point {      /* 48 bytes; written as three 16-byte stores */
    double height_m;                     /* t: the height over the sphere of radius R0 */
    float slope_deg, aspect_deg;
    int32_t kind;                        /* TOPO_SURFACE_*; every other field is 0 unless TOPO_SURFACE_TERRAIN */
    int32_t tile_lat_deg, tile_lon_deg;  /* tile of the triangle */
    uint32_t cell_x, cell_y, tri;        /* its cell and triangle: viewshed / horizon / ground / ray numbering */
    float w1, w2;                        /* u, v: the weights of the triangle's second and third vertex */
} topo_surface_point;
#define TOPO_SURFACE_TERRAIN 1
#define TOPO_SURFACE_NONE 0
#define TOPO_SURFACE_INVALID (-1)
/* Host memory, n (lon, lat) pairs in degrees -> n records; waits. */
int topo_surface_read(topo_ctx* ctx, uint32_t n, const double* lonlat_deg, topo_surface_point* out);
/* Device memory (both 16-byte aligned); asynchronous on the context's stream. */
int topo_surface_device(topo_ctx* ctx, uint32_t n, const double* lonlat_dev, topo_surface_point* out_dev);
/* The dense form: the f32 height -- (float) of what the list calls report, bit for bit -- at lon0 + c * dlon, lat0 + r * dlat (one
 * rounded product, one rounded sum) for c < nx, r < ny at out_dev + r * pitch_bytes + 4 * c (device memory; pointer and pitch
 * multiples of 4; the bytes between nx and the pitch are left alone); a quiet NaN where there is no terrain or the point is
 * invalid.  dlon and dlat may be negative or zero.  TOPO_ERR_INVALID also for a zero nx or ny, non-finite parameters and
 * ceil(nx / 64) * ny >= 2^32.  Asynchronous. */
int topo_surface_grid_device(topo_ctx* ctx, double lon0_deg, double lat0_deg, double dlon_deg, double dlat_deg, uint32_t nx, uint32_t ny, float* out_dev,
                             size_t pitch_bytes);
/* Profiles: the cross-section under a sight line, the companion of a line-of-sight answer.  A segment is a topo_ray with finite
 * t_min and t_max (otherwise, or if the ray is invalid, the segment is TOPO_SURFACE_INVALID: a zero summary, NaN samples).  Sample
 * k of m lies at t_k = t_min + (t_max - t_min) * (k / (m - 1)), p = origin + t_k * dir, every step rounded in f64; the terrain is
 * looked up under p / |p|, and line = |p| - R0.  A sample is the pair (terrain, line), each rounded once to f32, terrain a quiet NaN
 * where there is none; its clearance is the f32 difference line - terrain of the values as stored.  The summary is the smallest
 * clearance over the samples that have terrain, on equal values the lowest sample index; with no sample over terrain
 * min_clearance_m is a quiet NaN, min_sample 0xFFFFFFFF and kind TOPO_SURFACE_NONE.  The profile says BY HOW MUCH a line clears the
 * terrain AT ITS SAMPLES; exact line of sight remains topo_raycast_*.  2 <= m <= 65536, n * m < 2^31. */
typedef struct topo_profile_summary { float min_clearance_m; uint32_t min_sample; uint32_t n_terrain; int32_t kind; } topo_profile_summary;      /* 16 bytes, one store */
/* Device memory: segs_dev and summary_dev 16-byte aligned; samples_dev null, or 8-byte aligned: segment i's m pairs at samples_dev
 * + i * segment_stride_bytes (a multiple of 8, at least 8 * m; the bytes behind a segment's samples are left alone).  Asynchronous. */
int topo_profile_device(topo_ctx* ctx, uint32_t n, const topo_ray* segs_dev, uint32_t m, float* samples_dev, size_t segment_stride_bytes,
                        topo_profile_summary* summary_dev);
/* Host memory: samples null, or n * m pairs, densely packed; waits. */
int topo_profile_read(topo_ctx* ctx, uint32_t n, const topo_ray* segs, uint32_t m, float* samples, topo_profile_summary* summary);

/* ---- visibility: what an observer sees, as a map or over a list ------------------------------------------------------------------
 * "From this hut, which ground can be seen?"  "Which of these 5000 peaks are in sight from here?" -- without a rendered frame, its
 * pixels or its field of view.  No new geometry: a point is found on the drawn terrain exactly as topo_surface_* finds it, and the
 * sight line is tested exactly as the shadow ray of topo_sunlit_map_device is.
 * Observer.  u is the unit direction of (lon_deg, lat_deg); with TOPO_OBSERVER_ABOVE_TERRAIN in flags height_m is measured above
 * the drawn terrain under the point (base = the height topo_surface_* reports there), otherwise above the sphere R0 (base = 0);
 * O = ((R0 + base) + height_m) u.  An observer is UNUSABLE when its point is invalid (as topo_surface_* defines it), its height is
 * not finite, or the flag is set and no terrain lies under it: each of its targets is TOPO_VIS_NO_OBSERVER.
 * Target.  A point (lon, lat) and the call's target_height_m (finite, 0 <= h <= 1e5, else TOPO_ERR_INVALID).  An invalid point or one
 * with no terrain under it is TOPO_VIS_NONE; otherwise T = ((R0 + t) + h) u with t and the triangle from the surface rule.
 * Class.  D = O - T, L = |D|, d = D / L.  (1) !(L > 2e-3 m): the observer sits at the target, TOPO_VIS_VISIBLE.  (2) Only for h == 0:
 * with N = (v1 - v0) x (v2 - v0) of the target's triangle, turned to the side of u, !(N . D > 0) is TOPO_VIS_AWAY -- the ground itself
 * faces away.  (3) The ray from T along d against the triangles of the rays, a hit counting for 1e-3 m < t <= L: any hit
 * TOPO_VIS_HIDDEN, none TOPO_VIS_VISIBLE.  For h == 0 the target's own triangle does not count; for h > 0 every triangle does (a mast
 * on a back slope can be hidden by its own slope).  The answer is a function of the observer, the target and the tile set.
 * The calls read the resident tiles only and need no submission; they run on the context's stream (topo_set_stream) behind whatever
 * was queued there, and write nothing but their outputs.  observers is HOST memory, read before the call returns;
 * n_observers <= 64, and zero observers (or n = 0) is a no-op.  TOPO_ERR_INVALID for null pointers, more than 64 observers and a
 * target height out of range. */
typedef struct topo_observer { double lon_deg, lat_deg, height_m; uint32_t flags; uint32_t _reserved; } topo_observer;      /* 32 bytes */
#define TOPO_OBSERVER_ABOVE_TERRAIN 1u
#define TOPO_VIS_NONE 0          /* no terrain under the target, or an invalid point */
#define TOPO_VIS_VISIBLE 1
#define TOPO_VIS_AWAY 2          /* h == 0 only: the target's own triangle faces away from the observer */
#define TOPO_VIS_HIDDEN 3        /* other terrain is in the way */
#define TOPO_VIS_NO_OBSERVER 4   /* the observer is unusable */
/* The dense form: one byte per (observer o, row r, column c) at out_dev + o * layer_stride_bytes + r * pitch_bytes + c for the target
 * at lon0 + c * dlon, lat0 + r * dlat (one rounded product, one rounded sum, as topo_surface_grid_device) -- the byte the list call
 * gives for the same numbers.  Device memory, no alignment; the bytes between nx and the pitch and between layers are left alone.
 * dlon and dlat may be negative or zero.  TOPO_ERR_INVALID also for a zero nx or ny, non-finite grid parameters, pitch_bytes < nx,
 * layer_stride_bytes < ny * pitch_bytes and ceil(nx / 64) * ny * n_observers >= 2^32.  Asynchronous. */
int topo_visibility_grid_device(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, double lon0_deg, double lat0_deg, double dlon_deg, double dlat_deg,
                                uint32_t nx, uint32_t ny, double target_height_m, uint8_t* out_dev, size_t layer_stride_bytes, size_t pitch_bytes);
/* The list form: n (lon, lat) pairs in degrees at lonlat_dev (device memory, 16-byte aligned) -> out_dev[o * list_stride_bytes + i]
 * (device memory; list_stride_bytes >= n, the bytes behind a list are left alone).  Asynchronous. */
int topo_visibility_device(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_dev, double target_height_m,
                           uint8_t* out_dev, size_t list_stride_bytes);
/* Host memory: n pairs in, out[o * n + i]; waits. */
int topo_visibility_read(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_deg, double target_height_m, uint8_t* out);
/* Host helper, f64, no GPU: the ECEF point (R0 + height_m) u of (lon_deg, lat_deg) in the frame of the rays -- an endpoint of a
 * topo_ray, or the O and T above. */
void topo_ecef_from_lonlat(double lon_deg, double lat_deg, double height_m, double out[3]);

/* ---- refracted visibility: sight lines bent by atmospheric refraction ------------------------------------------------------------
 * The sight lines above are straight segments over a spherical Earth.  Surveyors, radio planners and viewshed tools apply the
 * standard refraction correction instead: with coefficient k (0.13 in the standard atmosphere; GDAL's viewshed calls it -cc 0.857 =
 * 1 - k), terrain at distance s from the observer appears raised by k s^2 / (2 R0) -- 1 m at 10 km, 100 m at 100 km, 400 m at 200 km.
 * The rule.  The refracted query of observer O with coefficient refraction_k is the visibility query above on the mesh LIFTED for O:
 * every vertex v keeps its direction and gains radius, v' = v + (c |v - O|^2 / |v|) v with c = k / (2 R0) and |v - O| the f64 chord
 * from the unlifted vertex to O; O itself is resolved on the unlifted mesh, exactly as above.  Everything else is the rule above on
 * the lifted vertices: the target lies on the lifted mesh, AWAY uses the lifted triangle's normal, target_height_m is added on top,
 * the sight line runs from T to O with the same bounds and the same skipped triangle; the classes are the same five.
 * refraction_k == 0 gives the bytes of topo_visibility_*, bit for bit.  Each call takes the arguments of its plain counterpart plus
 * refraction_k, and follows its contract (at most 64 observers, the no-ops, the strides, asynchrony, nothing written but the
 * outputs); TOPO_ERR_INVALID also for a refraction_k that is not finite or lies outside 0 <= k < 1.
 * Skyline, sun exposure, rays and rendered frames stay unrefracted. */
#define TOPO_REFRACTION_STANDARD 0.13
int topo_visibility_refracted_grid_device(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, double lon0_deg, double lat0_deg, double dlon_deg,
                                          double dlat_deg, uint32_t nx, uint32_t ny, double target_height_m, double refraction_k, uint8_t* out_dev,
                                          size_t layer_stride_bytes, size_t pitch_bytes);
int topo_visibility_refracted_device(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_dev, double target_height_m,
                                     double refraction_k, uint8_t* out_dev, size_t list_stride_bytes);
int topo_visibility_refracted_read(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_deg, double target_height_m,
                                   double refraction_k, uint8_t* out);
/* Host helper, f64, no GPU: out = point lifted for `observer` with coefficient k (ECEF metres, the frame of topo_ecef_from_lonlat) --
 * for callers who place their own objects in the refracted scene.  out may be point.  TOPO_ERR_INVALID for a null pointer or a k
 * outside 0 <= k < 1 (out is left alone). */
int topo_refraction_lift(const double observer[3], const double point[3], double k, double out[3]);

/* ---- skyline: the terrain horizon by azimuth from any point ----------------------------------------------------------------------
 * "How high does the terrain stand above the horizontal in each direction from here, and which ridge forms that line?" -- solar
 * access, radio horizon, ridge labels, the vertical extent of a panorama -- without a rendered frame, its rows or its field of view.
 * Observer.  A topo_observer, resolved exactly as for the visibility queries: O, rho = |O|.  The frame at O is that of
 * topo_pixel_angles and topo_unwrap_device: up = O / rho, east = z x up normalised, north = up x east.  An unusable observer, and one
 * whose east does not come out finite and non-zero (on the polar axis), is TOPO_SKY_NO_OBSERVER for all its azimuths.
 * Azimuth k of n_az is a_k = az0_deg + k * daz_deg (one rounded product, one rounded sum), clockwise from north;
 * h = cos a north + sin a east, m = h x up (to the observer's right).  daz may be negative or zero.
 * Crossing.  The mesh is that of the rays, with their rule of existence: a triangle exists iff its three vertex heights are finite.
 * For each edge of each existing triangle -- edge e joins vertices e and (e + 1) % 3 in index-buffer order -- with the endpoints in
 * canonical order (the lower vertex index y * w + x first) and translated by O: da = m . a, db = m . b; the edge crosses the plane iff
 * (da < 0) != (db < 0); X = a + (da / (da - db)) (b - a), s = h . X, z = up . X; the crossing counts iff min_range_m <= s <= max_range_m.
 * Winner.  The largest z / s; then the smaller s, the tile that comes first in draw order, the lower triangle index, the lower edge.
 * The answer is a function of the observer, the azimuth and the tile set.  Along a straight segment the elevation angle is monotone, so
 * the crossings carry the highest point of every triangle's cut: elevation_deg IS the terrain's horizon within the range limits.
 * No crossing: TOPO_SKY_NONE.  Both TOPO_SKY_NONE and TOPO_SKY_NO_OBSERVER report a quiet NaN elevation and 0 in every other field.
 * The calls read the resident tiles only and need no submission; they run on the context's stream (topo_set_stream) behind whatever
 * was queued there, and write nothing but their outputs.  observers is HOST memory, read before the call returns; n_observers <= 64;
 * zero observers or n_az = 0 is a no-op.  TOPO_ERR_INVALID for null or misaligned pointers, more than 64 observers, strides too small,
 * a non-finite az0, daz or range, anything but 0 < min_range_m <= max_range_m <= 1e6, no output at all and n_az * n_observers >= 2^32. */
typedef struct topo_skyline_sample {     /* 64 bytes; written as four 16-byte stores */
    double elevation_deg, range_m;       /* atan2(z, s) in degrees; |X|.  s = range cos(elevation), z = range sin(elevation) */
    double lon_deg, lat_deg;             /* of the crossing point O + X, as topo_ray_hit defines them */
    float height_m; int32_t kind;        /* |O + X| - R0, the f64 value rounded once; TOPO_SKY_* */
    int32_t tile_lat_deg, tile_lon_deg;  /* tile of the winning edge's triangle (named as in topo_ray_hit) */
    uint32_t cell_x, cell_y;             /* its cell: viewshed / horizon / ground / ray numbering */
    uint32_t tri, edge;                  /* tri = triangle & 1; edge 0, 1, 2 */
} topo_skyline_sample;
#define TOPO_SKY_NONE 0
#define TOPO_SKY_TERRAIN 1
#define TOPO_SKY_NO_OBSERVER 4           /* = TOPO_VIS_NO_OBSERVER */
/* Device memory, each output nullable, at least one given: observer o's n_az f32 elevations -- (float) of the record's elevation_deg,
 * bit for bit -- at elevation_dev + o * observer_stride_bytes (pointer and stride multiples of 4, stride >= 4 * n_az), its n_az records
 * at samples_dev + o * samples_stride_bytes (multiples of 16, stride >= 64 * n_az); the bytes between n_az entries and a stride are
 * left alone.  Asynchronous. */
int topo_skyline_device(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m,
                        double max_range_m, float* elevation_dev, size_t observer_stride_bytes, topo_skyline_sample* samples_dev, size_t samples_stride_bytes);
/* Host memory, each output nullable, at least one given: elevation[o * n_az + k], samples[o * n_az + k]; waits. */
int topo_skyline_read(topo_ctx* ctx, uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m,
                      double max_range_m, float* elevation, topo_skyline_sample* samples);

/* ---- sun exposure: a day of sun and shadow over points of the drawn terrain, as a map or over a list ---------------------------------
 * "How many hours of sun does this slope get on 21 December?"  "When does the north face come out of the shade?" -- without a rendered
 * frame: topo_sunlit_map_device covers one sun and the pixels of rendered views.  No new geometry: a point is found on the drawn terrain
 * exactly as topo_surface_* finds it, and the shadow ray is tested exactly as that of topo_sunlit_map_device is.
 * Suns.  Up to 64 per call, HOST memory, read before the call returns.  dir points TOWARDS the sun -- one ECEF direction for the whole
 * call, the sun being at infinity, as sun_dir of topo_sunlit_map_device; topo_sun_direction makes one from an azimuth and an elevation --
 * and is normalised in f64 as that call normalises sun_dir.  weight is finite and >= 0: minutes per sample, say, or minutes times
 * direct-normal irradiance.
 * Target.  A point (lon, lat), found as a visibility target with target_height_m == 0 is: an invalid point or one with no terrain under
 * it is NONE; otherwise T = (R0 + t) u with t and the triangle from the surface rule, and N = (v1 - v0) x (v2 - v0) of that triangle,
 * turned to the side of u.
 * Class of (target, sun s), in this order.  (1) !(u . s > 0): TOPO_SUN_NIGHT -- the sun is on or below the point's own horizontal plane.
 * The sphere is not geometry and a mosaic is finite: without this step a set sun would light every slope near the mosaic's edge.  The
 * dip of the horizon is IGNORED: from a summit the sun is seen a degree or two below that plane, and is night here.  (2) !(N . s > 0):
 * TOPO_SUN_AWAY.  (3) The ray from T along s against the triangles of the rays, a hit counting for 1e-3 m < t <= 1e6 m, the target's
 * own triangle left out: any hit TOPO_SUN_SHADOW, none TOPO_SUN_LIT.
 * Outputs per target, each nullable, at least one given.  lit: bit k is set iff sun k is LIT.  shadow: bit k is set iff sun k is SHADOW,
 * that is, cast by other terrain; AWAY and NIGHT set neither bit.  exposure: the sum, in ascending k over the LIT suns, of
 * weight_k * (N . s_k) / |N|, formed in f64 and rounded once to f32; 0 for terrain that is never lit, a quiet NaN for NONE, whose masks
 * are both 0.  The answer is a function of the target, the sun and the tile set: a sun's bit does not depend on the other suns of the
 * call or on its position among them.
 * The calls read the resident tiles only and need no submission; they run on the context's stream (topo_set_stream) behind whatever
 * was queued there, and write nothing but their outputs.  Zero suns (or n = 0) is a no-op.  TOPO_ERR_INVALID for a null suns, more than
 * 64 suns, a zero or non-finite dir, a non-finite or negative weight, no output at all and misaligned pointers. */
typedef struct topo_sun { double dir[3]; double weight; } topo_sun;      /* 32 bytes */
#define TOPO_SUN_NIGHT 4         /* the sun is on or below the target's horizontal plane (after TOPO_SUN_NONE .. TOPO_SUN_SHADOW) */
/* The dense form: the target at lon0 + c * dlon, lat0 + r * dlat (one rounded product, one rounded sum, as topo_visibility_grid_device)
 * for c < nx, r < ny has its masks at lit_dev / shadow_dev + r * mask_pitch_bytes + 8 * c (pointers and pitch multiples of 8, the pitch
 * >= 8 * nx) and its exposure at exposure_dev + r * exposure_pitch_bytes + 4 * c (multiples of 4, the pitch >= 4 * nx) -- what the list
 * call gives for the same numbers.  Device memory; the bytes between nx and a pitch are left alone.  dlon and dlat may be negative or
 * zero.  TOPO_ERR_INVALID also for a zero nx or ny, non-finite grid parameters, a pitch too small and ceil(nx / 64) * ny >= 2^32.
 * Asynchronous. */
int topo_sun_exposure_grid_device(topo_ctx* ctx, uint32_t n_suns, const topo_sun* suns, double lon0_deg, double lat0_deg, double dlon_deg, double dlat_deg, uint32_t nx,
                                  uint32_t ny, uint64_t* lit_dev, uint64_t* shadow_dev, float* exposure_dev, size_t mask_pitch_bytes, size_t exposure_pitch_bytes);
/* The list form: n (lon, lat) pairs in degrees at lonlat_dev (device memory, 16-byte aligned) -> lit_dev[i], shadow_dev[i] (8-byte
 * aligned), exposure_dev[i] (4-byte aligned).  Asynchronous. */
int topo_sun_exposure_device(topo_ctx* ctx, uint32_t n_suns, const topo_sun* suns, uint32_t n, const double* lonlat_dev, uint64_t* lit_dev, uint64_t* shadow_dev,
                             float* exposure_dev);
/* Host memory: n pairs in, lit[i], shadow[i], exposure[i]; waits. */
int topo_sun_exposure_read(topo_ctx* ctx, uint32_t n_suns, const topo_sun* suns, uint32_t n, const double* lonlat_deg, uint64_t* lit, uint64_t* shadow, float* exposure);

/* ---- peak labels: the peaks an image shows, laid out in rows -- per view or per strip, a whole submission in one call -----------------
 * Steps 1 and 2 of the reference's labelled panorama: get_visible_labels (render_engine.rs:338-396) and layout_labels /
 * process_label_layout (text_renderer.rs:300-372).  Tessellating leader lines and backgrounds and shaping text stay the host's; the
 * lines and glyphs are drawn by topo_overlay_lines* / topo_overlay_glyphs*.
 * Image.  views_per_image consecutive views of width x height, side by side: columns 0 .. Wi - 1, Wi = views_per_image * width.  1 is
 * the reference's single frame, 8 a panorama strip, laid out as the one image the viewer sees: labels do not collide across a sector
 * seam.  There is no wrap-around at 360 degrees.
 * Candidate.  For image i and peak p (ECEF f32 xyz) the image's views are taken in ascending order; the first view v in which the peak
 * passes the test of topo_visible_peaks -- through that view's camera_proj, against that view's depth -- makes it a candidate at
 * peak_x = v * width + x_pos, peak_y = y_pos.
 * Layout.  Candidates are taken in ascending peak index: the caller's array order is the priority order (the reference iterates a
 * BTreeMap, then each location's peaks).  w = widths[p]; a w that is not finite or < 0 is never labelled.  Else l = peak_x,
 * r = min(sat_u32(ceil((float)peak_x + w)), Wi - 1) -- f32 sum and ceil, sat_u32 Rust's `as u32` -- and the label takes the lowest
 * row k < max_rows in which no column of the closed range [l, r] is taken, and takes those columns there; touching counts as overlap.
 * No free row: visible but unlabelled.  label_x = (float)peak_x, label_y = row_height * (0.5f + (float)k) (the reference passes
 * LINE_HEIGHT + LINE_PADDING = 20), label_width = w.  csrc/topo_labels.h argues why this grid decides as the reference's sorted edge
 * sets do.
 * Limits.  TOPO_ERR_UNSUPPORTED for max_rows > 64 or Wi * max_rows > 524288: the occupancy grid of one image is at most 64 KiB of
 * bits (a 16384-column strip with the reference's 8 rows takes 16 KiB). */
typedef struct topo_label { uint32_t peak, view, row; float label_x, label_y, label_width, peak_x, peak_y; } topo_label; /* 32 bytes = LabelLayout */
typedef struct topo_label_params { float row_height; uint32_t max_rows; uint32_t views_per_image; uint32_t cap; } topo_label_params; /* 16 bytes */
/* The layout rule alone, on the host, for positions already known: n labels at columns x[j] < image_width with widths[j].  row_out[j]
 * is the row, -1 for no row free, -2 for an unusable width; out (nullable, room for n) receives the placed labels in order with
 * peak = j, view = 0, peak_y = 0.  Returns the number placed, or TOPO_ERR_INVALID (a null pointer with n > 0, image_width or max_rows
 * of 0, an x[j] >= image_width) or TOPO_ERR_UNSUPPORTED (the limits above).  Pure: no context, no GPU. */
int topo_label_layout(uint32_t n, const uint32_t* x, const float* widths, uint32_t image_width, float row_height, uint32_t max_rows, int32_t* row_out, topo_label* out);
/* Over whole submissions, on the device: n_views views (HOST memory, read before the call returns; only camera_proj is read) of
 * width x height whose depth is at depth_dev + v * depth_view_stride, rows depth_pitch apart (bytes) -- for example the arguments of
 * the topo_render_views_device, topo_render_panorama or topo_render_batch call before it (topo_render_batch: n_views = 8 n,
 * views_per_image = 8).  n_views must be a multiple of params->views_per_image; the images number n_views / views_per_image.  Peaks
 * (3 n_peaks floats) and widths (n_peaks floats) are device memory.  Image i writes its labels in placement order to labels_dev +
 * i * cap, only the first cap of them; counts_dev[i] is the number placed, whether or not they fitted in cap; state_dev (nullable)
 * [i * n_peaks + p] is 0 not visible, 1 labelled, 2 visible without a free row, 3 visible with an unusable width.
 * Asynchronous on the context's stream (topo_set_stream), in order behind whatever was queued there, as topo_visible_peaks_device;
 * touches no frame state and needs no tile.  TOPO_ERR_INVALID for null pointers, max_rows == 0, views_per_image == 0, n_views %
 * views_per_image != 0, a width or height of 0, a pitch smaller than a row or a view stride smaller than a view, and misaligned
 * pointers, pitches or strides (4 bytes). */
int topo_labels_device(topo_ctx* ctx, const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t width, uint32_t height,
                       const float* depth_dev, size_t depth_view_stride, size_t depth_pitch, uint32_t n_peaks, const float* peaks_xyz_dev, const float* widths_dev,
                       topo_label* labels_dev, uint32_t* counts_dev, uint8_t* state_dev);
/* The same with host memory for the peaks, the widths and the outputs; the depth stays a device pointer.  Waits. */
int topo_labels_read(topo_ctx* ctx, const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t width, uint32_t height,
                     const float* depth_dev, size_t depth_view_stride, size_t depth_pitch, uint32_t n_peaks, const float* peaks_xyz, const float* widths,
                     topo_label* labels, uint32_t* counts, uint8_t* state);

/* ---- summits: the peaks of the drawn mesh by isolation, and snapping given peaks to them ----------------------------------------------
 * "Which peaks does this DEM hold?" -- a peak list for topo_visibility_*, topo_labels_* and topo_visible_peaks with nothing fetched --
 * and "where is this database peak on the mesh that is drawn?": surveyed peaks sit a few posts off the DEM's own summit and tens of
 * metres above or below it.  csrc/topo_summits.h states the rule and argues the search; in short:
 * Posts.  A post is vertex (vx, vy) of a resident tile; it exists iff its tile's pixel scale is finite and not zero both ways and its
 * height is finite, < 1e9 and > -R0 (topo_surface_*'s rule).  lon_deg / lat_deg are where the mesh puts the vertex.  The distance of two
 * posts is the chord R0 |u_a - u_b| of their directions.  Q DOMINATES P iff it is higher, or equally high and earlier in (tile draw
 * order, vy * w + vx).  The ISOLATION of P is the distance to the nearest post that dominates it among the resident posts within
 * radius_m, +inf if there is none; P is a summit iff height_m >= min_height_m and isolation >= min_isolation_m.  Only resident posts
 * count: near the mosaic's border an isolation is an upper bound.  A plateau has one summit, its first post; of posts duplicated by
 * overlapping tiles only the earlier tile's is one (min_isolation_m > 0).
 * radius_m is finite, > 0 and <= 1e6; 0 <= min_isolation_m <= radius_m; min_height_m is not NaN (-inf: no limit); anything else, a
 * null or misaligned pointer (16 bytes for records and points, 4 for the count) and an unknown order are TOPO_ERR_INVALID with nothing
 * written.  The calls need no submission; they run on the context's stream (topo_set_stream) behind whatever was queued there.  A context
 * with no tiles is a successful no-op: the count is 0. */
typedef struct topo_summit_params { double radius_m, min_isolation_m; float min_height_m; uint32_t order; } topo_summit_params;   /* 24 bytes */
#define TOPO_SUMMIT_ORDER_TILE 0u       /* ascending (tile rank, vy * w + vx): the device order */
#define TOPO_SUMMIT_ORDER_HEIGHT 1u     /* height descending, ties in tile order            (read only) */
#define TOPO_SUMMIT_ORDER_ISOLATION 2u  /* isolation descending (+inf first), then height   (read only) */
typedef struct topo_summit {            /* 64 bytes; written as four 16-byte stores */
    double lon_deg, lat_deg, isolation_m;            /* isolation +inf: nothing higher within radius_m */
    float height_m, higher_height_m;                 /* higher_*: the nearest dominator; all 0 when there is none */
    int32_t tile_lat_deg, tile_lon_deg; uint32_t vx, vy;
    int32_t higher_tile_lat_deg, higher_tile_lon_deg; uint32_t higher_vx, higher_vy;
} topo_summit;
typedef struct topo_summit_snap {       /* 48 bytes; written as three 16-byte stores */
    double lon_deg, lat_deg, distance_m; float height_m; int32_t status;   /* 1 found, 0 none, -1 invalid; every other field 0 unless found */
    int32_t tile_lat_deg, tile_lon_deg; uint32_t vx, vy;
} topo_summit_snap;
#define TOPO_SNAP_FOUND 1
#define TOPO_SNAP_NONE 0
#define TOPO_SNAP_INVALID (-1)
/* Device memory.  *count_dev receives the number of summits found, which may exceed capacity; out_dev the first min(count, capacity) in
 * tile order (TOPO_SUMMIT_ORDER_TILE, the only order accepted here); nothing is written past that.  The bytes are a function of the
 * tile set and the parameters alone.  Asynchronous. */
int topo_summits_device(topo_ctx* ctx, const topo_summit_params* params, topo_summit* out_dev, uint32_t capacity, uint32_t* count_dev);
/* Host memory; waits.  The full set is ordered as params->order says, then the first min(count, capacity) are written; *count is the
 * full number.  TOPO_ERR_CAPACITY when count > capacity (the records that fit and *count are still written: size a second call by it). */
int topo_summits_read(topo_ctx* ctx, const topo_summit_params* params, topo_summit* out, uint32_t capacity, uint32_t* count);
/* Snap: for each of n (lon, lat) pairs in degrees the best existing post within radius_m of the point's direction -- the highest; on
 * equal height the nearer, then the earlier in (tile draw order, vy * w + vx).  TOPO_SNAP_NONE: no post in range; TOPO_SNAP_INVALID: a
 * non-finite longitude or a latitude outside +-90.  n == 0 is a no-op.  Device memory, 16-byte aligned; asynchronous. */
int topo_summit_snap_device(topo_ctx* ctx, uint32_t n, const double* lonlat_dev, double radius_m, topo_summit_snap* out_dev);
/* Host memory; waits. */
int topo_summit_snap_read(topo_ctx* ctx, uint32_t n, const double* lonlat_deg, double radius_m, topo_summit_snap* out);

/* ---- map views: relief, contours and the viewshed over any lon/lat grid ---------------------------------------------------------------
 * The picture a panorama viewer puts next to the panorama: the terrain from above, shaded, with height contours and the ground the
 * frames show.  csrc/topo_map.h states the rule and argues the kernel's shortcuts; in short:
 * Pixel (c, r), c < nx, r < ny, lies at lon0 + c * dlon, lat0 + r * dlat (one rounded product, one rounded sum, as
 * topo_surface_grid_device); dlon and dlat may be negative or zero.  Its terrain is what topo_surface_* finds there; a pixel with no
 * terrain or an invalid point is VOID.
 * TOPO_MAP_RELIEF.  The packed normals of the winning triangle's three vertices, unpacked and rotated to world as the frame does for a
 * vertex, interpolated with the f32 weights (1 - u - v, u, v); the linear value is the frame's view_mode 1 shading of that normal under
 * sun_direction (as topo_uniforms.sun_direction; topo_sun_direction(lon_c, lat_c, 315, 45, ...) narrowed to float is the conventional
 * north-west light), 0.01 + 0.7 max(n . sun, 0), without the dither; the grey code g is its sRGB encoding through the frame's table.
 * TOPO_MAP_CONTOURS, with contour_interval_m > 0.  The level of a terrain pixel is floor(height / interval).  A pixel is on a contour
 * iff its level differs from that of its east neighbour (c + 1, r) or its south neighbour (c, r + 1); a neighbour outside the grid or
 * void takes no part.  With index_every = n > 0 it is on an INDEX contour iff for one differing pair a multiple of n lies in (min level,
 * max level].  An interval of 0 switches the layer off.
 * TOPO_MAP_SEEN.  A terrain pixel is seen iff the bit of its winning (tile, cell) is set in the viewshed masks, exactly as
 * topo_viewshed_read reports them; the masks hold every frame queued before the call, on whatever stream it ran (the call joins the
 * frames in flight, as topo_viewshed_read does).  TOPO_ERR_INVALID if accumulation was never enabled.
 * flags: one byte per pixel, TOPO_MAP_FLAG_* (index implies contour); 0 for a void pixel.  rgba: four bytes per pixel, always R G B A
 * in memory: void_rgba for a void pixel; else (g, g, g, 255), g = 255 with the relief layer off; then, if seen, blended with seen_rgba
 * by its alpha, (c * (255 - a) + s * a + 127) / 255 per colour channel in integers; then, on a contour, blended the same way with
 * contour_rgba, or with index_rgba on an index contour.  Alpha stays 255 for terrain.  A layer that is off costs nothing and sets no flag.
 * The calls read the resident tiles only and need no submission; they run on the context's stream (topo_set_stream) behind whatever was
 * queued there and write nothing but their outputs.  With no tiles every pixel is void.
 * Errors: TOPO_ERR_INVALID for null params, misaligned pointers or pitches, a zero nx or ny, non-finite grid parameters or
 * sun_direction, a negative or non-finite interval, unknown layer bits, and ceil(nx / 64) * ny >= 2^32. */
#define TOPO_MAP_RELIEF 1u
#define TOPO_MAP_CONTOURS 2u
#define TOPO_MAP_SEEN 4u
#define TOPO_MAP_FLAG_TERRAIN 1u
#define TOPO_MAP_FLAG_CONTOUR 2u
#define TOPO_MAP_FLAG_INDEX 4u
#define TOPO_MAP_FLAG_SEEN 8u
typedef struct topo_map_params {         /* 88 bytes */
    double lon0_deg, lat0_deg, dlon_deg, dlat_deg;
    double contour_interval_m;
    uint32_t nx, ny;
    uint32_t index_every, layers;        /* layers: TOPO_MAP_RELIEF | TOPO_MAP_CONTOURS | TOPO_MAP_SEEN */
    float sun_direction[3];
    uint8_t void_rgba[4], seen_rgba[4], contour_rgba[4], index_rgba[4];
    uint32_t reserved;
} topo_map_params;
/* Device memory; asynchronous -- except with TOPO_MAP_SEEN, where the call WAITS ON THE HOST for the frames in flight on the contexts' own
 * streams (and, when the tile set or the masks changed since the last frame, for the context's stream) before it queues its kernel.
 * Each output may be NULL; with both NULL the call checks its arguments and does nothing.  Pixel (c, r):
 * four bytes at rgba_dev + r * rgba_pitch + 4 * c (pointer and pitch multiples of 4, pitch >= 4 * nx), one at flags_dev + r *
 * flags_pitch + c (pitch >= nx); the bytes between a row's end and the pitch are left alone. */
int topo_map_device(topo_ctx* ctx, const topo_map_params* params, uint8_t* rgba_dev, size_t rgba_pitch, uint8_t* flags_dev, size_t flags_pitch);
/* The same into host memory, densely packed (4 * nx * ny and nx * ny bytes; each may be NULL); waits. */
int topo_map_read(topo_ctx* ctx, const topo_map_params* params, uint8_t* rgba, uint8_t* flags);
/* The inverse of the pixel positions, to put the observer, a view cone, peaks or a track on the image: for each of n (lon, lat) pairs
 * in degrees the fractional (c, r) = ((lon - lon0) / dlon, (lat - lat0) / dlat) as f64, the longitude taken modulo 360 to within 180
 * degrees of the grid's centre column.  NaN for both of an invalid point (non-finite, |lat| > 90) or params, and for the coordinate
 * whose step is zero.  Pure: no context, no GPU. */
void topo_map_xy(const topo_map_params* params, uint32_t n, const double* lonlat_deg, double* xy_out);

/* ---- unwrap: a strip of perspective views as ONE azimuth / elevation image -------------------------------------------------------
 * A panorama strip is eight 45-degree perspective images: within a sector the azimuth per column goes with atan, the elevation of a
 * row depends on the column, and straight ridges kink at every seam.  topo_unwrap_device resamples finished views -- colour, depth --
 * into one image whose columns are linear in azimuth (clockwise from true north, topo_pixel_angles' frame at the views' common eye:
 * up = eye / |eye|, east = z x up, north = up x east) and whose rows are linear in elevation (TOPO_UNWRAP_EQUIRECTANGULAR) or in
 * tan(elevation) (TOPO_UNWRAP_CYLINDRICAL, the classic printed panorama).
 *
 * Mapping.  Output pixel (c, r) looks along d = cos(el_r) (sin(az_c) east + cos(az_c) north) + sin(el_r) up, with
 * az_c = az0 + (c + 0.5) az_span / out_w and el_r = el_top - (r + 0.5) (el_top - el_bottom) / out_h (cylindrical: tan(el_r) linear
 * between tan(el_top) and tan(el_bottom)).  View k sees d at clip coordinates cx, cy, cw = rows 0, 1, 3 of its camera_proj applied to
 * (d, 0) -- all views must have the same camera_pos, bit for bit, and only the direction part of camera_proj is read -- i.e. at
 * px = (cx / cw + 1) src_w / 2, py = (1 - cy / cw) src_h / 2; it CONTAINS the pixel iff cw > 0, 0 <= px < src_w, 0 <= py < src_h.
 * All of this is f64 (the f32 matrices widened and taken as exact).
 * Seam rule.  The source view is the containing view with the largest cw -- the one whose axis is nearest -- and on a tie the one
 * with the lowest index.  (At pitch 0 the sectors of topo_panorama_uniforms tile the sphere band exactly once; at other pitches
 * they overlap slightly and leave gaps.)
 * Filters.  TOPO_UNWRAP_NEAREST: source texel (floor px, floor py).  TOPO_UNWRAP_BILINEAR, colour only: the four texels around
 * (px - 0.5, py - 0.5) of the SAME view with 8-bit weights, tap coordinates clamped to the view (a seam is clamped, never crossed);
 * on the *Srgb formats the channels are decoded, blended in linear light (f32, fixed order) and encoded again; alpha blends as a
 * plain unorm.  Depth and the source map are nearest with either filter: a depth blended across a silhouette is no depth.
 * Fill.  A pixel no view contains gets rgba 0 0 0 0, depth a quiet NaN and source -1.
 *
 * Outputs (each nullable, at least one; pointers and pitches multiples of 16 bytes; the bytes between out_w and the pitch are left
 * alone): RGBA8 in the context's format (needs rgba_src_dev), f32 depth (needs depth_src_dev), and an int32 SOURCE MAP
 * (view * src_h + sy) * src_w + sx of the nearest texel, with which any other per-pixel layer of the views (topo_ground_map_device's
 * float4, a mask) is carried across by a plain gather; it needs n_views * src_h * src_w < 2^31.  The sources are caller-owned
 * device memory laid out as topo_render_views_device writes them (view k at + k * view_stride, rows pitch bytes apart; a
 * topo_render_panorama strip: view_stride = sector_h * pitch); 1 <= n_views <= 64.
 * Asynchronous on the context's stream (topo_set_stream), in order behind whatever was queued there, as topo_visible_peaks_device;
 * with a pipeline depth > 1 call topo_join first, the frames run on streams of their own.  After topo_render_panorama every rank
 * holds the whole strip and the context's stream has waited for the last exchange, so any rank can unwrap.
 * Errors: TOPO_ERR_INVALID for null or misaligned arguments, zero sizes, parameters out of range, views with different eyes and a
 * source map beyond 2^31 texels. */
#define TOPO_UNWRAP_EQUIRECTANGULAR 0u
#define TOPO_UNWRAP_CYLINDRICAL 1u
#define TOPO_UNWRAP_NEAREST 0u
#define TOPO_UNWRAP_BILINEAR 1u
typedef struct topo_unwrap_params {
    uint32_t projection, filter, out_w, out_h;
    double az0_deg, az_span_deg;        /* left edge of column 0, clockwise from north; span in (0, 360] */
    double el_top_deg, el_bottom_deg;   /* top edge of row 0, bottom edge of the last row; -90 < bottom < top < 90 */
} topo_unwrap_params;
int topo_unwrap_device(topo_ctx* ctx, const topo_unwrap_params* params, uint32_t n_views, const topo_uniforms* views,
                       uint32_t src_w, uint32_t src_h,
                       const uint8_t* rgba_src_dev, size_t rgba_view_stride, size_t rgba_pitch,
                       const float* depth_src_dev, size_t depth_view_stride, size_t depth_pitch,
                       uint8_t* rgba_out_dev, size_t rgba_out_pitch, float* depth_out_dev, size_t depth_out_pitch,
                       int32_t* src_out_dev, size_t src_out_pitch);
/* Host, no GPU: output-pixel coordinates (x, y) = xy_out[2i], [2i+1] of the azimuth / elevation pairs az_el[2i], [2i+1] (degrees: what
 * topo_pixel_angles returns), so that a label placed in a sector lands on the unwrapped image.  Column c's centre is x = c + 0.5,
 * row r's centre y = r + 0.5; an azimuth outside a partial span gives x >= out_w.  Invalid parameters write nothing. */
void topo_unwrap_xy(const topo_unwrap_params* params, uint32_t n, const double* az_el, double* xy_out);

/* ---- host-side helpers mirroring the reference's CPU code ---------------------------------------------- */

/* Uniforms::new(&camera, bounds) with Camera{eye, yaw, pitch, fov_y, NEAR, FAR, view_mode, sun_angle{theta,phi}}:
 * render/data.rs:44-58, data/camera.rs:44-53,97-128 (glam 0.31 arithmetic restated in f32). */
void topo_camera_uniforms(const float eye[3], float yaw, float pitch, float fov_y, float width, float height,
                          float sun_theta_deg, float sun_phi_deg, int32_t view_mode, topo_uniforms* out);
/* The cameras of a 360-degree strip of n_sectors perspective sectors (no reference counterpart: the
 * reference renders one perspective view).  Sector k looks at yaw0 - k * 360/n degrees -- the reference's yaw grows
 * counter-clockwise seen from above (Camera::direction, camera.rs:101-109), so the strip reads left to right -- with
 * the vertical field of view that makes every sector 360/n degrees wide: 2 atan(tan(180/n deg) * sector_h / sector_w)
 * (topo_sector_fov_y, radians).  Writes n_sectors Uniforms blocks, ready for topo_render_views_device. */
float topo_sector_fov_y(uint32_t sector_w, uint32_t sector_h, uint32_t n_sectors);
void topo_panorama_uniforms(const float eye[3], float yaw0, float pitch, uint32_t sector_w, uint32_t sector_h,
                            float sun_theta_deg, float sun_phi_deg, int32_t view_mode, uint32_t n_sectors, topo_uniforms* out);
/* TerrainUniforms::new(coordinate_transform, (width, height)) -> 96 bytes (raster_point, model_point, pixel_scale,
 * size, normal_to_world_rot column-major mat4)                              render/data.rs:113-151 */
void topo_terrain_uniforms(const float raster_point[2], const float model_point[2], const float pixel_scale[2],
                           uint32_t w, uint32_t h, float out24[24]);
/* geometry::transform(h, longitude_deg, latitude_deg)                       render/geometry.rs:12-20 */
void topo_geometry_transform(float h, float longitude_deg, float latitude_deg, float out[3]);
/* dist_from_depth                                                           data/camera.rs:12-14 */
float topo_dist_from_depth(float depth);
/* pad_256                                                                   data/mod.rs:9-11 */
uint32_t topo_pad_256(uint32_t size);

/* CoordinateTransform::from_geo_tag_data(pixel_scale, tie_points, model_transformation)   common/coordinate_transform.rs:23-57
 * GeoTIFF ModelPixelScaleTag (3 doubles) + ModelTiepointTag (6 doubles) -> the six f32 the render path consumes.  A null
 * pointer stands for an absent tag (None).  Returns TOPO_ERR_UNSUPPORTED for the reference's IncorrectGeoTags (a
 * ModelTransformationTag is present, or one of the two required tags is absent) and TOPO_ERR_INVALID for
 * IncorrectGeoTagData (wrong value counts). */
int topo_coordinate_transform(const double* pixel_scale, uint32_t n_pixel_scale, const double* tie_points, uint32_t n_tie_points,
                              const double* model_transformation, float raster_point[2], float model_point[2],
                              float pixel_scale_out[2]);
/* CoordinateTransform::to_model / to_raster                                  common/coordinate_transform.rs:59-71 */
void topo_to_model(const float raster_point[2], const float model_point[2], const float pixel_scale[2], float x, float y,
                   float out[2]);
void topo_to_raster(const float raster_point[2], const float model_point[2], const float pixel_scale[2], float lon, float lat,
                    float out[2]);
/* get_height_value_at (F32 tiles)                                            common/coordinate_transform.rs:73-90
 * The terrain height under (longitude, latitude), as the reference looks it up to place the camera
 * (render_engine.rs:322-328): index = (raster.y as usize) * w + (raster.x as usize) with Rust's saturating float
 * casts, no bounds check other than the slice's.  Returns TOPO_ERR_NOT_FOUND where the reference yields None. */
int topo_height_value_at(const float* heights, uint32_t w, uint32_t h, const float raster_point[2], const float model_point[2],
                         const float pixel_scale[2], double longitude, double latitude, float* out);

/* ---- GeoTIFF decode: fetch_terrain's decode step, background_runner.rs:113-136 ------------------
 * The reference hands the downloaded bytes to the `tiff` crate (0.11.2): find_tag(ModelPixelScale / ModelTiepoint /
 * ModelTransformation) -> CoordinateTransform::from_geo_tag_data, read_image_to_buffer -> DecodingResult::F32, dimensions().
 * Supported here: classic TIFF of either byte order, first IFD, strips or tiles, one 32-bit IEEE float sample per pixel,
 * compression none / Deflate / LZW / PackBits, predictor none / horizontal / floating point.  The container is parsed
 * and the byte streams are decompressed on the host; predictor, byte order and tile placement run on the GPU.
 * Errors: TOPO_ERR_INVALID (malformed file, IncorrectGeoTagData), TOPO_ERR_UNSUPPORTED (BigTIFF, other sample layouts or
 * compressions, IncorrectGeoTags).  Unlike the reference, which ignores a failed read_image_to_buffer and carries on with
 * an empty raster, a decode error is reported. */
/* Size and CoordinateTransform of the first image; no GPU involved. */
int topo_geotiff_info(const uint8_t* bytes, size_t n_bytes, uint32_t* width, uint32_t* height, float raster_point[2],
                      float model_point[2], float pixel_scale[2]);
/* The raster as width*height host floats (row-major, row 0 first) -- what the reference keeps for get_height_value_at. */
int topo_geotiff_decode(topo_ctx* ctx, const uint8_t* bytes, size_t n_bytes, float* heights_out, size_t capacity_floats);
/* Decode + add_terrain in one step; the raster goes from the decoder to the tile without leaving the device. */
int topo_add_terrain_geotiff(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg, const uint8_t* bytes, size_t n_bytes);

/* UiController::get_locations_range(location, range_dist)                    control/ui_controller.rs:61-83
 * (the tile working set around a viewpoint; the reference calls it with 100 000 m).  Writes up
 * to `cap` (lat_deg, lon_deg) pairs in the reference's order -- sorted by (|lat - c_lat|, |lon - c_lon|), stable over
 * the row-major cartesian product, where c_lat is always 89 because of the reference's `.min(-90).max(89)` -- and
 * returns the number of tiles in the range (which may exceed cap).  In the reference the subsequent load order is
 * that of a HashSet (unspecified); callers here get the sorted order. */
uint32_t topo_locations_range(float latitude, float longitude, float range_dist, int32_t* out_lat_lon, uint32_t cap);

/* UiController::change_location(location, data, engine)                        control/ui_controller.rs:23-59
 * The working-set maintenance around get_locations_range: tiles of the new range that are not loaded are to be requested
 * (the reference sends DataRequested to its background runner), loaded tiles outside it are unloaded
 * (terrain.unload_terrain).  The reference walks HashSets, so its orders are unspecified; here `request` comes in
 * get_locations_range's order and `unload` in the order of `loaded`.  Counts may exceed the caps (nothing is written past
 * them).  topo_change_location_plan is the pure set arithmetic over a caller-held list of (lat, lon) pairs;
 * topo_change_location applies it to the context: it unloads what falls outside (as topo_unload_terrain) and reports
 * what the host still has to fetch and hand to topo_add_terrain / topo_add_terrain_geotiff. */
void topo_change_location_plan(float latitude, float longitude, float range_dist, const int32_t* loaded_lat_lon, uint32_t n_loaded,
                               int32_t* unload_out, uint32_t unload_cap, uint32_t* n_unload, int32_t* request_out,
                               uint32_t request_cap, uint32_t* n_request);
int topo_change_location(topo_ctx* ctx, float latitude, float longitude, float range_dist, int32_t* request_out,
                         uint32_t request_cap, uint32_t* n_request, uint32_t* n_unloaded);

#ifdef __cplusplus
}
#endif
#endif /* TOPO_HIP_H */
