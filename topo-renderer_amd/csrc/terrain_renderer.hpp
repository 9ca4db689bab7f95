// terrain_renderer.hpp -- host side of the MI355X terrain path: a C++ mirror of the reference's
// `TerrainRenderer` (topo-renderer/src/render/terrain_renderer.rs) with the same five methods
// (new / update / add_terrain / unload_terrain / render).  The reference's host code is Rust; no Rust
// toolchain exists in this image, so the host side above the C ABI is C++ (include/topo_hip.h wraps this
// class one-to-one; INTEGRATION.md has the Rust shim).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/topo_hip.h"
#include "host_math.hpp"
#include "topo_kernels.h"

namespace topo {

constexpr uint32_t kPanoramaSectors = 8;      // fixed, independent of the GPU count, so the strip is the same for every N
struct Comm;                                  // panorama.cpp: an RCCL communicator + this process's rank

// BTreeMap<GeoLocation, _> key: Ord over {latitude{degree,direction S<N}, longitude{degree,direction W<E}}
// (topo-common/src/lib.rs:7-38); GeoLocation::from_coord maps sign > 0 to N/E, else S/W (:102-121).
using GeoKey = std::tuple<int, int, int, int>;
inline GeoKey geo_key(int lat, int lon) {
    return GeoKey(lat < 0 ? -lat : lat, lat > 0 ? 1 : 0, lon < 0 ? -lon : lon, lon > 0 ? 1 : 0);
}

#define TOPO_HIP_TRY(expr)                                   \
    do {                                                     \
        hipError_t e_ = (expr);                              \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);    \
    } while (0)

// A block of device memory that only grows (TerrainRenderer::ensure) and goes with its owner.  Owners bind the device and wait
// for their streams in their destructor's body; the blocks are freed behind it, as members.  The same shape owns pinned host
// memory (TerrainRenderer::ensure_pinned) and a registration of the caller's memory: non-copyable, movable, null = nothing to release.
template <hipError_t (*Free)(void*)>
struct Block {
    void* p = nullptr;
    size_t cap = 0;
    Block() = default;
    Block(Block&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Block& operator=(Block&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~Block() { reset(); }
    void reset() { if (p) (void)Free(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
using DeviceBuffer = Block<hipFree>;
using PinnedBuffer = Block<hipHostFree>;
using HostRegistration = Block<hipHostUnregister>;      // p, cap: the caller's buffer (hipHostRegister)

// An event or a stream of the host layer's own, owned the same way; reads as the handle wherever HIP wants one.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~Handle() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// Images of `rows` rows at the given pitches (bytes), one behind the other.
inline OutputParams image_output(uint8_t* rgba, size_t rgba_pitch, float* depth, size_t depth_pitch, uint32_t rows) {
    return OutputParams{rgba, rgba_pitch * rows, rgba_pitch, depth, depth_pitch * rows, depth_pitch};
}

struct Tile {          // RenderBuffer (render_buffer.rs:23-31) minus the wgpu plumbing; move-only: it owns its device memory
    int lat = 0, lon = 0;
    uint64_t seq = 0;  // insertion order (for topo_recompute_normals)
    DeviceBuffer pool;              // the one allocation the three pointers below (and dev) point into
    float* d_heights = nullptr;
    uint32_t* d_normals = nullptr;
    float* d_minmax = nullptr;
    // a sphere around the centres of the tile's block spheres (the cull's load-time table, read back once per tile): lets a
    // submission prove on the host that none of its blocks can be an occlusion-test candidate.  radius < 0: unknown.
    double centres[4] = {0.0, 0.0, 0.0, -1.0};
    double block_radius = -1.0;     // the largest radius among those block spheres (read back with them); < 0: unknown
    TileDev dev{};
    DeviceBuffer mask;              // viewshed: 1 bit per cell (bit x (h-1) + y), once accumulation has been enabled; goes with the tile
};

// The eight stages of a frame, in launch order; stage i spans events i .. i + 1 of the frame's TimedFrame.
enum Stage { kStClear, kStCull, kStRasterNear, kStRareBigNear, kStOcclusion, kStRasterFar, kStRareBigFar, kStResolve, kNumStages };

class TerrainRenderer {
   public:
    static int create(TerrainRenderer** out, int device, uint32_t w, uint32_t h, uint32_t format, std::string* err);
    ~TerrainRenderer();

    int add_terrain(int32_t lat, int32_t lon, const float* heights, bool heights_on_device, uint32_t w, uint32_t h,
                    const float rp[2], const float mp[2], const float ps[2]);
    int unload_terrain(int32_t lat, int32_t lon);
    bool last_far_phase() const { return last_far_phase_; }
    void set_tile_prefilter(bool on) { tile_prefilter_ = on; }                                                 // test hook
    void last_cull_pairs(uint32_t out[2]) const { out[0] = last_cull_pairs_[0]; out[1] = last_cull_pairs_[1]; }   // test hook: pairs launched, pairs in all
    int update(uint32_t w, uint32_t h, const topo_uniforms* u, const topo_post_uniforms* pu);
    int render(uint8_t* rgba, size_t rgba_pitch, float* depth, size_t depth_pitch);
    int render_views_device(uint32_t n, const topo_uniforms* views, uint32_t w, uint32_t h, const OutputParams& out);
    int render_device(uint8_t* rgba_dev, size_t rgba_pitch, float* depth_dev, size_t depth_pitch);
    int render_panorama(Comm* comm, const float eye[3], float yaw0, float pitch, uint32_t sector_w, uint32_t sector_h, float sun_theta_deg,
                        float sun_phi_deg, int32_t view_mode, uint8_t* strip_dev, float* depth_dev);
    int render_batch(uint32_t n_viewpoints, const float* eyes, const float* yaw0s, const float* sun_theta_phi_deg, float pitch, uint32_t sector_w,
                     uint32_t sector_h, int32_t view_mode, uint8_t* rgba_dev, float* depth_dev);
    int recompute_normals();
    int overlay_lines_device(const void* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, float line_width, uint8_t* rgba_dev,
                             size_t rgba_pitch);
    int overlay_glyphs(const void* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas, uint32_t atlas_w, uint32_t atlas_h, uint8_t* rgba, size_t rgba_pitch);
    int overlay_glyphs_device(const void* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas, uint32_t atlas_w, uint32_t atlas_h, uint8_t* rgba_dev,
                              size_t rgba_pitch);
    int overlay_lines(const void* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, float line_width, uint8_t* rgba,
                      size_t rgba_pitch);
    int change_location(float latitude, float longitude, float range_dist, std::vector<std::pair<int32_t, int32_t>>& request, uint32_t* n_unloaded);

    int set_stream(hipStream_t s);
    int synchronize();
    int set_pipeline_depth(int depth);
    int join();                 // waits for the frames in flight on the contexts' own streams
    int join_frames();          // topo_join: join + the frames' status (TOPO_ERR_CAPACITY for an incomplete frame)
    int set_normals_lds_rows(int rows);
    int set_queue_caps(uint32_t big_cap, uint32_t rare_cap);
    int pin_host_buffer(void* p, size_t bytes);
    int unpin_host_buffer(void* p);
    int get_timings(float out[TOPO_TIMING_SLOTS]);
    int get_timing_history(uint32_t n_frames, float* out_ms, uint32_t* n_out);
    int get_counters(uint32_t out[6]);
    int cover_stats(uint32_t out[3]);      // test hook: the last frame's covering items, regions claimed, claims lost
    void set_resolve_owned(bool on) { resolve_owned_ = on; }      // test hook: the claimed regions' strip records, from the next submission on
    int owned_strips(uint32_t out[2]);     // test hook: the last frame's strips that pass k_resolve's ownership test, strips with a record of the frame
    int read_cull_lists(uint32_t* near_out, uint32_t near_room, uint32_t* far_out, uint32_t far_room, uint32_t* survivors_out, uint32_t survivors_room,
                        uint32_t counts_out[5]);      // test hook: the last frame's near items, far candidates, far survivors
    int frame_status(uint32_t out[4]);
    int set_occlusion_split(float metres);
    int set_timing_slots(uint32_t mask);
    int read_normals(int32_t lat, int32_t lon, uint8_t* out);
    int read_tile_tables(int32_t lat, int32_t lon, float* minmax_out, float* trig_out, double* bounds_out, uint32_t* n_blocks_out);      // test hook
    int geotiff_to_device(const uint8_t* bytes, size_t n, DeviceBuffer& heights, uint32_t* w, uint32_t* h, float rp[2], float mp[2], float ps[2]);
    int geotiff_decode(const uint8_t* bytes, size_t n, float* heights_out, size_t capacity);
    int add_terrain_geotiff(int32_t lat, int32_t lon, const uint8_t* bytes, size_t n);
    int probe_sincos(const float* x, float* s, float* c, size_t n);
    int probe_div(int32_t kind, const float* x, const float* y, float* out, size_t n);
    int visible_peaks(uint32_t n, const float* peaks, uint8_t* visible, uint32_t* xy);
    int visible_peaks_device(const topo_uniforms* view, uint32_t w, uint32_t h, const float* depth_dev, size_t depth_pitch,
                             uint32_t n, const float* peaks_dev, uint8_t* visible_dev, uint32_t* xy_dev);

    // viewshed: the DEM cells that won >= 1 pixel of the frames rendered while accumulation is on, per tile
    int viewshed_enable(bool on);
    int viewshed_reset();
    int viewshed_read(int32_t lat, int32_t lon, uint8_t* mask_out, size_t pitch, uint64_t* n_visible);
    int viewshed_stats(uint64_t out[3]);      // test hook: terrain keys, combined updates, atomics issued since the last reset

    // horizon: the topmost terrain pixel of every column of the latest submission's views (topo_horizon_*)
    int horizon_shape(uint32_t* n_views, uint32_t* w, uint32_t* h);
    int horizon_read(uint32_t first_view, uint32_t n_views, topo_horizon_point* out, size_t view_stride);
    int horizon_device(uint32_t first_view, uint32_t n_views, topo_horizon_point* out_dev, size_t view_stride);

    // ground: the terrain point under pixels of the latest submission's views (topo_ground_*)
    int ground_read(uint32_t n, const topo_ground_query* queries, topo_ground_point* out);
    int ground_device(uint32_t n, const topo_ground_query* queries_dev, topo_ground_point* out_dev);
    int ground_map_device(uint32_t first_view, uint32_t n_views, float* out_dev, size_t view_stride_bytes, size_t pitch_bytes);

    // rays against the resident tiles (topo_raycast_*): no submission needed
    int raycast_read(uint32_t n, const topo_ray* rays, topo_ray_hit* out);
    int raycast_device(uint32_t n, const topo_ray* rays_dev, topo_ray_hit* out_dev);
    // ... and the sunlit layer of the latest submission's views, beside the ground map (topo_sunlit_map_device)
    int sunlit_map_device(uint32_t first_view, uint32_t n_views, const double sun_dir[3], uint8_t* out_dev, size_t view_stride_bytes, size_t pitch_bytes);

    // surface: the drawn terrain under a longitude and latitude -- lists, grids and profiles (topo_surface_*, topo_profile_*): no submission needed
    int surface_read(uint32_t n, const double* lonlat_deg, topo_surface_point* out);
    int surface_device(uint32_t n, const double* lonlat_dev, topo_surface_point* out_dev);
    int surface_grid_device(double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny, float* out_dev, size_t pitch_bytes);
    // the map view (topo_map_*): tile-set queries on stream_ like the surface calls; with TOPO_MAP_SEEN they join the frames in flight
    // first, as viewshed_read does, so that the masks hold every frame queued before the call
    int map_device(const topo_map_params* params, uint8_t* rgba_dev, size_t rgba_pitch, uint8_t* flags_dev, size_t flags_pitch);
    int map_read(const topo_map_params* params, uint8_t* rgba, uint8_t* flags);
    int profile_device(uint32_t n, const topo_ray* segs_dev, uint32_t m, float* samples_dev, size_t segment_stride_bytes, topo_profile_summary* summary_dev);
    int profile_read(uint32_t n, const topo_ray* segs, uint32_t m, float* samples, topo_profile_summary* summary);

    // visibility: what observers see of the drawn terrain -- maps and lists (topo_visibility_*): no submission needed.
    // refraction_k: null for straight sight lines, else the coefficient of topo_visibility_refracted_* (0 <= k < 1)
    int visibility_grid_device(uint32_t n_observers, const topo_observer* observers, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny,
                               double target_height_m, uint8_t* out_dev, size_t layer_stride_bytes, size_t pitch_bytes, const double* refraction_k = nullptr);
    int visibility_device(uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_dev, double target_height_m, uint8_t* out_dev,
                          size_t list_stride_bytes, const double* refraction_k = nullptr);
    int visibility_read(uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_deg, double target_height_m, uint8_t* out,
                        const double* refraction_k = nullptr);

    // skyline: the terrain horizon by azimuth from observers (topo_skyline_*): no submission needed
    int skyline_device(uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m, double max_range_m,
                       float* elevation_dev, size_t observer_stride_bytes, topo_skyline_sample* samples_dev, size_t samples_stride_bytes);
    int skyline_read(uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m, double max_range_m,
                     float* elevation, topo_skyline_sample* samples);

    // sun exposure: a day of sun and shadow over points of the drawn terrain -- maps and lists (topo_sun_exposure_*): no submission needed
    int sun_exposure_grid_device(uint32_t n_suns, const topo_sun* suns, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny, uint64_t* lit_dev,
                                 uint64_t* shadow_dev, float* exposure_dev, size_t mask_pitch_bytes, size_t exposure_pitch_bytes);
    int sun_exposure_device(uint32_t n_suns, const topo_sun* suns, uint32_t n, const double* lonlat_dev, uint64_t* lit_dev, uint64_t* shadow_dev, float* exposure_dev);
    int sun_exposure_read(uint32_t n_suns, const topo_sun* suns, uint32_t n, const double* lonlat_deg, uint64_t* lit, uint64_t* shadow, float* exposure);

    // peak labels: the peaks the caller's depth images show, laid out in rows, per image of views_per_image views (topo_labels_*): no submission needed
    int labels_device(const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t w, uint32_t h, const float* depth_dev, size_t depth_view_stride,
                      size_t depth_pitch, uint32_t n_peaks, const float* peaks_dev, const float* widths_dev, topo_label* labels_dev, uint32_t* counts_dev, uint8_t* state_dev);
    int labels_read(const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t w, uint32_t h, const float* depth_dev, size_t depth_view_stride,
                    size_t depth_pitch, uint32_t n_peaks, const float* peaks, const float* widths, topo_label* labels, uint32_t* counts, uint8_t* state);

    // summits: the posts of the resident DEMs no higher post stands near, and the best post around a point (topo_summits_*, topo_summit_snap_*): no submission needed
    int summits_device(const topo_summit_params* params, topo_summit* out_dev, uint32_t capacity, uint32_t* count_dev);
    int summits_read(const topo_summit_params* params, topo_summit* out, uint32_t capacity, uint32_t* count);
    int summit_snap_device(uint32_t n, const double* lonlat_dev, double radius_m, topo_summit_snap* out_dev);
    int summit_snap_read(uint32_t n, const double* lonlat_deg, double radius_m, topo_summit_snap* out);
    int set_summit_band_rows(uint32_t rows) { summit_band_rows_ = rows; return TOPO_OK; }      // test hook: 0 = the default
    int summit_counts(uint64_t out[2]);                                                         // test accessor

    // unwrap: finished views that share an eye as one azimuth / elevation image (topo_unwrap_device)
    int unwrap_device(const topo_unwrap_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t src_w, uint32_t src_h, const OutputParams& src,
                      const OutputParams& out, int32_t* src_out_dev, size_t src_out_pitch);

    const char* last_error() const { return err_.c_str(); }

   private:
    TerrainRenderer() = default;
    int init();                                                   // create(): the stream and the events every renderer has
    int fail(int code, const std::string& msg);
    int hip_fail(hipError_t e, const char* what);
    int bind_device();
    int ensure(hipStream_t s, DeviceBuffer& b, size_t need);      // grows b to `need` bytes; s: the stream to wait for before the old block goes
    int ensure_pinned(PinnedBuffer& b, size_t need);              // the same for pinned host memory nothing in flight uses
    int wait_all();                                               // join + stream_
    void collect_jobs(const Tile& nt, const std::map<GeoKey, uint32_t>& rank, std::vector<EdgeJob>& edges,
                      std::vector<CornerJob>& corners);   // the seam/corner orchestration of add_terrain
    int run_seam_jobs(const std::vector<EdgeJob>& edges, const std::vector<CornerJob>& corners);
    int upload_seam_jobs(const std::vector<EdgeJob>& edges, const std::vector<CornerJob>& corners);
    void launch_seam_jobs(size_t n_edges, size_t n_corners);
    void launch_load_kernels(uint32_t first, uint32_t count, hipEvent_t mid);      // tables + interior normals of a run of tiles
    std::map<GeoKey, uint32_t> ranks() const;
    Tile* find(int lat, int lon);
    int upload_tile_table();
    int overlay_upload(const void* a, size_t a_bytes, const void* b, size_t b_bytes, uint8_t** b_dev, bool* keys_fresh);
    template <class Draw> int overlay_host_image(uint8_t* rgba, size_t rgba_pitch, Draw draw);
    int alloc_mask(Tile& t);                                      // viewshed (terrain_queries.cpp)
    size_t mask_bytes() const { return (((size_t)(tile_w_ - 1) * (tile_h_ - 1) + 31) / 32) * 4; }

    int device_ = 0;
    uint32_t W_ = 0, H_ = 0;
    uint32_t format_ = TOPO_FORMAT_RGBA8_UNORM_SRGB;
    uint32_t tile_w_ = 0, tile_h_ = 0;
    topo_uniforms uniforms_{};
    topo_post_uniforms post_{{0.0f, 0.0f}, 100.0f, 0.0f};      // (pixelize_n 100: the branch off, as the reference always has it)
    bool have_uniforms_ = false;
    std::map<GeoKey, Tile> tiles_;
    uint64_t next_seq_ = 1;
    bool table_dirty_ = true;
    int lds_rows_ = 0;        // interior normals: 0 = without an LDS tile (k_normals_rolling: the sweep's optimum, profiles/r03_normals_lds_sweep.json;
                              // needs a tile width that is a multiple of four, else the LDS form with 32 rows); 4..64 = LDS tile height of k_normals_interior
    uint32_t big_cap_cfg_ = 0, rare_cap_cfg_ = 0;
    uint64_t rare_cap_auto_ = 0;           // rare-queue capacity topo_render grew to after an overflow (0 = default)
    uint32_t timing_slots_ = 0x3Fu;        // topo_set_timing_slots: which per-kernel durations to measure
    bool timing_total_ = true;        // a frame's first and last event (TOPO_TIMING_NO_TOTAL clears it)
    float occlusion_split_m_ = 90000.0f;   // flat optimum 60..120 km at c4 (profiles/README.md)

    Stream own_stream_;
    hipStream_t stream_ = nullptr;      // own_stream_, or the caller's (topo_set_stream)
    static constexpr int kEvRing = 32;
    static constexpr uint64_t kStatusRing = 64;
    uint64_t frame_seq_ = 0;          // frames submitted by this renderer
    Event load_ev_[3];                // recompute_normals: start, end, between the tables and the normals
    bool load_timed_ = false;

    // Everything one frame in flight owns.  With pipeline depth 1 (default) there is one context and it runs on
    // stream_; with depth d > 1 topo_render_views_device rotates through d contexts, each on a stream of its own, so
    // that the memory-latency-bound cull/raster phases of one frame run under the ALU-bound resolve of the previous one.
    struct FrameCtx {
        Stream stream;                       // own stream (depth > 1)
        // timing events of the last kEvRing frames of this context (a frame's durations stay readable while later frames are
        // submitted: topo_get_timing_history reads a whole timed region's frames after it, without a wait inside it)
        struct TimedFrame {
            Event ev[kNumStages + 1];
            uint32_t recorded = 0, slots = 0;      // the events recorded (bit i: ev[i]); the timing slots selected then
            uint64_t frame = 0;                    // the renderer-wide number of the frame that used the set
        } timed_frames[kEvRing];
        uint64_t frames = 0;                  // frames submitted on this context
        Event done;
        // the stream the context's latest frame was queued on: its own stream (depth > 1), stream_ (depth 1, and the slot-by-slot
        // panorama at any depth); null once a wait has covered it.  A context's frames are ordered (a frame on the own stream waits
        // for stream_, the panorama joins the contexts first), so waiting for this stream waits for all of them.
        hipStream_t last_stream = nullptr;
        // a frame queued with pipeline depth > 1 that join() has not waited for yet (at depth 1 every wait synchronizes stream_)
        bool timed = false, pending = false;
        // pinned ring of the last kStatusRing frames' kStatusWords counter words, each stored by its frame's k_resolve (the bounds-checking build: copied out behind it);
        // frames [checked, submitted) have not been looked at by check_frames yet
        PinnedBuffer h_status;
        uint64_t submitted = 0, checked = 0;
        uint32_t* status_words(uint64_t frame) const { return h_status.as<uint32_t>() + (frame % kStatusRing) * kStatusWords; }
        const uint32_t* latest_status() const { return status_words(submitted - 1); }
        DeviceBuffer d_vis, d_dirty;      // d_dirty: one mark per 64 visibility keys (kernels_common.h: struct Vis)
        DeviceBuffer d_work, d_work2, d_far, d_big, d_rare, d_counters;
        DeviceBuffer d_cover;             // the regions' owner words (topo_kernels.h: CoverParams)
        DeviceBuffer d_cover_recs;        // ... and the records of the claimed regions' strips (CoverParams::recs)
        uint32_t cover_serial = 0;        // the serial the context's latest frame claimed regions with
        CoverParams cover{};              // this frame's; serial 0: the path is off
        uint32_t cover_big_cap = 0;       // ... and its big queue's capacity (the test hook reads the queue back)
        bool lists_valid = false;         // the context's latest submission was queued whole, at the current pipeline depth
        uint32_t lists_near_cap = 0, lists_far_sub_cap = 0;      // the latest frame's near_cap / far_sub_cap (read_cull_lists, test hook)
        DeviceBuffer d_pre_rgba, d_pre_depth;      // the pixelise branch: the render-target image k_post_pixelize samples, and a depth image when the caller wants none
        // the context's latest submission as the queries read it (its keys and marks are d_vis / d_dirty until the next one)
        struct Submission {
            uint32_t n_views = 0;
            uint64_t tile_gen = 0;                  // tile_gen_ when it was rendered
            HorizonParams query{};                  // a query's parameters, as far as the submission sets them (its keys, marks, counter set, shape)
            std::vector<GroundView> views;          // its views' camera_proj and eye, whoever generated them (the ground query; ViewDev has no eye)
            bool views_on_device = false;           // d_ground_views holds them (uploaded by the submission's first ground query)
        } sub;
        DeviceBuffer d_ground_views;
    };
    static constexpr int kMaxPipeline = 4;
    FrameCtx ctx_[kMaxPipeline];
    int pipeline_depth_ = 1, next_ctx_ = 0, last_ctx_ = 0;
    int init_ctx(FrameCtx& c, bool own_stream);
    int check_frames();                        // after a wait: turn a finished frame's overflow status into TOPO_ERR_CAPACITY
    uint32_t last_status_[4] = {};             // status word + bounds record of the last frame looked at
    bool fold_frames(FrameCtx& c, uint64_t end);   // folds the finished, unchecked frames [checked, end) of c into last_status_; true if one overflowed
    bool fold_frames(FrameCtx& c) { return fold_frames(c, c.submitted); }
    bool fold_idle();                              // fold_frames over every context no frame is in flight on
    bool fold_latest(FrameCtx& c, bool retry);     // c's latest frame is the caller's own: folds c, true if that frame overflowed
    void record_bounds(const uint32_t* words);
    bool overflow_pending_ = false;
    // slots: the frame resolved in several launches (k_resolve over block ranges), after_slot(i, stream) called behind each --
    // null / 0: one launch over the whole frame
    struct ResolveSlot { uint32_t block_first, block_count; };
    int render_frame(FrameCtx& c, hipStream_t s, uint32_t n, const topo_uniforms* views, uint32_t w, uint32_t h, const OutputParams& out,
                     const ResolveSlot* slots = nullptr, uint32_t n_slots = 0, const std::function<int(uint32_t, hipStream_t)>* after_slot = nullptr);
    // render_frame's steps, in its order
    int grow_frame_buffers(FrameCtx& c, hipStream_t s, uint32_t n, uint32_t w, uint32_t h, FrameParams& p);
    int stage_views(FrameCtx& c, hipStream_t s, const topo_uniforms* views, FrameParams& p, ViewPack& pack, bool* pack_in_cull);
    void fill_params(FrameCtx& c, FrameParams& p);
    struct CullList { const uint16_t* codes; uint32_t n; };      // the kept (view, tile) pairs; codes null: every pair (the full grid)
    CullList cull_pairs(const topo_uniforms* views, const FrameParams& p);
    int queue_frame(FrameCtx& c, hipStream_t s, FrameParams& p, const ViewPack* pack_in_cull, const CullList& cull, bool far_phase, const OutputParams& out,
                    const ResolveSlot* slots, uint32_t n_slots, const std::function<int(uint32_t, hipStream_t)>* after_slot);
    void record_submission(FrameCtx& c, const FrameParams& p, const topo_uniforms* views);
    int frame_durations(const FrameCtx::TimedFrame& f, float out[7]);

    DeviceBuffer d_tiles_, d_views_, d_edge_jobs_, d_corner_jobs_, d_out_rgba_, d_out_depth_;
    // topo_render's way out to host memory: a pinned staging image and the events of its slices; the buffers the caller pinned
    PinnedBuffer h_stage_;
    Event stage_ev_[8];
    std::vector<HostRegistration> pinned_;
    int download(uint8_t* dst, size_t dst_pitch, const uint8_t* src_dev, size_t row);
    static constexpr int kViewSlots = 16;
    static constexpr uint32_t kMaxViewsPerSlot = 64;
    PinnedBuffer h_views_;                // pinned staging ring
    Event view_ev_[kViewSlots];
    bool view_used_[kViewSlots] = {};
    DeviceBuffer d_peaks_;            // xyz in, then visible + xy out
    DeviceBuffer d_proj_;
    DeviceBuffer d_overlay_geo_;      // overlay vertices + indices
    DeviceBuffer d_overlay_keys_;     // W*H overlay keys (depth | ~triangle), kept at the post quad's depth between calls
    uint32_t overlay_w_ = 0, overlay_h_ = 0;
    bool have_depth_ = false;
    uint32_t depth_w_ = 0, depth_h_ = 0;
    bool last_far_phase_ = true;           // whether the last submission launched the far phase (test hook)
    // the cull's tile prefilter: on / off (the tiles' spheres: tile_spheres), the last submission's kept pairs (the launch copies
    // them) and its counts (pairs launched, pairs in all: test hook)
    bool tile_prefilter_ = true;
    bool resolve_owned_ = true;      // topo_debug_set_resolve_owned
    uint16_t cull_codes_[kMaxCullPairs] = {};
    uint32_t last_cull_pairs_[2] = {0, 0};
    // viewshed: render_frame launches k_viewshed while vs_on_; the masks exist (every tile has one) once vs_ever_.  The masks are shared
    // by every frame context: frames in flight only OR into them, so they need no order among themselves.
    bool vs_on_ = false, vs_ever_ = false;
    DeviceBuffer d_vs_table_;      // rank -> the tile's mask, rebuilt with the tile table
    DeviceBuffer d_vs_stats_;      // kViewshedStatSlots x 4 counters of k_viewshed
    // what the frame path leaves for the queries: the frame context of the latest submission (-1: none, or one that failed half-way), and
    // the tile set's generation (add_terrain / unload_terrain bump it: a submission of another tile order can no longer be decoded)
    int latest_ctx_ = -1;
    uint64_t tile_gen_ = 0;

    // ---- the queries (terrain_queries.cpp): the frame path calls tile_spheres (host only) and query_fold_check, and never touches the rest.
    // Tables made from the tile set, in three levels, each made by the first caller that needs it after the tile set changed.
    struct TileTables {
        // the tiles' spheres (kTileSphereDoubles = kLosSphereDoubles each, draw order): host memory, the cull prefilter's and d_spheres' source
        std::vector<double> spheres;
        // decode: rank -> (lat, lon), and its host copy (the source of the upload); all a horizon query builds
        std::vector<int32_t> ll;
        DeviceBuffer d_ll;
        // geometry (ground, rays, sunlit): the tiles' f64 sin / cos tables (one entry per column and per row of every tile, draw
        // order: topo_ground.h; 38 KB per 1200 x 1200 tile; trig_doubles in all) and the device copy of the spheres
        DeviceBuffer d_trig, d_spheres;
        size_t trig_doubles = 0;
        uint64_t spheres_gen = ~0ull, decode_gen = ~0ull, geometry_gen = ~0ull;      // tile_gen_ when each level was made
    } tables_;
    enum TableLevel { kDecodeTables, kGeometryTables };
    const std::vector<double>& tile_spheres();
    int prepare_tables(TableLevel level, hipStream_t s);      // what a query kernel on s reads, up to `level`: once per public query
    // The queries' own buffers: the bounds record of every query kernel (TOPO_BOUNDS_CHECK build, folded into topo_frame_status), the
    // host reads' device buffers (horizon rows; ground queries, records; rays in, records out, their pinned staging; surface points in,
    // records or profile summaries out, their pinned staging, a profile read's samples; the visibility calls' observers as given and
    // as resolved -- the skyline calls' too --, a visibility read's classes, a skyline read's elevations and records, the sun exposure calls' suns and a sun exposure read's masks and exposures), and the device
    // copy of k_unwrap's f64 tables (topo_unwrap.h), kept for what they were built from -- the call's parameters, the views'
    // direction blocks and the eye (unwrap_key) -- with their host copy, the source of the upload; likewise the device table of the
    // label calls' view matrices with its host copy (label_projs: key and source of the upload), and a label read's inputs and outputs;
    // the summit calls' scratch (one band: topo_kernels.h) with their state record, and a summit read's records and count
    struct QueryBuffers {
        DeviceBuffer d_check, d_horizon_out, d_ground_q, d_ground_out, d_ray_in, d_ray_out, d_surface_in, d_surface_out, d_profile_samples, d_vis_observers, d_vis_eyes, d_vis_out,
            d_sky_elevation, d_sky_samples, d_suns, d_sun_lit, d_sun_shadow, d_sun_exposure, d_unwrap_tab, d_label_projs, d_label_in, d_label_out, d_summit_scratch, d_summit_out, d_summit_count, d_map_rgba, d_map_flags;
        PinnedBuffer h_ray_stage, h_surface_stage;
        std::vector<double> unwrap_tab;
        std::vector<uint8_t> unwrap_key;
        std::vector<float> label_projs;
    } query_;
    int ensure_query_check(hipStream_t s);      // the check build's bounds record (the product build: nothing)
    int query_fold_check();
    // A query on the latest submission: its context, the stream it was queued on (the query goes behind it) and its shape.  begin: if
    // views [first, first + n) of it can be answered; queued: a device variant's end (the pending mark); finish_read: a host read's.
    struct LatestSubmission { FrameCtx* c; hipStream_t s; uint32_t W, H, n_views; };
    int query_begin(uint32_t first_view, uint32_t n_views, LatestSubmission& q);
    int query_queued(const LatestSubmission& q);
    int query_finish_read(const LatestSubmission& q, const char* what);
    int horizon_launch(const LatestSubmission& q, uint32_t first_view, uint32_t n_views, HorizonPoint* out, size_t view_stride);
    int ground_prepare(const LatestSubmission& q);      // geometry tables + the submission's views on the device
    GroundParams ground_params(const LatestSubmission& q, uint32_t first_view, uint32_t n_views) const;
    RayParams ray_params() const;
    int visibility_begin(uint32_t n_observers, const topo_observer* observers, double target_height_m, const double* refraction_k);      // checks, then resolve_observers
    int resolve_observers(uint32_t n_observers, const topo_observer* observers);      // the tables, and the observers resolved into d_vis_eyes on stream_
    int skyline_check(uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m, double max_range_m);
    int sun_begin(uint32_t n_suns, const topo_sun* suns);      // checks, the tables, and the suns normalised into d_suns on stream_
    int summits_check(const topo_summit_params* params, bool device);      // what both summit calls refuse (their outputs apart)
    int summits_launch(const topo_summit_params& params, SummitRec* out_dev, uint32_t capacity, uint32_t* count_dev);      // the tables are prepared; queues the bands on stream_
    uint32_t summit_band_rows_ = 0;
    int labels_check(const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t w, uint32_t h, const float* depth_dev, size_t depth_view_stride,
                     size_t depth_pitch);      // what both label calls refuse, before anything is queued

    std::string err_;
};

int comm_unique_id(uint8_t out[128], std::string* err);
int comm_init(Comm** out, int device, const uint8_t id128[128], int rank, int world, std::string* err);
int comm_from_nccl(Comm** out, void* nccl_comm, int rank, int world, std::string* err);
void comm_destroy(Comm* c);
void panorama_sector_range(int rank, int world, uint32_t* first, uint32_t* count);
uint32_t panorama_slots(int world, uint32_t sector_w, uint32_t sector_h, topo_panorama_slot* out, uint32_t cap);

}  // namespace topo
