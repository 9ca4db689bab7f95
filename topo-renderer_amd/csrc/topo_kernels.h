// topo_kernels.h -- launch interface of the gfx950 kernels (topo_kernels.hip: the launchers; kernels_*.h: the kernels, by phase).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "topo_pipeline.h"
#include "topo_ground.h"
#include "topo_unwrap.h"
#include "topo_los.h"

namespace topo {

// Raster work decomposition: a tile's (w-1) x (h-1) cell grid is cut into blocks of kBCX x kBCY cells
// ((kBCX+1) x (kBCY+1) vertices staged in LDS by one 256-thread workgroup).  1199 = 19*60+59 = 79*15+14,
// so a 1200x1200 COP90 tile gives 20 x 80 blocks with no sliver blocks.
constexpr uint32_t kBCX = 60, kBCY = 15;
constexpr uint32_t kVX = kBCX + 1, kVY = kBCY + 1;
#ifndef TOPO_RESOLVE_RPW
#define TOPO_RESOLVE_RPW 8      // pixel rows per wave of k_resolve (4 or 8)
#endif
constexpr uint32_t kResolveBlockW = 64, kResolveBlockH = 4 * TOPO_RESOLVE_RPW;   // k_resolve's pixel blocks: four waves, a 64 x RPW strip each

struct WorkItem {          // one (view, tile, block) that survived the frustum cull
    uint32_t view_rank;    // view << 16 | tile rank (draw order)
    uint32_t block;        // by * bx_count + bx
};

struct FarItem {           // a frustum-surviving block beyond the occlusion split, with its conservative screen footprint
    uint32_t view_rank;
    uint32_t block;
    uint16_t x0, x1, y0, y1;   // inclusive pixel box of everything the block can draw (already clamped to the target)
    uint32_t zmin_bits;        // f32 bits of a lower bound of every depth the block can produce
};

struct BigItem {           // a triangle too large for the in-lane loop, restricted to one 64x64 px region
    uint32_t view;         // bit 31 (kBigCovered): the item covers its region and has bid for it -- k_raster_cover draws the winner, k_raster_big the others
    uint32_t id;           // draw << 1 | fan   (kNoTri = empty slot)
    uint32_t region;       // ry << 16 | rx  (64 px units)
    int32_t X[3], Y[3];    // the snapped vertices: the consumer re-runs the exact integer setup on them
    float z[3];
};

struct RareItem {          // a triangle the lean raster kernel does not handle itself: >= 64 px across, or near-clipped
    uint32_t view;
    uint32_t draw;         // tile rank * tris_per_tile + triangle
};

struct FrameParams {
    const TileDev* tiles;      // n_tiles entries in draw order (BTreeMap order, terrain_renderer.rs:407)
    const ViewDev* views;      // n_views
    uint64_t* vis;             // n_views * W * H visibility keys: depth bits << 32 | id
    uint8_t* dirty;            // one byte per 64 consecutive keys: 1 = some key of the segment was written this frame
    WorkItem* work;
    uint32_t* counters;        // kCounterWords words (kCtr*, below); two sets per frame context, alternating: a frame's set was zeroed by the clear of the frame before
    uint32_t* status_out;      // pinned host memory, or null: k_resolve's first workgroup stores the frame's kStatusWords counter words there (nothing
                               // changes them once the raster kernels are done), instead of a copy operation behind the frame
    BigItem* big;
    RareItem* rare;
    FarItem* far;              // far candidates (k_cull -> k_occlusion)
    WorkItem* work2;           // far survivors (k_occlusion -> second k_raster)
    uint32_t work_cap, big_cap, rare_cap;   // work_cap: entries of work2 (one per block and view)
    uint32_t far_sub_cap;                   // entries of each of the kFarLists sub-lists of `far` (enough for every candidate its workgroups can produce)
    uint32_t near_cap;                      // entries of work / work2 (ceil(15 / near_strip) strips per block)
    uint32_t near_strip;                    // cell rows per strip of a near block / far survivor (1 .. 15)
    float split_m;             // view depth (m) beyond which a block is an occlusion-test candidate; 0 = feature off
    uint32_t n_views, n_tiles;
    int32_t W, H;
    uint32_t tile_w, tile_h;
    uint32_t bx_count, by_count;
    uint32_t tris_per_tile;
    FastDiv div_tris, div_hm1;   // exact division by tris_per_tile / (tile_h - 1)
    uint32_t sky_c8;           // the cleared render-target texel (clear colour encoded for the target format), R G B A from the low byte
    uint32_t linear_target;    // 1: plain *Unorm targets (no sRGB encode/decode); 0: *UnormSrgb
    uint32_t bgra;             // 1: output texels are B G R A in memory
    uint32_t rblocks_x, rblocks_view;             // k_resolve's 64 x (4 RPW) px blocks: per row of a view, per view
    uint32_t post_off;         // 1: k_resolve stores the RENDER TARGET texel (no post pass), always R G B A -- the pixelise branch
                               // samples that image in a pass of its own (k_post_pixelize)
    uint32_t rblock_first, rblock_count;          // the blocks THIS launch of k_resolve shades (a frame can be resolved in several
                                                  // launches -- by view and band of rows -- so that an exchange of the finished part
                                                  // runs under the rest: topo_render_panorama)
    FastDiv div_rblocks_x, div_rblocks_view;
};

// Regions one near-field giant covers whole (k_raster_rare bids for them, k_raster_cover writes them with plain stores).  Per frame
// context: `owner`, one 64-bit word per (view, 64 x 64 px region) of the submission -- the largest bid so far, serial of the frame
// << 32 | big-queue index of the bidding item (atomicMax: a word of an older frame loses against any bid, so nothing has to be
// reset between frames).  serial == 0: the path is off.
// `recs`, beside them: the records of the claimed regions' strips (topo_pipeline.h: owned_record_index), 8 per region of
// kOwnedRecWords words each, written by k_raster_cover for the regions this frame's serial won and read by k_resolve, which then
// neither lists the winners of a strip all of whose pixels the owner has won nor computes its record again.  The same discipline:
// zeroed once, a record carries its frame's serial and one of an older frame never matches.  Null: k_resolve takes every strip
// the long way (TOPO_RESOLVE_OWNED=0).
struct CoverParams {
    uint64_t* owner;
    uint32_t serial;
    uint32_t cap;              // words of owner: n_views * regions_x * regions_y
    uint32_t regions_x, regions_y;
    uint32_t* recs;            // cap * 8 records, or null
};

struct OutputParams {
    uint8_t* rgba;             // device pointer
    size_t rgba_view_stride, rgba_pitch;   // bytes
    float* depth;              // device pointer or null
    size_t depth_view_stride, depth_pitch; // bytes
};

constexpr uint32_t kStatusBigOverflow = 1u;    // big-triangle queue full: handled in-lane (slower, still exact)
constexpr uint32_t kStatusRareOverflow = 2u;   // rare-triangle queue full: triangles were DROPPED -> the frame is invalid
constexpr uint32_t kFarLists = 64;             // the far-candidate list is kept as 64 sub-lists, each with a counter on a cache line of its own
constexpr uint32_t kStatusWords = 16;          // queue counters and status words of one frame: what reaches the host (the status ring)
constexpr uint32_t kCounterWords = kStatusWords + 16 * kFarLists;      // ... then the sub-list counters, each on a cache line of its own
constexpr uint32_t kBigCovered = 0x80000000u;   // BigItem::view flag (a submission holds far fewer views)
constexpr uint32_t kStatusBounds = 4u;         // TOPO_BOUNDS_CHECK build only: an out-of-range index was formed (and not used);
                                               // kCtrBoundsTag = site tag, kCtrBoundsLo / Hi = the offending value
// the words of a counter set
constexpr uint32_t kCtrWork = 0, kCtrBig = 1;                  // near work items, big-triangle items
constexpr uint32_t kCtrStatus = 2;                             // kStatus* bits
constexpr uint32_t kCtrRare = 3;                               // rare-triangle entries WANTED (beyond rare_cap: dropped)
constexpr uint32_t kCtrFarTested = 4, kCtrFarSurvived = 5;     // occlusion-test candidates, survivors (work2 entries)
constexpr uint32_t kCtrBigStart = 6, kCtrRareStart = 7;        // where the current phase's big / rare items start
constexpr uint32_t kCtrBoundsTag = 8, kCtrBoundsLo = 9, kCtrBoundsHi = 10;      // the first bounds violation (check build)
constexpr uint32_t far_list_counter(uint32_t q) { return kStatusWords + 16 * q; }      // the counter of far sub-list q

// load phase (add_terrain).  Every pass of the reference's add_terrain writes a disjoint set of texels (interior
// / one seam per adjacent pair / one corner per 2x2 block), so any number of them can run in one launch each;
// jobs name tiles by their index in the device tile table.
struct EdgeJob {           // compute_normals_left_right / _top_bottom (compute_normals_edge_shader.wgsl)
    uint32_t lt, rb;       // left-or-top tile, right-or-bottom tile
    uint32_t uni;          // the tile whose uniforms the pass reads: the one that was inserted last
    uint32_t top_bottom;
};
struct CornerJob {         // compute_normals_corner (compute_normals_corner_shader.wgsl)
    uint32_t lt, rt, lb, rb;
    uint32_t uni;
};

void launch_block_tables(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s);   // block min/max, cull bounds, sin/cos tables of `count` tiles
// The load path that reads the DEM once, taken when normals_tables_fused(): launch_trig_tables -> launch_normals_tables (interior
// normals AND the block minima / maxima) -> launch_block_bounds (the f64 cull bounds from them) [-> launch_normals_border].
bool normals_tables_fused(uint32_t w, uint32_t h, int lds_rows);
void launch_trig_tables(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s);
void launch_normals_tables(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s);
void launch_block_bounds(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s);
// interior normals of tiles[first .. first+count); also zeroes their border ring (fresh Rgba8Unorm texture)
void launch_normals_interior(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, int lds_rows,
                             hipStream_t s);
void launch_normals_border(const TileDev* tiles, const EdgeJob* edges, uint32_t n_edges, const CornerJob* corners, uint32_t n_corners, uint32_t w,
                           uint32_t h, hipStream_t s);      // the seam and corner passes of any number of jobs, one launch

// frame phase (render)
// `zero`: the counter set of the NEXT frame (the two sets of a frame context alternate), zeroed by the clear
// A submission's view constants travel as a kernel argument (up to kPackViews views = 704 bytes): the launch copies them, so the
// caller's array is free at once and no staging slot, copy-engine operation or event stands in front of the frame.
constexpr uint32_t kPackViews = 8;
struct ViewPack { ViewDev v[kPackViews]; };
void launch_put_views(const ViewPack& pack, uint32_t n, ViewDev* dst, hipStream_t s);
// (`start` / `stop`, where a launcher has them: events that take the kernel's own start / end time -- hipExtLaunchKernel: the
// dispatch's completion signal carries both, no marker packet stands between two kernels)
// The cull's grid: every (view, tile) pair (`pairs` null), or the n_pairs <= kMaxCullPairs pairs the host's tile prefilter kept
// (host_math.hpp: tile_prefilter), each a 16-bit code view * n_tiles + rank; the list travels in the launch's argument segment.
// n_pairs == 0: nothing to cull (launch_clear_cull still clears).
constexpr uint32_t kMaxCullPairs = 1024;
void launch_clear(const FrameParams& p, uint32_t* zero, hipStream_t s, hipEvent_t start = nullptr);        // re-initialises the marked segments
void launch_clear_cull(const FrameParams& p, uint32_t* zero, hipStream_t s, hipEvent_t start = nullptr, const ViewPack* pack = nullptr, uint32_t n_pack_views = 0,
                       const uint16_t* pairs = nullptr, uint32_t n_pairs = 0);   // the clear and the cull in one launch, side by side
void launch_cull(const FrameParams& p, hipStream_t s, const uint16_t* pairs = nullptr, uint32_t n_pairs = 0);
// workgroups of the cull (256 raster blocks each) for a submission's shape: the larger of the two grids, which sizes the far sub-lists
size_t cull_workgroups_max(uint32_t n_views, uint32_t n_tiles, uint32_t blocks_per_tile);
void launch_raster(const FrameParams& p, int phase, hipStream_t s);   // phase 0: near list, 1: far survivors
void launch_occlusion(const FrameParams& p, hipStream_t s);
void launch_raster_rare(const FrameParams& p, const CoverParams& cover, hipStream_t s);      // cover.serial != 0 (the near phase only): covering items bid for their regions
void launch_raster_cover(const FrameParams& p, const CoverParams& cover, hipStream_t s);     // between the near phase's launch_raster_rare and launch_raster_big
void launch_raster_big(const FrameParams& p, const CoverParams& cover, hipStream_t s);          // cover: the near phase's, as passed to launch_raster_rare
// cover: the frame's (the strip records k_raster_cover left: CoverParams::recs); CoverParams{}: every strip the long way
void launch_resolve(const FrameParams& p, const OutputParams& o, const CoverParams& cover, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// viewshed (topo_viewshed_*), behind the frame's last k_resolve: the DEM cells that won a pixel, OR-ed into per-tile bit masks.
// masks: device table, rank -> the tile's mask (bit = cell = x (h-1) + y); stats: kViewshedStatSlots x 4 counters (k_viewshed).
constexpr uint32_t kViewshedStatSlots = 1024;
void launch_viewshed(const FrameParams& p, uint32_t* const* masks, unsigned long long* stats, hipStream_t s);

// horizon (topo_horizon_*), behind a finished submission: per queried view and column, the topmost pixel whose key names a
// triangle, decoded to its tile and cell.  Reads the submission's keys, marks and status word; writes only `out`.
struct HorizonPoint {      // = topo_horizon_point (32 bytes)
    int32_t row;
    float depth;
    int32_t lat, lon;
    uint32_t cell_x, cell_y, fan, reserved;
};
struct HorizonParams {
    const uint64_t* vis;          // the submission's keys: n_keys = n_views * W * H
    const uint8_t* dirty;         // its segment marks, one per 64 keys
    const uint32_t* counters;     // its counter set (status word kCtrStatus)
    uint32_t* check;              // TOPO_BOUNDS_CHECK build: kStatusWords-word status record of the query (bounds violations); else unused
    const int32_t* tile_ll;       // rank -> (lat, lon) of the submission's tile order, n_tiles pairs
    HorizonPoint* out;            // view v's records at out + v * view_stride
    size_t view_stride;           // records
    size_t n_keys;
    uint32_t first_view, n_views; // the views queried
    uint32_t W, H;
    uint32_t n_tiles, tris_per_tile, hm1;
    FastDiv div_tris, div_hm1;
};
void launch_horizon(const HorizonParams& p, hipStream_t s);

// ground (topo_ground_*), behind a finished submission: the terrain point under a pixel, from its key's triangle, the tile's DEM
// and the view's camera_proj in f64 (topo_ground.h).  Reads what k_horizon reads plus the tile table and the DEMs; writes only `out`.
struct GroundPoint {       // = topo_ground_point (64 bytes)
    double lon_deg, lat_deg;
    float height_m, range_m, depth;
    int32_t kind;
    int32_t tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, fan;
    float w1, w2;
};
struct GroundQuery { uint32_t view, x, y, reserved; };      // = topo_ground_query
struct GroundParams {
    HorizonParams q;              // the submission as a query sees it (out / view_stride unused; first_view, n_views: the map's views)
    const TileDev* tiles;         // the tile table in the submission's draw order
    const GroundView* views;      // sub_views entries: every view of the submission
    const double* trig;           // the tiles' f64 (cos, sin) tables of their columns' longitudes and rows' latitudes (topo_ground.h), draw order
    size_t trig_doubles;          // their size: n_tiles * ground_table_doubles(tile_w, tile_h)
    uint32_t tile_w, tile_h;
    uint32_t sub_views;
};
void launch_ground_tables(const TileDev* tiles, uint32_t n_tiles, double* trig, uint32_t w, uint32_t h, hipStream_t s);
void launch_ground(const GroundParams& p, const GroundQuery* queries, GroundPoint* out, uint32_t n, hipStream_t s);
// float4 (lon, lat, height, range) per pixel of views [p.q.first_view, + p.q.n_views): view i at out + i * view_stride, rows pitch apart (bytes)
void launch_ground_map(const GroundParams& p, float* out, size_t view_stride, size_t pitch, hipStream_t s);

// rays (topo_raycast_*): n rays against the resident tiles (topo_los.h); needs no submission.  Reads the tile table, the DEMs and the
// block tables, the tiles' f64 tables and spheres; writes only `out`.
static_assert(kLosBCX == kBCX && kLosBCY == kBCY, "topo_los.h walks the raster blocks");
struct RayHit {            // = topo_ray_hit (64 bytes)
    double t, lon_deg, lat_deg;
    float height_m;
    int32_t kind;
    int32_t tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, front;
    float w1, w2;
};
struct RayParams {
    LosScene s;
    const int32_t* tile_ll;       // rank -> (lat, lon), n_tiles pairs
    uint32_t* check;              // TOPO_BOUNDS_CHECK build: the queries' status record; else unused
};
void launch_raycast(const RayParams& p, const LosRay* rays, RayHit* out, uint32_t n, hipStream_t s);      // (a wave per ray; -DTOPO_RAYCAST_LANE: a lane per ray)
// one byte (kSun*: topo_los.h) per pixel of views [g.q.first_view, + g.q.n_views) of a finished submission under a sun in direction
// `sun` (unit): view i at out + i * view_stride, rows pitch apart (bytes)
void launch_sunlit_map(const GroundParams& g, const LosScene& scene, const double sun[3], uint8_t* out, size_t view_stride, size_t pitch, hipStream_t s);

// surface (topo_surface_*, topo_profile_*): the drawn terrain under a longitude and latitude (topo_surface.h); needs no submission.
// Reads the tile table, the DEMs and the tiles' f64 tables (RayParams: the rays' scene); writes only its outputs.
struct SurfacePoint {      // = topo_surface_point (48 bytes)
    double height_m;
    float slope_deg, aspect_deg;
    int32_t kind;
    int32_t tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri;
    float w1, w2;
};
struct ProfileSummary {    // = topo_profile_summary (16 bytes)
    float min_clearance_m;
    uint32_t min_sample, n_terrain;
    int32_t kind;
};
void launch_surface(const RayParams& p, const double* lonlat, SurfacePoint* out, uint32_t n, hipStream_t s);      // n (lon, lat) pairs, degrees
// f32 heights at lon0 + c dlon, lat0 + r dlat for c < nx, r < ny, rows pitch bytes apart; ceil(nx / 64) * ny < 2^32
void launch_surface_grid(const RayParams& p, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny, float* out, size_t pitch, hipStream_t s);
// m samples (terrain, line) of each of n segments at samples + i * stride bytes (samples null: none), and the segments' summaries
void launch_profile(const RayParams& p, const LosRay* segs, uint32_t n, uint32_t m, float* samples, size_t stride, ProfileSummary* summary, hipStream_t s);

// map view (topo_map_*): relief, contours and the viewshed over a lon / lat raster (topo_map.h); needs no submission.  Reads what the
// surface queries read, the tiles' normals and, with the seen layer, the viewshed masks; writes only its outputs (each nullable).
struct MapCall;          // the call's parameters and the masks (topo_map.h)
// pixel (c, r): four bytes at rgba + r * rgba_pitch + 4 c, one at flags + r * flags_pitch + c; ceil(nx / 64) * ny < 2^32
void launch_map(const RayParams& p, const MapCall& m, uint8_t* rgba, size_t rgba_pitch, uint8_t* flags, size_t flags_pitch, hipStream_t s);
uint32_t map_rows_per_wave();      // R: the rows a wave of k_map owns (the tests are sized by it)

// visibility (topo_visibility_*): what observers see of the drawn terrain (topo_visibility.h); needs no submission.  Reads what the
// rays read (RayParams); writes only the observer table and its outputs.
struct VisObserver;      // = topo_observer (topo_visibility.h)
struct VisEye;           // a resolved observer: an entry of the context's table
void launch_visibility_observers(const RayParams& p, const VisObserver* obs, VisEye* eyes, uint32_t n, hipStream_t s);      // n <= 64
// one byte (kVis*) per (observer o, row r, column c) at out + o * layer_stride + r * pitch + c for the targets lon0 + c dlon,
// lat0 + r dlat at target_height; ceil(nx / 64) * ny * n_observers < 2^32
void launch_visibility_grid(const RayParams& p, const VisEye* eyes, uint32_t n_observers, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny,
                            double target_height, uint8_t* out, size_t layer_stride, size_t pitch, hipStream_t s);
// the same for n (lon, lat) pairs: out[o * list_stride + i]
void launch_visibility_list(const RayParams& p, const VisEye* eyes, uint32_t n_observers, const double* lonlat, uint32_t n, double target_height, uint8_t* out,
                            size_t list_stride, hipStream_t s);
// refracted visibility (topo_visibility_refracted_*): the same two forms on the mesh lifted for each observer with coefficient k
// (topo_refraction.h; 0 <= k < 1, checked by the caller); the observers are those launch_visibility_observers resolved
void launch_visibility_refracted_grid(const RayParams& p, const VisEye* eyes, uint32_t n_observers, double lon0, double lat0, double dlon, double dlat, uint32_t nx,
                                      uint32_t ny, double target_height, double k, uint8_t* out, size_t layer_stride, size_t pitch, hipStream_t s);
void launch_visibility_refracted_list(const RayParams& p, const VisEye* eyes, uint32_t n_observers, const double* lonlat, uint32_t n, double target_height, double k,
                                      uint8_t* out, size_t list_stride, hipStream_t s);

// skyline (topo_skyline_*): per (observer, azimuth) the highest terrain crossing of the vertical half-plane from the observer
// (topo_skyline.h); needs no submission.  Reads what the rays read (RayParams) and the table of resolved observers
// (launch_visibility_observers); writes only its outputs.
struct SkySample {         // = topo_skyline_sample (64 bytes)
    double elevation_deg, range_m, lon_deg, lat_deg;
    float height_m;
    int32_t kind;
    int32_t tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, edge;
};
struct SkyOut {            // each null or: observer o's n_az entries at + o * stride (bytes)
    uint8_t* elevation;    // f32
    size_t elevation_stride;
    uint8_t* samples;      // SkySample
    size_t samples_stride;
};
// azimuth k = az0 + k daz (degrees); n_observers * n_az < 2^32
void launch_skyline(const RayParams& p, const VisEye* eyes, uint32_t n_observers, double az0, double daz, uint32_t n_az, double min_range, double max_range,
                    const SkyOut& out, hipStream_t s);

// sun exposure (topo_sun_exposure_*): per target the LIT and SHADOW masks over the call's suns and the weighted exposure (topo_sun.h);
// needs no submission.  Reads what the rays read (RayParams) and the suns (device memory, n_suns <= 64 normalised records); writes
// only its outputs, each nullable.
struct SunDir;           // = topo_sun with a unit direction (topo_sun.h)
// row r, column c: masks at + r * mask_pitch + 8 c, exposure at + r * exposure_pitch + 4 c (bytes) for the targets lon0 + c dlon,
// lat0 + r dlat; ceil(nx / 64) * ny < 2^32
void launch_sun_exposure_grid(const RayParams& p, const SunDir* suns, uint32_t n_suns, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny,
                              uint64_t* lit, uint64_t* shadow, float* exposure, size_t mask_pitch, size_t exposure_pitch, hipStream_t s);
// the same for n (lon, lat) pairs: entry i at [i] of each output
void launch_sun_exposure_list(const RayParams& p, const SunDir* suns, uint32_t n_suns, const double* lonlat, uint32_t n, uint64_t* lit, uint64_t* shadow, float* exposure,
                              hipStream_t s);

// peak labels (topo_labels_*): per image of views_per_image consecutive views the peaks its depth shows and the label row of each
// (topo_labels.h); needs no submission and no tile.  Reads the views' matrices, the depth images, the peaks and the widths; writes only
// its outputs (state nullable).
struct LabelRec;         // = topo_label (topo_labels.h)
struct LabelParams {
    const float* projs;           // n_views matrices of 16 floats (camera_proj), device memory written before the launch
    const uint8_t* depth;         // view k at + k * depth_view_stride, rows depth_pitch apart (bytes)
    size_t depth_view_stride, depth_pitch;
    const float* peaks;           // n_peaks ECEF xyz
    const float* widths;          // n_peaks
    LabelRec* labels;             // image i: the first `cap` placed at + i * cap
    uint32_t* counts;             // image i: the number placed
    uint8_t* state;               // image i, peak p: at [i * n_peaks + p]
    uint32_t* check;              // TOPO_BOUNDS_CHECK build: the queries' status record; else unused
    uint32_t n_views, n_images, views_per_image, width, height, n_peaks, max_rows, cap;
    uint32_t waves;               // images per workgroup (set by the launcher)
    float row_height;
};
// max_rows <= 64 and views_per_image * width * max_rows <= 524288 (else nothing is launched)
void launch_labels(LabelParams p, hipStream_t s);

// unwrap (topo_unwrap_*): n_views views of src_w x src_h that share an eye, resampled into one out_w x out_h azimuth / elevation
// image (topo_unwrap.h).  Reads the tables and the source images; writes only the outputs given (each nullable; rgba_out needs
// rgba_src, depth_out needs depth_src).
struct UnwrapParams {
    const double* tab;            // the f64 tables: unwrap_table_doubles(n_views, out_w, out_h) doubles (host_math.hpp: unwrap_tables)
    const uint8_t* rgba_src;      // view k at + k * rgba_view_stride, rows rgba_pitch apart (bytes)
    size_t rgba_view_stride, rgba_pitch;
    const uint8_t* depth_src;
    size_t depth_view_stride, depth_pitch;
    uint8_t* rgba_out;            // rows *_out_pitch apart (bytes; pointers and pitches multiples of 16)
    size_t rgba_out_pitch;
    uint8_t* depth_out;
    size_t depth_out_pitch;
    uint8_t* src_out;             // int32 source map
    size_t src_out_pitch;
    uint32_t* check;              // TOPO_BOUNDS_CHECK build: the queries' status record; else unused
    uint32_t n_views, src_w, src_h, out_w, out_h;
    uint32_t blocks_x;            // workgroups per four output rows: ceil(out_w / 256) (set by the launcher)
    uint32_t srgb;                // 1: *Srgb format (bilinear blends in linear light)
};
void launch_unwrap(const UnwrapParams& p, bool bilinear, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// summits (topo_summits_*, topo_summit_snap_*): the posts of the resident DEMs no higher post stands near, and the best post around a
// point (topo_summits.h); needs no submission.  Reads what the rays read (RayParams); writes only its scratch and its outputs.
struct SummitRec {         // = topo_summit (64 bytes)
    double lon_deg, lat_deg, isolation_m;
    float height_m, higher_height_m;
    int32_t tile_lat, tile_lon;
    uint32_t vx, vy;
    int32_t higher_tile_lat, higher_tile_lon;
    uint32_t higher_vx, higher_vy;
};
struct SummitSnapRec {     // = topo_summit_snap (48 bytes)
    double lon_deg, lat_deg, distance_m;
    float height_m;
    int32_t status;
    int32_t tile_lat, tile_lon;
    uint32_t vx, vy;
};
struct SummitCall {
    double radius, min_isolation;
    float min_height;
};
// The scratch of one band of at most `posts` posts in `waves` waves (rows * ceil(tile_w / 64)): 5 bytes per post, 12 per wave.
constexpr uint32_t kSummitBandPosts = 1u << 22;      // the default band: as many whole rows as hold at most this many posts (one row at least) -- 20 MiB + 1.5 MiB of scratch
// the words of the state record: the band's candidates and survivors, the call's summits so far, the number of the band's first
// summit, the call's candidates so far (topo_debug_summit_counts)
constexpr uint32_t kSummitStateCandidates = 0, kSummitStateSurvivors = 1, kSummitStateTotal = 2, kSummitStateBase = 3, kSummitStateSeen = 4;
constexpr uint32_t kSummitStateWords = 8;            // candidates and survivors of the band, summits so far, the band's first record, candidates so far
struct SummitScratch {
    uint64_t* wave_mask;     // waves
    uint32_t* wave_count;    // waves
    uint32_t* candidates;    // posts: post indices of the band's tile, ascending
    uint8_t* keep;           // posts
    uint32_t* state;         // kSummitStateWords, zero at the start of a call
    uint32_t posts, waves;   // what the lists above have room for: the kernels' index checks are against these
};
void launch_summits_band(const RayParams& p, const SummitCall& c, uint32_t rank, uint32_t y0, uint32_t rows, const SummitScratch& x, SummitRec* out, uint32_t capacity,
                         hipStream_t s);
void launch_summits_finish(const RayParams& p, const SummitCall& c, const SummitScratch& x, SummitRec* out, uint32_t capacity, hipStream_t s);      // once, behind the last band
void launch_summit_snap(const RayParams& p, const double* lonlat, double radius, SummitSnapRec* out, uint32_t n, hipStream_t s);      // a wave per point

// overlay pass (line_shader.wgsl over the post pass's image): keys = W*H overlay keys, (re-)initialised when keys_fresh
void launch_overlay(const OverlayVertex* verts, const uint32_t* idx, uint32_t n_tris, uint32_t n_verts, float width, int32_t W, int32_t H, uint64_t* keys,
                    bool keys_fresh, uint8_t* rgba, size_t pitch, uint32_t linear_target, uint32_t bgra, hipStream_t s);

// depth consumer (RenderEngine::get_visible_labels, render_engine.rs:338-396)
void launch_overlay_glyphs(const GlyphInstance* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas, uint32_t aw, uint32_t ah, int32_t W, int32_t H,
                           uint64_t* keys, bool keys_fresh, uint8_t* rgba, size_t pitch, uint32_t linear_target, uint32_t bgra, hipStream_t s);
void launch_post_pixelize(uint32_t n_views, int32_t W, int32_t H, float vw, float vh, float pixelize_n, const uint8_t* pre_rgba, const OutputParams& out,
                          const float* depth, size_t depth_view_stride, size_t depth_pitch, uint32_t linear_target, uint32_t bgra, hipStream_t s);
void launch_visible_peaks(const float* proj16_dev, uint32_t w, uint32_t h, const float* depth, size_t depth_pitch, uint32_t n,
                          const float* peaks_xyz, uint8_t* visible, uint32_t* xy, hipStream_t s);

// unit-test probes
// GeoTIFF decode, device half: one workgroup per stored row of a strip/tile (geotiff.hpp).
struct TiffSegDev {
    uint64_t byte_off;       // of the segment's decompressed bytes in the staging buffer
    uint32_t row0;           // index of its first row in the global row list
    uint32_t x0, y0, w, h;   // position in the image, stored size
    uint32_t pad_;
};
void launch_tiff_rows(uint8_t* bytes, const TiffSegDev* segs, const uint32_t* row_seg, uint32_t n_rows, float* out, uint32_t W, uint32_t H,
                      uint32_t predictor, bool big_endian, hipStream_t s);
void launch_probe_sincos(const float* x, float* s, float* c, size_t n, hipStream_t st);
void launch_probe_div(int kind, const float* x, const float* y, float* out, size_t n, hipStream_t st);

}  // namespace topo
