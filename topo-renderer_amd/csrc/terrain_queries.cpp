// terrain_queries.cpp -- the queries of TerrainRenderer (viewshed, horizon, ground, rays and the sunlit layer, surface, map views, visibility, skyline, sun exposure, peak labels, unwrap), the tile-set
// tables they read and their handle on the latest submission.  The frame path is terrain_renderer.cpp (see terrain_renderer.hpp).
#include "terrain_renderer.hpp"
#include "topo_labels.h"
#include "topo_map.h"
#include "topo_surface.h"
#include "topo_skyline.h"
#include "topo_summits.h"
#include "topo_sun.h"
#include "topo_refraction.h"
#include "topo_visibility.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace topo {

static_assert(sizeof(HorizonPoint) == sizeof(topo_horizon_point) && sizeof(topo_horizon_point) == 32, "horizon record layout");
static_assert(sizeof(GroundPoint) == sizeof(topo_ground_point) && sizeof(topo_ground_point) == 64, "ground record layout");
static_assert(sizeof(GroundQuery) == sizeof(topo_ground_query) && sizeof(topo_ground_query) == 16, "ground query layout");
static_assert(sizeof(LosRay) == sizeof(topo_ray) && sizeof(topo_ray) == 64, "ray layout");
static_assert(sizeof(RayHit) == sizeof(topo_ray_hit) && sizeof(topo_ray_hit) == 64, "ray record layout");
static_assert(sizeof(SurfacePoint) == sizeof(topo_surface_point) && sizeof(topo_surface_point) == 48, "surface record layout");
static_assert(sizeof(ProfileSummary) == sizeof(topo_profile_summary) && sizeof(topo_profile_summary) == 16, "profile summary layout");
static_assert(kSurfaceTerrain == TOPO_SURFACE_TERRAIN && kSurfaceNone == TOPO_SURFACE_NONE && kSurfaceInvalid == TOPO_SURFACE_INVALID, "surface kinds");
static_assert(sizeof(VisObserver) == sizeof(topo_observer) && sizeof(topo_observer) == 32, "observer layout");
static_assert(kVisNone == TOPO_VIS_NONE && kVisVisible == TOPO_VIS_VISIBLE && kVisAway == TOPO_VIS_AWAY && kVisHidden == TOPO_VIS_HIDDEN && kVisNoObserver == TOPO_VIS_NO_OBSERVER &&
                  kObserverAboveTerrain == TOPO_OBSERVER_ABOVE_TERRAIN, "visibility classes");
static_assert(sizeof(SkySample) == sizeof(topo_skyline_sample) && sizeof(topo_skyline_sample) == 64, "skyline record layout");
static_assert(kSkyNone == TOPO_SKY_NONE && kSkyTerrain == TOPO_SKY_TERRAIN && kSkyNoObserver == TOPO_SKY_NO_OBSERVER, "skyline kinds");
static_assert(sizeof(SunDir) == sizeof(topo_sun) && sizeof(topo_sun) == 32, "sun layout");
static_assert(kSunNone == TOPO_SUN_NONE && kSunLit == TOPO_SUN_LIT && kSunAway == TOPO_SUN_AWAY && kSunShadow == TOPO_SUN_SHADOW && kSunNight == TOPO_SUN_NIGHT, "sun classes");
static_assert(sizeof(LabelRec) == sizeof(topo_label) && sizeof(topo_label) == 32 && sizeof(topo_label_params) == 16, "label layouts");
static_assert(sizeof(SummitRec) == sizeof(topo_summit) && sizeof(topo_summit) == 64 && sizeof(SummitSnapRec) == sizeof(topo_summit_snap) && sizeof(topo_summit_snap) == 48 &&
                  sizeof(topo_summit_params) == 24, "summit layouts");
static_assert(kSnapFound == TOPO_SNAP_FOUND && kSnapNone == TOPO_SNAP_NONE && kSnapInvalid == TOPO_SNAP_INVALID && kSummitOrderTile == TOPO_SUMMIT_ORDER_TILE &&
                  kSummitOrderHeight == TOPO_SUMMIT_ORDER_HEIGHT && kSummitOrderIsolation == TOPO_SUMMIT_ORDER_ISOLATION, "summit constants");
static_assert(sizeof(topo_map_params) == 88 && kMapRelief == TOPO_MAP_RELIEF && kMapContours == TOPO_MAP_CONTOURS && kMapSeen == TOPO_MAP_SEEN &&
                  kMapFlagTerrain == TOPO_MAP_FLAG_TERRAIN && kMapFlagContour == TOPO_MAP_FLAG_CONTOUR && kMapFlagIndex == TOPO_MAP_FLAG_INDEX && kMapFlagSeen == TOPO_MAP_FLAG_SEEN,
              "map parameters and constants");
static_assert(kTileSphereDoubles == kLosSphereDoubles, "the cull prefilter and the rays read the same spheres: one gather, one layout");

// ---- viewshed ----------------------------------------------------------------------------------------------------------------

int TerrainRenderer::alloc_mask(Tile& t) {
    DeviceBuffer m;      // (the tile gets it once it is zeroed)
    if (int rc = ensure(stream_, m, mask_bytes())) return rc;
    TOPO_HIP_TRY(hipMemsetAsync(m.p, 0, mask_bytes(), stream_));      // (frames on other streams are ordered after stream_)
    t.mask = std::move(m);
    return TOPO_OK;
}

// The masks are allocated when accumulation is first turned on (for the tiles loaded then; later tiles get theirs in add_terrain) and
// kept until the tile goes; turning accumulation off only stops the launches.
int TerrainRenderer::viewshed_enable(bool on) {
    if (int rc = bind_device()) return rc;
    if (on && !vs_ever_) {
        if (int rc = join()) return rc;
        const size_t stats = (size_t)kViewshedStatSlots * 4 * sizeof(unsigned long long);
        if (!d_vs_stats_.p) {
            if (int rc = ensure(stream_, d_vs_stats_, stats)) return rc;
            TOPO_HIP_TRY(hipMemsetAsync(d_vs_stats_.p, 0, stats, stream_));
        }
        for (auto& kv : tiles_)
            if (!kv.second.mask.p)
                if (int rc = alloc_mask(kv.second)) return rc;
        vs_ever_ = true;
        table_dirty_ = true;      // the next submission uploads the rank -> mask table with the tile table
    }
    vs_on_ = on;
    return TOPO_OK;
}

int TerrainRenderer::viewshed_reset() {
    if (int rc = bind_device()) return rc;
    if (!vs_ever_) return TOPO_OK;
    if (int rc = join()) return rc;      // frames in flight on the contexts' own streams; later ones are ordered after stream_
    for (auto& kv : tiles_) TOPO_HIP_TRY(hipMemsetAsync(kv.second.mask.p, 0, mask_bytes(), stream_));
    TOPO_HIP_TRY(hipMemsetAsync(d_vs_stats_.p, 0, (size_t)kViewshedStatSlots * 4 * sizeof(unsigned long long), stream_));
    return TOPO_OK;
}

int TerrainRenderer::viewshed_read(int32_t lat, int32_t lon, uint8_t* mask_out, size_t pitch, uint64_t* n_visible) {
    if (!mask_out) return fail(TOPO_ERR_INVALID, "mask_out is null");
    Tile* t = find(lat, lon);
    if (!t) return fail(TOPO_ERR_NOT_FOUND, "no such tile");
    if (!vs_ever_) return fail(TOPO_ERR_INVALID, "viewshed accumulation was never enabled");
    const uint32_t wm1 = tile_w_ - 1, hm1 = tile_h_ - 1;
    if (pitch < wm1) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    if (int rc = wait_all()) return rc;
    std::vector<uint32_t> words(mask_bytes() / 4);
    TOPO_HIP_TRY(hipMemcpy(words.data(), t->mask.p, mask_bytes(), hipMemcpyDeviceToHost));
    uint64_t count = 0;
    for (uint32_t x = 0, bit = 0; x < wm1; ++x)      // bit = x (h-1) + y: the cell of the draw id's triangle (triangle_vertices)
        for (uint32_t y = 0; y < hm1; ++y, ++bit) {
            const uint8_t v = (uint8_t)((words[bit >> 5] >> (bit & 31u)) & 1u);
            mask_out[(size_t)y * pitch + x] = v;
            count += v;
        }
    if (n_visible) *n_visible = count;
    return TOPO_OK;
}

int TerrainRenderer::viewshed_stats(uint64_t out[3]) {
    if (!out) return fail(TOPO_ERR_INVALID, "null argument");
    out[0] = out[1] = out[2] = 0;
    if (!vs_ever_) return TOPO_OK;
    if (int rc = wait_all()) return rc;
    std::vector<unsigned long long> s((size_t)kViewshedStatSlots * 4);
    TOPO_HIP_TRY(hipMemcpy(s.data(), d_vs_stats_.p, s.size() * sizeof(s[0]), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < s.size(); i += 4)
        for (int k = 0; k < 3; ++k) out[k] += s[i + k];
    return TOPO_OK;
}

// ---- what the queries share: the tile-set tables, the bounds record, the latest submission -------------------------------------

// The tiles' spheres, gathered once per tile set.  Host memory only -- no HIP call, no wait: the cull prefilter asks on every submission.
const std::vector<double>& TerrainRenderer::tile_spheres() {
    if (tables_.spheres_gen == tile_gen_) return tables_.spheres;
    tables_.spheres.clear();
    for (const auto& kv : tiles_) {      // draw order
        tables_.spheres.insert(tables_.spheres.end(), kv.second.centres, kv.second.centres + 4);
        tables_.spheres.push_back(kv.second.block_radius);
    }
    tables_.spheres_gen = tile_gen_;
    return tables_.spheres;
}

// The tables a query kernel on s reads besides the submission's own, up to `level`; every query calls this once.  A level is rebuilt
// after the tile set changed, once every earlier query has finished (add_terrain / unload_terrain join the frames, a query on a context's
// own stream marks it pending); with current tables nothing waits.  rank -> (lat, lon) is the current tile order: query_begin checked it.
int TerrainRenderer::prepare_tables(TableLevel level, hipStream_t s) {
    if (tables_.decode_gen != tile_gen_) {
        if (int rc = wait_all()) return rc;
        tables_.ll.clear();
        for (const auto& kv : tiles_) tables_.ll.insert(tables_.ll.end(), {kv.second.lat, kv.second.lon});      // draw order
        if (int rc = ensure(stream_, tables_.d_ll, (tables_.ll.size() + 2) * sizeof(int32_t))) return rc;
        if (!tables_.ll.empty()) TOPO_HIP_TRY(hipMemcpyAsync(tables_.d_ll.p, tables_.ll.data(), tables_.ll.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        tables_.decode_gen = tile_gen_;
    }
    if (int rc = ensure_query_check(s)) return rc;
    if (level == kDecodeTables || tables_.geometry_gen == tile_gen_) return TOPO_OK;
    // The tiles' f64 (cos, sin) tables and, for the rays, their spheres.  Nothing that could still read the old tables is left
    // running, and the new ones are complete before a query can be queued on any other stream.
    if (int rc = wait_all()) return rc;
    // The rays need no frame, so the device tile table (and the viewshed's rank -> mask table that travels with it) may still be
    // the one from before an unload: whoever needs it first refreshes it, here as in render_frame.  On the ground queries' path
    // this is a no-op: query_begin has refused a submission whose tile set changed, and a frame uploaded the table before it.
    if (int rc = upload_tile_table()) return rc;
    tables_.trig_doubles = tiles_.size() * ground_table_doubles(tile_w_, tile_h_);
    if (int rc = ensure(s, tables_.d_trig, (tables_.trig_doubles + 2) * sizeof(double))) return rc;
    launch_ground_tables(d_tiles_.as<const TileDev>(), (uint32_t)tiles_.size(), tables_.d_trig.as<double>(), tile_w_, tile_h_, s);
    TOPO_HIP_TRY(hipGetLastError());
    const std::vector<double>& spheres = tile_spheres();
    if (int rc = ensure(s, tables_.d_spheres, (spheres.size() + 2) * sizeof(double))) return rc;
    if (!spheres.empty()) TOPO_HIP_TRY(hipMemcpyAsync(tables_.d_spheres.p, spheres.data(), spheres.size() * sizeof(double), hipMemcpyHostToDevice, s));
    TOPO_HIP_TRY(hipStreamSynchronize(s));
    tables_.geometry_gen = tile_gen_;
    return TOPO_OK;
}

int TerrainRenderer::ensure_query_check([[maybe_unused]] hipStream_t s) {
#ifdef TOPO_BOUNDS_CHECK
    if (!query_.d_check.p) {
        if (int rc = ensure(s, query_.d_check, kStatusWords * sizeof(uint32_t))) return rc;
        TOPO_HIP_TRY(hipMemsetAsync(query_.d_check.p, 0, kStatusWords * sizeof(uint32_t), s));
    }
#endif
    return TOPO_OK;
}

// The bounds-checking build: what the query kernels recorded, into the status topo_frame_status reports (the queries have finished).
int TerrainRenderer::query_fold_check() {
#ifdef TOPO_BOUNDS_CHECK
    if (!query_.d_check.p) return TOPO_OK;
    uint32_t w[kStatusWords];
    TOPO_HIP_TRY(hipMemcpy(w, query_.d_check.p, sizeof w, hipMemcpyDeviceToHost));
    if (w[kCtrStatus] & kStatusBounds) {
        record_bounds(w);
        TOPO_HIP_TRY(hipMemset(query_.d_check.p, 0, sizeof w));
    }
#endif
    return TOPO_OK;
}

// The latest submission, if views [first, first + n) of it can be answered (tiles added, replaced or unloaded since have taken its draw
// order with them), and the stream a query is queued on, behind it (last_stream null: a wait covered it, the stream may be gone).
int TerrainRenderer::query_begin(uint32_t first, uint32_t n, LatestSubmission& q) {
    if (latest_ctx_ < 0) return fail(TOPO_ERR_INVALID, "no submission to query");
    FrameCtx& c = ctx_[latest_ctx_];
    if (c.sub.tile_gen != tile_gen_) return fail(TOPO_ERR_INVALID, "tiles were added or unloaded since the latest submission: its draw order is gone");
    if (n == 0 || first >= c.sub.n_views || n > c.sub.n_views - first) return fail(TOPO_ERR_INVALID, "views outside the latest submission");
    if (int rc = bind_device()) return rc;
    q = LatestSubmission{&c, c.last_stream ? c.last_stream : stream_, c.sub.query.W, c.sub.query.H, c.sub.n_views};
    return TOPO_OK;
}

// The end of a device variant: the query has just been launched on q.s.  On a context's own stream the next join (and whatever
// rewrites the frame: the context's next submission) waits for the query too -- it is still reading the submission's keys.
int TerrainRenderer::query_queued(const LatestSubmission& q) {
    TOPO_HIP_TRY(hipGetLastError());
    if (q.s != stream_) q.c->pending = true;
    return TOPO_OK;
}

// The end of a host read: waits for the submission and the query queued behind it on q.s.  The submission's status is folded as
// topo_render folds its own frame: the frames of its context in front of it go to the next topo_join (their overflow stays pending
// there), and its own overflow is this call's error -- the query of an incomplete frame -- and is not reported again by the next
// topo_join.
int TerrainRenderer::query_finish_read(const LatestSubmission& q, const char* what) {
    TOPO_HIP_TRY(hipStreamSynchronize(q.s));      // (the stream of the context's latest frame: all its frames are done)
    q.c->pending = false;
    const bool overflow = fold_latest(*q.c, false);
    if (int rc = query_fold_check()) return rc;
    if (overflow) return fail(TOPO_ERR_CAPACITY, std::string("rare-triangle queue overflowed: the latest submission is incomplete, and so is its ") + what);
    return TOPO_OK;
}

// A caller's n views of W x H texels of texel_bytes, rows `pitch` and views `view_stride` bytes apart: null, or what is wrong with it.
// (An entry point that wants them aligned says so before query_begin: a bad pointer is refused with or without a submission.)
static const char* view_image_error(uint32_t n, uint32_t W, uint32_t H, size_t texel_bytes, size_t view_stride, size_t pitch) {
    const size_t row = (size_t)W * texel_bytes;
    if (pitch < row) return "pitch smaller than a row";
    if (n > 1 && view_stride < pitch * (H - 1) + row) return "view stride smaller than a view";
    return nullptr;
}

// ---- horizon ------------------------------------------------------------------------------------------------------------------

int TerrainRenderer::horizon_shape(uint32_t* n_views, uint32_t* w, uint32_t* h) {
    if (!n_views || !w || !h) return fail(TOPO_ERR_INVALID, "null argument");
    if (latest_ctx_ < 0) return fail(TOPO_ERR_INVALID, "no submission to query");
    const FrameCtx::Submission& s = ctx_[latest_ctx_].sub;      // (its shape outlives the tile set it was rendered from)
    *n_views = s.n_views;
    *w = s.query.W;
    *h = s.query.H;
    return TOPO_OK;
}

// k_horizon over views [first, first + n) of q into `out` (device), on q.s.  The decode table is all a horizon builds.
int TerrainRenderer::horizon_launch(const LatestSubmission& q, uint32_t first, uint32_t n, HorizonPoint* out, size_t view_stride) {
    if (int rc = prepare_tables(kDecodeTables, q.s)) return rc;
    HorizonParams p = q.c->sub.query;
    p.check = query_.d_check.as<uint32_t>();
    p.tile_ll = tables_.d_ll.as<const int32_t>();
    p.out = out;
    p.view_stride = view_stride;
    p.first_view = first;
    p.n_views = n;
    launch_horizon(p, q.s);
    return TOPO_OK;
}

static const char* const kStrideError = "view stride smaller than a view's width";

// Host read: waits for the submission and the query.
int TerrainRenderer::horizon_read(uint32_t first, uint32_t n, topo_horizon_point* out, size_t view_stride) {
    if (!out) return fail(TOPO_ERR_INVALID, "null argument");
    LatestSubmission q{};
    if (int rc = query_begin(first, n, q)) return rc;
    if (view_stride < q.W) return fail(TOPO_ERR_INVALID, kStrideError);
    const size_t row = (size_t)q.W * sizeof(HorizonPoint);
    if (int rc = ensure(q.s, query_.d_horizon_out, row * n)) return rc;
    if (int rc = horizon_launch(q, first, n, query_.d_horizon_out.as<HorizonPoint>(), q.W)) return rc;
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipMemcpy2DAsync(out, view_stride * sizeof(topo_horizon_point), query_.d_horizon_out.p, row, row, n, hipMemcpyDeviceToHost, q.s));
    return query_finish_read(q, "horizon");
}

// Device variant: queued behind the submission on its stream; an incomplete frame writes row TOPO_HORIZON_INCOMPLETE.
int TerrainRenderer::horizon_device(uint32_t first, uint32_t n, topo_horizon_point* out_dev, size_t view_stride) {
    if (!out_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)out_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "out_dev must be 16-byte aligned");
    LatestSubmission q{};
    if (int rc = query_begin(first, n, q)) return rc;
    if (view_stride < q.W) return fail(TOPO_ERR_INVALID, kStrideError);
    if (int rc = horizon_launch(q, first, n, (HorizonPoint*)out_dev, view_stride)) return rc;
    return query_queued(q);
}

// ---- ground -------------------------------------------------------------------------------------------------------------------

// What a ground kernel over q reads: the geometry tables, and the submission's views, uploaded by its first ground query.
int TerrainRenderer::ground_prepare(const LatestSubmission& q) {
    if (int rc = prepare_tables(kGeometryTables, q.s)) return rc;
    if (FrameCtx& c = *q.c; !c.sub.views_on_device) {
        const size_t bytes = c.sub.views.size() * sizeof(GroundView);
        if (int rc = ensure(q.s, c.d_ground_views, bytes)) return rc;
        TOPO_HIP_TRY(hipMemcpyAsync(c.d_ground_views.p, c.sub.views.data(), bytes, hipMemcpyHostToDevice, q.s));
        c.sub.views_on_device = true;
    }
    return TOPO_OK;
}

// A ground kernel's parameters over views [first, first + n) of q, from what ground_prepare left (the tile table is the submission's).
GroundParams TerrainRenderer::ground_params(const LatestSubmission& q, uint32_t first, uint32_t n) const {
    GroundParams p{};
    p.q = q.c->sub.query;
    p.q.check = query_.d_check.as<uint32_t>();
    p.q.tile_ll = tables_.d_ll.as<const int32_t>();
    p.q.first_view = first;
    p.q.n_views = n;
    p.tiles = d_tiles_.as<const TileDev>();
    p.views = q.c->d_ground_views.as<const GroundView>();
    p.trig = tables_.d_trig.as<const double>();
    p.trig_doubles = tables_.trig_doubles;
    p.tile_w = tile_w_;
    p.tile_h = tile_h_;
    p.sub_views = q.n_views;
    return p;
}

// Host read: every query is checked against the submission's shape first; waits for the submission and the query.
int TerrainRenderer::ground_read(uint32_t n, const topo_ground_query* queries, topo_ground_point* out) {
    if (n == 0 || !queries || !out) return fail(TOPO_ERR_INVALID, "null/empty argument");
    LatestSubmission q{};
    if (int rc = query_begin(0, 1, q)) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (queries[i].view >= q.n_views || queries[i].x >= q.W || queries[i].y >= q.H)
            return fail(TOPO_ERR_INVALID, "a query names a view or pixel outside the latest submission");
    if (int rc = ensure(q.s, query_.d_ground_q, (size_t)n * sizeof(GroundQuery))) return rc;
    if (int rc = ensure(q.s, query_.d_ground_out, (size_t)n * sizeof(GroundPoint))) return rc;
    if (int rc = ground_prepare(q)) return rc;
    TOPO_HIP_TRY(hipMemcpyAsync(query_.d_ground_q.p, queries, (size_t)n * sizeof(GroundQuery), hipMemcpyHostToDevice, q.s));
    launch_ground(ground_params(q, 0, q.n_views), query_.d_ground_q.as<const GroundQuery>(), query_.d_ground_out.as<GroundPoint>(), n, q.s);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipMemcpyAsync(out, query_.d_ground_out.p, (size_t)n * sizeof(GroundPoint), hipMemcpyDeviceToHost, q.s));
    return query_finish_read(q, "ground points");
}

// Device variants: queued behind the submission on its stream.  The list's queries are in device memory, so the kernel checks them:
// one outside the submission answers kind -1; an incomplete frame writes kind -2 (list) or NaN (map).
int TerrainRenderer::ground_device(uint32_t n, const topo_ground_query* queries_dev, topo_ground_point* out_dev) {
    if (n == 0 || !queries_dev || !out_dev) return fail(TOPO_ERR_INVALID, "null/empty argument");
    if ((uintptr_t)out_dev % 16 != 0 || (uintptr_t)queries_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "queries_dev and out_dev must be 16-byte aligned");
    LatestSubmission q{};
    if (int rc = query_begin(0, 1, q)) return rc;
    if (int rc = ground_prepare(q)) return rc;
    launch_ground(ground_params(q, 0, q.n_views), (const GroundQuery*)queries_dev, (GroundPoint*)out_dev, n, q.s);
    return query_queued(q);
}

int TerrainRenderer::ground_map_device(uint32_t first, uint32_t n, float* out_dev, size_t view_stride, size_t pitch) {
    if (!out_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)out_dev % 16 != 0 || view_stride % 16 != 0 || pitch % 16 != 0) return fail(TOPO_ERR_INVALID, "out_dev, the view stride and the pitch must be multiples of 16 bytes");
    LatestSubmission q{};
    if (int rc = query_begin(first, n, q)) return rc;
    if (const char* why = view_image_error(n, q.W, q.H, 16, view_stride, pitch)) return fail(TOPO_ERR_INVALID, why);
    if (int rc = ground_prepare(q)) return rc;
    launch_ground_map(ground_params(q, first, n), out_dev, view_stride, pitch, q.s);
    return query_queued(q);
}

// ---- rays ---------------------------------------------------------------------------------------------------------------------

// The parameters of k_raycast over the resident tiles, from prepared geometry tables.
RayParams TerrainRenderer::ray_params() const {
    RayParams p{};
    const uint32_t n_tiles = (uint32_t)tiles_.size();
    p.s.tiles = d_tiles_.as<const TileDev>();
    p.s.trig = tables_.d_trig.as<const double>();
    p.s.spheres = tables_.d_spheres.as<const double>();
    p.s.trig_doubles = tables_.trig_doubles;
    p.s.n_tiles = n_tiles;
    p.s.tile_w = tile_w_;
    p.s.tile_h = tile_h_;
    p.s.bx_count = n_tiles ? (tile_w_ - 1 + kBCX - 1) / kBCX : 0;
    p.s.by_count = n_tiles ? (tile_h_ - 1 + kBCY - 1) / kBCY : 0;
    p.tile_ll = tables_.d_ll.as<const int32_t>();
    p.check = query_.d_check.as<uint32_t>();
    return p;
}

// Host read: the rays go in and the records come out through one pinned staging buffer; waits for the stream.
int TerrainRenderer::raycast_read(uint32_t n, const topo_ray* rays, topo_ray_hit* out) {
    if (n == 0) return TOPO_OK;
    if (!rays || !out) return fail(TOPO_ERR_INVALID, "null argument");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;      // (refreshes the tile table with them: a tile set changes both or neither)
    const size_t bytes = (size_t)n * sizeof(LosRay);
    if (int rc = ensure(stream_, query_.d_ray_in, bytes)) return rc;
    if (int rc = ensure(stream_, query_.d_ray_out, bytes)) return rc;
    if (bytes > query_.h_ray_stage.cap) TOPO_HIP_TRY(hipStreamSynchronize(stream_));      // (nothing in flight reads the old staging block)
    if (int rc = ensure_pinned(query_.h_ray_stage, bytes)) return rc;
    std::memcpy(query_.h_ray_stage.p, rays, bytes);
    TOPO_HIP_TRY(hipMemcpyAsync(query_.d_ray_in.p, query_.h_ray_stage.p, bytes, hipMemcpyHostToDevice, stream_));
    launch_raycast(ray_params(), query_.d_ray_in.as<const LosRay>(), query_.d_ray_out.as<RayHit>(), n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipMemcpyAsync(query_.h_ray_stage.p, query_.d_ray_out.p, bytes, hipMemcpyDeviceToHost, stream_));
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    std::memcpy(out, query_.h_ray_stage.p, bytes);
    return query_fold_check();
}

// Device variant: queued on stream_, in order.
int TerrainRenderer::raycast_device(uint32_t n, const topo_ray* rays_dev, topo_ray_hit* out_dev) {
    if (n == 0) return TOPO_OK;
    if (!rays_dev || !out_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)rays_dev % 16 != 0 || (uintptr_t)out_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "rays_dev and out_dev must be 16-byte aligned");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    launch_raycast(ray_params(), (const LosRay*)rays_dev, (RayHit*)out_dev, n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// The sunlit layer of views [first, first + n) of the latest submission: topo_ground_map_device's rules, one byte per pixel.  The
// rays' tables are the ground query's, prepared once: with current tables nothing waits in the middle of the stream.
int TerrainRenderer::sunlit_map_device(uint32_t first, uint32_t n, const double sun_dir[3], uint8_t* out_dev, size_t view_stride, size_t pitch) {
    if (!out_dev || !sun_dir) return fail(TOPO_ERR_INVALID, "null argument");
    const double len = std::sqrt(sun_dir[0] * sun_dir[0] + sun_dir[1] * sun_dir[1] + sun_dir[2] * sun_dir[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return fail(TOPO_ERR_INVALID, "sun_dir must be finite and non-zero");
    const double sun[3] = {sun_dir[0] / len, sun_dir[1] / len, sun_dir[2] / len};
    LatestSubmission q{};
    if (int rc = query_begin(first, n, q)) return rc;
    if (const char* why = view_image_error(n, q.W, q.H, 1, view_stride, pitch)) return fail(TOPO_ERR_INVALID, why);
    if (int rc = ground_prepare(q)) return rc;
    launch_sunlit_map(ground_params(q, first, n), ray_params().s, sun, out_dev, view_stride, pitch, q.s);
    return query_queued(q);
}

// ---- surface ------------------------------------------------------------------------------------------------------------------

// Host read: the points go in and the records come out through one pinned staging buffer, as the rays; waits for the stream.
int TerrainRenderer::surface_read(uint32_t n, const double* lonlat_deg, topo_surface_point* out) {
    if (n == 0) return TOPO_OK;
    if (!lonlat_deg || !out) return fail(TOPO_ERR_INVALID, "null argument");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    const size_t in_bytes = (size_t)n * 2 * sizeof(double), out_bytes = (size_t)n * sizeof(SurfacePoint);
    if (int rc = ensure(stream_, query_.d_surface_in, in_bytes)) return rc;
    if (int rc = ensure(stream_, query_.d_surface_out, out_bytes)) return rc;
    if (out_bytes > query_.h_surface_stage.cap) TOPO_HIP_TRY(hipStreamSynchronize(stream_));      // (nothing in flight reads the old staging block)
    if (int rc = ensure_pinned(query_.h_surface_stage, out_bytes)) return rc;
    std::memcpy(query_.h_surface_stage.p, lonlat_deg, in_bytes);
    TOPO_HIP_TRY(hipMemcpyAsync(query_.d_surface_in.p, query_.h_surface_stage.p, in_bytes, hipMemcpyHostToDevice, stream_));
    launch_surface(ray_params(), query_.d_surface_in.as<const double>(), query_.d_surface_out.as<SurfacePoint>(), n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipMemcpyAsync(query_.h_surface_stage.p, query_.d_surface_out.p, out_bytes, hipMemcpyDeviceToHost, stream_));
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    std::memcpy(out, query_.h_surface_stage.p, out_bytes);
    return query_fold_check();
}

// Device variants: queued on stream_, in order.
int TerrainRenderer::surface_device(uint32_t n, const double* lonlat_dev, topo_surface_point* out_dev) {
    if (n == 0) return TOPO_OK;
    if (!lonlat_dev || !out_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)lonlat_dev % 16 != 0 || (uintptr_t)out_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "lonlat_dev and out_dev must be 16-byte aligned");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    launch_surface(ray_params(), lonlat_dev, (SurfacePoint*)out_dev, n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

int TerrainRenderer::surface_grid_device(double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny, float* out_dev, size_t pitch_bytes) {
    if (!out_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if (nx == 0 || ny == 0) return fail(TOPO_ERR_INVALID, "an empty grid");
    if (!std::isfinite(lon0) || !std::isfinite(lat0) || !std::isfinite(dlon) || !std::isfinite(dlat)) return fail(TOPO_ERR_INVALID, "grid parameters must be finite");
    if ((uintptr_t)out_dev % 4 != 0 || pitch_bytes % 4 != 0) return fail(TOPO_ERR_INVALID, "out_dev and the pitch must be multiples of 4 bytes");
    if (pitch_bytes < (size_t)nx * sizeof(float)) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    if ((((uint64_t)nx + 63) / 64) * ny > 0xFFFFFFFFull) return fail(TOPO_ERR_INVALID, "grid too large");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    launch_surface_grid(ray_params(), lon0, lat0, dlon, dlat, nx, ny, out_dev, pitch_bytes, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// ---- map view -----------------------------------------------------------------------------------------------------------------

// What is wrong with a map call's parameters, or null.
static const char* map_params_error(const topo_map_params* p) {
    if (!p) return "params is null";
    if (p->nx == 0 || p->ny == 0) return "an empty grid";
    if (!std::isfinite(p->lon0_deg) || !std::isfinite(p->lat0_deg) || !std::isfinite(p->dlon_deg) || !std::isfinite(p->dlat_deg)) return "grid parameters must be finite";
    if (!(p->contour_interval_m >= 0.0) || !std::isfinite(p->contour_interval_m)) return "the contour interval must be finite and not negative";
    if (p->layers & ~kMapLayers) return "unknown layer bits";
    for (float s : p->sun_direction)
        if (!std::isfinite(s)) return "sun_direction must be finite";
    if ((((uint64_t)p->nx + 63) / 64) * p->ny > 0xFFFFFFFFull) return "grid too large";
    return nullptr;
}

// Device variant: queued on stream_, in order.  Both outputs null: checked, and nothing else.
int TerrainRenderer::map_device(const topo_map_params* params, uint8_t* rgba_dev, size_t rgba_pitch, uint8_t* flags_dev, size_t flags_pitch) {
    if (const char* why = map_params_error(params)) return fail(TOPO_ERR_INVALID, why);
    if (rgba_dev) {
        if ((uintptr_t)rgba_dev % 4 != 0 || rgba_pitch % 4 != 0) return fail(TOPO_ERR_INVALID, "rgba_dev and its pitch must be multiples of 4 bytes");
        if (rgba_pitch < (size_t)params->nx * 4) return fail(TOPO_ERR_INVALID, "rgba pitch smaller than a row");
    }
    if (flags_dev && flags_pitch < params->nx) return fail(TOPO_ERR_INVALID, "flags pitch smaller than a row");
    if ((params->layers & kMapSeen) && !vs_ever_) return fail(TOPO_ERR_INVALID, "viewshed accumulation was never enabled");
    if (!rgba_dev && !flags_dev) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    if (params->layers & kMapSeen) {
        // The frames in flight on the contexts' own streams OR into the masks: they are joined, as viewshed_read joins them (frames on
        // stream_ itself are in order anyway).  The rank -> mask table is brought up to date with the tile table.
        if (int rc = join()) return rc;
        if (int rc = upload_tile_table()) return rc;
    }
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    const MapCall m = map_call(*params, vs_ever_ ? d_vs_table_.as<const uint32_t* const>() : nullptr, (uint32_t)(mask_bytes() / 4), tiles_.size());
    launch_map(ray_params(), m, rgba_dev, rgba_pitch, flags_dev, flags_pitch, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read: densely packed outputs through device buffers of the context; waits for the stream.
int TerrainRenderer::map_read(const topo_map_params* params, uint8_t* rgba, uint8_t* flags) {
    if (const char* why = map_params_error(params)) return fail(TOPO_ERR_INVALID, why);
    if ((params->layers & kMapSeen) && !vs_ever_) return fail(TOPO_ERR_INVALID, "viewshed accumulation was never enabled");
    if (!rgba && !flags) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    const size_t px = (size_t)params->nx * params->ny;
    if (rgba)
        if (int rc = ensure(stream_, query_.d_map_rgba, px * 4)) return rc;
    if (flags)
        if (int rc = ensure(stream_, query_.d_map_flags, px)) return rc;
    if (int rc = map_device(params, rgba ? query_.d_map_rgba.as<uint8_t>() : nullptr, (size_t)params->nx * 4, flags ? query_.d_map_flags.as<uint8_t>() : nullptr, params->nx)) return rc;
    if (rgba) TOPO_HIP_TRY(hipMemcpyAsync(rgba, query_.d_map_rgba.p, px * 4, hipMemcpyDeviceToHost, stream_));
    if (flags) TOPO_HIP_TRY(hipMemcpyAsync(flags, query_.d_map_flags.p, px, hipMemcpyDeviceToHost, stream_));
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    return query_fold_check();
}

// What is wrong with a profile call's shape, or null.
static const char* profile_shape_error(uint32_t n, uint32_t m) {
    if (m < kProfileMinSamples || m > kProfileMaxSamples) return "m must lie in 2 .. 65536";
    if ((uint64_t)n * m >= (1ull << 31)) return "n * m must be below 2^31";
    return nullptr;
}

int TerrainRenderer::profile_device(uint32_t n, const topo_ray* segs_dev, uint32_t m, float* samples_dev, size_t segment_stride_bytes, topo_profile_summary* summary_dev) {
    if (n == 0) return TOPO_OK;
    if (!segs_dev || !summary_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if (const char* why = profile_shape_error(n, m)) return fail(TOPO_ERR_INVALID, why);
    if ((uintptr_t)segs_dev % 16 != 0 || (uintptr_t)summary_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "segs_dev and summary_dev must be 16-byte aligned");
    if (samples_dev) {
        if ((uintptr_t)samples_dev % 8 != 0 || segment_stride_bytes % 8 != 0) return fail(TOPO_ERR_INVALID, "samples_dev and the segment stride must be multiples of 8 bytes");
        if (segment_stride_bytes < (size_t)m * 2 * sizeof(float)) return fail(TOPO_ERR_INVALID, "segment stride smaller than a segment's samples");
    }
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    launch_profile(ray_params(), (const LosRay*)segs_dev, n, m, samples_dev, segment_stride_bytes, (ProfileSummary*)summary_dev, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read.  The caller's memory is pageable and the samples can be gigabytes (8 n m bytes), so nothing is staged: the stream is
// drained, the segments go up with a blocking copy, the kernel runs on the stream -- behind whatever was queued there -- and the
// results come down with blocking copies once it has finished.
int TerrainRenderer::profile_read(uint32_t n, const topo_ray* segs, uint32_t m, float* samples, topo_profile_summary* summary) {
    if (n == 0) return TOPO_OK;
    if (!segs || !summary) return fail(TOPO_ERR_INVALID, "null argument");
    if (const char* why = profile_shape_error(n, m)) return fail(TOPO_ERR_INVALID, why);
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    const size_t in_bytes = (size_t)n * sizeof(LosRay), sum_bytes = (size_t)n * sizeof(ProfileSummary), row = (size_t)m * 2 * sizeof(float);
    if (int rc = ensure(stream_, query_.d_ray_in, in_bytes)) return rc;
    if (int rc = ensure(stream_, query_.d_surface_out, sum_bytes)) return rc;
    if (samples)
        if (int rc = ensure(stream_, query_.d_profile_samples, row * n)) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(query_.d_ray_in.p, segs, in_bytes, hipMemcpyHostToDevice));
    launch_profile(ray_params(), query_.d_ray_in.as<const LosRay>(), n, m, samples ? query_.d_profile_samples.as<float>() : nullptr, row,
                   query_.d_surface_out.as<ProfileSummary>(), stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    if (samples) TOPO_HIP_TRY(hipMemcpy(samples, query_.d_profile_samples.p, row * n, hipMemcpyDeviceToHost));
    TOPO_HIP_TRY(hipMemcpy(summary, query_.d_surface_out.p, sum_bytes, hipMemcpyDeviceToHost));
    return query_fold_check();
}

// ---- visibility ----------------------------------------------------------------------------------------------------------------

// What every visibility call does first: its checks, the tables, and the observers -- host memory -- resolved into the context's
// table by k_visibility_observers on stream_ (behind the kernels of an earlier call that still read it).
int TerrainRenderer::visibility_begin(uint32_t n_observers, const topo_observer* observers, double target_height_m, const double* refraction_k) {
    if (!observers) return fail(TOPO_ERR_INVALID, "null argument");
    if (n_observers > kVisMaxObservers) return fail(TOPO_ERR_INVALID, "at most 64 observers");
    if (!(std::isfinite(target_height_m) && target_height_m >= 0.0 && target_height_m <= kVisMaxTargetHeight))
        return fail(TOPO_ERR_INVALID, "target_height_m must be finite and lie in 0 .. 1e5");
    if (refraction_k && !refraction_k_valid(*refraction_k)) return fail(TOPO_ERR_INVALID, "refraction_k must lie in 0 <= k < 1");
    return resolve_observers(n_observers, observers);
}

// n_observers <= 64 observers (host memory) into the context's table, by k_visibility_observers: the visibility calls' and the skyline's.
int TerrainRenderer::resolve_observers(uint32_t n_observers, const topo_observer* observers) {
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    if (int rc = ensure(stream_, query_.d_vis_observers, kVisMaxObservers * sizeof(VisObserver))) return rc;
    if (int rc = ensure(stream_, query_.d_vis_eyes, kVisMaxObservers * sizeof(VisEye))) return rc;
    TOPO_HIP_TRY(hipMemcpyAsync(query_.d_vis_observers.p, observers, (size_t)n_observers * sizeof(VisObserver), hipMemcpyHostToDevice, stream_));
    launch_visibility_observers(ray_params(), query_.d_vis_observers.as<const VisObserver>(), query_.d_vis_eyes.as<VisEye>(), n_observers, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Device variants: queued on stream_, in order.
int TerrainRenderer::visibility_grid_device(uint32_t n_observers, const topo_observer* observers, double lon0, double lat0, double dlon, double dlat, uint32_t nx,
                                            uint32_t ny, double target_height_m, uint8_t* out_dev, size_t layer_stride_bytes, size_t pitch_bytes,
                                            const double* refraction_k) {
    if (n_observers == 0) return TOPO_OK;
    if (!out_dev || !observers) return fail(TOPO_ERR_INVALID, "null argument");
    if (nx == 0 || ny == 0) return fail(TOPO_ERR_INVALID, "an empty grid");
    if (!std::isfinite(lon0) || !std::isfinite(lat0) || !std::isfinite(dlon) || !std::isfinite(dlat)) return fail(TOPO_ERR_INVALID, "grid parameters must be finite");
    if (pitch_bytes < nx) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    if (layer_stride_bytes / ny < pitch_bytes || layer_stride_bytes < (size_t)ny * pitch_bytes) return fail(TOPO_ERR_INVALID, "layer stride smaller than a layer");
    if (n_observers > kVisMaxObservers) return fail(TOPO_ERR_INVALID, "at most 64 observers");
    if ((((uint64_t)nx + 63) / 64) * ny * n_observers > 0xFFFFFFFFull) return fail(TOPO_ERR_INVALID, "grid too large");
    if (int rc = visibility_begin(n_observers, observers, target_height_m, refraction_k)) return rc;
    if (refraction_k)
        launch_visibility_refracted_grid(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, lon0, lat0, dlon, dlat, nx, ny, target_height_m, *refraction_k,
                                         out_dev, layer_stride_bytes, pitch_bytes, stream_);
    else
        launch_visibility_grid(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, lon0, lat0, dlon, dlat, nx, ny, target_height_m, out_dev,
                               layer_stride_bytes, pitch_bytes, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

int TerrainRenderer::visibility_device(uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_dev, double target_height_m,
                                       uint8_t* out_dev, size_t list_stride_bytes, const double* refraction_k) {
    if (n == 0 || n_observers == 0) return TOPO_OK;
    if (!lonlat_dev || !out_dev || !observers) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)lonlat_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "lonlat_dev must be 16-byte aligned");
    if (list_stride_bytes < n) return fail(TOPO_ERR_INVALID, "list stride smaller than the list");
    if (n_observers > kVisMaxObservers) return fail(TOPO_ERR_INVALID, "at most 64 observers");
    if ((((uint64_t)n + 63) / 64) * n_observers > 0xFFFFFFFFull) return fail(TOPO_ERR_INVALID, "list too large");
    if (int rc = visibility_begin(n_observers, observers, target_height_m, refraction_k)) return rc;
    if (refraction_k)
        launch_visibility_refracted_list(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, lonlat_dev, n, target_height_m, *refraction_k, out_dev,
                                         list_stride_bytes, stream_);
    else
        launch_visibility_list(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, lonlat_dev, n, target_height_m, out_dev, list_stride_bytes, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read: observer o's classes at out + o * n.  The caller's memory is pageable, so nothing is staged (as topo_profile_read):
// the stream is drained, the list goes up and the classes come down with blocking copies.
int TerrainRenderer::visibility_read(uint32_t n_observers, const topo_observer* observers, uint32_t n, const double* lonlat_deg, double target_height_m, uint8_t* out,
                                     const double* refraction_k) {
    if (n == 0 || n_observers == 0) return TOPO_OK;
    if (!lonlat_deg || !out || !observers) return fail(TOPO_ERR_INVALID, "null argument");
    if (n_observers > kVisMaxObservers) return fail(TOPO_ERR_INVALID, "at most 64 observers");
    if ((((uint64_t)n + 63) / 64) * n_observers > 0xFFFFFFFFull) return fail(TOPO_ERR_INVALID, "list too large");
    if (int rc = visibility_begin(n_observers, observers, target_height_m, refraction_k)) return rc;
    const size_t in_bytes = (size_t)n * 2 * sizeof(double), out_bytes = (size_t)n * n_observers;
    if (int rc = ensure(stream_, query_.d_surface_in, in_bytes)) return rc;
    if (int rc = ensure(stream_, query_.d_vis_out, out_bytes)) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(query_.d_surface_in.p, lonlat_deg, in_bytes, hipMemcpyHostToDevice));
    if (refraction_k)
        launch_visibility_refracted_list(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, query_.d_surface_in.as<const double>(), n, target_height_m,
                                         *refraction_k, query_.d_vis_out.as<uint8_t>(), n, stream_);
    else
        launch_visibility_list(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, query_.d_surface_in.as<const double>(), n, target_height_m,
                               query_.d_vis_out.as<uint8_t>(), n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(out, query_.d_vis_out.p, out_bytes, hipMemcpyDeviceToHost));
    return query_fold_check();
}

// ---- skyline --------------------------------------------------------------------------------------------------------------------

// What both skyline calls refuse (their outputs apart).
int TerrainRenderer::skyline_check(uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m,
                                   double max_range_m) {
    if (!observers) return fail(TOPO_ERR_INVALID, "null argument");
    if (n_observers > kSkyMaxObservers) return fail(TOPO_ERR_INVALID, "at most 64 observers");
    if (!std::isfinite(az0_deg) || !std::isfinite(daz_deg)) return fail(TOPO_ERR_INVALID, "az0_deg and daz_deg must be finite");
    if (!(min_range_m > 0.0 && min_range_m <= max_range_m && max_range_m <= kSkyMaxRange))      // (false for a NaN)
        return fail(TOPO_ERR_INVALID, "the ranges must satisfy 0 < min_range_m <= max_range_m <= 1e6");
    if ((uint64_t)n_az * n_observers > 0xFFFFFFFFull) return fail(TOPO_ERR_INVALID, "n_az * n_observers must be below 2^32");
    return TOPO_OK;
}

// Device variant: queued on stream_, in order.
int TerrainRenderer::skyline_device(uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m,
                                    double max_range_m, float* elevation_dev, size_t observer_stride_bytes, topo_skyline_sample* samples_dev, size_t samples_stride_bytes) {
    if (n_observers == 0 || n_az == 0) return TOPO_OK;
    if (int rc = skyline_check(n_observers, observers, az0_deg, daz_deg, n_az, min_range_m, max_range_m)) return rc;
    if (!elevation_dev && !samples_dev) return fail(TOPO_ERR_INVALID, "at least one output must be given");
    if (elevation_dev) {
        if ((uintptr_t)elevation_dev % 4 != 0 || observer_stride_bytes % 4 != 0) return fail(TOPO_ERR_INVALID, "elevation_dev and the observer stride must be multiples of 4 bytes");
        if (observer_stride_bytes / sizeof(float) < n_az) return fail(TOPO_ERR_INVALID, "observer stride smaller than an observer's elevations");
    }
    if (samples_dev) {
        if ((uintptr_t)samples_dev % 16 != 0 || samples_stride_bytes % 16 != 0) return fail(TOPO_ERR_INVALID, "samples_dev and the samples stride must be multiples of 16 bytes");
        if (samples_stride_bytes / sizeof(SkySample) < n_az) return fail(TOPO_ERR_INVALID, "samples stride smaller than an observer's records");
    }
    if (int rc = resolve_observers(n_observers, observers)) return rc;
    launch_skyline(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, az0_deg, daz_deg, n_az, min_range_m, max_range_m,
                   SkyOut{(uint8_t*)elevation_dev, observer_stride_bytes, (uint8_t*)samples_dev, samples_stride_bytes}, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read: observer o's entries at + o * n_az of either output.  The caller's memory is pageable, so nothing is staged (as
// topo_visibility_read): the results come down with blocking copies once the stream has finished.
int TerrainRenderer::skyline_read(uint32_t n_observers, const topo_observer* observers, double az0_deg, double daz_deg, uint32_t n_az, double min_range_m,
                                  double max_range_m, float* elevation, topo_skyline_sample* samples) {
    if (n_observers == 0 || n_az == 0) return TOPO_OK;
    if (int rc = skyline_check(n_observers, observers, az0_deg, daz_deg, n_az, min_range_m, max_range_m)) return rc;
    if (!elevation && !samples) return fail(TOPO_ERR_INVALID, "at least one output must be given");
    if (int rc = resolve_observers(n_observers, observers)) return rc;
    const size_t n = (size_t)n_observers * n_az, el_row = (size_t)n_az * sizeof(float), rec_row = (size_t)n_az * sizeof(SkySample);
    if (elevation)
        if (int rc = ensure(stream_, query_.d_sky_elevation, n * sizeof(float))) return rc;
    if (samples)
        if (int rc = ensure(stream_, query_.d_sky_samples, n * sizeof(SkySample))) return rc;
    launch_skyline(ray_params(), query_.d_vis_eyes.as<const VisEye>(), n_observers, az0_deg, daz_deg, n_az, min_range_m, max_range_m,
                   SkyOut{elevation ? query_.d_sky_elevation.as<uint8_t>() : nullptr, el_row, samples ? query_.d_sky_samples.as<uint8_t>() : nullptr, rec_row}, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    if (elevation) TOPO_HIP_TRY(hipMemcpy(elevation, query_.d_sky_elevation.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (samples) TOPO_HIP_TRY(hipMemcpy(samples, query_.d_sky_samples.p, n * sizeof(SkySample), hipMemcpyDeviceToHost));
    return query_fold_check();
}

// ---- summits --------------------------------------------------------------------------------------------------------------------

int TerrainRenderer::summits_check(const topo_summit_params* params, bool device) {
    if (!params) return fail(TOPO_ERR_INVALID, "null argument");
    if (!(std::isfinite(params->radius_m) && params->radius_m > 0.0 && params->radius_m <= kSummitMaxRadius)) return fail(TOPO_ERR_INVALID, "radius_m must be finite and lie in (0, 1e6]");
    if (!(params->min_isolation_m >= 0.0 && params->min_isolation_m <= params->radius_m)) return fail(TOPO_ERR_INVALID, "min_isolation_m must lie in 0 .. radius_m");
    if (std::isnan(params->min_height_m)) return fail(TOPO_ERR_INVALID, "min_height_m must not be NaN");
    if (params->order > kSummitOrderIsolation) return fail(TOPO_ERR_INVALID, "unknown order");
    if (device && params->order != kSummitOrderTile) return fail(TOPO_ERR_INVALID, "the device variant writes tile order only");
    return TOPO_OK;
}

// The bands of every tile, in tile order, on stream_: the first min(count, capacity) records to out_dev, the count to count_dev.  The
// scratch is one band's (topo_kernels.h: SummitScratch), carved out of one buffer; the state record lies in front of it.
int TerrainRenderer::summits_launch(const topo_summit_params& params, SummitRec* out_dev, uint32_t capacity, uint32_t* count_dev) {
    const uint32_t n_tiles = (uint32_t)tiles_.size();
    const uint32_t fit = std::max(1u, kSummitBandPosts / std::max(1u, tile_w_));
    const uint32_t band = std::min(tile_h_, summit_band_rows_ ? summit_band_rows_ : fit);
    const size_t posts = (size_t)band * tile_w_, waves = (size_t)band * ((tile_w_ + 63) / 64);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_mask = up(kSummitStateWords * sizeof(uint32_t)), o_count = o_mask + up(waves * 8), o_cand = o_count + up(waves * 4), o_keep = o_cand + up(posts * 4),
                 total = o_keep + up(posts);
    if (int rc = ensure(stream_, query_.d_summit_scratch, total)) return rc;
    uint8_t* const base = query_.d_summit_scratch.as<uint8_t>();
    const SummitScratch x{(uint64_t*)(base + o_mask), (uint32_t*)(base + o_count), (uint32_t*)(base + o_cand), base + o_keep, (uint32_t*)base, (uint32_t)posts, (uint32_t)waves};
    TOPO_HIP_TRY(hipMemsetAsync(x.state, 0, kSummitStateWords * sizeof(uint32_t), stream_));
    const RayParams p = ray_params();
    const SummitCall c{params.radius_m, params.min_isolation_m, params.min_height_m};
    for (uint32_t rank = 0; rank < n_tiles; ++rank)
        for (uint32_t y0 = 0; y0 < tile_h_; y0 += band) launch_summits_band(p, c, rank, y0, std::min(band, tile_h_ - y0), x, out_dev, capacity, stream_);
    launch_summits_finish(p, c, x, out_dev, capacity, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipMemcpyAsync(count_dev, x.state + kSummitStateTotal, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream_));      // (the summits so far: all of them)
    return TOPO_OK;
}

// Device variant: queued on stream_, in order.
int TerrainRenderer::summits_device(const topo_summit_params* params, topo_summit* out_dev, uint32_t capacity, uint32_t* count_dev) {
    if (int rc = summits_check(params, true)) return rc;
    if (!count_dev || (!out_dev && capacity)) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)out_dev % 16 != 0 || (uintptr_t)count_dev % 4 != 0) return fail(TOPO_ERR_INVALID, "out_dev must be 16-byte and count_dev 4-byte aligned");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    if (tiles_.empty()) {
        TOPO_HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint32_t), stream_));
        return TOPO_OK;
    }
    return summits_launch(*params, (SummitRec*)out_dev, capacity, count_dev);
}

// Host read.  The caller's memory is pageable, so nothing is staged (as topo_skyline_read): the records come down with a blocking copy
// once the stream has finished.  The full set is needed to order it, so the call runs into a buffer of its own, sized by a first run's
// count when the records of that run did not fit.
int TerrainRenderer::summits_read(const topo_summit_params* params, topo_summit* out, uint32_t capacity, uint32_t* count) {
    if (int rc = summits_check(params, false)) return rc;
    if (!count || (!out && capacity)) return fail(TOPO_ERR_INVALID, "null argument");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    *count = 0;
    if (tiles_.empty()) return TOPO_OK;
    if (int rc = ensure(stream_, query_.d_summit_count, 16)) return rc;
    uint32_t room = std::max(capacity, 1u << 16), found = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (int rc = ensure(stream_, query_.d_summit_out, (size_t)room * sizeof(SummitRec))) return rc;
        if (int rc = summits_launch(*params, query_.d_summit_out.as<SummitRec>(), room, query_.d_summit_count.as<uint32_t>())) return rc;
        TOPO_HIP_TRY(hipStreamSynchronize(stream_));
        TOPO_HIP_TRY(hipMemcpy(&found, query_.d_summit_count.p, sizeof found, hipMemcpyDeviceToHost));
        if (found <= room) break;
        room = found;
    }
    std::vector<topo_summit> all(found);
    if (found) TOPO_HIP_TRY(hipMemcpy(all.data(), query_.d_summit_out.p, (size_t)found * sizeof(topo_summit), hipMemcpyDeviceToHost));
    if (int rc = query_fold_check()) return rc;
    // (stable: ties stay in tile order)
    if (params->order == kSummitOrderHeight)
        std::stable_sort(all.begin(), all.end(), [](const topo_summit& a, const topo_summit& b) { return a.height_m > b.height_m; });
    else if (params->order == kSummitOrderIsolation)
        std::stable_sort(all.begin(), all.end(), [](const topo_summit& a, const topo_summit& b) {
            return a.isolation_m > b.isolation_m || (a.isolation_m == b.isolation_m && a.height_m > b.height_m);
        });
    *count = found;
    if (std::min(found, capacity)) std::memcpy(out, all.data(), (size_t)std::min(found, capacity) * sizeof(topo_summit));
    if (found > capacity) return fail(TOPO_ERR_CAPACITY, "more summits than capacity: *count says how many");
    return TOPO_OK;
}

// What the last summit call counted (summits_launch's state record): candidates after the prefilter, summits.
int TerrainRenderer::summit_counts(uint64_t out[2]) {
    if (!out) return fail(TOPO_ERR_INVALID, "null argument");
    out[0] = out[1] = 0;
    if (!query_.d_summit_scratch.p) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    uint32_t w[kSummitStateWords];
    TOPO_HIP_TRY(hipMemcpy(w, query_.d_summit_scratch.p, sizeof w, hipMemcpyDeviceToHost));
    out[0] = w[kSummitStateSeen];
    out[1] = w[kSummitStateTotal];
    return TOPO_OK;
}

static const char* snap_radius_error(double radius_m) {
    return std::isfinite(radius_m) && radius_m > 0.0 && radius_m <= kSummitMaxRadius ? nullptr : "radius_m must be finite and lie in (0, 1e6]";
}

int TerrainRenderer::summit_snap_device(uint32_t n, const double* lonlat_dev, double radius_m, topo_summit_snap* out_dev) {
    if (const char* why = snap_radius_error(radius_m)) return fail(TOPO_ERR_INVALID, why);
    if (n == 0) return TOPO_OK;
    if (!lonlat_dev || !out_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)lonlat_dev % 16 != 0 || (uintptr_t)out_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "lonlat_dev and out_dev must be 16-byte aligned");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    launch_summit_snap(ray_params(), lonlat_dev, radius_m, (SummitSnapRec*)out_dev, n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read: nothing is staged (as topo_visibility_read): blocking copies around the kernel.
int TerrainRenderer::summit_snap_read(uint32_t n, const double* lonlat_deg, double radius_m, topo_summit_snap* out) {
    if (const char* why = snap_radius_error(radius_m)) return fail(TOPO_ERR_INVALID, why);
    if (n == 0) return TOPO_OK;
    if (!lonlat_deg || !out) return fail(TOPO_ERR_INVALID, "null argument");
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    const size_t in_bytes = (size_t)n * 2 * sizeof(double), out_bytes = (size_t)n * sizeof(SummitSnapRec);
    if (int rc = ensure(stream_, query_.d_surface_in, in_bytes)) return rc;
    if (int rc = ensure(stream_, query_.d_summit_out, out_bytes)) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(query_.d_surface_in.p, lonlat_deg, in_bytes, hipMemcpyHostToDevice));
    launch_summit_snap(ray_params(), query_.d_surface_in.as<const double>(), radius_m, query_.d_summit_out.as<SummitSnapRec>(), n, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(out, query_.d_summit_out.p, out_bytes, hipMemcpyDeviceToHost));
    return query_fold_check();
}

// ---- sun exposure ---------------------------------------------------------------------------------------------------------------

// What every sun exposure call does first: its checks of the suns, the tables, and the suns -- host memory -- normalised as
// sunlit_map_device normalises its one and copied into the context's table on stream_ (behind the kernels of an earlier call that still
// read it).  Null lonlat and outputs are the callers' to refuse.
int TerrainRenderer::sun_begin(uint32_t n_suns, const topo_sun* suns) {
    if (!suns) return fail(TOPO_ERR_INVALID, "null argument");
    if (n_suns > kSunMaxSuns) return fail(TOPO_ERR_INVALID, "at most 64 suns");
    SunDir unit[kSunMaxSuns];
    for (uint32_t k = 0; k < n_suns; ++k) {
        const double* const d = suns[k].dir;
        const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(len > 0.0) || !std::isfinite(len)) return fail(TOPO_ERR_INVALID, "a sun's dir must be finite and non-zero");
        if (!(std::isfinite(suns[k].weight) && suns[k].weight >= 0.0)) return fail(TOPO_ERR_INVALID, "a sun's weight must be finite and not negative");
        unit[k] = SunDir{{d[0] / len, d[1] / len, d[2] / len}, suns[k].weight};
    }
    if (int rc = bind_device()) return rc;
    if (int rc = prepare_tables(kGeometryTables, stream_)) return rc;
    if (int rc = ensure(stream_, query_.d_suns, kSunMaxSuns * sizeof(SunDir))) return rc;
    TOPO_HIP_TRY(hipMemcpyAsync(query_.d_suns.p, unit, (size_t)n_suns * sizeof(SunDir), hipMemcpyHostToDevice, stream_));      // (pageable: read before it returns)
    return TOPO_OK;
}

// What is wrong with a sun exposure call's outputs (device or host: three nullable pointers), or null.
static const char* sun_outputs_error(const uint64_t* lit, const uint64_t* shadow, const float* exposure) {
    if (!lit && !shadow && !exposure) return "at least one output must be given";
    if ((uintptr_t)lit % 8 != 0 || (uintptr_t)shadow % 8 != 0) return "the masks must be 8-byte aligned";
    if ((uintptr_t)exposure % 4 != 0) return "the exposure must be 4-byte aligned";
    return nullptr;
}

// Device variants: queued on stream_, in order.
int TerrainRenderer::sun_exposure_grid_device(uint32_t n_suns, const topo_sun* suns, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny,
                                              uint64_t* lit_dev, uint64_t* shadow_dev, float* exposure_dev, size_t mask_pitch_bytes, size_t exposure_pitch_bytes) {
    if (n_suns == 0) return TOPO_OK;
    if (const char* why = sun_outputs_error(lit_dev, shadow_dev, exposure_dev)) return fail(TOPO_ERR_INVALID, why);
    if (nx == 0 || ny == 0) return fail(TOPO_ERR_INVALID, "an empty grid");
    if (!std::isfinite(lon0) || !std::isfinite(lat0) || !std::isfinite(dlon) || !std::isfinite(dlat)) return fail(TOPO_ERR_INVALID, "grid parameters must be finite");
    if (lit_dev || shadow_dev) {
        if (mask_pitch_bytes % 8 != 0) return fail(TOPO_ERR_INVALID, "the mask pitch must be a multiple of 8 bytes");
        if (mask_pitch_bytes / sizeof(uint64_t) < nx) return fail(TOPO_ERR_INVALID, "mask pitch smaller than a row");
    }
    if (exposure_dev) {
        if (exposure_pitch_bytes % 4 != 0) return fail(TOPO_ERR_INVALID, "the exposure pitch must be a multiple of 4 bytes");
        if (exposure_pitch_bytes / sizeof(float) < nx) return fail(TOPO_ERR_INVALID, "exposure pitch smaller than a row");
    }
    if ((((uint64_t)nx + 63) / 64) * ny > 0xFFFFFFFFull) return fail(TOPO_ERR_INVALID, "grid too large");
    if (int rc = sun_begin(n_suns, suns)) return rc;
    launch_sun_exposure_grid(ray_params(), query_.d_suns.as<const SunDir>(), n_suns, lon0, lat0, dlon, dlat, nx, ny, lit_dev, shadow_dev, exposure_dev, mask_pitch_bytes,
                             exposure_pitch_bytes, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

int TerrainRenderer::sun_exposure_device(uint32_t n_suns, const topo_sun* suns, uint32_t n, const double* lonlat_dev, uint64_t* lit_dev, uint64_t* shadow_dev,
                                         float* exposure_dev) {
    if (n == 0 || n_suns == 0) return TOPO_OK;
    if (!lonlat_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)lonlat_dev % 16 != 0) return fail(TOPO_ERR_INVALID, "lonlat_dev must be 16-byte aligned");
    if (const char* why = sun_outputs_error(lit_dev, shadow_dev, exposure_dev)) return fail(TOPO_ERR_INVALID, why);
    if (int rc = sun_begin(n_suns, suns)) return rc;
    launch_sun_exposure_list(ray_params(), query_.d_suns.as<const SunDir>(), n_suns, lonlat_dev, n, lit_dev, shadow_dev, exposure_dev, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read.  The caller's memory is pageable, so nothing is staged (as topo_visibility_read): the stream is drained, the list goes up
// and the outputs that were asked for come down with blocking copies.
int TerrainRenderer::sun_exposure_read(uint32_t n_suns, const topo_sun* suns, uint32_t n, const double* lonlat_deg, uint64_t* lit, uint64_t* shadow, float* exposure) {
    if (n == 0 || n_suns == 0) return TOPO_OK;
    if (!lonlat_deg) return fail(TOPO_ERR_INVALID, "null argument");
    if (const char* why = sun_outputs_error(lit, shadow, exposure)) return fail(TOPO_ERR_INVALID, why);
    if (int rc = sun_begin(n_suns, suns)) return rc;
    const size_t in_bytes = (size_t)n * 2 * sizeof(double), mask_bytes = (size_t)n * sizeof(uint64_t), exp_bytes = (size_t)n * sizeof(float);
    if (int rc = ensure(stream_, query_.d_surface_in, in_bytes)) return rc;
    if (lit)
        if (int rc = ensure(stream_, query_.d_sun_lit, mask_bytes)) return rc;
    if (shadow)
        if (int rc = ensure(stream_, query_.d_sun_shadow, mask_bytes)) return rc;
    if (exposure)
        if (int rc = ensure(stream_, query_.d_sun_exposure, exp_bytes)) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(query_.d_surface_in.p, lonlat_deg, in_bytes, hipMemcpyHostToDevice));
    launch_sun_exposure_list(ray_params(), query_.d_suns.as<const SunDir>(), n_suns, query_.d_surface_in.as<const double>(), n,
                             lit ? query_.d_sun_lit.as<uint64_t>() : nullptr, shadow ? query_.d_sun_shadow.as<uint64_t>() : nullptr,
                             exposure ? query_.d_sun_exposure.as<float>() : nullptr, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    if (lit) TOPO_HIP_TRY(hipMemcpy(lit, query_.d_sun_lit.p, mask_bytes, hipMemcpyDeviceToHost));
    if (shadow) TOPO_HIP_TRY(hipMemcpy(shadow, query_.d_sun_shadow.p, mask_bytes, hipMemcpyDeviceToHost));
    if (exposure) TOPO_HIP_TRY(hipMemcpy(exposure, query_.d_sun_exposure.p, exp_bytes, hipMemcpyDeviceToHost));
    return query_fold_check();
}

// ---- peak labels ------------------------------------------------------------------------------------------------------------------

// What both label calls refuse (null outputs are the callers' to refuse), before anything is queued.
int TerrainRenderer::labels_check(const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t w, uint32_t h, const float* depth_dev,
                                  size_t depth_view_stride, size_t depth_pitch) {
    if (!params || !depth_dev || (n_views && !views)) return fail(TOPO_ERR_INVALID, "null argument");
    if (params->views_per_image == 0) return fail(TOPO_ERR_INVALID, "views_per_image must not be 0");
    if (params->max_rows == 0) return fail(TOPO_ERR_INVALID, "max_rows must not be 0");
    if (n_views % params->views_per_image != 0) return fail(TOPO_ERR_INVALID, "n_views must be a multiple of views_per_image");
    if (w == 0 || h == 0) return fail(TOPO_ERR_INVALID, "view size must be non-zero");
    if ((uintptr_t)depth_dev % 4 != 0 || depth_pitch % 4 != 0 || depth_view_stride % 4 != 0)
        return fail(TOPO_ERR_INVALID, "depth pointer, pitch and view stride must be multiples of 4 bytes");
    if (const char* why = view_image_error(n_views, w, h, 4, depth_view_stride, depth_pitch)) return fail(TOPO_ERR_INVALID, why);
    int code;
    if (const char* why = label_grid_error((uint64_t)params->views_per_image * w, params->max_rows, &code)) return fail(code, why);
    return TOPO_OK;
}

// Queued on stream_, in order, like topo_visible_peaks_device: the depth is the caller's, whatever wrote it.  The views' matrices go
// into the context's device table on stream_ (behind the kernels of an earlier call that still read it) only when they differ from
// the last call's; their host copy is the key.
int TerrainRenderer::labels_device(const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t w, uint32_t h, const float* depth_dev,
                                   size_t depth_view_stride, size_t depth_pitch, uint32_t n_peaks, const float* peaks_dev, const float* widths_dev, topo_label* labels_dev,
                                   uint32_t* counts_dev, uint8_t* state_dev) {
    if (int rc = labels_check(params, n_views, views, w, h, depth_dev, depth_view_stride, depth_pitch)) return rc;
    if (!counts_dev || (params->cap && !labels_dev) || (n_peaks && (!peaks_dev || !widths_dev))) return fail(TOPO_ERR_INVALID, "null argument");
    if ((uintptr_t)peaks_dev % 4 != 0 || (uintptr_t)widths_dev % 4 != 0 || (uintptr_t)labels_dev % 4 != 0 || (uintptr_t)counts_dev % 4 != 0)
        return fail(TOPO_ERR_INVALID, "peaks, widths, labels and counts must be 4-byte aligned");
    if (n_views == 0) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    const size_t n_floats = (size_t)n_views * 16;
    const bool same = query_.d_label_projs.p && query_.label_projs.size() == n_floats &&
                      [&] {
                          for (uint32_t v = 0; v < n_views; ++v)
                              if (memcmp(&query_.label_projs[16 * (size_t)v], views[v].camera_proj, 16 * sizeof(float)) != 0) return false;
                          return true;
                      }();
    if (!same) {
        query_.label_projs.clear();      // (a failure below leaves no key behind)
        if (int rc = ensure(stream_, query_.d_label_projs, n_floats * sizeof(float))) return rc;
        std::vector<float> projs(n_floats);
        for (uint32_t v = 0; v < n_views; ++v) memcpy(&projs[16 * (size_t)v], views[v].camera_proj, 16 * sizeof(float));
        TOPO_HIP_TRY(hipMemcpyAsync(query_.d_label_projs.p, projs.data(), n_floats * sizeof(float), hipMemcpyHostToDevice, stream_));      // (pageable: read before it returns)
        query_.label_projs = std::move(projs);
    }
    if (int rc = ensure_query_check(stream_)) return rc;
    LabelParams p{};
    p.projs = query_.d_label_projs.as<const float>();
    p.depth = reinterpret_cast<const uint8_t*>(depth_dev);
    p.depth_view_stride = depth_view_stride;
    p.depth_pitch = depth_pitch;
    p.peaks = peaks_dev;
    p.widths = widths_dev;
    p.labels = reinterpret_cast<LabelRec*>(labels_dev);
    p.counts = counts_dev;
    p.state = state_dev;
    p.check = query_.d_check.as<uint32_t>();
    p.n_views = n_views;
    p.n_images = n_views / params->views_per_image;
    p.views_per_image = params->views_per_image;
    p.width = w;
    p.height = h;
    p.n_peaks = n_peaks;
    p.max_rows = params->max_rows;
    p.cap = params->cap;
    p.row_height = params->row_height;
    launch_labels(p, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Host read.  The caller's memory is pageable, so nothing is staged (as topo_sun_exposure_read): the stream is drained, the peaks and
// widths go up and the outputs come down with blocking copies.
int TerrainRenderer::labels_read(const topo_label_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t w, uint32_t h, const float* depth_dev,
                                 size_t depth_view_stride, size_t depth_pitch, uint32_t n_peaks, const float* peaks, const float* widths, topo_label* labels, uint32_t* counts,
                                 uint8_t* state) {
    if (int rc = labels_check(params, n_views, views, w, h, depth_dev, depth_view_stride, depth_pitch)) return rc;
    if (!counts || (params->cap && !labels) || (n_peaks && (!peaks || !widths))) return fail(TOPO_ERR_INVALID, "null argument");
    if (n_views == 0) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    const size_t n_images = n_views / params->views_per_image;
    const size_t peak_bytes = (size_t)n_peaks * 12, width_bytes = (size_t)n_peaks * 4, label_bytes = n_images * params->cap * sizeof(topo_label),
                 count_bytes = n_images * sizeof(uint32_t), state_bytes = state ? n_images * n_peaks : 0;
    if (int rc = ensure(stream_, query_.d_label_in, peak_bytes + width_bytes + 16)) return rc;
    if (int rc = ensure(stream_, query_.d_label_out, label_bytes + count_bytes + state_bytes + 16)) return rc;
    uint8_t* const in = query_.d_label_in.as<uint8_t>();
    uint8_t* const out = query_.d_label_out.as<uint8_t>();
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    if (n_peaks) {
        TOPO_HIP_TRY(hipMemcpy(in, peaks, peak_bytes, hipMemcpyHostToDevice));
        TOPO_HIP_TRY(hipMemcpy(in + peak_bytes, widths, width_bytes, hipMemcpyHostToDevice));
    }
    if (int rc = labels_device(params, n_views, views, w, h, depth_dev, depth_view_stride, depth_pitch, n_peaks, reinterpret_cast<const float*>(in),
                               reinterpret_cast<const float*>(in + peak_bytes), reinterpret_cast<topo_label*>(out), reinterpret_cast<uint32_t*>(out + label_bytes),
                               state ? out + label_bytes + count_bytes : nullptr))
        return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(counts, out + label_bytes, count_bytes, hipMemcpyDeviceToHost));
    // only what the kernel wrote comes down: the first min(count, cap) records of each image
    if (label_bytes) {
        std::vector<topo_label> got(n_images * params->cap);
        TOPO_HIP_TRY(hipMemcpy(got.data(), out, label_bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_images; ++i) {
            const size_t n = counts[i] < params->cap ? counts[i] : params->cap;
            if (n) memcpy(labels + i * params->cap, &got[i * params->cap], n * sizeof(topo_label));
        }
    }
    if (state_bytes) TOPO_HIP_TRY(hipMemcpy(state, out + label_bytes + count_bytes, state_bytes, hipMemcpyDeviceToHost));
    return query_fold_check();
}

// ---- unwrap -------------------------------------------------------------------------------------------------------------------

// Queued on stream_, in order, like topo_visible_peaks_device: the sources are the caller's, whatever wrote them.  The tables are
// rebuilt (host, f64) and uploaded only when the parameters, the views' matrices or the eye differ from the last call's.
int TerrainRenderer::unwrap_device(const topo_unwrap_params* params, uint32_t n_views, const topo_uniforms* views, uint32_t src_w, uint32_t src_h,
                                   const OutputParams& src, const OutputParams& out, int32_t* src_out_dev, size_t src_out_pitch) {
    if (const char* why = unwrap_params_error(params)) return fail(TOPO_ERR_INVALID, why);
    if (const char* why = unwrap_views_error(n_views, views, src_w, src_h)) return fail(TOPO_ERR_INVALID, why);
    if (!out.rgba && !out.depth && !src_out_dev) return fail(TOPO_ERR_INVALID, "at least one output must be given");
    if ((out.rgba && !src.rgba) || (out.depth && !src.depth)) return fail(TOPO_ERR_INVALID, "an output needs its source");
    const size_t row = (size_t)params->out_w * 4;
    auto bad_out = [&](const void* p, size_t pitch) { return p && ((uintptr_t)p % 16 != 0 || pitch % 16 != 0 || pitch < row); };
    if (bad_out(out.rgba, out.rgba_pitch) || bad_out(out.depth, out.depth_pitch) || bad_out(src_out_dev, src_out_pitch))
        return fail(TOPO_ERR_INVALID, "output pointers and pitches must be multiples of 16 bytes, a pitch at least a row");
    auto bad_src = [&](const void* p, size_t stride, size_t pitch) {
        return p && ((uintptr_t)p % 4 != 0 || pitch % 4 != 0 || stride % 4 != 0 || view_image_error(n_views, src_w, src_h, 4, stride, pitch));
    };
    if ((out.rgba && bad_src(src.rgba, src.rgba_view_stride, src.rgba_pitch)) || (out.depth && bad_src(src.depth, src.depth_view_stride, src.depth_pitch)))
        return fail(TOPO_ERR_INVALID, "source pointers, pitches and view strides must be multiples of 4 bytes, a pitch at least a row, a stride at least a view");
    if (src_out_dev && (uint64_t)n_views * src_h * src_w >= (1ull << 31)) return fail(TOPO_ERR_INVALID, "the source map needs n_views * src_h * src_w < 2^31");
    if ((((uint64_t)params->out_w + 255) / 256) * (((uint64_t)params->out_h + 3) / 4) > 0x7FFFFFFFull) return fail(TOPO_ERR_INVALID, "output too large");
    if (int rc = bind_device()) return rc;

    std::vector<uint8_t> key(sizeof *params + sizeof(uint32_t) + 3 * sizeof(float) + (size_t)n_views * 16 * sizeof(float));
    uint8_t* k = key.data();
    memcpy(k, params, sizeof *params); k += sizeof *params;
    memcpy(k, &n_views, sizeof n_views); k += sizeof n_views;
    memcpy(k, views[0].camera_pos, 3 * sizeof(float)); k += 3 * sizeof(float);
    for (uint32_t v = 0; v < n_views; ++v, k += 16 * sizeof(float)) memcpy(k, views[v].camera_proj, 16 * sizeof(float));
    const size_t tab_bytes = unwrap_table_doubles(n_views, params->out_w, params->out_h) * sizeof(double);
    if (key != query_.unwrap_key || !query_.d_unwrap_tab.p) {
        // an earlier unwrap may still read the old tables, an earlier upload the old host copy: both are on stream_
        TOPO_HIP_TRY(hipStreamSynchronize(stream_));
        query_.unwrap_key.clear();
        unwrap_tables(params, n_views, views, query_.unwrap_tab);
        if (int rc = ensure(stream_, query_.d_unwrap_tab, tab_bytes)) return rc;
        TOPO_HIP_TRY(hipMemcpyAsync(query_.d_unwrap_tab.p, query_.unwrap_tab.data(), tab_bytes, hipMemcpyHostToDevice, stream_));
        query_.unwrap_key = std::move(key);
    }
    if (int rc = ensure_query_check(stream_)) return rc;
    UnwrapParams p{};
    p.tab = query_.d_unwrap_tab.as<const double>();
    p.rgba_src = out.rgba ? src.rgba : nullptr;
    p.rgba_view_stride = src.rgba_view_stride;
    p.rgba_pitch = src.rgba_pitch;
    p.depth_src = out.depth ? reinterpret_cast<const uint8_t*>(src.depth) : nullptr;
    p.depth_view_stride = src.depth_view_stride;
    p.depth_pitch = src.depth_pitch;
    p.rgba_out = out.rgba;
    p.rgba_out_pitch = out.rgba_pitch;
    p.depth_out = reinterpret_cast<uint8_t*>(out.depth);
    p.depth_out_pitch = out.depth_pitch;
    p.src_out = reinterpret_cast<uint8_t*>(src_out_dev);
    p.src_out_pitch = src_out_pitch;
    p.check = query_.d_check.as<uint32_t>();
    p.n_views = n_views;
    p.src_w = src_w;
    p.src_h = src_h;
    p.out_w = params->out_w;
    p.out_h = params->out_h;
    p.srgb = format_ == TOPO_FORMAT_RGBA8_UNORM_SRGB || format_ == TOPO_FORMAT_BGRA8_UNORM_SRGB;
    launch_unwrap(p, params->filter == TOPO_UNWRAP_BILINEAR, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

}  // namespace topo
