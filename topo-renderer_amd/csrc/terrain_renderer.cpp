// terrain_renderer.cpp -- host orchestration of the HIP terrain path (see terrain_renderer.hpp).
#include "terrain_renderer.hpp"

#include "geotiff.hpp"

#include <algorithm>
#include <atomic>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace topo {

namespace {

// The experiment switches of the submission path (tools/README.md, in its table's order), read once per process.
struct Switches {
    static int env(const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; }
    const bool views_by_copy = env("TOPO_VIEWS_BY_COPY", 0) != 0;
    const bool views_in_cull = env("TOPO_VIEWS_IN_CULL", 1) != 0;
    const bool status_by_copy = env("TOPO_STATUS_BY_COPY", 0) != 0;
    const bool far_skip = env("TOPO_FAR_SKIP", 1) != 0;
    const bool events_by_marker = env("TOPO_EVENTS_BY_MARKER", 0) != 0;
    const bool fuse_clear_cull = env("TOPO_FUSE_CLEAR_CULL", 1) != 0;
    const bool tile_prefilter = env("TOPO_TILE_PREFILTER", 1) != 0;
    const int near_strip = env("TOPO_NEAR_STRIP", 0);      // 1..15; anything else: the default
    const int cover = env("TOPO_COVER", -1);      // 0: off, 1: on for every submission; unset: on for the large ones (kCoverMinPixels)
    const bool resolve_owned = env("TOPO_RESOLVE_OWNED", 1) != 0;      // the claimed regions' strip records (CoverParams::recs): follows the cover path; 0: off
};
const Switches& switches() { static const Switches s; return s; }

bool is_linear(uint32_t format) { return format == TOPO_FORMAT_RGBA8_UNORM || format == TOPO_FORMAT_BGRA8_UNORM; }
bool is_bgra(uint32_t format) { return format == TOPO_FORMAT_BGRA8_UNORM_SRGB || format == TOPO_FORMAT_BGRA8_UNORM; }

// Timing slot [0]..[5] of topo_get_timings / topo_set_timing_slots -> the stages whose durations it adds up: what queue_frame records
// events by and frame_durations sums by.  A stage needs the two events around it; the total, the frame's first and last.
constexpr int kTimingSlots = 6;
constexpr uint32_t kStagesOfSlot[kTimingSlots] = {1u << kStClear, 1u << kStCull, (1u << kStRasterNear) | (1u << kStRasterFar), 1u << kStOcclusion,
                                                  (1u << kStRareBigNear) | (1u << kStRareBigFar), 1u << kStResolve};
constexpr uint32_t stage_events(int stage) { return 3u << stage; }
constexpr uint32_t kLastEvent = 1u << kNumStages, kTotalEvents = 1u | kLastEvent;

}  // namespace

int TerrainRenderer::fail(int code, const std::string& msg) {
    err_ = msg;
    return code;
}

int TerrainRenderer::hip_fail(hipError_t e, const char* what) {
    err_ = std::string(what) + ": " + hipGetErrorString(e);
    return TOPO_ERR_HIP;
}

int TerrainRenderer::bind_device() {
    TOPO_HIP_TRY(hipSetDevice(device_));
    return TOPO_OK;
}

// TerrainRenderer::new (terrain_renderer.rs:37-69): targets are allocated lazily at the first render.
int TerrainRenderer::create(TerrainRenderer** out, int device, uint32_t w, uint32_t h, uint32_t format, std::string* err) {
    *out = nullptr;
    if (w == 0 || h == 0) { *err = "target size must be non-zero"; return TOPO_ERR_INVALID; }
    if (format < TOPO_FORMAT_RGBA8_UNORM_SRGB || format > TOPO_FORMAT_BGRA8_UNORM) {
        *err = "colour format must be Rgba8UnormSrgb, Bgra8UnormSrgb, Rgba8Unorm or Bgra8Unorm";
        return TOPO_ERR_UNSUPPORTED;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        *err = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
               " (this library has no CPU fallback)";
        return TOPO_ERR_HIP;
    }
    if (device < 0 || device >= count) { *err = "hip_device out of range"; return TOPO_ERR_INVALID; }
    TerrainRenderer* r = new TerrainRenderer();
    r->device_ = device;
    r->W_ = w;
    r->H_ = h;
    r->format_ = format;
    if (r->init() != TOPO_OK) {
        *err = "HIP initialisation failed: " + r->err_;
        delete r;
        return TOPO_ERR_HIP;
    }
    *out = r;
    return TOPO_OK;
}

int TerrainRenderer::init() {
    TOPO_HIP_TRY(hipSetDevice(device_));
    TOPO_HIP_TRY(hipStreamCreate(&own_stream_.h));
    stream_ = own_stream_;
    tile_prefilter_ = switches().tile_prefilter;
    for (auto& e : load_ev_) TOPO_HIP_TRY(hipEventCreate(&e.h));
    return init_ctx(ctx_[0], false);
}

TerrainRenderer::~TerrainRenderer() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (auto& c : ctx_)
        if (c.stream) (void)hipStreamSynchronize(c.stream);
    // (the members go now -- tiles, buffers, pinned memory, registrations, events, streams: the device is bound and every stream
    // has been waited for)
}

int TerrainRenderer::ensure(hipStream_t s, DeviceBuffer& b, size_t need) {
    if (need <= b.cap) return TOPO_OK;
    if (b.p) {
        TOPO_HIP_TRY(hipStreamSynchronize(s));
        TOPO_HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    TOPO_HIP_TRY(hipMalloc(&b.p, need));
    b.cap = need;
    return TOPO_OK;
}

int TerrainRenderer::ensure_pinned(PinnedBuffer& b, size_t need) {
    if (need <= b.cap) return TOPO_OK;
    b.reset();
    TOPO_HIP_TRY(hipHostMalloc(&b.p, need));
    b.cap = need;
    return TOPO_OK;
}

int TerrainRenderer::wait_all() {
    if (int rc = join()) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    return TOPO_OK;
}

Tile* TerrainRenderer::find(int lat, int lon) {
    auto it = tiles_.find(geo_key(lat, lon));
    return it == tiles_.end() ? nullptr : &it->second;
}

// The compute-pass orchestration of add_terrain (terrain_renderer.rs:192-347) for tile `nt`: a seam pass for each
// loaded edge neighbour and a corner pass for each complete 2x2 block, every one of them fed the NEW tile's
// uniforms (:275, :344).  "Loaded" = inserted before `nt` (all other tiles, except while replaying).  Jobs name
// tiles by rank (their index in the device tile table).
void TerrainRenderer::collect_jobs(const Tile& nt, const std::map<GeoKey, uint32_t>& rank, std::vector<EdgeJob>& edges,
                                   std::vector<CornerJob>& corners) {
    const int lat = nt.lat, lon = nt.lon;
    const uint32_t NONE = 0xFFFFFFFFu;
    auto loaded = [&](int la, int lo) -> uint32_t {
        Tile* t = find(la, lo);
        return (t && t != &nt && t->seq < nt.seq) ? rank.at(geo_key(la, lo)) : NONE;
    };
    const uint32_t me = rank.at(geo_key(lat, lon));
    const uint32_t left = loaded(lat, lon - 1), right = loaded(lat, lon + 1);
    const uint32_t top = loaded(lat + 1, lon), bottom = loaded(lat - 1, lon);
    const uint32_t top_left = loaded(lat + 1, lon - 1), top_right = loaded(lat + 1, lon + 1);
    const uint32_t bottom_left = loaded(lat - 1, lon - 1), bottom_right = loaded(lat - 1, lon + 1);
    if (left != NONE) edges.push_back(EdgeJob{left, me, me, 0});
    if (right != NONE) edges.push_back(EdgeJob{me, right, me, 0});
    if (top != NONE) edges.push_back(EdgeJob{top, me, me, 1});
    if (bottom != NONE) edges.push_back(EdgeJob{me, bottom, me, 1});
    if (top_left != NONE && top != NONE && left != NONE) corners.push_back(CornerJob{top_left, top, left, me, me});
    if (top != NONE && top_right != NONE && right != NONE) corners.push_back(CornerJob{top, top_right, me, right, me});
    if (left != NONE && bottom_left != NONE && bottom != NONE) corners.push_back(CornerJob{left, me, bottom_left, bottom, me});
    if (right != NONE && bottom != NONE && bottom_right != NONE) corners.push_back(CornerJob{me, right, bottom, bottom_right, me});
}

// Uploads the job lists and launches the seam and corner passes (each writes a disjoint set of texels, so one
// launch per kind covers any number of jobs).
int TerrainRenderer::upload_seam_jobs(const std::vector<EdgeJob>& edges, const std::vector<CornerJob>& corners) {
    if (!edges.empty()) {
        if (int rc = ensure(stream_, d_edge_jobs_, edges.size() * sizeof(EdgeJob))) return rc;
        TOPO_HIP_TRY(hipMemcpyAsync(d_edge_jobs_.p, edges.data(), edges.size() * sizeof(EdgeJob), hipMemcpyHostToDevice, stream_));
    }
    if (!corners.empty()) {
        if (int rc = ensure(stream_, d_corner_jobs_, corners.size() * sizeof(CornerJob))) return rc;
        TOPO_HIP_TRY(hipMemcpyAsync(d_corner_jobs_.p, corners.data(), corners.size() * sizeof(CornerJob), hipMemcpyHostToDevice, stream_));
    }
    // the job vectors are pageable host memory: hipMemcpyAsync has staged them before returning
    return TOPO_OK;
}
void TerrainRenderer::launch_seam_jobs(size_t n_edges, size_t n_corners) {
    launch_normals_border(d_tiles_.as<const TileDev>(), d_edge_jobs_.as<const EdgeJob>(), (uint32_t)n_edges, d_corner_jobs_.as<const CornerJob>(), (uint32_t)n_corners,
                          tile_w_, tile_h_, stream_);
}
int TerrainRenderer::run_seam_jobs(const std::vector<EdgeJob>& edges, const std::vector<CornerJob>& corners) {
    if (int rc = upload_seam_jobs(edges, corners)) return rc;
    launch_seam_jobs(edges.size(), corners.size());
    return TOPO_OK;
}

std::map<GeoKey, uint32_t> TerrainRenderer::ranks() const {
    std::map<GeoKey, uint32_t> r;
    uint32_t i = 0;
    for (const auto& kv : tiles_) r[kv.first] = i++;
    return r;
}

int TerrainRenderer::add_terrain(int32_t lat, int32_t lon, const float* heights, bool on_device, uint32_t w, uint32_t h,
                                 const float rp[2], const float mp[2], const float ps[2]) {
    if (!heights || !rp || !mp || !ps) return fail(TOPO_ERR_INVALID, "null argument");
    if (w < 3 || h < 3) return fail(TOPO_ERR_INVALID, "tile must be at least 3x3");
    if (w > 32768 || h > 32768) return fail(TOPO_ERR_INVALID, "tile too large");
    if (!tiles_.empty() && (w != tile_w_ || h != tile_h_))
        return fail(TOPO_ERR_INVALID, "mixed tile sizes are rejected (the reference caches one mesh: render_buffer.rs:12-15)");
    if (int rc = join()) return rc;
    const uint64_t tris = 2ull * (w - 1) * (h - 1);
    const size_t n_after = tiles_.size() + (find(lat, lon) ? 0 : 1);
    if (tris * n_after >= (1ull << 31) || n_after > 0xFFFFu) return fail(TOPO_ERR_CAPACITY, "draw-order id space exhausted");
    tile_w_ = w;
    tile_h_ = h;
    const size_t texels = (size_t)w * h;
    const uint32_t bxc = (w - 1 + kBCX - 1) / kBCX, byc = (h - 1 + kBCY - 1) / kBCY;
    Tile t;
    t.lat = lat;
    t.lon = lon;
    t.seq = next_seq_++;
    // ONE allocation per tile: heights, normals, then block min/max (2 floats per block), the sin/cos tables of the w columns
    // and the h rows, and the f64 cull bounds (sphere 4 + corners 12 + sagitta 1 + sideways bulge 1 doubles per block); every part 256-byte aligned
    const size_t tile_floats = (size_t)bxc * byc * 2 + 2 * ((size_t)w + h);
    auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t off_normals = up256(texels * 4), off_tables = off_normals + up256(texels * 4), off_bounds = off_tables + up256(tile_floats * sizeof(float));
    if (int rc = ensure(stream_, t.pool, off_bounds + (size_t)bxc * byc * 18 * sizeof(double))) return rc;
    t.d_heights = t.pool.as<float>();
    t.d_normals = reinterpret_cast<uint32_t*>(t.pool.as<uint8_t>() + off_normals);
    t.d_minmax = reinterpret_cast<float*>(t.pool.as<uint8_t>() + off_tables);
    // (the zero-initialised normal texture: k_normals_interior writes the untouched border ring as zero)
    if (const hipError_t e = hipMemcpyAsync(t.d_heights, heights, texels * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_))
        return hip_fail(e, "tile upload");
    if (vs_ever_)      // (a replaced tile's mask goes with it: the new one starts empty)
        if (int rc = alloc_mask(t)) return rc;
    // TerrainUniforms::new (render/data.rs:124-151)
    t.dev.heights = t.d_heights;
    t.dev.normals = t.d_normals;
    t.dev.block_minmax = t.d_minmax;
    t.dev.trig_lon = t.d_minmax + (size_t)bxc * byc * 2;
    t.dev.trig_lat = t.dev.trig_lon + 2 * (size_t)w;
    t.dev.block_bounds = reinterpret_cast<const double*>(t.pool.as<uint8_t>() + off_bounds);
    t.dev.raster_x = rp[0]; t.dev.raster_y = rp[1];
    t.dev.model_x = mp[0]; t.dev.model_y = mp[1];
    t.dev.scale_x = ps[0]; t.dev.scale_y = ps[1];
    terrain_rotation(mp[0], mp[1], t.dev.rot);
    // BTreeMap::insert replaces an existing entry; its GPU resources are dropped when this call returns, on whichever path, once
    // stream_ has been waited for (where that wait itself fails, hipFree waits for the device)
    struct Retired {
        Tile tile;
        hipStream_t stream;
        ~Retired() { if (tile.pool.p) (void)hipStreamSynchronize(stream); }
    } old{Tile{}, stream_};
    if (Tile* ex = find(lat, lon)) { old.tile = std::move(*ex); tiles_.erase(geo_key(lat, lon)); }
    Tile& nt = tiles_[geo_key(lat, lon)] = std::move(t);
    table_dirty_ = true;
    ++tile_gen_;
    if (int rc = upload_tile_table()) return rc;
    {
        const std::map<GeoKey, uint32_t> rk = ranks();
        std::vector<EdgeJob> edges;
        std::vector<CornerJob> corners;
        collect_jobs(nt, rk, edges, corners);
        launch_load_kernels(rk.at(geo_key(lat, lon)), 1, nullptr);
        if (int rc = run_seam_jobs(edges, corners)) return rc;
    }
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));   // `heights` (and the job lists) are only borrowed for the call
    {   // the sphere around the block spheres' centres (see Tile::centres); any non-finite entry leaves it unknown
        std::vector<double> sph((size_t)bxc * byc * 4);
        TOPO_HIP_TRY(hipMemcpy(sph.data(), nt.dev.block_bounds, sph.size() * sizeof(double), hipMemcpyDeviceToHost));
        double c[3] = {0.0, 0.0, 0.0}, r2 = 0.0, rmax = 0.0;
        bool finite = true;
        for (size_t i = 0; i < sph.size(); i += 4) {
            finite = finite && std::isfinite(sph[i]) && std::isfinite(sph[i + 1]) && std::isfinite(sph[i + 2]) && std::isfinite(sph[i + 3]);
            for (int k = 0; k < 3; ++k) c[k] += sph[i + k];
            rmax = std::max(rmax, sph[i + 3]);
        }
        for (int k = 0; k < 3; ++k) c[k] /= (double)(sph.size() / 4);
        for (size_t i = 0; i < sph.size() && finite; i += 4) {
            const double dx = sph[i] - c[0], dy = sph[i + 1] - c[1], dz = sph[i + 2] - c[2];
            r2 = std::max(r2, dx * dx + dy * dy + dz * dz);
        }
        nt.centres[0] = c[0]; nt.centres[1] = c[1]; nt.centres[2] = c[2];
        nt.centres[3] = finite ? std::sqrt(r2) : -1.0;
        nt.block_radius = finite ? rmax : -1.0;
    }
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// Every load-time kernel of tiles [first, first + count) of the device table except the seam passes.  Two forms: the DEM read
// ONCE (k_trig_tables -> normals + block minima / maxima in one pass -> k_block_bounds; COP90 / COP30 widths) or the tables kernel
// followed by the normals kernel (any size, any LDS tile size).  `mid`: recorded between the part that precedes the normals and
// the rest (the load phase's timing bracket).
void TerrainRenderer::launch_load_kernels(uint32_t first, uint32_t count, hipEvent_t mid) {
    const TileDev* tiles = d_tiles_.as<const TileDev>();
    if (normals_tables_fused(tile_w_, tile_h_, lds_rows_)) {
        launch_trig_tables(tiles, first, count, tile_w_, tile_h_, stream_);
        if (mid) (void)hipEventRecord(mid, stream_);
        launch_normals_tables(tiles, first, count, tile_w_, tile_h_, stream_);
        launch_block_bounds(tiles, first, count, tile_w_, tile_h_, stream_);
    } else {
        launch_block_tables(tiles, first, count, tile_w_, tile_h_, stream_);
        if (mid) (void)hipEventRecord(mid, stream_);
        launch_normals_interior(tiles, first, count, tile_w_, tile_h_, lds_rows_, stream_);
    }
}

// unload_terrain (terrain_renderer.rs:361-363): neighbours keep whatever seam normals they have.
int TerrainRenderer::unload_terrain(int32_t lat, int32_t lon) {
    Tile* t = find(lat, lon);
    if (!t) return TOPO_OK;   // BTreeMap::remove of a missing key is a no-op
    if (int rc = wait_all()) return rc;
    tiles_.erase(geo_key(lat, lon));
    table_dirty_ = true;
    ++tile_gen_;
    return TOPO_OK;
}

int TerrainRenderer::recompute_normals() {
    if (int rc = join()) return rc;
    std::vector<Tile*> order;
    for (auto& kv : tiles_) order.push_back(&kv.second);
    std::sort(order.begin(), order.end(), [](Tile* a, Tile* b) { return a->seq < b->seq; });
    if (int rc = upload_tile_table()) return rc;
    const std::map<GeoKey, uint32_t> rk = ranks();
    std::vector<EdgeJob> edges;
    std::vector<CornerJob> corners;
    for (Tile* t : order) collect_jobs(*t, rk, edges, corners);
    if (int rc = ensure(stream_, d_edge_jobs_, (edges.size() + 1) * sizeof(EdgeJob))) return rc;
    if (int rc = ensure(stream_, d_corner_jobs_, (corners.size() + 1) * sizeof(CornerJob))) return rc;
    if (int rc = upload_seam_jobs(edges, corners)) return rc;      // (the job lists: host -> device, ahead of the kernels that are timed)
    // the whole load phase of the resident tiles, every load-time kernel inside the bracket: the tables of the frame phase
    // (ev 0 -> 2), then the normals K1-K3 (ev 2 -> 1)
    TOPO_HIP_TRY(hipEventRecord(load_ev_[0], stream_));
    launch_load_kernels(0, (uint32_t)order.size(), load_ev_[2]);
    launch_seam_jobs(edges.size(), corners.size());
    TOPO_HIP_TRY(hipEventRecord(load_ev_[1], stream_));
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));   // the job lists are locals
    load_timed_ = true;
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// update (terrain_renderer.rs:151-171)
int TerrainRenderer::update(uint32_t w, uint32_t h, const topo_uniforms* u, const topo_post_uniforms* pu) {
    if (!u || !pu) return fail(TOPO_ERR_INVALID, "null argument");
    if (w == 0 || h == 0) return fail(TOPO_ERR_INVALID, "target size must be non-zero");
    if (pu->pixelize_n < 99.99999f && !(pu->pixelize_n >= 1.0f)) return fail(TOPO_ERR_INVALID, "pixelize_n must be at least 1");
    if (pu->pixelize_n < 99.99999f && !(pu->viewport[0] >= 1.0f && pu->viewport[1] >= 1.0f)) return fail(TOPO_ERR_INVALID, "viewport must be at least 1 x 1");
    W_ = w;
    H_ = h;
    uniforms_ = *u;
    post_ = *pu;
    have_uniforms_ = true;
    return TOPO_OK;
}

int TerrainRenderer::upload_tile_table() {
    if (!table_dirty_) return TOPO_OK;
    std::vector<TileDev> table;
    for (auto& kv : tiles_) table.push_back(kv.second.dev);   // std::map iterates in BTreeMap order
    if (!table.empty()) {
        if (int rc = ensure(stream_, d_tiles_, table.size() * sizeof(TileDev))) return rc;
        TOPO_HIP_TRY(hipStreamSynchronize(stream_));
        TOPO_HIP_TRY(hipMemcpy(d_tiles_.p, table.data(), table.size() * sizeof(TileDev), hipMemcpyHostToDevice));
        if (vs_ever_) {      // the viewshed's rank -> mask table: ranks shift whenever tiles come and go
            std::vector<uint32_t*> masks;
            for (auto& kv : tiles_) masks.push_back(kv.second.mask.as<uint32_t>());
            if (int rc = ensure(stream_, d_vs_table_, masks.size() * sizeof(uint32_t*))) return rc;
            TOPO_HIP_TRY(hipMemcpy(d_vs_table_.p, masks.data(), masks.size() * sizeof(uint32_t*), hipMemcpyHostToDevice));
        }
    }
    table_dirty_ = false;
    return TOPO_OK;
}

int TerrainRenderer::init_ctx(FrameCtx& c, bool own_stream) {
    for (auto& f : c.timed_frames)
        for (auto& e : f.ev)
            if (!e) TOPO_HIP_TRY(hipEventCreate(&e.h));
    if (!c.done) TOPO_HIP_TRY(hipEventCreateWithFlags(&c.done.h, hipEventDisableTiming));
    if (own_stream && !c.stream) TOPO_HIP_TRY(hipStreamCreateWithFlags(&c.stream.h, hipStreamNonBlocking));
    return TOPO_OK;
}

// Frames in flight on the contexts' own streams are not ordered with stream_: everything that frees or rewrites what a
// frame reads (tiles, the tile table), and every consumer of a frame's outputs, joins them first.  A pending context's
// latest frame may also sit on stream_ (the slot-by-slot panorama at depth > 1): join waits for the stream it was queued on.
int TerrainRenderer::join() {
    if (int rc = bind_device()) return rc;
    for (auto& c : ctx_)
        if (c.pending) {
            if (c.last_stream) TOPO_HIP_TRY(hipStreamSynchronize(c.last_stream));
            c.pending = false;
        }
    return TOPO_OK;
}

// The status word of a frame is per frame (k_clear resets it, render_frame copies the counters to pinned memory behind
// k_resolve).  Called once the frames' streams have been waited for: a frame whose rare-triangle queue overflowed has
// dropped triangles -- its outputs are incomplete -- and that is an error of the call that waited for it
// (topo_join / topo_synchronize; topo_render answers for its own frame), reported once: the first of those calls after the
// frame finished returns one TOPO_ERR_CAPACITY for all the overflowed frames it waited for.
bool TerrainRenderer::fold_frames(FrameCtx& c, uint64_t end) {
    bool overflow = false;
    for (; c.checked < end; ++c.checked) {
        const uint32_t* w = c.status_words(c.checked);
        // status bits accumulate over the frames folded since the last topo_frame_status (which clears them): a burst of frames
        // cannot hide an earlier frame's overflow or bounds violation behind a clean last frame
        last_status_[0] |= w[kCtrStatus];
        if (w[kCtrStatus] & kStatusBounds) record_bounds(w);
        overflow |= (w[kCtrStatus] & kStatusRareOverflow) != 0;
    }
    return overflow;
}

// A bounds record (of a frame's counter set, or a horizon query's) into the status topo_frame_status reports.
void TerrainRenderer::record_bounds(const uint32_t* w) {
    last_status_[0] |= kStatusBounds;
    last_status_[1] = w[kCtrBoundsTag]; last_status_[2] = w[kCtrBoundsLo]; last_status_[3] = w[kCtrBoundsHi];
}

bool TerrainRenderer::fold_idle() {
    bool overflow = false;
    for (auto& c : ctx_)
        if (!c.pending && c.h_status.p) overflow |= fold_frames(c);
    return overflow;
}

// For the calls that answer for the latest frame of c themselves (topo_render, topo_horizon_read), after waiting for it.  The frames
// of c in front of it go to the next topo_join: their overflow stays pending.  Its own status bits reach topo_frame_status, and
// whether it overflowed is returned -- the caller's error, not pending, not reported again by the next topo_join.  `retry`: the
// caller throws an overflowed frame away and renders it again, so its status describes no frame anyone gets and is skipped.
bool TerrainRenderer::fold_latest(FrameCtx& c, bool retry) {
    overflow_pending_ |= fold_frames(c, c.submitted - 1);
    const bool overflow = (c.latest_status()[kCtrStatus] & kStatusRareOverflow) != 0;
    if (overflow && retry) ++c.checked;
    else (void)fold_frames(c);
    return overflow;
}

int TerrainRenderer::check_frames() {
    const bool overflow = fold_idle() | overflow_pending_;
    overflow_pending_ = false;
    if (overflow) return fail(TOPO_ERR_CAPACITY, "rare-triangle queue overflowed: a frame is incomplete (raise the queue capacity or render fewer views per submission)");
    return TOPO_OK;
}

int TerrainRenderer::set_pipeline_depth(int depth) {
    if (depth < 1 || depth > kMaxPipeline) return fail(TOPO_ERR_INVALID, "pipeline depth must be 1..4");
    if (int rc = wait_all()) return rc;
    for (int i = 0; i < depth; ++i)
        if (int rc = init_ctx(ctx_[i], depth > 1)) return rc;
    pipeline_depth_ = depth;
    next_ctx_ = last_ctx_ = 0;
    for (FrameCtx& fc : ctx_) fc.lists_valid = false;      // (read_cull_lists: "the last submission" is one made at the current depth)
    return TOPO_OK;
}

// The view count and target size every submission must keep to: the kernels store footprints and region coordinates in 16 bits
// (FarItem, BigItem) and the view index of a work item in 16 (DESIGN.md "Size limits").  Both entry points into render_frame
// (render_views_device, the slot path of render_panorama) check them before anything is queued.
static const char* submission_error(uint32_t n, uint32_t w, uint32_t h) {
    if (n > 0xFFFFu) return "too many views";
    if (w == 0 || h == 0 || w > 65536 || h > 65536) return "bad target size";
    return nullptr;
}

int TerrainRenderer::render_views_device(uint32_t n, const topo_uniforms* views, uint32_t w, uint32_t h, const OutputParams& out) {
    if (n == 0 || !views || !out.rgba) return fail(TOPO_ERR_INVALID, "null/empty argument");
    if (const char* e = submission_error(n, w, h)) return fail(TOPO_ERR_INVALID, e);
    if (int rc = bind_device()) return rc;
    if (table_dirty_)
        if (int rc = join()) return rc;
    if (int rc = upload_tile_table()) return rc;
    FrameCtx& c = ctx_[next_ctx_];
    last_ctx_ = next_ctx_;
    next_ctx_ = (next_ctx_ + 1) % pipeline_depth_;
    if (pipeline_depth_ == 1) return render_frame(c, stream_, n, views, w, h, out);
    // the tile table (and whatever else the caller queued) was produced on stream_: order the frame after it
    TOPO_HIP_TRY(hipEventRecord(c.done, stream_));
    TOPO_HIP_TRY(hipStreamWaitEvent(c.stream, c.done, 0));
    return render_frame(c, c.stream, n, views, w, h, out);
}

// Is the far phase worth its four launches (each ~4 us of GPU and ~9 us of host time)?  k_cull makes an occlusion-test
// candidate of a block whose nearest possible view depth, w(centre) - radius |w row|, exceeds the split;
// w(centre) <= w(C) + R |w row| for the sphere (C, R) around the tile's block centres (Tile::centres).  The split is a
// performance knob with a flat optimum (60..120 km at c4; results do not depend on it): when that bound stays below 4/3 of
// it for every view and tile -- a lone tile around the viewpoint -- the frame's split (*split_m) is raised above the bound, no
// block becomes a candidate and the far phase need not be launched (true).  A function of its arguments alone: no HIP, no state.
static bool far_phase_empty(const topo_uniforms* views, uint32_t n, const std::map<GeoKey, Tile>& tiles, float* split_m) {
    double bound = 0.0;
    for (uint32_t i = 0; i < n && bound >= 0.0; ++i) {
        const float* m = views[i].camera_proj;
        const double wn = std::sqrt((double)m[3] * m[3] + (double)m[7] * m[7] + (double)m[11] * m[11]);
        for (const auto& kv : tiles) {
            const double* s = kv.second.centres;
            const double w_far = (double)m[3] * s[0] + (double)m[7] * s[1] + (double)m[11] * s[2] + (double)m[15] + s[3] * wn;
            if (!(s[3] >= 0.0) || !(w_far < 1e30)) { bound = -1.0; break; }      // unknown sphere, NaN or huge: keep the far phase
            bound = std::max(bound, w_far);
        }
    }
    if (!(bound >= 0.0 && bound + 2.0 < (double)*split_m * (4.0 / 3.0))) return false;
    *split_m = std::max(*split_m, (float)(bound + 2.0));      // (>= bound + 1 after the rounding to f32: no candidates)
    return true;
}

// clear and cull in one launch: unless switched off, whenever there are tiles to cull
static bool fused_clear_cull(const FrameParams& p) { return switches().fuse_clear_cull && p.n_tiles != 0; }

int TerrainRenderer::render_frame(FrameCtx& c, hipStream_t stream, uint32_t n, const topo_uniforms* views, uint32_t w, uint32_t h,
                                  const OutputParams& out, const ResolveSlot* slots, uint32_t n_slots,
                                  const std::function<int(uint32_t, hipStream_t)>* after_slot) {
    if (n == 0) return fail(TOPO_ERR_INVALID, "null/empty argument");
    if (const char* e = submission_error(n, w, h)) return fail(TOPO_ERR_INVALID, e);
    latest_ctx_ = -1;      // (until this submission is queued whole: a failure half-way leaves nothing to query)
    c.lists_valid = false;
    FrameParams p{};
    if (int rc = grow_frame_buffers(c, stream, n, w, h, p)) return rc;
    ViewPack pack{};
    bool pack_in_cull = false;
    if (int rc = stage_views(c, stream, views, p, pack, &pack_in_cull)) return rc;
    fill_params(c, p);
    last_far_phase_ = p.split_m > 0.0f && !(switches().far_skip && far_phase_empty(views, n, tiles_, &p.split_m));
    const CullList cull = cull_pairs(views, p);
    if (int rc = queue_frame(c, stream, p, pack_in_cull ? &pack : nullptr, cull, last_far_phase_, out, slots, n_slots, after_slot)) return rc;
    record_submission(c, p, views);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

// The (view, tile) pairs the cull is launched over: those the host's prefilter keeps (host_math.hpp: tile_prefilter), when the
// prefilter is on (TOPO_TILE_PREFILTER=0, topo_debug_set_tile_prefilter: off) and their list fits the launch's argument segment;
// otherwise every pair, as the full grid (`codes` null).  The tiles' spheres are gathered once per tile set (tile_spheres).
TerrainRenderer::CullList TerrainRenderer::cull_pairs(const topo_uniforms* views, const FrameParams& p) {
    const size_t all = (size_t)p.n_views * p.n_tiles;
    last_cull_pairs_[0] = last_cull_pairs_[1] = (uint32_t)all;
    CullList list{nullptr, 0};
    if (!tile_prefilter_ || all == 0 || all > 65536) return list;
    const uint32_t kept = tile_prefilter(views, p.n_views, tile_spheres().data(), p.n_tiles, cull_codes_, kMaxCullPairs);
    if (kept > kMaxCullPairs) return list;
    last_cull_pairs_[0] = kept;
    list.codes = cull_codes_;
    list.n = kept;
    return list;
}

// Sizes the frame's queues and lists (into p) and grows the context's buffers to them; the status ring of the context.
int TerrainRenderer::grow_frame_buffers(FrameCtx& c, hipStream_t stream, uint32_t n, uint32_t w, uint32_t h, FrameParams& p) {
    p.n_views = n;
    p.n_tiles = (uint32_t)tiles_.size();
    p.W = (int32_t)w;
    p.H = (int32_t)h;
    p.bx_count = p.n_tiles ? (tile_w_ - 1 + kBCX - 1) / kBCX : 0;
    p.by_count = p.n_tiles ? (tile_h_ - 1 + kBCY - 1) / kBCY : 0;
    const size_t pixels = (size_t)n * w * h;
    const size_t work_cap = (size_t)n * p.n_tiles * p.bx_count * p.by_count;
    p.big_cap = big_cap_cfg_ ? big_cap_cfg_ : (1u << 22);
    p.rare_cap = rare_cap_cfg_ ? rare_cap_cfg_ : (rare_cap_auto_ ? (uint32_t)rare_cap_auto_ : (1u << 22));
    if (work_cap >= (1ull << 30)) return fail(TOPO_ERR_CAPACITY, "too many raster blocks in one submission");
    if (pixels >= (1ull << 32)) return fail(TOPO_ERR_CAPACITY, "more than 2^32 pixels in one submission");
    const size_t vis_keys = (pixels + 63) & ~(size_t)63;   // whole 64-key segments: k_clear rewrites segments, not keys
    if (vis_keys * 8 > c.d_vis.cap) {
        // a fresh buffer holds garbage: mark every segment so that the first k_clear initialises all of it
        if (int rc = ensure(stream, c.d_vis, vis_keys * 8)) return rc;
        if (int rc = ensure(stream, c.d_dirty, vis_keys / 64 + 64)) return rc;
        TOPO_HIP_TRY(hipMemsetAsync(c.d_dirty.p, 1, c.d_dirty.cap, stream));
    }
    if (int rc = ensure(stream_, d_views_, sizeof(ViewDev) * kMaxViewsPerSlot * kViewSlots)) return rc;
    // A near block (and a far survivor) is cut into strips of near_strip cell rows, one wave each: the raster phase is as long
    // as its longest strip, and a strip's vertex rows cost less than the pixels of its triangles.  Measured (tools/exp_strip.sh,
    // ms per frame at 1 / 2 / 4 rows): c1 0.146 / 0.148 / 0.157, c2 0.186 / 0.184 / 0.194, c3 0.382 / 0.372 / 0.390,
    // c4 0.964 / 0.933 / 0.942.  TOPO_NEAR_STRIP overrides (experiments).
    const int strip_env = switches().near_strip;
    p.near_strip = strip_env >= 1 && strip_env <= 15 ? (uint32_t)strip_env : (work_cap <= 64 * 1024 ? 1u : 2u);
    const size_t near_cap = (size_t)((kBCY + p.near_strip - 1) / p.near_strip) * work_cap;
    if (int rc = ensure(stream, c.d_work, (near_cap ? near_cap : 1) * sizeof(WorkItem))) return rc;
    if (int rc = ensure(stream, c.d_work2, (near_cap ? near_cap : 1) * sizeof(WorkItem))) return rc;   // far survivors, in strips too
    // the far-candidate list: kFarLists sub-lists, cull workgroup b (256 blocks) appending to sub-list b % kFarLists
    const size_t far_sub_cap = (cull_workgroups_max(n, p.n_tiles, p.bx_count * p.by_count) + kFarLists - 1) / kFarLists * 256;
    if (int rc = ensure(stream, c.d_far, (far_sub_cap ? far_sub_cap * kFarLists : 1) * sizeof(FarItem))) return rc;
    if (int rc = ensure(stream, c.d_big, p.big_cap * sizeof(BigItem))) return rc;
    if (int rc = ensure(stream, c.d_rare, p.rare_cap * sizeof(RareItem))) return rc;
    // covered regions (CoverParams): a 64-bit owner word per (view, 64 x 64 px region).  A fresh table is zeroed -- older than any
    // serial -- and so is the table when the context's serial wraps.
    c.cover = CoverParams{};
    // The path costs a launch over every region and the claims' arithmetic in k_raster_rare whatever the submission's size, and
    // saves in proportion to its terrain pixels: by default it is taken where it was measured to pay, above kCoverMinPixels (the
    // c4 panorama's 67 M pixels: profiles/cover_regions_ab.txt); smaller submissions keep the atomic way.
    constexpr size_t kCoverMinPixels = (size_t)1 << 25;
    if (p.n_tiles && (switches().cover > 0 || (switches().cover < 0 && pixels > kCoverMinPixels))) {
        const uint32_t regions_x = (w + 63) / 64, regions_y = (h + 63) / 64;
        const size_t regions = (size_t)n * regions_x * regions_y;      // < 2^32 / 4096 words
        const bool fresh = regions * sizeof(uint64_t) > c.d_cover.cap;
        if (int rc = ensure(stream, c.d_cover, regions * sizeof(uint64_t))) return rc;
        // the strip records of the claimed regions, for k_resolve: the owner words' lifetime, growth and discipline -- zeroed when
        // fresh and when the serial wraps (a record of serial 0 never matches), never reset between frames (c4: 19 MB per context)
        const size_t recs_bytes = regions * kOwnedStrips * kOwnedRecWords * sizeof(uint32_t);
        const bool owned = resolve_owned_ && switches().resolve_owned;
        const bool recs_fresh = owned && recs_bytes > c.d_cover_recs.cap;
        if (owned)
            if (int rc = ensure(stream, c.d_cover_recs, recs_bytes)) return rc;
        if (recs_fresh || (c.d_cover_recs.p && c.cover_serial == 0xFFFFFFFFu)) TOPO_HIP_TRY(hipMemsetAsync(c.d_cover_recs.p, 0, c.d_cover_recs.cap, stream));
        if (fresh || c.cover_serial == 0xFFFFFFFFu) {
            TOPO_HIP_TRY(hipMemsetAsync(c.d_cover.p, 0, c.d_cover.cap, stream));
            c.cover_serial = 0;
        }
        c.cover = CoverParams{c.d_cover.as<uint64_t>(), ++c.cover_serial, (uint32_t)regions, regions_x, regions_y, owned ? c.d_cover_recs.as<uint32_t>() : nullptr};
        c.cover_big_cap = p.big_cap;
    }
    if (!c.d_counters.p) {
        if (int rc = ensure(stream, c.d_counters, 2 * kCounterWords * sizeof(uint32_t))) return rc;      // two sets, alternating
        TOPO_HIP_TRY(hipMemsetAsync(c.d_counters.p, 0, 2 * kCounterWords * sizeof(uint32_t), stream));
    }
    if (int rc = ensure_pinned(c.h_status, kStatusRing * kStatusWords * sizeof(uint32_t))) return rc;
    if (c.submitted - c.checked == kStatusRing) {      // nobody has waited for this context's frames for a whole ring: fold them now
        if (c.last_stream) TOPO_HIP_TRY(hipStreamSynchronize(c.last_stream));      // (where the latest of them was queued)
        overflow_pending_ |= fold_frames(c);
    }
    c.last_stream = stream;
    c.pending = pipeline_depth_ > 1;
    p.work_cap = (uint32_t)work_cap;
    p.far_sub_cap = (uint32_t)far_sub_cap;
    p.near_cap = (uint32_t)near_cap;
    return TOPO_OK;
}

// View constants.  Up to kPackViews views (a panorama's eight sectors) travel as the argument of a one-workgroup kernel
// (k_put_views: the launch copies them; a copy-engine operation and the event guarding its pinned source cost the GPU 13 us
// per frame and the host two more calls).  Larger submissions go through a small ring of pinned staging slots, each guarded
// by an event, so a submission never has to wait for the stream (pageable sources would force a synchronous staging copy).
// Either way each slot has its own device copy, so a later submission cannot overwrite constants a running frame reads.
// (With the frame's first kernel being k_clear_cull -- there are tiles to cull -- the pack rides in THAT launch's argument
// segment, *pack_in_cull: no upload kernel either; TOPO_VIEWS_IN_CULL=0: always k_put_views.)
int TerrainRenderer::stage_views(FrameCtx& c, hipStream_t stream, const topo_uniforms* views, FrameParams& p, ViewPack& pack, bool* pack_in_cull) {
    const uint32_t n = p.n_views;
    if (n > kMaxViewsPerSlot) return fail(TOPO_ERR_INVALID, "too many views in one submission");
    static_assert(kViewSlots % kMaxPipeline == 0, "every frame context has its own share of the slots");
    // a slot belongs to one frame context, so whatever used it before is ahead of this submission in the same stream
    const int slot = (int)(&c - ctx_) * (kViewSlots / kMaxPipeline) + (int)(c.frames % (kViewSlots / kMaxPipeline));
    ViewDev* d_slot = d_views_.as<ViewDev>() + (size_t)slot * kMaxViewsPerSlot;
    p.views = d_slot;
    auto fill_views = [&](ViewDev* vd) {
        for (uint32_t i = 0; i < n; ++i) {
            memcpy(vd[i].proj, views[i].camera_proj, sizeof vd[i].proj);
            vd[i].cam_x = views[i].camera_pos[0];
            vd[i].cam_y = views[i].camera_pos[1];
            memcpy(vd[i].sun, views[i].sun_direction, sizeof vd[i].sun);
            vd[i].view_mode = views[i].view_mode;
        }
    };
    const bool packed = n <= kPackViews && !switches().views_by_copy;
    *pack_in_cull = packed && fused_clear_cull(p) && switches().views_in_cull;
    if (packed) {
        fill_views(pack.v);
        if (!*pack_in_cull) launch_put_views(pack, n, d_slot, stream);
        return TOPO_OK;
    }
    if (!view_ev_[kViewSlots - 1]) {      // first use (or whatever of it an earlier, failed one left undone)
        if (int rc = ensure_pinned(h_views_, sizeof(ViewDev) * kMaxViewsPerSlot * kViewSlots)) return rc;
        for (auto& e : view_ev_)
            if (!e) TOPO_HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
    }
    if (view_used_[slot]) TOPO_HIP_TRY(hipEventSynchronize(view_ev_[slot]));
    ViewDev* vd = h_views_.as<ViewDev>() + (size_t)slot * kMaxViewsPerSlot;
    fill_views(vd);
    TOPO_HIP_TRY(hipMemcpyAsync(d_slot, vd, n * sizeof(ViewDev), hipMemcpyHostToDevice, stream));
    TOPO_HIP_TRY(hipEventRecord(view_ev_[slot], stream));
    view_used_[slot] = true;
    return TOPO_OK;
}

// Everything of FrameParams that grow_frame_buffers and stage_views have not set (post_off and the resolve range: queue_frame).
void TerrainRenderer::fill_params(FrameCtx& c, FrameParams& p) {
    p.tiles = d_tiles_.as<const TileDev>();
    p.vis = c.d_vis.as<uint64_t>();
    p.dirty = c.d_dirty.as<uint8_t>();
    p.work = c.d_work.as<WorkItem>();
    // this frame's counter set; the other one is zeroed by this frame's clear for the next frame of the context
    p.counters = c.d_counters.as<uint32_t>() + (c.frames & 1u) * kCounterWords;
    // this frame's counters (queue fills, status bits), for whoever waits for the frame (check_frames, get_counters): stored by
    // k_resolve into the pinned ring.  The bounds-checking build, whose k_resolve may still set a status bit, copies them
    // behind the frame instead.
#ifdef TOPO_BOUNDS_CHECK
    p.status_out = nullptr;
#else
    p.status_out = switches().status_by_copy ? nullptr : c.status_words(c.submitted);
#endif
    p.big = c.d_big.as<BigItem>();
    p.rare = c.d_rare.as<RareItem>();
    p.far = c.d_far.as<FarItem>();
    p.work2 = c.d_work2.as<WorkItem>();
    p.split_m = occlusion_split_m_;
    p.tile_w = tile_w_;
    p.tile_h = tile_h_;
    p.tris_per_tile = p.n_tiles ? 2u * (tile_w_ - 1) * (tile_h_ - 1) : 8u;
    p.div_tris = fastdiv_make(p.tris_per_tile);
    p.div_hm1 = fastdiv_make(p.n_tiles ? tile_h_ - 1 : 2u);
    p.rblocks_x = ((uint32_t)p.W + kResolveBlockW - 1) / kResolveBlockW;
    p.rblocks_view = p.rblocks_x * (((uint32_t)p.H + kResolveBlockH - 1) / kResolveBlockH);
    p.div_rblocks_x = fastdiv_make(p.rblocks_x > 1 ? p.rblocks_x : 2u);
    p.div_rblocks_view = fastdiv_make(p.rblocks_view > 1 ? p.rblocks_view : 2u);
    // the cleared render target texel: Color{0, 0.71, 0.885, 1} (terrain_renderer.rs:379-384) stored as Rgba8UnormSrgb
    float thresh[256];
    for (int i = 0; i < 256; ++i) thresh[i] = bits_f(TOPO_SRGB_THRESH_BITS[i]);
    p.linear_target = is_linear(format_) ? 1u : 0u;
    p.bgra = is_bgra(format_) ? 1u : 0u;
    p.sky_c8 = (p.linear_target ? to_unorm8(0.0f) | (to_unorm8(0.71f) << 8) | (to_unorm8(0.885f) << 16)
                                : srgb_encode(thresh, 0.0f) | (srgb_encode(thresh, 0.71f) << 8) | (srgb_encode(thresh, 0.885f) << 16)) |
               (to_unorm8(1.0f) << 24);
}

// clear -> cull -> [near blocks: raster, rare, big] -> occlusion test of the far blocks -> [survivors: raster,
// rare, big] -> resolve: the stages of `Stage`, event i in front of stage i and the last one behind the frame.
int TerrainRenderer::queue_frame(FrameCtx& c, hipStream_t stream, FrameParams& p, const ViewPack* pack_in_cull, const CullList& cull, bool far_phase, const OutputParams& out,
                                 const ResolveSlot* slots, uint32_t n_slots, const std::function<int(uint32_t, hipStream_t)>* after_slot) {
    const uint32_t n = p.n_views, w = (uint32_t)p.W, h = (uint32_t)p.H;
    uint32_t* const counters_next = c.d_counters.as<uint32_t>() + ((c.frames & 1u) ^ 1u) * kCounterWords;
    // A timing event between two kernels costs ~6 us of idle GPU (the next kernel waits for the marker), so only the
    // events the selected timing slots need are recorded (topo_set_timing_slots); the total's pair unless that is switched off too.
    uint32_t ev_need = timing_total_ ? kTotalEvents : 0u;
    for (int sl = 0; sl < kTimingSlots; ++sl)
        for (int st = 0; st < kNumStages; ++st)
            if ((timing_slots_ & (1u << sl)) && (kStagesOfSlot[sl] & (1u << st))) ev_need |= stage_events(st);
    // With nothing but k_resolve's duration and / or the total selected (bench.py's timed region) the events are not markers between
    // the kernels but the kernels' own start and end times (hipExtLaunchKernel: the first event = start of the frame's first kernel,
    // the last two = start / end of k_resolve): a pair of markers costs a frame 8-10 us, these next to nothing.
    const bool pixelize = post_.pixelize_n < 99.99999f;
    const bool own_times = !switches().events_by_marker && !pixelize && (ev_need & ~(kTotalEvents | stage_events(kStResolve))) == 0;
    FrameCtx::TimedFrame& tf = c.timed_frames[c.frames++ % kEvRing];
    tf.recorded = ev_need;
    tf.slots = timing_slots_;
    tf.frame = ++frame_seq_;
    // event i, if it is needed: a marker on the stream (mark), or -- the three own_times hands to a launch instead -- the kernel's own (own)
    auto mark = [&](int i, bool may_be_own = false) { return (ev_need >> i & 1u) && !(may_be_own && own_times) ? hipEventRecord(tf.ev[i], stream) : hipSuccess; };
    auto own = [&](int i) -> hipEvent_t { return (ev_need >> i & 1u) && own_times ? (hipEvent_t)tf.ev[i] : nullptr; };
    TOPO_HIP_TRY(mark(kStClear, true));
    const hipEvent_t ev_first = own(kStClear);
    // clear and cull side by side in one launch (timing slot "clear" then holds both, "cull" nothing); TOPO_FUSE_CLEAR_CULL=0 or
    // an empty tile set: one after the other
    const bool fuse = fused_clear_cull(p);
    if (fuse) launch_clear_cull(p, counters_next, stream, ev_first, pack_in_cull, n, cull.codes, cull.n);
    else launch_clear(p, counters_next, stream, ev_first);
    TOPO_HIP_TRY(mark(kStCull));
    if (!fuse) launch_cull(p, stream, cull.codes, cull.n);
    TOPO_HIP_TRY(mark(kStRasterNear));
    launch_raster(p, 0, stream);
    TOPO_HIP_TRY(mark(kStRareBigNear));
    launch_raster_rare(p, c.cover, stream);
    launch_raster_cover(p, c.cover, stream);      // the regions one giant covers whole, with plain stores; the rest: k_raster_big's atomics
    launch_raster_big(p, c.cover, stream);
    TOPO_HIP_TRY(mark(kStOcclusion));
    if (far_phase) launch_occlusion(p, stream);
    TOPO_HIP_TRY(mark(kStRasterFar));
    if (far_phase) launch_raster(p, 1, stream);
    TOPO_HIP_TRY(mark(kStRareBigFar));
    if (far_phase) {
        launch_raster_rare(p, CoverParams{}, stream);
        launch_raster_big(p, CoverParams{}, stream);
    }
    TOPO_HIP_TRY(mark(kStResolve, true));
    const hipEvent_t ev_rstart = own(kStResolve), ev_rstop = own(kNumStages);
    // The pixelise branch of the post shader (pixelize_n < 99.99999; the reference never takes it) samples the render target
    // away from the pixel's own texel: k_resolve then stores the render-target texels into an image of the frame context's
    // (post_off) and k_post_pixelize makes the surface image from it and the depth image.  The images belong to the context,
    // like d_vis: frames in flight on other contexts neither share nor reallocate them.
    OutputParams kout = out;
    if (pixelize) {
        if (n_slots) return fail(TOPO_ERR_UNSUPPORTED, "the pixelise branch is not available on the slot-by-slot (multi-GPU) path");
        const size_t img = (size_t)w * h * 4;
        if (int rc = ensure(stream, c.d_pre_rgba, img * n)) return rc;
        if (!out.depth)
            if (int rc = ensure(stream, c.d_pre_depth, img * n)) return rc;
        kout.rgba = c.d_pre_rgba.as<uint8_t>();
        kout.rgba_view_stride = img;
        kout.rgba_pitch = (size_t)w * 4;
        if (!out.depth) { kout.depth = c.d_pre_depth.as<float>(); kout.depth_view_stride = img; kout.depth_pitch = (size_t)w * 4; }
        p.post_off = 1;
    }
    if (n_slots == 0) {
        p.rblock_first = 0;
        p.rblock_count = p.rblocks_view * n;
        launch_resolve(p, kout, c.cover, stream, ev_rstart, ev_rstop);
        if (pixelize)
            launch_post_pixelize(n, (int32_t)w, (int32_t)h, post_.viewport[0] >= 1.0f ? post_.viewport[0] : (float)w, post_.viewport[1] >= 1.0f ? post_.viewport[1] : (float)h,
                                 post_.pixelize_n, c.d_pre_rgba.as<const uint8_t>(), out, kout.depth, kout.depth_view_stride, kout.depth_pitch, p.linear_target, p.bgra, stream);
    } else {
        for (uint32_t i = 0; i < n_slots; ++i) {
            if ((uint64_t)slots[i].block_first + slots[i].block_count > (uint64_t)p.rblocks_view * n) return fail(TOPO_ERR_INVALID, "resolve slot outside the frame");
            p.rblock_first = slots[i].block_first;
            p.rblock_count = slots[i].block_count;
            launch_resolve(p, out, c.cover, stream, i == 0 ? ev_rstart : nullptr, i + 1 == n_slots ? ev_rstop : nullptr);
            if (after_slot)
                if (int rc = (*after_slot)(i, stream)) return rc;
        }
    }
    if (vs_on_)      // behind the frame's last k_resolve (and its last slot): the cells that won a pixel, into the tiles' masks
        launch_viewshed(p, d_vs_table_.as<uint32_t* const>(), d_vs_stats_.as<unsigned long long>(), stream);
    TOPO_HIP_TRY(mark(kNumStages, true));
    if (!p.status_out) TOPO_HIP_TRY(hipMemcpyAsync(c.status_words(c.submitted), p.counters, kStatusWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return TOPO_OK;
}

// The submission as the status ring, the timings and the horizon and ground queries see it.
void TerrainRenderer::record_submission(FrameCtx& c, const FrameParams& p, const topo_uniforms* views) {
    ++c.submitted;
    c.timed = true;
    c.sub.n_views = p.n_views;
    c.sub.tile_gen = tile_gen_;
    c.sub.views.resize(p.n_views);
    for (uint32_t i = 0; i < p.n_views; ++i) {
        memcpy(c.sub.views[i].proj, views[i].camera_proj, sizeof c.sub.views[i].proj);
        memcpy(c.sub.views[i].pos, views[i].camera_pos, sizeof c.sub.views[i].pos);
        c.sub.views[i].pad_ = 0.0f;
    }
    c.sub.views_on_device = false;
    c.lists_valid = true;
    c.lists_near_cap = p.near_cap;
    c.lists_far_sub_cap = p.far_sub_cap;
    HorizonParams& q = c.sub.query;
    q.vis = p.vis;
    q.dirty = p.dirty;
    q.counters = p.counters;
    q.W = (uint32_t)p.W;
    q.H = (uint32_t)p.H;
    q.n_keys = (size_t)p.n_views * q.W * q.H;
    q.n_tiles = p.n_tiles;
    q.tris_per_tile = p.tris_per_tile;
    q.hm1 = p.n_tiles ? tile_h_ - 1 : 2u;
    q.div_tris = p.div_tris;
    q.div_hm1 = p.div_hm1;
    latest_ctx_ = (int)(&c - ctx_);
}

int TerrainRenderer::render_device(uint8_t* rgba_dev, size_t rgba_pitch, float* depth_dev, size_t depth_pitch) {
    if (!rgba_dev) return fail(TOPO_ERR_INVALID, "rgba_dev is null");
    if (!have_uniforms_) return fail(TOPO_ERR_INVALID, "topo_update has not been called");
    if (rgba_pitch < (size_t)W_ * 4 || (depth_dev && depth_pitch < (size_t)W_ * 4)) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    return render_views_device(1, &uniforms_, W_, H_, image_output(rgba_dev, rgba_pitch, depth_dev, depth_pitch, H_));
}

// render (terrain_renderer.rs:365-452) + depth copy (render_engine.rs:219-249), host outputs.
int TerrainRenderer::render(uint8_t* rgba, size_t rgba_pitch, float* depth, size_t depth_pitch) {
    if (!rgba) return fail(TOPO_ERR_INVALID, "rgba_out is null");
    if (!have_uniforms_) return fail(TOPO_ERR_INVALID, "topo_update has not been called");
    if (rgba_pitch < (size_t)W_ * 4 || (depth && depth_pitch < (size_t)W_ * 4)) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    if (int rc = bind_device()) return rc;
    const size_t row = (size_t)W_ * 4;
    if (int rc = ensure(stream_, d_out_rgba_, row * H_)) return rc;
    if (depth)
        if (int rc = ensure(stream_, d_out_depth_, row * H_)) return rc;
    const OutputParams o = image_output(d_out_rgba_.as<uint8_t>(), row, depth ? d_out_depth_.as<float>() : nullptr, row, H_);
    // A frame whose rare-triangle queue overflowed is incomplete.  The synchronous entry point does not hand such a frame
    // out: it grows the queue to what the frame asked for and renders it again (an explicit topo_debug_set_queue_caps
    // setting is a test hook and is left alone: then the call fails with TOPO_ERR_CAPACITY).
    // Frames queued earlier through the asynchronous entry points are waited for, but an overflow of one of THEM is not this
    // call's error (the caller could not tell which frame failed, and this frame would go unrendered): it stays pending and
    // is reported, once, by the next topo_join / topo_synchronize -- the calls that wait for those frames.
    if (int rc = wait_all()) return rc;
    overflow_pending_ |= fold_idle();
    for (int attempt = 0;; ++attempt) {
        if (int rc = render_views_device(1, &uniforms_, W_, H_, o)) return rc;
        if (int rc = wait_all()) return rc;       // (pipelined contexts run on their own streams)
        FrameCtx& fc = ctx_[last_ctx_];
        const bool retry = rare_cap_cfg_ == 0 && attempt < 3;
        if (!fold_latest(fc, retry)) break;      // (the frames in front of this one were folded above)
        if (!retry) return fail(TOPO_ERR_CAPACITY, "rare-triangle queue overflowed: frame incomplete");
        const uint32_t wanted = fc.latest_status()[kCtrRare];
        rare_cap_auto_ = (uint64_t)wanted + wanted / 4u + 1024u;      // the overflowed frame counted what it needs
        if (rare_cap_auto_ > (1ull << 28)) return fail(TOPO_ERR_CAPACITY, "rare-triangle queue would exceed 2^28 entries");
    }
    if (int rc = download(rgba, rgba_pitch, d_out_rgba_.as<const uint8_t>(), row)) return rc;
    if (depth)
        if (int rc = download((uint8_t*)depth, depth_pitch, d_out_depth_.as<const uint8_t>(), row)) return rc;
    have_depth_ = depth != nullptr;
    depth_w_ = W_;
    depth_h_ = H_;
    return TOPO_OK;
}

// One H_-row image from device memory into the caller's HOST buffer.  A copy into pageable memory makes the runtime stage it
// through its own small pinned buffers, synchronously: ~10 GB/s, 6.8 ms for the RGBA + depth of a 2048 x 4096 frame, fifty
// times the frame's render time.  So: buffers the caller has pinned (topo_pin_host_buffer) are written directly, at the
// link's rate; any other buffer is filled through a pinned staging buffer of the context's own, in slices -- the device
// copies slice k + 1 while a few host threads move slice k on to the caller's rows.
int TerrainRenderer::download(uint8_t* dst, size_t dst_pitch, const uint8_t* src_dev, size_t row) {
    const size_t span = dst_pitch * (H_ - 1) + row;
    for (const auto& pin : pinned_)
        if (dst >= pin.as<uint8_t>() && dst + span <= pin.as<uint8_t>() + pin.cap) {
            TOPO_HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch, src_dev, row, row, H_, hipMemcpyDeviceToHost, stream_));
            TOPO_HIP_TRY(hipStreamSynchronize(stream_));
            return TOPO_OK;
        }
    const size_t total = row * H_;
    if (int rc = ensure_pinned(h_stage_, total)) return rc;
    uint8_t* const stage = h_stage_.as<uint8_t>();
    constexpr int kSlices = 8;
    for (auto& e : stage_ev_)
        if (!e) TOPO_HIP_TRY(hipEventCreateWithFlags(&e.h, hipEventDisableTiming));
    const uint32_t rows_per = (H_ + kSlices - 1) / kSlices;
    int n_slices = 0;
    for (uint32_t r0 = 0; r0 < H_; r0 += rows_per, ++n_slices) {
        const uint32_t rows = std::min(rows_per, H_ - r0);
        TOPO_HIP_TRY(hipMemcpyAsync(stage + (size_t)r0 * row, src_dev + (size_t)r0 * row, (size_t)rows * row, hipMemcpyDeviceToHost, stream_));
        TOPO_HIP_TRY(hipEventRecord(stage_ev_[n_slices], stream_));
    }
    const unsigned hw = std::thread::hardware_concurrency();
    const int n_threads = (int)std::min<size_t>(std::max(1u, std::min(hw ? hw : 4u, 8u)), std::max<size_t>(1, total >> 20));      // one per MiB, at most 8
    std::atomic<int> failed{0};
    auto worker = [&](int t) {
        (void)hipSetDevice(device_);
        for (int k = 0; k < n_slices; ++k) {
            if (hipEventSynchronize(stage_ev_[k]) != hipSuccess) { failed = 1; return; }
            const uint32_t r0 = (uint32_t)k * rows_per, rows = std::min(rows_per, H_ - r0);
            const uint32_t a = r0 + (uint32_t)((uint64_t)rows * t / n_threads), b = r0 + (uint32_t)((uint64_t)rows * (t + 1) / n_threads);
            if (dst_pitch == row) memcpy(dst + (size_t)a * row, stage + (size_t)a * row, (size_t)(b - a) * row);
            else
                for (uint32_t r = a; r < b; ++r) memcpy(dst + (size_t)r * dst_pitch, stage + (size_t)r * row, row);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; ++t) pool.emplace_back(worker, t);
    worker(0);
    for (auto& th : pool) th.join();
    if (failed) return fail(TOPO_ERR_HIP, "device-to-host copy failed");
    return TOPO_OK;
}

// The caller's own output buffers, pinned once (hipHostRegister): topo_render then copies into them directly.
int TerrainRenderer::pin_host_buffer(void* p, size_t bytes) {
    if (!p || bytes == 0) return fail(TOPO_ERR_INVALID, "null/empty buffer");
    if (int rc = bind_device()) return rc;
    for (const auto& pin : pinned_)
        if (pin.p == p) return pin.cap == bytes ? TOPO_OK : fail(TOPO_ERR_INVALID, "buffer already pinned with another size");
    TOPO_HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    pinned_.emplace_back();
    pinned_.back().p = p;
    pinned_.back().cap = bytes;
    return TOPO_OK;
}

int TerrainRenderer::unpin_host_buffer(void* p) {
    for (size_t i = 0; i < pinned_.size(); ++i)
        if (pinned_[i].p == p) {
            if (int rc = bind_device()) return rc;
            TOPO_HIP_TRY(hipStreamSynchronize(stream_));
            pinned_.erase(pinned_.begin() + (long)i);      // (unregisters it)
            return TOPO_OK;
        }
    return fail(TOPO_ERR_NOT_FOUND, "buffer was not pinned by topo_pin_host_buffer");
}

// What both overlay passes start with: the call's geometry on the device -- part a, then part b 16-byte aligned behind it
// (*b_dev) -- and the W x H overlay keys, *keys_fresh when the pass has to initialise them.
int TerrainRenderer::overlay_upload(const void* a, size_t a_bytes, const void* b, size_t b_bytes, uint8_t** b_dev, bool* keys_fresh) {
    if (int rc = bind_device()) return rc;
    const size_t b_off = (a_bytes + 15) & ~(size_t)15, keys_b = (size_t)W_ * H_ * 8;
    if (int rc = ensure(stream_, d_overlay_geo_, b_off + b_bytes + 16)) return rc;
    *keys_fresh = keys_b > d_overlay_keys_.cap || overlay_w_ != W_ || overlay_h_ != H_;
    if (int rc = ensure(stream_, d_overlay_keys_, keys_b)) return rc;
    overlay_w_ = W_; overlay_h_ = H_;
    *b_dev = d_overlay_geo_.as<uint8_t>() + b_off;
    if (a_bytes) TOPO_HIP_TRY(hipMemcpyAsync(d_overlay_geo_.p, a, a_bytes, hipMemcpyHostToDevice, stream_));
    if (b_bytes) TOPO_HIP_TRY(hipMemcpyAsync(*b_dev, b, b_bytes, hipMemcpyHostToDevice, stream_));
    return TOPO_OK;
}

// Host image in, host image out (the frame topo_render returned, or any W x H image in the context's format): `draw` is one of
// the device forms below, over the image's device copy.
template <class Draw>
int TerrainRenderer::overlay_host_image(uint8_t* rgba, size_t rgba_pitch, Draw draw) {
    if (!rgba) return fail(TOPO_ERR_INVALID, "null argument");
    if (rgba_pitch < (size_t)W_ * 4) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    if (int rc = bind_device()) return rc;
    const size_t row = (size_t)W_ * 4;
    if (int rc = ensure(stream_, d_out_rgba_, row * H_)) return rc;
    TOPO_HIP_TRY(hipMemcpy2DAsync(d_out_rgba_.p, row, rgba, rgba_pitch, row, H_, hipMemcpyHostToDevice, stream_));
    if (int rc = draw(d_out_rgba_.as<uint8_t>(), row)) return rc;
    TOPO_HIP_TRY(hipMemcpy2DAsync(rgba, rgba_pitch, d_out_rgba_.p, row, row, H_, hipMemcpyDeviceToHost, stream_));
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    return TOPO_OK;
}

// LineRenderer::render (line_renderer.rs:200-212) over an image this context produced: the overlay triangles are drawn
// on top of the post pass's output with the reference's layering (depth Greater against the post quad's 1/4096).
int TerrainRenderer::overlay_lines_device(const void* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, float line_width,
                                          uint8_t* rgba_dev, size_t rgba_pitch) {
    if ((n_vertices && !vertices) || (n_indices && !indices) || !rgba_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if (n_indices % 3 != 0) return fail(TOPO_ERR_INVALID, "the overlay is a triangle list: index count must be a multiple of 3");
    if (rgba_pitch < (size_t)W_ * 4) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    uint8_t* d_idx = nullptr;
    bool fresh = false;
    if (int rc = overlay_upload(vertices, (size_t)n_vertices * sizeof(OverlayVertex), indices, (size_t)n_indices * 4, &d_idx, &fresh)) return rc;
    launch_overlay(d_overlay_geo_.as<const OverlayVertex>(), (const uint32_t*)d_idx, n_indices / 3, n_vertices, line_width, (int32_t)W_, (int32_t)H_,
                   d_overlay_keys_.as<uint64_t>(), fresh, rgba_dev, rgba_pitch, is_linear(format_), is_bgra(format_), stream_);
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));      // the geometry is only borrowed for the call
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

int TerrainRenderer::overlay_lines(const void* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, float line_width,
                                   uint8_t* rgba, size_t rgba_pitch) {
    return overlay_host_image(rgba, rgba_pitch, [&](uint8_t* img, size_t pitch) {
        return overlay_lines_device(vertices, n_vertices, indices, n_indices, line_width, img, pitch);
    });
}

// TextRenderer::render (text_renderer.rs:198-204) over an image this context produced: glyphon's glyph quads, alpha-blended,
// the first quad over a pixel keeping it (depth Greater with write at one depth).
int TerrainRenderer::overlay_glyphs_device(const void* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas, uint32_t atlas_w, uint32_t atlas_h,
                                           uint8_t* rgba_dev, size_t rgba_pitch) {
    if ((n_glyphs && (!glyphs || !atlas)) || !rgba_dev) return fail(TOPO_ERR_INVALID, "null argument");
    if (rgba_pitch < (size_t)W_ * 4) return fail(TOPO_ERR_INVALID, "pitch smaller than a row");
    if (!(depth > 1.0f / 4096.0f) || !(depth <= 1.0f)) return fail(TOPO_ERR_INVALID, "glyph depth must lie above the post quad's 1/4096 (the reference: 100/4096)");
    const GlyphInstance* gs = (const GlyphInstance*)glyphs;
    for (uint32_t i = 0; i < n_glyphs; ++i)
        if (gs[i].content_type_with_srgb[0] != 1) return fail(TOPO_ERR_UNSUPPORTED, "only mask glyphs (glyphon content type 1) are drawn; colour glyphs are not");
    uint8_t* d_atlas = nullptr;
    bool fresh = false;
    if (int rc = overlay_upload(glyphs, (size_t)n_glyphs * sizeof(GlyphInstance), atlas, (size_t)atlas_w * atlas_h, &d_atlas, &fresh)) return rc;
    launch_overlay_glyphs(d_overlay_geo_.as<const GlyphInstance>(), n_glyphs, depth, d_atlas, atlas_w, atlas_h, (int32_t)W_, (int32_t)H_,
                          d_overlay_keys_.as<uint64_t>(), fresh, rgba_dev, rgba_pitch, is_linear(format_), is_bgra(format_), stream_);
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));      // glyphs and atlas are only borrowed for the call
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

int TerrainRenderer::overlay_glyphs(const void* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas, uint32_t atlas_w, uint32_t atlas_h, uint8_t* rgba,
                                    size_t rgba_pitch) {
    return overlay_host_image(rgba, rgba_pitch, [&](uint8_t* img, size_t pitch) {
        return overlay_glyphs_device(glyphs, n_glyphs, depth, atlas, atlas_w, atlas_h, img, pitch);
    });
}

// RenderEngine::get_visible_labels over the depth the context already holds on the device.
int TerrainRenderer::visible_peaks_device(const topo_uniforms* view, uint32_t w, uint32_t h, const float* depth_dev, size_t depth_pitch,
                                          uint32_t n, const float* peaks_dev, uint8_t* visible_dev, uint32_t* xy_dev) {
    if (!view || !depth_dev || (n && (!peaks_dev || !visible_dev || !xy_dev))) return fail(TOPO_ERR_INVALID, "null argument");
    if (int rc = bind_device()) return rc;
    if (int rc = ensure(stream_, d_proj_, 16 * sizeof(float))) return rc;
    TOPO_HIP_TRY(hipMemcpyAsync(d_proj_.p, view->camera_proj, 16 * sizeof(float), hipMemcpyHostToDevice, stream_));
    launch_visible_peaks(d_proj_.as<const float>(), w, h, depth_dev, depth_pitch, n, peaks_dev, visible_dev, xy_dev, stream_);
    TOPO_HIP_TRY(hipGetLastError());
    return TOPO_OK;
}

int TerrainRenderer::visible_peaks(uint32_t n, const float* peaks, uint8_t* visible, uint32_t* xy) {
    if (n && (!peaks || !visible || !xy)) return fail(TOPO_ERR_INVALID, "null argument");
    if (!have_depth_ || depth_w_ != W_ || depth_h_ != H_)
        return fail(TOPO_ERR_INVALID, "topo_visible_peaks needs the depth of a preceding topo_render(.., depth_out, ..) at the current size");
    if (n == 0) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    const size_t in_b = (size_t)n * 12, xy_b = (size_t)n * 8, vis_b = ((size_t)n + 15) & ~(size_t)15;
    if (int rc = ensure(stream_, d_peaks_, in_b + xy_b + vis_b)) return rc;
    uint8_t* base = d_peaks_.as<uint8_t>();
    TOPO_HIP_TRY(hipMemcpyAsync(base, peaks, in_b, hipMemcpyHostToDevice, stream_));
    if (int rc = visible_peaks_device(&uniforms_, W_, H_, d_out_depth_.as<const float>(), (size_t)W_ * 4, n, (const float*)base,
                                      base + in_b + xy_b, (uint32_t*)(base + in_b)))
        return rc;
    TOPO_HIP_TRY(hipMemcpyAsync(xy, base + in_b, xy_b, hipMemcpyDeviceToHost, stream_));
    TOPO_HIP_TRY(hipMemcpyAsync(visible, base + in_b + xy_b, n, hipMemcpyDeviceToHost, stream_));
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    return TOPO_OK;
}

int TerrainRenderer::set_stream(hipStream_t s) {
    if (int rc = wait_all()) return rc;
    for (auto& c : ctx_) c.last_stream = nullptr;      // (every frame has finished; the old stream may go away)
    stream_ = s ? s : own_stream_;
    return TOPO_OK;
}

int TerrainRenderer::synchronize() {
    if (int rc = wait_all()) return rc;
    return check_frames();
}

int TerrainRenderer::join_frames() {
    if (int rc = join()) return rc;      // (depth > 1: also a slot-by-slot panorama's frame on stream_)
    if (pipeline_depth_ == 1) TOPO_HIP_TRY(hipStreamSynchronize(stream_));      // one frame in flight: it runs on stream_
    return check_frames();
}

int TerrainRenderer::frame_status(uint32_t out[4]) {
    if (int rc = wait_all()) return rc;
    // (folds the finished frames into last_status_; an overflow is reported through out[0] here, and stays pending as the error
    // of the next call that waits for frames)
    overflow_pending_ |= fold_idle();
    if (int rc = query_fold_check()) return rc;
    for (int i = 0; i < 4; ++i) out[i] = last_status_[i];
    last_status_[0] = last_status_[1] = last_status_[2] = last_status_[3] = 0;
    return TOPO_OK;
}

int TerrainRenderer::set_normals_lds_rows(int rows) {
    if (rows != 0 && rows != 4 && rows != 8 && rows != 16 && rows != 32 && rows != 64) return fail(TOPO_ERR_INVALID, "lds rows must be 4, 8, 16, 32 or 64 (0: the form without an LDS tile)");
    lds_rows_ = rows;
    return TOPO_OK;
}

int TerrainRenderer::set_timing_slots(uint32_t mask) {
    timing_slots_ = mask & 0x3Fu;
    timing_total_ = !(mask & TOPO_TIMING_NO_TOTAL);
    return TOPO_OK;
}

int TerrainRenderer::set_occlusion_split(float metres) {
    if (!(metres >= 0.0f)) return fail(TOPO_ERR_INVALID, "split must be >= 0");
    occlusion_split_m_ = metres;
    return TOPO_OK;
}

int TerrainRenderer::set_queue_caps(uint32_t big_cap, uint32_t rare_cap) {
    big_cap_cfg_ = big_cap;
    // bit 31 of rare_cap: "start at this capacity but grow on demand" (what the default does from 4 Mi entries)
    rare_cap_cfg_ = (rare_cap & 0x80000000u) ? 0u : rare_cap;
    rare_cap_auto_ = (rare_cap & 0x80000000u) ? (rare_cap & 0x7FFFFFFFu) : 0u;
    return join();
}

// Durations of the frame timed by f (out[0..6]; the frame must have completed): a slot selected for it is the sum of its stages, any
// other reads 0 (a neighbour's events may have bracketed its stages by chance).
int TerrainRenderer::frame_durations(const FrameCtx::TimedFrame& f, float out[7]) {
    for (int sl = 0; sl <= kTimingSlots; ++sl) out[sl] = 0.0f;
    for (int sl = 0; sl < kTimingSlots; ++sl)
        for (int st = 0; st < kNumStages; ++st)
            if ((f.slots & (1u << sl)) && (kStagesOfSlot[sl] & (1u << st)) && (f.recorded & stage_events(st)) == stage_events(st)) {
                float d = 0.0f;
                TOPO_HIP_TRY(hipEventElapsedTime(&d, f.ev[st], f.ev[st + 1]));
                out[sl] += d;
            }
    if ((f.recorded & kTotalEvents) == kTotalEvents) TOPO_HIP_TRY(hipEventElapsedTime(&out[kTimingSlots], f.ev[0], f.ev[kNumStages]));
    return TOPO_OK;
}

int TerrainRenderer::get_timings(float out[TOPO_TIMING_SLOTS]) {
    for (int i = 0; i < TOPO_TIMING_SLOTS; ++i) out[i] = 0.0f;
    if (int rc = bind_device()) return rc;
    // depth 1: the last frame.  Pipelined: the OLDEST frame in flight (the context the next submission will reuse), so
    // that reading timings every frame does not wait for the frame just submitted
    FrameCtx& c = ctx_[pipeline_depth_ > 1 ? next_ctx_ : last_ctx_];
    if (c.timed && c.frames) {
        const FrameCtx::TimedFrame& f = c.timed_frames[(c.frames - 1) % kEvRing];
        if (f.recorded & kLastEvent) TOPO_HIP_TRY(hipEventSynchronize(f.ev[kNumStages]));
        else if (c.last_stream) TOPO_HIP_TRY(hipStreamSynchronize(c.last_stream));      // (TOPO_TIMING_NO_TOTAL: no event behind the frame)
        if (int rc = frame_durations(f, out)) return rc;
    }
    if (load_timed_) {
        TOPO_HIP_TRY(hipEventSynchronize(load_ev_[1]));
        TOPO_HIP_TRY(hipEventElapsedTime(&out[7], load_ev_[0], load_ev_[1]));      // the whole load phase
        TOPO_HIP_TRY(hipEventElapsedTime(&out[8], load_ev_[0], load_ev_[2]));      // its tables part
    }
    return TOPO_OK;
}

// The last n_frames frames (at most kEvRing per context), oldest first, 7 durations each (slots [0]..[6] of topo_get_timings).
// Waits for the frames in flight: meant to be called after a timed region, not inside it.
int TerrainRenderer::get_timing_history(uint32_t n_frames, float* out_ms, uint32_t* n_out) {
    *n_out = 0;
    if (!out_ms && n_frames) return fail(TOPO_ERR_INVALID, "null argument");
    if (int rc = wait_all()) return rc;
    std::vector<const FrameCtx::TimedFrame*> refs;
    for (const FrameCtx& c : ctx_)
        for (uint64_t k = 0; k < std::min<uint64_t>(c.frames, kEvRing); ++k) refs.push_back(&c.timed_frames[(c.frames - 1 - k) % kEvRing]);
    std::sort(refs.begin(), refs.end(), [](const FrameCtx::TimedFrame* a, const FrameCtx::TimedFrame* b) { return a->frame < b->frame; });
    const size_t n = std::min<size_t>(n_frames, refs.size());
    for (size_t i = 0; i < n; ++i)
        if (int rc = frame_durations(*refs[refs.size() - n + i], out_ms + 7 * i)) return rc;
    *n_out = (uint32_t)n;
    return TOPO_OK;
}

int TerrainRenderer::get_counters(uint32_t out[6]) {
    for (int i = 0; i < 6; ++i) out[i] = 0;
    FrameCtx& fc = ctx_[last_ctx_];
    if (!fc.h_status.p) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    if (fc.last_stream) TOPO_HIP_TRY(hipStreamSynchronize(fc.last_stream));      // the stream the frame was queued on
    uint32_t c[kStatusWords] = {};
    if (fc.submitted) memcpy(c, fc.latest_status(), sizeof c);
    if (getenv("TOPO_DEBUG_COUNTERS")) {   // raw queue counters, for kernel experiments
        fprintf(stderr, "[topo] counters:");
        for (uint32_t i = 0; i < kStatusWords; ++i) fprintf(stderr, " %u", c[i]);
        fprintf(stderr, "\n");
    }
    static_assert(kCtrWork == 0 && kCtrFarSurvived == 5, "topo_get_counters hands out words kCtrWork .. kCtrFarSurvived");
    for (uint32_t i = kCtrWork; i <= kCtrFarSurvived; ++i) out[i] = c[i];
    return TOPO_OK;
}

int TerrainRenderer::cover_stats(uint32_t out[3]) {
    out[0] = out[1] = out[2] = 0;
    FrameCtx& fc = ctx_[last_ctx_];
    if (!fc.h_status.p || !fc.submitted) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    if (fc.last_stream) TOPO_HIP_TRY(hipStreamSynchronize(fc.last_stream));
    // The frame itself counts nothing (a counter every claim goes through would be thousands of atomics on one address): the
    // covering items are the flagged entries of the frame's part of the big queue, the claims won the owner words of its serial.
    const CoverParams& cv = fc.cover;
    if (!cv.serial) return TOPO_OK;
    const uint32_t n_big = std::min(fc.latest_status()[kCtrBig], fc.cover_big_cap);
    std::vector<BigItem> items(n_big);
    std::vector<uint64_t> owner(cv.cap);
    if (n_big) TOPO_HIP_TRY(hipMemcpy(items.data(), fc.d_big.p, n_big * sizeof(BigItem), hipMemcpyDeviceToHost));
    if (cv.cap) TOPO_HIP_TRY(hipMemcpy(owner.data(), cv.owner, cv.cap * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (const BigItem& it : items) out[0] += it.id != kNoTri && (it.view & kBigCovered) ? 1u : 0u;
    for (uint64_t w : owner) out[1] += (uint32_t)(w >> 32) == cv.serial ? 1u : 0u;
    out[2] = out[0] - out[1];      // every covering item either wins its region or loses it to another one
    return TOPO_OK;
}

// The strips of the last frame that k_resolve's ownership test accepts, and the strips whose record carries the frame's serial,
// counted here from the keys and the table as the frame left them (the frame keeps no statistics).
int TerrainRenderer::owned_strips(uint32_t out[2]) {
    out[0] = out[1] = 0;
    FrameCtx& fc = ctx_[last_ctx_];
    if (!fc.h_status.p || !fc.submitted) return TOPO_OK;
    if (int rc = bind_device()) return rc;
    if (fc.last_stream) TOPO_HIP_TRY(hipStreamSynchronize(fc.last_stream));
    const CoverParams& cv = fc.cover;
    const HorizonParams& q = fc.sub.query;
    if (!cv.serial || !cv.recs || !q.vis) return TOPO_OK;
    const uint32_t W = q.W, H = q.H, n_views = fc.sub.n_views;
    std::vector<uint32_t> recs((size_t)cv.cap * kOwnedStrips * kOwnedRecWords);
    std::vector<uint64_t> keys((size_t)W * H);
    if (!recs.empty()) TOPO_HIP_TRY(hipMemcpy(recs.data(), cv.recs, recs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t v = 0; v < n_views; ++v) {
        TOPO_HIP_TRY(hipMemcpy(keys.data(), q.vis + (size_t)v * W * H, keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < H; y += kOwnedStripRows)
            for (uint32_t x = 0; x < W; x += 64) {
                const size_t at = owned_record_index(cv.regions_x, cv.regions_y, v, (int32_t)x, (int32_t)y);
                if (at >= (size_t)cv.cap * kOwnedStrips) return fail(TOPO_ERR_INVALID, "a strip of the frame has no record in the table");
                const uint32_t* rec = recs.data() + at * kOwnedRecWords;
                if (rec[kOwnedSerialWord] != cv.serial) continue;
                ++out[1];
                bool same = true;
                for (uint32_t py = y; py < std::min(y + kOwnedStripRows, H) && same; ++py)
                    for (uint32_t px = x; px < std::min(x + 64u, W) && same; ++px) same = (uint32_t)keys[(size_t)py * W + px] == rec[kOwnedIdWord];
                out[0] += same ? 1u : 0u;
            }
    }
    return TOPO_OK;
}

// What the last frame's cull and occlusion test decided.  The lists and the counter set stay as the frame left them until the
// context's next submission: a frame's clear zeroes the OTHER counter set (the next frame's), the status ring gets a copy of the
// first kStatusWords words and never writes back, the queries behind a frame (horizon, ground, viewshed) only read the status word,
// and d_work / d_far / d_work2 are written by k_cull and k_occlusion alone and reallocated by grow_frame_buffers alone, both inside
// a submission.  With more than one frame in flight the "last" context is not well defined for a caller: depth 1 only.
int TerrainRenderer::read_cull_lists(uint32_t* near_out, uint32_t near_room, uint32_t* far_out, uint32_t far_room, uint32_t* survivors_out,
                                     uint32_t survivors_room, uint32_t counts_out[5]) {
    static_assert(sizeof(WorkItem) == 8 && sizeof(FarItem) == 20, "the lists go out as 2 and 5 words per entry");
    if (!counts_out) return fail(TOPO_ERR_INVALID, "null argument");
    if (pipeline_depth_ != 1) return fail(TOPO_ERR_INVALID, "the cull lists can be read at pipeline depth 1 only");
    FrameCtx& fc = ctx_[last_ctx_];
    // (lists_valid: a submission that failed half-way, or one from before a change of the pipeline depth, has left nothing to read)
    if (!fc.submitted || !fc.lists_valid || !fc.sub.query.counters) return fail(TOPO_ERR_INVALID, "no submission has been made");
    if (int rc = bind_device()) return rc;
    if (int rc = wait_all()) return rc;
    std::vector<uint32_t> ctr(kCounterWords);
    TOPO_HIP_TRY(hipMemcpy(ctr.data(), fc.sub.query.counters, kCounterWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t n_near = std::min(ctr[kCtrWork], fc.lists_near_cap), n_surv = std::min(ctr[kCtrFarSurvived], fc.lists_near_cap);
    uint32_t n_far = 0;
    for (uint32_t q = 0; q < kFarLists; ++q) n_far += std::min(ctr[far_list_counter(q)], fc.lists_far_sub_cap);
    counts_out[0] = n_near; counts_out[1] = n_far; counts_out[2] = n_surv;
    counts_out[3] = ctr[kCtrFarTested]; counts_out[4] = ctr[kCtrFarSurvived];
    if (near_out && std::min(n_near, near_room))
        TOPO_HIP_TRY(hipMemcpy(near_out, fc.d_work.p, (size_t)std::min(n_near, near_room) * sizeof(WorkItem), hipMemcpyDeviceToHost));
    if (survivors_out && std::min(n_surv, survivors_room))
        TOPO_HIP_TRY(hipMemcpy(survivors_out, fc.d_work2.p, (size_t)std::min(n_surv, survivors_room) * sizeof(WorkItem), hipMemcpyDeviceToHost));
    if (far_out) {
        uint32_t at = 0;      // the sub-lists one behind the other, in k_occlusion's order
        for (uint32_t q = 0; q < kFarLists && at < far_room; ++q) {
            const uint32_t n = std::min(std::min(ctr[far_list_counter(q)], fc.lists_far_sub_cap), far_room - at);
            if (n) TOPO_HIP_TRY(hipMemcpy(far_out + (size_t)at * 5, fc.d_far.as<FarItem>() + (size_t)q * fc.lists_far_sub_cap, (size_t)n * sizeof(FarItem), hipMemcpyDeviceToHost));
            at += n;
        }
    }
    return TOPO_OK;
}

int TerrainRenderer::read_normals(int32_t lat, int32_t lon, uint8_t* out) {
    Tile* t = find(lat, lon);
    if (!t) return fail(TOPO_ERR_NOT_FOUND, "no such tile");
    if (int rc = bind_device()) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(out, t->d_normals, (size_t)tile_w_ * tile_h_ * 4, hipMemcpyDeviceToHost));
    return TOPO_OK;
}

int TerrainRenderer::read_tile_tables(int32_t lat, int32_t lon, float* minmax_out, float* trig_out, double* bounds_out, uint32_t* n_blocks_out) {
    Tile* t = find(lat, lon);
    if (!t) return fail(TOPO_ERR_NOT_FOUND, "no such tile");
    if (int rc = bind_device()) return rc;
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    const uint32_t bxc = (tile_w_ - 1 + kBCX - 1) / kBCX, byc = (tile_h_ - 1 + kBCY - 1) / kBCY;
    const size_t nb = (size_t)bxc * byc;
    if (n_blocks_out) *n_blocks_out = (uint32_t)nb;
    if (minmax_out) TOPO_HIP_TRY(hipMemcpy(minmax_out, t->dev.block_minmax, nb * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (trig_out) TOPO_HIP_TRY(hipMemcpy(trig_out, t->dev.trig_lon, 2 * ((size_t)tile_w_ + tile_h_) * sizeof(float), hipMemcpyDeviceToHost));
    if (bounds_out) TOPO_HIP_TRY(hipMemcpy(bounds_out, t->dev.block_bounds, nb * 18 * sizeof(double), hipMemcpyDeviceToHost));
    return TOPO_OK;
}

// ---- GeoTIFF (fetch_terrain's decode step, background_runner.rs:113-136) ---------------------------------------
int geotiff_transform(const TiffInfo& ti, float rp[2], float mp[2], float ps[2]) {
    // CoordinateTransform::from_geo_tag_data (coordinate_transform.rs:23-57)
    if (ti.has_model_transformation) return TOPO_ERR_UNSUPPORTED;
    if (!ti.has_pixel_scale || !ti.has_tie_points) return TOPO_ERR_UNSUPPORTED;
    if (ti.pixel_scale.size() != 3 || ti.tie_points.size() != 6) return TOPO_ERR_INVALID;
    rp[0] = (float)ti.tie_points[0]; rp[1] = (float)ti.tie_points[1];
    mp[0] = (float)ti.tie_points[3]; mp[1] = (float)ti.tie_points[4];
    ps[0] = (float)ti.pixel_scale[0]; ps[1] = (float)ti.pixel_scale[1];
    return TOPO_OK;
}

// Decodes the first image of the file into a device raster, `heights` (an empty buffer of the caller's).
int TerrainRenderer::geotiff_to_device(const uint8_t* bytes, size_t n, DeviceBuffer& heights, uint32_t* w, uint32_t* h, float rp[2],
                                       float mp[2], float ps[2]) {
    TiffInfo ti;
    std::string e;
    if (int rc = tiff_parse(bytes, n, ti, e)) return fail(rc, "GeoTIFF: " + e);
    if (int rc = geotiff_transform(ti, rp, mp, ps))
        return fail(rc, rc == TOPO_ERR_UNSUPPORTED ? "GeoTIFF: IncorrectGeoTags (ModelPixelScale + ModelTiepoint without ModelTransformation required)"
                                                    : "GeoTIFF: IncorrectGeoTagData (ModelPixelScale needs 3 and ModelTiepoint 6 values)");
    if (int rc = bind_device()) return rc;
    // host: the byte streams of all strips/tiles, decompressed back to back (4-byte aligned: sizes are multiples of 4)
    std::vector<TiffSegDev> segs;
    std::vector<uint32_t> row_seg;
    size_t total = 0;
    for (const TiffSegment& s : ti.segments) {
        TiffSegDev d{};
        d.byte_off = total; d.row0 = (uint32_t)row_seg.size();
        d.x0 = s.x0; d.y0 = s.y0; d.w = s.w; d.h = s.h;
        for (uint32_t r = 0; r < s.h; ++r) row_seg.push_back((uint32_t)segs.size());
        segs.push_back(d);
        total += (size_t)s.w * s.h * 4;
    }
    std::vector<uint8_t> staged(total);
    {   // strips/tiles are independent byte streams: inflate them on a few host threads
        const unsigned hw = std::thread::hardware_concurrency();
        const size_t n_thr = std::min<size_t>(segs.size(), std::min<unsigned>(hw ? hw : 1, 8));
        std::vector<int> rcs(n_thr, TOPO_OK);
        std::vector<std::string> errs(n_thr);
        std::atomic<size_t> next{0};
        auto work = [&](size_t tid) {
            for (size_t k = next++; k < segs.size(); k = next++)
                if (int rc = tiff_segment_bytes(bytes, n, ti, ti.segments[k], staged.data() + segs[k].byte_off, errs[tid])) { rcs[tid] = rc; return; }
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < n_thr; ++t) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
        for (size_t t = 0; t < n_thr; ++t)
            if (rcs[t]) return fail(rcs[t], "GeoTIFF: " + errs[t]);
    }
    DeviceBuffer d_bytes, d_segs, d_rows;
    if (int rc = ensure(stream_, d_bytes, total ? total : 4)) return rc;
    if (int rc = ensure(stream_, d_segs, segs.size() * sizeof(TiffSegDev))) return rc;
    if (int rc = ensure(stream_, d_rows, row_seg.size() * sizeof(uint32_t))) return rc;
    if (int rc = ensure(stream_, heights, (size_t)ti.width * ti.height * sizeof(float))) return rc;
    TOPO_HIP_TRY(hipMemcpyAsync(d_bytes.p, staged.data(), total, hipMemcpyHostToDevice, stream_));
    TOPO_HIP_TRY(hipMemcpyAsync(d_segs.p, segs.data(), segs.size() * sizeof(TiffSegDev), hipMemcpyHostToDevice, stream_));
    TOPO_HIP_TRY(hipMemcpyAsync(d_rows.p, row_seg.data(), row_seg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    launch_tiff_rows(d_bytes.as<uint8_t>(), d_segs.as<const TiffSegDev>(), d_rows.as<const uint32_t>(), (uint32_t)row_seg.size(), heights.as<float>(), ti.width,
                     ti.height, ti.predictor, ti.big_endian, stream_);
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));          // the staging vectors are only borrowed for the call
    *w = ti.width;
    *h = ti.height;
    return TOPO_OK;
}

int TerrainRenderer::geotiff_decode(const uint8_t* bytes, size_t n, float* heights_out, size_t capacity) {
    if (!bytes || !heights_out) return fail(TOPO_ERR_INVALID, "null argument");
    DeviceBuffer d;
    uint32_t w = 0, h = 0;
    float rp[2], mp[2], ps[2];
    if (int rc = geotiff_to_device(bytes, n, d, &w, &h, rp, mp, ps)) return rc;
    if ((size_t)w * h > capacity) return fail(TOPO_ERR_CAPACITY, "heights_out is smaller than the image");
    if (hipMemcpy(heights_out, d.p, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return fail(TOPO_ERR_HIP, "copy of the decoded raster failed");
    return TOPO_OK;
}

int TerrainRenderer::add_terrain_geotiff(int32_t lat, int32_t lon, const uint8_t* bytes, size_t n) {
    if (!bytes) return fail(TOPO_ERR_INVALID, "null argument");
    DeviceBuffer d;
    uint32_t w = 0, h = 0;
    float rp[2], mp[2], ps[2];
    if (int rc = geotiff_to_device(bytes, n, d, &w, &h, rp, mp, ps)) return rc;
    return add_terrain(lat, lon, d.as<const float>(), true, w, h, rp, mp, ps);      // copies device-to-device
}

int TerrainRenderer::probe_sincos(const float* x, float* s, float* c, size_t n) {
    if (int rc = bind_device()) return rc;
    DeviceBuffer dx, ds, dc;
    for (DeviceBuffer* b : {&dx, &ds, &dc})
        if (int rc = ensure(stream_, *b, n * 4)) return rc;
    TOPO_HIP_TRY(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice));
    launch_probe_sincos(dx.as<const float>(), ds.as<float>(), dc.as<float>(), n, stream_);
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(s, ds.p, n * 4, hipMemcpyDeviceToHost));
    TOPO_HIP_TRY(hipMemcpy(c, dc.p, n * 4, hipMemcpyDeviceToHost));
    return TOPO_OK;
}

int TerrainRenderer::probe_div(int32_t kind, const float* x, const float* y, float* out, size_t n) {
    if (kind < 0 || kind > 8 || !x || !y || !out) return fail(TOPO_ERR_INVALID, "probe_div: bad argument");
    if (int rc = bind_device()) return rc;
    DeviceBuffer dx, dy, dq;
    for (DeviceBuffer* b : {&dx, &dy, &dq})
        if (int rc = ensure(stream_, *b, n * 4)) return rc;
    TOPO_HIP_TRY(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice));
    TOPO_HIP_TRY(hipMemcpy(dy.p, y, n * 4, hipMemcpyHostToDevice));
    launch_probe_div(kind, dx.as<const float>(), dy.as<const float>(), dq.as<float>(), n, stream_);
    TOPO_HIP_TRY(hipStreamSynchronize(stream_));
    TOPO_HIP_TRY(hipMemcpy(out, dq.p, n * 4, hipMemcpyDeviceToHost));
    return TOPO_OK;
}

int TerrainRenderer::change_location(float latitude, float longitude, float range_dist, std::vector<std::pair<int32_t, int32_t>>& request,
                                     uint32_t* n_unloaded) {
    std::vector<int32_t> loaded;
    for (const auto& kv : tiles_) { loaded.push_back(kv.second.lat); loaded.push_back(kv.second.lon); }
    std::vector<std::pair<int32_t, int32_t>> unload;
    change_location_plan(latitude, longitude, range_dist, loaded.data(), (uint32_t)(loaded.size() / 2), unload, request);
    for (const auto& u : unload)
        if (int rc = unload_terrain(u.first, u.second)) return rc;
    if (n_unloaded) *n_unloaded = (uint32_t)unload.size();
    return TOPO_OK;
}

}  // namespace topo
