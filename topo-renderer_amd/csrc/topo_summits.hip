// topo_summits.hip -- the device translation unit of the summit queries (topo_summits_*, topo_summit_snap_*): kernels_summits.h and its
// launchers.  Apart from the other units on purpose: their code comes out as before, whatever is added here.  Compiled with
// -ffp-contract=off, as everything.
#include "kernels_summits.h"

namespace topo {

static_assert(sizeof(SummitRec) == 64 && sizeof(SummitSnapRec) == 48, "summit record layouts");

static unsigned groups_of(uint64_t waves) { return (unsigned)((waves + 3) / 4); }

// One band -- rows [y0, y0 + rows) of tile `rank` -- through the first two stages (kernels_summits.h).  The scratch holds rows * tile_w
// posts and rows * ceil(tile_w / 64) waves (SummitScratch: topo_kernels.h); state[] carries the counts and the running offset.
void launch_summits_band(const RayParams& p, const SummitCall& c, uint32_t rank, uint32_t y0, uint32_t rows, const SummitScratch& x, SummitRec* out, uint32_t capacity,
                         hipStream_t s) {
    if (rows == 0 || p.s.tile_w == 0) return;
    const uint32_t wpr = (p.s.tile_w + 63) / 64, n_waves = rows * wpr, posts = rows * p.s.tile_w;
    const uint32_t item_waves = (posts + 63) / 64;      // (<= n_waves: a row's waves hold at least its posts)
    const unsigned walkers = groups_of(posts) < 4096u ? groups_of(posts) : 4096u;      // grid-stride: a wave per list entry, the count is on the device
    if (posts > x.posts || n_waves > x.waves) return;      // (the caller sized the scratch for its bands)
    hipLaunchKernelGGL(k_summit_candidates, dim3(groups_of(n_waves)), dim3(256), 0, s, p, c.min_isolation, c.min_height, rank, y0, rows, wpr, x.wave_mask, x.wave_count, x.waves);
    hipLaunchKernelGGL(k_summit_scan, dim3(1), dim3(1024), 0, s, x.wave_count, n_waves, (const uint32_t*)nullptr, x.waves, x.state, kSummitStateCandidates, 0u, p.check);
    hipLaunchKernelGGL(k_summit_scatter, dim3(groups_of(n_waves)), dim3(256), 0, s, x.wave_mask, x.wave_count, n_waves, y0, p.s.tile_w, wpr, x.candidates, x.posts, x.waves,
                       p.check);
    hipLaunchKernelGGL(k_summit_reject, dim3(walkers), dim3(256), 0, s, p, c.min_isolation, rank, x.candidates, x.state, x.posts, x.keep);
    hipLaunchKernelGGL(k_summit_flags, dim3(groups_of(item_waves)), dim3(256), 0, s, x.keep, x.state, x.posts, x.wave_mask, x.wave_count, x.waves, p.check);
    hipLaunchKernelGGL(k_summit_scan, dim3(1), dim3(1024), 0, s, x.wave_count, item_waves, x.state + kSummitStateCandidates, x.waves, x.state, kSummitStateSurvivors, 1u, p.check);
    hipLaunchKernelGGL(k_summit_append, dim3(groups_of(item_waves)), dim3(256), 0, s, x.wave_mask, x.wave_count, item_waves, x.state, x.candidates, x.posts, rank, out, capacity,
                       x.waves, p.check);
}

// Behind the last band: the records of the first min(summits, capacity) summits (a wave each, grid-stride: the count is on the device).
void launch_summits_finish(const RayParams& p, const SummitCall& c, const SummitScratch& x, SummitRec* out, uint32_t capacity, hipStream_t s) {
    if (capacity == 0) return;
    const unsigned groups = groups_of(capacity) < 8192u ? groups_of(capacity) : 8192u;
    hipLaunchKernelGGL(k_summit_isolation, dim3(groups), dim3(256), 0, s, p, c.radius, x.state, out, capacity);
}

void launch_summit_snap(const RayParams& p, const double* lonlat, double radius, SummitSnapRec* out, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_summit_snap, dim3(n / 4 + (n % 4 != 0)), dim3(256), 0, s, p, reinterpret_cast<const double2*>(lonlat), radius, out, n);      // a wave per point
}

}  // namespace topo
