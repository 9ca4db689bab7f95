// topo_visibility.h -- what an observer sees (topo_visibility_*): the rule, and the two steps k_visibility_grid / k_visibility_list
// take for every target.
//
// It adds no geometry of its own.  A point (lon, lat) is found on the drawn terrain exactly as surface_lookup finds it
// (topo_surface.h: the largest t, then the lower tile rank, then the lower triangle index), and a sight line is tested exactly as the
// sunlit layer's shadow ray is (topo_los.h: los_cast<true>, any hit for kSunTMin <= t <= t_max, the origin's own triangle left out).
//
// Observer.  (lon, lat, height, flags): u = surface_direction(lon, lat); flags & kObserverAboveTerrain: base = the t of
// surface_lookup under u, else base = 0 (the height is measured from the sphere R0); O = ((R0 + base) + height) u.  An observer is
// UNUSABLE when the point is not valid (surface_point_valid), the height is not finite, or the flag is set and no terrain lies
// under the point: every target of an unusable observer is kVisNoObserver.
//
// Target.  (lon, lat) and the call's height h (0 <= h <= 1e5, checked by the host).  An invalid point or one without terrain is
// kVisNone; otherwise T = ((R0 + t) + h) u with t, rank, tri from surface_lookup.
//
// Class.  D = O - T, L = |D|, d = D / L.
//   1  !(L > 2e-3): the observer sits at the target: kVisVisible.
//   2  only for h == 0: N = (v1 - v0) x (v2 - v0) of the winning triangle, turned to the side of u; !(N . D > 0): kVisAway -- the
//      ground itself faces away from the observer.
//   3  the ray from T along d, kSunTMin <= t <= L, any hit.  h == 0: the target's own triangle does not count, as in los_sunlit;
//      h > 0: every triangle counts (a mast on a back slope can be hidden by its own slope).  A hit: kVisHidden; none: kVisVisible.
// "Is there any hit" is a function of the ray and the tile set, not of the traversal: a lane per target (los_cast<true>), a wave per
// ray (kernels_visibility.h) and the loop over every triangle (visibility_class<true>, the emulation's) give the same bytes.
//
// Pure functions (TOPO_HD), as topo_surface.h: the kernels call them for every target, and tests/visibility_emul.cpp runs the same
// code under g++.
#pragma once

#include "topo_surface.h"

namespace topo {

constexpr uint8_t kVisNone = 0, kVisVisible = 1, kVisAway = 2, kVisHidden = 3, kVisNoObserver = 4;      // (the first four = kSun*)
constexpr uint8_t kVisCast = 0xFF;                  // visibility_target: not settled yet, the ray decides
constexpr uint32_t kObserverAboveTerrain = 1u;
constexpr uint32_t kVisMaxObservers = 64;
constexpr double kVisMinRange = 2.0e-3;             // metres: closer than this the observer sits at the target
constexpr double kVisMaxTargetHeight = 1.0e5;

struct VisObserver {       // = topo_observer (32 bytes)
    double lon_deg, lat_deg, height_m;
    uint32_t flags, _reserved;
};

struct VisEye {            // a resolved observer (32 bytes): O, and whether it can be used
    double p[3];
    uint32_t usable, _pad;
};

static_assert(kVisNone == kSunNone && kVisVisible == kSunLit && kVisAway == kSunAway && kVisHidden == kSunShadow, "the classes mirror the sunlit layer's");

// kAll: every triangle instead of the lookup / the traversal (the emulation's brute force; never on the device).
template <bool kAll, class Check>
TOPO_HD void visibility_surface(const LosScene& S, const double u[3], SurfaceHit& best, Check&& chk) {
    if constexpr (kAll) surface_all(S, u, best, chk);
    else surface_lookup(S, u, best, chk);
}

// The observer's point (header comment: observer).
template <bool kAll, class Check>
TOPO_HD void visibility_observer(const LosScene& S, const VisObserver& ob, VisEye& eye, Check&& chk) {
    eye = VisEye{{0.0, 0.0, 0.0}, 0u, 0u};
    if (!surface_point_valid(ob.lon_deg, ob.lat_deg) || !ground_finite(ob.height_m)) return;
    double u[3];
    surface_direction(ob.lon_deg, ob.lat_deg, u);
    double base = 0.0;
    if (ob.flags & kObserverAboveTerrain) {
        SurfaceHit best;
        visibility_surface<kAll>(S, u, best, chk);
        if (!best.hit) return;
        base = best.t;
    }
    const double r = (kGroundR0 + base) + ob.height_m;
#pragma unroll
    for (int k = 0; k < 3; ++k) eye.p[k] = r * u[k];
    eye.usable = 1u;
}

// N . D of triangle `tri` of tile `rank`, N = (v1 - v0) x (v2 - v0) turned to the side of u; false: the index check failed.
template <class Check>
TOPO_HD bool visibility_facing(const LosScene& S, uint32_t rank, uint32_t tri, const double u[3], const double D[3], double& nd, Check&& chk) {
    nd = 0.0;
    uint32_t vx[3], vy[3];
    triangle_vertices(tri, S.tile_h - 1, vx, vy);
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    bool ok = rank < S.n_tiles;
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && vx[m] < S.tile_w && vy[m] < S.tile_h && tab + 2 * ((size_t)S.tile_w + vy[m]) + 1 < S.trig_doubles;
    if (!(chk(ok, ((uint64_t)rank << 32) | tri) && ok)) return false;
    const auto hts = TOPO_GLOBAL_F32(S.tiles[rank].heights);
    double p[3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const size_t lo = tab + 2 * (size_t)vx[m], la = tab + 2 * ((size_t)S.tile_w + vy[m]);
        ground_vertex_from(hts[(size_t)vy[m] * S.tile_w + vx[m]], S.trig[lo], S.trig[lo + 1], S.trig[la], S.trig[la + 1], p[m]);
    }
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nu = n[0] * u[0] + n[1] * u[1] + n[2] * u[2];
    nd = n[0] * D[0] + n[1] * D[1] + n[2] * D[2];
    if (nu < 0.0) nd = -nd;
    return true;
}

// Steps 1 and 2 of a target (lon, lat) at height h seen from `eye`: its class, or kVisCast with the ray of step 3 in r and the
// triangle that does not count in (skip_rank, skip_tri) (kLosNoTri: none).
template <bool kAll, class Check>
TOPO_HD uint8_t visibility_target(const LosScene& S, const VisEye& eye, double lon_deg, double lat_deg, double h, LosRay& r, uint32_t& skip_rank, uint32_t& skip_tri,
                                  Check&& chk) {
    skip_rank = skip_tri = kLosNoTri;
    if (!eye.usable) return kVisNoObserver;
    if (!surface_point_valid(lon_deg, lat_deg)) return kVisNone;
    double u[3];
    surface_direction(lon_deg, lat_deg, u);
    SurfaceHit best;
    visibility_surface<kAll>(S, u, best, chk);
    // (the rank is tested in the product build too: what it indexes is a table)
    if (!best.hit || !(chk(best.rank < S.n_tiles, best.rank) && best.rank < S.n_tiles)) return kVisNone;
    const double rad = (kGroundR0 + best.t) + h;
    double D[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = rad * u[k];
        D[k] = eye.p[k] - r.o[k];
    }
    const double L = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
    if (!(L > kVisMinRange)) return kVisVisible;
    if (h == 0.0) {
        double nd;
        if (!visibility_facing(S, best.rank, best.tri, u, D, nd, chk)) return kVisNone;
        if (!(nd > 0.0)) return kVisAway;
        skip_rank = best.rank;
        skip_tri = best.tri;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) r.d[k] = D[k] / L;
    r.tmin = kSunTMin;
    r.tmax = L;
    return kVisCast;
}

// The class of a target: steps 1 to 3, a lane's work from end to end.
template <bool kAll, class Check>
TOPO_HD uint8_t visibility_class(const LosScene& S, const VisEye& eye, double lon_deg, double lat_deg, double h, Check&& chk) {
    LosRay r;
    uint32_t skip_rank, skip_tri;
    const uint8_t c = visibility_target<kAll>(S, eye, lon_deg, lat_deg, h, r, skip_rank, skip_tri, chk);
    if (c != kVisCast) return c;
    LosHit hit;
    if constexpr (kAll) los_cast_all<true>(S, r, skip_rank, skip_tri, hit, chk);
    else los_cast<true>(S, r, skip_rank, skip_tri, hit, chk);
    return hit.hit ? kVisHidden : kVisVisible;
}

}  // namespace topo
