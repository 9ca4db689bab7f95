// topo_sun.h -- a day of sun and shadow over points of the drawn terrain (topo_sun_exposure_*): the rule, and the steps
// k_sun_exposure_grid / k_sun_exposure_list take for every target and every sun.
//
// It adds no geometry of its own.  A point (lon, lat) is found on the drawn terrain exactly as a visibility target with h == 0 is
// (topo_visibility.h: surface_lookup, then the triangle's normal turned to the side of u), and the shadow ray is tested exactly as
// the sunlit layer's is (topo_los.h: los_cast<true>, any hit for kSunTMin <= t <= kSunTMax, the target's own triangle left out).
//
// Suns.  Up to kSunMaxSuns per call, each a unit direction s TOWARDS the sun -- one ECEF direction for the whole call: the sun is at
// infinity -- and a weight (finite, >= 0; normalised and checked by the host).
//
// Target.  An invalid point or one without terrain is NONE; otherwise t, rank, tri from surface_lookup, T = (R0 + t) u and
// N = (v1 - v0) x (v2 - v0) of that triangle, turned to the side of u.
//
// Class of (target, sun s), in this order:
//   1  !(u . s > 0): kSunNight -- the sun is on or below the point's own horizontal plane.  The sphere is not geometry and a mosaic is
//      finite: without this step a set sun would light every slope near the mosaic's edge.  The DIP of the horizon is ignored: a
//      point h above the sphere sees the sun down to about -sqrt(2 h / R0) (1.8 degrees at 3000 m), and such a sun is night here.
//   2  !(N . s > 0): kSunAway -- the ground itself faces away from the sun.
//   3  the ray from T along s, kSunTMin <= t <= kSunTMax, any hit, the target's own triangle left out.  A hit: kSunShadow; none: kSunLit.
// Per target: bit k of `lit` is set iff sun k is LIT, bit k of `shadow` iff it is SHADOW; exposure is the sum, in ascending k over the
// LIT suns, of (weight_k * (N . s_k)) / |N| -- formed in f64, rounded once to f32; 0 for terrain never lit, a quiet NaN for NONE.
// The class is a function of the target, the sun and the tile set: not of the other suns of the call, not of the traversal -- a lane
// per target (los_cast<true>), a wave per ray (kernels_sun.h) and the loop over every triangle (the emulation's) give the same bits.
//
// Pure functions (TOPO_HD), as topo_visibility.h: the kernels call them for every target, and tests/sun_emul.cpp runs the same code
// under g++.
#pragma once

#include "topo_visibility.h"

namespace topo {

constexpr uint8_t kSunNight = 4;                    // (after kSunNone .. kSunShadow: topo_los.h)
constexpr uint8_t kSunCast = 0xFF;                  // sun_settle: not settled yet, the ray decides
constexpr uint32_t kSunMaxSuns = 64;

struct SunDir {            // = topo_sun (32 bytes), dir normalised
    double d[3], weight;
};

struct SunTarget {         // a target, looked up once for all the suns of a call
    double T[3], u[3], N[3];      // N turned to the side of u
    double n_len;                 // |N|
    uint32_t rank, tri;
    bool terrain;                 // false: NONE, and nothing else is set
};

// N = (v1 - v0) x (v2 - v0) of triangle `tri` of tile `rank`, turned to the side of u (visibility_facing's arithmetic: N . D here is
// its nd, bit for bit); false: the index check failed.
template <class Check>
TOPO_HD bool sun_normal(const LosScene& S, uint32_t rank, uint32_t tri, const double u[3], double N[3], Check&& chk) {
    N[0] = N[1] = N[2] = 0.0;
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
    const bool flip = n[0] * u[0] + n[1] * u[1] + n[2] * u[2] < 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) N[k] = flip ? -n[k] : n[k];
    return true;
}

// The target at (lon, lat) (header comment: target).  kAll: every triangle instead of the lookup (the emulation's brute force).
template <bool kAll, class Check>
TOPO_HD void sun_target(const LosScene& S, double lon_deg, double lat_deg, SunTarget& g, Check&& chk) {
    g = SunTarget{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, kLosNoTri, kLosNoTri, false};
    if (!surface_point_valid(lon_deg, lat_deg)) return;
    double u[3];
    surface_direction(lon_deg, lat_deg, u);
    SurfaceHit best;
    visibility_surface<kAll>(S, u, best, chk);
    // (the rank is tested in the product build too: what it indexes is a table)
    if (!best.hit || !(chk(best.rank < S.n_tiles, best.rank) && best.rank < S.n_tiles)) return;
    if (!sun_normal(S, best.rank, best.tri, u, g.N, chk)) return;
    const double rad = kGroundR0 + best.t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.u[k] = u[k];
        g.T[k] = rad * u[k];
    }
    g.n_len = sqrt(g.N[0] * g.N[0] + g.N[1] * g.N[1] + g.N[2] * g.N[2]);
    g.rank = best.rank;
    g.tri = best.tri;
    g.terrain = true;
}

// Steps 1 and 2 of a terrain target under the sun s: kSunNight, kSunAway, or kSunCast with N . s in ns -- the ray of step 3 decides.
TOPO_HD uint8_t sun_settle(const SunTarget& g, const double s[3], double& ns) {
    ns = g.N[0] * s[0] + g.N[1] * s[1] + g.N[2] * s[2];
    const double us = g.u[0] * s[0] + g.u[1] * s[1] + g.u[2] * s[2];
    if (!(us > 0.0)) return kSunNight;
    if (!(ns > 0.0)) return kSunAway;
    return kSunCast;
}

// The ray of step 3.
TOPO_HD LosRay sun_ray(const SunTarget& g, const double s[3]) { return LosRay{{g.T[0], g.T[1], g.T[2]}, {s[0], s[1], s[2]}, kSunTMin, kSunTMax}; }

// A LIT sun's share of the exposure.
TOPO_HD double sun_term(const SunTarget& g, double weight, double ns) { return (weight * ns) / g.n_len; }

// The class of (target, sun): steps 1 to 3, a lane's work from end to end; ns as sun_settle leaves it.
template <bool kAll, class Check>
TOPO_HD uint8_t sun_class(const LosScene& S, const SunTarget& g, const double s[3], double& ns, Check&& chk) {
    ns = 0.0;
    if (!g.terrain) return kSunNone;
    const uint8_t c = sun_settle(g, s, ns);
    if (c != kSunCast) return c;
    const LosRay r = sun_ray(g, s);
    LosHit hit;
    if constexpr (kAll) los_cast_all<true>(S, r, g.rank, g.tri, hit, chk);
    else los_cast<true>(S, r, g.rank, g.tri, hit, chk);
    return hit.hit ? kSunShadow : kSunLit;
}

// What a target's answers gather in: the two masks and the f64 sum.
struct SunSums {
    uint64_t lit, shadow;
    double exposure;
};

TOPO_HD void sun_take(SunSums& a, const SunTarget& g, uint32_t k, uint8_t cls, double weight, double ns) {
    const uint64_t bit = 1ull << k;
    if (cls == kSunLit) {
        a.lit |= bit;
        a.exposure += sun_term(g, weight, ns);
    } else if (cls == kSunShadow) {
        a.shadow |= bit;
    }
}

// The exposure as it is stored: the f64 sum rounded once; a quiet NaN for NONE.
TOPO_HD float sun_exposure_f32(const SunTarget& g, const SunSums& a) { return g.terrain ? (float)a.exposure : __builtin_nanf(""); }

}  // namespace topo
