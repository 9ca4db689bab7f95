"""An independent numpy f64 restatement of the summit rule (include/topo_hip.h, csrc/topo_summits.h) for tests/test_summits_*.py.

Nothing of the product's search is used: a post's longitude and latitude come from the tile transform, distances from those by the
haversine chord 2 R0 sqrt(sin^2(dlat / 2) + cos lat_a cos lat_b sin^2(dlon / 2)) -- not from unit vectors or trig tables --, and the
posts to compare with are found by sorting the latitudes: the angular distance of two points is at least the difference of their
latitudes, so only the posts of a latitude band can lie in range.  Whatever a 1e-3 m change of a distance could flip is marked
ambiguous: membership (an isolation within TOL of min_isolation_m, or a deciding post within TOL of radius_m), the isolation value
(the nearest dominator within TOL of radius_m) and the identity of the nearest dominator (a runner-up within TOL)."""
from __future__ import annotations

import numpy as np

R0 = 6371000.0
TOL = 1e-3
FOUND, NONE, INVALID = 1, 0, -1
REC = np.dtype([("rank", "<u4"), ("idx", "<u4"), ("height_m", "<f4"), ("isolation_m", "<f8"), ("has_higher", "?"), ("higher_rank", "<u4"), ("higher_idx", "<u4"),
                ("member", "?"), ("member_ambiguous", "?"), ("isolation_ambiguous", "?"), ("higher_ambiguous", "?")])
SNAP = np.dtype([("status", "<i4"), ("rank", "<u4"), ("idx", "<u4"), ("height_m", "<f4"), ("distance_m", "<f8"), ("ambiguous", "?")])


def chord(lat_a, lon_a, lat_b, lon_b):
    """Radians in, metres out."""
    s = np.sin(0.5 * (lat_a - lat_b)) ** 2 + np.cos(lat_a) * np.cos(lat_b) * np.sin(0.5 * (lon_a - lon_b)) ** 2
    return 2.0 * R0 * np.sqrt(s)


def band_angle(radius):
    """The angle (radians) the chord `radius` spans, and a little."""
    return 2.0 * np.arcsin(min(1.0, (radius + 1.0) / (2.0 * R0))) + 1e-9


class Posts:
    """Every post of the tiles [(heights (h, w) f32, raster_point, model_point, pixel_scale)], flattened in tile order."""

    def __init__(self, tiles):
        lon, lat, hts, ok = [], [], [], []
        for hgt, rp, mp, ps in tiles:
            hgt = np.asarray(hgt, np.float32)
            rp, mp, ps = (np.asarray(a, np.float32).astype(np.float64) for a in (rp, mp, ps))
            th, tw = hgt.shape
            lo = (np.arange(tw, dtype=np.float64) - rp[0]) * ps[0] + mp[0]
            la = (np.arange(th, dtype=np.float64) - rp[1]) * -ps[1] + mp[1]
            tile_ok = bool(np.isfinite(ps).all() and (ps != 0).all())
            h64 = hgt.astype(np.float64)
            with np.errstate(invalid="ignore"):
                ex = np.isfinite(h64) & (h64 < 1e9) & (h64 > -R0) & tile_ok
            lon.append(np.broadcast_to(lo[None, :], hgt.shape).ravel())
            lat.append(np.broadcast_to(la[:, None], hgt.shape).ravel())
            hts.append(hgt.ravel())
            ok.append(ex.ravel())
        self.shape = np.asarray(tiles[0][0]).shape
        self.per_tile = self.shape[0] * self.shape[1]
        self.lon_deg, self.lat_deg = np.concatenate(lon), np.concatenate(lat)
        self.lon, self.lat = np.radians(self.lon_deg), np.radians(self.lat_deg)
        self.h = np.concatenate(hts)
        self.exists = np.concatenate(ok)
        self.key = np.arange(len(self.h), dtype=np.int64)      # rank * w * h + index: the order of the tie-break
        e = np.nonzero(self.exists)[0]
        self.sorted = e[np.argsort(self.lat[e], kind="stable")]      # the existing posts by latitude
        self.sorted_lat = self.lat[self.sorted]

    def band(self, lat_lo, lat_hi):
        a, b = np.searchsorted(self.sorted_lat, lat_lo, "left"), np.searchsorted(self.sorted_lat, lat_hi, "right")
        return self.sorted[a:b]

    def neighbour_certainly_nearer(self, limit):
        """Per post: an in-tile 8-neighbour exists, dominates it and lies nearer than `limit`."""
        th, tw = self.shape
        out = np.zeros(len(self.h), bool)
        n_tiles = len(self.h) // self.per_tile
        h = self.h.reshape(n_tiles, th, tw)
        ex, la, lo, key = (a.reshape(n_tiles, th, tw) for a in (self.exists, self.lat, self.lon, self.key))
        res = out.reshape(n_tiles, th, tw)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                ys, yd = slice(max(dy, 0), th + min(dy, 0)), slice(max(-dy, 0), th + min(-dy, 0))      # neighbour rows, own rows
                xs, xd = slice(max(dx, 0), tw + min(dx, 0)), slice(max(-dx, 0), tw + min(-dx, 0))
                hq, hp = h[:, ys, xs], h[:, yd, xd]
                with np.errstate(invalid="ignore"):
                    dom = ex[:, ys, xs] & ((hq > hp) | ((hq == hp) & (key[:, ys, xs] < key[:, yd, xd])))
                d = chord(la[:, ys, xs], lo[:, ys, xs], la[:, yd, xd], lo[:, yd, xd])
                res[:, yd, xd] |= dom & (d < limit)
        return out


def summits(posts: Posts, radius, min_isolation, min_height):
    """REC records, in tile order, of every post that exists, is high enough and is not certainly dominated by a neighbour nearer than
    min_isolation - TOL (those are certainly no summits)."""
    with np.errstate(invalid="ignore"):
        cand = posts.exists & (posts.h >= np.float32(min_height))
    cand &= ~posts.neighbour_certainly_nearer(min_isolation - TOL)
    ids = np.nonzero(cand)[0]
    out = np.zeros(len(ids), REC)
    out["rank"], out["idx"], out["height_m"] = ids // posts.per_tile, ids % posts.per_tile, posts.h[ids]
    theta = band_angle(radius)
    order = np.argsort(posts.lat[ids], kind="stable")
    at = 0
    while at < len(order):
        first = ids[order[at]]
        band = posts.band(posts.lat[first] - theta, posts.lat[first] + theta + 2e-4)      # (the chunk spans at most 2e-4 rad of latitude)
        n = max(1, int(2_000_000 // max(1, len(band))))
        sel = order[at:at + n]
        sel = sel[posts.lat[ids[sel]] <= posts.lat[first] + 2e-4]
        at += len(sel)
        p = ids[sel]
        D = chord(posts.lat[p][:, None], posts.lon[p][:, None], posts.lat[band][None, :], posts.lon[band][None, :])
        hq, hp = posts.h[band][None, :], posts.h[p][:, None]
        dom = (hq > hp) | ((hq == hp) & (posts.key[band][None, :] < posts.key[p][:, None]))
        inf = np.inf
        d_nom = np.where(dom & (D <= radius), D, inf)
        d_loose = np.where(dom & (D <= radius + TOL), D, inf).min(axis=1) if len(band) else np.full(len(p), inf)
        d_strict = np.where(dom & (D <= radius - TOL), D, inf).min(axis=1) if len(band) else np.full(len(p), inf)
        iso = d_nom.min(axis=1) if len(band) else np.full(len(p), inf)
        has = np.isfinite(iso)
        exact = d_nom == iso[:, None]
        win = np.where(exact, posts.key[band][None, :], np.iinfo(np.int64).max).argmin(axis=1) if len(band) else np.zeros(len(p), np.int64)
        winner = band[win] if len(band) else np.zeros(len(p), np.int64)
        close = (d_nom <= iso[:, None] + TOL).sum(axis=1) if len(band) else np.zeros(len(p), np.int64)
        r = out[sel]
        r["isolation_m"], r["has_higher"] = iso, has
        r["higher_rank"], r["higher_idx"] = np.where(has, winner // posts.per_tile, 0), np.where(has, winner % posts.per_tile, 0)
        r["member"] = iso >= min_isolation
        certain_no, certain_yes = d_strict + TOL < min_isolation, d_loose - TOL >= min_isolation
        r["member_ambiguous"] = ~(certain_no | certain_yes)
        r["isolation_ambiguous"] = d_loose != d_strict
        r["higher_ambiguous"] = has & (close > 1)
        out[sel] = r
    return out


def snap(posts: Posts, lonlat, radius):
    """SNAP records of (n, 2) points in degrees."""
    pts = np.asarray(lonlat, np.float64).reshape(-1, 2)
    out = np.zeros(len(pts), SNAP)
    theta = band_angle(radius)
    for i, (lon_deg, lat_deg) in enumerate(pts):
        if not (np.isfinite(lon_deg) and abs(lat_deg) <= 90.0):
            out[i]["status"] = INVALID
            continue
        lon, lat = np.radians(lon_deg), np.radians(lat_deg)
        band = posts.band(lat - theta, lat + theta)
        D = chord(lat, lon, posts.lat[band], posts.lon[band])
        h = posts.h[band]
        near = D <= radius + TOL
        band, D, h = band[near], D[near], h[near]
        nominal = D <= radius
        if not nominal.any():
            out[i]["status"], out[i]["ambiguous"] = NONE, bool(len(band))
            continue
        top = h[nominal].max()
        best = np.lexsort((posts.key[band], D, -h.astype(np.float64), ~nominal))[0]
        out[i]["status"], out[i]["rank"], out[i]["idx"] = FOUND, band[best] // posts.per_tile, band[best] % posts.per_tile
        out[i]["height_m"], out[i]["distance_m"] = h[best], D[best]
        border = np.abs(D - radius) <= TOL
        apart = (posts.lon[band] != posts.lon[band[best]]) | (posts.lat[band] != posts.lat[band[best]])      # (a duplicate of the winner is decided by its rank)
        twins = nominal & (h == top) & (D <= D[best] + TOL) & apart
        out[i]["ambiguous"] = bool((border & (h >= top)).any() or twins.any())
    return out
