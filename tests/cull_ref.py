"""An independent f64 reference of the cull's geometry (numpy, no project code): the vertices of a raster block, the load-time
tables block_bounds_store leaves for it (min/max, bounding sphere, corner directions, sagitta), the flat-faced slab the occlusion
filter builds from them and how far the block's vertices stick out of each of its six faces, and clip / screen coordinates of a view.

A tile is (heights (h, w) f32, (raster_point, model_point, pixel_scale)); vertex (x, y) lies at longitude
(x - raster_x) * scale_x + model_x and latitude (y - raster_y) * -scale_y + model_y degrees (the transform's f32 values, the
arithmetic in f64) and at the ideal position (R0 + height) * (cos lat cos lon, cos lat sin lon, sin lat).  A raster block is 60 x 15
cells = 61 x 16 vertices, clipped at the tile's last column and row; blocks are numbered row-major, by * bx_count + bx."""
from __future__ import annotations

import math

import numpy as np

R0 = 6371000.0
BCX, BCY = 60, 15
RAD = 0.017453292519943295


def block_counts(tw, th):
    return (tw - 1 + BCX - 1) // BCX, (th - 1 + BCY - 1) // BCY


def block_range(tw, th, blk):
    """(x0, x1, y0, y1): the block's first and last vertex column and row (inclusive)."""
    bxc, _ = block_counts(tw, th)
    by, bx = divmod(int(blk), bxc)
    return bx * BCX, min(bx * BCX + BCX, tw - 1), by * BCY, min(by * BCY + BCY, th - 1)


def lon_rad(transform, x):
    rp, mp, ps = (np.asarray(a, np.float32).astype(np.float64) for a in transform)
    return ((np.asarray(x, np.float64) - rp[0]) * ps[0] + mp[0]) * RAD


def lat_rad(transform, y):
    rp, mp, ps = (np.asarray(a, np.float32).astype(np.float64) for a in transform)
    return ((np.asarray(y, np.float64) - rp[1]) * -ps[1] + mp[1]) * RAD


def direction(lon, lat, dtype=np.float64):
    lon, lat = np.broadcast_arrays(np.asarray(lon, dtype), np.asarray(lat, dtype))
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def block_vertices(heights, transform, blk):
    """(rows, columns, 3) f64: the ideal positions of the block's vertices (non-finite heights give non-finite positions)."""
    th, tw = heights.shape
    x0, x1, y0, y1 = block_range(tw, th, blk)
    d = direction(lon_rad(transform, np.arange(x0, x1 + 1))[None, :], lat_rad(transform, np.arange(y0, y1 + 1))[:, None])
    with np.errstate(all="ignore"):
        return (R0 + heights[y0:y1 + 1, x0:x1 + 1].astype(np.float64))[..., None] * d


def block_minmax(heights, blk):
    """The f32 minimum and maximum of the block's heights as a fold from (+inf, -inf) that a NaN leaves alone (fminf / fmaxf):
    the exact min and max wherever the block holds no NaN."""
    th, tw = heights.shape
    x0, x1, y0, y1 = block_range(tw, th, blk)
    v = np.asarray(heights[y0:y1 + 1, x0:x1 + 1], np.float32).ravel()
    return np.fmin.reduce(np.append(v, np.float32(np.inf))), np.fmax.reduce(np.append(v, np.float32(-np.inf)))


# The tables are compared to 1e-9 m, one unit in the last place of a double at the Earth's radius: the angles are the f64 values
# above (plain IEEE operations, the same on every machine), everything from them on -- sin, cos, products, the sphere, the sagitta --
# is evaluated in long double (x86: 64-bit mantissa), so that the reference's own rounding is a thousandth of that.
LD = np.longdouble


def block_corner_dirs(transform, tw, th, blk):
    """(4, 3): the unit directions of the corners, k = (last column ? 1 : 0) + (last row ? 2 : 0); and the centre's direction.
    Long double."""
    x0, x1, y0, y1 = block_range(tw, th, blk)
    lo, la = lon_rad(transform, [x0, x1]), lat_rad(transform, [y0, y1])
    u = np.stack([direction(lo[k & 1], la[k >> 1], LD) for k in range(4)])
    return u, direction(lon_rad(transform, 0.5 * (x0 + x1)), lat_rad(transform, 0.5 * (y0 + y1)), LD)


def block_sagitta(u, uc, hmax):
    """(R0 + max(hmax, 0) + 2) (1 - cos theta_max), theta_max the angle between the centre and its farthest corner."""
    return float((LD(R0) + LD(max(float(hmax), 0.0)) + LD(2)) * (LD(1) - (u * uc).sum(axis=1).min()))


def block_sphere(u, uc, hmin, hmax):
    """(centre (3,), radius), long double: the centre's direction at the middle height; the farthest corner's chord at that height +
    half the height range + 8 m + the 64 m the code adds for the f32 noise of the real vertex path."""
    rm = LD(R0) + LD(0.5) * (LD(float(hmin)) + LD(float(hmax)))
    c = rm * uc
    radius = np.sqrt(((rm * u - c) ** 2).sum(axis=1).max()) + LD(0.5) * (LD(float(hmax)) - LD(float(hmin))) + LD(72)
    return c, radius


def block_bulge(transform, tw, th, blk, hmax, sagitta):
    """How far the block's first or last row (whichever is more) bows out of the plane through the Earth's centre and the row's
    two ends, at the slab's top radius R0 + max(hmax, 0) + 2 + sagitta, metres: the largest distance of 201 points of the row's
    parallel from that plane.  Long double."""
    x0, x1, y0, y1 = block_range(tw, th, blk)
    lon = np.linspace(LD(lon_rad(transform, x0)), LD(lon_rad(transform, x1)), 201)
    worst = LD(0)
    for y in (y0, y1):
        p = direction(lon, np.full(201, LD(lat_rad(transform, y))), LD)
        n = np.cross(p[0], p[-1])
        worst = max(worst, np.abs(p @ n).max() / np.sqrt((n * n).sum()))
    return float((LD(R0) + LD(max(float(hmax), 0.0)) + LD(2) + LD(sagitta)) * worst)


def slab_corners(u, hmin, hmax, sagitta):
    """(8, 3): corner k & 3 at radius R0 + hmin - 1 (k < 4) or R0 + hmax + 2 + sagitta (k >= 4)."""
    lo, hi = R0 + float(hmin) - 1.0, R0 + float(hmax) + 2.0 + float(sagitta)
    return np.concatenate([lo * u, hi * u])


# the slab's faces as corner indices: west and east meridian faces, the faces along the first and the last row's parallel, bottom, top
FACES = {"west": (0, 2, 4, 6), "east": (1, 3, 5, 7), "first_row": (0, 1, 4, 5), "last_row": (2, 3, 6, 7), "bottom": (0, 1, 2, 3), "top": (4, 5, 6, 7)}


def slab_faces(corners):
    """{name: (unit outward normal (3,), offset d, planarity)}: the plane n . p = d through the face's four corners (a least-squares
    fit) with n pointing away from the slab's centroid; planarity = the largest distance of one of the four from it, metres."""
    mid = corners.mean(axis=0)
    out = {}
    for name, idx in FACES.items():
        q = corners[list(idx)]
        c = q.mean(axis=0)
        n = np.linalg.svd(q - c)[2][2]
        if n @ (mid - c) > 0:
            n = -n
        out[name] = (n, float(n @ c), float(np.abs((q - c) @ n).max()))
    return out


def excursions(points, faces):
    """{name: the largest signed distance (metres) of one of the points beyond the face}; negative: all of them inside."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    return {name: float((p @ n - d).max()) for name, (n, d, _) in faces.items()}


def equator_side(transform, tw, th, blk):
    """The name of the slab face along the block's equator-side parallel, and that row of the block."""
    _, _, y0, y1 = block_range(tw, th, blk)
    la = lat_rad(transform, [y0, y1])
    return ("first_row", y0) if abs(la[0]) < abs(la[1]) else ("last_row", y1)


def clip_coords(proj, points):
    """(n, 4) f64 clip coordinates of (n, 3) points under the column-major 4 x 4 camera_proj (its f32 values, the arithmetic in f64)."""
    m = np.asarray(proj, np.float32).astype(np.float64).reshape(4, 4).T
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return p @ m[:, :3].T + m[:, 3]


def inside_clip(clip):
    """Which of the clip coordinates lie inside the clip volume: |x| <= w, |y| <= w, 0 <= z <= w."""
    x, y, z, w = clip[:, 0], clip[:, 1], clip[:, 2], clip[:, 3]
    return (np.abs(x) <= w) & (np.abs(y) <= w) & (z >= 0) & (z <= w)


def screen(clip, W, H):
    """(n, 2) screen positions in pixels: x right, y down, pixel (i, j) covering [i, i + 1) x [j, j + 1)."""
    with np.errstate(all="ignore"):
        return np.stack([(clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * W, (0.5 - clip[:, 1] / clip[:, 3] * 0.5) * H], axis=-1)


def slab_box(proj, W, H, corners):
    """The far box as the cull's comment describes it, before clamping: (x0, x1, y0, y1) = floor / ceil of the eight projected slab
    corners' extent, 2 px outward; and the smallest w of the eight with the z_clip there."""
    c = clip_coords(proj, corners)
    s = screen(c, W, H)
    k = int(np.argmin(c[:, 3]))
    return (math.floor(s[:, 0].min()) - 2, math.ceil(s[:, 0].max()) + 2, math.floor(s[:, 1].min()) - 2, math.ceil(s[:, 1].max()) + 2), float(c[k, 3]), float(c[k, 2])


def focal_px(proj, W, H):
    """(fx, fy): pixels per unit of tangent, from the lengths of camera_proj's x and y rows over its w row's."""
    m = np.asarray(proj, np.float32).astype(np.float64).reshape(4, 4).T
    wn = np.linalg.norm(m[3, :3])
    return 0.5 * W * np.linalg.norm(m[0, :3]) / wn, 0.5 * H * np.linalg.norm(m[1, :3]) / wn


class BlockRef:
    """Everything above for one block of one tile."""

    def __init__(self, heights, transform, blk):
        th, tw = heights.shape
        self.blk, self.range = int(blk), block_range(tw, th, blk)
        self.vertices = block_vertices(heights, transform, blk)
        self.hmin, self.hmax = block_minmax(heights, blk)
        x0, x1, y0, y1 = self.range
        self.finite = bool(np.isfinite(heights[y0:y1 + 1, x0:x1 + 1]).all())
        u, uc = block_corner_dirs(transform, tw, th, blk)      # long double, for the tables; rounded to f64 for everything else
        self.u, self.uc = u.astype(np.float64), uc.astype(np.float64)
        self.ordered = bool(self.hmin <= self.hmax)
        if self.ordered:
            with np.errstate(all="ignore"):
                self.sagitta = block_sagitta(u, uc, self.hmax)
                self.bulge = block_bulge(transform, tw, th, blk, self.hmax, self.sagitta)
                self.centre_ld, self.radius_ld = block_sphere(u, uc, self.hmin, self.hmax)
                self.radius = float(self.radius_ld)
                # the centre in f64, as R * cos lat * cos lon from left to right: what the tables are held to 1e-9 m against (a
                # double at the Earth's radius has 0.93e-9 m in its last place, and the long double value lies up to 1.2e-9 m from
                # a rounded f64 evaluation, whoever makes it)
                rm = R0 + 0.5 * (float(self.hmin) + float(self.hmax))
                lo, la = lon_rad(transform, 0.5 * (x0 + x1)), lat_rad(transform, 0.5 * (y0 + y1))
                self.centre = np.array([rm * np.cos(la) * np.cos(lo), rm * np.cos(la) * np.sin(lo), rm * np.sin(la)])
                self.corners = slab_corners(self.u, self.hmin, self.hmax, self.sagitta)
        self.side, self.side_row = equator_side(transform, tw, th, blk)

    def faces(self):
        return slab_faces(self.corners)

    def edge_vertices(self):
        """The vertices of the block's equator-side row."""
        return self.vertices[self.side_row - self.range[2]]
