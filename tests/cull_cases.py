"""The scenes of tests/test_cull_cpu.py and tests/test_cull_gpu.py: tiles for the load-time tables, scenes and poses for the cull's
lists, and the poses that put the sideways bulge of a block's equator-side edge on the screen.

Field of view: topo_update accepts any camera_proj (it checks the target size and the post uniforms only), so nothing bounds the
focal length f = H / (2 tan(fov_y / 2)) in pixels, nor f / depth: the bulge poses below reach 6 px per metre at their blocks
(fov_y 0.05 degrees on a 64-row target, 12 km away) and the accepted inputs allow any multiple of that."""
from __future__ import annotations

import math

import numpy as np

import cull_ref as CR
import topo_renderer_amd as T
from scenes import relief
from viewshed_ref import geo_order

W, H = 96, 64      # every frame of these tests


class Tiles:
    """Tiles of one size with explicit transforms: tiles = {(lat, lon): (heights f32 (h, w), (raster_point, model_point, pixel_scale))}."""

    def __init__(self, tiles):
        self.tiles = dict(tiles)
        self.locs = list(self.tiles)
        self.order = geo_order(self.locs)      # rank -> location, the draw order
        self.th, self.tw = next(iter(self.tiles.values()))[0].shape
        self.bxc, self.byc = CR.block_counts(self.tw, self.th)
        self.n_blocks = self.bxc * self.byc
        self._refs = {}

    def load(self, renderer):
        for loc in self.locs:
            renderer.add_terrain(loc[0], loc[1], self.tiles[loc][0], *self.tiles[loc][1])

    def ref(self, loc, blk):
        """The f64 reference of one block, computed once."""
        if (loc, blk) not in self._refs:
            self._refs[(loc, blk)] = CR.BlockRef(self.tiles[loc][0], self.tiles[loc][1], blk)
        return self._refs[(loc, blk)]


def transform(lat, lon, tw, th, cells_per_degree=None):
    """The GeoTIFF tags of a tile whose north-west corner is (lat + 1, lon): one degree across (the default), or with square cells of
    1 / cells_per_degree degrees."""
    sx, sy = (1.0 / tw, 1.0 / th) if cells_per_degree is None else (1.0 / cells_per_degree,) * 2
    return np.float32([0, 0]), np.float32([lon, lat + 1]), np.float32([sx, sy])


def sampled(height_fn, tr, tw, th):
    """height_fn(lat_deg, lon_deg) at the vertices of a tile."""
    lat = np.degrees(CR.lat_rad(tr, np.arange(th)))[:, None]
    lon = np.degrees(CR.lon_rad(tr, np.arange(tw)))[None, :]
    return np.ascontiguousarray(height_fn(lat, lon) + 0.0 * lat + 0.0 * lon, dtype=np.float32)


# ---- table cases: tile shape x placement ----------------------------------------------------------------------------------------------
TABLE_SHAPES = [(24, 24), (61, 16), (62, 17), (244, 31), (245, 31), (480, 31)]      # (columns, rows)
PLACEMENTS = {      # the tile sets of tests/geo_scenes.py's placements, and the 45N 15E quadrant
    "quadrant": [(46, 15), (46, 16), (45, 15), (45, 16)],
    "origin": [(0, -1), (0, 0), (-1, -1), (-1, 0)],
    "antimeridian": [(10, 179), (10, -180), (9, 179), (9, -180)],
}
TABLE_CASES = [(name, tw, th) for name in PLACEMENTS for tw, th in TABLE_SHAPES] + [("void", 245, 31)]
_TABLES = {}


def table_case(name, tw, th):
    """One-degree tiles of tw x th vertices of `relief`; "void": the quadrant's tiles with one block of NaN all over and one NaN in
    another block of the first tile, and a -32767 sentinel and an infinity in the second."""
    key = (name, tw, th)
    if key not in _TABLES:
        locs = PLACEMENTS["quadrant" if name == "void" else name]
        tiles = {}
        for loc in locs:
            tr = transform(loc[0], loc[1], tw, th)
            tiles[loc] = (sampled(relief, tr, tw, th), tr)
        if name == "void":
            a, b = tiles[locs[0]][0], tiles[locs[1]][0]
            a[0:16, 60:121] = np.nan          # block 1 and the columns it shares with blocks 0 and 2
            a[20, 200] = np.nan
            b[3, 7], b[17, 100] = -32767.0, np.inf
        _TABLES[key] = Tiles(tiles)
    return _TABLES[key]


# ---- the tables against the reference ----------------------------------------------------------------------------------------------------
# The radius is the length of a difference of two positions, each a product of the radius and two f64 sin / cos values: a position
# is good to about 2.5 units in its last place (0.93e-9 m at the Earth's radius: one for each sin / cos, half for each product), the
# difference to 5, the length of its three components to 5 sqrt(3) = 8.7 of them, 8.1e-9 m.  (A host evaluation of the same
# expressions with correctly rounded sin / cos lies up to 1.8e-9 m from the long double value.)
RADIUS_TOL = 1e-8



def assert_tables(tiles, read, what):
    """Every block's tables -- read(lat, lon) -> {"minmax": (n, 2) f32, "bounds": 18 n f64} -- against the reference: min / max bit for
    bit, sphere centre to 1e-9 m, corner directions to 1e-14, sagitta to 1e-9 relative, radius and bulge to what their expressions
    allow in f64, and every ideal vertex inside radius - 64."""
    worst = dict(bulge=0.0, centre=0.0, centre_ld=0.0, radius=0.0, corner=0.0, sagitta=0.0, slack=np.inf)
    for loc in tiles.locs:
        t = read(*loc)
        nb = tiles.n_blocks
        assert t["minmax"].shape == (nb, 2), (what, loc)
        b = t["bounds"]
        sphere, dirs, sag, bulge = b[:4 * nb].reshape(nb, 4), b[4 * nb:16 * nb].reshape(nb, 4, 3), b[16 * nb:17 * nb], b[17 * nb:]
        assert bulge.shape == (nb,)
        for blk in range(nb):
            r = tiles.ref(loc, blk)
            want = np.float32([r.hmin, r.hmax])
            assert np.array_equal(t["minmax"][blk].view(np.uint32), want.view(np.uint32)), (what, loc, blk, t["minmax"][blk], want)
            worst["corner"] = max(worst["corner"], float(np.abs(dirs[blk] - r.u).max()))
            assert np.abs(dirs[blk] - r.u).max() <= 1e-14, (what, loc, blk, "corner directions")
            if not (np.isfinite(r.hmin) and np.isfinite(r.hmax)):
                continue      # an infinity in the block, or NaN all over: no sphere to speak of, and the cull never filters on it
            dc = float(np.abs(sphere[blk, :3] - r.centre).max())
            worst["centre_ld"] = max(worst["centre_ld"], float(np.abs(sphere[blk, :3].astype(CR.LD) - r.centre_ld).max()))
            dr = float(abs(CR.LD(sphere[blk, 3]) - r.radius_ld))
            ds = abs(float(sag[blk]) - r.sagitta) / r.sagitta
            worst["centre"], worst["radius"], worst["sagitta"] = max(worst["centre"], dc), max(worst["radius"], dr), max(worst["sagitta"], ds)
            assert dc <= 1e-9, (what, loc, blk, "sphere centre", dc)
            assert dr <= RADIUS_TOL, (what, loc, blk, "sphere radius", dr)
            assert ds <= 1e-9, (what, loc, blk, "sagitta", float(sag[blk]), r.sagitta)
            # the bulge is R |n . m| / |n|, n = a x b the cross product of the f64 unit vectors of a row's two ends: a component of n is
            # a difference of two products of numbers below 1 (three roundings, 2^-52 at the most together), the dot product with m adds
            # three terms' roundings of that size or less, so n . m is good to 8 x 2^-52 absolutely whatever |n| is -- in metres
            # 8 x 2^-52 x R / |a x b|: 4e-6 m for a full block of a 244-column tile, 6e-5 m for a one-cell sliver (and 8 m of vertex
            # noise stand beside the bulge in the margin it feeds)
            sep = min(float(np.linalg.norm(np.cross(r.u[0], r.u[1]))), float(np.linalg.norm(np.cross(r.u[2], r.u[3]))))
            tol = 8.0 * 2.0 ** -52 * (CR.R0 + 9000.0) / sep + 1e-9 * r.bulge
            worst["bulge"] = max(worst["bulge"], abs(float(bulge[blk]) - r.bulge) / tol)
            assert abs(float(bulge[blk]) - r.bulge) <= tol, (what, loc, blk, "bulge", float(bulge[blk]), r.bulge, tol)
            v = r.vertices.reshape(-1, 3)
            v = v[np.isfinite(v).all(axis=1)]
            slack = float(sphere[blk, 3]) - 64.0 - float(np.sqrt(((v - sphere[blk, :3]) ** 2).sum(axis=1)).max())
            worst["slack"] = min(worst["slack"], slack)
            assert slack >= 0.0, (what, loc, blk, "a vertex lies outside radius - 64", slack)
    print(f"{what}: largest deviation centre {worst['centre']:.2e} m ({worst['centre_ld']:.2e} m from the long double value), radius {worst['radius']:.2e} m, corner directions {worst['corner']:.2e}, "
          f"sagitta {worst['sagitta']:.2e} (relative), bulge {worst['bulge']:.2e} of its tolerance; smallest slack of a vertex inside radius - 64: {worst['slack']:.2f} m")


# ---- cameras --------------------------------------------------------------------------------------------------------------------------
def yaw_pitch_towards(eye, direction):
    """The yaw and pitch (radians) with which camera_uniforms looks from `eye` along `direction`: its view direction is
    rot * (cos yaw cos pitch, sin pitch, sin yaw cos pitch), rot the shortest rotation that takes -Y to the eye's up."""
    up = np.asarray(eye, np.float64) / np.linalg.norm(eye)
    frm = np.array([0.0, -1.0, 0.0])
    q = np.append(np.cross(frm, up), 1.0 + frm @ up)
    q /= np.linalg.norm(q)
    b, w = -q[:3], q[3]      # the inverse rotation
    d = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    v = d * (w * w - b @ b) + b * (2.0 * (d @ b)) + np.cross(b, d) * (2.0 * w)
    return math.atan2(v[2], v[0]), math.asin(max(-1.0, min(1.0, v[1])))


def look(eye, direction, fov_deg, lon_deg, lat_deg):
    eye = np.asarray(eye, np.float32)
    yaw, pitch = yaw_pitch_towards(eye.astype(np.float64), direction)
    return T.camera_uniforms(eye, yaw, pitch, math.radians(fov_deg), W, H, lon_deg, lat_deg, 0)


def proj_of(u):
    return np.asarray(u, np.float32)[:16]


def table_pose(tiles):
    """An oblique view over a table case's mosaic: from 4000 m over a vertex of the first tile towards the middle of the last one,
    25 degrees down, 60 degrees of field."""
    a, b = tiles.locs[0], tiles.locs[-1]
    (ha, tra), (hb, trb) = tiles.tiles[a], tiles.tiles[b]
    x, y = tiles.tw // 5, tiles.th // 4
    lon, lat = math.degrees(CR.lon_rad(tra, x)), math.degrees(CR.lat_rad(tra, y))
    eye = T.geometry_transform(float(np.nan_to_num(ha[y, x], nan=1500.0, posinf=1500.0, neginf=1500.0)) + 4000.0, lon, lat)
    aim = (CR.R0 + 1500.0) * CR.direction(CR.lon_rad(trb, tiles.tw // 2), CR.lat_rad(trb, tiles.th // 2))
    up = eye.astype(np.float64) / np.linalg.norm(eye)
    d = aim - eye.astype(np.float64)
    level = d - (d @ up) * up
    level /= np.linalg.norm(level)
    return look(eye, math.cos(math.radians(25.0)) * level - math.sin(math.radians(25.0)) * up, 60.0, lon, lat)


# ---- list scenes: ordinary poses ------------------------------------------------------------------------------------------------------
def ridges(lat, lon):
    """Ridges 400 m high and a few kilometres apart: terrain that hides terrain at the scale of a 0.2 x 0.05 degree tile."""
    return 1500.0 + 400.0 * np.sin(np.radians(9000.0 * lon + 2500.0 * lat)) * np.cos(np.radians(12000.0 * lat)) + 150.0 * np.sin(np.radians(31000.0 * lon))


LIST_SHAPE = (245, 62)      # 5 x 5 blocks: a 4-cell sliver column, a 1-cell-row sliver row, an odd width (k_block_tables' scalar path)
LIST_SPLIT = 5000.0
LIST_SCENES = {"quadrant": [(45, 15), (45, 16)], "origin": [(0, -1), (-1, -1)], "antimeridian": [(10, 179), (10, -180)], "void": [(45, 15), (45, 16)]}
_LISTS = {}


class ListScene:
    def __init__(self, name, tiles, poses):
        self.name, self.tiles, self.poses, self.split = name, tiles, poses, LIST_SPLIT      # poses: [(what, uniforms)]


def list_scene(name):
    """Two tiles of LIST_SHAPE with COP90-sized cells (1/1200 degree: a block's sagitta is 0.3 m, so its blocks can be occlusion-test
    candidates), each at its own degree's north-west corner, seen from three eyes over the first tile: two oblique views from 900
    and 4000 m up and one from below the lowest vertex of the block above the eye.  "void": one NaN vertex in a far block, one block
    NaN all over."""
    if name not in _LISTS:
        tw, th = LIST_SHAPE
        tiles = {}
        for loc in LIST_SCENES[name]:
            tr = transform(loc[0], loc[1], tw, th, cells_per_degree=1200)
            tiles[loc] = (sampled(ridges, tr, tw, th), tr)
        first = LIST_SCENES[name][0]
        hts, tr = tiles[first]
        clean = hts.copy()
        if name == "void":
            hts[47, 200] = np.nan                  # block (3, 3): an ordinary block with one vertex missing
            hts[31:45, 121:180] = np.nan           # the interior of block (2, 2) ...
            hts[30:46, 120:181] = np.nan           # ... and its shared border rows and columns: the block is NaN all over
        ts = Tiles(tiles)
        poses = []
        for what, (x, y), dh, towards, pitch_down, fov in (("oblique 900 m", (8, 6), 900.0, (240, 58), 6.0, 60.0),
                                                         ("oblique 4000 m", (236, 4), 4000.0, (20, 60), 20.0, 50.0),
                                                         ("steep 900 m", (8, 6), 900.0, (240, 58), 22.0, 30.0),
                                                         ("below the surface", (30, 30), None, (230, 35), -8.0, 70.0)):
            lon, lat = math.degrees(CR.lon_rad(tr, x)), math.degrees(CR.lat_rad(tr, y))
            if dh is None:      # 60 m below the lowest vertex of the eye's own block
                blk = (y // CR.BCY) * ts.bxc + x // CR.BCX
                height = float(CR.block_minmax(clean, blk)[0]) - 60.0
            else:
                height = float(clean[y, x]) + dh
            eye = T.geometry_transform(height, lon, lat)
            tx, ty = towards
            aim = (CR.R0 + float(clean[ty, tx])) * CR.direction(CR.lon_rad(tr, tx), CR.lat_rad(tr, ty))
            d = aim - eye.astype(np.float64)
            up = eye.astype(np.float64) / np.linalg.norm(eye)
            d = d / np.linalg.norm(d)
            level = d - (d @ up) * up
            level /= np.linalg.norm(level)
            d = math.cos(math.radians(pitch_down)) * level - math.sin(math.radians(pitch_down)) * up
            poses.append((what, look(eye, d, fov, lon, lat)))
        _LISTS[name] = ListScene(name, ts, poses)
    return _LISTS[name]


# ---- bulge cases ----------------------------------------------------------------------------------------------------------------------
def gentle(lat, lon):
    """A few metres of relief at 3000 m: the slab of a block is then a dozen metres thick."""
    return 3000.0 + 4.0 * np.sin(np.radians(700.0 * lon)) + 3.0 * np.cos(np.radians(900.0 * lat))


# name: (tile latitude, columns of the 1200-row tile, block (bx, by), d beyond the edge's end (m), split (m), fov_y (degrees))
BULGE = {
    "60N 2x": (60, 600, (4, 40), 12000.0, 5000.0, 0.03),
    "70N 3x": (70, 400, (3, 40), 12000.0, 5000.0, 0.05),
    "80N 5x": (80, 240, (2, 40), 12000.0, 5000.0, 0.05),
    "80N square": (80, 1200, (9, 40), 6000.0, 3000.0, 0.008),
    "81S 5x": (-81, 240, (2, 40), 12000.0, 5000.0, 0.05),
}
BULGE_LON = 20
_BULGE = {}


class BulgeCase:
    def __init__(self, name):
        lat, tw, (bx, by), d, split, fov = BULGE[name]
        th = 1200
        tr = transform(lat, BULGE_LON, tw, th)
        self.name, self.split, self.fov, self.loc = name, split, fov, (lat, BULGE_LON)
        self.tiles = Tiles({self.loc: (sampled(gentle, tr, tw, th), tr)})
        self.blk = by * self.tiles.bxc + bx
        self.ref = self.tiles.ref(self.loc, self.blk)
        edge = self.ref.edge_vertices()
        chord = edge[-1] - edge[0]
        chord /= np.linalg.norm(chord)
        eye = np.float32(edge[-1] + d * chord)      # the f32 eye the renderer gets
        self.eye = eye
        x1, y = self.ref.range[1], self.ref.side_row
        self.uniforms = look(eye, edge[-1] - eye.astype(np.float64), fov, math.degrees(CR.lon_rad(tr, x1)), math.degrees(CR.lat_rad(tr, y)))
        self.proj = proj_of(self.uniforms)

    def condition(self):
        """What the reference alone says of the pose: dict(w_near: the smallest view depth of the block's sphere, bulge_m: the edge's
        excursion beyond the slab's equator-side face, box: the unclamped slab-corner box, overshoot_px: how far the edge's vertices
        project beyond it on a side the target does not clamp)."""
        r = self.ref
        m = np.asarray(self.proj, np.float64).reshape(4, 4).T
        wn = np.linalg.norm(m[3, :3])
        w_near = float(m[3, :3] @ r.centre + m[3, 3]) / wn - r.radius
        bulge = CR.excursions(r.edge_vertices(), r.faces())[r.side]
        box, wmin, _ = CR.slab_box(self.proj, W, H, r.corners)
        s = CR.screen(CR.clip_coords(self.proj, r.edge_vertices()), W, H)
        over = overshoot(box, s)
        return dict(w_near=w_near, bulge_m=bulge, box=box, wmin=wmin, overshoot_px=over)


def overshoot(box, s, size=(W, H)):
    """The largest distance (pixels) of one of the screen positions s beyond [x0, x1 + 1] x [y0, y1 + 1] on a side of the box that
    lies inside the target (the others are clamped: whatever lies beyond them is off the target); <= 0: none."""
    x0, x1, y0, y1 = box
    worst = -np.inf
    if x0 > 0:
        worst = max(worst, float((x0 - s[:, 0]).max()))
    if x1 < size[0] - 1:
        worst = max(worst, float((s[:, 0] - (x1 + 1)).max()))
    if y0 > 0:
        worst = max(worst, float((y0 - s[:, 1]).max()))
    if y1 < size[1] - 1:
        worst = max(worst, float((s[:, 1] - (y1 + 1)).max()))
    return worst


def bulge_case(name):
    if name not in _BULGE:
        _BULGE[name] = BulgeCase(name)
    return _BULGE[name]


# ---- the oracle's side: its f32 vertex path and its frame's winners -------------------------------------------------------------------
POST = np.array([W, H, 100.0, 0.0], np.float32)
DROP_PAD = 8
_ORACLES = {}


def oracle_of(orc, key, tiles):
    """One oracle per tile set, loaded once."""
    if key not in _ORACLES:
        o = orc.OracleRenderer(W, H)
        tiles.load(o)
        _ORACLES[key] = o
    return _ORACLES[key]


def probe_block(o, tiles, loc, blk):
    """(n, 4) f32 clip coordinates of the block's vertices by the oracle's own vertex path (vs_main under the uniforms of its last
    update), row by row; vertices with a non-finite height left out."""
    x0, x1, y0, y1 = CR.block_range(tiles.tw, tiles.th, blk)
    hts = tiles.tiles[loc][0]
    out = []
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            if np.isfinite(hts[y, x]):
                out.append(o.vs_main_probe(loc[0], loc[1], x, y)[:4])
    return np.array(out, np.float32).reshape(-1, 4)


def screen_f32(clip):
    """Screen position and depth of f32 clip coordinates, evaluated in f64: ((n, 2), (n,))."""
    c = np.asarray(clip, np.float64)
    return CR.screen(c, W, H), c[:, 2] / c[:, 3]


def winners_by_block(tiles, depth, win):
    """{(rank, blk): (ys, xs, depths)} of an oracle frame's winners (rank * 2 (w - 1)(h - 1) + triangle; triangle >> 1 = cell,
    cell = x (h - 1) + y)."""
    ys, xs = np.nonzero(win != 0xFFFFFFFF)
    ids = win[ys, xs].astype(np.int64)
    tris = 2 * (tiles.tw - 1) * (tiles.th - 1)
    rank, cell = ids // tris, (ids % tris) >> 1
    blk = (cell % (tiles.th - 1)) // CR.BCY * tiles.bxc + (cell // (tiles.th - 1)) // CR.BCX
    out = {}
    for key in set(zip(rank.tolist(), blk.tolist())):
        sel = (rank == key[0]) & (blk == key[1])
        out[key] = (ys[sel], xs[sel], depth[ys[sel], xs[sel]])
    return out


def expected(orc, key, tiles, uniforms, split):
    """What the reference and the oracle's frame predict of a frame's lists, with no device involved: dict(classes: predict(),
    depth / win: the oracle's frame, won: winners_by_block(), must_survive: the far blocks that win a pixel, must_drop: the far blocks
    in whose reference box (the slab-corner box with DROP_PAD more pixels on every side, clamped) every pixel of the oracle's frame is won by a
    near block and nearer than the slab's nearest depth by more than 1e-6 -- the occlusion test has nothing to keep them for, whatever margin of
    a few pixels its own box has)."""
    o = oracle_of(orc, key, tiles)
    o.update(W, H, uniforms, POST)
    depth, win = o.render_winners()
    won = winners_by_block(tiles, depth, win)
    classes = predict(tiles, proj_of(uniforms), split)
    must_survive = {k for k in won if classes.get(k) == "far"}
    must_drop = set()
    # the occlusion test sees the near phase's depths only: a pixel counts as covered where a NEAR block wins it
    near_depth = np.full((H, W), np.inf, np.float32)
    for k, (ys, xs, ds) in won.items():
        if classes.get(k) == "near":
            near_depth[ys, xs] = ds
    for (rank, blk), c in classes.items():
        if c != "far" or (rank, blk) in won:
            continue
        r = tiles.ref(tiles.order[rank], blk)
        (x0, x1, y0, y1), wmin, zc = CR.slab_box(proj_of(uniforms), W, H, r.corners)
        # (a candidate for certain only if the corners' own extent, without any margin, meets the target: a box off the target is dropped by the cull itself)
        on_target = x0 + 2 <= W - 1 and x1 - 2 >= 0 and y0 + 2 <= H - 1 and y1 - 2 >= 0
        x0, x1, y0, y1 = max(x0 - DROP_PAD, 0), min(x1 + DROP_PAD, W - 1), max(y0 - DROP_PAD, 0), min(y1 + DROP_PAD, H - 1)
        if wmin > 1000.0 and on_target and float(near_depth[y0:y1 + 1, x0:x1 + 1].max()) < (zc - 8.0) / wmin - 1e-6:
            must_drop.add((rank, blk))
    return dict(classes=classes, depth=depth, win=win, won=won, must_survive=must_survive, must_drop=must_drop)


# What a list scene must show over its poses, at least, by the reference's prediction: a scene in which one class is empty tests nothing of it.
LIST_MINIMA = dict(near=5, far=5, survivors=5, dropped=2, absent=10)


def predicted_counts(e):
    """Lower bounds of a frame's lists from expected(): the blocks the reference classifies near, the far blocks that win a pixel
    (candidates and survivors for certain), the far blocks hidden behind nearer terrain (candidates, and dropped for certain), the
    blocks the sphere test culls."""
    n = lambda c: sum(1 for v in e["classes"].values() if v == c)
    return dict(near=n("near"), far=len(e["must_survive"]) + len(e["must_drop"]), survivors=len(e["must_survive"]), dropped=len(e["must_drop"]), absent=n("culled"))


# ---- what the reference predicts of a frame's lists -----------------------------------------------------------------------------------
def predict(tiles, proj, split):
    """{(rank, blk): "near" | "far" | "culled"} by the cull's own rules restated on the reference's tables: culled if the block's
    sphere lies wholly outside one of the six clip planes, far if its nearest possible view depth exceeds the split and its sagitta
    is at most 1 m, near otherwise and whenever the block's min / max are not ordered."""
    m = np.asarray(proj, np.float32).astype(np.float64).reshape(4, 4).T
    planes = [m[3] + m[0], m[3] - m[0], m[3] + m[1], m[3] - m[1], m[2], m[3] - m[2]]
    out = {}
    for rank, loc in enumerate(tiles.order):
        for blk in range(tiles.n_blocks):
            r = tiles.ref(loc, blk)
            if not r.ordered:
                out[(rank, blk)] = "near"
                continue
            with np.errstate(invalid="ignore"):      # (an infinity in the block: a sphere of NaN fails every comparison, as in the kernel)
                outside = any(p[:3] @ r.centre + p[3] < -r.radius * np.linalg.norm(p[:3]) for p in planes)
                w_near = (m[3, :3] @ r.centre + m[3, 3]) - r.radius * np.linalg.norm(m[3, :3])
            if outside:
                out[(rank, blk)] = "culled"
                continue
            out[(rank, blk)] = "far" if split > 0 and w_near > split and r.sagitta <= 1.0 else "near"
    return out
