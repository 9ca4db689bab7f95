"""What k_resolve's owned strips rest on, without a GPU (tests/owned_emul.cpp: a g++ build of topo_pipeline.h):

  the index function of the strip records -- k_raster_cover names a record by (region, strip), k_resolve by (view, its block's
  column, the wave's first row): both go through owned_record_index and must name the same record for the same strip, every strip
  that starts inside the target must have one, no two strips may share one, and none may lie outside the table;

  the record route -- resolve_setup at a strip's origin, computed without the table of the normal decode as k_raster_cover computes
  it, then resolve_pixel for every pixel of the strip, against resolve_varyings, bit for bit, for owners of record kind 1, of kind 2
  (doubled area >= 2^52) and of kind 3 (cut by the near plane)."""
import numpy as np
import pytest

import cover_emul as CE
import owned_emul as OE


@pytest.mark.parametrize("W,H", [(128, 72), (200, 150), (2048, 4096)])
@pytest.mark.parametrize("n_views", [1, 2, 8])
def test_producer_and_consumer_name_the_same_record(W, H, n_views):
    prod, prod_xy, cap = OE.producer_strips(W, H, n_views)
    cons, cons_xy = OE.consumer_strips(W, H, n_views)
    # every strip that starts inside the target, once: (W + 63) / 64 columns x (H + 7) / 8 rows per view
    want = {(v, x, y) for v in range(n_views) for x in range(0, W, 64) for y in range(0, H, 8)}
    p = {tuple(int(c) for c in xy): int(i) for xy, i in zip(prod_xy, prod)}
    c = {tuple(int(c) for c in xy): int(i) for xy, i in zip(cons_xy, cons)}
    assert len(p) == len(prod) and len(c) == len(cons), "a strip was named twice"
    assert set(p) == want and set(c) == want, (len(p), len(c), len(want))
    assert p == c, "the producer and the consumer disagree about a strip's record"
    assert len(set(p.values())) == len(p), "two strips share a record"
    assert cap == n_views * ((W + 63) // 64) * ((H + 63) // 64) * 8 and max(p.values()) < cap and min(p.values()) >= 0


def _route_over_one_winner_strips(topo, scene, W, H, pose):
    sc = OE.case_scene(scene)
    u = sc.uniforms(W, H, *pose, 0)
    st = CE.cover_frame(topo, sc, W, H, u, want_keys=True)
    kinds = {}
    for x, y, tri_id in OE.one_winner_strips(st["keys"]):
        r = OE.route(topo, sc, W, H, u, tri_id, x, y)
        assert r["differ"] == 0, (scene, W, H, pose, x, y, tri_id, r)
        assert r["words"][34] == tri_id
        kinds[r["kind"]] = kinds.get(r["kind"], 0) + 1
    return st, kinds


def test_record_route_equals_resolve_varyings_for_every_kind_of_owner(topo):
    """Over every strip with one winner of the emulated frames (whether its region was claimed or not: the route does not care), at
    the strips' own origins, cut by the right and the lower edge: 333 x 200 views 2 (kind 1: 112 strips), 3 and 4 (owners cut by the
    near plane: kind 3), 200 x 150 and 128 x 72, and the plain under the 5 degree lens (kind 2)."""
    seen = {}
    for scene, W, H, pose in [("mesa", 333, 200, CE.POSES_MESA[2]), ("mesa", 333, 200, CE.POSES_MESA[3]), ("mesa", 333, 200, CE.POSES_MESA[4]),
                              ("mesa", 200, 150, CE.POSES_MESA[2]), ("mesa", 128, 72, CE.POSES_MESA[2]), ("giant", 200, 150, OE.CASES["giant_200x150"][3][0][0])]:
        st, kinds = _route_over_one_winner_strips(topo, scene, W, H, pose)
        print(scene, W, H, pose, "claims", st["won"], "one-winner strips by record kind", kinds)
        assert st["won"] > 0 and kinds
        for k, n in kinds.items():
            seen[k] = seen.get(k, 0) + n
    assert set(seen) == {1, 2, 3}, seen
