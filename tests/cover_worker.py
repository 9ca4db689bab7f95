"""Child process of tests/test_cover_gpu.py: renders the scenes of cover_emul.CASES with the covered-region path as the environment
sets it (TOPO_COVER is read once per process), and writes the frames, the counters and the hook's statistics to the .npz named on
the command line."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_path):
    import torch
    import topo_renderer_amd as T
    import cover_emul as CE

    arrays, meta = {}, {}

    def submit(r, views, W, H):
        n = len(views)
        rgba = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda")
        depth = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()      # (the renderer runs on streams of its own)
        r.render_views_device(views, W, H, rgba.data_ptr(), H * W * 4, W * 4, depth.data_ptr(), H * W * 4, W * 4)
        return rgba, depth

    def keep(name, r, rgba, depth):
        arrays[name + "/rgba"], arrays[name + "/depth"] = rgba.cpu().numpy(), depth.cpu().numpy()
        meta[name] = {"counters": r.counters(), "cover": r.debug_cover_stats(), "status": r.frame_status()}

    renderers = {}
    for case, (scene, W, H, subs) in CE.CASES.items():
        sc = CE.case_scene(scene)
        if scene not in renderers:
            renderers[scene] = T.TerrainRenderer(W, H)
            sc.load(renderers[scene])
        r = renderers[scene]
        for i, sub in enumerate(subs):
            rgba, depth = submit(r, [sc.uniforms(W, H, *pose, 0) for pose in sub], W, H)
            r.synchronize()
            keep(f"{case}/{i}", r, rgba, depth)

    # frames in flight: the submissions of one case back to back on two frame contexts, twice over (every context claims again
    # with its next serial)
    case = "mesa_333x200"
    scene, W, H, subs = CE.CASES[case]
    sc, r = CE.case_scene(scene), renderers[scene]
    r.set_pipeline_depth(2)
    outs = [submit(r, [sc.uniforms(W, H, *pose, 0) for pose in sub], W, H) for sub in subs + subs]
    r.join()
    for i, (rgba, depth) in enumerate(outs):
        arrays[f"in_flight/{i}/rgba"], arrays[f"in_flight/{i}/depth"] = rgba.cpu().numpy(), depth.cpu().numpy()
    meta["in_flight"] = {"cover": r.debug_cover_stats(), "status": r.frame_status()}
    r.set_pipeline_depth(1)

    # a big queue too small for the items: the triangles it has no room for are rasterised in place and claim nothing
    r.debug_set_queue_caps(CE.SMALL_BIG_CAP, 0)
    rgba, depth = submit(r, [sc.uniforms(W, H, *subs[2][0], 0)], W, H)      # (the view with the most covered regions)
    r.synchronize()
    keep("small_queue", r, rgba, depth)
    r.debug_set_queue_caps(0, 0)

    np.savez(out_path, meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)


if __name__ == "__main__":
    main(sys.argv[1])
