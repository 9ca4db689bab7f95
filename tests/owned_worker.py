"""Child process of tests/test_owned_strips_gpu.py: renders the cases of owned_emul.CASES with the covered-region path forced on
(TOPO_COVER=1 in the environment: the switch is read once per process) and k_resolve's owned strips switched on and off through the
test hook, on ONE renderer per colour format -- so the table of strip records always holds records of earlier frames, other
viewpoints and other target shapes -- and writes the frames and the hooks' counts to the .npz named on the command line."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMAT_CASE = ("mesa_333x200", 3)      # the near-cut owners and a lost bid: rendered in every colour format
MODE_CASE = ("mesa_333x200", 2)        # the view with the most claimed regions: rendered in every view mode


def main(out_path):
    import torch
    import topo_renderer_amd as T
    import owned_emul as OE

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
        meta[name] = {"owned": r.debug_owned_strips(), "cover": r.debug_cover_stats(), "status": r.frame_status(), "counters": r.counters()}

    def both(name, r, views, W, H):      # the path on, then off
        for setting in ("on", "off"):
            r.debug_set_resolve_owned(setting == "on")
            rgba, depth = submit(r, views, W, H)
            r.synchronize()
            keep(f"{name}/{setting}", r, rgba, depth)
        r.debug_set_resolve_owned(True)

    renderers = {}

    def renderer(scene, W, H, fmt=T.FORMAT_RGBA8_UNORM_SRGB):
        if (scene, fmt) not in renderers:
            renderers[(scene, fmt)] = T.TerrainRenderer(W, H, color_format=fmt)
            OE.case_scene(scene).load(renderers[(scene, fmt)])
        return renderers[(scene, fmt)]

    for case, (scene, W, H, subs) in OE.CASES.items():
        sc, r = OE.case_scene(scene), renderer(scene, W, H)
        for i, sub in enumerate(subs):
            both(f"{case}/{i}", r, [sc.uniforms(W, H, *pose, 0) for pose in sub], W, H)

    scene, W, H, subs = OE.CASES[MODE_CASE[0]]
    sc = OE.case_scene(scene)
    for mode in (1, 2):
        both(f"mode{mode}", renderer(scene, W, H), [sc.uniforms(W, H, *subs[MODE_CASE[1]][0], mode)], W, H)
    scene, W, H, subs = OE.CASES[FORMAT_CASE[0]]
    for fmt in (T.FORMAT_BGRA8_UNORM_SRGB, T.FORMAT_RGBA8_UNORM, T.FORMAT_BGRA8_UNORM):
        r = renderer(scene, W, H, fmt)
        both(f"format{fmt}/warm", r, [sc.uniforms(W, H, *subs[MODE_CASE[1]][0], 0)], W, H)      # (another viewpoint first: stale records)
        both(f"format{fmt}", r, [sc.uniforms(W, H, *subs[FORMAT_CASE[1]][0], 0)], W, H)

    # frames in flight: the single-view submissions of the 333 x 200 case back to back on two frame contexts, twice over (each
    # context's table then holds the records of its own earlier frames), the path on and then off
    scene, W, H, subs = OE.CASES["mesa_333x200"]
    r = renderer(scene, W, H)
    r.set_pipeline_depth(2)
    for setting in ("on", "off"):
        r.debug_set_resolve_owned(setting == "on")
        outs = [submit(r, [sc.uniforms(W, H, *pose, 0) for pose in sub], W, H) for sub in subs + subs]
        r.join()
        for j, (rgba, depth) in enumerate(outs):
            arrays[f"in_flight/{j}/{setting}/rgba"], arrays[f"in_flight/{j}/{setting}/depth"] = rgba.cpu().numpy(), depth.cpu().numpy()
        meta[f"in_flight/{setting}"] = {"owned": r.debug_owned_strips(), "status": r.frame_status()}
    r.debug_set_resolve_owned(True)
    r.set_pipeline_depth(1)

    np.savez(out_path, meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)


if __name__ == "__main__":
    main(sys.argv[1])
