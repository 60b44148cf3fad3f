"""Boxes detected and crops embedded per step (vc_stream_crop_stats) on bench.py's own streams, for profiles/embed_kept_only.md.

    python tools/experiments/embed_kept_stats.py [--steps 4] [point ...]

Points: s640-bf16, m1024-bf16, l1280-fp8 (bench.py's workloads), K32_injected, K256_injected, s720p_bf16 (its extra points).  Runs with
the engine option embed_kept_only as the environment sets it (VC_EMBED_KEPT_ONLY); prints one JSON line per point."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench  # noqa: E402

HEAD = bench.WORKLOADS["s640-bf16"]
POINTS = {
    "s640-bf16": (HEAD, {}),
    "m1024-bf16": (bench.WORKLOADS["m1024-bf16"], {}),
    "l1280-fp8": (bench.WORKLOADS["l1280-fp8"], {}),
    "K32_injected": (HEAD, dict(n_obj=32, inject=32, clip=256)),
    "K256_injected": (HEAD, dict(n_obj=256, inject=256, B=32, clip=128)),
    "s720p_bf16": (bench.WL_720P, dict(frame_hw=(720, 1280), zone=bench.ZONE_720P, clip=256)),
}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("points", nargs="*", default=["s640-bf16"])
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
for name in args.points:
    wl, kw = POINTS[name]
    st = bench.Stream(wl, 0, 0, dev, **kw)
    st.eng.stream_reset()                                   # counters from zero
    st.run_steps(0, args.steps, True)
    boxes, crops = st.eng.stream_crop_stats()
    print(json.dumps({"point": name, "embed_kept_only": int(os.environ.get("VC_EMBED_KEPT_ONLY", "1")), "steps": args.steps, "frames_per_step": st.B,
                      "boxes_per_step": boxes / args.steps, "crops_per_step": crops / args.steps, "dropped": 1.0 - crops / max(boxes, 1),
                      "boxes_per_frame": boxes / (args.steps * st.B), "crops_per_frame": crops / (args.steps * st.B)}), flush=True)
    st.eng.close()
    del st
    torch.cuda.empty_cache()
