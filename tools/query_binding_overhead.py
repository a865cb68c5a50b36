"""Host microseconds per call of capi.py's query wrappers: what the binding itself costs a sync=False loop.

A renderer created on a torch stream, the Cornell box with three instances, N = 64 rays / points, a preallocated out= tensor or
resume page, sync=False: `--calls` back-to-back calls timed on the host clock, then one synchronisation (timed separately: the
kernels of 64 rays are short, so the loop measures the enqueue path and not the GPU), `--blocks` times over; a wrapper's figure is
its least disturbed block, the minimum.  Only public wrappers are used, so the tool
runs unchanged against another checkout's binding: --root names the tree whose capsaicin_amd package (and library) is imported.
One JSON line: {"label", "calls", "blocks", "host_us": {wrapper: microseconds per call}, "host_us_blocks": {wrapper: every block's},
"drain_us": {wrapper: the final wait per call}}."""
import argparse
import json
import os
import sys
import time

import numpy as np

N = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=300)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    from capsaicin_amd import capi
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == root, capi.__file__

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    host_us, all_us, drain_us = {}, {}, {}
    with torch.cuda.stream(stream):
        r = capi.Renderer(0, stream.cuda_stream)
        geo = capi.Geometry(os.path.join(root, "assets", "cornell_box.obj"))
        r.upload_geometry(geo)
        r.build_bvh()
        t = np.zeros((3, 3, 4), np.float32)
        t[:, 0, 0] = t[:, 1, 1] = t[:, 2, 2] = 1.0
        t[1, 0, 3], t[2, 0, 0], t[2, 0, 3] = 2.5, -1.0, -2.5
        r.set_instances(t)
        P = geo.positions.reshape(-1, 3)
        lo, hi = P.min(0), P.max(0)
        rng = np.random.default_rng(64)
        rays = np.zeros((N, 8), np.float32)
        rays[:, 0:3] = rng.uniform(lo + 0.1, hi - 0.1, (N, 3))
        d = rng.normal(size=(N, 3))
        rays[:, 4:7], rays[:, 7] = d / np.linalg.norm(d, axis=1, keepdims=True), np.inf
        points = np.zeros((N, 4), np.float32)
        points[:, 0:3], points[:, 3] = rng.uniform(lo + 0.1, hi - 0.1, (N, 3)), np.inf
        rays, points = torch.as_tensor(rays, device=dev), torch.as_tensor(points, device=dev)
        hits = torch.empty((N, 4), dtype=torch.float32, device=dev)
        records = torch.empty((N, 8), dtype=torch.float32, device=dev)
        # a page to resume from is the previous call's: every call of the loop asks for the page after it (soon an empty one)
        page = r.trace_rays_multi(rays, 4)
        pages = r.trace_instances_multi(rays, 4)
        loops = {
            "trace_rays": lambda: r.trace_rays(rays, out=hits, sync=False),
            "trace_rays_multi": lambda: r.trace_rays_multi(rays, 4, resume=page, sync=False),
            "trace_instances": lambda: r.trace_instances(rays, out=hits, sync=False),
            "trace_instances_multi": lambda: r.trace_instances_multi(rays, 4, resume=pages, sync=False),
            "closest_points": lambda: r.closest_points(points, out=records, sync=False),
        }
        for name, call in loops.items():
            for _ in range(args.warmup):
                call()
            stream.synchronize()
            blocks = []
            for _ in range(args.blocks):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                t1 = time.perf_counter()
                stream.synchronize()
                blocks.append(((t1 - t0) / args.calls * 1e6, (time.perf_counter() - t1) / args.calls * 1e6))
            host_us[name] = round(min(b[0] for b in blocks), 3)
            all_us[name] = [round(b[0], 3) for b in blocks]
            drain_us[name] = round(min(b[1] for b in blocks), 3)
        r.close()
    print(json.dumps({"label": args.label, "calls": args.calls, "blocks": args.blocks, "host_us": host_us, "host_us_blocks": all_us, "drain_us": drain_us}))


if __name__ == "__main__":
    main()
