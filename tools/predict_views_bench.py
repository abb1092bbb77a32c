"""Times one ``predict.predict_views`` call for 2 and 4 views beside the host route: V ``predict_tracks`` calls with the cameras' extrinsics,
``.cpu()``, then the rules in numpy (``fuse_views_host``, ``solve_view_roots_host``, ``root_trajectory_host``).  Median of 3 in one
process, seeded weights, synthetic tracks.  Informational: no threshold.

    python tools/predict_views_bench.py [--config h36m_81] [--persons 2] [--frames 1000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _cameras(V):
    from uplift_upsample_3dhpe_amd import predict
    cams = []
    for v in range(V):
        ang = 2.0 * np.pi * v / max(V, 3)
        pos = np.array([4.2 * np.cos(ang), 4.2 * np.sin(ang), 1.5])
        z = np.array([0.0, 0.0, 0.9]) - pos
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        q, t = predict.extrinsics_from_opencv(R, -R @ pos)
        cams.append(predict.Camera(1145.0, 1143.5, 512.25, 515.75, orientation=q, translation=t))
    return cams


def _views(cams, persons, frames, J):
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(0)
    fx, fy, cx, cy = cams[0].intrinsics
    views = [[] for _ in cams]
    for i in range(persons):
        t = np.arange(frames)[:, None, None]
        world = rng.normal(0.0, 0.25, (J, 3)) + [0.5 * i - 0.3, -0.4, 0.9] + t * np.array([0.001, 0.002, 0.0]) + rng.normal(0.0, 0.004, (frames, J, 3))
        for v, c in enumerate(cams):
            p = predict.world_to_camera_host(world, c)
            views[v].append(np.stack([fx * p[..., 0] / p[..., 2] + cx, fy * p[..., 1] / p[..., 2] + cy], axis=-1).astype(np.float32))
    return views


def _median(fn, n=3):
    import torch
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--config", default="h36m_81")
    p.add_argument("--persons", type=int, default=2)
    p.add_argument("--frames", type=int, default=1000)
    args = p.parse_args(argv)
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import predict
    from uplift_upsample_3dhpe_amd import synthetic as util
    cfg = util.load_config(args.config)
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=2, perturb=0.1))
    J, N = int(cfg.NUM_KEYPOINTS), args.persons
    kw = dict(resolutions=(1024, 1024))
    rows = []
    for V in (2, 4):
        cams = _cameras(V)
        views = _views(cams, N, args.frames, J)
        lens = [args.frames] * N

        def device():
            return [torch.cat(r, 0).cpu() for r in predict.predict_views(model, cfg, views, cams, **kw)]

        def host():
            world = [torch.cat(predict.predict_tracks(model, cfg, views[v], camera=cams[v], **kw)[0], 0).cpu().numpy() for v in range(V)]
            kp = np.stack([np.concatenate(views[v]) for v in range(V)])
            fused, count, _ = predict.fuse_views_host(np.stack(world), kp)
            roots, solved = predict.solve_view_roots_host(fused, kp, cams)
            return fused, predict.root_trajectory_host(roots, solved, lens), count

        device(), host()                                                 # warm-up: graphs, tables
        a, b = device(), host()
        # (the host route runs V calls whose batches are composed differently from the one flattened run: compared by value, not by bits)
        pose_diff = float(np.nanmax(np.abs(a[0].numpy() - b[0])))
        root_diff = float(np.nanmax(np.abs(a[1].numpy() - b[1][0])))
        rows.append(dict(views=V, persons=N, frames=args.frames, predict_views_ms=round(_median(device), 2), host_route_ms=round(_median(host), 2),
                         max_abs_pose_diff=pose_diff, max_abs_root_diff=root_diff, solved=int((b[1][1] == 1).sum())))
    print(json.dumps(dict(config=args.config, rows=rows)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
