"""Times one ``predict.predict_views`` call for 2 and 4 views beside the host route: V ``predict_tracks`` calls with the cameras' extrinsics,
``.cpu()``, then the rules in numpy (``fuse_views_host``, ``solve_view_roots_host``, ``root_trajectory_host``).  Median of 3 in one
process, seeded weights, synthetic tracks.  Informational: no threshold.

``--match`` times ``predict_views(match=True)`` on shuffled views (3 cameras; every person in camera 0, all but one in the others) beside
``match_views_host`` followed by today's ``predict_views`` on the views regrouped per person (a person a camera does not see: an all-NaN
track there, ``valid="finite"``), and ``match_views`` alone at M = 16 and 64 tracks of 2500 frames beside its mirror (the mirror once).

``--align [--max_lag L]`` times ``align_views`` (3 cameras, ``--persons`` swaying persons, views of ``--frames`` -10 / +0 / -20 frames with
clock offsets 0 / -3 / +5, and 16 tracks of 2500 frames at ``max_lag`` 50) beside ``align_views_host`` (the mirror once), and
``predict_views(align=True)`` beside ``predict_views`` on the views cropped beforehand.

``--triangulate`` times ``predict_views(triangulate=True)`` (3 cameras, 0.5 px of pixel noise) beside the call without it, and beside the
host route: the call without it with ``return_views=True``, ``.cpu()``, then ``fuse_views_host``, ``triangulate_joints_host``,
``place_joints_host``, ``solve_view_roots_host`` and ``root_trajectory_host``.

``--calibrate`` times ``predict_views(calibrate=True)`` (3 cameras without extrinsics, 0.5 px of pixel noise) beside the call on the
cameras it returns, and ``calibrate_views`` on that call's lifts and keypoints beside ``calibrate_views_host`` (the mirror once).  With
seeded weights the lifts are not poses, so the cameras found are not the true ones: only the time is read.

``--match_lifts`` times ``predict_views(match=MatchLifts(...))`` on the shuffled views of ``--match`` beside ``predict_tracks``, ``.cpu()``,
``match_lifts_host`` and today's ``predict_views`` on the views regrouped per person, and ``match_lifts`` on that call's lifts beside its
mirror (the mirror once).  With seeded weights the lifts are not poses, so ``max_dist`` allows every pair: only the time is read.

    python tools/predict_views_bench.py [--config h36m_81] [--persons 2] [--frames 1000]
                                        [--match | --align [--max_lag 50] | --triangulate | --calibrate | --match_lifts]
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


def _shuffled(cams, persons, frames, J, seed=1):
    """Persons 1.2 m apart on steps of 0.6 m (the scenes of tests/view_match_util.py): camera 0 sees all, camera v > 0 all but person
    v - 1 (where there are that many), each view in an order of its own -> views, the true person of every track."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cams[0].intrinsics
    t = np.arange(frames)[:, None, None]
    world = []
    for i in range(persons):
        ang = 2.0 * np.pi * i / max(persons, 3) + 0.4
        centre = np.array([np.cos(ang), np.sin(ang), 0.0]) * 1.2 / (2.0 * np.sin(np.pi / max(persons, 3))) + [0.0, 0.0, 0.9 + 0.6 * (i % 4)]
        world.append(centre + rng.normal(0.0, 0.25, (J, 3)) + t * np.array([0.0004, -0.0003, 0.0]) + rng.normal(0.0, 0.004, (frames, J, 3)))
    views, truth = [], []
    for v, c in enumerate(cams):
        who = [int(i) for i in rng.permutation(persons) if v == 0 or i != v - 1 or persons == 1]
        tracks = []
        for i in who:
            p = predict.world_to_camera_host(world[i], c)
            px = np.stack([fx * p[..., 0] / p[..., 2] + cx, fy * p[..., 1] / p[..., 2] + cy], axis=-1) + rng.normal(0.0, 0.5, (frames, J, 2))
            tracks.append(px.astype(np.float32))
        views.append(tracks)
        truth.append(who)
    return views, truth


def _match_rows(model, cfg, args):
    import torch
    from uplift_upsample_3dhpe_amd import predict
    J, N, T = int(cfg.NUM_KEYPOINTS), max(args.persons, 2), args.frames
    kw = dict(resolutions=(1024, 1024))
    cams = _cameras(3)
    views, truth = _shuffled(cams, N, T, J)

    def device():
        r = predict.predict_views(model, cfg, views, cams, match=True, **kw)
        return [torch.cat(a, 0).cpu() for a in r[:4]], r[-1]

    def host():
        person, n, table, _, _ = predict.match_views_host(views, cams)
        flat = [t for tracks in views for t in tracks]
        gone = np.full((T, J, 2), np.nan, np.float32)
        regrouped = [[flat[m] if m >= 0 else gone for m in table[v, :int(n[0])]] for v in range(len(cams))]
        return [torch.cat(a, 0).cpu() for a in predict.predict_views(model, cfg, regrouped, cams, valid="finite", **kw)], person

    device(), host()
    a, b = device(), host()
    ok = [k for per_view in a[1] for k in per_view] == [int(k) for k in b[1]]
    pairs = set(zip([k for per_view in a[1] for k in per_view], [k for per_view in truth for k in per_view]))
    rows = [dict(row="predict_views(match=True)", views=3, persons=N, tracks=sum(len(v) for v in views), frames=T,
                 device_ms=round(_median(lambda: device()), 2), host_match_then_predict_views_ms=round(_median(lambda: host()), 2),
                 same_persons_as_host=bool(ok), true_partition=len(pairs) == len({g for g, _ in pairs}) == len({w for _, w in pairs}),
                 max_abs_root_diff=float(np.nanmax(np.abs(a[0][1].numpy() - b[0][1].numpy()))))]
    for M in (16, 64):                                                   # match_views alone: 8 cameras, M / 8 tracks each, 2500 frames
        cams8 = _cameras(8)
        per = M // 8
        v8, _ = _shuffled(cams8, per + 1, 2500, J, seed=M)
        v8 = [tracks[:per] for tracks in v8]
        dev8 = [[torch.from_numpy(t).cuda() for t in tracks] for tracks in v8]
        got = [r.cpu().numpy() for r in predict.match_views(dev8, cams8)]
        t0 = time.perf_counter()
        want = predict.match_views_host(v8, cams8)
        mirror_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
        rows.append(dict(row="match_views", tracks=M, frames=2500, joints=J, device_ms=round(_median(lambda: predict.match_views(dev8, cams8)), 3),
                         device_then_cpu_ms=round(_median(lambda: [r.cpu() for r in predict.match_views(dev8, cams8)]), 3),
                         mirror_ms_one_run=round(mirror_ms, 1), bits_equal=bool(same), persons=int(want[1][0])))
    return rows


def _swaying(cams, persons, lengths, offsets, J, seed=1):
    """Persons on steps whose centres sway by 0.3 m per axis, periods of 35 to 90 frames (the scenes of tests/view_align_util.py); view v
    is cut from the common timeline at offsets[v] with lengths[v] frames, every person in every view, in order."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cams[0].intrinsics
    base = min(offsets)
    Tc = max(n + o - base for n, o in zip(lengths, offsets))
    t = np.arange(Tc)[:, None]
    world = []
    for i in range(persons):
        ang = 2.0 * np.pi * i / max(persons, 3) + 0.4
        centre = np.array([np.cos(ang), np.sin(ang), 0.0]) * 1.2 / (2.0 * np.sin(np.pi / max(persons, 3))) + [0.0, 0.0, 0.9 + 0.6 * (i % 4)]
        sway = 0.3 * np.sin(2.0 * np.pi * t / rng.uniform(35.0, 90.0, 3) + rng.uniform(0.0, 2.0 * np.pi, 3))
        world.append(centre + rng.normal(0.0, 0.25, (J, 3)) + sway[:, None, :] + rng.normal(0.0, 0.004, (Tc, J, 3)))
    views = []
    for v, c in enumerate(cams):
        start = offsets[v] - base
        tracks = []
        for i in range(persons):
            p = predict.world_to_camera_host(world[i][start:start + lengths[v]], c)
            px = np.stack([fx * p[..., 0] / p[..., 2] + cx, fy * p[..., 1] / p[..., 2] + cy], axis=-1) + rng.normal(0.0, 0.5, (lengths[v], J, 2))
            tracks.append(px.astype(np.float32))
        views.append(tracks)
    return views


def _align_rows(model, cfg, args):
    import torch
    from uplift_upsample_3dhpe_amd import predict
    J, N, T, L = int(cfg.NUM_KEYPOINTS), max(args.persons, 1), args.frames, args.max_lag
    kw = dict(resolutions=(1024, 1024))
    params = predict.AlignViews(max_lag=L)
    rows = []
    for cams, persons, lengths, offsets in ((_cameras(3), N, [T - 10, T, T - 20], [0, -3, 5]), (_cameras(8), 2, [2500] * 8, [0, 3, -4, 7, -9, 12, -15, 20])):
        views = _swaying(cams, persons, lengths, offsets, J)
        dev = [[torch.from_numpy(t).cuda() for t in tracks] for tracks in views]
        got = [r.cpu().numpy() for r in predict.align_views(dev, cams, max_lag=L, same_index=True)]
        t0 = time.perf_counter()
        want = predict.align_views_host(views, cams, max_lag=L, same_index=True)
        mirror_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
        rows.append(dict(row="align_views", views=len(cams), tracks=persons * len(cams), frames=lengths[1], joints=J, max_lag=L,
                         device_ms=round(_median(lambda: predict.align_views(dev, cams, max_lag=L, same_index=True)), 3),
                         device_then_cpu_ms=round(_median(lambda: [r.cpu() for r in predict.align_views(dev, cams, max_lag=L, same_index=True)]), 3),
                         mirror_ms_one_run=round(mirror_ms, 1), bits_equal=bool(same), offsets=[int(o) for o in want[0]],
                         true_offsets=bool([int(o) for o in want[0]] == offsets)))
        if len(cams) == 3:
            cropped = predict.crop_views(views, offsets)[0]

            def aligned():
                return [torch.cat(a, 0).cpu() for a in predict.predict_views(model, cfg, views, cams, align=params, **kw)[:4]]

            def precropped():
                return [torch.cat(a, 0).cpu() for a in predict.predict_views(model, cfg, cropped, cams, **kw)]

            aligned(), precropped()
            a, b = aligned(), precropped()
            rows.append(dict(row="predict_views(align=True)", views=3, persons=persons, frames=lengths, max_lag=L,
                             device_ms=round(_median(aligned), 2), precropped_predict_views_ms=round(_median(precropped), 2),
                             bits_equal=all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))))
    return rows


def _triangulate_rows(model, cfg, args):
    import torch
    from uplift_upsample_3dhpe_amd import predict
    J, N, T, V = int(cfg.NUM_KEYPOINTS), max(args.persons, 1), args.frames, 3
    kw = dict(resolutions=(1024, 1024))
    cams = _cameras(V)
    rng = np.random.default_rng(3)
    views = [[(t + rng.normal(0.0, 0.5, t.shape)).astype(np.float32) for t in tracks] for tracks in _views(cams, N, T, J)]
    kp = np.stack([np.concatenate(views[v]) for v in range(V)])
    lens = [T] * N

    def with_stage():
        return [torch.cat(r, 0).cpu() for r in predict.predict_views(model, cfg, views, cams, triangulate=True, **kw)]

    def without():
        return [torch.cat(r, 0).cpu() for r in predict.predict_views(model, cfg, views, cams, **kw)]

    def host():
        r = predict.predict_views(model, cfg, views, cams, return_views=True, **kw)
        world = np.stack([torch.cat(per_view, 0).cpu().numpy() for per_view in r[-1]])
        fused, count, sees = predict.fuse_views_host(world, kp)
        X, agreed = predict.triangulate_joints_host(kp, cams, sees)
        hybrid, joint_views = predict.place_joints_host(fused, X, agreed, int(cfg.ROOT_KEYTPOINT))
        roots, solved = predict.solve_view_roots_host(hybrid, kp, cams)
        return hybrid, predict.root_trajectory_host(roots, solved, lens), count, joint_views

    with_stage(), without(), host()
    a, b = with_stage(), host()
    same = all(np.array_equal(x.numpy().view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, (b[0], b[1][0], b[1][1], b[2], b[3])))
    return [dict(row="predict_views(triangulate=True)", views=V, persons=N, frames=T, joints=J, with_triangulate_ms=round(_median(with_stage), 2),
                 without_ms=round(_median(without), 2), host_route_ms=round(_median(host), 2), bits_equal_to_host_route=bool(same),
                 placed_share=round(float((b[3] > 0).mean()), 4))]


def _calibrate_rows(model, cfg, args):
    import torch
    from uplift_upsample_3dhpe_amd import predict
    J, N, T, V = int(cfg.NUM_KEYPOINTS), max(args.persons, 1), args.frames, 3
    kw = dict(resolutions=(1024, 1024))
    true = _cameras(V)
    bare = [c.without(extrinsics=True) for c in true]
    rng = np.random.default_rng(3)
    views = [[(t + rng.normal(0.0, 0.5, t.shape)).astype(np.float32) for t in tracks] for tracks in _views(true, N, T, J)]
    found = predict.predict_views(model, cfg, views, bare, calibrate=True, **kw)
    cams, calibration = found[-2], found[-1]

    def with_stage():
        return [torch.cat(r, 0).cpu() for r in predict.predict_views(model, cfg, views, bare, calibrate=True, **kw)[:-2]]

    def on_returned():
        return [torch.cat(r, 0).cpu() for r in predict.predict_views(model, cfg, views, cams, **kw)]

    with_stage(), on_returned()
    a, b = with_stage(), on_returned()
    same = all(np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8)) for x, y in zip(a, b))
    rows = [dict(row="predict_views(calibrate=True)", views=V, persons=N, frames=T, joints=J, with_calibrate_ms=round(_median(with_stage), 2),
                 on_returned_cameras_ms=round(_median(on_returned), 2), bits_equal=bool(same), states=[s for s, _ in calibration],
                 terms=[n for _, n in calibration])]
    # the stage alone, on the lifts (camera axes) and the keypoints of a call: the per-view lifts of return_views, taken back by each camera
    lifts = predict.predict_views(model, cfg, views, cams, return_views=True, **kw)[-1]
    poses = torch.stack([torch.cat(per_view, 0) for per_view in lifts]).contiguous()      # world axes of the cameras found: any axes time alike
    kp = torch.stack([torch.cat([torch.from_numpy(t) for t in tracks], 0) for tracks in views]).cuda().contiguous()

    def device():
        pose, terms = predict.calibrate_views(poses, kp, bare)
        return pose.cpu(), terms.cpu()

    device()
    got = device()
    t0 = time.perf_counter()
    want = predict.calibrate_views_host(poses.cpu().numpy(), kp.cpu().numpy(), bare)
    host_ms = (time.perf_counter() - t0) * 1e3
    rows.append(dict(row="calibrate_views", views=V, rows=N * T, joints=J, device_ms=round(_median(device), 3), mirror_ms_once=round(host_ms, 1),
                     bits_equal=bool(np.array_equal(got[0].numpy().view(np.uint8), want[0].view(np.uint8)) and np.array_equal(got[1].numpy(), want[1]))))
    return rows


def _match_lifts_rows(model, cfg, args):
    import torch
    from uplift_upsample_3dhpe_amd import predict
    J, N, T = int(cfg.NUM_KEYPOINTS), max(args.persons, 2), args.frames
    kw = dict(resolutions=(1024, 1024))
    cams = _cameras(3)
    views, _ = _shuffled(cams, N, T, J)
    counts = [len(v) for v in views]
    view_of = np.repeat(np.arange(3, dtype=np.int32), counts)
    flat = [t for tracks in views for t in tracks]
    M = len(flat)
    pinhole = [cams[v].without(distortion=True, extrinsics=True) for v in view_of]
    params = dict(max_dist=10.0, min_terms=50)                           # seeded weights: the lifts are not poses, so every pair is allowed

    def lifts():
        return torch.cat(predict.predict_tracks(model, cfg, flat, camera=pinhole, **kw)[0], 0).reshape(M, T, J, 3)

    def device():
        r = predict.predict_views(model, cfg, views, cams, match=predict.MatchLifts(**params), **kw)
        return [torch.cat(a, 0).cpu() for a in r[:4]], r[-1]

    def host():
        person, n, table, _, _ = predict.match_lifts_host(lifts().cpu().numpy(), np.stack(flat), view_of, None, 3, **params)
        gone = np.full((T, J, 2), np.nan, np.float32)
        regrouped = [[flat[m] if m >= 0 else gone for m in table[v, :int(n[0])]] for v in range(len(cams))]
        return [torch.cat(a, 0).cpu() for a in predict.predict_views(model, cfg, regrouped, cams, valid="finite", **kw)], person

    device(), host()
    a, b = device(), host()
    ok = [k for per_view in a[1] for k in per_view] == [int(k) for k in b[1]]
    rows = [dict(row="predict_views(match=MatchLifts)", views=3, persons=N, tracks=M, frames=T, device_ms=round(_median(lambda: device()), 2),
                 host_match_then_predict_views_ms=round(_median(lambda: host()), 2), same_persons_as_host=bool(ok))]
    # match_lifts alone on that call's lifts and keypoints, beside its mirror (the mirror once)
    poses, kp = lifts().contiguous(), torch.from_numpy(np.stack(flat)).cuda()
    got = [r.cpu().numpy() for r in predict.match_lifts(poses, kp, view_of, **params)]
    t0 = time.perf_counter()
    want = predict.match_lifts_host(poses.cpu().numpy(), kp.cpu().numpy(), view_of, **params)
    mirror_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(g.view(np.uint8), w.view(np.uint8)) for g, w in zip(got, want))
    rows.append(dict(row="match_lifts", tracks=M, frames=T, joints=J, device_ms=round(_median(lambda: predict.match_lifts(poses, kp, view_of, **params)), 3),
                     device_then_cpu_ms=round(_median(lambda: [r.cpu() for r in predict.match_lifts(poses, kp, view_of, **params)]), 3),
                     mirror_ms_one_run=round(mirror_ms, 1), bits_equal=bool(same), persons=int(want[1][0])))
    return rows


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
    p.add_argument("--match", action="store_true", help="time predict_views(match=True) and match_views instead")
    p.add_argument("--align", action="store_true", help="time align_views and predict_views(align=True) instead")
    p.add_argument("--triangulate", action="store_true", help="time predict_views(triangulate=True) beside the call without it and the host route")
    p.add_argument("--calibrate", action="store_true", help="time predict_views(calibrate=True) beside the call on the returned cameras, and calibrate_views beside its mirror")
    p.add_argument("--match_lifts", action="store_true", help="time predict_views(match=MatchLifts(...)) beside match_lifts_host and the regrouped call, and match_lifts beside its mirror")
    p.add_argument("--max_lag", type=int, default=50, help="the largest clock offset looked for with --align, in frames")
    args = p.parse_args(argv)
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import predict
    from uplift_upsample_3dhpe_amd import synthetic as util
    cfg = util.load_config(args.config)
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=2, perturb=0.1))
    if args.match:
        print(json.dumps(dict(config=args.config, rows=_match_rows(model, cfg, args))))
        return 0
    if args.align:
        print(json.dumps(dict(config=args.config, rows=_align_rows(model, cfg, args))))
        return 0
    if args.triangulate:
        print(json.dumps(dict(config=args.config, rows=_triangulate_rows(model, cfg, args))))
        return 0
    if args.calibrate:
        print(json.dumps(dict(config=args.config, rows=_calibrate_rows(model, cfg, args))))
        return 0
    if args.match_lifts:
        print(json.dumps(dict(config=args.config, rows=_match_lifts_rows(model, cfg, args))))
        return 0
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
