"""predict.predict_tracks end to end on seeded synthetic pixel tracks (no dataset), against the same tracks pushed through the public
pieces that existed before it: host normalisation (h36m.normalize_screen_coordinates), PoseTable / SequenceGenerator,
eval.predict_windows, then .cpu() + evaluation.interpolate_between_keyframes in numpy.  Both start from host arrays of pixel coordinates;
predict_tracks ends with the dense poses on the device (also reported: with their copy to the host), the composition with them on the host.
Median of --reps calls after one warm-up call each; frames/s = all frames of all tracks / seconds.
--missing P: also predict_tracks(valid=flags) with a seeded fraction P of the frames missing (missed detections), same tracks.
--fps F: also the same tracks taken as filmed at F frames per second (a float or NUM/DEN): predict_tracks(fps=F) against the host route --
numpy normalisation and resampling to the model's rate by predict.resample_plan, the plain call, .cpu() and numpy interpolation back to the
tracks' own frames.
--repair_joints G [--missing_joints P]: also predict_tracks(valid=joint flags, repair_joints=G) with every joint dropped independently with
probability P (NaN coordinates, flag 0), against the same call with predict.repair_joints_host -- the rule in numpy, written to be read, not
to be fast -- run on the host in front of it; the two must agree bit for bit.
--keypoints NAME [--missing_joints P]: also the same number of tracks in the layout of the preset NAME ("coco17", "body25"), every detector
joint dropped with probability P (flag 0): predict_tracks(keypoints=NAME, valid=joint flags, repair_joints=G or 5) against the same tracks
mapped by predict.map_keypoints_host in front of the plain call; the two must agree bit for bit.
--camera FX FY CX CY: also predict_tracks(camera=...) -- the roots solved and joined on the device -- against the same call without camera
followed by .cpu() of every pose and predict.solve_roots_host / predict.root_trajectory_host, the rule in numpy (written to be read, not to be
fast); the two must agree bit for bit.
--smooth: also predict_tracks(smooth=True) -- with --camera predict_tracks(camera=..., smooth=True), poses and roots filtered -- next to the
same call without smooth in the same process: smooth_extra_ms is the difference of the two medians (one or two more launches, each a serial
walk over the frames of a track); the result must equal predict.one_euro_host on the unfiltered result bit for bit.
--zero_lag (with --smooth): also predict_tracks(smooth=OneEuro(zero_lag=True)), the two-pass filter, beside the causal call and the plain call
in the same process: zero_lag_extra_ms is its median minus the plain call's, zero_lag_over_causal_ms its median minus the causal call's (the
same launches, each lane walking its track twice); the result must equal predict.one_euro_host with that filter bit for bit.  Informational:
no threshold.
--bones: also predict_tracks(bones="track") -- with --camera predict_tracks(camera=..., bones="track") -- next to the same call without bones in
the same process: bones_extra_ms is the difference of the two medians (two more launches: the lengths, the fix); the poses must equal
predict.fix_bones_host with predict.bone_lengths_host on the result without bones, bit for bit.  Informational: no threshold.
--rotations: also predict_tracks(rotations=True) next to the plain call in the same process: rotations_extra_ms is the difference of the two
medians (one more launch), host_rotations_ms the plain call followed by .cpu() of the poses and the numpy rule
(predict.joint_rotations_host); the quaternions must equal that rule on the returned poses bit for bit.  Informational: no threshold.
--interpolation cubic: also predict_tracks(interpolation="cubic") next to the plain (linear) call on the same tracks in the same process:
cubic_extra_ms is the difference of the two medians (uu3d_assemble_tracks_cubic in place of uu3d_assemble_tracks: four predictions read per
interpolated value in place of two); every predicted frame must carry the linear call's bits (cubic_keyframe_bits_equal) and the frames between
must not (cubic_max_abs_diff_to_linear).  Informational: no threshold.
--distortion K1 K2 P1 P2 K3 (with --camera): also predict_tracks(camera=Camera(FX, FY, CX, CY, distortion=...)) on the tracks as that lens shows
them (predict.distort_points_host) beside predict_tracks(camera=(FX, FY, CX, CY)) in the same process: distortion_extra_ms is the difference of
the two medians (one more launch: uu3d_undistort_points in front of everything), host_distortion_ms the tuple's call with
predict.undistort_points_host, the rule in numpy, in front of it; the two must agree bit for bit.  Informational: no threshold.
--extrinsics QW QX QY QZ TX TY TZ (with --camera): also predict_tracks(camera=Camera(FX, FY, CX, CY, orientation=(QW, QX, QY, QZ),
translation=(TX, TY, TZ))) beside predict_tracks(camera=(FX, FY, CX, CY)) in the same process: world_extra_ms is the difference of the two
medians (one more launch: uu3d_camera_to_world behind the root solve), host_world_ms the tuple's call followed by .cpu() and
predict.camera_to_world_host, the rule in numpy; the two must agree bit for bit.  Informational: no threshold.
   python tools/predict_tracks_bench.py [--tracks 40] [--frames 2500] [--batch 512] [--reps 3] [--cases h36m_351:5,h36m_81:4] [--missing 0.3]
                                        [--fps 30] [--repair_joints 5 --missing_joints 0.1] [--keypoints coco17]
                                        [--camera 1145 1145 960 540] [--smooth [--zero_lag]] [--bones] [--rotations] [--interpolation cubic]
                                        [--distortion -0.28 0.09 0.0005 -0.0003 -0.012] [--extrinsics 0.81 -0.53 0.2 0.15 1.8 4.9 1.6]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=40)
    ap.add_argument("--frames", type=int, default=2500)
    ap.add_argument("--batch", type=int, default=512, help="windows per batch (x 2 sequences with the flip)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="h36m_351:5,h36m_81:4")
    ap.add_argument("--no_reuse", action="store_true", help="the window forward instead of the frames form, in both paths")
    ap.add_argument("--missing", type=float, default=0.0, help="also time predict_tracks(valid=...) with this fraction of the frames missing")
    ap.add_argument("--fps", default=None, help="also time predict_tracks(fps=F) against numpy resampling on the host; a float or NUM/DEN")
    ap.add_argument("--repair_joints", type=int, default=None, metavar="G", help="also time predict_tracks(valid=joint flags, repair_joints=G)")
    ap.add_argument("--missing_joints", type=float, default=0.1, metavar="P", help="with --repair_joints: every joint is dropped with probability P")
    ap.add_argument("--keypoints", default=None, metavar="NAME", help="also time predict_tracks(keypoints=NAME) against predict.map_keypoints_host in front")
    ap.add_argument("--camera", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"),
                    help="also time predict_tracks(camera=...) against .cpu() and the numpy rule behind the plain call")
    ap.add_argument("--smooth", action="store_true", help="also time predict_tracks(smooth=True) (with --camera: poses and roots) against the same call without")
    ap.add_argument("--zero_lag", action="store_true", help="with --smooth: also time predict_tracks(smooth=OneEuro(zero_lag=True)) beside the causal call")
    ap.add_argument("--bones", action="store_true", help='also time predict_tracks(bones="track") (with --camera: with the camera) against the same call without')
    ap.add_argument("--rotations", action="store_true", help="also time predict_tracks(rotations=True) against the plain call and against .cpu() and the numpy rule")
    ap.add_argument("--interpolation", choices=["linear", "cubic"], default="linear",
                    help='cubic: also time predict_tracks(interpolation="cubic") beside the plain (linear) call')
    ap.add_argument("--distortion", type=float, nargs=5, default=None, metavar=("K1", "K2", "P1", "P2", "K3"),
                    help="with --camera: also time predict_tracks(camera=Camera(..., distortion=...)) beside the call with the plain tuple")
    ap.add_argument("--extrinsics", type=float, nargs=7, default=None, metavar=("QW", "QX", "QY", "QZ", "TX", "TY", "TZ"),
                    help="with --camera: also time predict_tracks(camera=Camera(..., orientation=, translation=)) beside the call with the plain tuple")
    args = ap.parse_args()
    if args.extrinsics is not None and args.camera is None:
        ap.error("--extrinsics is used together with --camera")
    if args.zero_lag and not args.smooth:
        ap.error("--zero_lag is used together with --smooth")
    if args.distortion is not None and args.camera is None:
        ap.error("--distortion is used together with --camera")
    import numpy as np, torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd import eval as ev
    from uplift_upsample_3dhpe_amd import evaluation, h36m, predict
    from uplift_upsample_3dhpe_amd.data import PoseTable, SequenceGenerator
    rng = np.random.default_rng(0)
    W, H = 1920, 1080
    # smooth tracks in pixels: a random walk per joint around a random place in the image
    px = [(np.cumsum(rng.normal(0, 2.0, size=(args.frames, 17, 2)), 0) + rng.uniform(0.25, 0.75, size=(1, 17, 2)) * [W, H]).astype(np.float32)
          for _ in range(args.tracks)]
    total = args.tracks * args.frames
    flags = [rng.random(args.frames) >= args.missing for _ in range(args.tracks)] if args.missing > 0 else None
    jflags = broken = None
    if args.repair_joints is not None:
        jflags = [rng.random((args.frames, 17)) >= args.missing_joints for _ in range(args.tracks)]
        broken = [np.where(f[:, :, None], t, np.float32(np.nan)).astype(np.float32) for t, f in zip(px, jflags)]
    kpx = kflags = None
    if args.keypoints is not None:
        K = predict.keypoint_map(args.keypoints).inputs
        kpx = [(np.cumsum(rng.normal(0, 2.0, size=(args.frames, K, 2)), 0) + rng.uniform(0.25, 0.75, size=(1, K, 2)) * [W, H]).astype(np.float32)
               for _ in range(args.tracks)]
        kflags = [rng.random((args.frames, K)) >= args.missing_joints for _ in range(args.tracks)]
    lens_camera = seen = None
    if args.distortion is not None:                                     # the same tracks as the lens shows them to a detector
        lens_camera = predict.Camera(*args.camera, distortion=args.distortion)
        seen = [predict.distort_points_host(t, lens_camera).astype(np.float32) for t in px]
    world_camera = None
    if args.extrinsics is not None:
        world_camera = predict.Camera(*args.camera, orientation=args.extrinsics[:4], translation=args.extrinsics[4:])
    reuse = not args.no_reuse
    fps = None if args.fps is None else predict.frame_rate(args.fps)
    results = []
    for case in args.cases.split(","):
        name, msv = case.split(":")
        cfg = util.load_config(name)
        cfg.MASK_STRIDE = int(msv)
        arch = pkg.arch_from_config(cfg)
        model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0, perturb=0.1))

        def new_path(to_host=False):
            out = predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch)
            return [o.cpu() for o in out] if to_host else out

        def missing_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          valid=flags)

        def composition():
            p2 = [h36m.normalize_screen_coordinates(t, w=W, h=H).astype(np.float32) for t in px]
            gen = SequenceGenerator(PoseTable(p2, device=model.device), seq_len=cfg.SEQUENCE_LENGTH, stride=cfg.SEQUENCE_STRIDE,
                                    padding_type=cfg.PADDING_TYPE, flip_augment=False, flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER,
                                    mask_stride=cfg.MASK_STRIDE, stride_mask_align_global=True, shuffle=False)
            desc = gen.descriptors()
            run = np.flatnonzero(ev.needed_windows(desc[:, 1], cfg))
            cen = ev.predict_windows(model, gen, desc[run], cfg, args.batch, flip=True, reuse_frames=reuse)
            pred = np.zeros((len(desc), 17, 3), np.float32)
            pred[run] = cen.cpu().numpy()
            pred, _ = evaluation.interpolate_between_keyframes(pred, desc[:, 1], cfg.SEQUENCE_STRIDE)
            pred = pred - pred[:, cfg.ROOT_KEYTPOINT:cfg.ROOT_KEYTPOINT + 1]
            return np.split(pred, np.cumsum([len(t) for t in px])[:-1])

        def fps_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          fps=fps)

        def fps_host():
            p2 = np.concatenate([h36m.normalize_screen_coordinates(t, w=W, h=H).astype(np.float32) for t in px], 0)
            model_lens, left, right, weight = predict.resample_plan([len(t) for t in px], fps)
            w = weight[:, None, None]
            table = np.where((left == right)[:, None, None], p2[left], (p2[left].astype(np.float64) * (1.0 - w) + p2[right].astype(np.float64) * w).astype(np.float32))
            out = predict.predict_tracks(model, cfg, np.split(table, np.cumsum(model_lens)[:-1]), mask_stride=int(msv), flip=True, reuse_frames=reuse,
                                         batch_size=args.batch)
            res = []
            for o, t in zip(out, px):                                  # back to the tracks' own frames: linear between the bracketing model frames
                o = o.cpu().numpy()
                num = np.arange(len(t)) * (50 * fps.denominator)
                p = num // fps.numerator
                fr = ((num - p * fps.numerator) / fps.numerator)[:, None, None]
                res.append((o[p] * (1.0 - fr) + o[np.minimum(p + 1, len(o) - 1)] * fr).astype(np.float32))
            return res

        def repair_path():
            return predict.predict_tracks(model, cfg, broken, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          valid=jflags, repair_joints=args.repair_joints)

        def repair_host():
            repaired, frame_flags, _ = predict.repair_joints_host(broken, jflags, args.repair_joints)
            return predict.predict_tracks(model, cfg, repaired, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          valid=frame_flags)

        def keypoints_path():
            return predict.predict_tracks(model, cfg, kpx, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          valid=kflags, repair_joints=args.repair_joints or 5, keypoints=args.keypoints)

        def keypoints_host():
            mapped, mapped_flags = predict.map_keypoints_host(args.keypoints, kpx, kflags)
            return predict.predict_tracks(model, cfg, mapped, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          valid=mapped_flags, repair_joints=args.repair_joints or 5)

        def camera_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          camera=tuple(args.camera))

        def camera_host():
            poses = np.concatenate([o.cpu().numpy() for o in new_path()], 0)
            lens = [len(t) for t in px]
            roots, solved = predict.solve_roots_host(poses, np.concatenate(px, 0), tuple(args.camera), lens=lens)
            return predict.root_trajectory_host(roots, solved, lens)

        def distortion_path():
            return predict.predict_tracks(model, cfg, seen, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          camera=lens_camera)

        def distortion_host():
            return predict.predict_tracks(model, cfg, predict.undistort_points_host(seen, lens_camera), resolutions=(W, H), mask_stride=int(msv),
                                          flip=True, reuse_frames=reuse, batch_size=args.batch, camera=tuple(args.camera))

        def world_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          camera=world_camera)

        def world_host():
            poses, roots, state = camera_path()
            sizes = [len(p) for p in poses]
            return predict.camera_to_world_host(torch.cat(poses, 0).cpu().numpy(), torch.cat(roots, 0).cpu().numpy(), torch.cat(state, 0).cpu().numpy(),
                                                world_camera, lens=[sum(sizes)])

        def smooth_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          smooth=True, **({} if args.camera is None else {"camera": tuple(args.camera)}))

        def zero_lag_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          smooth=predict.OneEuro(zero_lag=True), **({} if args.camera is None else {"camera": tuple(args.camera)}))

        def bones_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          bones="track", **({} if args.camera is None else {"camera": tuple(args.camera)}))

        def rotations_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          rotations=True)

        def rotations_host():
            return predict.joint_rotations_host(torch.cat(new_path(), 0).cpu().numpy())[0]

        def cubic_path():
            return predict.predict_tracks(model, cfg, px, resolutions=(W, H), mask_stride=int(msv), flip=True, reuse_frames=reuse, batch_size=args.batch,
                                          interpolation="cubic")

        row = dict(config=name, mask_stride=int(msv), tracks=args.tracks, frames=total, batch=args.batch, reuse_frames=reuse)
        outs = {}
        cases = [("predict_tracks", new_path), ("predict_tracks_to_host", lambda: new_path(True)), ("composition", composition)]
        if flags is not None:
            row["missing"] = args.missing
            cases.append(("predict_tracks_valid", missing_path))
        if fps is not None:
            row["fps"] = str(fps)
            cases += [("predict_tracks_fps", fps_path), ("host_resample", fps_host)]
        if jflags is not None:
            row["repair_joints"], row["missing_joints"] = args.repair_joints, args.missing_joints
            cases += [("predict_tracks_repair", repair_path), ("host_repair", repair_host)]
        if kpx is not None:
            row["keypoints"], row["missing_joints"] = args.keypoints, args.missing_joints
            cases += [("predict_tracks_keypoints", keypoints_path), ("host_keypoints", keypoints_host)]
        if args.camera is not None:
            row["camera"] = list(args.camera)
            cases += [("predict_tracks_camera", camera_path), ("host_camera", camera_host)]
        if lens_camera is not None:
            row["distortion"] = list(args.distortion)
            cases += [("predict_tracks_distortion", distortion_path), ("host_distortion", distortion_host)]
        if world_camera is not None:
            row["extrinsics"] = list(args.extrinsics)
            cases += [("predict_tracks_world", world_path), ("host_world", world_host)]
        if args.smooth:
            cases.append(("predict_tracks_smooth", smooth_path))
        if args.zero_lag:
            cases.append(("predict_tracks_zero_lag", zero_lag_path))
        if args.bones:
            cases.append(("predict_tracks_bones", bones_path))
        if args.rotations:
            cases += [("predict_tracks_rotations", rotations_path), ("host_rotations", rotations_host)]
        if args.interpolation == "cubic":
            cases.append(("predict_tracks_cubic", cubic_path))
        for key, fn in cases:
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                outs[key] = fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            row[key + "_ms"] = round(1e3 * t, 1)
            row[key + "_frames_per_s"] = round(total / t, 1)
        row["speedup"] = round(row["composition_ms"] / row["predict_tracks_ms"], 3)
        row["max_abs_diff"] = float(max(np.abs(a.numpy() - b).max() for a, b in zip(outs["predict_tracks_to_host"], outs["composition"])))
        if fps is not None:
            row["fps_speedup"] = round(row["host_resample_ms"] / row["predict_tracks_fps_ms"], 3)
            row["fps_max_abs_diff"] = float(max(np.abs(a.cpu().numpy() - b).max() for a, b in zip(outs["predict_tracks_fps"], outs["host_resample"])))
        if jflags is not None:
            row["repair_speedup"] = round(row["host_repair_ms"] / row["predict_tracks_repair_ms"], 3)
            row["repair_bits_equal"] = bool(all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                for a, b in zip(outs["predict_tracks_repair"], outs["host_repair"])))
        if kpx is not None:
            row["keypoints_speedup"] = round(row["host_keypoints_ms"] / row["predict_tracks_keypoints_ms"], 3)
            row["keypoints_bits_equal"] = bool(all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                   for a, b in zip(outs["predict_tracks_keypoints"], outs["host_keypoints"])))
        if args.camera is not None:
            row["camera_speedup"] = round(row["host_camera_ms"] / row["predict_tracks_camera_ms"], 3)
            row["camera_extra_ms"] = round(row["predict_tracks_camera_ms"] - row["predict_tracks_ms"], 1)
            roots, state = (torch.cat(x, 0).cpu().numpy() for x in outs["predict_tracks_camera"][1:])
            row["camera_bits_equal"] = bool(np.array_equal(roots.view(np.uint32), outs["host_camera"][0].view(np.uint32))
                                            and np.array_equal(state, outs["host_camera"][1]))
            row["camera_solved_frames"] = int((state == 1).sum())
        if lens_camera is not None:
            row["distortion_extra_ms"] = round(row["predict_tracks_distortion_ms"] - row["predict_tracks_camera_ms"], 1)
            row["distortion_bits_equal"] = bool(all(torch.equal(torch.cat(a, 0).view(torch.int32) if a[0].dtype == torch.float32 else torch.cat(a, 0),
                                                                torch.cat(b, 0).view(torch.int32) if b[0].dtype == torch.float32 else torch.cat(b, 0))
                                                    for a, b in zip(outs["predict_tracks_distortion"], outs["host_distortion"])))
            row["distortion_lost_points"] = int(sum(np.isnan(t).any(axis=2).sum() for t in predict.undistort_points_host(seen, lens_camera)))
        if world_camera is not None:
            row["world_extra_ms"] = round(row["predict_tracks_world_ms"] - row["predict_tracks_camera_ms"], 1)
            same = lambda a, b: bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32)))
            got = [torch.cat(x, 0).cpu().numpy() for x in outs["predict_tracks_world"][:2]]
            row["world_bits_equal"] = same(got[0], outs["host_world"][0]) and same(got[1], outs["host_world"][1])
        if args.smooth:
            base = "predict_tracks_camera" if args.camera is not None else "predict_tracks"
            row["smooth_extra_ms"] = round(row["predict_tracks_smooth_ms"] - row[base + "_ms"], 1)
            lens, F = [len(t) for t in px], predict.OneEuro()
            plain, got = outs[base], outs["predict_tracks_smooth"]
            same = lambda a, b, F=F, **kw: np.array_equal(torch.cat(a, 0).cpu().numpy().view(np.uint32),
                                                          predict.one_euro_host(torch.cat(b, 0).cpu().numpy(), lens, 50, F, **kw).view(np.uint32))
            if args.camera is None:
                row["smooth_bits_equal"] = bool(same(got, plain))
            else:
                row["smooth_bits_equal"] = bool(same(got[0], plain[0]) and same(got[1], plain[1], state=torch.cat(plain[2], 0).cpu().numpy()))
            if args.zero_lag:
                row["zero_lag_extra_ms"] = round(row["predict_tracks_zero_lag_ms"] - row[base + "_ms"], 1)
                row["zero_lag_over_causal_ms"] = round(row["predict_tracks_zero_lag_ms"] - row["predict_tracks_smooth_ms"], 1)
                got, Z = outs["predict_tracks_zero_lag"], predict.OneEuro(zero_lag=True)
                if args.camera is None:
                    row["zero_lag_bits_equal"] = bool(same(got, plain, F=Z))
                else:
                    row["zero_lag_bits_equal"] = bool(same(got[0], plain[0], F=Z)
                                                      and same(got[1], plain[1], F=Z, state=torch.cat(plain[2], 0).cpu().numpy()))
        if args.bones:
            base = "predict_tracks_camera" if args.camera is not None else "predict_tracks"
            row["bones_extra_ms"] = round(row["predict_tracks_bones_ms"] - row[base + "_ms"], 1)
            lens = [len(t) for t in px]
            plain = torch.cat(outs[base][0] if args.camera is not None else outs[base], 0).cpu().numpy()
            got = torch.cat(outs["predict_tracks_bones"][0] if args.camera is not None else outs["predict_tracks_bones"], 0).cpu().numpy()
            want = predict.fix_bones_host(plain, lens, predict.bone_lengths_host(plain, lens))
            row["bones_bits_equal"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        if args.rotations:
            row["rotations_extra_ms"] = round(row["predict_tracks_rotations_ms"] - row["predict_tracks_ms"], 1)
            got = torch.cat(outs["predict_tracks_rotations"][1], 0).cpu().numpy()
            row["rotations_bits_equal"] = bool(np.array_equal(got.view(np.uint32), outs["host_rotations"].view(np.uint32)))
        if args.interpolation == "cubic":
            row["cubic_extra_ms"] = round(row["predict_tracks_cubic_ms"] - row["predict_tracks_ms"], 1)
            stride = ev.prediction_stride(cfg)
            keys = torch.arange(args.frames, device=model.device) % (stride or 1) == 0
            row["cubic_keyframe_bits_equal"] = bool(all(torch.equal(a[keys].view(torch.int32), b[keys].view(torch.int32))
                                                        for a, b in zip(outs["predict_tracks_cubic"], outs["predict_tracks"])))
            row["cubic_max_abs_diff_to_linear"] = float(max((a - b).abs().max() for a, b in zip(outs["predict_tracks_cubic"], outs["predict_tracks"])))
        row["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
        results.append(row)
        del model
    return results


if __name__ == "__main__":
    main()
