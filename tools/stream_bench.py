"""Microseconds per tick of stream.StreamSession (one frame of 2D keypoints per slot in, one 3D pose per slot out), flip on, against the
way to get the same pose without it: the host builds this tick's window and stride mask for every slot from the frames so far (numpy),
uploads them with their mirrored copies and calls ``model([x, mask])`` once -- the spatial stack over all frames of every window, every tick.
A tick = host clock from the call to the synchronised result (a live consumer reads every pose); host input in all three variants.
Median (and 90th percentile) over --ticks ticks after --warmup ticks, per config and slot count.
A case is CONFIG:s_in, or generic:J,d_s,d_t,heads,N:s_in for a model with generic dims (e.g. --cases generic:25,16,64,4,27:4): its tick
(the one-workgroup-per-frame spatial stack + the generic forward's second stage in the graph) beside the same baseline.
   python tools/stream_bench.py [--slots 1,8,64] [--cases h36m_81:4,h36m_351:5] [--ticks 300] [--warmup 60] [--lookahead 0] [--fps F [--out_fps G] [--interpolation cubic]]
                                [--repair_joints G] [--detections D] [--camera FX FY CX CY [--distortion K1 K2 P1 P2 K3 | --extrinsics QW QX QY QZ TX TY TZ]] [--smooth] [--bones] [--rotations] [--drain] [--views V]
--fps F (a float or NUM/DEN): microseconds per PUSH of StreamSession(fps=F) -- one source frame in, one pose out, on average
model_fps / F sub-ticks -- next to the plain session pushed at the model's rate (the cost of one model tick); the lookahead is raised to
the smallest one the rate allows.  The numpy baseline is left out.
--out_fps G (with --fps): the push of StreamSession(fps=F, out_fps=G) -- every due pose per push, up to ceil(G / F) -- as out_fps_graph_us,
next to the fps-only push (one pose per push) and the plain session.
--interpolation cubic (with --fps, with or without --out_fps): the push of StreamSession(fps=F[, out_fps=G], interpolation="cubic") -- the
emit reads four ring rows in place of two, at the cubic's own smallest lookahead -- as cubic_graph_us beside the linear session of the same
rates in the same process (fps_graph_us / out_fps_graph_us); cubic_minus_linear_us is the difference of the two medians.  Informational.
--repair_joints G [--missing_joints P] (not with --fps): the tick of StreamSession(repair_joints=G) as repair_graph_us -- per-joint flags
with a share P (default 0.1) of the joints unobserved, K = G // s_in + 2 frames of spatial features per slot and tick -- next to the
tick of StreamSession(missed_detections=True) fed the same frames with the per-frame flags those joints imply (md_graph_us).  The numpy
baseline is left out.
--detections D (not with --fps / --repair_joints): a synthetic scene of min(slots, D) people whose rows are shuffled in every frame --
the tick of StreamSession(detections=D) fed the lists (det_graph_us) next to the tick of StreamSession(missed_detections=True) on the same
frames in the same process, fed what predict.associate_host makes of them, worked out before the clock starts (md_graph_us), and next to
the HOST ROUTE a user takes without the option (host_route_us): the detections start on the device, are copied back, matched in numpy
(predict.AssociationHost), reset() is called for the slots born, then push().  The numpy baseline is left out.
--camera FX FY CX CY (not with the options above): the tick of StreamSession(camera=...) -- one more launch at the end of the captured
tick, two more buffers returned -- as camera_graph_us next to the tick of the same session without camera (graph_us) on the same frames in
the same process: both sessions are alive side by side and every tick is pushed into both, the order alternating from tick to tick.
camera_minus_graph_us is the difference of the two medians.  The numpy baseline is left out.
--distortion K1 K2 P1 P2 K3 (with --camera, not with the other options): the tick of StreamSession(camera=Camera(FX, FY, CX, CY, distortion=...))
-- one more launch, uu3d_undistort_points, the first of the captured tick -- as distortion_graph_us next to the tick of the session with the
plain tuple (camera_graph_us) on the same frames in the same process, measured side by side in the same way.  distortion_minus_camera_us is
the difference of the two medians.  Informational: no threshold.  The numpy baseline is left out.
--extrinsics QW QX QY QZ TX TY TZ (with --camera, not with the other options): the tick of StreamSession(camera=Camera(FX, FY, CX, CY,
orientation=(QW, QX, QY, QZ), translation=(TX, TY, TZ))) -- one more launch, uu3d_camera_to_world, directly behind uu3d_stream_root -- as
world_graph_us next to the tick of the session with the plain tuple (camera_graph_us) on the same frames in the same process, measured side
by side in the same way.  world_minus_camera_us is the difference of the two medians.  Informational: no threshold.
--views V (alone; --slots must be multiples of V): the tick of StreamSession(camera=[V Cameras with extrinsics], views=V) -- one more launch,
uu3d_stream_views, directly behind uu3d_camera_to_world, the slots view-major, slots / V persons returned -- as views_graph_us next to the
tick of the same session without views (one Camera per slot: world_graph_us) on the same frames in the same process, measured side by side
in the same way.  views_minus_world_us is the difference of the two medians.  The cameras stand on a ring of 4 m around the origin, 1145
pixels of focal length.  Informational: no threshold.
--smooth (alone or with --camera, not with the other options): the tick of StreamSession(smooth=True) -- one more launch at the end of the
captured tick, with --camera two (poses and roots) -- as smooth_graph_us next to the tick of the same session without smooth (graph_us;
with --camera both sessions have the camera), measured side by side in the same way.  smooth_minus_graph_us is the difference of the two
medians.  The numpy baseline is left out.
--rotations (alone or with --camera, not with --smooth, --bones or the other options): the tick of StreamSession(rotations=True) -- one
more launch, the last of the captured tick -- as rotations_graph_us next to the tick of the same session without it (graph_us) and next
to that tick followed by .cpu() of the poses and the numpy rule, rotations.joint_rotations_host (rotations_host_us), measured side by
side in the same way.  rotations_minus_graph_us is the difference of the first two medians.  Informational: no threshold.
--bones (alone or with --camera, not with --smooth or the other options): the tick of StreamSession(bones="track") -- one more launch
behind the emit, in front of the root solve -- as bones_graph_us next to the tick of the same session without bones (graph_us; with
--camera both sessions have the camera), measured side by side in the same way.  bones_minus_graph_us is the difference of the two
medians.  Informational: no threshold.  The numpy baseline is left out.
--drain (alone): StreamSession.finish() -- `lookahead` drain ticks and the reset, from the call to the synchronised result -- at lookahead 13
and at the largest one, as finish_us, beside the plain tick of the same session in the same process (graph_us); finish_over_tick is their
ratio, finish_per_drain_tick_us = finish_us / lookahead.  Each finish follows 8 pushes of a new track; the first finish (allocation and the
capture) is not timed.  Use --slots 1,64.  The numpy baseline is left out."""
import argparse, json, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--cases", default="h36m_81:4,h36m_351:5")
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--lookahead", type=int, default=0)
    ap.add_argument("--fps", default=None)
    ap.add_argument("--out_fps", default=None)
    ap.add_argument("--interpolation", default="linear", choices=("linear", "cubic"))
    ap.add_argument("--repair_joints", type=int, default=None)
    ap.add_argument("--missing_joints", type=float, default=0.1)
    ap.add_argument("--detections", type=int, default=None)
    ap.add_argument("--camera", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), default=None)
    ap.add_argument("--distortion", type=float, nargs=5, metavar=("K1", "K2", "P1", "P2", "K3"), default=None)
    ap.add_argument("--extrinsics", type=float, nargs=7, metavar=("QW", "QX", "QY", "QZ", "TX", "TY", "TZ"), default=None)
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--bones", action="store_true")
    ap.add_argument("--rotations", action="store_true")
    ap.add_argument("--drain", action="store_true")
    ap.add_argument("--views", type=int, default=None)
    args = ap.parse_args()
    if args.bones and (args.smooth or args.fps is not None or args.repair_joints is not None or args.detections is not None):
        ap.error("--bones is not measured together with --smooth / --fps / --repair_joints / --detections")
    if args.rotations and (args.bones or args.smooth or args.fps is not None or args.repair_joints is not None or args.detections is not None):
        ap.error("--rotations is not measured together with --bones / --smooth / --fps / --repair_joints / --detections")
    if args.drain and (args.rotations or args.bones or args.smooth or args.camera is not None or args.fps is not None or args.repair_joints is not None or args.detections is not None):
        ap.error("--drain is measured alone")
    if args.smooth and (args.fps is not None or args.repair_joints is not None or args.detections is not None):
        ap.error("--smooth is not measured together with --fps / --repair_joints / --detections")
    if args.camera is not None and (args.fps is not None or args.repair_joints is not None or args.detections is not None):
        ap.error("--camera is not measured together with --fps / --repair_joints / --detections")
    if args.repair_joints is not None and args.fps is not None:
        ap.error("--repair_joints is not measured together with --fps")
    if args.detections is not None and (args.fps is not None or args.repair_joints is not None):
        ap.error("--detections is not measured together with --fps / --repair_joints")
    if args.distortion is not None and (args.camera is None or args.smooth or args.bones or args.rotations):
        ap.error("--distortion is measured with --camera alone")
    if args.extrinsics is not None and (args.camera is None or args.smooth or args.bones or args.rotations or args.distortion is not None):
        ap.error("--extrinsics is measured with --camera alone")
    if args.views is not None and (args.drain or args.rotations or args.bones or args.smooth or args.camera is not None or args.fps is not None
                                   or args.repair_joints is not None or args.detections is not None):
        ap.error("--views is measured alone")
    if args.views is not None and (not 1 <= args.views <= 8 or any(int(v) % args.views for v in args.slots.split(","))):
        ap.error("--views takes V in 1 .. 8 and --slots that are multiples of V")
    if args.out_fps is not None and args.fps is None:
        ap.error("--out_fps needs --fps")
    if args.interpolation == "cubic" and args.fps is None:
        ap.error("--interpolation cubic needs --fps")
    import numpy as np, torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd import h36m, stream
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs the GPU: nothing is measured without one")
    W, H = 1920, 1080
    total = args.warmup + args.ticks
    results = []
    for case in re.findall(r"generic:[\d,]+:\d+|[^,]+", args.cases):      # (a generic case has commas of its own)
        name, msv = case.rsplit(":", 1)
        ms = int(msv)
        if name.startswith("generic:"):
            # generic:J,d_s,d_t,heads,N:s_in -- a model with generic dims on h36m_81's other settings (two spatial and two temporal blocks,
            # MLP ratio 2; STRIDES: N's prime factors; the flip table: joint 0 stays, the others swap in pairs)
            gJ, gds, gdt, gh, gN = (int(v) for v in name.split(":", 1)[1].split(","))
            cfg = util.load_config("h36m_81")
            strides, rest = [], gN
            for p in (3, 5, 7):
                while rest % p == 0:
                    strides.append(p); rest //= p
            if rest != 1 or not strides:
                ap.error("generic: N must be a product of 3s, 5s and 7s")
            cfg.NUM_KEYPOINTS, cfg.SPATIAL_EMBED_DIM, cfg.TEMPORAL_EMBED_DIM, cfg.NUM_HEADS = gJ, gds, gdt, gh
            cfg.SEQUENCE_LENGTH, cfg.STRIDES, cfg.PADDINGS, cfg.MLP_RATIO, cfg.MASK_STRIDE = gN, strides, None, 2.0, ms
            cfg.SPATIAL_TRANSFORMER_BLOCKS, cfg.TEMPORAL_TRANSFORMER_BLOCKS = 2, 2
            cfg.ROOT_KEYTPOINT = min(int(cfg.ROOT_KEYTPOINT), gJ - 1)
            flip_order = list(range(gJ))
            for i in range(1, gJ - 1, 2):
                flip_order[i], flip_order[i + 1] = i + 1, i
            cfg.AUGM_FLIP_KEYPOINT_ORDER = flip_order
        else:
            cfg = util.load_config(name)
        arch = pkg.arch_from_config(cfg)
        model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0, perturb=0.1))
        N, S, J = cfg.SEQUENCE_LENGTH, cfg.SEQUENCE_STRIDE, int(cfg.NUM_KEYPOINTS)
        order = np.asarray(cfg.AUGM_FLIP_KEYPOINT_ORDER)
        d_order = torch.as_tensor(order, dtype=torch.long, device=model.device)
        for T in (int(v) for v in args.slots.split(",")):
            rng = np.random.default_rng(0)
            px = (np.cumsum(rng.normal(0, 2.0, size=(total, T, J, 2)), 0) + rng.uniform(0.25, 0.75, size=(1, T, J, 2)) * [W, H]).astype(np.float32)

            seen = rng.uniform(size=(total, T, J)) >= args.missing_joints      # per-joint flags of --repair_joints

            def session(graph, valid=None, **rate):
                s = stream.StreamSession(model, cfg, slots=T, resolutions=(W, H), mask_stride=ms, flip=True, graph=graph,
                                         **({"lookahead": args.lookahead} if "lookahead" not in rate else {}), **rate)
                ts = []
                for k in range(total):
                    t0 = time.perf_counter()
                    s.push(px[k], **({} if valid is None else {"valid": valid[k]}))
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                s.check_range()
                s.close()
                return ts[args.warmup:]

            def baseline():
                hist = np.zeros((total, T, J, 2), np.float32)
                ts = []
                n = np.arange(N)
                for k in range(total):
                    t0 = time.perf_counter()
                    hist[k] = h36m.normalize_screen_coordinates(px[k], w=W, h=H)
                    L, c = k + 1, k - args.lookahead
                    if c >= 0:
                        f = c + (n - N // 2) * S
                        lo, hi = c % S, (L - 1 - c % S) // S * S + c % S
                        inside = (f >= 0) & (f < L)
                        src = np.clip(f, lo, hi)
                        m = (f % ms == 0)
                        if cfg.PADDING_TYPE != "copy":
                            m = m & inside
                        x = hist[src].transpose(1, 0, 2, 3) * m[None, :, None, None]                      # (T, N, J, 2), masked frames zeroed
                        xf = x[:, :, order].copy(); xf[..., 0] *= -1.0
                        xb = torch.from_numpy(np.ascontiguousarray(np.concatenate([x, xf], 0), np.float32)).pin_memory().to(model.device, non_blocking=True)
                        mb = torch.from_numpy(np.tile((f % ms == 0)[None], (2 * T, 1))).pin_memory().to(model.device, non_blocking=True)
                        _, cen = model([xb, mb], training=False)
                        fl = torch.cat([cen[T:, :, :1] * -1.0, cen[T:, :, 1:]], -1).index_select(1, d_order)
                        pose = (cen[:T] + fl) / 2.0
                        pose = pose - pose[:, cfg.ROOT_KEYTPOINT:cfg.ROOT_KEYTPOINT + 1]
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                return ts[args.warmup:]

            def detections_variants():
                from uplift_upsample_3dhpe_amd import predict
                Dn = args.detections
                P = min(T, Dn)
                dets = np.zeros((total, Dn, J, 2), np.float32)
                for k in range(total):
                    dets[k, :P] = px[k, rng.permutation(P)]
                host = predict.associate_host(dets, np.full(total, P), slots=T)
                t_i, s_i = np.nonzero(host.slot_det >= 0)
                frames = np.zeros((total, T, J, 2), np.float32)
                frames[t_i, s_i] = dets[t_i, host.slot_det[t_i, s_i]]
                d_dets = torch.from_numpy(dets).to(model.device)

                def timed(s, tick):
                    ts = []
                    for k in range(total):
                        t0 = time.perf_counter()
                        tick(s, k)
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t0)
                    s.check_range()
                    s.close()
                    return ts[args.warmup:]

                new = lambda **kw: stream.StreamSession(model, cfg, slots=T, resolutions=(W, H), mask_stride=ms, flip=True, lookahead=args.lookahead, **kw)

                def md_tick(s, k):
                    if host.born[k].any():
                        s.reset(slots=np.flatnonzero(host.born[k]))
                    s.push(frames[k], active=host.alive[k] != 0, valid=host.slot_full[k])

                def host_route():
                    rule = predict.AssociationHost(T, Dn, J)
                    kp = np.zeros((T, J, 2), np.float32)

                    def tick(s, k):
                        det = d_dets[k].cpu().numpy()                  # the detector's output sits on the device: copy it back and wait
                        _, slot_det, born = rule.step(det, P)
                        kp[:] = 0.0
                        kp[slot_det >= 0] = det[slot_det[slot_det >= 0]]
                        if born.any():
                            s.reset(slots=np.flatnonzero(born))
                        s.push(kp, active=rule.alive, valid=slot_det >= 0)
                    return timed(new(missed_detections=True), tick)

                row.update(detections=Dn, people=P, tracks=int(host.num_tracks), dropped=int(host.dropped))
                return (("det_graph", lambda: timed(new(detections=Dn), lambda s, k: s.push_detections(d_dets[k], P))),
                        ("md_graph", lambda: timed(new(missed_detections=True), md_tick)), ("host_route", host_route))

            def camera_variants():
                new = lambda **kw: stream.StreamSession(model, cfg, slots=T, resolutions=(W, H), mask_stride=ms, flip=True, lookahead=args.lookahead, **kw)
                place = {} if args.camera is None else {"camera": tuple(args.camera)}
                if args.smooth:                                       # both with the camera (if any), one of them with the filter behind the tick
                    pair = {"smooth_graph": new(smooth=True, **place), "graph": new(**place)}
                elif args.bones:                                      # ... one of them with the fix behind the emit
                    pair = {"bones_graph": new(bones="track", **place), "graph": new(**place)}
                elif args.rotations:                                  # ... one with the launch at the tick's end, one followed by the host rule
                    pair = {"rotations_graph": new(rotations=True, **place), "graph": new(**place), "rotations_host": new(**place)}
                elif args.distortion is not None:                     # both with the camera, one of them with the lens in front of the tick
                    pair = {"distortion_graph": new(camera=stream.Camera(*args.camera, distortion=args.distortion)),
                            "camera_graph": new(camera=tuple(args.camera))}
                elif args.extrinsics is not None:                     # both with the camera, one of them with the world launch behind the root solve
                    pair = {"world_graph": new(camera=stream.Camera(*args.camera, orientation=args.extrinsics[:4], translation=args.extrinsics[4:])),
                            "camera_graph": new(camera=tuple(args.camera))}
                else:
                    pair = {"camera_graph": new(camera=tuple(args.camera)), "graph": new()}
                ts = {key: [] for key in pair}
                for k in range(total):
                    for key in (list(pair) if k % 2 == 0 else list(pair)[::-1]):
                        t0 = time.perf_counter()
                        out = pair[key].push(px[k])
                        if key == "rotations_host":                   # the poses to the host (it waits), then the rule in numpy
                            stream.joint_rotations_host(out[0].cpu().numpy())
                        torch.cuda.synchronize()
                        ts[key].append(time.perf_counter() - t0)
                for s in pair.values():
                    s.check_range()
                    s.close()
                row.update(camera=None if args.camera is None else list(args.camera), smooth=bool(args.smooth), bones=bool(args.bones),
                           rotations=bool(args.rotations), **({} if args.distortion is None else {"distortion": list(args.distortion)}),
                           **({} if args.extrinsics is None else {"extrinsics": list(args.extrinsics)}))
                return tuple((key, lambda key=key: ts[key][args.warmup:]) for key in pair)

            def views_variants():
                V = args.views
                half = [0.5 * np.pi * (v + 0.5) / V for v in range(V)]        # camera v: yawed about the world's z, 4 m from the origin
                rig = [stream.Camera(1145.0, 1145.0, 0.5 * W, 0.5 * H, orientation=(np.cos(h), 0.0, 0.0, np.sin(h)),
                                     translation=(4.0 * np.cos(2.0 * h), 4.0 * np.sin(2.0 * h), 1.5)) for h in half]
                new = lambda **kw: stream.StreamSession(model, cfg, slots=T, resolutions=(W, H), mask_stride=ms, flip=True, lookahead=args.lookahead, **kw)
                pair = {"views_graph": new(camera=rig, views=V), "world_graph": new(camera=[c for c in rig for _ in range(T // V)])}
                ts = {key: [] for key in pair}
                for k in range(total):
                    for key in (list(pair) if k % 2 == 0 else list(pair)[::-1]):
                        t0 = time.perf_counter()
                        pair[key].push(px[k])
                        torch.cuda.synchronize()
                        ts[key].append(time.perf_counter() - t0)
                for s in pair.values():
                    s.check_range()
                    s.close()
                row.update(views=V, persons=T // V)
                return tuple((key, lambda key=key: ts[key][args.warmup:]) for key in pair)

            if args.drain:
                for a in sorted({min(13, stream.max_lookahead(cfg)), stream.max_lookahead(cfg)}):
                    s = stream.StreamSession(model, cfg, slots=T, resolutions=(W, H), mask_stride=ms, flip=True, lookahead=a)
                    tick, fin = [], []
                    k = 0
                    for rep in range(max(args.ticks // 8, 4) + 1):
                        for _ in range(8):
                            t0 = time.perf_counter()
                            s.push(px[k % total])
                            torch.cuda.synchronize()
                            tick.append(time.perf_counter() - t0)
                            k += 1
                        t0 = time.perf_counter()
                        s.finish()
                        torch.cuda.synchronize()
                        fin.append(time.perf_counter() - t0)
                    s.check_range()
                    s.close()
                    tick, fin = np.asarray(tick[8:]), np.asarray(fin[1:])
                    row = dict(config=name, mask_stride=ms, slots=T, lookahead=a, finishes=len(fin), graph_us=round(1e6 * float(np.median(tick)), 1),
                               finish_us=round(1e6 * float(np.median(fin)), 1), finish_p90_us=round(1e6 * float(np.percentile(fin, 90)), 1))
                    row["finish_over_tick"] = round(row["finish_us"] / row["graph_us"], 2)
                    row["finish_per_drain_tick_us"] = round(row["finish_us"] / a, 1)
                    row["device"] = torch.cuda.get_device_name(0)
                    print(json.dumps(row), flush=True)
                    results.append(row)
                continue
            row = dict(config=name, mask_stride=ms, slots=T, lookahead=args.lookahead, ticks=args.ticks)
            variants = (("graph", lambda: session(True)), ("no_graph", lambda: session(False)), ("baseline", baseline))
            if args.fps is not None:
                la = max(args.lookahead, stream.rate_plan(cfg, args.fps, None, ms).min_lookahead)
                plan = stream.rate_plan(cfg, args.fps, la, ms)
                row.update(fps=args.fps, lookahead=la, model_lookahead=plan.a_m, sub_ticks_per_push=round(plan.A / plan.B, 4))
                variants = (("fps_graph", lambda: session(True, fps=args.fps, lookahead=la)), ("graph", lambda: session(True)))
                if args.out_fps is not None:
                    out_plan = stream.rate_plan(cfg, args.fps, la, ms, out_fps=args.out_fps)
                    row.update(out_fps=args.out_fps, max_out=out_plan.max_out, key_ring=out_plan.D)
                    variants = (("out_fps_graph", lambda: session(True, fps=args.fps, out_fps=args.out_fps, lookahead=la)),) + variants
                if args.interpolation == "cubic":
                    cubic_la = max(args.lookahead, stream.rate_plan(cfg, args.fps, None, ms, out_fps=args.out_fps, interpolation="cubic").min_lookahead)
                    cubic_plan = stream.rate_plan(cfg, args.fps, cubic_la, ms, out_fps=args.out_fps, interpolation="cubic")
                    row.update(interpolation="cubic", cubic_lookahead=cubic_la, cubic_model_lookahead=cubic_plan.a_m, cubic_key_ring=cubic_plan.D)
                    variants = (("cubic_graph", lambda: session(True, fps=args.fps, lookahead=cubic_la, interpolation="cubic",
                                                                **({} if args.out_fps is None else {"out_fps": args.out_fps}))),) + variants
            if args.repair_joints is not None:
                row.update(repair_joints=args.repair_joints, missing_joints=args.missing_joints,
                           staged_frames=stream.staged_frames(args.repair_joints, ms))
                variants = (("repair_graph", lambda: session(True, valid=seen, repair_joints=args.repair_joints)),
                            ("md_graph", lambda: session(True, valid=seen.all(axis=2), missed_detections=True)))
            if args.detections is not None:
                variants = detections_variants()
            if args.camera is not None or args.smooth or args.bones or args.rotations:
                variants = camera_variants()
            if args.views is not None:
                variants = views_variants()
            for key, fn in variants:
                ts = np.asarray(fn())
                row[key + "_us"] = round(1e6 * float(np.median(ts)), 1)
                row[key + "_p90_us"] = round(1e6 * float(np.percentile(ts, 90)), 1)
            if args.views is not None:
                row["views_minus_world_us"] = round(row["views_graph_us"] - row["world_graph_us"], 1)
            elif args.smooth:
                row["smooth_minus_graph_us"] = round(row["smooth_graph_us"] - row["graph_us"], 1)
            elif args.bones:
                row["bones_minus_graph_us"] = round(row["bones_graph_us"] - row["graph_us"], 1)
            elif args.rotations:
                row["rotations_minus_graph_us"] = round(row["rotations_graph_us"] - row["graph_us"], 1)
            elif args.distortion is not None:
                row["distortion_minus_camera_us"] = round(row["distortion_graph_us"] - row["camera_graph_us"], 1)
            elif args.extrinsics is not None:
                row["world_minus_camera_us"] = round(row["world_graph_us"] - row["camera_graph_us"], 1)
            elif args.camera is not None:
                row["camera_minus_graph_us"] = round(row["camera_graph_us"] - row["graph_us"], 1)
            elif args.detections is not None:
                row["det_minus_md_us"] = round(row["det_graph_us"] - row["md_graph_us"], 1)
            elif args.repair_joints is not None:
                row["repair_minus_md_us"] = round(row["repair_graph_us"] - row["md_graph_us"], 1)
            elif args.fps is None:
                row["speedup_vs_baseline"] = round(row["baseline_us"] / row["graph_us"], 2)
            else:
                row["push_over_model_tick"] = round(row["fps_graph_us"] / row["graph_us"], 2)
                if args.out_fps is not None:
                    row["out_fps_minus_fps_us"] = round(row["out_fps_graph_us"] - row["fps_graph_us"], 1)
                if args.interpolation == "cubic":
                    row["cubic_minus_linear_us"] = round(row["cubic_graph_us"] - row["fps_graph_us" if args.out_fps is None else "out_fps_graph_us"], 1)
            row["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(row), flush=True)
            results.append(row)
        del model
    return results


if __name__ == "__main__":
    main()
