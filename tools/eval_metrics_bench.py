"""The evaluation report on the host (evaluation.evaluate_predictions, float64 numpy) against the device
(evaluation_device.evaluate_predictions_device, csrc/uu3d_metrics.h), both from device-resident predictions to the finished dict, on
synthetic input of the size of the Human3.6M test split at 50 Hz (543 344 poses, 17 joints, SEQUENCE_STRIDE 5, TEST_STRIDED_EVAL);
alternating runs, medians.  Then run_eval's own "seconds" (eval.evaluate_windows: the part of run_eval behind the dataset files -- forwards,
gather over the ranks, report) on seeded synthetic tracks as tools/eval_reuse_bench.py builds them, flag off and on alternating in one
process, with and without reuse_frames.
   timeout 900 python tools/eval_metrics_bench.py [--poses 543344] [--reps 5] [--videos 40] [--frames 2500] [--batch 512]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=543344)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--videos", type=int, default=40)
    ap.add_argument("--frames", type=int, default=2500)
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    import numpy as np, torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd import eval as ev, evaluation as E, evaluation_device as ED
    from uplift_upsample_3dhpe_amd.data import PoseTable, SequenceGenerator
    cfg = util.load_config("h36m_351")
    cfg.MASK_STRIDE = 5
    rng = np.random.default_rng(0)

    # ---- (a) the report alone ----
    P, J = args.poses, 17
    n_videos = 236
    lens = np.full(n_videos, P // n_videos); lens[:P % n_videos] += 1
    idx = np.concatenate([np.arange(n) for n in lens])
    actions = np.repeat(np.arange(n_videos) % 15, lens)
    gt3 = rng.normal(0, 0.35, size=(P, J, 3)).astype(np.float32)
    key = idx % cfg.SEQUENCE_STRIDE == 0
    pred_key = (gt3[key] * rng.uniform(0.8, 1.25, size=(int(key.sum()), 1, 1)) + rng.normal(0, 0.04, size=(int(key.sum()), J, 3))).astype(np.float32)
    rows = np.full(P, -1); rows[key] = np.arange(key.sum())
    d_pred, d_gt = torch.from_numpy(pred_key).cuda(), torch.from_numpy(gt3).cuda()

    def host():
        pred = np.zeros((P, J, 3), np.float64)
        pred[key] = d_pred.cpu().numpy().astype(np.float64)
        gt = d_gt.cpu().numpy().astype(np.float64)
        gt = gt - gt[:, cfg.ROOT_KEYTPOINT:cfg.ROOT_KEYTPOINT + 1]
        return E.evaluate_predictions(pred, gt, actions, idx, cfg)

    def device():
        return ED.evaluate_predictions_device(d_pred, d_gt, actions, idx, cfg, rows=rows)
    device(); torch.cuda.synchronize()
    th, td = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); rh = host(); th.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); rd = device(); td.append(time.perf_counter() - t0)
    # the kernels alone (ALL FRAMES pass: interpolation + metrics + sums, no error array), by events
    left, right, weight, _ = E.keyframe_plan(idx, cfg.SEQUENCE_STRIDE, rows=rows)
    dl, dr, dw, da = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (left.astype(np.int32), right.astype(np.int32), weight, actions.astype(np.int32)))
    tk = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ED.pose_errors(d_pred, d_gt, cfg.ROOT_KEYTPOINT, left=dl, right=dr, weight=dw, actions=da, num_actions=15, want_errors=False, want_sums=True); e1.record()
        e1.synchronize(); tk.append(e0.elapsed_time(e1))
    row = dict(part="report", poses=P, host_s=round(float(np.median(th)), 4), device_s=round(float(np.median(td)), 4),
               kernel_ms=round(float(np.median(tk[1:])), 4),
               max_abs_diff_mm=float(max(abs(rh["all_frames"][0][k] - rd["all_frames"][0][k]) for k in E.METRICS)))
    row["speedup"] = round(row["host_s"] / row["device_s"], 1)
    print(json.dumps(row), flush=True)

    # ---- (b) run_eval's seconds, device_metrics off and on ----
    p2 = [np.cumsum(rng.normal(0, 0.01, size=(args.frames, 17, 2)), 0).astype(np.float32) + rng.uniform(-0.5, 0.5, size=(1, 17, 2)).astype(np.float32)
          for _ in range(args.videos)]
    p3 = [rng.normal(0, 0.35, size=(args.frames, 17, 3)).astype(np.float32) for _ in range(args.videos)]
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0, perturb=0.1))
    table = PoseTable(p2, poses_3d=p3, actions=np.arange(args.videos) % 15, device=model.device)
    gen = SequenceGenerator(table, seq_len=cfg.SEQUENCE_LENGTH, stride=cfg.SEQUENCE_STRIDE, padding_type=cfg.PADDING_TYPE, flip_augment=False,
                            flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=cfg.MASK_STRIDE, stride_mask_align_global=True, shuffle=False)
    desc = gen.descriptors()
    quiet = lambda *a: None
    for reuse in (False, True):
        ev.evaluate_windows(model, gen, desc, cfg, batch_size=args.batch, reuse_frames=reuse, device_metrics=True, log=quiet)   # warm-up
        ts = {False: [], True: []}
        for _ in range(args.reps):
            for dm in (False, True):
                res = ev.evaluate_windows(model, gen, desc, cfg, batch_size=args.batch, reuse_frames=reuse, device_metrics=dm, log=quiet)
                ts[dm].append(res["seconds"])
        row = dict(part="run_eval seconds", reuse_frames=reuse, windows=res["num_windows"], forwarded=res["num_forwarded"], batch=args.batch,
                   host_metrics_s=round(float(np.median(ts[False])), 4), device_metrics_s=round(float(np.median(ts[True])), 4))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
