"""One f16x3 forward and one exact-f32 forward (UU3D_SCHEDULE_EXACT_F32: the range fallback of model(...)) of the same batch, timed in one
process with HIP events.  Informational: the exact-f32 path is a fallback, no rate is promised for it.

    python tools/exact_f32_forward_bench.py [--config dense_351] [--batch 32] [--steps 20] [--warmup 5]

Prints one JSON line: milliseconds per forward (median over the steps) for both, and their ratio."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dense_351")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util

    cfg = util.load_config(args.config)
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0, perturb=0.05))
    x, m = util.synthetic_batch(cfg, batch=args.batch, seed=0)
    xt = torch.from_numpy(x * m[:, :, None, None].astype(np.float32)).cuda()
    mt = model._mask_u8(torch.from_numpy(m).cuda())
    B = args.batch
    full = torch.empty((B, arch.num_frames, arch.num_keypoints, 3), dtype=torch.float32, device="cuda")
    cen = torch.empty((B, arch.num_keypoints, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def time_ms(exact):
        ms = []
        for i in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            model._forward(xt, mt, full, cen, 0, stream, exact_f32=exact)
            e1.record(stream)
            e1.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        assert bool(torch.isfinite(cen).all())
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    h3, f32 = time_ms(False), time_ms(True)
    assert model.check_range(raise_error=False) is False
    print(json.dumps(dict(config=args.config, tokens=arch.num_frames, batch=B, steps=args.steps,
                          f16x3_ms=round(h3[0], 4), f16x3_ms_min_max=[round(h3[1], 4), round(h3[2], 4)],
                          exact_f32_ms=round(f32[0], 4), exact_f32_ms_min_max=[round(f32[1], 4), round(f32[2], 4)],
                          ratio=round(f32[0] / h3[0], 2))))


if __name__ == "__main__":
    main()
