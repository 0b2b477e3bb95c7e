#!/usr/bin/env python3
"""Time one FateZero job on an SD-2-base-shaped UNet on one MI355X and print ONE JSON line with the fields of bench.py's plain line.

The job is bench.py's (jeep -> Porsche, capture inversion + 1 CFG edit with Replace and blend-masked self-attention, 8 frames x 512^2
x (50 + 50) DDIM steps by default, latents in / out) with only the model swapped: SD-2-base's UNet (320/640/1280/1280, heads 5/10/20/20
of 64, Linear proj_in / proj_out, a 1024-wide text context) with procedural weights, and a 1024-wide hash text encoder.  The line also
records the map arena it reserved (`arena_step_bytes` x `arena_steps`).  bench.py itself is imported, not changed.

    python scripts/sd2_job.py --steps 2 --warmup 1
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

SD2_BASE = dict(sample_size=64, in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                cross_attention_dim=1024, attention_head_dim=(5, 10, 20, 20), norm_num_groups=32, use_linear_projection=True)


def build_sd2_pipeline(device, seed=0, model_config=None):
    from fatezero_amd.synthetic import HashTextEncoder, WordTokenizer, init_like_tuned_checkpoint
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    torch.manual_seed(seed)
    with torch.device(device):
        unet = UNetPseudo3DConditionModel(**SD2_BASE, **(model_config or {"lora": 160}))
    init_like_tuned_checkpoint(unet, seed)
    unet = unet.half().eval()
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=HashTextEncoder(1024).to(device), tokenizer=WordTokenizer(),
                                         unet=unet, scheduler=DDIMScheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1, help="timed jobs")
    ap.add_argument("--warmup", type=int, default=1, help="untimed warm-up jobs")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--latent-size", type=int, default=64)
    ap.add_argument("--model", choices=["sd2", "sd1"], default="sd2",
                    help="sd1: bench.py's SD-1.x pipeline through the same timing code (the comparison line, with its arena's step bytes)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sd2_job.py measures the MI355X path; there is no CPU fallback"
    device = torch.device("cuda", 0)
    pipe = build_sd2_pipeline(device) if args.model == "sd2" else bench.build_pipeline(device)
    L = args.latent_size
    z0 = torch.randn(1, 4, args.frames, L, L, generator=torch.Generator().manual_seed(1234)).to(device)
    for _ in range(args.warmup):
        bench.run_job(pipe, z0, args.ddim_steps, device)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    edited = None
    for i in range(args.steps):
        edited = bench.run_job(pipe, z0, args.ddim_steps, device)
        marks[i + 1].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    per_job_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    arena = pipe.store_controller.arena
    px = 8 * L
    line = {"metric": f"edited frames/sec ({args.frames}f x {px}^2 x {args.ddim_steps} DDIM steps: capture inversion + 1 CFG edit, "
                      "latents in/out), " + ("SD-2-base" if args.model == "sd2" else "SD-1.x") + " UNet",
            "value": args.frames * args.steps / dt, "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "fp16", "data": "synthetic",
            "config": {"workload": f"config/teaser/jeep_posche.yaml shape: {args.frames} x {px}x{px} (latents {args.frames}x{L}x{L}x4), "
                                   f"{args.ddim_steps}-step DDIM inversion with HBM map capture + {args.ddim_steps}-step CFG edit (Replace, "
                                   "blend-masked self-attention), " + ("SD-2-base pseudo-3D UNet (heads 5/10/20/20 x 64, linear projections, "
                                   "1024-wide context)" if args.model == "sd2" else "SD-1.x pseudo-3D UNet") + " lora=160, random-init weights",
                       "frames": args.frames, "ddim_steps": args.ddim_steps, "n_edit": 1, "parallelism": "single GPU",
                       "arena_GB": pipe.store_controller.arena_bytes / 1e9, "arena_step_bytes": arena.step_bytes,
                       "arena_steps": (0 if arena.reserved is None or not arena.step_bytes else arena.reserved.numel() // arena.step_bytes),
                       "outputs_finite": bool(torch.isfinite(edited.float()).all()), "n_ranks_seen": 1},
            "roofline": None, "rooflines": None, "cpu_baseline": None,
            "ms_per_step_spread": {"min": per_job_ms[0], "median": per_job_ms[len(per_job_ms) // 2], "max": per_job_ms[-1],
                                   "jobs": len(per_job_ms),
                                   "how": "HIP events at the job boundaries of the timed region (launch stream, no sync inside)"}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
