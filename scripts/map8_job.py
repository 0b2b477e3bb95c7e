#!/usr/bin/env python3
"""Same-process A/B of bench.py's job with the captured self-attention maps in fp16, in E5M2 (`map_dtype="e5m2"`) and in UE4M4 (`"ue4m4"`): one
JSON line with the time of each job, `arena_bytes()` of each store, and the distance of each 8-bit job's edited latents from the fp16-arena
job's, relative to the latent scale (the `edited_*` keys at the top level are the E5M2 job's, as before; `ue4m4_vs_fp16` holds the other's).

The job is bench.py's (jeep -> Porsche, capture inversion + 1 CFG edit with Replace and blend-masked self-attention, 8 frames x 512^2 x
(50 + 50) DDIM steps by default, latents in / out); bench.py itself is imported, not changed.

    python scripts/map8_job.py --ddim-steps 50 --jobs 2
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def run_job(pipe, z0, ddim_steps, device, map_dtype, blend_th=None):
    """bench.run_job's job (capture inversion + the Porsche edit) with a fresh store of the given format.  blend_th: overrides the config's
    0.3 (with bench.py's weights every self-attention row then keeps the LIVE attention and the stored self maps are never read; 2 is the
    reference's default blend: every row takes the stored map)."""
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import AttentionStore, MapArena
    pipe.scheduler.set_timesteps(ddim_steps)
    pipe.release_attention_maps()
    if map_dtype != pipe.map_dtype:
        MapArena.reset_pools()  # the other format's (larger or smaller) recycled block must not size this job's arena
    pipe.store_controller, pipe.map_dtype = AttentionStore(map_dtype=map_dtype), map_dtype
    emb_src = pipe._encode_prompt(bench.SRC_PROMPT, device, 1, True, None)
    lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb_src,
                                             store_attention=True, LOW_RESOURCE=True, latents=z0)
    kw = bench.EDIT_KW if blend_th is None else dict(bench.EDIT_KW, blend_th=[blend_th, blend_th])
    out = pipe(prompt=bench.TGT_PROMPT, source_prompt=bench.SRC_PROMPT, edit_type="swap", num_inference_steps=ddim_steps,
               latents=lat[-1], output_type="latent", **kw)
    return out["sdimage_output"].images


FORMATS = ("fp16", "e5m2", "ue4m4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1, help="timed jobs per format (after one untimed warm-up job each)")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--latent-size", type=int, default=64)
    ap.add_argument("--blend-th", type=float, default=None, help="blend threshold of the edit (default: the config's 0.3)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "map8_job.py measures the MI355X path; there is no CPU fallback"
    device = torch.device("cuda", 0)
    pipe = bench.build_pipeline(device)
    L = args.latent_size
    z0 = torch.randn(1, 4, args.frames, L, L, generator=torch.Generator().manual_seed(1234)).to(device)
    res = {}
    for fmt in (FORMATS * 2)[: len(FORMATS) if args.jobs == 1 else 2 * len(FORMATS)]:  # (interleaved: clocks drift over minutes)
        if fmt not in res:
            run_job(pipe, z0, args.ddim_steps, device, fmt, args.blend_th)  # warm-up: allocations, plans
            res[fmt] = {"ms": []}
        for _ in range(max(1, args.jobs // 2) if args.jobs > 1 else 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            edited = run_job(pipe, z0, args.ddim_steps, device, fmt, args.blend_th)
            e1.record()
            torch.cuda.synchronize()
            res[fmt]["ms"].append(e0.elapsed_time(e1))
        res[fmt]["edited"] = edited.float().cpu()
        res[fmt]["arena_bytes"] = int(pipe.store_controller.arena_bytes)
        res[fmt]["arena_step_bytes"] = int(pipe.store_controller.arena.step_bytes)
    a, b, c = res["fp16"].pop("edited"), res["e5m2"].pop("edited"), res["ue4m4"].pop("edited")
    scale = float(a.abs().max())

    def deviation(x):
        diff = (a - x).abs()
        return {"edited_max_abs_diff": float(diff.max()), "edited_max_diff_over_scale": float(diff.max()) / scale,
                "edited_q99_diff_over_scale": float(torch.quantile(diff.flatten()[:: max(1, diff.numel() // 1000000)], 0.99)) / scale,
                "edited_rms_diff_over_scale": float(diff.pow(2).mean().sqrt()) / scale}
    line = {"blend_th": args.blend_th, "stored_rows_fraction": bench.stored_rows_fraction(pipe), "job": f"{args.frames}f x {8 * L}^2 x {args.ddim_steps} + {args.ddim_steps} DDIM steps (bench.py's job)", "fp16": res["fp16"], "e5m2": res["e5m2"],
            "ue4m4": res["ue4m4"],
            "arena_ratio": res["e5m2"]["arena_bytes"] / res["fp16"]["arena_bytes"],
            "arena_ratio_ue4m4": res["ue4m4"]["arena_bytes"] / res["fp16"]["arena_bytes"],
            "time_ratio_e5m2_over_fp16": min(res["e5m2"]["ms"]) / min(res["fp16"]["ms"]),
            "time_ratio_ue4m4_over_fp16": min(res["ue4m4"]["ms"]) / min(res["fp16"]["ms"]),
            "edited_latent_scale": scale, **deviation(b), "ue4m4_vs_fp16": deviation(c),
            "outputs_finite": bool(torch.isfinite(a).all() and torch.isfinite(b).all() and torch.isfinite(c).all())}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
