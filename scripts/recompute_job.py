#!/usr/bin/env python3
"""Same-process A/B of bench.py's job with the inversion's attention maps resident (one slab per DDIM step) and recomputed
(`recompute_maps=True`: one slab, every edit step re-runs the inversion forward it reads): one JSON line with the time of each job,
`arena_bytes` of each store and `torch.equal` of the edited latents, also written to profiles/recompute_job.json.

The job is bench.py's (jeep -> Porsche, capture inversion + 1 CFG edit with Replace and blend-masked self-attention, 8 frames x 512^2 x
(50 + 50) DDIM steps by default, latents in / out); bench.py itself is imported, not changed.

    python scripts/recompute_job.py --ddim-steps 50 --jobs 2 [--map-dtype e5m2] [--blend-th 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

MODES = ("resident", "recompute")


def run_job(pipe, z0, ddim_steps, device, recompute, blend_th=None):
    """bench.run_job's job (capture inversion + the Porsche edit) in the given mode."""
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import MapArena
    pipe.scheduler.set_timesteps(ddim_steps)
    pipe.release_attention_maps()
    if recompute != pipe.recompute_maps:
        MapArena.reset_pools()  # the resident job's recycled block must not be counted into (or held under) the one-step job
        pipe.set_recompute_maps(recompute)
    emb_src = pipe._encode_prompt(bench.SRC_PROMPT, device, 1, True, None)
    lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb_src,
                                             store_attention=True, LOW_RESOURCE=True, latents=z0)
    kw = bench.EDIT_KW if blend_th is None else dict(bench.EDIT_KW, blend_th=[blend_th, blend_th])
    out = pipe(prompt=bench.TGT_PROMPT, source_prompt=bench.SRC_PROMPT, edit_type="swap", num_inference_steps=ddim_steps,
               latents=lat[-1], output_type="latent", **kw)
    return out["sdimage_output"].images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=2, help="timed jobs per mode (after one untimed warm-up job each), alternating")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--latent-size", type=int, default=64)
    ap.add_argument("--map-dtype", default="fp16", choices=("fp16", "e5m2", "ue4m4"))
    ap.add_argument("--blend-th", type=float, default=None, help="blend threshold of the edit (default: the config's 0.3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute_job.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "recompute_job.py measures the MI355X path; there is no CPU fallback"
    device = torch.device("cuda", 0)
    pipe = bench.build_pipeline(device)
    pipe.set_map_dtype(args.map_dtype)
    L = args.latent_size
    z0 = torch.randn(1, 4, args.frames, L, L, generator=torch.Generator().manual_seed(1234)).to(device)
    res = {m: {"ms": []} for m in MODES}
    for m in MODES:
        run_job(pipe, z0, args.ddim_steps, device, m == "recompute", args.blend_th)  # warm-up: allocations, weight packs
    for _ in range(max(1, args.jobs)):
        for m in MODES:  # (alternating: clocks drift over minutes)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            edited = run_job(pipe, z0, args.ddim_steps, device, m == "recompute", args.blend_th)
            e1.record()
            torch.cuda.synchronize()
            res[m]["ms"].append(e0.elapsed_time(e1))
            res[m]["edited"] = edited.float().cpu()
            res[m]["arena_bytes"] = int(pipe.store_controller.arena_bytes)
            res[m]["arena_step_bytes"] = int(pipe.store_controller.arena.step_bytes)
    a, b = res["resident"].pop("edited"), res["recompute"].pop("edited")
    line = {"job": f"{args.frames}f x {8 * L}^2 x {args.ddim_steps} + {args.ddim_steps} DDIM steps (bench.py's job)", "map_dtype": args.map_dtype,
            "blend_th": args.blend_th, "stored_rows_fraction": bench.stored_rows_fraction(pipe), "resident": res["resident"],
            "recompute": res["recompute"], "arena_ratio": res["recompute"]["arena_bytes"] / res["resident"]["arena_bytes"],
            "time_ratio_recompute_over_resident": min(res["recompute"]["ms"]) / min(res["resident"]["ms"]),
            "edited_equal": bool(torch.equal(a, b)), "edited_max_abs_diff": float((a - b).abs().max()),
            "outputs_finite": bool(torch.isfinite(a).all() and torch.isfinite(b).all())}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
