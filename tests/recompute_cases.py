"""`recompute_maps` (P2pDDIMSpatioTemporalPipeline(..., recompute_maps=True): the inversion keeps latents instead of attention maps, every edit
step re-runs the inversion forward it reads into a one-step slab): the jobs shared by the CPU-emulation suite
(tests/test_recompute_maps_emu.py, tests/test_recompute_maps_gloo.py) and the MI355X suite (tests/test_recompute_maps_gpu.py).

Every comparison is between two runs of THIS engine on the same inputs -- the recomputed job against its resident twin -- and is bit for bit:
the recompute pass issues the launches of the inversion forward on the bytes the inversion forward read.  A resident run is computed once per
(job, device) and shared (`job`, cached); nothing modifies what it returns."""
import functools
import glob
import os

import numpy as np
import torch

from helpers import ReplayTokenizer, load_json

import pipeline_cases as PC
from fatezero_amd import kernels as K
from fatezero_amd.video_diffusion.models import unet_3d_condition as U
from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
from fatezero_amd.video_diffusion.schedulers import DDIMScheduler

SPLIT_BAND = PC.FULL_MASK_BAND  # what the harness asks of a blend threshold that "splits the rows": 20-80 % of the mask on either side

# One edit: (prompt case of tests/golden/host_constants.json, Replace?, equalizer, blend words).  Both share the source prompt.
EDITS = {
    "replace": dict(prompt_case="teaser_posche", is_replace=True, eq_params=None, blend_words=[["silver", "jeep"], ["Porsche", "car"]]),
    # Refine + Reweight: the target prompt is three words longer than the source
    "refine_reweight": dict(prompt_case="teaser_watercolor", is_replace=False, eq_params={"words": ["watercolor"], "values": [10]},
                            blend_words=[["jeep"], ["jeep"]]),
}
# The core job of the emulator suite.  40^2 latents, not 16^2: the blend masks are built from `down_cross[2:4] + up_cross[:3]`
# (spatial_blend.py: by list position), which are maps of ONE level only when the first UNet level is above the 32^2-token capture limit
# -- 40^2 is the smallest latent of a side divisible by 8 for which that holds (levels 1600 / 400 / 100 / 25 tokens: none a multiple of
# the 128-row query tile or the 64-key tile, 13 / 4 / 1 / 1 query tiles per head).
EMU = dict(kind="tiny16", F=4, L=40, T=4, model_config={"lora": 16})
# tests/test_map8_gpu.py's tiny job (map8_cases.WHOLE_JOB_CASE) for the MI355X suite
GPU = dict(kind="tiny40", F=4, L=64, T=4, model_config={"lora": 16})


def _inputs(geo, seed=21):
    g = torch.Generator().manual_seed(seed)
    cdim = PC.TINY[geo["kind"]]["cross_attention_dim"]
    z0 = torch.randn(1, 4, geo["F"], geo["L"], geo["L"], generator=g)
    emb_src = torch.randn(2, 77, cdim, generator=g) * 0.5
    embs = {name: emb_src + 0.25 * torch.randn(2, 77, cdim, generator=g) for name in EDITS}
    return z0, emb_src, embs


def run_job(device, geo, *, recompute, edits=("replace",), map_dtype="fp16", blend=True, blend_th=0.3, blend_latents=True, save_self_attention=False,
            shared_head=True, save_path=None, frame_shard=None, disk_store=False, z_dtype=torch.float32):
    """Inversion (with `store_attention=True`) + one edit per name in `edits`.  Returns everything the two modes must agree on."""
    old_switch, U.CFG_SHARED_HEAD = U.CFG_SHARED_HEAD, shared_head
    try:
        unet = PC.build_unet(geo["kind"], geo["model_config"], device)
        pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=ReplayTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                             map_dtype=map_dtype, recompute_maps=recompute, disk_store=disk_store)
        pipe.frame_shard = frame_shard
        pipe.set_progress_bar_config(disable=True)
        T = geo["T"]
        pipe.scheduler.set_timesteps(T)
        z0, emb_src, embs = _inputs(geo)
        src = load_json("host_constants.json")["teaser_posche"]["prompts"][0]
        lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb_src.to(device),
                                                 store_attention=True, LOW_RESOURCE=True, latents=z0.to(device=device, dtype=z_dtype),
                                                 prompt=src, save_path=save_path)
        store = pipe.store_controller
        res = {"inverted": [x.float().cpu() for x in lat], "arena_bytes_after_inversion": store.arena_bytes, "edits": {}, "pipe": pipe,
               "steps": T, "store_steps": len(store.attention_store_all_step)}
        for name in edits:
            E = EDITS[name]
            tgt = load_json("host_constants.json")[E["prompt_case"]]["prompts"][1]
            kw = dict(prompt=tgt, source_prompt=src, num_inference_steps=T, cross_replace_steps={"default_": 0.5}, self_replace_steps=0.5,
                      use_inversion_attention=True, is_replace_controller=E["is_replace"], blend_th=[blend_th, blend_th],
                      save_self_attention=save_self_attention, guidance_scale=7.5, blend_words=E["blend_words"] if blend else None,
                      blend_self_attention=blend, blend_latents=blend_latents and blend)
            if E["eq_params"] is not None:
                kw["eq_params"] = E["eq_params"]
            pipe._encode_prompt = lambda *a, _e=embs[name], **k: _e.to(device)
            out = pipe(latents=lat[-1], edit_type="swap", output_type="latent", **kw)
            ctrl = pipe.last_edit_controller
            strips = out["attention_output"]
            r = {"latents": out["sdimage_output"].images.float().cpu(),
                 "attention_masks": [] if ctrl.attention_blend is None else [m.cpu() for m in ctrl.attention_blend.mask_list],
                 "mask_list": None if out["mask_list"] is None else [m.cpu() for m in out["mask_list"]],
                 "applied_masks": [] if ctrl.latent_blend is None else [m.cpu() for m in ctrl.latent_blend.applied_mask_list],
                 "attention_output": None if strips is None else [np.asarray(s) for s in strips]}
            ml = r["attention_masks"]
            r["mask_ones_frac"] = float(sum(float(m.float().sum()) for m in ml) / max(1, sum(m.numel() for m in ml)))
            res["edits"][name] = r
        res["arena_bytes"] = store.arena_bytes
        res["issue_stats"] = None if unet._issuer is None else dict(unet._issuer.stats)
        return res
    finally:
        U.CFG_SHARED_HEAD = old_switch


@functools.lru_cache(maxsize=None)
def job(device, geo_name, recompute, **kw):
    """`run_job` computed once per argument set (keyword values hashable: edits as a tuple)."""
    return run_job(device, {"emu": EMU, "gpu": GPU}[geo_name], recompute=recompute, **kw)


def assert_same_edit(a, b, what=""):
    """Two runs' edits: latents, every blend mask, `mask_list`, `attention_output` -- torch.equal / array_equal."""
    assert list(a["edits"]) == list(b["edits"])
    for x, y in zip(a["inverted"], b["inverted"]):
        assert torch.equal(x, y), (what, "inverted latents")
    for name in a["edits"]:
        ea, eb = a["edits"][name], b["edits"][name]
        assert torch.isfinite(ea["latents"]).all()
        assert torch.equal(ea["latents"], eb["latents"]), (what, name, float((ea["latents"] - eb["latents"]).abs().max()))
        for field in ("attention_masks", "mask_list", "applied_masks"):
            la, lb = ea[field], eb[field]
            assert (la is None) == (lb is None) and (la is None or len(la) == len(lb)), (what, name, field)
            for i, (m, n) in enumerate(zip(la or [], lb or [])):
                assert torch.equal(m, n), (what, name, field, i)
        sa, sb = ea["attention_output"], eb["attention_output"]
        assert (sa is None) == (sb is None) and (sa is None or len(sa) == len(sb)), (what, name, "attention_output")
        for i, (m, n) in enumerate(zip(sa or [], sb or [])):
            assert np.array_equal(m, n), (what, name, "attention_output", i)


def assert_arena_is_one_step(rec, res, slabs=1):
    """arena_bytes of the recomputed job == the resident job's / its step count x the slab count.  One slab: attention reads store step
    n - 1 - i at edit step i (`_step_in_store`), and the latent blend's own `sis` in step_callback is the same n - 1 - i."""
    assert res["store_steps"] == rec["store_steps"] == res["steps"]
    assert res["arena_bytes"] % res["steps"] == 0
    assert rec["arena_bytes"] == res["arena_bytes"] // res["steps"] * slabs, (rec["arena_bytes"], res["arena_bytes"], res["steps"])
    assert rec["arena_bytes_after_inversion"] == rec["arena_bytes"], "the inversion captures into the slab the edit recomputes into"


def assert_split(r, name="replace"):
    lo, hi = SPLIT_BAND
    assert lo <= r["edits"][name]["mask_ones_frac"] <= hi, r["edits"][name]["mask_ones_frac"]


def png_bytes(folder):
    """The pictures under `folder`, as arrays in the order of their relative paths' sort by directory (file names carry a time stamp)."""
    from PIL import Image
    out = []
    for root, _, files in sorted(os.walk(folder)):
        for f in sorted(files):
            if f.endswith(".png"):
                out.append(np.asarray(Image.open(os.path.join(root, f))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# fz_latent_tokens
# ---------------------------------------------------------------------------------------------------------------------------------------
LATENT_TOKEN_SHAPES = [(1, 64), (3, 64), (8, 64), (1, 15), (3, 15), (8, 15)]  # (F, h*w): one block / several, a token count that is odd


def check_latent_tokens(device, frames, hw, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * frames + hw)
    z = (torch.randn(4, frames, hw, generator=g) * 3.0)
    # values that only round-to-nearest-even gets right in fp16: exact ties between two halves (odd multiples of 2^-11 around 1.0) and
    # a value just below the largest finite half
    z.view(-1)[:4] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 65504.0 - 8.0])
    z = z.to(dtype).to(device)
    want = z.permute(1, 2, 0).to(torch.float16).contiguous()
    out = torch.full((frames + 1, hw, 4), 7.0, dtype=torch.float16, device=device)  # one frame of canary behind the output
    got = K.latent_tokens(z, out=out[:frames])
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out[:frames].cpu(), want.cpu()), (frames, hw, dtype)
    assert (out[frames] == 7.0).all(), "wrote past the last token"
    assert torch.equal(K.latent_tokens(z).cpu(), want.cpu())


def check_latent_tokens_bad_args(device):
    import ctypes as C
    from fatezero_amd import _native as N
    L = N.lib()
    z = torch.zeros(4, 2, 16, dtype=torch.float32, device=device)
    o = torch.zeros(2, 16, 4, dtype=torch.float16, device=device)
    zp, op, st = C.c_void_p(z.data_ptr()), C.c_void_p(o.data_ptr()), C.c_void_p(0)
    bad = N.FZ_ERR_BAD_ARG
    assert L.fz_latent_tokens(None, N.FZ_LATENT_F32, op, 2, 16, st) == bad
    assert L.fz_latent_tokens(zp, N.FZ_LATENT_F32, None, 2, 16, st) == bad
    assert L.fz_latent_tokens(zp, 2, op, 2, 16, st) == bad           # a z_dtype that is neither
    assert L.fz_latent_tokens(zp, -1, op, 2, 16, st) == bad
    assert L.fz_latent_tokens(zp, N.FZ_LATENT_F32, op, 0, 16, st) == bad
    assert L.fz_latent_tokens(zp, N.FZ_LATENT_F32, op, 2, 0, st) == bad
    assert L.fz_latent_tokens(zp, N.FZ_LATENT_F32, op, -2, 16, st) == bad
    assert L.fz_latent_tokens(zp, N.FZ_LATENT_F32, C.c_void_p(o.data_ptr() + 2), 1, 16, st) == bad   # tokens not 8-byte aligned
    assert L.fz_latent_tokens(C.c_void_p(z.data_ptr() + 2), N.FZ_LATENT_F32, op, 1, 16, st) == bad   # fp32 latent not 4-byte aligned
    assert L.fz_latent_tokens(C.c_void_p(z.data_ptr() + 1), N.FZ_LATENT_F16, op, 1, 16, st) == bad   # fp16 latent not 2-byte aligned
    assert L.fz_latent_tokens(op, N.FZ_LATENT_F16, op, 2, 16, st) == bad                               # in place
    assert (o == 0).all()
    # the wrapper refuses what it can see before the library does
    import pytest
    for zz, oo in ((z[:3], None), (z.double(), None), (z.permute(0, 2, 1), None), (z, torch.zeros(2, 16, 4, device=device)),
                   (z, torch.zeros(2, 15, 4, dtype=torch.float16, device=device)), (z, torch.zeros(17, 16, 4, dtype=torch.float16, device=device)[1::8])):
        with pytest.raises(ValueError, match="fz_latent_tokens"):
            K.latent_tokens(zz, out=oo)


def glob_count(folder, pattern):
    return len(glob.glob(os.path.join(folder, pattern), recursive=True))
