"""UE4M4 storage of captured self-attention maps (FZ_ATTN_CAPTURE8U / FZ_ATTN_INJECT8U, AttentionStore(map_dtype="ue4m4")): cases shared by the
CPU-emulation suite (tests/test_map8u_emu.py) and the MI355X suite (tests/test_map8u_gpu.py).

The format: a probability's fp16 bit pattern h is <= 0x3C00, the stored byte is (h + 0x1F + ((h >> 6) & 1)) >> 6 -- bits 13..6, rounded to
nearest-even -- and byte b stands for the half b << 6.  Kernel level: the 8-bit launches are checked against the fp16 launches of the SAME inputs
bit for bit, as tests/map8_cases.py does for E5M2; each case computes its launches once (`kernel_case`, cached)."""
import functools

import torch

from fatezero_amd import kernels as K

import kernel_cases as KC
import map8_cases as M

# (d, lq, lkf, index_list, clip).  The five shapes of the E5M2 suite, and the smallest at which a paired store (two 64-key tiles of a kv slot
# leaving as one 128-byte row segment: csrc/attn_self.hip keeps that form selectable, whichever form the library ships runs here) can go wrong,
# each with two kv slots: exactly one pair per slot (128), a pair plus a lone tile (192: three
# tiles per slot, so the second slot's tiles have the other parity in the launch's running tile count), a pair plus a 16-key partial tile
# (144; with 144 queries: a query tail under the paired flush).
KERNEL_CASES = dict(M.KERNEL_CASES)
KERNEL_CASES.update({
    "d40_lq64_lkf128_one_pair": (40, 64, 128, [-1, "first"], 2),
    "d80_lq64_lkf192_pair_and_lone": (80, 64, 192, [-1, "first"], 2),
    "d64_lq64_lkf144_pair_and_partial": (64, 64, 144, [-1, "first"], 2),
    "d40_lq144_lkf144_pair_and_partial": (40, 144, 144, [-1, "first"], 2),
})
REAL_16x16 = M.REAL_16x16
HEADS = M.HEADS
SENTINEL = M.SENTINEL
TOP_BYTE = 0xF0  # 1.0


def formula(bits):
    """The rounding of include/fatezero_hip.h on fp16 bit patterns (any integer tensor)."""
    return (bits + 0x1F + ((bits >> 6) & 1)) >> 6


@functools.lru_cache(maxsize=None)
def kernel_case(name, device, heads=HEADS):
    d, lq, lkf, index_list, clip = KERNEL_CASES[name] if name in KERNEL_CASES else REAL_16x16[1]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    batch = 2  # the second half of the batch is the controlled one (frame0 != 0), as in a CFG edit
    n, c = batch * clip, heads * d
    q = KC._mk((n, lq, c), g, device, 1.5)
    k = KC._mk((n, lkf, c), g, device, 1.5)
    v = KC._mk((n, lkf, c), g, device)
    vt = K.transpose_pad(v, K.pad64(lkf))
    n_kv = max(1, len(index_list))
    lk = n_kv * lkf
    kw = dict(clip_len=clip, heads=heads, index_list=index_list, frame0=clip, n_frames=clip, p_frame_off=1)  # p frame 0 is never touched

    def out():
        o = torch.full((n, lq, c), float("nan"), dtype=torch.float16, device=device)
        K.attn_self(q, k, vt, o, clip_len=clip, heads=heads, index_list=index_list, mode=K.FZ_ATTN_FLASH, frame0=0, n_frames=clip)
        return o

    r = dict(d=d, lq=lq, lkf=lkf, clip=clip, heads=heads, n=n, lk=lk)
    p16 = torch.full((clip + 1, heads, lq, lk), float("nan"), dtype=torch.float16, device=device)
    r["o_cap16"] = K.attn_self(q, k, vt, out(), mode=K.FZ_ATTN_CAPTURE, p=p16, **kw)
    p8 = torch.full((clip + 1, heads, lq, lk), SENTINEL, dtype=torch.uint8, device=device)
    r["o_cap8"] = K.attn_self(q, k, vt, out(), mode=K.FZ_ATTN_CAPTURE8U, p=p8, **kw)
    r["p16"], r["p8"] = p16, p8
    # the 8-bit inject on the bytes, the fp16 inject on the fp16 tensor that holds the same values
    deq = K.ue4m4_to_half(p8)
    r["deq"] = deq
    r["mask"] = M._split_mask(clip, lq, device)
    for tag, mask in (("all_stored", None), ("split", r["mask"])):
        kk = k if (mask is not None or lkf != lq) else None  # (without k the wrapper takes lkf = lq; with no mask the kernel never reads it)
        r["o_inj8_" + tag] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT8U, p=p8, row_mask=mask, **kw)
        r["o_inj16_" + tag] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT, p=deq, row_mask=mask, **kw)
    # every byte value 0x00 .. 0xF0 in one map (INJECT does not ask for normalised rows)
    pall = ((torch.arange(p8.numel(), dtype=torch.int64) * 7) % (TOP_BYTE + 1)).to(torch.uint8).reshape(p8.shape).to(device)
    kk = k if lkf != lq else None
    r["p_all"] = pall
    r["o_inj8_all_bytes"] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT8U, p=pall, **kw)
    r["o_inj16_all_bytes"] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT, p=K.ue4m4_to_half(pall), **kw)
    r["qkv"] = (q, k, v, index_list)
    return r


def check_capture_bytes(r):
    p16, p8 = r["p16"].cpu(), r["p8"].cpu()
    assert torch.isfinite(p16[1:].float()).all()
    want = K.half_to_ue4m4(p16[1:])
    assert torch.equal(want.to(torch.int32), formula(p16[1:].contiguous().view(torch.int16).to(torch.int32)))
    assert torch.equal(p8[1:], want), int((p8[1:] != want).sum())
    assert int(p8[1:].max()) <= TOP_BYTE
    assert (p8[0] == SENTINEL).all(), "frame 0 of the map lies in front of p_frame_off: never written"
    assert torch.equal(r["o_cap8"].cpu(), r["o_cap16"].cpu()), "the launch's own output must not depend on the storage format"
    # what the rounding costs, reported: at most 2^-5 relative (4 of 10 mantissa bits kept), half a UE4M4 subnormal step below 2^-14
    rel = ((K.ue4m4_to_half(p8[1:]).float() - p16[1:].float()).abs() / p16[1:].float().clamp_min(2.0 ** -14)).max()
    assert float(rel) <= 2.0 ** -5, float(rel)
    return float(rel)


def check_inject_same_bits(r):
    M.check_inject8_same_bits(r)  # all-stored and split mask, bit for bit; the mask splits every 32-row slice
    a, b = r["o_inj8_all_bytes"].cpu(), r["o_inj16_all_bytes"].cpu()
    assert sorted(set(r["p_all"][1:].flatten().tolist())) == list(range(TOP_BYTE + 1))
    assert torch.isfinite(a.float()).all() and torch.equal(a, b), float((a.float() - b.float()).abs().max())


def check_inject_vs_fp32(r):
    return M.check_inject8_vs_fp32(r)  # the fp32 restatement on r["deq"], 4e-3 . max


# ---------------------------------------------------------------------------------------------------------------
# whole jobs
# ---------------------------------------------------------------------------------------------------------------
WHOLE_JOB = "map8u_tiny40_4f"


@functools.lru_cache(maxsize=None)
def whole_job(device, map_dtype, oracle_device=None, fp32_leg=True):
    """map8_cases.WHOLE_JOB_CASE (tiny40, 4 frames, 64^2 latents, T = 4 + 4, Replace + blend-masked self-attention, split regime) through
    pipeline_cases.run_geometry_case on a pipeline built with `map_dtype`.  Returns run_geometry_case's result dict (fp32_leg=False: without
    the all-fp32 edit leg)."""
    import pipeline_cases as PC
    PC.GEOMETRY_CASES[WHOLE_JOB] = M.WHOLE_JOB_CASE
    orig, made = PC.P2pDDIMSpatioTemporalPipeline, []

    def build(*a, **k):
        made.append(orig(*a, map_dtype=map_dtype, **k))
        return made[-1]
    PC.P2pDDIMSpatioTemporalPipeline = build
    try:
        res = PC.run_geometry_case(WHOLE_JOB, device, oracle_device=oracle_device, fp32_leg=fp32_leg)
    finally:
        PC.P2pDDIMSpatioTemporalPipeline = orig
        del PC.GEOMETRY_CASES[WHOLE_JOB]
    store = made[0].store_controller
    assert len(made) == 1 and store.map_dtype == map_dtype and len(store.attention_store_all_step) == M.WHOLE_JOB_CASE["T"], (len(made), map_dtype)
    self_maps = store.maps_of_step(0)["down_self"]
    assert self_maps and all(cm.fmt == map_dtype and cm.is_8bit == (map_dtype != "fp16") for cm in self_maps)
    made[0].release_attention_maps()
    return res


def full_width_job(device, map_dtype, kind="tiny16", frames=4, L=16, T=2, seed=7):
    """The tiny job with EVERY self-attention row taking the stored map: capture inversion, then a Replace edit whose self window covers all T
    steps, without blend words -- the launches get no row mask, which is what a blend threshold above 1 amounts to (no row keeps the live
    attention); the blender itself needs the five 16 x 16 cross maps of 64^2 latents, which these tiny latents do not have.  Returns
    (inverted latents, edited latents, fraction of rows that kept the live attention)."""
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    unet = PC.build_unet(kind, {"lora": 16}, device)
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                         map_dtype=map_dtype)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(2, 77, 64, generator=g).to(device)
    pipe._encode_prompt = lambda *a, **k: emb
    z0 = torch.randn(1, 4, frames, L, L, generator=g).to(device)
    pipe.scheduler.set_timesteps(T)
    lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True,
                                             LOW_RESOURCE=True, latents=z0)
    assert pipe.store_controller.map_dtype == map_dtype
    out = pipe(prompt="a red car", source_prompt="a blue car", edit_type="swap", num_inference_steps=T, latents=lat[-1], output_type="latent",
               cross_replace_steps={"default_": 0.5}, self_replace_steps=1.0, use_inversion_attention=True, is_replace_controller=True,
               save_self_attention=False, guidance_scale=3.0)
    ctrl = pipe.last_edit_controller
    assert ctrl.attention_blend is None and tuple(ctrl.num_self_replace) == (0, T), ctrl.num_self_replace
    live = 0.0
    edited = out["sdimage_output"].images.float().cpu()
    pipe.release_attention_maps()
    return [x.float().cpu() for x in lat], edited, live


def finer_than_e5m2(device, **kw):
    """full_width_job in all three formats: deviation of the 8-bit jobs' edited latents from the fp16-arena job's.  Returns the figures; the one
    requirement (the issue's): rms(ue4m4) < rms(e5m2)."""
    runs = {fmt: full_width_job(device, fmt, **kw) for fmt in ("fp16", "e5m2", "ue4m4")}
    ref = runs["fp16"][1]
    scale = float(ref.abs().max())
    out = {"latent_scale": scale, "live_rows_fraction": runs["fp16"][2]}
    for fmt in ("e5m2", "ue4m4"):
        for a, b in zip(runs["fp16"][0], runs[fmt][0]):
            assert torch.equal(a, b)  # the inversion does not see the format
        assert torch.isfinite(runs[fmt][1]).all() and runs[fmt][2] == 0.0
        diff = (runs[fmt][1] - ref).abs()
        out[fmt] = {"max_over_scale": float(diff.max()) / scale, "rms_over_scale": float(diff.pow(2).mean().sqrt()) / scale}
    out["rms_ratio_e5m2_over_ue4m4"] = out["e5m2"]["rms_over_scale"] / max(out["ue4m4"]["rms_over_scale"], 1e-30)
    out["max_ratio_e5m2_over_ue4m4"] = out["e5m2"]["max_over_scale"] / max(out["ue4m4"]["max_over_scale"], 1e-30)
    print("full-width job, 8-bit arenas against the fp16 arena:", out)
    assert runs["fp16"][2] == 0.0, "every row takes the stored map"
    assert out["e5m2"]["rms_over_scale"] > 0.0, "the job does read the stored maps"
    assert out["ue4m4"]["rms_over_scale"] < out["e5m2"]["rms_over_scale"], out
    return out
