"""SparseCausalAttention_index lists of five to eight entries (FZ_MAX_KV_SLOTS = 8): cases shared by the CPU-emulation suite
(tests/test_kv_slots_emu.py) and the MI355X suite (tests/test_kv_slots_gpu.py).

Kernel level: kernel_cases.case_attn_self as it stands (its fp32 reference is generic in the list; its bounds are kept: 4e-3 of the scale on O,
<= 1.6 fp16 ulp on a stored P, row sums within 3e-3); the 8-bit map properties of map8_cases / map8u_cases restated for an eight-entry list; the
frame-sharded kernel form of kernel_cases.case_sharded_pieces restated for six slots.  Pipeline level: whole tiny16 jobs of 6 frames against the
fp32 oracle (pipeline_cases.run_geometry_case, run live) and against themselves in the other storage modes (recompute_cases.run_job)."""
import functools

import torch

from fatezero_amd import kernels as K

import kernel_cases as KC
import map8_cases as M
import pipeline_cases as PC
import recompute_cases as RC

L5 = [-2, -1, "first", 1, 2]
L8 = ["first", -3, -2, -1, 1, 2, 3, "last"]
L6_TWO_QUERY_BLOCKS = [-2, -1, "mid", 1, 2, "last"]
L5_MIXED_ORDER = ["first", -1, "first", -1, "first"]  # frames 0 and 1 single-source, frames 2 and 3 not
L9 = ["first", -4, -3, -2, -1, 1, 2, 3, "last"]
LISTS = {"L5": L5, "L8": L8}

# ---------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------
# 1: lq = 100 gives every slot a padded key tail; frames 0, 1, 4, 5 of a 6-frame clip have partly coinciding slots (each contributes)
FLASH_HEAD_DIMS = [(40, True), (64, False), (80, False)]  # (d, q in the log2 domain)


def flash_case(device, index_list, d, fold):
    return KC.case_attn_self(device, batch=1, clip=6, heads=2, d=d, lq=100, index_list=index_list, mode=K.FZ_ATTN_FLASH, fold=fold)


def flash_two_query_blocks(device):
    """2: attn_flash_kernel<40, 2, 2> (lq >= 512, q in the log2 domain), the running max moving in almost every tile, slot boundaries included."""
    return KC.case_attn_self(device, batch=1, clip=3, heads=1, d=40, lq=600, index_list=L6_TWO_QUERY_BLOCKS, mode=K.FZ_ATTN_FLASH, fold=True,
                             shape="ramp")


def flash_all_slots_one_source(device):
    """3: a one-frame clip: all eight slots are frame 0, read once; 16 (head, frame) groups: the launcher's dispatch order is in use."""
    return KC.case_attn_self(device, batch=2, clip=1, heads=8, d=40, lq=64, index_list=L8, mode=K.FZ_ATTN_FLASH, fold=True)


def flash_mixed_dispatch_order(device):
    """4: single-source and full-length frames in one launch of five slots, 8 | heads."""
    return KC.case_attn_self(device, batch=2, clip=4, heads=8, d=40, lq=32, index_list=L5_MIXED_ORDER, mode=K.FZ_ATTN_FLASH, fold=True)


CAPTURE_SHAPES = [(40, 81), (80, 128)]  # (d, lq): 81 is the unaligned, element-wise map path


def capture_case(device, index_list, d, lq):
    return KC.case_attn_self(device, batch=1, clip=3, heads=2, d=d, lq=lq, index_list=index_list, mode=K.FZ_ATTN_CAPTURE)


MASK_KINDS = [None, "random", "rows"]


def inject_case(device, index_list, mask_kind):
    return KC.case_attn_self(device, batch=2, clip=3, heads=2, d=40, lq=64, index_list=index_list, mode=K.FZ_ATTN_INJECT, mask_kind=mask_kind)


# 7: 8-bit maps under the eight-entry list.  (d, lq, lkf, clip): vector paths; the element-wise path (72 % 16 != 0)
MAP8_SHAPES = {"d40_lq64": (40, 64, 64, 3), "d160_lkf72_elementwise": (160, 64, 72, 2)}
MAP8_FORMATS = {"e5m2": (K.FZ_ATTN_CAPTURE8, K.FZ_ATTN_INJECT8, K.half_to_e5m2, K.e5m2_to_half),
                "ue4m4": (K.FZ_ATTN_CAPTURE8U, K.FZ_ATTN_INJECT8U, K.half_to_ue4m4, K.ue4m4_to_half)}


@functools.lru_cache(maxsize=None)
def map8_case(name, fmt, device, heads=M.HEADS):
    """map8_cases.kernel_case / map8u_cases.kernel_case for L8: the launches of one (shape, format), computed once."""
    d, lq, lkf, clip = MAP8_SHAPES[name]
    cap8, inj8, _, decode = MAP8_FORMATS[fmt]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n, c = 2 * clip, heads * d  # the second half of the batch is the controlled one (frame0 != 0), as in a CFG edit
    q = KC._mk((n, lq, c), g, device, 1.5)
    k = KC._mk((n, lkf, c), g, device, 1.5)
    v = KC._mk((n, lkf, c), g, device)
    vt = K.transpose_pad(v, K.pad64(lkf))
    lk = len(L8) * lkf
    kw = dict(clip_len=clip, heads=heads, index_list=L8, frame0=clip, n_frames=clip, p_frame_off=1)  # p frame 0 is never touched

    def out():
        o = torch.full((n, lq, c), float("nan"), dtype=torch.float16, device=device)
        K.attn_self(q, k, vt, o, clip_len=clip, heads=heads, index_list=L8, mode=K.FZ_ATTN_FLASH, frame0=0, n_frames=clip)
        return o

    r = dict(fmt=fmt, clip=clip, lq=lq)
    p16 = torch.full((clip + 1, heads, lq, lk), float("nan"), dtype=torch.float16, device=device)
    r["o_cap16"] = K.attn_self(q, k, vt, out(), mode=K.FZ_ATTN_CAPTURE, p=p16, **kw)
    p8 = torch.full((clip + 1, heads, lq, lk), M.SENTINEL, dtype=torch.uint8, device=device)
    r["o_cap8"] = K.attn_self(q, k, vt, out(), mode=cap8, p=p8, **kw)
    r["p16"], r["p8"] = p16, p8
    deq = decode(p8)
    r["mask"] = M._split_mask(clip, lq, device)
    for tag, mask in (("all_stored", None), ("split", r["mask"])):
        kk = k if (mask is not None or lkf != lq) else None  # (without k the wrapper takes lkf = lq; with no mask the kernel never reads it)
        r["o_inj8_" + tag] = K.attn_self(q, kk, vt, out(), mode=inj8, p=p8, row_mask=mask, **kw)
        r["o_inj16_" + tag] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT, p=deq, row_mask=mask, **kw)
    return r


def check_map8(r):
    encode = MAP8_FORMATS[r["fmt"]][2]
    p16, p8 = r["p16"].cpu(), r["p8"].cpu()
    assert torch.isfinite(p16[1:].float()).all()
    want = encode(p16[1:])
    assert torch.equal(p8[1:], want), int((p8[1:] != want).sum())                      # the fp16 capture's map, rounded: bit for bit
    assert (p8[0] == M.SENTINEL).all(), "frame 0 of the map lies in front of p_frame_off: never written"
    assert torch.equal(r["o_cap8"].cpu(), r["o_cap16"].cpu()), "the launch's own output must not depend on the storage format"
    M.check_inject8_same_bits(r)                                                       # all-stored and split, bit for bit; the mask does split


def sharded_six_slots(device, *, batch=2, clip=6, lo=1, hi=4, heads=2, d=40, tokens=48, seed=0):
    """8: kernel_cases.case_sharded_pieces' attention part for six slots: the rank owning frames [lo, hi) launches on the extended frame axis
    [two left halo frames | own | two right halo frames | anchors 0 and clip - 1]; FLASH and CAPTURE bit-equal to the whole-clip launch.
    lo = 1: the left halo reaches in front of the clip (the owner's clamp to the clip's first frame)."""
    g = torch.Generator().manual_seed(seed)
    c, fl = heads * d, hi - lo
    idx = [-2, -1, "first", 1, 2, "last"]

    def own(t):
        return t.reshape(batch, clip, *t.shape[1:])[:, lo:hi].reshape(batch * fl, *t.shape[1:]).contiguous()

    def ext(t):
        t4 = t.reshape(batch, clip, *t.shape[1:])
        sel = [max(lo - 2, 0), max(lo - 1, 0)] + list(range(lo, hi)) + [min(hi, clip - 1), min(hi + 1, clip - 1)] + [0, clip - 1]
        return t4[:, sel].reshape(batch * len(sel), *t.shape[1:]).contiguous()

    qk = KC._mk((batch * clip, tokens, 2 * c), g, device, 1.5)
    q, k = qk[..., :c], qk[..., c:]
    v = KC._mk((batch * clip, tokens, c), g, device)
    vt = KC._vt(v, K.pad64(tokens))
    skw = dict(kv_slots_override=([0, 0, 1, 0, 0, 1], [-2, -1, fl + 4, 1, 2, fl + 5]), kv_clip_len=fl + 6, kv_frame_off=2)
    o_full = torch.empty(batch * clip, tokens, c, dtype=torch.float16, device=device)
    K.attn_self(q, k, vt, o_full, clip_len=clip, heads=heads, index_list=idx, mode=K.FZ_ATTN_FLASH)
    o_own = torch.full((batch * fl, tokens, c), float("nan"), dtype=torch.float16, device=device)
    K.attn_self(own(q), ext(k), ext(vt), o_own, clip_len=fl, heads=heads, index_list=idx, mode=K.FZ_ATTN_FLASH, **skw)
    assert torch.isfinite(o_full.float()).all() and torch.equal(o_own, own(o_full)), "extended K/V frame axis must address the same frames"
    p_full = torch.empty(batch * clip, heads, tokens, 6 * tokens, dtype=torch.float16, device=device)
    K.attn_self(q, k, vt, o_full, clip_len=clip, heads=heads, index_list=idx, mode=K.FZ_ATTN_CAPTURE, p=p_full)
    p_own = torch.full((batch * fl, heads, tokens, 6 * tokens), float("nan"), dtype=torch.float16, device=device)
    K.attn_self(own(q), ext(k), ext(vt), o_own, clip_len=fl, heads=heads, index_list=idx, mode=K.FZ_ATTN_CAPTURE, p=p_own, **skw)
    assert torch.equal(p_own, own(p_full)) and torch.equal(o_own, own(o_full))
    # and the slot layout is what the whole-clip launch stands for: fp32 torch on the concatenated frames
    p_ref, _ = KC.ref_self_attention(q.float().cpu(), k.float().cpu(), v.float().cpu(), heads, clip, idx)
    assert float((p_full.float().cpu() - p_ref).abs().max()) < 2e-3


def check_limits(device):
    """9: nine entries are refused by name, by kv_slots, by the launch wrapper and where the UNet is built."""
    import pytest
    for what in (lambda: K.kv_slots(L9, 12), lambda: PC.build_unet("tiny16", {"lora": 16, "SparseCausalAttention_index": L9}, "cpu")):
        with pytest.raises(ValueError) as e:
            what()
        msg = str(e.value)
        assert "FZ_MAX_KV_SLOTS" in msg and "8" in msg and repr(L9) in msg, msg
    q = torch.zeros(2, 64, 32, dtype=torch.float16, device=device)
    vt = torch.zeros(2, 32, 64, dtype=torch.float16, device=device)
    with pytest.raises(ValueError, match="FZ_MAX_KV_SLOTS"):
        K.attn_self(q, q, vt, torch.empty_like(q), clip_len=2, heads=2, index_list=L9)
    with pytest.raises(ValueError, match="FZ_MAX_KV_SLOTS"):
        K.attn_self(q, q, vt, torch.empty_like(q), clip_len=2, heads=2, index_list=[0], kv_slots_override=([0] * 9, [0] * 9), kv_clip_len=2)
    assert K.kv_slots(L8, 12) == ([1, 0, 0, 0, 0, 0, 0, 1], [0, -3, -2, -1, 1, 2, 3, 11])
    assert K.MAX_KV_SLOTS == 8


# ---------------------------------------------------------------------------------------------------------------
# pipeline level: tiny16, 6 frames
# ---------------------------------------------------------------------------------------------------------------
# The blend masks are built from `down_cross[2:4] + up_cross[:3]` (by list position), maps of one level only when the first UNet level lies above
# the 32^2-token capture limit (recompute_cases.EMU): the jobs whose inject launches run under a row mask use 40^2 latents, the smallest such
# latent; the jobs without blend words use the 16^2 latents of tests/test_dist_gpu.py::_job.
FRAMES = 6
BLEND_L = 40
# Threshold of the attention-blend mask.  On the emulator the fraction of ones falls from 0.88 at 0.3 over 0.51 / 0.52 (L5 / L8) at 0.55 to 0.24 at
# 0.8: 0.55 sits in the middle of the 20-80 % band (asserted on the emulator by tests/test_kv_slots_emu.py, on MI355X by the whole-job test)
BLEND_TH = 0.55
WHOLE_JOB = "kv_slots_tiny16_6f"
# Edit on identical maps against the oracle, max / latent scale.  pipeline_cases.EDIT_TOL_SAME_MAPS (1.5e-2) was measured on recordings of two
# to four frames; THIS job (6 frames, 40^2 latents, T = 4, the error grows over the steps of the self window) measures on MI355X, by list
# length: 2 entries ([-1, 'first']) 1.396 %, 3 entries 1.074 %, L5 1.325 %, L8 1.519 % -- no trend in the number of slots, and the two-entry list
# the old bound was made with already sits at 93 % of it (profiles/kv8_parity_numbers.txt).  Bound by the project's rule,
# 1.7 x the worst measured: the figure pipeline_cases.GEO_EDIT_TOL_SAME_MAPS gives the same harness.  The other constants hold as they stand.
KV_EDIT_TOL_SAME_MAPS = 2.6e-2


def model_config(index_list):
    return {"lora": 16, "SparseCausalAttention_index": list(index_list)}


def geo(index_list, L=BLEND_L, T=4):
    return dict(kind="tiny16", F=FRAMES, L=L, T=T, model_config=model_config(index_list))


def whole_job_case(index_list):
    """Inversion with capture + Replace edit with blend-masked self-attention: cross window [0, 2), self window [0, 2) of T = 4."""
    return dict(kind="tiny16", F=FRAMES, L=BLEND_L, T=4, model_config=model_config(index_list), prompt_case="teaser_posche", is_replace=True,
                cross_replace={"default_": 0.5}, self_replace=0.5, eq_params=None, blend_words=[["silver", "jeep"], ["Porsche", "car"]],
                blend_th=[BLEND_TH, BLEND_TH], blend_latents=False, regime="split")


SELF_LEVELS = [(20, 5), (10, 5), (5, 1)]  # (side, self-attention layers) of the levels of at most 32^2 tokens under 40^2 latents


@functools.lru_cache(maxsize=None)
def blend_mask_fractions(device, list_name, ths=(BLEND_TH,)):
    """The fraction of ones of the attention-blend masks of whole_job_case at each threshold of `ths`, without the edit: the masks are
    thresholded from the STORED cross maps of the source prompt, so the capture inversion of run_geometry_case (same seed, same draws) and the
    edit controller's blender (attention_util.make_controller's arguments) called as plan_controlled calls it -- once per self-attention layer
    of at most 32^2 tokens, at every step of the self window, on the store step that step reads -- give the edit's `mask_list`."""
    from helpers import ReplayTokenizer, load_json
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.prompt_attention.spatial_blend import SpatialBlender
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    G = whole_job_case(LISTS[list_name])
    T = G["T"]
    unet = PC.build_unet(G["kind"], G["model_config"], device)
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=ReplayTokenizer(), unet=unet, scheduler=DDIMScheduler())
    pipe.set_progress_bar_config(disable=True)
    pipe.scheduler.set_timesteps(T)
    z0, emb_src, _ = RC._inputs(G)  # seed 21: z0, then the source embedding -- the draws of run_geometry_case
    pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb_src.to(device),
                                       store_attention=True, LOW_RESOURCE=True, latents=z0.to(device))
    store = pipe.store_controller
    prompts = load_json("host_constants.json")[G["prompt_case"]]["prompts"]
    out = {}
    for th in ths:
        blender = SpatialBlender(prompts, G["blend_words"], start_blend=0.0, end_blend=2, tokenizer=ReplayTokenizer(), th=(th, th),
                                 NUM_DDIM_STEPS=T, prompt_choose="source")
        ones = total = 0.0
        for i in PC.controller_windows(T, G["cross_replace"], G["self_replace"], False)["self"]:
            sis = T - 1 - i  # use_inversion_attention: edit step i reads store step T - 1 - i
            for side, layers in SELF_LEVELS:
                m = blender(store.maps_of_step(sis), step_in_store=sis, target_h=side, target_w=side)
                ones, total = ones + layers * float(m.float().sum()), total + layers * m.numel()
        out[th] = ones / total
    pipe.release_attention_maps()
    return out


@functools.lru_cache(maxsize=None)
def whole_job(device, list_name, oracle_device=None):
    """pipeline_cases.run_geometry_case (native pipeline vs the fp32 oracle, run live; the leg on identical maps) on whole_job_case.  Returns
    (its result dict, the shapes of the self-attention maps the native store captured at step 0, keyed by store key)."""
    index_list = LISTS[list_name]
    PC.GEOMETRY_CASES[WHOLE_JOB] = whole_job_case(index_list)
    orig, made = PC.P2pDDIMSpatioTemporalPipeline, []

    def build(*a, **k):
        made.append(orig(*a, **k))
        return made[-1]
    PC.P2pDDIMSpatioTemporalPipeline = build
    try:
        res = PC.run_geometry_case(WHOLE_JOB, device, oracle_device=oracle_device, fp32_leg=False)
    finally:
        PC.P2pDDIMSpatioTemporalPipeline = orig
        del PC.GEOMETRY_CASES[WHOLE_JOB]
    assert len(made) == 1
    step0 = made[0].store_controller.attention_store_all_step[0]
    shapes = {k: [tuple(t.shape) for t in v] for k, v in step0.items() if k.endswith("self")}
    made[0].release_attention_maps()
    return res, shapes


def check_whole_job(res, shapes, index_list):
    """10 + 11, with the constants of pipeline_cases.py (and KV_EDIT_TOL_SAME_MAPS, above, for the edit)."""
    print("kv slots whole job", len(index_list), {k: res[k] for k in ("inv_err", "inv_scale", "self_map_err", "map_err", "edit_err_same_maps",
                                                                       "edit_scale", "attn_mask_flips_same_maps", "mask_ones_frac")})
    assert res["outputs_finite"], res
    assert res["inv_err"] <= PC.LATENT_TOL * res["inv_scale"], res
    # 11: run_geometry_case compared every stored map of steps 0 and T - 1, all len(L) slot blocks of every frame, with the oracle's map of the
    # same shape -- the oracle concatenates the frames its sparse_causal_frame_indices names
    assert res["self_map_err"] <= PC.SELF_MAP_TOL, res
    assert res["attn_mask_flips_same_maps"] == 0, res
    assert res["edit_err_same_maps"] <= KV_EDIT_TOL_SAME_MAPS * res["edit_scale"], res
    lo, hi = PC.FULL_MASK_BAND
    assert lo <= res["mask_ones_frac"] <= hi, res["mask_ones_frac"]  # the inject launches ran under a row mask that splits the rows
    n_maps = 0
    for key, lst in shapes.items():
        for f, heads, lq, lk in lst:
            assert f == FRAMES and lk == len(index_list) * lq, (key, (f, heads, lq, lk))
            n_maps += 1
    assert n_maps >= 6, shapes  # the 20^2, 10^2 and 5^2 levels, down and up (and mid) -- every level that stores a self map


@functools.lru_cache(maxsize=None)
def job(device, list_name, L=16, **kw):
    """recompute_cases.run_job on the 6-frame job of `list_name`; L = 16: without blend words (the launches get no row mask)."""
    kw.setdefault("recompute", False)
    if L == 16:
        kw.update(blend=False, blend_latents=False)
    else:
        kw.setdefault("blend_th", BLEND_TH)
        kw.setdefault("blend_latents", False)
    return RC.run_job(device, geo(LISTS[list_name], L=L), **kw)
