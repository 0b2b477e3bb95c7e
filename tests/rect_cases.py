"""Rectangular (widescreen / portrait) clips: cases shared by the CPU-emulation suite (tests/test_rect_emu.py) and the MI355X suite
(tests/test_rect_gpu.py).

Conventions under test: order is (height, width); token index y * w + x; an attention level of `lq` tokens under an extent (H, W) of the same
aspect ratio is h = round(sqrt(lq * H / W)), w = lq // h with h * w == lq and h * W == w * H (`level_hw` below restates the rule, so the
tests do not lean on the code they check)."""
import math

import torch
import torch.nn.functional as F

from helpers import ReplayTokenizer, load_json
from oracle import fatezero_oracle as O
from oracle.weights import procedural_state_dict

import pipeline_cases as PC
from pipeline_cases import GEO_EDIT_TOL_SAME_MAPS, GEO_LATENT_TOL, GEO_MAP_TOL, GEO_SELF_MAP_TOL  # imported, not copied

from fatezero_amd import kernels as K
from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
from fatezero_amd.video_diffusion.prompt_attention import attention_util
from fatezero_amd.video_diffusion.schedulers import DDIMScheduler


def level_hw(lq, extent):
    H, W = extent
    h = int(round(math.sqrt(lq * H / W)))
    w = lq // h
    assert h * w == lq and h * W == w * H, (lq, extent)
    return h, w


# ------------------------------------------------------------------------------------------------------------
# A. blend mask, bit-exact
# ------------------------------------------------------------------------------------------------------------
BLEND_TH = 0.6
# (map (rh, rw), output (out_h, out_w), prompts, or_with_first)
BLEND_CASES = [
    ((10, 16), (20, 32), 1, False),
    ((16, 10), (64, 40), 1, False),   # portrait
    ((5, 8), (40, 64), 1, False),
    ((10, 16), (10, 16), 1, False),   # no resize
    ((9, 16), (18, 32), 1, False),    # odd side
    ((10, 16), (40, 64), 2, True),    # two prompts, or_with_first
    ((20, 36), (40, 72), 1, False),
]
BLEND_IDS = ["%dx%d-%dx%d-p%d" % (m + o + (p,)) for m, o, p, _ in BLEND_CASES]


def blob_maps_hw(P_, F_, heads, rh, rw, g, lk=77, n_maps=5):
    """kernel_cases.blob_maps on an rh x rw grid: per map, cx, cy, then the logits, all from the one generator."""
    out = []
    yy, xx = torch.meshgrid(torch.arange(rh), torch.arange(rw), indexing="ij")
    sigma = math.sqrt(rh * rw) / 4
    for _ in range(n_maps):
        cx = torch.rand(P_, F_, 1, 1, lk, generator=g) * rw
        cy = torch.rand(P_, F_, 1, 1, lk, generator=g) * rh
        d2 = (xx.reshape(1, 1, 1, rh * rw, 1) - cx) ** 2 + (yy.reshape(1, 1, 1, rh * rw, 1) - cy) ** 2
        logits = torch.randn(P_, F_, heads, rh * rw, lk, generator=g) * 0.5 - d2 / (2 * sigma ** 2)
        out.append(logits.softmax(-1))
    return out


def ref_blend_scores(maps, alpha, rh, rw, h, w):
    """kernel_cases.ref_blend_mask up to the threshold, with (rh, rw) in the reshape: the normalised score [P, F, h, w]."""
    rr = []
    for item in maps:
        p, c, heads, npix, wd = item.shape
        assert npix == rh * rw
        rr.append(item.reshape(p, c, heads, rh, rw, wd).permute(0, 2, 1, 3, 4, 5))
    m = torch.cat(rr, dim=1)
    m = (m * alpha[:, None, None, None, None, :]).sum(-1).mean(1)
    m = F.max_pool2d(m, (3, 3), (1, 1), padding=(1, 1))
    score = F.interpolate(m, size=(h, w))
    return score / score.max(-2, keepdim=True)[0].max(-1, keepdim=True)[0]


def ref_blend_mask_hw(maps, alpha, th, rh, rw, h, w, or_first):
    mask = ref_blend_scores(maps, alpha, rh, rw, h, w).gt(th)
    if or_first:
        mask = mask[:1] + mask
    return mask


def blend_inputs(device, prompts, frames, heads, rh, rw, seed):
    g = torch.Generator().manual_seed(seed)
    dev_maps = []
    for m in blob_maps_hw(prompts, frames, heads, rh, rw, g):
        buf = torch.zeros(prompts, frames, heads, rh * rw, K.CROSS_P_STRIDE, dtype=torch.float16)
        buf[..., :77] = m.half()
        dev_maps.append(buf.to(device))
    alpha = torch.zeros(prompts, 80)
    alpha[:, [2, 3]] = 1.0
    return dev_maps, alpha


def case_blend_mask_hw(device, *, map_hw, out_hw, prompts, or_first, frames, heads, seed=0, th=BLEND_TH, against_oracle=False):
    (rh, rw), (oh, ow) = map_hw, out_hw
    dev_maps, alpha = blend_inputs(device, prompts, frames, heads, rh, rw, seed)
    out = K.blend_mask(dev_maps, alpha.to(device), th, out_hw, or_with_first=or_first, map_hw=(rh, rw))
    maps32 = [b.float().cpu()[..., :77] for b in dev_maps]
    score = ref_blend_scores(maps32, alpha[:, :77], rh, rw, oh, ow)
    ref = ref_blend_mask_hw(maps32, alpha[:, :77], th, rh, rw, oh, ow, or_first)
    res = {"ones": float(ref.float().mean()), "margin": float((score - th).abs().min()),
           "diff": int((out.cpu().bool() != ref).sum())}
    print("blend_mask_hw", map_hw, out_hw, "P", prompts, "seed", seed, res)
    if against_oracle:  # the restated reference is the oracle's arithmetic: the same masks, element for element
        m6 = torch.cat([m.reshape(prompts, frames, heads, rh, rw, 77).permute(0, 2, 1, 3, 4, 5) for m in maps32], dim=1)
        want = O.blend_get_mask(m6, alpha[:, :77].reshape(prompts, 1, 1, 1, 1, 77), (th, th), True, oh, ow,
                                "both" if or_first else "source")
        assert torch.equal(want.bool(), ref.bool())
    assert 0.02 < res["ones"] < 0.98, f"degenerate mask ({res['ones']})"
    assert res["margin"] >= 1e-5, f"a normalised score sits {res['margin']} from the threshold: take another seed"
    assert res["diff"] == 0, f"{res['diff']} differing mask elements"
    return res


def case_square_entry_equals_hw_entry(device, frames=2, heads=2, seed=0):
    """fz_blend_mask_hw(16, 16) is fz_blend_mask(16), bit for bit."""
    dev_maps, alpha = blend_inputs(device, 2, frames, heads, 16, 16, seed)
    a = K.blend_mask(dev_maps, alpha.to(device), BLEND_TH, (64, 64), or_with_first=True)
    b = K.blend_mask(dev_maps, alpha.to(device), BLEND_TH, (64, 64), or_with_first=True, map_hw=(16, 16))
    assert 0.02 < float(a.mean()) < 0.98
    assert torch.equal(a, b)


FZ_ERR_BAD_ARG = -1  # csrc/fz_rt.h


def case_oversized_map_is_refused(device):
    """41 x 40 = 1640 pixels > BM_MAX_PIX: FZ_ERR_BAD_ARG, nothing launched."""
    import pytest
    dev_maps = [torch.zeros(1, 1, 1, 41 * 40, K.CROSS_P_STRIDE, dtype=torch.float16, device=device)]
    alpha = torch.zeros(1, 80, device=device)
    with pytest.raises(RuntimeError, match=r"fz_blend_mask_hw failed with code %d$" % FZ_ERR_BAD_ARG):
        K.blend_mask(dev_maps, alpha, BLEND_TH, (82, 80), or_with_first=False, map_hw=(41, 40))


# ------------------------------------------------------------------------------------------------------------
# C. the controller on a rectangular job
# ------------------------------------------------------------------------------------------------------------
class RectBlender(O.Blender):
    """The oracle's Blender with (h, w) maps: its __call__ restated with the one reshape changed; the mask arithmetic is the oracle's
    blend_get_mask."""

    def __call__(self, attention_store, target_h=None, target_w=None, x_t=None):
        if target_h is None and x_t is not None:
            target_h, target_w = x_t.shape[-2:]
        self.counter += 1
        maps = attention_store["down_cross"][2:4] + attention_store["up_cross"][:3]
        rearranged = []
        for item in maps:
            if item.dim() == 4:
                item = item[None]
            p, c, heads, r, w = item.shape
            rh, rw = level_hw(r, (target_h, target_w))
            rearranged.append(item.reshape(p, c, heads, rh, rw, w).permute(0, 2, 1, 3, 4, 5).float())
        maps = torch.cat(rearranged, dim=1)
        alpha = self.alpha_layers[0:1] if self.prompt_choose == "source" else self.alpha_layers
        mask = O.blend_get_mask(maps, alpha, self.th, True, target_h, target_w, self.prompt_choose).float()
        self.mask_list.append(mask[0][:, None, :, :].clone())
        if x_t is not None:
            if x_t.dim() == 5:
                mask = mask[:, None]
            if self.start_blend < self.counter < self.end_blend:
                self.applied_mask_list.append(mask[1:, 0] if mask.dim() == 5 else mask[1:])
                x_t = x_t[:1] + mask * (x_t - x_t[:1])
            return x_t
        return mask


class RectEditController(O.EditController):
    """The oracle's EditController; only the blend-masked self-attention branch (the one with the square reshape) is restated with (h, w)."""
    latent_hw = None

    def forward(self, attn, is_cross, place):
        masked = (not is_cross and attn.shape[-2] <= 32 ** 2 and self.attention_blend is not None
                  and self.num_self_replace[0] <= self.cur_step < self.num_self_replace[1])
        if not masked:
            return super().forward(attn, is_cross, place)
        O.StoreController.forward(self, attn, is_cross, place)
        self._consts_to(attn.device)
        key = f"{place}_self"
        pos = self.pos[key]
        all_step = self.store.attention_store_all_step
        sis = len(all_step) - self.cur_step - 1 if self.use_inversion_attention else self.cur_step
        step_dict = all_step[sis]
        base = step_dict[key][pos].to(attn.device)
        self.pos[key] += 1
        f = attn.shape[0]
        attn5 = attn.reshape(1, f, *attn.shape[1:]).clone()
        h, w = level_hw(attn5.shape[-2], self.latent_hw)
        mask = self.attention_blend(step_dict, target_h=h, target_w=w)  # [1,F,h,w]
        m = mask.permute(1, 0, 2, 3).reshape(mask.shape[1], mask.shape[0], h * w)[..., None]
        attn5 = m * attn5 + (1 - m) * base[None]
        return attn5.reshape(f, *attn5.shape[2:])


def make_rect_oracle_controller(latent_hw, *args, **kwargs):
    c = O.make_edit_controller(*args, **kwargs)
    c.__class__ = RectEditController
    c.latent_hw = tuple(latent_hw)
    for b in (c.attention_blend, c.latent_blend):
        if b is not None:
            b.__class__ = RectBlender
    return c


class ForeignStyle:
    """A controller with only the reference's tensor protocol (protocol_cases._Recorder), wrapped around a native edit controller: the
    pipeline cannot plan with it, so every controlled layer goes through `AttentionControlEdit.forward`."""

    def __init__(self, inner):
        self.inner = inner
        self.calls = []
        self.num_att_layers = -1

    def __call__(self, attn, is_cross, place):
        self.calls.append((tuple(attn.shape), bool(is_cross), place))
        return self.inner(attn, is_cross, place)

    def step_callback(self, x_t):
        return self.inner.step_callback(x_t)

    def between_steps(self):
        return self.inner.between_steps()


def run_rect_job(device, *, kind, F_, T, hw, oracle_device=None, seed=21, save_path=None, protocol_leg=True):
    """pipeline_cases.run_geometry_case's first leg (native job vs the fp32 oracle; the oracle's edit on the natively captured maps) for the
    `mini_emu` controller setting on (H, W) latents, plus the tensor-protocol leg and the mask dumps."""
    G = PC.GEOMETRY_CASES["mini_emu"]
    H, W = hw
    odev = torch.device(device if oracle_device is None else oracle_device)
    arch, mc = PC.TINY[kind], dict(G["model_config"])
    consts = load_json("host_constants.json")[G["prompt_case"]]
    src, tgt = consts["prompts"]
    th = list(G["blend_th"])
    unet = UNetPseudo3DConditionModel(sample_size=64, **arch, **mc)
    sd = procedural_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()])
    unet.load_state_dict(sd)
    unet = unet.half().to(device).eval()
    fast_before = O.FAST_LARGE_ATTENTION
    O.FAST_LARGE_ATTENTION = True
    try:
        ounet = O.OracleUNet(sd, O.UNetConfig(**arch, model_config=mc), device=odev)
        tok = ReplayTokenizer()
        pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=tok, unet=unet, scheduler=DDIMScheduler())
        pipe.set_progress_bar_config(disable=True)
        pipe.scheduler.set_timesteps(T)
        g = torch.Generator().manual_seed(seed)
        cdim = arch["cross_attention_dim"]
        z0 = torch.randn(1, 4, F_, H, W, generator=g)
        emb_src = torch.randn(2, 77, cdim, generator=g) * 0.5
        emb_tgt = emb_src + 0.25 * torch.randn(2, 77, cdim, generator=g)
        res = {"hw": (H, W), "frames": F_, "T": T, "kind": kind}
        import time
        clock, t0 = {}, time.time()

        def lap(name):
            nonlocal t0
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            clock[name], t0 = round(time.time() - t0, 2), time.time()
        # ---- inversion with capture
        lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb_src.to(device),
                                                 store_attention=True, LOW_RESOURCE=True, latents=z0.to(device))
        lap("native_inversion")
        ostore = O.StoreController()
        olat = O.ddim_inversion(ounet, O.DDIMSchedule(T), z0, emb_src[1:], ostore)
        lap("oracle_inversion")
        res["inv_scale"] = float(olat[-1].abs().max())
        res["inv_err"] = max(float((lat[i].float().cpu() - olat[i].cpu()).abs().max()) for i in range(1, T + 1))
        store = pipe.store_controller
        assert len(store.attention_store_all_step) == len(ostore.attention_store_all_step) == T
        worst_cross = worst_self = 0.0
        for step in (0, T - 1):
            for k, lst in ostore.attention_store_all_step[step].items():
                got = store.attention_store_all_step[step][k]
                assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in lst], (k, step)
                for a, b in zip(got, lst):
                    e = float((a.float().cpu() - b.cpu()).abs().max())
                    if k.endswith("cross"):
                        worst_cross = max(worst_cross, e)
                    else:
                        worst_self = max(worst_self, e)
        res["map_err"], res["self_map_err"] = worst_cross, worst_self
        # ---- edit
        kw = dict(prompt=tgt, source_prompt=src, num_inference_steps=T, cross_replace_steps=dict(G["cross_replace"]),
                  self_replace_steps=G["self_replace"], use_inversion_attention=True, is_replace_controller=True,
                  blend_th=list(th), save_self_attention=False, guidance_scale=7.5, blend_words=G["blend_words"], blend_self_attention=True,
                  blend_latents=True)
        if save_path is not None:
            kw["save_path"] = save_path
        pipe._encode_prompt = lambda *a, **k: emb_tgt.to(device)
        zT = lat[-1].float().cpu()
        out = pipe(latents=zT.to(device), edit_type="swap", output_type="latent", **kw)
        edited = out["sdimage_output"].images.float().cpu()
        nctrl = pipe.last_edit_controller
        lap("native_edit")
        assert tuple(nctrl.latent_hw) == (H, W) and tuple(store.latent_hw) == (H, W)
        if save_path is not None:
            res["mask_pngs_checked"] = PC.check_mask_dumps(save_path, nctrl)
        ost = O.StoreController()
        ost.attention_store_all_step = [{k: [t.float().to(odev) for t in v] for k, v in d.items()} for d in store.attention_store_all_step]
        ost.latents_store = [t.float().to(odev) for t in store.latents_store]
        octrl = make_rect_oracle_controller((H, W), tok, [src, tgt], ost, T, True, dict(G["cross_replace"]), G["self_replace"],
                                            blend_words=G["blend_words"], eq_params=None, blend_th=tuple(th), blend_self_attention=True,
                                            blend_latents=True, save_self_attention=False)
        # teacher forcing of the applied latent masks, as run_geometry_case does: the oracle computes and records its own masks but blends
        # with what the native run applied (the target half of an applied mask is thresholded from LIVE maps, fp16 here and fp32 there)
        lb, queue = octrl.latent_blend, list(nctrl.latent_blend.applied_mask_list)

        def forced_call(attention_store, target_h=None, target_w=None, x_t=None, _orig=lb.__call__):
            n_before = len(lb.applied_mask_list)
            x_own = _orig(attention_store, target_h, target_w, x_t=x_t)
            if len(lb.applied_mask_list) == n_before:
                return x_own
            m = queue.pop(0).to(x_t).reshape(1, 1, *x_t.shape[2:])
            return torch.cat([x_t[:1], x_t[:1] + m * (x_t[1:] - x_t[:1])], dim=0)
        octrl.latent_blend = type("ForcedBlender", (), {"__call__": staticmethod(forced_call), "mask_list": lb.mask_list,
                                                        "applied_mask_list": lb.applied_mask_list})()
        o_edit = O.ddim_edit(ounet, O.DDIMSchedule(T), zT, emb_tgt, octrl, guidance_scale=7.5).cpu()
        lap("oracle_edit")
        res["edit_scale"] = float(o_edit.abs().max())
        res["edit_err_same_maps"] = float((edited - o_edit).abs().max())
        ml = nctrl.attention_blend.mask_list
        res["attn_mask_shapes"] = sorted({tuple(m.shape[-2:]) for m in ml})
        res["attn_mask_flips_same_maps"], res["attn_mask_total"] = PC._mask_flips(ml, octrl.attention_blend.mask_list)
        res["latent_mask_flips_same_maps"], res["latent_mask_total"] = PC._mask_flips(nctrl.latent_blend.mask_list, lb.mask_list)
        res["latent_mask_shapes"] = sorted({tuple(m.shape[-2:]) for m in nctrl.latent_blend.mask_list})
        res["mask_ones_frac"] = float(sum(float(m.float().sum()) for m in ml) / max(1, sum(m.numel() for m in ml)))
        res["applied_masks"] = len(nctrl.latent_blend.applied_mask_list)
        res["outputs_finite"] = bool(torch.isfinite(edited).all())
        strips = out["attention_output"]
        res["strip_shape"] = None if strips is None or len(strips) == 0 else tuple(strips[0].shape)
        # ---- the tensor protocol: the same controller class behind a foreign-style wrapper, every layer through forward()
        if protocol_leg:
            inner = attention_util.make_controller(
                tok, [src, tgt], NUM_DDIM_STEPS=T, is_replace_controller=True, cross_replace_steps=dict(G["cross_replace"]),
                self_replace_steps=G["self_replace"], blend_words=G["blend_words"], additional_attention_store=store,
                use_inversion_attention=True, blend_th=list(th), blend_self_attention=True, blend_latents=False, save_self_attention=False)
            inner.latent_hw = (H, W)  # (a wrapped controller is foreign to the pipeline: nobody else tells it)
            rec = ForeignStyle(inner)
            attention_util.register_attention_control(pipe, rec)
            last_masked = inner.num_self_replace[1] - 1   # row masks exist inside the self-replace window only: the run ends where it closes

            class WindowClosed(Exception):
                pass

            def stop_behind_the_window(i, t, x):
                if i >= last_masked:
                    raise WindowClosed
            try:
                pipe.sd_ddim_pipeline(prompt=tgt, latents=zT.to(device), num_inference_steps=T, guidance_scale=7.5, controller=rec,
                                      output_type="latent", callback=stop_behind_the_window, callback_steps=1)
            except WindowClosed:
                pass
            attention_util.register_attention_control(pipe, pipe.empty_controller)
            assert 0 <= last_masked < T - 1 and inner.cur_step == last_masked + 1, (last_masked, inner.cur_step)
            pl = inner.attention_blend.mask_list
            res["protocol_calls"] = len(rec.calls)
            res["protocol_masks"] = len(pl)
            res["protocol_masks_equal"] = len(pl) == len(ml) and all(torch.equal(a, b) for a, b in zip(pl, ml))
            lap("protocol_edit")
        res["seconds"] = clock
        return res
    finally:
        O.FAST_LARGE_ATTENTION = fast_before


def check_rect_job(res):
    print("rect job", res)
    H, W = res["hw"]
    assert res["outputs_finite"], res
    assert res["inv_err"] <= GEO_LATENT_TOL * res["inv_scale"], res
    assert res["map_err"] <= GEO_MAP_TOL and res["self_map_err"] <= GEO_SELF_MAP_TOL, res
    assert res["attn_mask_flips_same_maps"] == 0 and res["attn_mask_total"] > 0, res
    assert res["latent_mask_flips_same_maps"] == 0 and res["latent_mask_total"] > 0, res
    assert res["edit_err_same_maps"] <= GEO_EDIT_TOL_SAME_MAPS * res["edit_scale"], res
    # the masks are (h, w) maps of the clip's aspect ratio at every blended level, and the latent masks have the latent size
    assert res["attn_mask_shapes"] == sorted({(H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8)}), res
    assert res["latent_mask_shapes"] == [(H, W)] and res["applied_masks"] > 0, res
    assert 0.0 < res["mask_ones_frac"] < 1.0, res
    # the cross-attention strips: one heat map per token with the clip's aspect ratio (longer side 256 pixels) and the text band under it
    th_, tw_ = (round(256 * H / W), 256) if W >= H else (256, round(256 * W / H))
    assert res["strip_shape"] is not None and res["strip_shape"][0] == th_ + int(th_ * 0.2) and res["strip_shape"][1] % tw_ == 0, res
    assert res["strip_shape"][1] // tw_ > 1 and res["strip_shape"][2] == 3, res
    if "protocol_masks_equal" in res:
        assert res["protocol_masks"] > 0 and res["protocol_masks_equal"], res
    if "mask_pngs_checked" in res:
        assert res["mask_pngs_checked"] > 0, res


# ------------------------------------------------------------------------------------------------------------
# D. rectangular launches through the library's own dispatch
# ------------------------------------------------------------------------------------------------------------
def run_unet_forward_hw(device, hw, kind="tiny40", F_=4, seed=13, t=481, oracle_device=None):
    """pipeline_cases.run_fullwidth_forward at tiny width on (H, W) latents."""
    arch, mc = PC.TINY[kind], {"lora": 16}
    unet = UNetPseudo3DConditionModel(sample_size=64, **arch, **mc)
    sd = procedural_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()])
    unet.load_state_dict(sd)
    unet = unet.half().to(device).eval()
    ounet = O.OracleUNet(sd, O.UNetConfig(**arch, model_config=mc), device=oracle_device)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, 4, F_, hw[0], hw[1], generator=g)
    ctx = torch.randn(1, 77, arch["cross_attention_dim"], generator=g) * 0.5
    y = unet(z.to(device).half(), t, ctx.to(device).half()).sample.float().cpu()
    fast_before = O.FAST_LARGE_ATTENTION
    O.FAST_LARGE_ATTENTION = oracle_device is not None
    try:
        ref = ounet(z, t, ctx).cpu()
    finally:
        O.FAST_LARGE_ATTENTION = fast_before
    assert y.shape == ref.shape == (1, 4, F_, hw[0], hw[1])
    return {"hw": tuple(hw), "err": float((y - ref).abs().max()), "scale": float(ref.abs().max())}


def case_vae_roundtrip_hw(device, hw, n=2, seed=0, tol_enc=2e-2, tol_dec=3e-2):
    """vae_cases.case_vae_roundtrip (its TINY architecture, its default tolerances) on frames of hw = (height, width) pixels."""
    import vae_cases as VC
    from oracle import vae_oracle
    cfg = VC.TINY
    vae, sd = VC.seeded_vae(cfg, seed)
    vae = vae.to(device).half()
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand(n, 3, hw[0], hw[1], generator=g) * 2 - 1).half().float()
    mom_ref = vae_oracle.encode_moments(sd, cfg, x)
    post = vae.encode(x.to(device).half()).latent_dist
    mom = post.parameters.float().cpu()
    assert mom.shape == mom_ref.shape == (n, 8, hw[0] // 2, hw[1] // 2), (mom.shape, mom_ref.shape)
    e_enc = float((mom - mom_ref).abs().max() / mom_ref.abs().max())
    mean_ref, _ = vae_oracle.posterior(mom_ref)
    zin = (mean_ref * 0.5).half().float()
    img_ref = vae_oracle.decode(sd, cfg, zin)
    img = vae.decode(zin.to(device).half()).sample.float().cpu()
    assert img.shape == img_ref.shape == (n, 3, hw[0], hw[1]), (img.shape, img_ref.shape)
    e_dec = float((img - img_ref).abs().max() / img_ref.abs().max())
    print("vae", hw, e_enc, e_dec)
    assert e_enc < tol_enc and e_dec < tol_dec, (e_enc, e_dec)
    return {"enc_rel_err": e_enc, "dec_rel_err": e_dec}
