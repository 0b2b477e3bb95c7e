"""FateZero editing pipeline (reference: video_diffusion/pipelines/p2p_ddim_spatial_temporal.py).

`P2pDDIMSpatioTemporalPipeline` keeps the reference's constructor, attributes (`store_controller`,
`empty_controller`, ...), methods and keyword arguments.  The two hot loops are re-built around the native engine:

  * latents live in one fp32 buffer [4, F, h*w] plus an fp16 token-major copy [F(or 2F), h*w, 4] that is the UNet
    input; one fused kernel per step does classifier-free guidance + the DDIM (or inverse DDIM) update + the
    next UNet input (`fz_latent_update`), so no torch elementwise chain, no `torch.cat([latents] * 2)`, no
    `torch.cuda.empty_cache()` (p2p_ddim_spatial_temporal.py:391-421) survives;
  * the UNet is called through `forward_tokens` (no layout conversions inside the loop);
  * capture / injection of attention maps happens inside the attention kernels according to the registered
    controller's plan; maps never leave HBM.
"""
import os
from typing import Callable, List, Optional, Union

import numpy as np
import torch

from ... import dist as fz_dist
from ... import kernels as K
from ..models.resnet import Tokens
from ..models.unet_3d_condition import cfg_shared_head_active
from ..prompt_attention import attention_util, spatial_blend
from .stable_diffusion import SpatioTemporalStableDiffusionPipeline, StableDiffusionPipelineOutput


class _LatentState:
    """fp32 master latents [4, F, hw] + the fp16 token-major UNet input.  The `reps` halves of the CFG batch are the SAME latents: with the
    UNet's CFG-shared head (unet_3d_condition.py: CFG_SHARED_HEAD; never under a frame shard) the input is ONE copy [F, hw, 4] handed out as
    `Tokens(..., b=reps, rep=reps)`; otherwise [reps*F, hw, 4] with the copies written out."""

    def __init__(self, latents: torch.Tensor, reps: int, share: bool = True):
        b, c, f, h, w = latents.shape
        if b != 1:
            raise ValueError("Only support single video editing")  # attention_util.py:192 of the reference
        self.f, self.h, self.w, self.reps = f, h, w, reps
        self.copies = 1 if (reps > 1 and share and cfg_shared_head_active()) else reps  # copies of the latents the token buffer holds
        # always a private copy: the master buffer is updated in place every step and must never alias the caller's latents
        self.z = latents[0].to(torch.float32, copy=True).reshape(c, f, h * w).contiguous()
        self.tok = torch.empty(self.copies * f, h * w, c, dtype=torch.float16, device=latents.device)
        self.sync_tokens()

    def sync_tokens(self):
        t = self.z.permute(1, 2, 0).to(torch.float16)
        for r in range(self.copies):
            self.tok[r * self.f:(r + 1) * self.f].copy_(t)

    def tokens(self) -> Tokens:
        return Tokens(self.tok, self.reps, self.f, self.h, self.w, rep=self.reps // self.copies)

    def as_latents(self, dtype) -> torch.Tensor:
        return self.z.view(1, self.z.shape[0], self.f, self.h, self.w).to(dtype)

    def assign(self, latents: torch.Tensor):
        self.z.copy_(latents[0].float().reshape(self.z.shape))
        self.sync_tokens()

    def update(self, eps_u, eps_c, guidance, cz, ce):
        K.latent_update(self.z, eps_u, eps_c, guidance, cz, ce, next_in=self.tok[: self.f])
        for r in range(1, self.copies):
            self.tok[r * self.f:(r + 1) * self.f].copy_(self.tok[: self.f])


class P2pDDIMSpatioTemporalPipeline(SpatioTemporalStableDiffusionPipeline):
    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, disk_store: bool = False, map_dtype: str = "fp16",
                 recompute_maps: bool = False):
        """`map_dtype` (extension): "fp16" (default), "e5m2" or "ue4m4" -- the captured SELF-attention maps at one byte per probability, which
        halves the map arena (attention_store.py; "ue4m4" keeps 4 mantissa bits where "e5m2" keeps 2); cross maps, the inversion trajectory and every other tensor are unaffected.
        `recompute_maps` (extension, opt-in): the inversion stores no attention maps, only the latent every iteration was fed; each edit step
        first re-runs the one inversion forward whose maps it reads (same kernels, same bytes: the edit is bit-identical to the resident
        one) into a one-step slab, so the map arena is one step instead of one per DDIM step, at the price of an F-frame forward per edit
        step.  Composes with every `map_dtype`; needs `use_inversion_attention=True`; with it `disk_store=True` has nothing to spill."""
        super().__init__(vae, text_encoder, tokenizer, unet, scheduler)
        self.map_dtype = self.default_map_dtype = map_dtype  # (default_map_dtype: what a YAML config without the key falls back to)
        self.recompute_maps = self.default_recompute_maps = bool(recompute_maps)
        self._source_tokens = None  # recompute_maps: the token-major input of the per-step source forward (one buffer, refilled every step)
        self.store_controller = attention_util.AttentionStore(disk_store=disk_store, map_dtype=map_dtype, recompute=self.recompute_maps)
        self.empty_controller = attention_util.EmptyControl()
        # extension: a fatezero_amd.dist.FrameShard splits the clip's frames over the ranks of a process group; every rank
        # is handed (and returns) the full latents, keeps only its own frames' maps / masks in between
        self.frame_shard = None

    def _gather_frames(self, latents_local: List[torch.Tensor]) -> List[torch.Tensor]:
        """[.., 4, F_local, h, w] latents of this rank -> the same list with all F frames (one all-gather)."""
        shard = self.frame_shard
        x = torch.stack(latents_local)                        # [S, B, C, Fl, h, w]
        s_, b_, c_, fl, h_, w_ = x.shape
        full = shard.all_gather_frames(x.permute(0, 1, 3, 2, 4, 5).reshape(s_ * b_, fl, c_, h_, w_))
        full = full.reshape(s_, b_, shard.clip_len, c_, h_, w_).permute(0, 1, 3, 2, 4, 5)
        return [full[i].contiguous() for i in range(s_)]

    def set_map_dtype(self, map_dtype: str):
        """Switch the storage of the captured self-attention maps ("fp16" | "e5m2" | "ue4m4") for the jobs that follow: the maps of the last
        inversion are dropped and a store of the new format takes the old one's place."""
        if map_dtype != self.map_dtype:
            store = self.store_controller.with_map_dtype(map_dtype)  # (raises on an unknown name)
            self.release_attention_maps()
            self.store_controller, self.map_dtype = store, map_dtype

    def set_recompute_maps(self, recompute_maps: bool):
        """Switch the recompute mode (class docstring) for the jobs that follow: what the last inversion kept is dropped and a store of the
        other mode takes the old one's place."""
        if bool(recompute_maps) != self.recompute_maps:
            store = self.store_controller.with_recompute(bool(recompute_maps))
            self.release_attention_maps()
            self.store_controller, self.recompute_maps = store, bool(recompute_maps)

    def _refuse_issue_plans(self):
        """recompute_maps and the native issue plans (fatezero_amd/issue.py) do not run together: on the MI355X a second editing prompt
        replayed from plans beside the recomputed source forwards came out different from the walked job (the first one was bit-identical;
        the cause is not found), so the combination is refused by name instead of being trusted."""
        if getattr(self.unet, "_issuer", None) is not None or os.environ.get("FZ_ISSUE_PLANS") == "1":
            raise RuntimeError("recompute_maps=True does not run under native issue plans (FZ_ISSUE_PLANS=1 / unet.enable_issue_plans()): "
                               "switch one of the two off")

    def _recompute_source_maps(self, controller, frames, h, w):
        """recompute_maps, in front of an edit step: the inversion forward of the store step this edit step reads (attention and latent blend ask
        for the same one: n - 1 - i), from that iteration's stored input latent, at its timestep, under the source context, one copy, with the
        store controller registered as the inversion registers it -- into the store's step slab.  Ends behind the last captured map."""
        store = controller.additional_attention_store
        sis = controller._step_in_store()
        if store.slab_step == sis:  # (the first edit after the inversion: its last iteration's maps are still in the slab)
            return
        latent, t, ctx = store.source_input(sis)
        if tuple(latent.shape[-3:]) != (frames, h, w):
            raise ValueError(f"recompute_maps: the inversion kept latents of {tuple(latent.shape[-3:])} (frames, h, w), the edit runs on "
                             f"{(frames, h, w)}")
        tok = self._source_tokens
        if tok is None or tuple(tok.shape) != (frames, h * w, 4) or tok.device != latent.device:
            tok = self._source_tokens = torch.empty(frames, h * w, 4, dtype=torch.float16, device=latent.device)
        K.latent_tokens(latent[0].reshape(4, frames, h * w), out=tok)
        low = store.LOW_RESOURCE
        store.LOW_RESOURCE = True
        attention_util.register_attention_control(self, store)
        try:
            store.begin_recompute(sis)
            self.unet.forward_tokens(Tokens(tok, 1, frames, h, w), t, ctx, maps_up_to=attention_util.MAX_CONTROLLED_TOKENS)
            store.end_recompute(sis)
        finally:
            store.LOW_RESOURCE = low
            attention_util.register_attention_control(self, controller)

    def release_attention_maps(self):
        """Free the HBM map arena of the last inversion (and the edit controller that references it) so that the next
        job recycles the block instead of allocating a second one."""
        self.last_edit_controller = None
        if self.store_controller is not None:
            self.store_controller.release_arena()

    def check_inputs(self, prompt, height, width, callback_steps, strength=None):
        if not isinstance(prompt, str) and not isinstance(prompt, list):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if strength is not None and (strength <= 0 or strength > 1):
            raise ValueError(f"The value of strength should in (0.0, 1.0] but is {strength}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if (callback_steps is None) or (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type"
                             f" {type(callback_steps)}.")

    # ------------------------------------------------------------------------------------------------------
    # inversion (p2p_ddim_spatial_temporal.py:69-148)
    # ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare_latents_ddim_inverted(self, image, batch_size, num_images_per_prompt, text_embeddings,
                                      store_attention=False, prompt=None, generator=None, LOW_RESOURCE=True,
                                      save_path=None, latents=None):
        """`latents` (extension): start from given clean latents [1,4,F,h,w] instead of VAE-encoding `image`."""
        self.prepare_before_train_loop()
        # recompute_maps: the same inversion -- the store registered, the capturing launches, the running sum behind the cross-attention
        # strips -- with every iteration's maps written over the previous one's; what the store keeps is each iteration's input latent
        recompute = bool(store_attention and getattr(self.store_controller, "recompute", False))
        if recompute:
            self._refuse_issue_plans()
        if store_attention:
            attention_util.register_attention_control(self, self.store_controller)
        resource_default_value = self.store_controller.LOW_RESOURCE
        self.store_controller.LOW_RESOURCE = LOW_RESOURCE  # in inversion: no CFG, record every frame's attention
        batch_size = batch_size * num_images_per_prompt
        if latents is None:
            if isinstance(generator, list) and len(generator) != batch_size:
                raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an "
                                 f"effective batch size of {batch_size}. Make sure the batch size matches the length of "
                                 "the generators.")
            if isinstance(generator, list):
                init = torch.cat([self.vae.encode(image[i:i + 1]).latent_dist.sample(generator[i]) for i in range(batch_size)], 0)
            else:
                init = self.vae.encode(image).latent_dist.sample(generator)
            init = 0.18215 * init
            if batch_size > init.shape[0] and batch_size % init.shape[0] != 0:
                raise ValueError(f"Cannot duplicate `image` of batch size {init.shape[0]} to {batch_size} text prompts.")
            if batch_size > init.shape[0]:
                init = torch.cat([init] * (batch_size // init.shape[0]), dim=0)
            bf, c, h, w = init.shape
            latents = init.reshape(batch_size, bf // batch_size, c, h, w).permute(0, 2, 1, 3, 4)  # (b f) c h w -> b c f h w
        self.store_controller.expected_steps = len(self.scheduler.timesteps) if store_attention else None
        self.store_controller.latent_hw = tuple(latents.shape[-2:])  # the clip's own geometry: map sizes of every level follow from it
        if recompute:
            ddim_latents_all_step = self.ddim_clean2noisy_loop(latents, text_embeddings, self.store_controller, keep_source=True)
        else:
            ddim_latents_all_step = self.ddim_clean2noisy_loop(latents, text_embeddings, self.store_controller)
        if store_attention and (save_path is not None):
            os.makedirs(save_path + "/cross_attention", exist_ok=True)
            attention_util.show_cross_attention(self.tokenizer, prompt, self.store_controller, 16, ["up", "down"],
                                                save_path=save_path + "/cross_attention")
            attention_util.register_attention_control(self, self.empty_controller)  # detach the controller for safety
        self.store_controller.LOW_RESOURCE = resource_default_value
        return ddim_latents_all_step

    @torch.no_grad()
    def ddim_clean2noisy_loop(self, latent, text_embeddings, controller=None, keep_source=False):
        """`keep_source` (extension, recompute_maps): `controller` -- an AttentionStore(recompute=True) -- keeps what every iteration's
        forward is fed (this rank's frames of `latent`, the source context, the timesteps; the later inputs are its `latents_store`)."""
        weight_dtype = latent.dtype
        uncond_embeddings, cond_embeddings = text_embeddings.chunk(2)
        shard = self.frame_shard
        if shard is not None:
            latent = shard.local(latent, 2).contiguous()
        all_latent = [latent]
        state = _LatentState(latent.detach(), reps=1)
        cond = cond_embeddings.to(torch.float16)
        if keep_source:
            controller.begin_source_pass(latent, cond)
        timesteps = self.scheduler.timesteps
        with fz_dist.frame_sharded(shard):
            for i in self.progress_bar(range(len(timesteps))):
                t = int(timesteps[len(timesteps) - i - 1])
                if keep_source:
                    controller.source_timesteps.append(t)
                eps = self.unet.forward_tokens(state.tokens(), t, cond)
                cz, ce = self.scheduler.inverse_step_coefficients(t)
                state.update(None, eps.data, 0.0, cz, ce)
                cur = state.as_latents(weight_dtype).clone()
                if controller is not None:
                    controller.step_callback(cur)
                all_latent.append(cur)
        if shard is not None:
            all_latent = self._gather_frames(all_latent)
        return all_latent

    def next_clean2noise_step(self, model_output, timestep: int, sample):
        """Tensor form of the inverse DDIM step (p2p_ddim_spatial_temporal.py:150-161), eta = 0."""
        cz, ce = self.scheduler.inverse_step_coefficients(timestep)
        return cz * sample + ce * model_output

    def get_timesteps(self, num_inference_steps, strength, device):
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return self.scheduler.timesteps[t_start:], num_inference_steps - t_start

    # ------------------------------------------------------------------------------------------------------
    # editing (p2p_ddim_spatial_temporal.py:172-259)
    # ------------------------------------------------------------------------------------------------------
    def p2preplace_edit(self, **kwargs):
        len_source = len(kwargs["source_prompt"].split(" "))
        len_target = len(kwargs["prompt"].split(" "))
        equal_length = (len_source == len_target)
        edit_controller = attention_util.make_controller(
            self.tokenizer, [kwargs["source_prompt"], kwargs["prompt"]],
            NUM_DDIM_STEPS=kwargs["num_inference_steps"],
            is_replace_controller=kwargs.get("is_replace_controller", True) and equal_length,
            cross_replace_steps=kwargs["cross_replace_steps"], self_replace_steps=kwargs["self_replace_steps"],
            blend_words=kwargs.get("blend_words", None), equilizer_params=kwargs.get("eq_params", None),
            additional_attention_store=self.store_controller, use_inversion_attention=kwargs["use_inversion_attention"],
            blend_th=kwargs.get("blend_th", (0.3, 0.3)), blend_self_attention=kwargs.get("blend_self_attention", None),
            blend_latents=kwargs.get("blend_latents", None), save_path=kwargs.get("save_path", None),
            save_self_attention=kwargs.get("save_self_attention", True), disk_store=kwargs.get("disk_store", False),
            map_dtype=kwargs.get("map_dtype") or self.map_dtype)
        attention_util.register_attention_control(self, edit_controller)
        self.last_edit_controller = edit_controller
        sdimage_output = self.sd_ddim_pipeline(controller=edit_controller, **kwargs)
        # the blend-mask PNGs (save_path) were queued off-loop: all on disk from here on.  A failed dump (disk full, no PIL, dead writer)
        # does not cost the caller the finished edit, but it is not silent either: the errors ride in the result (`mask_dump_errors`)
        # beside the warning; FZ_STRICT_MASK_DUMPS=1 restores the reference's behaviour (its synchronous save_image raises)
        dump_errors = spatial_blend.flush_mask_dumps(raise_on_error=os.environ.get("FZ_STRICT_MASK_DUMPS") == "1")
        mask_list = edit_controller.latent_blend.mask_list if hasattr(edit_controller.latent_blend, "mask_list") else None
        attention_output = self._attention_strips(kwargs["prompt"], edit_controller)
        dict_output = {"sdimage_output": sdimage_output, "attention_output": attention_output, "mask_list": mask_list}
        if dump_errors:
            dict_output["mask_dump_errors"] = dump_errors
        attention_util.register_attention_control(self, self.empty_controller)
        return dict_output

    def _attention_strips(self, prompt, controller):
        """`show_cross_attention(tokenizer, prompt, controller, 16, ["up", "down"])` of the reference
        (p2p_ddim_spatial_temporal.py:211-215).  The reference crashes there when no 16x16 cross map exists (any input that
        is not 512x512: `torch.cat` of an empty list); here that case yields None."""
        if len(controller.attention_store.keys()) == 0:
            return None
        try:
            return attention_util.show_cross_attention(self.tokenizer, prompt, controller, 16, ["up", "down"])
        except ValueError:
            return None

    @torch.no_grad()
    def __call__(self, **kwargs):
        edit_type = kwargs["edit_type"]
        assert edit_type in ["save", "swap", None]
        asked = kwargs.get("recompute_maps")  # per call / per p2p_config entry: may only repeat what the inversion ran with
        if asked is not None and bool(asked) != self.recompute_maps:
            raise ValueError(f"recompute_maps={bool(asked)} for this edit, but the pipeline (and its inversion) runs with "
                             f"recompute_maps={self.recompute_maps}: what the inversion keeps decides the mode -- set it on the pipeline "
                             "(constructor / set_recompute_maps / editing_config.recompute_attention_maps) before the inversion")
        if self.recompute_maps and edit_type is not None and (edit_type == "save" or not kwargs.get("use_inversion_attention", False)):
            raise ValueError("recompute_maps=True needs use_inversion_attention=True: with use_inversion_attention=False the stored maps come "
                             "from an edit pass ('save', then 'swap'), there is no inversion forward to recompute them from")
        if edit_type is None:
            return self.sd_ddim_pipeline(controller=None, **kwargs)
        if edit_type == "save":
            del self.store_controller
            self.store_controller = attention_util.AttentionStore()
            attention_util.register_attention_control(self, self.store_controller)
            sdimage_output = self.sd_ddim_pipeline(controller=self.store_controller, **kwargs)
            attention_output = self._attention_strips(kwargs["prompt"], self.store_controller)
            dict_output = {"sdimage_output": sdimage_output, "attention_output": attention_output, "mask_list": None}
            attention_util.register_attention_control(self, self.empty_controller)
            return dict_output
        return self.p2preplace_edit(**kwargs)

    @torch.no_grad()
    def sd_ddim_pipeline(self, prompt: Union[str, List[str]], image=None, height: Optional[int] = None,
                         width: Optional[int] = None, strength: float = None, num_inference_steps: int = 50,
                         guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: Optional[int] = 1,
                         eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                         output_type: Optional[str] = "pil", return_dict: bool = True,
                         callback: Optional[Callable[[int, int, torch.Tensor], None]] = None,
                         callback_steps: Optional[int] = 1, controller=None, **args):
        """CFG DDIM denoise loop (p2p_ddim_spatial_temporal.py:261-435). `output_type='latent'` (extension) returns the
        final latents without a VAE."""
        # the frame size is the one of the latents / images handed in; an explicit height / width may only repeat it
        if latents is not None:
            given = (latents.shape[-2] * self.vae_scale_factor, latents.shape[-1] * self.vae_scale_factor)
        elif image is not None:
            given = tuple(image.shape[-2:])
        else:
            given = None
        if given is not None:
            for name, asked, have in (("height", height, given[0]), ("width", width, given[1])):
                if asked is not None and asked != have:
                    raise ValueError(f"`{name}`={asked} contradicts the {'latents' if latents is not None else 'images'} handed in, "
                                     f"which are {given[0]} x {given[1]} pixels (height x width)")
            height, width = given
        sample_size = getattr(self.unet.config, "sample_size", None) or 64
        height = height or sample_size * self.vae_scale_factor
        width = width or sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps, strength)
        if eta != 0.0:
            raise NotImplementedError("the editing path always runs eta = 0")
        batch_size = 1 if isinstance(prompt, str) else len(prompt)
        device = self._execution_device
        do_cfg = guidance_scale > 1.0
        text_embeddings = self._encode_prompt(prompt, device, num_images_per_prompt, do_cfg, negative_prompt)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        timesteps = self.scheduler.timesteps
        if latents is None:
            latents = self.prepare_latents_ddim_inverted(image, batch_size, num_images_per_prompt, text_embeddings,
                                                         store_attention=False, generator=generator)[-1]
        latents_dtype = latents.dtype
        if isinstance(controller, attention_util.AttentionControl):
            controller.latent_hw = tuple(latents.shape[-2:])
        shard = self.frame_shard
        if shard is not None:
            latents = shard.local(latents, 2).contiguous()
        state = _LatentState(latents.detach(), reps=2 if do_cfg else 1, share=shard is None)
        emb = text_embeddings.to(torch.float16)
        n_t = len(timesteps)
        recompute = (isinstance(controller, attention_util.AttentionControlEdit) and controller.use_inversion_attention
                     and getattr(controller.additional_attention_store, "recompute", False))
        if recompute:
            self._refuse_issue_plans()
        with fz_dist.frame_sharded(shard):
            for i, t in enumerate(self.progress_bar(timesteps)):
                t = int(t)
                if recompute:  # this step's stored maps: re-run the inversion forward they come from, into the one-step slab
                    self._recompute_source_maps(controller, state.f, state.h, state.w)
                eps = self.unet.forward_tokens(state.tokens(), t, emb).data
                cz, ce = self.scheduler.step_coefficients(t)
                if do_cfg:
                    state.update(eps[: state.f], eps[state.f:], guidance_scale, cz, ce)
                else:
                    state.update(None, eps, 0.0, cz, ce)
                if controller is not None:
                    cur = state.as_latents(latents_dtype)
                    new = controller.step_callback(cur)
                    if new is not cur:  # latent blend (attention_util.py:47-78) changed the latents
                        state.assign(new)
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, state.as_latents(latents_dtype).clone())  # the master buffer is updated in place
        latents = state.as_latents(latents_dtype).clone()
        if shard is not None:
            latents = self._gather_frames([latents])[0]
        if output_type == "latent":
            image = latents
        else:
            image = self.decode_latents(latents)
            if output_type == "pil":
                image = self.numpy_to_pil(image)
        if not return_dict:
            return (image, None)
        return StableDiffusionPipelineOutput(images=image, nsfw_content_detected=None)
