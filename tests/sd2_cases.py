"""SD-2.x cases shared by tests/test_sd2_emu.py (CPU emulation) and tests/test_sd2_gpu.py (MI355X): the tiny SD-2-shaped UNets recorded
from the unmodified reference (scripts/gen_golden_sd2.py), an fp32 restatement of the SD-2 UNet for shapes no recording reaches, the
SD-2 pipeline scenario, and a synthetic SD-2 checkpoint folder in the on-disk layout of stable-diffusion-2-base."""
import contextlib
import json
import os

import torch

import pipeline_cases as PC
from test_cli_emu import synthetic_checkpoint as _sd1_checkpoint
from helpers import load_json, load_npz
from oracle import fatezero_oracle as O
from oracle.weights import procedural_state_dict

from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel

# stable-diffusion-2-base's unet/config.json as a newer diffusers writes it (the keys after `upcast_attention` are that version's
# additions, each at its default)
SD2_BASE_UNET = {
    "_class_name": "UNet2DConditionModel", "_diffusers_version": "0.21.0", "act_fn": "silu", "attention_head_dim": [5, 10, 20, 20],
    "block_out_channels": [320, 640, 1280, 1280], "center_input_sample": False, "cross_attention_dim": 1024,
    "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    "downsample_padding": 1, "dual_cross_attention": False, "flip_sin_to_cos": True, "freq_shift": 0, "in_channels": 4,
    "layers_per_block": 2, "mid_block_scale_factor": 1, "norm_eps": 1e-05, "norm_num_groups": 32, "num_class_embeds": None,
    "only_cross_attention": False, "out_channels": 4, "sample_size": 64,
    "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"],
    "use_linear_projection": True, "upcast_attention": False,
    "addition_embed_type": None, "addition_embed_type_num_heads": 64, "addition_time_embed_dim": None, "attention_type": "default",
    "class_embed_type": None, "class_embeddings_concat": False, "conv_in_kernel": 3, "conv_out_kernel": 3, "cross_attention_norm": None,
    "dropout": 0.0, "encoder_hid_dim": None, "encoder_hid_dim_type": None, "mid_block_only_cross_attention": None,
    "mid_block_type": "UNetMidBlock2DCrossAttn", "num_attention_heads": None, "projection_class_embeddings_input_dim": None,
    "resnet_out_scale_factor": 1.0, "resnet_skip_time_act": False, "resnet_time_scale_shift": "default",
    "reverse_transformer_layers_per_block": None, "time_cond_proj_dim": None, "time_embedding_act_fn": None,
    "time_embedding_dim": None, "time_embedding_type": "positional", "timestep_post_act": None, "transformer_layers_per_block": 1,
}
SD2_BASE_SCHEDULER = {
    "_class_name": "PNDMScheduler", "_diffusers_version": "0.21.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
    "beta_start": 0.00085, "clip_sample": False, "num_train_timesteps": 1000, "prediction_type": "epsilon", "set_alpha_to_one": False,
    "skip_prk_steps": True, "steps_offset": 1, "timestep_spacing": "leading", "trained_betas": None,
}
SD2_BASE_TEXT = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                     max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, bos_token_id=0, eos_token_id=2, pad_token_id=1,
                     projection_dim=512)
SD2_FULL = {k: SD2_BASE_UNET[k] for k in ("block_out_channels", "norm_num_groups", "cross_attention_dim", "attention_head_dim",
                                           "use_linear_projection")}


def sd2_arch(kind):
    """The tiny architecture of a recording (kept in sd2_unet_meta.json by the recorder)."""
    for m in load_json("sd2_unet_meta.json").values():
        if m["kind"] == kind:
            return dict(m["arch"])
    raise KeyError(kind)


def build_sd2_unet(arch, model_config, device, dtype=torch.float16, seed=0):
    unet = UNetPseudo3DConditionModel(sample_size=64, **arch, **model_config)
    shapes = [(k, tuple(v.shape)) for k, v in unet.state_dict().items()]
    unet.load_state_dict(procedural_state_dict(shapes, seed))
    return unet.to(dtype).to(device).eval(), shapes


class SD2OracleUNet(O.OracleUNet):
    """fp32 restatement of the SD-2.x UNet on top of the SD-1.x one (oracle/fatezero_oracle.py): a head count per channel width (the
    `attention_head_dim` list; the temporal attention uses the block's count, attention.py:215-222) and Linear proj_in / proj_out,
    which on the '(h w) c' rows are the 1x1 convolution of the same [C, C] matrix.  Pinned on CPU to the reference's recordings."""

    def __init__(self, state_dict, arch, model_config=None, device=None):
        sd = {k: (v[:, :, None, None] if (k.endswith("proj_in.weight") or k.endswith("proj_out.weight")) and v.dim() == 2 else v)
              for k, v in state_dict.items()}
        heads = arch["attention_head_dim"]
        heads = [heads] * 4 if isinstance(heads, int) else list(heads)
        cfg = O.UNetConfig(block_out_channels=arch["block_out_channels"], attention_head_dim=heads[0],
                           cross_attention_dim=arch["cross_attention_dim"], norm_num_groups=arch["norm_num_groups"],
                           model_config=model_config)
        super().__init__(sd, cfg, device=device)
        self.heads_of = {}
        for i, name in enumerate(("down_blocks.0", "down_blocks.1", "down_blocks.2")):
            self.heads_of[name] = heads[i]
        self.heads_of["mid_block"] = heads[-1]
        for i, h in enumerate(reversed(heads)):
            self.heads_of[f"up_blocks.{i}"] = h

    def _transformer(self, x, ctx, name, place, controller):
        self.cfg.heads = self.heads_of[name.rsplit(".attentions", 1)[0]]
        return super()._transformer(x, ctx, name, place, controller)


def run_sd2_unet_golden(name, device):
    """Native forward on a recording of the unmodified reference."""
    m = load_json("sd2_unet_meta.json")[name]
    g = load_npz(name + ".npz")
    unet, _ = build_sd2_unet(m["arch"], m["model_config"], device)
    x, ctx = torch.from_numpy(g["x"]), torch.from_numpy(g["ctx"])
    y = unet(x.to(device), int(g["t"]), ctx.to(device)).sample.float().cpu()
    ref = torch.from_numpy(g["y"])
    return {"err": float((y - ref).abs().max()), "scale": float(ref.abs().max())}


def run_sd2_oracle_golden(name):
    m = load_json("sd2_unet_meta.json")[name]
    g = load_npz(name + ".npz")
    sd = procedural_state_dict([(n, tuple(s)) for n, s in m["state_dict_shapes"]])
    ou = SD2OracleUNet(sd, m["arch"], m["model_config"])
    y = ou(torch.from_numpy(g["x"]), int(g["t"]), torch.from_numpy(g["ctx"]))
    ref = torch.from_numpy(g["y"])
    return {"err": float((y - ref).abs().max()), "scale": float(ref.abs().max())}


def sd2_oracle_edit_on_native_maps(kind, meta, consts, gz, store, tok):
    """pipeline_cases.oracle_edit_on_native_maps with the SD-2 restatement: the fp32 oracle's edit pass on the maps / latents captured
    by the NATIVE inversion.  With identical inversion maps on both sides the attention-blend masks must agree bit for bit."""
    um = next(m for m in load_json("sd2_unet_meta.json").values() if m["kind"] == kind and m["model_config"] == meta["model_config"])
    unet = SD2OracleUNet(procedural_state_dict([(n, tuple(s)) for n, s in um["state_dict_shapes"]]), um["arch"], meta["model_config"])
    ost = O.StoreController()
    ost.attention_store_all_step = [{k: [t.float().cpu() for t in v] for k, v in d.items()}
                                    for d in store.attention_store_all_step]
    ost.latents_store = [t.float().cpu() for t in store.latents_store]
    kw = meta["kwargs"]
    ctrl = O.make_edit_controller(
        tok, consts["prompts"], ost, meta["T"], kw["is_replace_controller"], dict(kw["cross_replace_steps"]),
        kw["self_replace_steps"], blend_words=kw.get("blend_words"), eq_params=kw.get("eq_params"),
        blend_th=tuple(kw["blend_th"]), blend_self_attention=kw.get("blend_self_attention", False),
        blend_latents=kw.get("blend_latents", False), save_self_attention=kw["save_self_attention"])
    edited = O.ddim_edit(unet, O.DDIMSchedule(meta["T"]), torch.from_numpy(gz["zT"]), torch.from_numpy(gz["emb_tgt"]), ctrl,
                         guidance_scale=kw["guidance_scale"])
    return edited, ctrl


@contextlib.contextmanager
def _sd2_pipeline_fixtures(kind):
    """pipeline_cases.run_pipeline_case on the SD-2 recording: the tiny SD-2 net instead of tiny16, the sd2_* fixture files, and the
    SD-2 restatement for its oracle-on-native-maps leg."""
    saved = PC.build_unet, PC.load_json, PC.load_npz, PC.oracle_edit_on_native_maps
    arch = sd2_arch(kind)
    PC.build_unet = lambda _kind, mc, device: build_sd2_unet(arch, mc, device)[0]
    PC.load_json = lambda name: load_json({"pipeline_meta.json": "sd2_pipeline_meta.json"}.get(name, name))
    PC.load_npz = lambda name: load_npz(name)
    PC.oracle_edit_on_native_maps = lambda *a: sd2_oracle_edit_on_native_maps(kind, *a)
    try:
        yield
    finally:
        PC.build_unet, PC.load_json, PC.load_npz, PC.oracle_edit_on_native_maps = saved


def run_sd2_pipeline_case(device, name="sd2_pipe_replace_blend", mixed_oracle=True):
    """The SD-2 whole job (inversion with capture + Replace edit with attention blend, T = 4 + 4) against the reference recording and,
    `mixed_oracle`, against the fp32 oracle's edit on the native inversion maps (0 attention-blend mask flips asserted by PC.check)."""
    kind = load_json("sd2_pipeline_meta.json")[name]["sd2_kind"]
    with _sd2_pipeline_fixtures(kind):
        return PC.run_pipeline_case(name, device, mixed_oracle=mixed_oracle)


def write_sd2_checkpoint(root, tiny_kind="sd2_d64"):
    """<root>/{tokenizer,text_encoder,vae,unet,scheduler}: SD-2-base's configs (newer-diffusers keys included) at tiny widths with
    procedural weights; the tokenizer pads with '!' like SD-2's OpenCLIP tokenizer."""
    from fatezero_amd.video_diffusion.models.clip_text import CLIPTextModel
    _sd1_checkpoint(root)  # the SD-1.x-shaped folder; the parts SD-2 changes are rewritten below
    arch = sd2_arch(tiny_kind)
    cfg = dict(SD2_BASE_UNET, **{k: v for k, v in arch.items()})
    json.dump(cfg, open(os.path.join(root, "unet", "config.json"), "w"))
    os.remove(os.path.join(root, "unet", "diffusion_pytorch_model.bin"))
    blank = UNetPseudo3DConditionModel.from_2d_model(os.path.join(root, "unet"), {"lora": 16})
    sd2 = {k: v for k, v in procedural_state_dict([(k, tuple(v.shape)) for k, v in blank.state_dict().items()]).items()
           if "_temporal" not in k}
    torch.save(sd2, os.path.join(root, "unet", "diffusion_pytorch_model.bin"))
    tdir = os.path.join(root, "text_encoder")
    tcfg = json.load(open(os.path.join(tdir, "config.json")))
    tcfg.update(hidden_size=arch["cross_attention_dim"], hidden_act="gelu", num_attention_heads=2)
    torch.manual_seed(1)
    te = CLIPTextModel(tcfg)
    json.dump(tcfg, open(os.path.join(tdir, "config.json"), "w"))
    torch.save(te.state_dict(), os.path.join(tdir, "pytorch_model.bin"))
    json.dump(SD2_BASE_SCHEDULER, open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    tok = os.path.join(root, "tokenizer")
    special = {"bos_token": {"content": "<|startoftext|>"}, "eos_token": {"content": "<|endoftext|>"}, "pad_token": "!",
               "unk_token": {"content": "<|endoftext|>"}}
    json.dump(special, open(os.path.join(tok, "special_tokens_map.json"), "w"))
    tc = os.path.join(tok, "tokenizer_config.json")
    if os.path.exists(tc):
        os.remove(tc)
    return sd2
