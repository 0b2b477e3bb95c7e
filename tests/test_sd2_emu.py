"""Stable Diffusion 2.x (epsilon prediction) checkpoints on the CPU emulation: the UNet surface (Linear proj_in / proj_out, per-level
heads, a non-768 context, upcast_attention) against vectors recorded from the unmodified reference (scripts/gen_golden_sd2.py), the
configs of a stable-diffusion-2-base folder through the loaders and the YAML entry point, the tokenizer's '!' padding, the gelu text
encoder against transformers, and which fused chains an SD-2 block takes."""
import json
import os

import pytest
import torch

from fatezero_amd import _native, build
from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
from fatezero_amd.video_diffusion.schedulers import DDIMScheduler

import sd2_cases as S

UNET_TOL = 1.5e-2  # max |err| / max |y|: the tolerance of the SD-1.x tiny-UNet goldens (tests/test_pipeline_emu.py)


@pytest.fixture()
def emu_backend():
    _native.use_test_backend(build.build_emu())
    yield
    _native.reset_backend()


# ---------------------------------------------------------------------------------------------------------------- model surface
def test_linear_projection_keys_and_shapes_are_the_references():
    arch = S.sd2_arch("sd2_d64")
    unet = UNetPseudo3DConditionModel(sample_size=64, **arch, lora=16)  # (the recording's model_config)
    sd = unet.state_dict()
    want = {n: tuple(s) for n, s in S.load_json("sd2_unet_meta.json")["sd2_unet_d64"]["state_dict_shapes"]}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sd["down_blocks.0.attentions.0.proj_in.weight"].shape == (64, 64)
    assert sd["up_blocks.3.attentions.2.proj_out.weight"].shape == (64, 64)
    assert unet.config.use_linear_projection is True


def test_per_level_heads_follow_the_list_and_temporal_heads_match():
    unet = UNetPseudo3DConditionModel(sample_size=64, **S.sd2_arch("sd2_mixed_upcast"))
    blocks = {"down_blocks.0": 2, "down_blocks.1": 2, "down_blocks.2": 4, "mid_block": 4, "up_blocks.1": 4, "up_blocks.2": 2,
              "up_blocks.3": 2}
    for name, heads in blocks.items():
        tb = unet.get_submodule(name + ".attentions.0.transformer_blocks.0")
        assert tb.attn1.heads == tb.attn2.heads == tb.attn_temporal.heads == heads, name
    assert unet.get_submodule("down_blocks.0.attentions.0.transformer_blocks.0.attn2").to_k.weight.shape[1] == 96


@pytest.mark.parametrize("name", ["sd2_unet_d64", "sd2_unet_mixed_upcast"])
def test_sd2_unet_reference_golden_emu(name, emu_backend):
    r = S.run_sd2_unet_golden(name, "cpu")
    print(name, r)
    assert r["err"] <= UNET_TOL * r["scale"], r


@pytest.mark.parametrize("name", ["sd2_unet_d64", "sd2_unet_mixed_upcast"])
def test_sd2_fp32_restatement_matches_reference(name):
    # the restatement the full-width GPU test compares against, pinned to the reference here
    r = S.run_sd2_oracle_golden(name)
    print(name, r)
    assert r["err"] <= 1e-4 * r["scale"], r


def test_sd2_pipeline_reference_golden_emu(emu_backend):
    """Inversion (capture) + a 4-step Replace edit with attention blend on the SD-2-shaped net, against the reference run."""
    import pipeline_cases as PC
    res = S.run_sd2_pipeline_case("cpu")
    print(res)
    PC.check(res)
    assert res["attn_mask_total"] > 0
    assert res["attn_mask_flips_same_maps"] == 0  # (PC.check asserts it too; stated here as the point of the case)


def test_unknown_newer_unet_keys_are_rejected():
    arch = S.sd2_arch("sd2_d64")
    UNetPseudo3DConditionModel(sample_size=64, **arch, time_embedding_type="positional", conv_in_kernel=3,
                               transformer_layers_per_block=1, num_attention_heads=None, upcast_attention=True)
    for key, bad in [("time_embedding_type", "fourier"), ("conv_in_kernel", 7), ("transformer_layers_per_block", 2),
                     ("addition_embed_type", "text_time"), ("num_attention_heads", [2, 2, 2, 2])]:
        with pytest.raises(NotImplementedError, match=key):
            UNetPseudo3DConditionModel(sample_size=64, **arch, **{key: bad})
    with pytest.raises(NotImplementedError):
        UNetPseudo3DConditionModel(sample_size=64, **arch, only_cross_attention=[True, False, False, False])


def test_from_2d_model_loads_an_sd2_base_unet_folder(tmp_path):
    folder = tmp_path / "unet"
    os.makedirs(folder)
    cfg = dict(S.SD2_BASE_UNET, **S.sd2_arch("sd2_d64"))
    json.dump(cfg, open(folder / "config.json", "w"))
    blank = UNetPseudo3DConditionModel.from_2d_model(str(folder), {"lora": 16})
    sd2 = {k: torch.randn(v.shape) * 0.05 for k, v in blank.state_dict().items() if "_temporal" not in k}
    assert sd2["down_blocks.1.attentions.1.proj_in.weight"].dim() == 2
    from safetensors.torch import save_file
    save_file(sd2, str(folder / "diffusion_pytorch_model.safetensors"))
    model = UNetPseudo3DConditionModel.from_2d_model(str(folder), {"lora": 16})
    sd3 = model.state_dict()
    for k, v in sd2.items():
        assert torch.equal(sd3[k], v), k
    with pytest.raises(ValueError):  # an SD-1.x-shaped (1x1 conv) proj_in does not load into the linear form
        model.load_2d_state_dict({**sd2, "down_blocks.0.attentions.0.proj_in.weight": torch.zeros(64, 64, 1, 1)})


# ---------------------------------------------------------------------------------------------------------------- scheduler
def test_scheduler_accepts_sd2_base_config(tmp_path):
    os.makedirs(tmp_path / "scheduler")
    json.dump(S.SD2_BASE_SCHEDULER, open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    s = DDIMScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    s.set_timesteps(50)
    ref = DDIMScheduler()
    ref.set_timesteps(50)
    assert torch.equal(s.timesteps, ref.timesteps) and torch.equal(s.alphas_cumprod, ref.alphas_cumprod)
    DDIMScheduler.from_config(dict(S.SD2_BASE_SCHEDULER, thresholding=False, rescale_betas_zero_snr=False,
                                   dynamic_thresholding_ratio=0.995, sample_max_value=1.0))


@pytest.mark.parametrize("key,bad", [("timestep_spacing", "trailing"), ("thresholding", True), ("rescale_betas_zero_snr", True),
                                     ("trained_betas", [0.1] * 1000)])
def test_scheduler_rejects_non_default_newer_keys(key, bad):
    with pytest.raises(NotImplementedError, match=key):
        DDIMScheduler.from_config(dict(S.SD2_BASE_SCHEDULER, **{key: bad}))


def test_v_prediction_is_refused_with_its_reason():
    with pytest.raises(NotImplementedError, match="epsilon"):
        DDIMScheduler.from_config(dict(S.SD2_BASE_SCHEDULER, prediction_type="v_prediction"))


# ---------------------------------------------------------------------------------------------------------------- tokenizer / text encoder
def test_tokenizer_pads_with_exclamation_mark(tmp_path):
    from fatezero_amd.video_diffusion.models.clip_text import CLIPTokenizer
    from test_clip_text_emu import synthetic_bpe
    folder = str(tmp_path / "tokenizer")
    synthetic_bpe(folder)
    sd1 = CLIPTokenizer.from_pretrained(folder)
    if os.path.exists(os.path.join(folder, "tokenizer_config.json")):
        os.remove(os.path.join(folder, "tokenizer_config.json"))
    json.dump({"pad_token": "!", "bos_token": {"content": "<|startoftext|>"}, "eos_token": {"content": "<|endoftext|>"}},
              open(os.path.join(folder, "special_tokens_map.json"), "w"))
    tok = CLIPTokenizer.from_pretrained(folder)
    assert tok.pad_token == "!" and tok.pad_token_id == 0
    ids = tok("a silver jeep", padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids[0]
    ids1 = sd1("a silver jeep", padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids[0]
    n = int((ids1 != sd1.eos_token_id).sum()) + 1  # bos, words, eos
    assert torch.equal(ids[:n], ids1[:n]) and int(ids[n - 1]) == tok.eos_token_id
    assert (ids[n:] == 0).all() and (ids1[n:] == sd1.eos_token_id).all()
    # tokenizer_config.json wins over special_tokens_map.json (transformers' order)
    json.dump({"pad_token": "<|endoftext|>"}, open(os.path.join(folder, "tokenizer_config.json"), "w"))
    assert CLIPTokenizer.from_pretrained(folder).pad_token_id == sd1.eos_token_id


def test_gelu_text_encoder_matches_transformers(emu_backend):
    """SD-2's text tower (hidden_act gelu) at a tiny width against transformers' CLIPTextModel built from the same config."""
    transformers = pytest.importorskip("transformers")
    from fatezero_amd.video_diffusion.models.clip_text import CLIPTextModel
    cfg = dict(S.SD2_BASE_TEXT, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, vocab_size=1000)
    torch.manual_seed(0)
    ref = transformers.CLIPTextModel(transformers.CLIPTextConfig(**cfg)).eval()
    mine = CLIPTextModel(cfg)
    mine.load_state_dict(ref.state_dict())
    ids = torch.tensor([[0 + 998, 5, 17, 300, 999] + [0] * 72])  # bos-like, words, eos = the largest id, '!' padding (id 0)
    with torch.no_grad():
        want = ref(ids).last_hidden_state
    got = mine(ids)[0].float()
    err = float((got - want).abs().max())
    print("gelu text encoder err", err, float(want.abs().max()))
    assert err <= 1e-2 * float(want.abs().max()), err
    assert mine.config.hidden_act == "gelu"


# ---------------------------------------------------------------------------------------------------------------- fused chains
def test_chain_eligibility_at_sd2_shapes(emu_backend):
    """fz_xattn_chain is specialised to 8 heads of 40: at SD-2's 5 x 64 the 320-wide cross-attention declines it (three launches);
    fz_ff_chain does not depend on heads and stays on, exactly as for SD-1.x at the same rows."""
    from fatezero_amd import kernels as K
    from fatezero_amd.video_diffusion.models.attention import SpatioTemporalTransformerModel
    rows_per_frame, frames = 4096, 16
    sd2 = SpatioTemporalTransformerModel(5, 64, in_channels=320, cross_attention_dim=1024, use_linear_projection=True)
    sd1 = SpatioTemporalTransformerModel(8, 40, in_channels=320, cross_attention_dim=768)
    ctx2 = torch.zeros(2, 77, 1024, dtype=torch.float16)
    ctx1 = torch.zeros(2, 77, 768, dtype=torch.float16)
    a2, a1 = sd2.transformer_blocks[0].attn2, sd1.transformer_blocks[0].attn2
    assert a1._chain_applies(frames, rows_per_frame, 320, torch.float16, ctx1)
    assert not a2._chain_applies(frames, rows_per_frame, 320, torch.float16, ctx2)
    assert not K.xattn_chain_preferred(frames * rows_per_frame, rows_per_frame, 320, 5, 77)
    assert K.ff_chain_preferred(frames * rows_per_frame, 320, 1280)


# ---------------------------------------------------------------------------------------------------------------- YAML entry point
def test_cli_runs_a_yaml_job_on_an_sd2_base_folder(tmp_path, emu_backend, monkeypatch):
    import test_cli_emu as CE
    monkeypatch.setattr(CE, "synthetic_checkpoint", S.write_sd2_checkpoint)
    out = CE.run_cli_job(tmp_path, "cpu")
    assert len(out["samples"]) == 2
    from fatezero_amd.video_diffusion.models.clip_text import CLIPTokenizer
    tok = CLIPTokenizer.from_pretrained(str(tmp_path / "ckpt"), subfolder="tokenizer")
    assert tok.pad_token == "!"
