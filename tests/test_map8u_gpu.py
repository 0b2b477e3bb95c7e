"""Opt-in UE4M4 storage of the captured self-attention maps on the MI355X: the kernel cases of tests/test_map8u_emu.py through the C ABI of
libfatezero_hip.so, one launch at a real 16^2-level shape, a tiny whole job against the fp32 oracle, and the full-width comparison with E5M2."""
import pytest
import torch

import map8u_cases as U
from test_map8_gpu import MAP8_EDIT_TOL_VS_FP32  # the bound the E5M2 job was accepted at: the finer format has no excuse to exceed it

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_capture8u_stores_the_fp16_map_rounded_to_ue4m4(name):
    U.check_capture_bytes(U.kernel_case(name, DEV))


@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_inject8u_equals_fp16_inject_of_the_same_values(name):
    U.check_inject_same_bits(U.kernel_case(name, DEV))


@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_inject8u_against_fp32(name):
    U.check_inject_vs_fp32(U.kernel_case(name, DEV))


def test_real_16x16_level_shape():
    """8 frames, 8 heads, D = 80, 256 queries, two kv slots (512 keys): whole query tiles and whole key tiles, the vector paths only."""
    r = U.kernel_case(U.REAL_16x16[0], DEV, heads=U.REAL_16x16[2])
    U.check_capture_bytes(r)
    U.check_inject_same_bits(r)
    U.check_inject_vs_fp32(r)


def test_inversion_latents_do_not_depend_on_the_format():
    """tiny40 geometry, 2 frames, 32^2 latents, T = 2: the capture inversion with the UE4M4 arena returns the fp16 arena's latents bit for
    bit, its stored bytes are the fp16 job's maps rounded, and its arena is the size of the E5M2 one."""
    import pipeline_cases as PC
    from fatezero_amd import kernels as K
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    unet = PC.build_unet("tiny40", {"lora": 16}, DEV)
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(2, 77, 64, generator=g).to(DEV)
    z0 = torch.randn(1, 4, 2, 32, 32, generator=g).to(DEV)
    runs = {}
    for fmt in ("fp16", "e5m2", "ue4m4"):
        pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                             map_dtype=fmt)
        pipe.set_progress_bar_config(disable=True)
        pipe.scheduler.set_timesteps(2)
        lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True,
                                                 LOW_RESOURCE=True, latents=z0)
        runs[fmt] = (pipe, lat)
    for a, b in zip(runs["fp16"][1], runs["ue4m4"][1]):
        assert torch.equal(a, b)
    s16, s5, su = (runs[f][0].store_controller for f in ("fp16", "e5m2", "ue4m4"))
    assert su.arena_bytes == s5.arena_bytes < s16.arena_bytes
    n = 0
    for k in ("down_self", "mid_self", "up_self"):
        for cu, c16 in zip(su.maps_of_step(-1)[k], s16.maps_of_step(-1)[k]):
            n += 1
            assert cu.fmt == "ue4m4" and cu.storage.dtype == torch.uint8
            assert torch.equal(cu.storage.cpu(), K.half_to_ue4m4(c16.storage.cpu()))
            assert torch.equal(cu.view.cpu(), (cu.storage.cpu().to(torch.int16) << 6).view(torch.float16))
    assert n > 0


def test_whole_job_vs_fp32_oracle():
    """The tiny whole job in ue4m4 against the fp32 oracle (executed by torch on the GPU); the fp16 job's inversion and same-maps leg beside it
    for the stored-map bound.  Measured on MI355X (profiles/map8u_parity_numbers.txt): edit against the all-fp32 run, max / latent scale,
    ue4m4 0.940 % in this test and 1.082 % with all three formats in one run (e5m2 1.188 %, fp16 0.940 % there; the GPU-executed oracle is not
    bit-reproducible); stored self maps 4.08e-3 against fp16's 6.1e-4 + 2^-6."""
    ru = U.whole_job(DEV, "ue4m4", oracle_device=DEV)
    r16 = U.whole_job(DEV, "fp16", oracle_device=DEV, fp32_leg=False)
    show = ("inv_err", "inv_scale", "self_map_err", "map_err", "edit_scale", "edit_err_same_maps", "edit_err_same_maps_q99", "edit_err_vs_fp32",
            "edit_err_vs_fp32_q99", "attn_mask_flips_same_maps", "attn_mask_flips_vs_fp32", "attn_mask_total", "mask_ones_frac")
    print("map8u whole job ue4m4", {k: ru[k] for k in show})
    print("map8u whole job fp16 ", {k: r16[k] for k in show if k in r16})
    print("map8u whole job: edit vs the all-fp32 run / latent scale: ue4m4 %.4f %%, bound %.4f %%"
          % (100 * ru["edit_err_vs_fp32"] / ru["edit_scale"], 100 * MAP8_EDIT_TOL_VS_FP32))
    assert ru["outputs_finite"] and r16["outputs_finite"]
    assert abs(ru["inv_err"] - r16["inv_err"]) <= 1e-4 * r16["inv_scale"] and abs(ru["map_err"] - r16["map_err"]) <= 1e-4
    # stored self maps against the oracle's: the fp16 error plus half a UE4M4 step just below 1.0 (1.0 itself is representable)
    assert ru["self_map_err"] <= r16["self_map_err"] + 2.0 ** -6, (ru["self_map_err"], r16["self_map_err"])
    import pipeline_cases as PC
    assert ru["attn_mask_flips_same_maps"] == 0
    assert ru["edit_err_same_maps"] <= PC.GEO_EDIT_TOL_SAME_MAPS * ru["edit_scale"], ru["edit_err_same_maps"]
    assert ru["edit_err_same_maps_q99"] <= PC.GEO_EDIT_Q99_TOL * ru["edit_scale"]
    assert PC.FULL_MASK_BAND[0] <= ru["mask_ones_frac"] <= PC.FULL_MASK_BAND[1], ru["mask_ones_frac"]  # the mask does split the rows
    # the all-fp32 leg: the quantisation is on one side only
    assert ru["edit_err_vs_fp32"] <= MAP8_EDIT_TOL_VS_FP32 * ru["edit_scale"], (ru["edit_err_vs_fp32"], ru["edit_scale"])


def test_full_width_edit_deviates_less_from_the_fp16_arena_than_e5m2():
    """Every self-attention row of every edit step takes the stored map: tiny40 geometry, 2 frames, 32^2 latents, T = 2.  Required: rms
    deviation of the edited latents from the fp16-arena job smaller for ue4m4 than for e5m2; max and ratios are printed (measured:
    e5m2 max 0.506 % / rms 0.1149 % of the latent scale, ue4m4 0.378 % / 0.0840 %: rms ratio 1.37, max ratio 1.34)."""
    U.finer_than_e5m2(DEV, kind="tiny40", frames=2, L=32, T=2)
