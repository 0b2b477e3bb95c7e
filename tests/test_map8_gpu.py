"""Opt-in E5M2 storage of the captured self-attention maps on the MI355X: the kernel cases of tests/test_map8_emu.py through the C ABI of
libfatezero_hip.so, one launch at a real 16^2-level shape, and a tiny whole job against the fp32 oracle."""
import pytest
import torch

import map8_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Edited latents of the 8-bit whole job against the all-fp32 oracle run, max / latent scale: 1.5 x the 8-bit job's own value measured on
# MI355X (the margin MASK_FLIP_TOL uses for box-to-box fp16 reordering).  Measured against the same oracle (profiles/map8_parity_numbers.txt):
# E5M2 arena 1.057 %, fp16 arena 1.022 % -- 1.034 x; no attention-blend mask pixel flipped in either job.
MAP8_MEASURED = dict(e5m2=1.0573e-2, fp16=1.0221e-2)
MAP8_EDIT_TOL_VS_FP32 = 1.5 * MAP8_MEASURED["e5m2"]


@pytest.mark.parametrize("name", list(M.KERNEL_CASES))
def test_capture8_stores_the_fp16_map_rounded_to_e5m2(name):
    M.check_capture8_bytes(M.kernel_case(name, DEV))


@pytest.mark.parametrize("name", list(M.KERNEL_CASES))
def test_inject8_equals_fp16_inject_of_the_same_values(name):
    M.check_inject8_same_bits(M.kernel_case(name, DEV))


@pytest.mark.parametrize("name", list(M.KERNEL_CASES))
def test_inject8_against_fp32(name):
    M.check_inject8_vs_fp32(M.kernel_case(name, DEV))


def test_real_16x16_level_shape():
    """8 frames, 8 heads, D = 80, 256 queries, two kv slots (512 keys): whole 128-row query tiles and whole 64-key tiles -- the vector paths
    only (64-byte row segments out, two 16-byte loads per lane and tile in)."""
    r = M.kernel_case(M.REAL_16x16[0], DEV, heads=M.REAL_16x16[2])
    M.check_capture8_bytes(r)
    M.check_inject8_same_bits(r)
    M.check_inject8_vs_fp32(r)


def test_whole_job_vs_fp32_oracle():
    """The tiny whole job in both formats against the same fp32 oracle (executed by torch on the GPU, as the fp16 whole-job cases do)."""
    r8 = M.whole_job(DEV, "e5m2", oracle_device=DEV)
    r16 = M.whole_job(DEV, "fp16", oracle_device=DEV)
    show = ("inv_err", "inv_scale", "self_map_err", "map_err", "edit_scale", "edit_err_same_maps", "edit_err_same_maps_q99", "edit_err_vs_fp32",
            "edit_err_vs_fp32_q99", "attn_mask_flips_same_maps", "attn_mask_flips_vs_fp32", "attn_mask_total", "mask_ones_frac")
    print("map8 whole job e5m2", {k: r8[k] for k in show})
    print("map8 whole job fp16", {k: r16[k] for k in show})
    assert r8["outputs_finite"] and r16["outputs_finite"]
    # the inversion does not see the format (bit for bit: test_inversion_latents_do_not_depend_on_the_format below; the GPU-executed oracle is
    # not bit-reproducible run to run, so the two error figures agree only to its noise)
    assert abs(r8["inv_err"] - r16["inv_err"]) <= 1e-4 * r16["inv_scale"] and abs(r8["map_err"] - r16["map_err"]) <= 1e-4
    # stored self maps against the oracle's: the fp16 error plus at most half an E5M2 step of a probability <= 1 (2^-3 relative)
    assert r8["self_map_err"] <= r16["self_map_err"] + 2.0 ** -3
    # identical stored maps on both sides (the oracle reads the dequantised maps): the attention-blend masks are bit-exact, and the edit is
    # within the bounds of the fp16 cases -- the quantisation is on both sides of this comparison
    import pipeline_cases as PC
    assert r8["attn_mask_flips_same_maps"] == 0
    assert r8["edit_err_same_maps"] <= PC.GEO_EDIT_TOL_SAME_MAPS * r8["edit_scale"], r8["edit_err_same_maps"]
    assert r8["edit_err_same_maps_q99"] <= PC.GEO_EDIT_Q99_TOL * r8["edit_scale"]
    assert PC.FULL_MASK_BAND[0] <= r8["mask_ones_frac"] <= PC.FULL_MASK_BAND[1], r8["mask_ones_frac"]  # the mask does split the rows
    # the all-fp32 leg: HERE the quantisation is on one side only.  Mask flips are reported (above), not bounded.
    assert r8["edit_err_vs_fp32"] <= MAP8_EDIT_TOL_VS_FP32 * r8["edit_scale"], (r8["edit_err_vs_fp32"], r8["edit_scale"])


def test_inversion_latents_do_not_depend_on_the_format():
    """tiny40 geometry, 2 frames, 32^2 latents, T = 2: the capture inversion with the E5M2 arena returns the fp16 arena's latents bit for
    bit, and its stored bytes are the fp16 job's maps rounded."""
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    unet = PC.build_unet("tiny40", {"lora": 16}, DEV)
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(2, 77, 64, generator=g).to(DEV)
    z0 = torch.randn(1, 4, 2, 32, 32, generator=g).to(DEV)
    runs = {}
    for fmt in ("fp16", "e5m2"):
        pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                             map_dtype=fmt)
        pipe.set_progress_bar_config(disable=True)
        pipe.scheduler.set_timesteps(2)
        lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True,
                                                 LOW_RESOURCE=True, latents=z0)
        runs[fmt] = (pipe, lat)
    for a, b in zip(runs["fp16"][1], runs["e5m2"][1]):
        assert torch.equal(a, b)
    s16, s8 = runs["fp16"][0].store_controller, runs["e5m2"][0].store_controller
    assert s8.arena_bytes < s16.arena_bytes
    for k in ("down_self", "mid_self", "up_self"):
        for cm8, cm16 in zip(s8.maps_of_step(-1)[k], s16.maps_of_step(-1)[k]):
            assert cm8.storage.dtype == torch.uint8
            assert torch.equal(cm8.storage.cpu(), cm16.storage.cpu().to(torch.float8_e5m2).view(torch.uint8))
            assert torch.equal(cm8.view.cpu(), cm8.storage.cpu().view(torch.float8_e5m2).to(torch.float16))
