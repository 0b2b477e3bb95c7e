"""Rectangular (widescreen / portrait) clips on MI355X: the blend-mask kernel on res_h x res_w maps, the edit controller on 40 x 64 latents
against the fp32 oracle (executed by torch on the GPU, as the geometry cases of tests/test_pipeline_gpu.py do), and the rectangular launches
of the convolutions, the UNet and the VAE through the library's own dispatch."""
import pytest
import torch

import kernel_cases as KC
import pipeline_cases as PC
import rect_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- A. blend mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_hw,out_hw,prompts,or_first", RC.BLEND_CASES, ids=RC.BLEND_IDS)
def test_blend_mask_hw_bit_exact(map_hw, out_hw, prompts, or_first):
    for seed in (0, 1, 2):
        RC.case_blend_mask_hw(DEV, map_hw=map_hw, out_hw=out_hw, prompts=prompts, or_first=or_first, frames=8, heads=8, seed=seed)


def test_square_entry_is_the_hw_entry_with_equal_sides():
    RC.case_square_entry_equals_hw_entry(DEV, frames=8, heads=8)


def test_map_beyond_bm_max_pix_is_a_bad_argument():
    RC.case_oversized_map_is_refused(DEV)


# ---- C. the controller on a rectangular job -------------------------------------------------------------------------------------------
def test_edit_controller_on_rectangular_latents(tmp_path):
    """tiny40, F = 4, T = 4, 40 x 64 latents, Replace + blend words + attention blend + latent blend: see tests/test_rect_emu.py."""
    RC.check_rect_job(RC.run_rect_job(DEV, kind="tiny40", F_=4, T=4, hw=(40, 64), oracle_device=DEV, save_path=str(tmp_path / "masks")))


# ---- D. rectangular launches through the library's own dispatch ----------------------------------------------------------------------
# The shape classes of the halo kernel's rule (256 % w == 0 and whole 256-pixel tiles per frame or whole frames per tile), each with the tile
# the LIBRARY picks for it (tile_cfg = 0: at these small launches mostly the implicit GEMM, whose tiles then straddle rows of unequal h, w).
@pytest.mark.parametrize("kw", [
    dict(n=2, h=8, w=32, cin=64, cout=160),      # a frame is one 256-pixel tile
    dict(n=2, h=40, w=64, cin=64, cout=160),     # ten tiles per frame, h != w
    dict(n=2, h=40, w=64, cin=64, cout=64),      # 64 output channels: the narrow form's class
    dict(n=2, h=20, w=32, cin=64, cout=160),     # 640 pixels: neither whole tiles nor whole frames per tile, the implicit GEMM
    dict(n=4, h=4, w=16, cin=64, cout=160),      # four frames per tile
    dict(n=2, h=40, w=64, cin=64, cout=160, stride=2),      # -> 20 x 32
    dict(n=2, h=10, w=16, cin=64, cout=160, upsample=True),  # -> 20 x 32, nine taps on the upsampled frame
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_conv3x3_rectangular_own_dispatch(kw):
    print(kw, KC.case_conv3x3(DEV, **kw))


def test_conv3x3_up2_rectangular():
    """The sub-pixel form of the upsampler.  10 x 16 (160 pixels: 256 is no multiple of it) is outside what the halo kernel carries -- the
    library says so and the UNet takes fz_conv3x3(upsample = 1) there (the case above); the form itself runs on the rectangular shape next to
    it that the kernel carries, 8 x 32 -> 16 x 64."""
    from fatezero_amd import kernels as K
    assert not K.conv3x3_up2_ok(2, 10, 16, 64, 160) and not K.conv3x3_up2_preferred(2, 10, 16, 64, 160)
    print(KC.case_conv3x3_up2(DEV, n=2, h=8, w=32, cin=64, cout=160))


@pytest.mark.parametrize("hw", [(40, 64), (64, 40)], ids=["40x64", "64x40"])
def test_unet_forward_rectangular(hw):
    r = RC.run_unet_forward_hw(DEV, hw, kind="tiny40", F_=4, oracle_device=DEV)
    print(r)
    assert r["err"] <= PC.FULL_LATENT_TOL * r["scale"], r


def test_vae_roundtrip_rectangular():
    RC.case_vae_roundtrip_hw(DEV, (64, 40))
