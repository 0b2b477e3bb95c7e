"""Stable Diffusion 2.x on MI355X: the attention kernels at head dim 64 and SD-2's head counts (flash -- the <64, W2, QB1> form the
dispatch uses at every lq --, capture, inject, 77-key cross, temporal) against fp32 torch, the reference recordings of the tiny SD-2 nets, a full-width SD-2 UNet
forward against the fp32 restatement (tests/sd2_cases.py, pinned to the recordings on CPU), and a whole SD-2 job."""
import pytest
import torch

from fatezero_amd import kernels as K

import kernel_cases as KC
import pipeline_cases as PC
import sd2_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("frames,heads,lq", [(8, 5, 4096), (16, 5, 4096), (8, 10, 1024), (16, 10, 1024), (16, 20, 256)])
def test_flash_d64_sd2_shapes(frames, heads, lq):
    # 64^2 level: 5 heads x lq 4096, 32^2: 10 heads x lq 1024, 16^2: 20 heads; kv slots [-1, 'first']
    r = KC.case_attn_self(DEV, batch=frames // 8, clip=8, heads=heads, d=64, lq=lq, index_list=[-1, "first"], mode=K.FZ_ATTN_FLASH)
    print("flash d64", frames, heads, lq, r)


def test_flash_d64_ragged_and_slots():
    KC.case_attn_self(DEV, batch=1, clip=3, heads=5, d=64, lq=600, index_list=[-1, "mid", 1], mode=K.FZ_ATTN_FLASH)
    KC.case_attn_self(DEV, batch=1, clip=4, heads=5, d=64, lq=1296, index_list=[-1, "first"], mode=K.FZ_ATTN_FLASH, shape="ramp")


@pytest.mark.parametrize("heads,lq", [(10, 1024), (20, 256), (20, 64)])
def test_capture_and_inject_d64(heads, lq):
    KC.case_attn_self(DEV, batch=2, clip=2, heads=heads, d=64, lq=lq, index_list=[-1, "first"], mode=K.FZ_ATTN_CAPTURE)
    KC.case_attn_self(DEV, batch=2, clip=2, heads=heads, d=64, lq=lq, index_list=[-1, "first"], mode=K.FZ_ATTN_INJECT,
                      mask_kind="random")


@pytest.mark.parametrize("heads,lq,mode", [(5, 4096, K.FZ_ATTN_FLASH), (10, 1024, K.FZ_ATTN_CAPTURE), (20, 256, K.FZ_ATTN_INJECT),
                                           (20, 64, K.FZ_ATTN_CAPTURE)])
def test_cross_d64(heads, lq, mode):
    KC.case_attn_cross(DEV, batch=2, clip=2, heads=heads, d=64, lq=lq, mode=mode)


@pytest.mark.parametrize("heads,tokens,clip", [(5, 4096, 8), (10, 1024, 16), (20, 256, 8)])
def test_temporal_d64(heads, tokens, clip):
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=heads, d=64, tokens=tokens)


@pytest.mark.parametrize("name", ["sd2_unet_d64", "sd2_unet_mixed_upcast"])
def test_sd2_unet_reference_golden_gpu(name):
    r = S.run_sd2_unet_golden(name, DEV)
    print(name, r)
    assert r["err"] <= 1.5e-2 * r["scale"], r


def test_sd2_fullwidth_unet_forward_f8():
    """SD-2-base width (320/640/1280/1280, heads 5/10/20/20 of 64, Linear projections, 1024-wide context), 8 frames of 64^2 latents,
    one forward against the fp32 restatement run by torch on the same GPU."""
    mc = {"lora": 160}
    unet, shapes = S.build_sd2_unet(S.SD2_FULL, mc, DEV)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 4, 8, 64, 64, generator=g)
    ctx = torch.randn(1, 77, 1024, generator=g)
    y = unet(x.to(DEV), 481, ctx.to(DEV)).sample.float()
    from oracle.weights import procedural_state_dict
    ou = S.SD2OracleUNet(procedural_state_dict(shapes), S.SD2_FULL, mc, device=DEV)
    ref = ou(x, 481, ctx)
    err, scale = float((y - ref).abs().max()), float(ref.abs().max())
    print("full-width SD-2 forward", err, scale)
    assert torch.isfinite(y).all()
    assert err <= 1.5e-2 * scale, (err, scale)


def test_sd2_pipeline_reference_golden_gpu():
    """Inversion with capture + 4-step Replace edit with attention blend on the SD-2-shaped net vs the reference recording, and vs the
    fp32 oracle's edit on the natively captured maps: 0 attention-blend mask flips on identical maps, the SD-1 whole-job tolerances."""
    res = S.run_sd2_pipeline_case(DEV)
    print(res)
    PC.check(res)
    assert res["attn_mask_total"] > 0 and res["attn_mask_flips_same_maps"] == 0
