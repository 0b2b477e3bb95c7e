"""The CFG-shared head on the MI355X: the broadcast forms of the kernels at its divergence point against the expanded operands (bit for bit),
the UNet with the shared input against the expanded one on the fallback path (tiny widths) and on the chain path (full SD-1.x width, 6 frames:
fz_xattn_chain_preferred holds), and Replace jobs with the switch on against off, walked and under issue plans.
Measured figures: profiles/r07_cfg_shared_head_parity.txt."""
import pytest
import torch

from fatezero_amd import _native

import cfg_shared_cases as CS
import pipeline_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("front", [False, True])
@pytest.mark.parametrize("tokens", [128, 256])
@pytest.mark.parametrize("frames", [(2, 1, 1), (4, 2, 2)])
def test_xattn_chain_reads_shared_input_frames(frames, tokens, front):
    out_frames, in_frames, clip = frames
    print(CS.case_xattn_in_frames(DEV, tokens=tokens, out_frames=out_frames, in_frames=in_frames, clip=clip, front=front, seed=tokens + out_frames))


def test_gemm_residual_broadcast():
    assert CS.case_gemm_res_rows(DEV, entry="gemm") == [True]
    assert CS.case_gemm_res_rows(DEV, entry="lnout", tile_cfg=254122, seed=1) == [True, True]
    assert CS.case_gemm_res_rows(DEV, entry="gn", tile_cfg=254122, seed=2) == [True, True]
    assert CS.case_gemm_res_rows(DEV, entry="gemm", k=1280, split_k=2, seed=3) == [True]
    assert CS.case_gemm_res_rows(DEV, entry="lnout", k=1280, split_k=2, seed=4) == [True, False]
    assert CS.case_gemm_res_rows(DEV, entry="gn", seed=5)[0]
    # the judged proj_out launch: 16 x 4096 rows, the residual shared by the halves -- the library's own tile, statistics from its epilogue
    assert CS.case_gemm_res_rows(DEV, entry="gn", rows=16 * 4096, res_rows=8 * 4096, seed=6) == [True, True]


def test_groupnorm_cat_second_source_broadcast():
    print(CS.case_groupnorm_cat_x2_frames(DEV))
    print(CS.case_groupnorm_cat_x2_frames(DEV, n=4, n2=2, span=1, tokens=16, c1=32, c2=32, groups=8, seed=1))
    print(CS.case_groupnorm_cat_x2_frames(DEV, n=4, n2=2, span=2, tokens=640, c1=320, c2=320, seed=2))
    print(CS.case_groupnorm_cat_x2_frames(DEV, n=16, n2=8, span=8, tokens=4096, c1=320, c2=320, seed=3))   # the judged launch (last up resnet)


@pytest.mark.parametrize("kind,mc", [("tiny16", {"lora": 16}), ("tiny40", {"lora": 16, "SparseCausalAttention_index": ["mid"]})])
def test_model_fallback_path(kind, mc):
    unet = PC.build_unet(kind, mc, DEV)
    y_rep, y_exp = CS.cfg_forward_pair(unet, DEV, frames=2, latent=16, ctx_dim=64)
    print("fallback", kind, CS.check_on_off(y_rep, y_exp))


def test_model_chain_path_full_width():
    """Full SD-1.x width, 6 frames, 64 x 64 latents, one CFG forward: 6 x 4096 rows per half, a clip at which the chain launch is preferred
    -- attn2 of the first block reads the shared norm2 output / hidden states through FzXattnChain.in_frames, proj_out and the last
    up resnet read the shared residual / skip; no copy launch."""
    from fatezero_amd import kernels as K
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    from oracle.weights import procedural_state_dict
    assert K.xattn_chain_preferred(2 * 6 * 4096, 4096, 320, 8, 77)
    unet = UNetPseudo3DConditionModel(sample_size=64, **PC.SD15, lora=160)
    unet.load_state_dict(procedural_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()]))
    unet = unet.half().to(DEV).eval()
    copies = []
    orig = K.repeat_frames
    K.repeat_frames = lambda *a, **k: (copies.append(1), orig(*a, **k))[1]
    try:
        n0 = K.launch_count()
        y_rep, y_exp = CS.cfg_forward_pair(unet, DEV, frames=6, latent=64, ctx_dim=768)
    finally:
        K.repeat_frames = orig
    assert not copies, "the chain path must take no expanding copy"
    print("chain path, launches of the two forwards:", K.launch_count() - n0, CS.check_on_off(y_rep, y_exp))
    assert _native.loaded_path().endswith("libfatezero_hip.so")


def test_replace_job_switch_on_vs_off():
    """pipe_small_replace: two prompts, Replace, 32 x 32 latents, T = 4 -- both replace windows open for steps 0-1 and closed for 2-3; the first
    level has 32 x 32 queries, so the head stops in front of attn1 (the cond half is injected while the window is open).  Same stored maps,
    edited latents within the on / off bound."""
    r = CS.pipeline_on_off("pipe_small_replace", DEV)
    print("pipe_small_replace", r)
    sc = r["edit_scale"]
    assert r["edit_max_diff"] <= CS.ON_OFF_MAX_TOL * sc and r["edit_q99_diff"] <= CS.ON_OFF_Q99_TOL * sc, r
    assert r["map_max_diff"] == 0.0 and r.get("attn_mask_flips", 0) == 0, r


def test_blend_masked_job_switch_on_vs_off():
    """pipe_replace_blend: 64 x 64 latents with blend-masked self-attention, 2 frames -- attn1 of the first level stays shared and attn2 ends the
    head through the fallback copies.  The 2- and 4-frame launches of the 64 x 64-level convolutions take different tiles, so the two runs are
    two fp16 evaluations of the same 4-step CFG job: the edited latents are held to the bands pipeline_cases states for such a job against its
    recording (EDIT_Q99_TOL / EDIT_MAX_TOL); the blend masks (thresholded from the STORED maps) must not move at all and the inversion's maps
    are the same tensors.  The edit pass's own accumulated cross maps follow the latents and are printed, not bounded."""
    r = CS.pipeline_on_off("pipe_replace_blend", DEV)
    print("pipe_replace_blend", r)
    sc = r["edit_scale"]
    assert r["edit_max_diff"] <= PC.EDIT_MAX_TOL * sc and r["edit_q99_diff"] <= PC.EDIT_Q99_TOL * sc, r
    d = r["map_diffs"]
    assert d.get("inv_cross", 0.0) == 0.0 and d.get("inv_self", 0.0) == 0.0, r
    assert r["attn_mask_flips"] == 0 and r["attn_mask_total"] > 0, r


def test_replace_job_under_issue_plans_equals_eager(monkeypatch):
    r = CS.pipeline_on_off("pipe_small_replace", DEV, issue_plans=True, monkeypatch=monkeypatch)
    print(r)
    st = r["stats"]
    assert st["replayed"] >= 1 and not st["unrecordable"] and not st["unsupported"], st
    assert r["edit_equal"] and r["map_max_diff"] == 0.0, r
