"""The CFG-shared head on the CPU emulation backend: the broadcast forms of the kernels at its divergence point (FzXattnChain.in_frames,
FzGemmDesc.res_rows, fz_groupnorm_cat's x2_frames) against the expanded operands, the tiny UNets with the shared input against the expanded one
(the fallback path: the chain launch is not preferred at these sizes, the shared tensors are expanded by fz_repeat), and a Replace job whose
windows open and close with the switch on against off, walked and under the native issue plans."""
import pytest
import torch

from fatezero_amd import _native, build

import cfg_shared_cases as CS
import pipeline_cases as PC


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(build.build_emu())
    yield
    _native.reset_backend()


@pytest.mark.parametrize("front", [False, True])
@pytest.mark.parametrize("tokens", [128, 256])
@pytest.mark.parametrize("frames", [(2, 1, 1), (4, 2, 2)])
def test_xattn_chain_reads_shared_input_frames(frames, tokens, front):
    out_frames, in_frames, clip = frames
    print(CS.case_xattn_in_frames("cpu", tokens=tokens, out_frames=out_frames, in_frames=in_frames, clip=clip, front=front, seed=tokens + out_frames))


def test_gemm_residual_broadcast():
    """rows 512, res_rows 256, K 320, N 320 through the three entry points (the whole-row tile pinned where the library would pick a
    narrower one at so few rows: the LayerNorm / GroupNorm-statistics epilogues must run), and the split-K tail at K 1280."""
    assert CS.case_gemm_res_rows("cpu", entry="gemm") == [True]
    assert CS.case_gemm_res_rows("cpu", entry="lnout", tile_cfg=254122, seed=1) == [True, True]
    assert CS.case_gemm_res_rows("cpu", entry="gn", tile_cfg=254122, seed=2) == [True, True]
    assert CS.case_gemm_res_rows("cpu", entry="gemm", k=1280, split_k=2, seed=3) == [True]
    assert CS.case_gemm_res_rows("cpu", entry="lnout", k=1280, split_k=2, seed=4) == [True, False]   # (split-K: no LayerNorm from it, y complete)
    assert CS.case_gemm_res_rows("cpu", entry="gn", seed=5)[0]                                        # the library's own tile choice


def test_groupnorm_cat_second_source_broadcast():
    print(CS.case_groupnorm_cat_x2_frames("cpu"))                                   # three-kernel form or the one-launch form, as the library picks
    print(CS.case_groupnorm_cat_x2_frames("cpu", n=4, n2=2, span=1, tokens=16, c1=32, c2=32, groups=8, seed=1))   # the one-launch form
    print(CS.case_groupnorm_cat_x2_frames("cpu", n=4, n2=2, span=2, tokens=640, c1=320, c2=320, seed=2))          # several chunks per frame


def test_repeat_frames():
    from fatezero_amd import kernels as K
    x = torch.randn(3, 5, 8).half()
    assert torch.equal(K.repeat_frames(x, 2), torch.cat([x, x], 0))


@pytest.mark.parametrize("kind,mc", [("tiny16", {"lora": 16}), ("tiny40", {"lora": 16, "SparseCausalAttention_index": ["mid"]})])
def test_model_shared_input_equals_expanded_input(kind, mc):
    """2 frames, 16 x 16 latents, one CFG forward: rep = 2 against the expanded rep = 1 input.  No controller: attn1 stays shared, attn2 ends
    the head through the fallback (two fz_repeat launches).  The emulator runs the same tiles for 2 and 4 frames here: bit-equal."""
    unet = PC.build_unet(kind, mc, "cpu")
    y_rep, y_exp = CS.cfg_forward_pair(unet, "cpu", frames=2, latent=16, ctx_dim=64)
    d = float((y_rep.float() - y_exp.float()).abs().max())
    print(kind, "max |shared - expanded|", d, "scale", float(y_exp.float().abs().max()))
    assert torch.equal(y_rep, y_exp)
    y_off, _ = CS.with_switch(False, lambda: CS.cfg_forward_pair(unet, "cpu", frames=2, latent=16, ctx_dim=64))
    assert torch.equal(y_off, y_exp)   # switch off: the shared input is expanded on entry


def test_a_caller_with_two_different_halves_is_never_deduplicated():
    unet = PC.build_unet("tiny16", {"lora": 16}, "cpu")
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 4, 2, 16, 16, generator=g).half()
    ctx = torch.randn(1, 77, 64, generator=g).half().expand(2, -1, -1).contiguous()
    y = unet(z, 481, ctx).sample
    ya = unet(z[:1], 481, ctx[:1]).sample
    yb = unet(z[1:], 481, ctx[1:]).sample
    assert not torch.equal(y[0], y[1])
    assert float((y[0] - ya[0]).abs().max()) <= 1.5e-2 * float(ya.abs().max()) and float((y[1] - yb[0]).abs().max()) <= 1.5e-2 * float(yb.abs().max())


def test_replace_job_switch_on_equals_off():
    """Two-prompt Replace job (4 frames, 16 x 16 latents, T = 4: the cross- and self-replace windows are open for steps 0-1, closed for 2-3).
    The first level has 16 x 16 queries, inside the controllers' 32 x 32 limit: the head must stop in front of attn1 (the cond half is
    injected while the window is open) and the controller must count the same calls."""
    r = CS.pipeline_on_off("pipe_f4_prev_first", "cpu")
    print(r)
    assert r["edit_equal"] and r["map_max_diff"] == 0.0 and r.get("attn_mask_flips", 0) == 0, r


def test_replace_job_under_issue_plans_equals_eager(monkeypatch):
    r = CS.pipeline_on_off("pipe_f4_prev_first", "cpu", issue_plans=True, monkeypatch=monkeypatch)
    print(r)
    st = r["stats"]
    assert st["replayed"] >= 1 and not st["unrecordable"] and not st["unsupported"], st
    assert r["edit_equal"] and r["map_max_diff"] == 0.0, r
