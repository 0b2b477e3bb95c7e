"""`recompute_maps` WITHOUT a GPU, on the CPU emulation of the kernels (test infrastructure): the recomputed job against its resident twin bit
for bit, the one-step arena, the early exit of the source forward, fz_latent_tokens, the public switches.  The MI355X versions live in
tests/test_recompute_maps_gpu.py (where every variation is a job of its own: a whole job is milliseconds there and more than half a minute
of emulation here, so this file runs the variations in two combined jobs).

Sizes.  The core job runs on 40^2 latents, 2 frames: a blend mask needs `down_cross[2:4] + up_cross[:3]` to be maps of one level, which
they are only when the first UNet level is above the 32^2-token capture limit -- 16^2 latents raise in SpatialBlender by design -- and 40^2
is the smallest such latent.  The variation jobs need no blend mask and run on 16^2 latents, 2 frames, T = 3 + 3 (an emulated forward costs
~2.5 s whatever its size): edit step 0 reads the maps the inversion left in the slab, steps 1 and 2 each recompute one."""
import os
import sys

import pytest
import torch

from fatezero_amd import _native, build
from fatezero_amd import kernels as K

import recompute_cases as R

DEV = "cpu"
CORE = dict(R.EMU, F=2)
CORE_TH = 0.7  # 43 % of the attention-blend mask elements keep the live attention at this geometry (asserted: 20-80 %)
SMALL = dict(R.EMU, F=2, L=16, T=3)


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(build.build_emu())
    yield
    _native.reset_backend()


# ---------------------------------------------------------------------------------------------------------------
# fz_latent_tokens
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("frames,hw", R.LATENT_TOKEN_SHAPES)
def test_latent_tokens_equals_permute_and_cast(frames, hw, dtype):
    R.check_latent_tokens(DEV, frames, hw, dtype)


def test_latent_tokens_bad_arguments():
    R.check_latent_tokens_bad_args(DEV)


def test_latent_tokens_gives_the_bytes_the_latent_update_hands_on():
    """The recompute pass feeds the UNet fz_latent_tokens(stored latent); the inversion fed it the `next_in` of fz_latent_update (or the
    permute + cast of `_LatentState.sync_tokens` at iteration 0).  Same bytes, for an fp32 and for an fp16 latent store."""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(4, 3, 15, generator=g) * 2
    eps = torch.randn(3, 15, 4, generator=g).half()
    nxt = torch.empty(3, 15, 4, dtype=torch.float16)
    K.latent_update(z, None, eps, 0.0, 1.01, -0.07, next_in=nxt)
    assert torch.equal(K.latent_tokens(z.clone()), nxt)
    assert torch.equal(K.latent_tokens(z.half()), nxt)  # (the pipeline keeps `as_latents(weight_dtype)`: fp16 weights, an fp16 store)


# ---------------------------------------------------------------------------------------------------------------
# the core job: Replace + blend-masked self-attention + latent blend, the edit pass keeping its own self maps
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core():
    kw = dict(blend_th=CORE_TH, save_self_attention=True)
    out = {}
    for mode in (False, True):
        out[mode] = R.run_job(DEV, CORE, recompute=mode, **kw)
    return out


def test_core_job_is_bit_identical_to_the_resident_run(core):
    R.assert_split(core[False])  # the threshold does split the rows of the attention-blend masks
    assert len(core[False]["edits"]["replace"]["applied_masks"]) > 0  # ... and the latent blend was live
    R.assert_same_edit(core[True], core[False])


def test_arena_is_one_step(core):
    R.assert_arena_is_one_step(core[True], core[False], slabs=1)


def test_store_serves_only_the_resident_step(core):
    store = core[True]["pipe"].store_controller
    n = core[True]["steps"]
    assert store.recompute and store.slab_step == 0  # the last edit step read inversion iteration 0
    assert store.maps_of_step(0)["down_cross"]
    with pytest.raises(RuntimeError, match="recompute_maps"):
        store.maps_of_step(n - 1)
    filled = [i for i, d in enumerate(store.attention_store_all_step) if any(len(v) for v in d.values())]
    assert filled == [0] and len(store.attention_store_all_step) == n
    assert store.issue_signature() != core[False]["pipe"].store_controller.issue_signature()
    assert core[True]["pipe"].last_edit_controller.issue_signature() != core[False]["pipe"].last_edit_controller.issue_signature()


# ---------------------------------------------------------------------------------------------------------------
# variations (combined: module docstring)
# ---------------------------------------------------------------------------------------------------------------
VARIATIONS = {
    # Refine + Reweight toward a longer prompt, E5M2 slab, the edit pass keeping no self maps
    "refine_reweight_e5m2_no_self_store": dict(edits=("refine_reweight",), map_dtype="e5m2", save_self_attention=False, blend=False),
    # two editing prompts after one inversion (the second edit recomputes every step), UE4M4 slab, the CFG-shared head off
    "two_prompts_ue4m4_unshared_head": dict(edits=("replace", "refine_reweight"), map_dtype="ue4m4", shared_head=False, blend=False),
}


@pytest.mark.parametrize("name", list(VARIATIONS))
def test_variation_is_bit_identical_to_its_resident_twin(name, tmp_path):
    """... and the inversion-time `show_cross_attention` dump under `save_path` (16^2 latents have the 16 x 16 level it renders; the core
    job's 40^2 have none): the same pictures, from the same running sum of the cross maps."""
    kw = VARIATIONS[name]
    res = R.run_job(DEV, SMALL, recompute=False, save_path=str(tmp_path / "resident"), **kw)
    rec = R.run_job(DEV, SMALL, recompute=True, save_path=str(tmp_path / "recompute"), **kw)
    a, b = R.png_bytes(str(tmp_path / "recompute" / "cross_attention")), R.png_bytes(str(tmp_path / "resident" / "cross_attention"))
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all()
    R.assert_same_edit(rec, res, name)
    R.assert_arena_is_one_step(rec, res)
    fmt = kw["map_dtype"]
    cms = rec["pipe"].store_controller.maps_of_step(0)["down_self"]
    assert cms and all(cm.fmt == fmt and cm.storage.dtype == torch.uint8 for cm in cms)


def test_issue_plans_are_refused_by_name(monkeypatch):
    """The mode does not run under native issue plans (on the MI355X the second of two editing prompts came out different from the walked job
    with plans on; the cause is not found): inversion and edit refuse the combination, naming both switches."""
    pipe = _bare_pipe(recompute_maps=True)
    pipe.scheduler.set_timesteps(2)
    g = torch.Generator().manual_seed(1)
    emb, z = torch.randn(2, 77, 64, generator=g), torch.randn(1, 4, 2, 16, 16, generator=g)
    inv = dict(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True, LOW_RESOURCE=True, latents=z)
    monkeypatch.setenv("FZ_ISSUE_PLANS", "1")
    with pytest.raises(RuntimeError, match="recompute_maps") as e:
        pipe.prepare_latents_ddim_inverted(**inv)
    assert "FZ_ISSUE_PLANS" in str(e.value) and "enable_issue_plans" in str(e.value)
    monkeypatch.delenv("FZ_ISSUE_PLANS")
    lat = pipe.prepare_latents_ddim_inverted(**inv)  # (without plans the same call runs)
    pipe.unet.enable_issue_plans()
    pipe._encode_prompt = lambda *a, **k: emb
    with pytest.raises(RuntimeError, match="issue plans"):
        pipe(prompt="a silver jeep driving down a curvy road in the countryside,", edit_type="swap", latents=lat[-1], num_inference_steps=2,
             source_prompt="a silver jeep driving down a curvy road in the countryside,", cross_replace_steps={"default_": 0.5},
             self_replace_steps=0.5, use_inversion_attention=True, output_type="latent")
    assert pipe.unet._issuer.stats["recorded"] == 0


# ---------------------------------------------------------------------------------------------------------------
# the early exit
# ---------------------------------------------------------------------------------------------------------------
def test_early_exit_captures_the_full_forwards_maps():
    from types import SimpleNamespace
    import pipeline_cases as PC
    from fatezero_amd.video_diffusion.models.resnet import Tokens
    from fatezero_amd.video_diffusion.prompt_attention.attention_register import register_attention_control
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import MAX_CONTROLLED_TOKENS, AttentionStore
    g = torch.Generator().manual_seed(5)
    unet = PC.build_unet("tiny16", {"lora": 16}, DEV)
    ctx = torch.randn(1, 77, 64, generator=g).half()
    launches = {}
    for L, last_level in ((16, 256), (40, 400)):  # every level captured / the first level above the limit: the exit skips its up block
        tok = torch.randn(2, L * L, 4, generator=g).half()
        maps = {}
        for limit in (None, MAX_CONTROLLED_TOKENS):
            store = AttentionStore()
            store.LOW_RESOURCE = True
            register_attention_control(SimpleNamespace(unet=unet), store)
            n0 = K.launch_count()
            y = unet.forward_tokens(Tokens(tok, 1, 2, L, L), 481, ctx, maps_up_to=limit)
            launches[(L, limit)] = K.launch_count() - n0
            store.step_callback(torch.zeros(1))
            maps[limit] = store.maps_of_step(0)
            if limit is not None:
                assert y.data.shape[1] == last_level  # stopped at the last captured level, in front of conv_norm_out / conv_out
        full, early = maps[None], maps[MAX_CONTROLLED_TOKENS]
        n = 0
        for k in full:
            assert len(full[k]) == len(early[k])
            for a, b in zip(full[k], early[k]):
                assert torch.equal(a.storage, b.storage)
                n += 1
        assert n > 0
        assert launches[(L, MAX_CONTROLLED_TOKENS)] < launches[(L, None)]
    # what the exit saves: conv_norm_out + conv_out at 16^2; the upsampler and the whole 1600-token up block as well at 40^2
    assert launches[(40, None)] - launches[(40, MAX_CONTROLLED_TOKENS)] > launches[(16, None)] - launches[(16, MAX_CONTROLLED_TOKENS)]


def test_issue_plan_of_the_early_exit_forward_between_forwards_of_another_context():
    """40^2 latents: the exit skips attention layers, whose context projections are then those of the forward in between (the edit's): the
    early-exit forward is still recorded and replayed, and its maps are the walked forward's."""
    from types import SimpleNamespace
    import pipeline_cases as PC
    from fatezero_amd.video_diffusion.models.resnet import Tokens
    from fatezero_amd.video_diffusion.prompt_attention.attention_register import register_attention_control
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import MAX_CONTROLLED_TOKENS, AttentionStore
    g = torch.Generator().manual_seed(6)
    unet = PC.build_unet("tiny16", {"lora": 16}, DEV)
    unet.enable_issue_plans()
    L = 40
    tok = torch.randn(1, L * L, 4, generator=g).half()
    ctx_src, ctx_edit = torch.randn(1, 77, 64, generator=g).half(), torch.randn(1, 77, 64, generator=g).half()
    maps = []
    for _ in range(3):  # walked, recorded, replayed
        register_attention_control(SimpleNamespace(unet=unet), None)
        unet.forward_tokens(Tokens(tok, 1, 1, L, L), 481, ctx_edit)
        store = AttentionStore()
        store.LOW_RESOURCE = True
        register_attention_control(SimpleNamespace(unet=unet), store)
        unet.forward_tokens(Tokens(tok, 1, 1, L, L), 481, ctx_src, maps_up_to=MAX_CONTROLLED_TOKENS)
        store.step_callback(torch.zeros(1))
        maps.append([cm.storage.clone() for k in sorted(store.maps_of_step(0)) for cm in store.maps_of_step(0)[k]])
    st = unet._issuer.stats
    assert st["unrecordable"] == [] and st["recorded"] == 2 and st["replayed"] == 2, st
    assert len(maps[0]) > 0
    for later in maps[1:]:
        assert len(later) == len(maps[0]) and all(torch.equal(a, b) for a, b in zip(later, maps[0]))


# ---------------------------------------------------------------------------------------------------------------
# switches
# ---------------------------------------------------------------------------------------------------------------
def _bare_pipe(**kw):
    import pipeline_cases as PC
    from helpers import ReplayTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=ReplayTokenizer(), unet=PC.build_unet("tiny16", {"lora": 16}, DEV),
                                         scheduler=DDIMScheduler(), **kw)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def test_without_inversion_attention_the_mode_is_refused_by_name():
    pipe = _bare_pipe(recompute_maps=True)
    z = torch.zeros(1, 4, 2, 16, 16)
    common = dict(prompt="a", source_prompt="a", latents=z, num_inference_steps=2, cross_replace_steps={"default_": 0.5}, self_replace_steps=0.5)
    for edit_type in ("save", "swap"):
        with pytest.raises(ValueError, match="recompute_maps") as e:
            pipe(edit_type=edit_type, use_inversion_attention=False, **common)
        assert "use_inversion_attention" in str(e.value)
    # per call / per p2p_config entry: the key may only repeat the pipeline's mode
    with pytest.raises(ValueError, match="recompute_maps"):
        pipe(edit_type="swap", use_inversion_attention=True, recompute_maps=False, **common)
    with pytest.raises(ValueError, match="recompute_maps"):
        _bare_pipe()(edit_type="swap", use_inversion_attention=True, recompute_maps=True, **common)


def test_pipeline_and_config_switches():
    from fatezero_amd import config_driver as CD
    pipe = _bare_pipe(recompute_maps=True, map_dtype="e5m2", disk_store=True)
    st = pipe.store_controller
    assert pipe.recompute_maps and st.recompute and st.map_dtype == "e5m2"
    assert st.arena.spill is False  # disk_store with recompute_maps spills nothing: there is one step to hold
    pipe.set_map_dtype("ue4m4")
    assert pipe.store_controller.recompute and pipe.store_controller.map_dtype == "ue4m4"
    pipe.set_recompute_maps(False)
    assert not pipe.recompute_maps and not pipe.store_controller.recompute and pipe.store_controller.map_dtype == "ue4m4"
    assert pipe.store_controller.arena.spill is True
    assert pipe.default_recompute_maps is True
    assert CD.recompute_maps_of({"use_inversion_attention": True}) is False
    assert CD.recompute_maps_of({"use_inversion_attention": True, "recompute_attention_maps": True}) is True
    assert CD.recompute_maps_of({"use_inversion_attention": True}, True) is True
    assert CD.recompute_maps_of({"use_inversion_attention": True, "recompute_attention_maps": True}, False) is False
    with pytest.raises(ValueError, match="use_inversion_attention"):
        CD.recompute_maps_of({"recompute_attention_maps": True})
    with pytest.raises(ValueError, match="recompute_attention_maps"):
        CD.recompute_maps_of({"use_inversion_attention": True, "recompute_attention_maps": "yes"})


def test_yaml_key_and_command_line_switch_run_the_job(monkeypatch, tmp_path):
    """`test_fatezero.py --config X [--recompute-maps]` end to end on the synthetic checkpoint of tests/test_cli_emu.py, and the YAML key: the
    same samples as the plain run, from a one-step arena."""
    import numpy as np
    import dataset_cases as DC
    from test_cli_emu import YAML, synthetic_checkpoint
    from fatezero_amd import cli
    ckpt, frames = str(tmp_path / "ckpt"), str(tmp_path / "frames")
    synthetic_checkpoint(ckpt)
    DC.write_frames(frames, n=3, h=40, w=48)
    os.makedirs(tmp_path / "config")
    text = YAML.format(ckpt=ckpt, frames=frames).replace("num_inference_steps: 3", "num_inference_steps: 2")
    assert "use_inversion_attention: true" in text
    plain, keyed = str(tmp_path / "config" / "plain.yaml"), str(tmp_path / "config" / "keyed.yaml")
    open(plain, "w").write(text)
    open(keyed, "w").write(text.replace("editing_config:\n", "editing_config:\n    recompute_attention_maps: true\n", 1))
    seen = []
    real_test, real_inst = cli.test, cli.instantiate_from_config

    def spy_test(*a, **k):
        out = real_test(*a, device="cpu", **k)
        seen[-1]["out"] = out
        return out

    def spy_inst(*a, **k):
        seen.append({"pipe": real_inst(*a, **k)})
        return seen[-1]["pipe"]
    monkeypatch.setattr(cli, "test", spy_test)
    monkeypatch.setattr(cli, "instantiate_from_config", spy_inst)

    def run(argv):
        monkeypatch.setattr(sys, "argv", ["test_fatezero.py"] + argv)
        with pytest.raises(SystemExit) as e:
            cli.run()
        assert e.value.code == 0
        r = seen[-1]
        return r["out"], r["pipe"].store_controller
    out0, st0 = run(["--config", plain])
    out1, st1 = run(["--config", plain, "--recompute-maps"])
    out2, st2 = run(["--config", keyed])
    out3, st3 = run(["--config", keyed, "--no-recompute-maps"])
    assert (st0.recompute, st1.recompute, st2.recompute, st3.recompute) == (False, True, True, False)
    assert st1.arena_bytes == st2.arena_bytes == st0.arena_bytes // 2 and st3.arena_bytes == st0.arena_bytes
    for out in (out1, out2, out3):
        for a, b in zip(out0["latents_all_step"], out["latents_all_step"]):
            assert torch.equal(a, b)
        s0, s1 = out0["samples"], out["samples"]
        assert s0 is not None and len(s0) == len(s1) > 0
        for a, b in zip(s0, s1):  # (one grid image per frame: input | prompt 0 | prompt 1)
            assert np.array_equal(np.asarray(a), np.asarray(b))
