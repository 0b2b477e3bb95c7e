"""Opt-in E5M2 storage of the captured self-attention maps, checked WITHOUT a GPU on the CPU emulation of the kernels (test infrastructure):
the 8-bit capture / inject launches against the fp16 launches bit for bit, the arena and its readers, and the public switches (pipeline
keyword, YAML key, --map-dtype).  The MI355X versions live in tests/test_map8_gpu.py."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from fatezero_amd import _native, build
from fatezero_amd import kernels as K

import map8_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(build.build_emu())
    yield
    _native.reset_backend()


# ---------------------------------------------------------------------------------------------------------------
# 1-3: kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.KERNEL_CASES))
def test_capture8_stores_the_fp16_map_rounded_to_e5m2(name):
    M.check_capture8_bytes(M.kernel_case(name, DEV))


@pytest.mark.parametrize("name", list(M.KERNEL_CASES))
def test_inject8_equals_fp16_inject_of_the_same_values(name):
    M.check_inject8_same_bits(M.kernel_case(name, DEV))


@pytest.mark.parametrize("name", list(M.KERNEL_CASES))
def test_inject8_against_fp32(name):
    M.check_inject8_vs_fp32(M.kernel_case(name, DEV))


def test_wrapper_validates_dtype_and_mode():
    q = torch.zeros(2, 64, 32, dtype=torch.float16)
    vt = torch.zeros(2, 32, 64, dtype=torch.float16)
    kw = dict(clip_len=2, heads=2, index_list=[0])
    with pytest.raises(TypeError, match="uint8"):
        K.attn_self(q, q, vt, torch.empty_like(q), mode=K.FZ_ATTN_CAPTURE8, p=torch.zeros(2, 2, 64, 64, dtype=torch.float16), **kw)
    with pytest.raises(TypeError, match="CAPTURE8"):
        K.attn_self(q, q, vt, torch.empty_like(q), mode=K.FZ_ATTN_CAPTURE, p=torch.zeros(2, 2, 64, 64, dtype=torch.uint8), **kw)
    assert K.self_mode_for(K.FZ_ATTN_INJECT, torch.zeros(1, dtype=torch.uint8)) == K.FZ_ATTN_INJECT8
    assert K.self_mode_for(K.FZ_ATTN_CAPTURE, torch.zeros(1, dtype=torch.float16)) == K.FZ_ATTN_CAPTURE


def test_rounding_helper_is_round_to_nearest_even_on_every_probability_bit_pattern():
    """Every fp16 bit pattern in [0, 1]: the integer arithmetic of the kernel (restated here on the host) equals torch's conversion, and the way
    back is exact."""
    bits = torch.arange(0, 0x3C01, dtype=torch.int32)
    h = bits.to(torch.int16).view(torch.float16)
    want = h.to(torch.float8_e5m2).view(torch.uint8).to(torch.int32)
    got = (bits + 0x7F + ((bits >> 8) & 1)) >> 8
    assert torch.equal(got, want)
    assert torch.equal(K.half_to_e5m2(h).to(torch.int32), want)
    assert torch.equal(K.e5m2_to_half(want.to(torch.uint8)), want.to(torch.uint8).view(torch.float8_e5m2).to(torch.float16))


# ---------------------------------------------------------------------------------------------------------------
# 4: the store
# ---------------------------------------------------------------------------------------------------------------
def _tiny_job(map_dtype=None, disk_store=False, kind="tiny16", frames=4, T=2, L=16, pipe_kw=None, seed=7, edit=True, store_kw=None):
    """A tiny whole job: capture inversion + CFG edit (Replace; the self window is the first half of the T steps).  Returns (pipe, inverted latents, edited)."""
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    unet = PC.build_unet(kind, {"lora": 16}, "cpu")
    kw = dict(pipe_kw or {})
    if map_dtype is not None:
        kw["map_dtype"] = map_dtype
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                         disk_store=disk_store, **kw)
    if store_kw:
        from fatezero_amd.video_diffusion.prompt_attention.attention_store import AttentionStore
        pipe.store_controller = AttentionStore(disk_store=disk_store, **store_kw)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(2, 77, 64, generator=g)
    pipe._encode_prompt = lambda *a, **k: emb
    z0 = torch.randn(1, 4, frames, L, L, generator=g)
    pipe.scheduler.set_timesteps(T)
    lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True,
                                             LOW_RESOURCE=True, latents=z0)
    edited = None
    if edit:
        out = pipe(prompt="a red car", source_prompt="a blue car", edit_type="swap", num_inference_steps=T, latents=lat[-1],
                   output_type="latent", cross_replace_steps={"default_": 0.5}, self_replace_steps=0.5, use_inversion_attention=True,
                   is_replace_controller=True, save_self_attention=False, guidance_scale=3.0, disk_store=disk_store)
        edited = out["sdimage_output"].images
    return pipe, lat, edited


@pytest.fixture(scope="module")
def jobs():
    """The fp16 job and the 8-bit job, run once for the store tests below (tiny16 width, 4 frames, 16^2 latents, T = 2: every self map is a
    whole number of the arena's 256-byte slots in both formats, so "half" is exact)."""
    return {"fp16": _tiny_job(), "e5m2": _tiny_job("e5m2")}


@pytest.fixture(scope="module")
def inversions40():
    """Capture inversions at tiny40 geometry (head dims 40 / 80 / 160; 2 frames, 8^2 latents, T = 4) in both formats."""
    kw = dict(kind="tiny40", frames=2, L=8, T=4, edit=False)
    return {"fp16": _tiny_job(**kw), "e5m2": _tiny_job("e5m2", **kw)}


def _self_cross_bytes(store):
    sb = cb = 0
    for maps in store._all_step_maps:
        for k, lst in maps.items():
            for cm in lst:
                n = (cm.storage.numel() * cm.storage.element_size() + 255) // 256 * 256
                if k.endswith("self"):
                    sb += n
                else:
                    cb += n
    return sb, cb


def test_arena_bytes_is_cross_plus_half_of_self(jobs):
    s16, s8 = jobs["fp16"][0].store_controller, jobs["e5m2"][0].store_controller
    self16, cross16 = _self_cross_bytes(s16)
    assert s16.arena_bytes == self16 + cross16 and self16 > 0 and cross16 > 0
    for maps in s16._all_step_maps:  # (no self map of this job is small enough for the 256-byte slot rounding to matter: halves are exact)
        for cm in maps["down_self"] + maps["mid_self"] + maps["up_self"]:
            assert cm.storage.numel() % 256 == 0
    assert s8.arena_bytes == cross16 + self16 // 2, (s8.arena_bytes, cross16, self16)
    assert s8.map_dtype == "e5m2" and s16.map_dtype == "fp16"


def test_inversion_latents_do_not_depend_on_the_format_and_readers_see_exact_fp16(jobs):
    (p16, lat16, ed16), (p8, lat8, ed8) = jobs["fp16"], jobs["e5m2"]
    for a, b in zip(lat16, lat8):
        assert torch.equal(a, b)  # CAPTURE8's own output is CAPTURE's: the trajectory is the fp16 job's
    s16, s8 = p16.store_controller, p8.store_controller
    n_self = 0
    for step in range(len(s8.attention_store_all_step)):
        maps8, maps16 = s8.maps_of_step(step), s16.maps_of_step(step)
        for k in maps8:
            views = s8.attention_store_all_step[step][k]
            assert len(views) == len(maps8[k]) == len(maps16[k])
            for i, (cm8, cm16) in enumerate(zip(maps8[k], maps16[k])):
                if k.endswith("cross"):
                    assert cm8.storage.dtype == torch.float16 and torch.equal(cm8.storage, cm16.storage)
                    assert torch.equal(views[i], cm16.view)
                    continue
                n_self += 1
                assert cm8.storage.dtype == torch.uint8 and cm8.storage.shape == cm16.storage.shape
                # same inputs, same trajectory: the bytes are the fp16 job's map, rounded
                assert torch.equal(cm8.storage, cm16.storage.to(torch.float8_e5m2).view(torch.uint8)), (step, k, i)
                want = cm8.storage.view(torch.float8_e5m2).to(torch.float16)
                for got in (cm8.view, views[i], list(views)[i]):
                    assert got.dtype == torch.float16 and got.shape == cm16.view.shape and torch.equal(got, want), (step, k, i)
    assert n_self > 0
    assert torch.isfinite(ed8.float()).all()
    # the edit DOES see the rounding (self window [0, 1)): small against the latent scale, not zero
    d = float((ed8.float() - ed16.float()).abs().max())
    assert 0 < d <= 0.05 * float(ed16.float().abs().max()), d


def test_step_maps_are_plain_lists_of_real_tensors(jobs, monkeypatch):
    """What `attention_store_all_step[step][key]` hands out with 8-bit storage is a plain list of real fp16 tensors: torch.cat / torch.stack take
    it, it concatenates and copies like any list -- resident steps and steps that came back from the host tier alike."""
    from fatezero_amd.video_diffusion.prompt_attention import attention_store as AS
    stores = [jobs["e5m2"][0].store_controller]
    monkeypatch.setenv("FZ_ARENA_HBM_GB", "0")
    monkeypatch.setattr(AS, "SPILL_RING", 2)
    stores.append(_tiny_job("e5m2", disk_store=True, frames=2, L=8, edit=False)[0].store_controller)
    assert isinstance(stores[1].attention_store_all_step[-1], AS.HostStepMaps)
    for store in stores:
        for step in (0, len(store.attention_store_all_step) - 1):
            d = store.attention_store_all_step[step]
            cms = store.maps_of_step(step)
            for k, lst in d.items():
                assert type(lst) is list and type(d[k]) is list and type(d.get(k)) is list and len(lst) == len(cms[k])
                assert all(type(t) is torch.Tensor and t.dtype == torch.float16 for t in lst), k
                want = [cm.storage.view(torch.float8_e5m2).to(torch.float16) if cm.is_8bit else cm.view for cm in cms[k]]
                assert all(torch.equal(a, b) for a, b in zip(lst, want))
                if not lst:
                    continue
                both = lst + lst
                assert type(both) is list and len(both) == 2 * len(lst) and all(type(t) is torch.Tensor for t in both)
                cp = lst.copy()
                assert type(cp) is list and all(torch.equal(a, b) for a, b in zip(cp, want))
                by_shape = {}
                for t in lst:
                    by_shape.setdefault(tuple(t.shape[1:]), []).append(t)
                for group in by_shape.values():
                    n = sum(t.shape[0] for t in group)
                    assert torch.cat(group).shape[0] == n and torch.cat(group, dim=0).dtype == torch.float16
                    if len({t.shape for t in group}) == 1:
                        assert torch.stack(group).shape[0] == len(group)
            assert set(d.copy()) == set(d) and all(type(v) is list for v in d.values())


def test_default_store_is_unchanged():
    """The default is fp16 and what it was: the same job through a store built WITHOUT the keyword and through map_dtype="fp16"."""
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import AttentionStore
    assert AttentionStore().map_dtype == "fp16"
    pa, lat_a, _ = _tiny_job(frames=2, L=8, T=2, edit=False)
    pb, lat_b, _ = _tiny_job("fp16", frames=2, L=8, T=2, edit=False)
    assert torch.equal(lat_a[-1], lat_b[-1])
    assert pa.store_controller.arena_bytes == pb.store_controller.arena_bytes
    for da, db in zip(pa.store_controller.attention_store_all_step, pb.store_controller.attention_store_all_step):
        for k in da:
            assert type(da[k]) is list
            for a, b in zip(da[k], db[k]):
                assert a.dtype == torch.float16 and torch.equal(a, b)


def test_unknown_map_dtype_names_the_choices():
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import AttentionStore
    with pytest.raises(ValueError, match=r"'fp16'.*'e5m2'"):
        AttentionStore(map_dtype="e4m3")
    from fatezero_amd import config_driver
    with pytest.raises(ValueError, match=r"'fp16'.*'e5m2'"):
        config_driver.map_dtype_of({"attention_map_dtype": "int8"})
    assert config_driver.map_dtype_of({}) == "fp16" and config_driver.map_dtype_of({"attention_map_dtype": "e5m2"}) == "e5m2"
    assert config_driver.map_dtype_of({"attention_map_dtype": "e5m2"}, "fp16") == "fp16"


def test_spill_tier_moves_the_8bit_slabs_bit_identically(jobs, monkeypatch):
    from fatezero_amd.video_diffusion.prompt_attention import attention_store as AS
    p0, lat0, ed0 = jobs["e5m2"]
    monkeypatch.setenv("FZ_ARENA_HBM_GB", "0")
    monkeypatch.setattr(AS, "SPILL_RING", 2)
    p1, lat1, ed1 = _tiny_job("e5m2", disk_store=True)
    s0, s1 = p0.store_controller, p1.store_controller
    T = len(s1.attention_store_all_step)
    assert sorted(s1.arena.spilled) == list(range(1, T))
    assert s1.arena.spilled_bytes == (T - 1) * s1.arena.step_bytes and s1.arena.step_bytes * T == s0.arena_bytes  # slabs of the 8-bit size
    assert torch.equal(lat1[-1], lat0[-1]) and torch.equal(ed1, ed0)
    for step in range(T):
        st1, st0 = s1.attention_store_all_step[step], s0.attention_store_all_step[step]
        if step > 0:
            assert isinstance(st1, AS.HostStepMaps)
        for k in st0:
            assert len(st1[k]) == len(st0[k])
            for a, b in zip(st1[k], st0[k]):
                assert a.dtype == torch.float16 and torch.equal(a, b), (step, k)
        for k, lst in s1.maps_of_step(step).items():
            for cm1, cm0 in zip(lst, s0.maps_of_step(step)[k]):
                assert cm1.storage.dtype == cm0.storage.dtype and torch.equal(cm1.storage, cm0.storage), (step, k)


def test_reference_protocol_and_running_sum_read_dequantised_maps():
    """The tensor protocol (`controller(attn, is_cross, place)`) quantises on the host the way the kernel does, and accumulate_self sums the
    dequantised values."""
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import AttentionStore
    st = AttentionStore(map_dtype="e5m2", accumulate_self=True)
    st.LOW_RESOURCE = True
    g = torch.Generator().manual_seed(3)
    sums = None
    for step in range(2):
        a_self = torch.rand(2, 2, 64, 128, generator=g).softmax(-1).half()
        a_cross = torch.rand(2, 2, 64, 77, generator=g).softmax(-1).half()
        assert st(a_self, False, "down") is a_self and st(a_cross, True, "down") is a_cross
        deq = a_self.to(torch.float8_e5m2).to(torch.float16)
        assert torch.equal(st.step_store["down_self"][0], deq) and torch.equal(st.step_store["down_cross"][0], a_cross)
        sums = deq.float() if sums is None else sums + deq.float()
        st.step_callback(torch.zeros(1))
    assert torch.equal(st.attention_store["down_self"][0], sums)
    avg = st.get_average_attention()["down_self"][0]
    assert torch.equal(avg, sums / 2)


# ---------------------------------------------------------------------------------------------------------------
# 5: pipeline keyword, YAML key, command line, issue plans, frame sharding
# ---------------------------------------------------------------------------------------------------------------
def test_pipeline_keyword_at_tiny40_geometry(inversions40):
    (p16, lat16, _), (p8, lat8, _) = inversions40["fp16"], inversions40["e5m2"]
    assert len(lat8) == len(lat16) == 5
    for a, b in zip(lat16, lat8):
        assert torch.equal(a, b)
    s16, s8 = p16.store_controller, p8.store_controller
    assert s8.arena_bytes < s16.arena_bytes
    for k in ("down_self", "mid_self", "up_self"):
        for cm8, cm16 in zip(s8.maps_of_step(-1)[k], s16.maps_of_step(-1)[k]):
            assert torch.equal(cm8.storage, cm16.storage.to(torch.float8_e5m2).view(torch.uint8))


def test_yaml_key_selects_the_format(inversions40):
    from fatezero_amd import config_driver
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    p8, lat8, _ = inversions40["e5m2"]
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=p8.unet, scheduler=DDIMScheduler())
    pipe.set_progress_bar_config(disable=True)
    assert pipe.map_dtype == "fp16"
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(2, 77, 64, generator=g)
    pipe._encode_prompt = lambda *a, **k: emb
    z0 = torch.randn(1, 4, 2, 8, 8, generator=g)
    cfg = {"dataset_config": {"prompt": "a blue car"},
           "editing_config": {"use_invertion_latents": True, "use_inversion_attention": True, "num_inference_steps": 4,
                              "attention_map_dtype": "e5m2", "editing_prompts": []}}
    out = config_driver.run_config(pipe, cfg, latents=z0, device="cpu")
    assert pipe.map_dtype == "e5m2" and pipe.store_controller.map_dtype == "e5m2"
    assert torch.equal(out["inverted"][-1], lat8[-1])
    assert pipe.store_controller.arena_bytes == p8.store_controller.arena_bytes
    assert pipe.store_controller.maps_of_step(0)["down_self"][0].storage.dtype == torch.uint8
    # a following config WITHOUT the key runs in the format the pipeline was built with
    del cfg["editing_config"]["attention_map_dtype"]
    cfg["editing_config"]["use_invertion_latents"] = False
    config_driver.run_config(pipe, cfg, latents=z0, device="cpu")
    assert pipe.map_dtype == "fp16" and pipe.store_controller.map_dtype == "fp16"


def test_command_line_switch_and_yaml_key_run_the_job(monkeypatch, tmp_path):
    """`test_fatezero.py --config X [--map-dtype F]` end to end on the synthetic checkpoint of tests/test_cli_emu.py (tokenizer, text encoder,
    VAE, 2-D UNet, PNG frames, YAML): the fp16 job, the job with `--map-dtype e5m2`, and the job whose YAML says
    `attention_map_dtype: e5m2` (that the switch overrides the YAML: test_unknown_map_dtype_names_the_choices).  The 8-bit jobs hold a smaller arena and return the fp16 job's inversion
    latents bit for bit."""
    import dataset_cases as DC
    from test_cli_emu import YAML, synthetic_checkpoint
    from fatezero_amd import cli
    ckpt, frames = str(tmp_path / "ckpt"), str(tmp_path / "frames")
    synthetic_checkpoint(ckpt)
    DC.write_frames(frames, n=3, h=40, w=48)
    os.makedirs(tmp_path / "config")
    text = YAML.format(ckpt=ckpt, frames=frames).replace("num_inference_steps: 3", "num_inference_steps: 2")
    assert "num_inference_steps: 2" in text
    plain, keyed = str(tmp_path / "config" / "plain.yaml"), str(tmp_path / "config" / "keyed.yaml")
    open(plain, "w").write(text)
    open(keyed, "w").write(text.replace("editing_config:\n", "editing_config:\n    attention_map_dtype: e5m2\n", 1))
    assert "attention_map_dtype: e5m2" in open(keyed).read()
    seen = []
    real_test, real_inst = cli.test, cli.instantiate_from_config

    def spy_test(*a, **k):
        out = real_test(*a, device="cpu", **k)
        seen[-1]["out"] = out
        return out

    def spy_inst(*a, **k):
        pipe = real_inst(*a, **k)
        seen.append({"pipe": pipe})
        return pipe
    monkeypatch.setattr(cli, "test", spy_test)
    monkeypatch.setattr(cli, "instantiate_from_config", spy_inst)

    def run(argv):
        monkeypatch.setattr(sys, "argv", ["test_fatezero.py"] + argv)
        with pytest.raises(SystemExit) as e:
            cli.run()
        assert e.value.code == 0
        r = seen[-1]
        store = r["pipe"].store_controller
        return r["out"]["latents_all_step"], store.map_dtype, store.arena_bytes, r["out"]["samples"]
    lat16, fmt16, bytes16, smp16 = run(["--config", plain])
    lat8, fmt8, bytes8, smp8 = run(["--config", plain, "--map-dtype", "e5m2"])
    latk, fmtk, bytesk, _ = run(["--config", keyed])
    assert (fmt16, fmt8, fmtk) == ("fp16", "e5m2", "e5m2")
    assert bytes8 == bytesk < bytes16
    assert len(lat16) == len(lat8) == len(latk) == 3
    for a, b, c in zip(lat16, lat8, latk):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert len(smp8) == len(smp16) == 2
    monkeypatch.setattr(sys, "argv", ["test_fatezero.py", "--config", plain, "--map-dtype", "e4m3"])
    with pytest.raises(SystemExit) as e:  # click refuses a format that does not exist
        cli.run()
    assert e.value.code != 0


def test_switching_the_format_records_a_new_issue_plan():
    """Issue plans on, an fp16 job, an 8-bit job, an fp16 job again on one UNet: each format walks and records its own plan (the launch list
    differs: other kernels, other slab offsets), the third job replays the first job's plan from its first step."""
    from types import SimpleNamespace
    import pipeline_cases as PC
    from fatezero_amd.video_diffusion.prompt_attention.attention_register import register_attention_control
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import AttentionStore
    assert AttentionStore(map_dtype="fp16").issue_signature() != AttentionStore(map_dtype="e5m2").issue_signature()
    g = torch.Generator().manual_seed(4)
    z = torch.randn(1, 4, 2, 8, 8, generator=g).half()
    ctx = torch.randn(1, 77, 64, generator=g).half()

    def run(plans):
        unet = PC.build_unet("tiny16", {"lora": 16}, "cpu")
        if plans:
            unet.enable_issue_plans()
        outs, stats = [], []
        for fmt in ("fp16", "e5m2", "fp16"):
            store = AttentionStore(map_dtype=fmt)
            store.LOW_RESOURCE = True
            register_attention_control(SimpleNamespace(unet=unet), store)
            x = z
            for i in range(3):
                x = unet(x, 900 - 200 * i, ctx).sample
                store.step_callback(x)
                outs.append(x.clone())
            assert store.maps_of_step(0)["mid_self"][0].storage.dtype == (torch.uint8 if fmt == "e5m2" else torch.float16)
            stats.append(dict(unet._issuer.stats) if plans else None)
        return outs, stats
    outs0, _ = run(False)
    outs1, stats = run(True)
    assert all(torch.equal(a, b) for a, b in zip(outs0, outs1))
    assert all(torch.equal(a, b) for a, b in zip(outs0[:3], outs0[3:6]))  # the forward does not depend on the storage format
    a, b, c = stats
    assert (a["walked"], a["recorded"], a["replayed"]) == (1, 1, 1), a
    assert (b["walked"], b["recorded"], b["replayed"]) == (2, 2, 2), b     # the other format: a new walk, a new plan
    assert (c["walked"], c["recorded"], c["replayed"]) == (2, 2, 5), c     # back to the first: its plan is still there


# -- frame sharding: a per-rank 8-bit arena, nothing exchanged for it --------------------------------------------------
def _shard_job(frames):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fatezero_amd import _native as N, build as B
    N.use_test_backend(B.build_emu())
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    unet = PC.build_unet("tiny16", {"lora": 16, "SparseCausalAttention_index": [-1, "first"]}, "cpu")
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                         map_dtype="e5m2")
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(2, 77, 64, generator=g)
    pipe._encode_prompt = lambda *a, **k: emb
    z0 = torch.randn(1, 4, frames, 8, 8, generator=g)

    def job():
        pipe.scheduler.set_timesteps(2)
        lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb,
                                                 store_attention=True, LOW_RESOURCE=True, latents=z0)
        out = pipe(prompt="a red car", source_prompt="a blue car", edit_type="swap", num_inference_steps=2, latents=lat[-1],
                   output_type="latent", cross_replace_steps={"default_": 0.5}, self_replace_steps=0.5, use_inversion_attention=True,
                   is_replace_controller=True, save_self_attention=False, guidance_scale=3.0)
        return torch.stack([lat[-1], out["sdimage_output"].images])
    return pipe, job


def _shard_worker(rank, world, port, frames, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      FZ_EMU_THREADS="2")
    torch.set_num_threads(2)
    sys.path.insert(0, ROOT)
    from fatezero_amd import dist as D
    import torch.distributed as dist
    D.init("gloo")
    shard = D.FrameShard(frames)
    pipe, job = _shard_job(frames)
    pipe.frame_shard = shard
    res = job()
    store = pipe.store_controller
    cms = store.maps_of_step(0)["down_self"]
    if rank == 0:
        q.put((res.clone(), [cm.storage.shape[0] for cm in cms], [str(cm.storage.dtype) for cm in cms], shard.n_local))
    dist.barrier()
    dist.destroy_process_group()


def test_frame_sharded_8bit_job_matches_single_process():
    frames, world = 4, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, frames, q)) for r in range(world)]
    for p in procs:
        p.start()
    got, n_maps, dtypes, n_local = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    for k in ("WORLD_SIZE", "RANK"):
        os.environ.pop(k, None)
    _, job = _shard_job(frames)
    ref = job()
    assert n_maps and all(n == n_local for n in n_maps) and all(d == "torch.uint8" for d in dtypes), (n_maps, dtypes, n_local)
    err, scale = float((got.float() - ref.float()).abs().max()), float(ref.float().abs().max())
    assert torch.isfinite(got.float()).all()
    assert err <= 1.5e-2 * scale, (err, scale)  # the tolerance of the fp16 sharded job (tests/test_dist_gloo.py)
