"""Rectangular (widescreen / portrait) clips without a GPU: the blend-mask kernel on res_h x res_w maps (CPU emulation of the kernel
sources), the ABI of the new entry, the edit controller on 40 x 64 and 64 x 40 latents against the fp32 oracle, and the front end
(dataset, YAML, a whole command-line job).  tests/test_rect_gpu.py runs the kernel and controller cases on MI355X."""
import os
import re
import subprocess

import pytest
import torch

from fatezero_amd import _native, build

import rect_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(build.build_emu())
    yield
    _native.reset_backend()


# ---- A. blend mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_hw,out_hw,prompts,or_first", RC.BLEND_CASES, ids=RC.BLEND_IDS)
def test_blend_mask_hw_bit_exact(map_hw, out_hw, prompts, or_first):
    RC.case_blend_mask_hw("cpu", map_hw=map_hw, out_hw=out_hw, prompts=prompts, or_first=or_first, frames=2, heads=2, seed=0,
                          against_oracle=True)


def test_square_entry_is_the_hw_entry_with_equal_sides():
    RC.case_square_entry_equals_hw_entry("cpu")


def test_map_beyond_bm_max_pix_is_a_bad_argument():
    RC.case_oversized_map_is_refused("cpu")


def test_map_hw_must_describe_the_maps():
    maps, alpha = RC.blend_inputs("cpu", 1, 1, 1, 10, 16, 0)
    with pytest.raises(ValueError, match="160 pixels"):
        RC.K.blend_mask(maps, alpha, 0.6, (20, 32), or_with_first=False, map_hw=(16, 16))
    with pytest.raises(AssertionError, match="the shape of attention map must be a square"):   # map_hw=None: today's inference, today's message
        RC.K.blend_mask(maps, alpha, 0.6, (20, 32), or_with_first=False)


def test_level_rule():
    from fatezero_amd.video_diffusion.prompt_attention.attention_store import map_hw
    for extent in ((40, 64), (64, 40), (72, 40), (64, 64), (24, 8)):
        for k in (1, 2, 4, 8):
            lq = (extent[0] // k) * (extent[1] // k)
            assert map_hw(lq, extent) == (extent[0] // k, extent[1] // k) == RC.level_hw(lq, extent)
    assert map_hw(256, None) == (16, 16) and map_hw(160, None) == (12, 12)  # no extent: the reference's int(sqrt(lq)), whatever it yields
    with pytest.raises(ValueError, match=r"lq=150.*\(40, 64\)"):
        map_hw(150, (40, 64))
    with pytest.raises(ValueError, match=r"lq=160.*\(64, 64\)"):
        map_hw(160, (64, 64))


# ---- B. ABI ------------------------------------------------------------------------------------------------------------------------
def test_blend_mask_hw_is_exported_declared_and_documented():
    for lib in (build.build_hip(), build.build_emu()):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert re.search(r"\bT fz_blend_mask_hw\b", out), f"fz_blend_mask_hw is not exported by {lib}"
        assert re.search(r"\bT fz_blend_mask\b", out)
    header = open(os.path.join(ROOT, "include", "fatezero_hip.h")).read()
    m = re.search(r"int fz_blend_mask_hw\((.*?)\);", header, re.S)
    assert m, "include/fatezero_hip.h does not declare fz_blend_mask_hw"
    names = [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert names == ["maps", "n_maps", "n_prompts", "prompt_stride", "frames", "heads", "res_h", "res_w", "p_row_stride", "alpha", "th",
                     "out_h", "out_w", "or_with_first", "out", "scratch", "stream"]
    # the stub of INTEGRATION.md: the argtypes line a binding would copy is the one fatezero_amd/_native.py uses
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    line = re.search(r"^lib\.fz_blend_mask_hw\.argtypes = (\[.*\])$", md, re.M)
    assert line, "INTEGRATION.md carries no fz_blend_mask_hw stub"
    import ctypes
    restype, argtypes = _native._SIGS["fz_blend_mask_hw"]
    assert eval(line.group(1), {"C": ctypes}) == argtypes and restype is ctypes.c_int and len(argtypes) == len(names)
    assert re.search(r"^lib\.fz_blend_mask_hw\.restype = C\.c_int$", md, re.M)


# ---- C. the controller on a rectangular job -------------------------------------------------------------------------------------------
_jobs = {}


def _job(hw, tmp_path_factory):
    if hw not in _jobs:   # one run per geometry, shared by the tests below and left unchanged
        _jobs[hw] = RC.run_rect_job("cpu", kind="tiny16", F_=2, T=6, hw=hw, save_path=str(tmp_path_factory.mktemp("masks%dx%d" % hw)))
    return _jobs[hw]


@pytest.mark.slow   # ~3 minutes of emulation per geometry
@pytest.mark.parametrize("hw", [(40, 64), (64, 40)], ids=["40x64", "64x40"])
def test_edit_controller_on_rectangular_latents(hw, tmp_path_factory):
    """mini_emu's controller setting (tiny16, F = 2, T = 6, Replace, blend words, th [0.3, 0.3], attention blend + latent blend): inversion
    latents and captured maps against the fp32 oracle, masks on identical stored maps bit for bit, the edit against the oracle's edit on the
    natively captured maps, the tensor protocol's row masks equal to the plan path's, the PNG dumps decoding to the h x w masks."""
    RC.check_rect_job(_job(hw, tmp_path_factory))


# ---- E. front end ----------------------------------------------------------------------------------------------------------------------
def _ids():
    return torch.zeros(1, 77, dtype=torch.long)


@pytest.mark.parametrize("frame_hw", [(50, 100), (100, 50)], ids=["50x100", "100x50"])
def test_dataset_rectangular_image_size(frame_hw, tmp_path):
    import dataset_cases as DC
    from fatezero_amd.video_diffusion.data import transform as T
    from fatezero_amd.video_diffusion.data.dataset import ImageSequenceDataset
    folder = str(tmp_path / "frames")
    DC.write_frames(folder, n=3, h=frame_hw[0], w=frame_hw[1])
    ds = ImageSequenceDataset(path=folder, prompt_ids=_ids(), prompt="x", n_sample_frame=2, image_size=[40, 64], offset=dict(
        left=0, right=0, top=0, bottom=0))
    x = ds[0]["images"]
    assert tuple(x.shape) == (3, 2, 40, 64) and float(x.min()) >= -1 and float(x.max()) <= 1
    raw = ds.tensorize_frames([ds.load_frame(i) for i in (0, 1)])
    want = T.center_crop(T.resize_by(raw, max(40 / frame_hw[0], 64 / frame_hw[1])), height=40, width=64)
    assert torch.equal(x, want)
    # the frame covers the target on both sides before the crop, and one side fits exactly
    scaled = T.resize_by(raw, max(40 / frame_hw[0], 64 / frame_hw[1]))
    assert scaled.shape[-2] >= 40 and scaled.shape[-1] >= 64 and (scaled.shape[-2] == 40 or scaled.shape[-1] == 64)
    # an int keeps the square path, bit for bit
    sq = ImageSequenceDataset(path=folder, prompt_ids=_ids(), prompt="x", n_sample_frame=2, image_size=32, offset=dict(
        left=0, right=0, top=0, bottom=0))[0]["images"]
    assert torch.equal(sq, T.center_crop(T.short_size_scale(raw, size=32), height=32, width=32))


def test_dataset_refuses_a_side_the_unet_cannot_take(tmp_path):
    import dataset_cases as DC
    from fatezero_amd.video_diffusion.data.dataset import ImageSequenceDataset
    folder = str(tmp_path / "frames")
    DC.write_frames(folder, n=2, h=50, w=100)
    with pytest.raises(ValueError, match=r"width 60 .*multiple of 8"):
        ImageSequenceDataset(path=folder, prompt_ids=_ids(), prompt="x", n_sample_frame=2, image_size=[40, 60])
    with pytest.raises(ValueError, match=r"height 40 .*multiple of 64"):   # SD-1.x: VAE factor 8 x three UNet downsamplers
        ImageSequenceDataset(path=folder, prompt_ids=_ids(), prompt="x", n_sample_frame=2, image_size=[40, 64], size_multiple=64)
    with pytest.raises(ValueError, match="int or a \\[height, width\\] pair"):
        ImageSequenceDataset(path=folder, prompt_ids=_ids(), prompt="x", n_sample_frame=2, image_size=[40, 64, 3])


def test_config_driver_accepts_the_pair(tmp_path):
    from fatezero_amd import config_driver
    path = tmp_path / "job.yaml"
    path.write_text("dataset_config:\n    path: frames\n    image_size: [320, 512]\nediting_config:\n    size: ${dataset_config.image_size}\n")
    cfg = config_driver.load_config(str(path))
    assert config_driver.image_size_of(cfg["dataset_config"]) == (320, 512)
    assert cfg["editing_config"]["size"] == [320, 512]
    assert config_driver.image_size_of({"image_size": 512}) == 512 and config_driver.image_size_of({}) == 512
    for bad in ([320], [320, 512, 3], "512", [320.5, 512], True):
        with pytest.raises(ValueError, match="image_size"):
            config_driver.image_size_of({"image_size": bad})


def test_command_line_image_size_replaces_the_yaml_value(tmp_path, monkeypatch):
    from fatezero_amd import cli
    os.makedirs(tmp_path / "ckpt" / "unet")
    path = tmp_path / "job.yaml"
    path.write_text(f"pretrained_model_path: {tmp_path / 'ckpt'}\ndataset_config:\n    path: frames\n    image_size: 512\n")
    monkeypatch.setattr(cli, "test", lambda **kw: kw)
    assert cli.run_config_file(str(path), image_size=(320, 512))[0]["dataset_config"]["image_size"] == (320, 512)
    assert cli.run_config_file(str(path))[0]["dataset_config"]["image_size"] == 512
    with pytest.raises(ValueError, match="image_size"):
        cli.run_config_file(str(path), image_size=(320, 512, 3))


def test_pipeline_takes_the_size_from_its_latents():
    """An explicit height / width may repeat the size of the latents handed in; one that contradicts them is an error, raised before any
    launch."""
    import protocol_cases as PRC
    pipe, _, z0, _, emb_tgt = PRC.build("cpu", {"lora": 16}, L=8)
    pipe._encode_prompt = lambda *a, **k: emb_tgt
    z = torch.randn(1, 4, 2, 8, 16)
    with pytest.raises(ValueError, match="`width`=64 contradicts the latents"):
        pipe.sd_ddim_pipeline(prompt=PRC.TGT, latents=z, height=64, width=64, num_inference_steps=1, output_type="latent")
    out = pipe.sd_ddim_pipeline(prompt=PRC.TGT, latents=z, height=64, width=128, num_inference_steps=1, output_type="latent").images
    assert tuple(out.shape) == (1, 4, 2, 8, 16) and bool(torch.isfinite(out.float()).all())


@pytest.mark.slow   # ~2 minutes of emulation
def test_cli_job_on_a_rectangular_clip(tmp_path):
    """test_cli_emu's job with `image_size: [80, 128]` (the tiny VAE halves a side once: 40 x 64 latents): the inverted
    latents, the edited frames and the grids keep the clip's aspect ratio."""
    import dataset_cases as DC
    import test_cli_emu as TC
    import test_fatezero
    from fatezero_amd import config_driver
    from PIL import Image
    ckpt, frames = str(tmp_path / "ckpt"), str(tmp_path / "frames")
    TC.synthetic_checkpoint(ckpt)
    DC.write_frames(frames, n=3, h=90, w=160)
    text = TC.YAML.format(ckpt=ckpt, frames=frames)
    assert "image_size: 32" in text
    cfg_path = str(tmp_path / "config" / "job.yaml")
    os.makedirs(os.path.dirname(cfg_path))
    open(cfg_path, "w").write(text.replace("image_size: 32", "image_size: [80, 128]"))
    cfg = config_driver.load_config(cfg_path)
    out = test_fatezero.test(config=cfg_path, device="cpu", **cfg)
    assert out["latents_all_step"][-1].shape == (1, 4, 2, 40, 64)
    sample = os.path.join(out["logdir"], "sample")
    with Image.open(os.path.join(sample, "step_0_1_0.gif")) as g:
        assert g.size == (128, 80) and getattr(g, "n_frames", 1) == 2      # PIL: (width, height)
    pngs = sorted(os.listdir(os.path.join(sample, "step_0_1_0")))
    assert len(pngs) == 2
    with Image.open(os.path.join(sample, "step_0_1_0", pngs[0])) as im:
        assert im.size == (128, 80)
    with Image.open(os.path.join(out["logdir"], "train_samples.gif")) as g:
        assert g.size[0] * 80 == g.size[1] * 128 or g.size == (128, 80)
    assert len(out["samples"]) == 2
    # a side the models cannot take is refused when the dataset is built (tiny VAE factor 2 x UNet factor 8 = 16)
    open(cfg_path, "w").write(text.replace("image_size: 32", "image_size: [80, 120]"))
    with pytest.raises(ValueError, match=r"width 120 .*multiple of 16"):
        test_fatezero.test(config=cfg_path, device="cpu", **config_driver.load_config(cfg_path))
