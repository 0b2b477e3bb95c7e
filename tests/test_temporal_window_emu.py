"""Windowed temporal attention WITHOUT a GPU: fz_attn_temporal_win (csrc/attn_temporal.hip: attn_temporal_win_kernel up to 64 frames,
attn_temporal_band_kernel beyond) on the CPU emulation of csrc/fz_rt.h, its codes, and `model_config.temporal_attention_window` through
the model, the issue plans, a whole job, a 2-rank gloo job and the config driver.  Cases: tests/temporal_window_cases.py; the MI355X
versions live in tests/test_temporal_window_gpu.py."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from fatezero_amd import _native, build
from fatezero_amd import kernels as K

import temporal_window_cases as TW

DEV = "cpu"
MAXW = K.TEMPORAL_MAX_WINDOW


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(os.environ.get("FZ_EMU_LIB") or build.build_emu())
    yield
    _native.reset_backend()


def test_limit_in_header_and_python():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "fatezero_hip.h")).read()
    assert int(re.search(r"#define FZ_TEMPORAL_MAX_WINDOW (\d+)", hdr).group(1)) == MAXW >= 64
    assert (32 + 2 * MAXW + 31) // 32 + 1 <= 8  # key tiles of a 32-query tile: the long kernel's register file of scores


# ---- 1. thread kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,window", TW.THREAD_CASES)
def test_thread_kernels_vs_fp32(frames, window):
    TW.case_window(DEV, batch=2, frames=frames, heads=2, d=40, tokens=5, window=window, seed=frames + window)


# ---- 2. band kernel at its first length -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,d", TW.BAND_DIMS)
@pytest.mark.parametrize("frames,window", TW.BAND_CASES)
def test_band_kernel_vs_fp32(frames, window, heads, d):
    TW.case_window(DEV, batch=1, frames=frames, heads=heads, d=d, tokens=3, window=window, seed=frames + window + d)


@pytest.mark.parametrize("frames,window", TW.BAND_CASES)
def test_band_kernel_batch2(frames, window):
    TW.case_window(DEV, batch=2, frames=frames, heads=2, d=40, tokens=3, window=window, seed=7)


# ---- 3. past the long kernel's 256 frames and at the limit ------------------------------------------------------------------------
@pytest.mark.parametrize("frames,window,heads,d", TW.LONG_CASES)
def test_band_kernel_long_clips(frames, window, heads, d):
    TW.case_window(DEV, batch=1, frames=frames, heads=heads, d=d, tokens=2, window=window, seed=frames)


# ---- 4. frame-sharded form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_frames,q_frames,q_frame0,window", TW.SHARD_CASES)
def test_query_frames_of_one_rank_equal_the_whole_clip_rows(kv_frames, q_frames, q_frame0, window):
    TW.case_shard(DEV, kv_frames=kv_frames, q_frames=q_frames, q_frame0=q_frame0, window=window)


# ---- 5. a window that covers the clip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", TW.FULL_CASES)
def test_full_window_is_the_unwindowed_launch(frames):
    TW.case_full_window(DEV, frames)


# ---- 6. strided output ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,window", [(8, 1), (100, 9)])
def test_strided_rows_and_untouched_neighbours(frames, window):
    TW.case_strided_out(DEV, frames, window)


# ---- 7. codes ---------------------------------------------------------------------------------------------------------------------
def _win_rc(fq, fk, q0, w, heads=1, d=16, tokens=1):
    q = torch.zeros(max(fq, 1), tokens, heads * d, dtype=torch.float16)
    kv = torch.zeros(max(fk, 1), tokens, heads * d, dtype=torch.float16)
    out = torch.zeros_like(q)
    P = lambda t: C.c_void_p(t.data_ptr())
    return _native.lib().fz_attn_temporal_win(P(q), P(kv), P(kv), P(out), 1, fq, fk, q0, w, tokens, heads, d, heads * d, heads * d,
                                              heads * d, 0.25, C.c_void_p(0))


def test_codes_of_the_c_entry_point():
    assert _win_rc(8, 8, 0, 1) == 0
    assert _win_rc(8, 8, 0, -1) == -1                  # negative window
    assert _win_rc(4, 8, 5, 1) == -1                   # q_frame0 + q_frames > kv_frames
    assert _win_rc(4, 8, -1, 1) == -1
    assert _win_rc(300, 300, 0, MAXW + 1) == -2        # FZ_ERR_UNSUPPORTED: above the limit and not covering the clip
    assert _win_rc(300, 300, 0, MAXW) == 0
    assert _win_rc(300, 300, 0, 299) == 0              # covers the clip: the unwindowed launch
    assert _win_rc(40, 40, 0, 38) == 0                 # up to 64 frames every window is served
    f = K.TEMPORAL_MAX_FRAMES + 1
    assert _win_rc(f, f, 0, 4) == -1                   # clip above FZ_TEMPORAL_MAX_FRAMES
    assert _win_rc(8, f, 0, 4) == -1


def test_errors_of_the_python_wrapper():
    def call(fq, fk, **kw):
        q = torch.zeros(fq, 1, 16, dtype=torch.float16)
        kv = torch.zeros(fk, 1, 16, dtype=torch.float16)
        K.attn_temporal(q, kv, kv, torch.zeros_like(q), batch=1, clip_len=fq, kv_frames=fk, heads=1, **kw)
    call(8, 8, window=1)
    for bad in (-1, 1.0, "2", True):
        with pytest.raises(ValueError, match="window"):
            call(8, 8, window=bad)
    with pytest.raises(ValueError, match="q_frame0"):
        call(4, 8, window=1, q_frame0=5)
    with pytest.raises(ValueError, match="FZ_TEMPORAL_MAX_WINDOW"):
        call(300, 300, window=MAXW + 1)
    call(300, 300, window=299)
    f = K.TEMPORAL_MAX_FRAMES + 1
    with pytest.raises(ValueError, match=str(K.TEMPORAL_MAX_FRAMES)):
        call(f, f, window=4)


# ---- 8. / 9. one UNet forward against the fp32 oracle with the band mask ----------------------------------------------------------
@pytest.mark.parametrize("window", [1, 2])
def test_unet_forward_12_frames_vs_band_oracle(window, monkeypatch):
    TW.case_unet_forward_vs_band_oracle(DEV, monkeypatch, frames=12, window=window)


@pytest.mark.slow
def test_unet_forward_72_frames_window_4_vs_band_oracle(monkeypatch):
    # the band kernel in all 16 blocks; the unwindowed sibling: tests/test_long_clip_emu.py::test_unet_forward_72_frames_vs_oracle
    TW.case_unet_forward_vs_band_oracle(DEV, monkeypatch, frames=72, window=4)


# ---- 10. absent, None and F - 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_absent_none_and_full_window_give_equal_outputs():
    TW.case_absent_none_and_full_window_are_equal(DEV, frames=4)  # (four forwards on the emulator: the shortest clip a window of 1 bites)


def test_a_bad_window_fails_where_the_model_is_built():
    import pipeline_cases as PC
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError, match="temporal_attention_window"):
            UNetPseudo3DConditionModel(sample_size=64, **PC.TINY["tiny16"], lora=16, temporal_attention_window=bad)


# ---- 11. a tiny whole job ----------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_tiny_whole_job_recomputed_equals_resident_and_differs_from_unwindowed():
    TW.case_tiny_whole_job(DEV, frames=6, steps=4, window=1)


# ---- 12. issue plans --------------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_issue_plans_carry_the_window():
    import pipeline_cases as PC
    from fatezero_amd.video_diffusion.models.attention import SpatioTemporalTransformerBlock
    g = torch.Generator().manual_seed(1)
    z = torch.randn(1, 4, 4, 8, 8, generator=g).half()
    ctx = torch.randn(1, 77, 64, generator=g).half()

    def walked(window):
        return PC.build_unet("tiny16", {"lora": 16, "temporal_attention_window": window}, DEV)(z, 5, ctx).sample
    unet = PC.build_unet("tiny16", {"lora": 16, "temporal_attention_window": 1}, DEV)
    unet.enable_issue_plans()
    ys1 = [unet(z, 5, ctx).sample.clone() for _ in range(3)]  # walked, recorded, replayed
    st1 = dict(unet._issuer.stats)
    assert st1["recorded"] == 1 and st1["replayed"] == 1 and not st1["unrecordable"] and not st1["unsupported"], st1
    assert torch.equal(ys1[2], walked(1))  # a windowed model's replayed forward equals its walked one
    # the same model with another window: the plan of window 1 must not be replayed
    for m in unet.modules():
        if isinstance(m, SpatioTemporalTransformerBlock):
            m.model_config["temporal_attention_window"] = 2
    ys2 = [unet(z, 5, ctx).sample.clone() for _ in range(3)]
    st2 = dict(unet._issuer.stats)
    assert st2["recorded"] == 2 and st2["replayed"] == 2 and st2["walked"] == st1["walked"] + 1, (st1, st2)
    w2 = walked(2)
    assert all(torch.equal(y, w2) for y in ys2) and not torch.equal(ys1[2], w2)


# ---- 13. two gloo ranks -----------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_frame_sharded_windowed_job_on_two_gloo_ranks():
    """8 frames over 2 ranks, W = 1: every rank attends the band around its own frames in the all-gathered K | V (q_frame0 = the
    start of its frames).  Equal to the single-process job within the tolerance of the sharded jobs (1.5e-2 of the range, that of
    tests/test_recompute_maps_gloo.py and tests/test_dist_gloo.py: the sharded GroupNorm merges chunk partials) -- and the window moves
    the single-process job by far more than that, so a sharded branch that ignored the window (or took q_frame0 = 0 on rank 1) fails."""
    import torch.multiprocessing as mp
    frames, world, window = 8, 2, 1
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = 39500 + (os.getpid() % 2000)
    procs = [mctx.Process(target=TW.gloo_worker, args=(r, world, port, frames, window, q)) for r in range(world)]
    for p in procs:
        p.start()
    sharded = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    single = TW.tiny_job(DEV, frames=frames, steps=3, window=window)
    plain = TW.tiny_job(DEV, frames=frames, steps=3, window=None)
    scale = float(single.abs().max())
    err, moved = float((sharded - single).abs().max()), float((single - plain).abs().max())
    print({"err": err, "moved": moved, "scale": scale})
    assert torch.isfinite(sharded).all() and moved > 3 * 1.5e-2 * scale, (moved, scale)
    assert err <= 1.5e-2 * scale, (err, scale)


# ---- 14. config -------------------------------------------------------------------------------------------------------------------
def _config_folder(tmp_path, model_config_yaml):
    import json
    from test_checkpoint_io import CFG_2D
    os.makedirs(tmp_path / "ckpt" / "unet")
    json.dump(CFG_2D, open(tmp_path / "ckpt" / "unet" / "config.json", "w"))
    path = tmp_path / "job.yaml"
    path.write_text(f"pretrained_model_path: {tmp_path / 'ckpt'}\ndataset_config:\n    path: frames\nediting_config:\n"
                    f"    num_inference_steps: 2\nmodel_config:\n    lora: 16\n{model_config_yaml}")
    return str(path)


def test_yaml_key_reaches_every_block_and_the_switch_overrides_it(tmp_path, monkeypatch):
    from fatezero_amd import cli, config_driver
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    from fatezero_amd.video_diffusion.models.attention import SpatioTemporalTransformerBlock
    path = _config_folder(tmp_path, "    temporal_attention_window: 3\n")
    seen = []
    monkeypatch.setattr(cli, "test", lambda **kw: seen.append(kw) or kw)
    cli.run_config_file(path)
    assert seen[-1]["model_config"]["temporal_attention_window"] == 3
    unet = UNetPseudo3DConditionModel.from_2d_model(os.path.join(seen[-1]["pretrained_model_path"], "unet"), seen[-1]["model_config"])
    blocks = [m for m in unet.modules() if isinstance(m, SpatioTemporalTransformerBlock)]
    assert len(blocks) >= 4 and all(b.temporal_window == 3 for b in blocks)

    def run(argv):
        monkeypatch.setattr(sys, "argv", ["test_fatezero.py"] + argv)
        with pytest.raises(SystemExit) as e:
            cli.run()
        assert e.value.code == 0
        return seen[-1]["model_config"]
    assert run(["--config", path])["temporal_attention_window"] == 3
    assert run(["--config", path, "--temporal-window", "5"]) == {"lora": 16, "temporal_attention_window": 5}
    assert run(["--config", path, "--temporal-window", "0"])["temporal_attention_window"] == 0
    with pytest.raises(ValueError, match="temporal_attention_window"):
        cli.run_config_file(path, temporal_window=-1)
    assert config_driver.temporal_window_of({}) is None and config_driver.temporal_window_of({"temporal_attention_window": None}) is None
    assert config_driver.temporal_window_of({"temporal_attention_window": 4}) == 4
    assert config_driver.temporal_window_of({"temporal_attention_window": 4}, 7) == 7


@pytest.mark.parametrize("bad", ["-2", "1.5", "'4'", "true"])
def test_a_bad_yaml_value_raises_before_any_checkpoint_file_is_opened(bad, tmp_path, monkeypatch):
    from fatezero_amd import cli, config_driver
    path = _config_folder(tmp_path, f"    temporal_attention_window: {bad}\n")

    class Opened:
        @staticmethod
        def from_pretrained(*a, **k):
            raise AssertionError("a checkpoint file was opened before the window was checked")
    for name in ("CLIPTokenizer", "CLIPTextModel", "AutoencoderKL", "UNetPseudo3DConditionModel"):
        monkeypatch.setattr(cli, name, Opened)
    cfg = config_driver.load_config(path)
    with pytest.raises(ValueError, match="temporal_attention_window"):
        cli.test(config=path, logdir=str(tmp_path / "result"), **cfg)
