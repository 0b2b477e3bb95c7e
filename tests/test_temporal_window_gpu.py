"""Windowed temporal attention on the MI355X: fz_attn_temporal_win (csrc/attn_temporal.hip: attn_temporal_win_kernel up to 64 frames,
attn_temporal_band_kernel beyond) at the shapes of tests/temporal_window_cases.py, and `model_config.temporal_attention_window` through
a UNet forward against the fp32 oracle with the band mask.  The emulator versions (plus the codes, the issue plans, the whole job, the
gloo job and the config driver) live in tests/test_temporal_window_emu.py."""
import pytest
import torch

from fatezero_amd import _native
from fatezero_amd import kernels as K

import temporal_window_cases as TW

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def hip_backend():
    _native.reset_backend()
    assert "hip" in K.version()
    assert _native.loaded_path().endswith("libfatezero_hip.so")
    yield


@pytest.mark.parametrize("frames,window", TW.THREAD_CASES)
def test_thread_kernels_vs_fp32(frames, window):
    TW.case_window(DEV, batch=2, frames=frames, heads=2, d=40, tokens=5, window=window, seed=frames + window)


@pytest.mark.parametrize("heads,d", TW.BAND_DIMS)
@pytest.mark.parametrize("frames,window", TW.BAND_CASES)
def test_band_kernel_vs_fp32(frames, window, heads, d):
    TW.case_window(DEV, batch=1, frames=frames, heads=heads, d=d, tokens=3, window=window, seed=frames + window + d)


@pytest.mark.parametrize("frames,window", TW.BAND_CASES)
def test_band_kernel_batch2(frames, window):
    TW.case_window(DEV, batch=2, frames=frames, heads=2, d=40, tokens=3, window=window, seed=7)


@pytest.mark.parametrize("frames,window,heads,d", TW.LONG_CASES)
def test_band_kernel_long_clips(frames, window, heads, d):
    TW.case_window(DEV, batch=1, frames=frames, heads=heads, d=d, tokens=2, window=window, seed=frames)


@pytest.mark.parametrize("kv_frames,q_frames,q_frame0,window", TW.SHARD_CASES)
def test_query_frames_of_one_rank_equal_the_whole_clip_rows(kv_frames, q_frames, q_frame0, window):
    TW.case_shard(DEV, kv_frames=kv_frames, q_frames=q_frames, q_frame0=q_frame0, window=window)


@pytest.mark.parametrize("frames", TW.FULL_CASES)
def test_full_window_is_the_unwindowed_launch(frames):
    TW.case_full_window(DEV, frames)


@pytest.mark.parametrize("frames,window", [(8, 1), (100, 9)])
def test_strided_rows_and_untouched_neighbours(frames, window):
    TW.case_strided_out(DEV, frames, window)


def test_unet_forward_12_frames_window_1_vs_band_oracle(monkeypatch):
    TW.case_unet_forward_vs_band_oracle(DEV, monkeypatch, frames=12, window=1)


@pytest.mark.slow
def test_unet_forward_72_frames_window_4_vs_band_oracle(monkeypatch):
    TW.case_unet_forward_vs_band_oracle(DEV, monkeypatch, frames=72, window=4)
