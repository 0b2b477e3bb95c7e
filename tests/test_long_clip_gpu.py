"""Clips longer than 64 frames on the MI355X: the long-clip temporal-attention kernel (csrc/attn_temporal.hip,
attn_temporal_long_kernel) at the launch shapes of 96- and 128-frame jobs, and a whole 96-frame capture inversion + CFG edit against
the fp32 oracle.  The emulator versions (every tile boundary, the limit) live in tests/test_long_clip_emu.py."""
import pytest
import torch

from fatezero_amd import _native
from fatezero_amd import kernels as K

import kernel_cases as KC
import pipeline_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"

# cfg4's synthetic variant (Replace + blend words + latent blend, ['mid'] / least_sc_channel, tiny40 width, 64^2 latents, T = 10: the
# cross, self and latent-blend windows all open and close) on a 96-frame clip; registered here, pipeline_cases.py stays as it is
LONG_CASE = "cfg4_attribute_96f_latentblend"
PC.GEOMETRY_CASES.setdefault(LONG_CASE, dict(PC.GEOMETRY_CASES["cfg4_attribute_24f_latentblend"], F=96))


@pytest.fixture(scope="module", autouse=True)
def hip_backend():
    _native.reset_backend()
    assert "hip" in K.version()
    assert _native.loaded_path().endswith("libfatezero_hip.so")
    yield


# the four levels of SD-1.x at 512^2 (8 heads of 40 / 80 / 160 / 160) and the 64^2 level of SD-2.x (5 heads of 64)
SHAPES = [(4096, 8, 40), (1024, 8, 80), (256, 8, 160), (64, 8, 160), (4096, 5, 64)]


@pytest.mark.parametrize("clip", [96, 128])
@pytest.mark.parametrize("tokens,heads,d", SHAPES)
def test_temporal_long_launch_shapes(clip, tokens, heads, d):
    r = KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=heads, d=d, tokens=tokens, seed=clip)
    print("temporal long", clip, tokens, heads, d, r)


@pytest.mark.parametrize("clip,tokens,heads,d", [(96, 4096, 8, 40), (128, 1024, 8, 80), (128, 256, 8, 160), (100, 64, 8, 160),
                                                 (96, 1024, 10, 64)])
def test_temporal_long_cfg_batch(clip, tokens, heads, d):
    # batch 2: the CFG edit runs the uncond / cond halves in one launch
    r = KC.case_attn_temporal(DEV, batch=2, clip=clip, heads=heads, d=d, tokens=tokens, seed=2)
    print("temporal long b2", clip, tokens, heads, d, r)


@pytest.mark.parametrize("clip", [65, 72, 160, 200, K.TEMPORAL_MAX_FRAMES])
def test_temporal_long_other_tile_counts(clip):
    # 3, 5, 7 and 8 key tiles (ragged and full), 160 channels at the limit: one head per workgroup on the opt-in LDS path
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=8, d=40, tokens=300, seed=clip)
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=8, d=160, tokens=17, seed=clip + 1)


@pytest.mark.parametrize("batch,tokens,heads,d", [(1, 4096, 8, 40), (2, 256, 8, 160), (1, 1024, 5, 64)])
def test_temporal_long_frame_sharded_form(batch, tokens, heads, d):
    # q_frames = 16 of kv_frames = 128 (8 ranks x 16 frames): the rows of the whole-clip launch, bit for bit
    clip, lo, hi = 128, 48, 64
    g = torch.Generator().manual_seed(4)
    c, fl = heads * d, hi - lo

    def own(t):
        return t.reshape(batch, clip, *t.shape[1:])[:, lo:hi].reshape(batch * fl, *t.shape[1:]).contiguous()
    qkv = KC._mk((batch * clip, tokens, 3 * c), g, DEV)
    t_full = torch.empty(batch * clip, tokens, c, dtype=torch.float16, device=DEV)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], t_full, batch=batch, clip_len=clip, heads=heads)
    kv = qkv[..., c:].contiguous()
    t_own = torch.full((batch * fl, tokens, c), float("nan"), dtype=torch.float16, device=DEV)
    K.attn_temporal(own(qkv)[..., :c], kv[..., :c], kv[..., c:], t_own, batch=batch, clip_len=fl, kv_frames=clip, heads=heads)
    assert torch.equal(t_own, own(t_full))


def test_beyond_the_limit_is_an_error_on_the_gpu():
    f = K.TEMPORAL_MAX_FRAMES + 1
    x = torch.zeros(f, 4, 80, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match=str(K.TEMPORAL_MAX_FRAMES)):
        K.attn_temporal(x, x, x, torch.empty_like(x), batch=1, clip_len=f, heads=2)


def test_whole_job_96_frames_vs_oracle():
    """A whole capture inversion + CFG edit of a 96-frame clip (tiny40 width, 64^2 latents, T = 10) through the harness and the
    tolerances of the 16-32-frame cases (pipeline_cases.run_geometry_case / check_geometry, GEO_* as they stand)."""
    res = PC.run_geometry_case(LONG_CASE, "cuda", oracle_device="cuda")
    print("geometry", res)
    PC.check_geometry(res)
    assert _native.loaded_path().endswith("libfatezero_hip.so")
