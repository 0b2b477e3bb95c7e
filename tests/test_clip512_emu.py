"""Clips of 257 to 512 frames, WITHOUT a GPU: the streaming temporal-attention kernel (csrc/attn_temporal.hip,
attn_temporal_stream_kernel) on the CPU emulation of csrc/fz_rt.h -- its chunk boundaries (key chunks of 256 frames, 32-frame key
and query tiles, groups of four query tiles, head groups), the limit FZ_TEMPORAL_MAX_FRAMES = 512, the frame-sharded form, and a
UNet forward beyond 256 frames against the fp32 oracle.  The MI355X versions live in tests/test_clip512_gpu.py."""
import ctypes as C
import os
import re

import pytest
import torch

from fatezero_amd import _native, build
from fatezero_amd import kernels as K

import kernel_cases as KC

LIMIT = K.TEMPORAL_MAX_FRAMES
DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(os.environ.get("FZ_EMU_LIB") or build.build_emu())
    yield
    _native.reset_backend()


def test_limit_is_512_in_header_and_python():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "fatezero_hip.h")).read()
    assert int(re.search(r"#define FZ_TEMPORAL_MAX_FRAMES (\d+)", hdr).group(1)) == LIMIT == 512


# the first length past the long kernel, a full chunk plus one tile, ragged last tiles in the second chunk, the limit
@pytest.mark.parametrize("clip", [257, 288, 320, 384, 385, 480, 511, 512])
@pytest.mark.parametrize("d", [16, 40, 64])
def test_temporal_stream_vs_fp32(clip, d):
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=2, d=d, tokens=3, seed=clip + d)


@pytest.mark.parametrize("clip,heads,d", [(300, 2, 40), (512, 2, 16)])
def test_temporal_stream_batch2(clip, heads, d):
    KC.case_attn_temporal(DEV, batch=2, clip=clip, heads=heads, d=d, tokens=3, seed=7)


@pytest.mark.parametrize("clip,heads,d", [(288, 8, 80), (512, 1, 160), (320, 5, 64), (288, 16, 40)])
def test_temporal_stream_head_groups(clip, heads, d):
    # heads per workgroup: the largest divisor of `heads` whose transposed 256-key V chunk fits 64 KB and whose O accumulators are
    # at most five 32-channel tiles: 8 x 80 -> 1 head (three tiles), 160 channels -> one head on the opt-in LDS path (82.5 KB,
    # five tiles), 5 x 64 -> 1, 16 x 40 -> 2 heads (four tiles)
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=heads, d=d, tokens=2, seed=3)


def _own_vs_full(batch, clip, lo, hi, heads, d, tokens, seed=0):
    """tests/test_long_clip_emu.py::_own_vs_full beyond 256 frames: a rank's own query frames against all frames' K / V give the
    rows of the whole-clip launch, bit for bit."""
    g = torch.Generator().manual_seed(seed)
    c, fl = heads * d, hi - lo

    def own(t):
        return t.reshape(batch, clip, *t.shape[1:])[:, lo:hi].reshape(batch * fl, *t.shape[1:]).contiguous()
    qkv = KC._mk((batch * clip, tokens, 3 * c), g, DEV)
    t_full = torch.empty(batch * clip, tokens, c, dtype=torch.float16)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], t_full, batch=batch, clip_len=clip, heads=heads)
    kv = qkv[..., c:].contiguous()
    t_own = torch.full((batch * fl, tokens, c), float("nan"), dtype=torch.float16)
    K.attn_temporal(own(qkv)[..., :c], kv[..., :c], kv[..., c:], t_own, batch=batch, clip_len=fl, kv_frames=clip, heads=heads)
    assert torch.equal(t_own, own(t_full))


@pytest.mark.parametrize("batch,clip,lo,hi,heads,d", [(1, 320, 250, 290, 2, 40), (1, 512, 500, 512, 1, 40), (2, 288, 0, 33, 2, 16),
                                                      (1, 300, 299, 300, 2, 64)])
def test_temporal_stream_query_frames_of_one_rank(batch, clip, lo, hi, heads, d):
    _own_vs_full(batch, clip, lo, hi, heads, d, tokens=2)


# 256 frames, the last length of attn_temporal_long_kernel (eight key tiles, whole score rows in registers).  tests/test_long_clip_emu.py
# parameterises its longest cases by the limit, so they follow it to 512; these pin the same cases at 256
@pytest.mark.parametrize("d", [16, 40, 64])
def test_temporal_long_256_vs_fp32(d):
    KC.case_attn_temporal(DEV, batch=1, clip=256, heads=2, d=d, tokens=3, seed=256 + d)


def test_temporal_long_256_batch2():
    KC.case_attn_temporal(DEV, batch=2, clip=256, heads=2, d=16, tokens=2, seed=7)


def test_temporal_long_256_head_group_opt_in_lds():
    # 160 channels at 256 frames: one head per workgroup on the long kernel's opt-in LDS path (84.5 KB)
    KC.case_attn_temporal(DEV, batch=1, clip=256, heads=1, d=160, tokens=2, seed=3)


def test_temporal_long_256_query_frames_of_one_rank():
    _own_vs_full(1, 256, 60, 130, 1, 40, tokens=2)


@pytest.mark.parametrize("fq,fk", [(300, 40), (8, 300)])
def test_temporal_stream_mixed_lengths(fq, fk):
    # either count beyond 256 selects the streaming kernel: ten query tiles against two key tiles, one query tile against two chunks
    g = torch.Generator().manual_seed(1)
    heads, d, tokens = 2, 40, 2
    c = heads * d
    q = KC._mk((fq, tokens, c), g, DEV)
    kv = KC._mk((fk, tokens, 2 * c), g, DEV)
    out = torch.full((fq, tokens, c), float("nan"), dtype=torch.float16)
    K.attn_temporal(q, kv[..., :c], kv[..., c:], out, batch=1, clip_len=fq, kv_frames=fk, heads=heads)
    qh = q.float().reshape(fq, tokens, heads, d).permute(1, 2, 0, 3)
    kh = kv[..., :c].float().reshape(fk, tokens, heads, d).permute(1, 2, 0, 3)
    vh = kv[..., c:].float().reshape(fk, tokens, heads, d).permute(1, 2, 0, 3)
    o = ((qh @ kh.transpose(-1, -2) * d ** -0.5).softmax(-1).half().float() @ vh).permute(2, 0, 1, 3).reshape(fq, tokens, c)
    err = (out.float() - o).abs().max().item()
    assert err < 4e-3 * max(1.0, float(o.abs().max())), err


def test_temporal_stream_strided_rows_and_untouched_neighbours():
    # q / k / v are column slices of one packed row (stride 3C) and `out` a column slice of a wider buffer: nothing outside the
    # [tokens][C] block of `out` may be written
    g = torch.Generator().manual_seed(5)
    clip, heads, d, tokens = 300, 2, 40, 3
    c = heads * d
    qkv = KC._mk((clip, tokens, 3 * c), g, DEV)
    wide = torch.full((clip, tokens, c + 16), 7.0, dtype=torch.float16)
    ref = torch.empty(clip, tokens, c, dtype=torch.float16)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], ref, batch=1, clip_len=clip, heads=heads)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], wide[..., 8:8 + c], batch=1, clip_len=clip, heads=heads)
    assert torch.equal(wide[..., 8:8 + c], ref)
    assert bool((wide[..., :8] == 7.0).all()) and bool((wide[..., 8 + c:] == 7.0).all())


def test_beyond_512_is_an_error():
    heads, d, tokens = 1, 16, 1
    for fq, fk in ((513, 513), (8, 513), (513, 8)):
        q = torch.zeros(fq, tokens, heads * d, dtype=torch.float16)
        kv = torch.zeros(fk, tokens, heads * d, dtype=torch.float16)
        out = torch.zeros_like(q)
        with pytest.raises(ValueError, match="512"):
            K.attn_temporal(q, kv, kv, out, batch=1, clip_len=fq, kv_frames=fk, heads=heads)
        rc = _native.lib().fz_attn_temporal_ex(C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr()),
                                               C.c_void_p(out.data_ptr()), 1, fq, fk, tokens, heads, d, heads * d, heads * d,
                                               heads * d, 0.25, C.c_void_p(0))
        assert rc == -1  # FZ_ERR_BAD_ARG
    x = torch.zeros(513, tokens, heads * d, dtype=torch.float16)
    rc = _native.lib().fz_attn_temporal(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()),
                                        C.c_void_p(x.data_ptr()), 1, 513, tokens, heads, d, heads * d, heads * d, 0.25, C.c_void_p(0))
    assert rc == -1


@pytest.mark.slow
def test_unet_forward_264_frames_vs_oracle():
    """One UNet forward (tiny16 width, 8^2 latents) on a 264-frame clip against the fp32 oracle on the CPU, the pattern and the
    bound of tests/test_long_clip_emu.py::test_unet_forward_72_frames_vs_oracle (1.5e-2 of the output range): temporal attention
    with nine key tiles (a full chunk and a ragged tile in the second) in all 16 transformer blocks."""
    import pipeline_cases as PC
    from oracle import fatezero_oracle as O
    from oracle.weights import procedural_state_dict
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    frames, mc = 264, {"lora": 16}
    unet = UNetPseudo3DConditionModel(sample_size=64, **PC.TINY["tiny16"], **mc)
    sd = procedural_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()])
    unet.load_state_dict(sd)
    unet = unet.half().eval()
    ounet = O.OracleUNet(sd, O.UNetConfig(**PC.TINY["tiny16"], model_config=mc))
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 4, frames, 8, 8, generator=g)
    ctx = torch.randn(1, 77, 64, generator=g) * 0.5
    y = unet(z.half(), 481, ctx.half()).sample.float()
    ref = ounet(z, 481, ctx)
    err, scale = float((y - ref).abs().max()), float(ref.abs().max())
    print({"frames": frames, "err": err, "scale": scale})
    assert torch.isfinite(y).all() and err <= 1.5e-2 * scale, (err, scale)
