"""Clips longer than 64 frames, WITHOUT a GPU: the long-clip temporal-attention kernel (csrc/attn_temporal.hip,
attn_temporal_long_kernel) on the CPU emulation of csrc/fz_rt.h -- its tile boundaries (32-frame key tiles, 32-frame query tiles,
16-channel contraction chunks, 32-channel output tiles), the limit FZ_TEMPORAL_MAX_FRAMES, the frame-sharded form, and a UNet
forward beyond 64 frames against the fp32 oracle.  The MI355X versions live in tests/test_long_clip_gpu.py."""
import ctypes as C
import os

import pytest
import torch

from fatezero_amd import _native, build
from fatezero_amd import kernels as K

import kernel_cases as KC

LIMIT = K.TEMPORAL_MAX_FRAMES


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(os.environ.get("FZ_EMU_LIB") or build.build_emu())
    yield
    _native.reset_backend()


DEV = "cpu"


def test_limit_is_the_headers():
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "fatezero_hip.h")).read()
    assert int(re.search(r"#define FZ_TEMPORAL_MAX_FRAMES (\d+)", hdr).group(1)) == LIMIT >= 256


# every key-tile count of the kernel (3..8 tiles of 32 frames), full and ragged last tiles, the first length past the old kernels
@pytest.mark.parametrize("clip", [65, 72, 96, 100, 128, 129, 160, 191, 224, 255, LIMIT])
@pytest.mark.parametrize("d", [16, 40, 64])
def test_temporal_long_vs_fp32(clip, d):
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=2, d=d, tokens=3, seed=clip + d)


@pytest.mark.parametrize("clip,heads,d,tokens", [(65, 2, 40, 3), (96, 3, 16, 2), (100, 1, 64, 2), (128, 2, 40, 2), (LIMIT, 2, 16, 2)])
def test_temporal_long_batch2(clip, heads, d, tokens):
    KC.case_attn_temporal(DEV, batch=2, clip=clip, heads=heads, d=d, tokens=tokens, seed=7)


@pytest.mark.parametrize("clip,heads,d", [(96, 8, 80), (72, 8, 160), (LIMIT, 1, 160), (100, 5, 64), (96, 16, 40)])
def test_temporal_long_head_groups(clip, heads, d):
    # the launcher packs the largest divisor of `heads` whose transposed V fits 64 KB into a workgroup: 8 x 80 at 96 frames -> 2 heads,
    # 8 x 160 -> 1, 160 channels at the limit -> one head on the opt-in LDS path (84.5 KB), 5 x 64 (an SD-2.x level) -> 1, 16 x 40 -> 4
    KC.case_attn_temporal(DEV, batch=1, clip=clip, heads=heads, d=d, tokens=2, seed=3)


def _own_vs_full(batch, clip, lo, hi, heads, d, tokens, seed=0):
    """tests/kernel_cases.py:255-270 for the temporal kernel alone: a rank's own query frames against all frames' K / V give the
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


@pytest.mark.parametrize("batch,clip,lo,hi,heads,d", [(1, 96, 24, 48, 2, 40), (2, 128, 112, 128, 2, 16), (1, 100, 0, 33, 2, 64),
                                                      (1, LIMIT, 60, 130, 1, 40), (1, 72, 71, 72, 2, 16)])
def test_temporal_long_query_frames_of_one_rank(batch, clip, lo, hi, heads, d):
    _own_vs_full(batch, clip, lo, hi, heads, d, tokens=2)


def test_temporal_long_queries_only():
    # q_frames > 64 >= kv_frames: legal for the _ex entry, served by the long kernel with two key tiles
    g = torch.Generator().manual_seed(1)
    heads, d, tokens, fq, fk = 2, 40, 2, 70, 40
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


def test_temporal_long_strided_rows_and_untouched_neighbours():
    # q / k / v are column slices of one packed row (stride 3C) and `out` a column slice of a wider buffer: nothing outside the
    # [tokens][C] block of `out` may be written
    g = torch.Generator().manual_seed(5)
    clip, heads, d, tokens = 72, 2, 40, 3
    c = heads * d
    qkv = KC._mk((clip, tokens, 3 * c), g, DEV)
    wide = torch.full((clip, tokens, c + 16), 7.0, dtype=torch.float16)
    ref = torch.empty(clip, tokens, c, dtype=torch.float16)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], ref, batch=1, clip_len=clip, heads=heads)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], wide[..., 8:8 + c], batch=1, clip_len=clip, heads=heads)
    assert torch.equal(wide[..., 8:8 + c], ref)
    assert bool((wide[..., :8] == 7.0).all()) and bool((wide[..., 8 + c:] == 7.0).all())


def test_beyond_the_limit_is_an_error():
    heads, d, tokens = 1, 16, 1
    for fq, fk in ((LIMIT + 1, LIMIT + 1), (8, LIMIT + 1), (LIMIT + 1, 8)):
        q = torch.zeros(fq, tokens, heads * d, dtype=torch.float16)
        kv = torch.zeros(fk, tokens, heads * d, dtype=torch.float16)
        out = torch.zeros_like(q)
        with pytest.raises(ValueError, match=str(LIMIT)):
            K.attn_temporal(q, kv, kv, out, batch=1, clip_len=fq, kv_frames=fk, heads=heads)
        rc = _native.lib().fz_attn_temporal_ex(C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr()),
                                               C.c_void_p(out.data_ptr()), 1, fq, fk, tokens, heads, d, heads * d, heads * d,
                                               heads * d, 0.25, C.c_void_p(0))
        assert rc == -1  # FZ_ERR_BAD_ARG
    f = LIMIT + 1
    x = torch.zeros(f, tokens, heads * d, dtype=torch.float16)
    rc = _native.lib().fz_attn_temporal(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()),
                                        C.c_void_p(x.data_ptr()), 1, f, tokens, heads, d, heads * d, heads * d, 0.25, C.c_void_p(0))
    assert rc == -1


# ---------------------------------------------------------------------------------------------------------------
# the rest of the stack beyond 64 frames
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_unet_forward_72_frames_vs_oracle():
    """One UNet forward (tiny16 width, 8^2 latents: the smallest the three downsamplers accept) on a 72-frame clip against the fp32
    oracle on the CPU, with the tolerance of the emulator's forward cases (tests/test_pipeline_emu.py: 1.5e-2 of the output range).
    GroupNorm statistics over 72 frames x tokens rows, the temporal convolution's frame axis, sparse-causal sources clamped at frame 71,
    and temporal attention with three key tiles (the last one ragged) in all 16 transformer blocks."""
    import pipeline_cases as PC
    from oracle import fatezero_oracle as O
    from oracle.weights import procedural_state_dict
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    frames, mc = 72, {"lora": 16}
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


@pytest.mark.slow
def test_frame_sharded_96_frames_four_ranks_match_single_process():
    """A 96-frame clip over 4 gloo ranks (24 frames each; every rank's temporal attention runs q_frames = 24 against the all-gathered
    kv_frames = 96) against the single-process job: the comparison and the tolerance of
    tests/test_dist_gloo.py::test_frame_sharded_clip_four_ranks_eight_frames."""
    import test_dist_gloo as TG
    got, n_maps, n_local, stats = TG._spawn(4, 96, [-1, "first"], True)
    TG._check_exchange_structure(stats)
    _, job = TG._frame_job_factory(96, [-1, "first"])
    try:
        ref = job()
    finally:
        _native.use_test_backend(os.environ.get("FZ_EMU_LIB") or build.build_emu())  # (the module fixture's backend)
    assert n_local == 24 and n_maps and all(n == 24 for n in n_maps), (n_maps, n_local)
    err = float((got.float() - ref.float()).abs().max())
    scale = float(ref.float().abs().max())
    print({"err": err, "scale": scale})
    assert torch.isfinite(got.float()).all() and err <= 1.5e-2 * scale, (err, scale)
