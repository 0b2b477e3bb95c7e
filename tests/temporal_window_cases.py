"""Windowed temporal attention (`model_config.temporal_attention_window`, fz_attn_temporal_win): cases shared by the CPU-emulation suite
(tests/test_temporal_window_emu.py) and the MI355X suite (tests/test_temporal_window_gpu.py).

Kernel reference: fp32 torch with |j - (q_frame0 + i)| > W filled with -inf before the softmax, P through .half().float(), tolerance
4e-3 * max(1, |o|max) -- that of kernel_cases.case_attn_temporal -- and `out` pre-filled with NaN.  q / k / v are column slices of one
packed 3C buffer, as the model passes them.
Model reference: the fp32 oracle with oracle.fatezero_oracle.controlled_attention wrapped so that the controller-free, non-cross calls
whose sequence length is the clip length (the temporal ones: the token counts of the tiny models are 64 / 16 / 4 / 1) get the band mask."""
import torch

from fatezero_amd import kernels as K

import kernel_cases as KC

MAXW = K.TEMPORAL_MAX_WINDOW

# (frames, window): 1. the one-thread-per-query-frame kernels; heads 2, d 40, tokens 5 (a ragged token block), batch 2
THREAD_CASES = [(8, 0), (8, 1), (8, 3), (5, 2), (64, 5)]
# 2. the band kernel at its first length: (frames, window); d in BAND_DIMS; tokens 3; batch 1 and 2
BAND_CASES = [(65, 0), (65, 1), (65, 31), (65, 32), (65, 33), (100, 64), (130, MAXW)]
BAND_DIMS = [(2, 40), (2, 80), (2, 160), (5, 64)]  # (heads, head_dim); 5 x 64: SD-2.x
# 3. past the long kernel's 256 frames and at the limit: (frames, window, heads, head_dim); tokens 2
LONG_CASES = [(264, 16, 2, 40), (512, 8, 2, 40), (512, 8, 2, 160)]
# 4. a rank's own query frames against all frames' K / V: (kv_frames, q_frames, q_frame0, window)
SHARD_CASES = [(130, 33, 0, 20), (130, 33, 17, 20), (130, 33, 97, 20), (16, 4, 8, 2)]
# 5. a window that covers the clip is today's launch
FULL_CASES = [8, 65, 264]


def packed_qkv(device, batch, frames, tokens, heads, d, seed):
    g = torch.Generator().manual_seed(seed)
    return KC._mk((batch * frames, tokens, 3 * heads * d), g, device)


def ref_windowed(q, k, v, *, batch, q_frames, kv_frames, heads, d, window, q_frame0=0):
    """fp32 reference on the CPU: [B*q_frames, tokens, C]."""
    tokens = q.shape[1]

    def r(t, f):  # '(b f) d c -> (b d) f c' then heads
        return t.float().cpu().reshape(batch, f, tokens, heads, d).permute(0, 2, 3, 1, 4)  # [b, tok, h, f, d]
    qh, kh, vh = r(q, q_frames), r(k, kv_frames), r(v, kv_frames)
    s = qh @ kh.transpose(-1, -2) * d ** -0.5
    i = torch.arange(q_frames)[:, None] + q_frame0
    j = torch.arange(kv_frames)[None, :]
    s = s.masked_fill((j - i).abs() > window, float("-inf"))
    p = s.softmax(-1).half().float()
    return (p @ vh).permute(0, 3, 1, 2, 4).reshape(batch * q_frames, tokens, heads * d)


def run_windowed(qkv, *, batch, frames, heads, window, out=None):
    c = qkv.shape[-1] // 3
    if out is None:
        out = torch.full((batch * frames, qkv.shape[1], c), float("nan"), dtype=torch.float16, device=qkv.device)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], out, batch=batch, clip_len=frames, heads=heads, window=window)
    return out


def case_window(device, *, batch, frames, heads, d, tokens, window, seed=0):
    c = heads * d
    qkv = packed_qkv(device, batch, frames, tokens, heads, d, seed)
    out = run_windowed(qkv, batch=batch, frames=frames, heads=heads, window=window)
    o = ref_windowed(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], batch=batch, q_frames=frames, kv_frames=frames, heads=heads, d=d,
                     window=window)
    err = (out.float().cpu() - o).abs().max().item()
    print({"frames": frames, "window": window, "heads": heads, "d": d, "batch": batch, "o_max_err": err, "o_max": float(o.abs().max())})
    assert err < 4e-3 * max(1.0, float(o.abs().max())), err  # (NaN left in `out` fails this comparison too)
    if window == 0:  # the softmax over one key is exactly 1: V of the same frame, bit for bit
        assert torch.equal(out, qkv[..., 2 * c:])
    return out


def case_shard(device, *, kv_frames, q_frames, q_frame0, window, batch=2, heads=2, d=40, tokens=3, seed=11):
    """The rank's rows are torch.equal to the same rows of the whole-clip windowed launch (and within tolerance of the reference)."""
    c = heads * d
    qkv = packed_qkv(device, batch, kv_frames, tokens, heads, d, seed)
    full = run_windowed(qkv, batch=batch, frames=kv_frames, heads=heads, window=window)

    def own(t):
        return t.reshape(batch, kv_frames, *t.shape[1:])[:, q_frame0:q_frame0 + q_frames].reshape(batch * q_frames, *t.shape[1:])
    q = own(qkv)[..., :c]  # (still a column slice of a 3C-wide row)
    kv = qkv[..., c:]
    out = torch.full((batch * q_frames, tokens, c), float("nan"), dtype=torch.float16, device=device)
    K.attn_temporal(q, kv[..., :c], kv[..., c:], out, batch=batch, clip_len=q_frames, kv_frames=kv_frames, heads=heads, window=window,
                    q_frame0=q_frame0)
    o = ref_windowed(q, kv[..., :c], kv[..., c:], batch=batch, q_frames=q_frames, kv_frames=kv_frames, heads=heads, d=d, window=window,
                     q_frame0=q_frame0)
    err = (out.float().cpu() - o).abs().max().item()
    assert err < 4e-3 * max(1.0, float(o.abs().max())), err
    assert torch.equal(out, own(full))


def case_full_window(device, frames, *, heads=2, d=40, tokens=3, seed=5):
    """window = F - 1 and F + 5 are the call without a window, bit for bit."""
    c = heads * d
    qkv = packed_qkv(device, 1, frames, tokens, heads, d, seed)
    plain = torch.full((frames, tokens, c), float("nan"), dtype=torch.float16, device=device)
    K.attn_temporal(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], plain, batch=1, clip_len=frames, heads=heads)
    assert torch.isfinite(plain).all()
    for w in (frames - 1, frames + 5):
        assert torch.equal(run_windowed(qkv, batch=1, frames=frames, heads=heads, window=w), plain), w


def case_strided_out(device, frames, window, *, heads=2, d=40, tokens=3, seed=5):
    """`out` is a column slice of a wider buffer pre-filled with a sentinel: the contiguous result, and the sentinel untouched."""
    c = heads * d
    qkv = packed_qkv(device, 1, frames, tokens, heads, d, seed)
    ref = run_windowed(qkv, batch=1, frames=frames, heads=heads, window=window)
    wide = torch.full((frames, tokens, c + 16), 7.0, dtype=torch.float16, device=device)
    run_windowed(qkv, batch=1, frames=frames, heads=heads, window=window, out=wide[..., 8:8 + c])
    assert torch.isfinite(ref).all() and torch.equal(wide[..., 8:8 + c], ref)
    assert bool((wide[..., :8] == 7.0).all()) and bool((wide[..., 8 + c:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# model and job cases
# ---------------------------------------------------------------------------------------------------------------------------------
FORWARD_TOL = 1.5e-2  # of the output range: the bound of the emulator's UNet-forward cases


def band_oracle(monkeypatch, frames, window):
    """Wrap oracle.fatezero_oracle.controlled_attention (through pytest's monkeypatch; no file under oracle/ changes): the
    controller-free, non-cross calls whose sequence length is `frames` attend only the keys within `window` of the query."""
    from oracle import fatezero_oracle as O
    real = O.controlled_attention
    hits = [0]

    def wrapped(q, k, v, heads, scale, controller, is_cross, place):
        if controller is None and not is_cross and q.shape[1] == frames and k.shape[1] == frames:
            hits[0] += 1
            bt, n, c = q.shape

            def split(t):
                return t.reshape(bt, n, heads, c // heads).permute(0, 2, 1, 3)
            s = split(q) @ split(k).transpose(-1, -2) * scale
            idx = torch.arange(n, device=q.device)
            s = s.masked_fill((idx[None, :] - idx[:, None]).abs() > window, float("-inf"))
            return (s.softmax(-1) @ split(v)).permute(0, 2, 1, 3).reshape(bt, n, c)
        return real(q, k, v, heads, scale, controller, is_cross, place)
    monkeypatch.setattr(O, "controlled_attention", wrapped)
    return hits


def tiny16_pair(mc_extra=None):
    """(native UNet in fp16, its state dict) of the tiny16 width with `lora: 16` and procedural weights."""
    import pipeline_cases as PC
    from oracle.weights import procedural_state_dict
    from fatezero_amd.video_diffusion.models import UNetPseudo3DConditionModel
    mc = dict({"lora": 16}, **(mc_extra or {}))
    unet = UNetPseudo3DConditionModel(sample_size=64, **PC.TINY["tiny16"], **mc)
    sd = procedural_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()])
    unet.load_state_dict(sd)
    return unet.half().eval(), sd


def forward_inputs(frames, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 4, frames, 8, 8, generator=g), torch.randn(1, 77, 64, generator=g) * 0.5


def case_unet_forward_vs_band_oracle(device, monkeypatch, *, frames, window):
    """One tiny16 UNet forward against the fp32 oracle with the band mask.  First: the windowed and unwindowed references differ by more
    than 3 x the tolerance, so a model that ignores the key cannot pass."""
    import pipeline_cases as PC
    from oracle import fatezero_oracle as O
    unet, sd = tiny16_pair({"temporal_attention_window": window})
    ounet = O.OracleUNet(sd, O.UNetConfig(**PC.TINY["tiny16"], model_config={"lora": 16}))
    z, ctx = forward_inputs(frames)
    ref_full = ounet(z, 481, ctx)
    with monkeypatch.context() as mp:
        hits = band_oracle(mp, frames, window)
        ref = ounet(z, 481, ctx)
    scale = float(ref.abs().max())
    moved = float((ref - ref_full).abs().max())
    print({"frames": frames, "window": window, "oracle_moved": moved, "scale": scale, "temporal_calls": hits[0]})
    assert hits[0] == 16, hits  # every transformer block's temporal attention, nothing else
    assert moved > 3 * FORWARD_TOL * scale, (moved, scale)
    unet = unet.to(device)
    y = unet(z.half().to(device), 481, ctx.half().to(device)).sample.float().cpu()
    err = float((y - ref).abs().max())
    print({"frames": frames, "window": window, "err": err, "scale": scale})
    assert torch.isfinite(y).all() and err <= FORWARD_TOL * scale, (err, scale)


def case_absent_none_and_full_window_are_equal(device, frames=12):
    """`temporal_attention_window` absent, None and F - 1: torch.equal outputs (and a window that bites moves the output)."""
    z, ctx = forward_inputs(frames)
    outs = []
    for extra in ({}, {"temporal_attention_window": None}, {"temporal_attention_window": frames - 1}, {"temporal_attention_window": 1}):
        unet, _ = tiny16_pair(extra)
        outs.append(unet.to(device)(z.half().to(device), 481, ctx.half().to(device)).sample)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.equal(outs[0], outs[3])


def tiny_job(device, *, frames, steps, window, recompute=False, shard=None):
    """Capture inversion + CFG edit of a tiny16 clip at 8^2 latents (the job of tests/test_recompute_maps_gloo.py):
    [inverted latent, edited latent]."""
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    mc = {"lora": 16, "SparseCausalAttention_index": [-1, "first"]}
    if window is not None:
        mc["temporal_attention_window"] = window
    unet = PC.build_unet("tiny16", mc, device)
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                         recompute_maps=recompute)
    pipe.frame_shard = shard
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(7)
    emb = (torch.randn(2, 77, 64, generator=g)).to(device)
    pipe._encode_prompt = lambda *a, **k: emb
    z0 = torch.randn(1, 4, frames, 8, 8, generator=g).to(device)
    pipe.scheduler.set_timesteps(steps)
    lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True,
                                             LOW_RESOURCE=True, latents=z0)
    out = pipe(prompt="a red car", source_prompt="a blue car", edit_type="swap", num_inference_steps=steps, latents=lat[-1],
               output_type="latent", cross_replace_steps={"default_": 0.5}, self_replace_steps=0.5, use_inversion_attention=True,
               is_replace_controller=True, save_self_attention=False, guidance_scale=3.0)
    return torch.stack([lat[-1].float().cpu(), out["sdimage_output"].images.float().cpu()])


def case_tiny_whole_job(device, frames=6, steps=4, window=1):
    """recompute_maps=True is torch.equal to the resident job under a window, and both differ from the unwindowed job."""
    res = tiny_job(device, frames=frames, steps=steps, window=window)
    rec = tiny_job(device, frames=frames, steps=steps, window=window, recompute=True)
    plain = tiny_job(device, frames=frames, steps=steps, window=None)
    assert torch.isfinite(res).all() and torch.isfinite(plain).all()
    assert torch.equal(rec, res), float((rec - res).abs().max())
    moved, scale = float((res - plain).abs().max()), float(plain.abs().max())
    print({"frames": frames, "steps": steps, "window": window, "moved": moved, "scale": scale})
    assert moved > 3 * FORWARD_TOL * scale, (moved, scale)  # far outside what fp16 noise between two equal jobs could be


def gloo_worker(rank, world, port, frames, window, q):
    """One rank of a frame-sharded windowed job on the CPU emulation (spawned; the harness of tests/test_recompute_maps_gloo.py)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      FZ_EMU_THREADS="2")
    torch.set_num_threads(2)
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from fatezero_amd import _native as N, build as B, dist as D
    import torch.distributed as dist
    N.use_test_backend(os.environ.get("FZ_EMU_LIB") or B.build_emu())
    D.init("gloo")
    shard = D.FrameShard(frames)
    got = tiny_job("cpu", frames=frames, steps=3, window=window, shard=shard)
    if rank == 0:
        q.put(got.clone())
    dist.barrier()
    dist.destroy_process_group()
