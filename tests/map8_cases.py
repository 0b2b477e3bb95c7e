"""E5M2 storage of captured self-attention maps (FZ_ATTN_CAPTURE8 / FZ_ATTN_INJECT8, AttentionStore(map_dtype="e5m2")): cases shared by the
CPU-emulation suite (tests/test_map8_emu.py) and the MI355X suite (tests/test_map8_gpu.py).

Kernel level: the 8-bit launches are checked against the fp16 launches of the SAME inputs -- the stored bytes are the fp16 map rounded by
torch (`P16.to(torch.float8_e5m2)`), the inject reads back exactly the fp16 values those bytes stand for -- so every comparison but the
fp32 restatement is bit for bit.  Each case computes its launches once (`kernel_case`, cached) and the tests read from that."""
import functools

import torch

from fatezero_amd import kernels as K

import kernel_cases as KC

# (d, lq, lkf, index_list, clip): query tails below 128 rows (64, 80, 144 = 128 + 16), key tails below 64 (80, 144, 72), the element-wise
# path (lkf = 72: 72 % 16 != 0 while the fp16 kernel still takes its vector path, 72 % 8 == 0), one and two kv slots, every head dim of SD-1.x
KERNEL_CASES = {
    "d40_lq64": (40, 64, 64, [-1, "first"], 2),
    "d64_lq80_one_slot": (64, 80, 80, ["mid"], 3),
    "d80_lq144": (80, 144, 144, [-1, "first"], 2),
    "d160_lkf72_elementwise": (160, 64, 72, [-1, "first"], 2),
    "d40_lq144_lkf72_one_slot": (40, 144, 72, [0], 3),
}
REAL_16x16 = ("real16", (80, 256, 256, [-1, "first"], 8), 8)  # the 16^2 level of an 8-frame 512^2 clip: full tiles, vector paths only
HEADS = 2
SENTINEL = 0xA5


def _split_mask(clip, lq, device):
    """1 keeps the live attention.  Every 32-row wave slice of every query tile holds both kinds of row."""
    m = torch.zeros(clip, lq)
    m[:, ::3] = 1.0
    m[:, 5:11] = 1.0
    return m.to(device)


@functools.lru_cache(maxsize=None)
def kernel_case(name, device, heads=HEADS):
    d, lq, lkf, index_list, clip = KERNEL_CASES[name] if name in KERNEL_CASES else REAL_16x16[1]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    batch = 2  # the second half of the batch is the controlled one (frame0 != 0), as in a CFG edit
    n, c = batch * clip, heads * d
    q = KC._mk((n, lq, c), g, device, 1.5)
    k = KC._mk((n, lkf, c), g, device, 1.5)
    v = KC._mk((n, lkf, c), g, device)
    vt = K.transpose_pad(v, K.pad64(lkf))
    n_kv = max(1, len(index_list))
    lk = n_kv * lkf
    kw = dict(clip_len=clip, heads=heads, index_list=index_list, frame0=clip, n_frames=clip, p_frame_off=1)  # p frame 0 is never touched

    def out():
        o = torch.full((n, lq, c), float("nan"), dtype=torch.float16, device=device)
        K.attn_self(q, k, vt, o, clip_len=clip, heads=heads, index_list=index_list, mode=K.FZ_ATTN_FLASH, frame0=0, n_frames=clip)
        return o

    r = dict(d=d, lq=lq, lkf=lkf, clip=clip, heads=heads, n=n, lk=lk)
    # ---- capture: fp16 and 8-bit -----------------------------------------------------------------------------
    p16 = torch.full((clip + 1, heads, lq, lk), float("nan"), dtype=torch.float16, device=device)
    r["o_cap16"] = K.attn_self(q, k, vt, out(), mode=K.FZ_ATTN_CAPTURE, p=p16, **kw)
    p8 = torch.full((clip + 1, heads, lq, lk), SENTINEL, dtype=torch.uint8, device=device)
    r["o_cap8"] = K.attn_self(q, k, vt, out(), mode=K.FZ_ATTN_CAPTURE8, p=p8, **kw)
    r["p16"], r["p8"] = p16, p8
    # ---- inject: the 8-bit launch on the bytes, the fp16 launch on the fp16 tensor that holds the same values ----
    deq = K.e5m2_to_half(p8)
    r["deq"] = deq
    for tag, mask in (("all_stored", None), ("split", _split_mask(clip, lq, device))):
        kk = k if (mask is not None or lkf != lq) else None  # (without k the wrapper takes lkf = lq; with no mask the kernel never reads it)
        r["o_inj8_" + tag] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT8, p=p8.view(torch.float8_e5m2) if tag == "split" else p8,
                                         row_mask=mask, **kw)
        r["o_inj16_" + tag] = K.attn_self(q, kk, vt, out(), mode=K.FZ_ATTN_INJECT, p=deq, row_mask=mask, **kw)
    r["mask"] = _split_mask(clip, lq, device)
    r["qkv"] = (q, k, v, index_list)
    return r


def check_capture8_bytes(r):
    p16, p8 = r["p16"].cpu(), r["p8"].cpu()
    assert torch.isfinite(p16[1:].float()).all()
    want = p16[1:].to(torch.float8_e5m2).view(torch.uint8)
    assert torch.equal(p8[1:], want), int((p8[1:] != want).sum())
    assert (p8[0] == SENTINEL).all(), "frame 0 of the map lies in front of p_frame_off: never written"
    assert torch.equal(r["o_cap8"].cpu(), r["o_cap16"].cpu()), "the launch's own output must not depend on the storage format"
    # the helper the store uses for its fp16 views is the exact inverse on these bytes
    assert torch.equal(K.e5m2_to_half(p8[1:]), want.view(torch.float8_e5m2).to(torch.float16))
    # what the rounding costs, reported: at most 2^-3 relative (2 of 10 mantissa bits kept), half an E5M2 subnormal step below that
    rel = ((K.e5m2_to_half(p8[1:]).float() - p16[1:].float()).abs() / p16[1:].float().clamp_min(2.0 ** -14)).max()
    assert float(rel) <= 2.0 ** -3, float(rel)
    return float(rel)


def check_inject8_same_bits(r):
    for tag in ("all_stored", "split"):
        a, b = r["o_inj8_" + tag].cpu(), r["o_inj16_" + tag].cpu()
        assert torch.isfinite(a.float()).all(), tag
        assert torch.equal(a, b), (tag, float((a.float() - b.float()).abs().max()))
    m = r["mask"].cpu()
    for f in range(m.shape[0]):  # the split mask really splits every 32-row slice
        for r0 in range(0, m.shape[1], 32):
            s = m[f, r0:r0 + 32]
            assert 0 < float(s.sum()) < s.numel()


def check_inject8_vs_fp32(r):
    """fp32 torch restatement on the DEQUANTISED map (the quantisation is not in this comparison), at the tolerance of the fp16 inject
    cases (kernel_cases.case_attn_self)."""
    q, k, v, index_list = r["qkv"]
    clip, heads, n, lq = r["clip"], r["heads"], r["n"], r["lq"]
    qf, kf, vf = q.float().cpu(), k.float().cpu(), v.float().cpu()
    c = qf.shape[-1]
    d = c // heads
    b = n // clip
    idx = KC._frame_indices(index_list, clip)
    k5, v5 = kf.reshape(b, clip, -1, c), vf.reshape(b, clip, -1, c)
    kc = torch.cat([k5[:, fi] for fi in idx], dim=2).reshape(n, -1, c)
    vc = torch.cat([v5[:, fi] for fi in idx], dim=2).reshape(n, -1, c)
    qh = qf.reshape(n, lq, heads, d).permute(0, 2, 1, 3)
    kh = kc.reshape(n, -1, heads, d).permute(0, 2, 1, 3)
    vh = vc.reshape(n, -1, heads, d).permute(0, 2, 1, 3)
    p_live = (qh @ kh.transpose(-1, -2) * d ** -0.5).softmax(-1)
    base = r["deq"][1:].float().cpu()
    worst = 0.0
    for tag in ("all_stored", "split"):
        p_new = p_live.clone()
        if tag == "all_stored":
            p_new[clip:] = base
        else:
            m = r["mask"].cpu()[:, None, :, None]
            p_new[clip:] = m * p_live[clip:] + (1 - m) * base
        o_ref = (p_new @ vh).permute(0, 2, 1, 3).reshape(n, lq, c)
        err = float((r["o_inj8_" + tag].float().cpu() - o_ref).abs().max())
        assert err < 4e-3 * max(1.0, float(o_ref.abs().max())), (tag, err)
        worst = max(worst, err)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the tiny whole job against the fp32 oracle (MI355X suite): pipeline_cases.run_geometry_case as it stands, on a pipeline built with
# `map_dtype`
# ---------------------------------------------------------------------------------------------------------------
WHOLE_JOB = "map8_tiny40_4f"
WHOLE_JOB_CASE = dict(kind="tiny40", F=4, L=64, T=4, model_config={"lora": 16}, prompt_case="teaser_posche", is_replace=True,
                      cross_replace={"default_": 0.5}, self_replace=0.5, eq_params=None,
                      blend_words=[["silver", "jeep"], ["Porsche", "car"]], blend_th=None, blend_latents=False, regime="split")


def whole_job(device, map_dtype, oracle_device=None):
    """tiny40 geometry (head dims 40 / 80 / 160, default index [-1, 'first']), 4 frames, 64^2 latents, T = 4 + 4: Replace + blend-masked
    self-attention, cross window [0, 2), self window [0, 2).  Returns run_geometry_case's result dict."""
    import pipeline_cases as PC
    PC.GEOMETRY_CASES[WHOLE_JOB] = WHOLE_JOB_CASE
    orig, made = PC.P2pDDIMSpatioTemporalPipeline, []

    def build(*a, **k):
        made.append(orig(*a, map_dtype=map_dtype, **k))
        return made[-1]
    PC.P2pDDIMSpatioTemporalPipeline = build
    try:
        res = PC.run_geometry_case(WHOLE_JOB, device, oracle_device=oracle_device)
    finally:
        PC.P2pDDIMSpatioTemporalPipeline = orig
        del PC.GEOMETRY_CASES[WHOLE_JOB]
    # the harness did build its pipeline through the name replaced above, and that pipeline's store has the format asked for
    assert len(made) == 1 and made[0].store_controller.map_dtype == map_dtype and len(made[0].store_controller.attention_store_all_step) == \
        WHOLE_JOB_CASE["T"], (len(made), map_dtype)
    self_maps = made[0].store_controller.maps_of_step(0)["down_self"]
    assert self_maps and all(cm.is_8bit == (map_dtype == "e5m2") for cm in self_maps)
    return res
