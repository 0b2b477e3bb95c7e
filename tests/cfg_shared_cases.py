"""The CFG-shared head (unet_3d_condition.py: CFG_SHARED_HEAD): the broadcast forms of the kernels at its divergence point against the same
entry fed the explicitly expanded operand, and the model / pipeline with the shared input against the expanded one.  Shared by the
CPU-emulation suite and the MI355X suite."""
import torch
import torch.nn.functional as F

from fatezero_amd import kernels as K
from fatezero_amd.video_diffusion.models import unet_3d_condition as U
from fatezero_amd.video_diffusion.models.resnet import Tokens


def _rep(t, r):
    return t.repeat(r, *([1] * (t.dim() - 1))).contiguous()


def case_xattn_in_frames(device, *, tokens, out_frames, in_frames, clip, front, lk=77, seed=0):
    """fz_xattn_chain with FzXattnChain.in_frames: output frame n reads the rows of input frame n % in_frames and the context pack of batch
    element n // clip.  torch.equal to the same entry on the expanded input, and within case_xattn_chain's tolerances of fp32 torch
    (tests/kernel_cases.py: 6e-3 of the scale for y, 2e-3 for the LayerNorm output)."""
    g = torch.Generator().manual_seed(seed)
    c, heads, dh = 320, 8, 40
    n, nb = out_frames, (out_frames + clip - 1) // clip
    r = out_frames // in_frames
    x = (torch.randn(in_frames, tokens, c, generator=g) * 1.2).half()
    res = (torch.randn(in_frames, tokens, c, generator=g) * 1.5).half()
    wq = (torch.randn(c, c, generator=g) * c ** -0.5 * 2.0).half()
    wk = (torch.randn(c, 768, generator=g) * 768 ** -0.5 * 2.0).half()
    wv = (torch.randn(c, 768, generator=g) * 768 ** -0.5).half()
    wo = (torch.randn(c, c, generator=g) * c ** -0.5).half()
    bo = (torch.randn(c, generator=g) * 0.3).half()
    wo1 = (torch.randn(c, c, generator=g) * c ** -0.5).half()
    bo1 = (torch.randn(c, generator=g) * 0.3).half()
    ctx = torch.randn(nb, lk, 768, generator=g).half()
    gam = [(1.0 + 0.2 * torch.randn(c, generator=g)).half() for _ in range(2)]
    bet = [(0.1 * torch.randn(c, generator=g)).half() for _ in range(2)]
    dev = lambda t: t.to(device)
    scale = dh ** -0.5
    kk = K.gemm(dev(ctx), dev(wk))
    vt = K.gemm_vt(dev(ctx), dev(wv), K.CROSS_KEYS)
    kvp = K.xattn_chain_kv_pack(kk, vt, lk)
    packed = K.xattn_chain_pack(dev(wq), dev(wo), (dev(wo1), dev(bo1), dev(gam[0]), dev(bet[0])) if front else None)
    kw = dict(frames_per_batch=clip, heads=heads, lk=lk, scale=scale, ln=(dev(gam[1]), dev(bet[1]), 1e-5))
    if front:
        kw["front_eps"] = 1e-5
    got = K.xattn_chain(dev(x), packed, kvp, dev(bo), res=dev(res), out_frames=n, **kw)
    want = K.xattn_chain(dev(_rep(x, r)), packed, kvp, dev(bo), res=dev(_rep(res, r)), **kw)
    assert all(a.shape[0] == n for a in got)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # fp32 torch on the fp16 operands (kernel_cases.case_xattn_chain's reference)
    xf, rf = _rep(x, r).float(), _rep(res, r).float()
    if front:
        h1 = ((xf @ wo1.float().t() + bo1.float()).half().float() + rf).half().float()
        xn = F.layer_norm(h1, (c,), gam[0].float(), bet[0].float(), 1e-5).half().float()
        rf = h1
    else:
        xn = xf
    qf = (xn @ wq.float().t()).half().float().reshape(n, tokens, heads, dh).permute(0, 2, 1, 3)
    kf = kk.float().cpu().reshape(nb, lk, heads, dh).permute(0, 2, 1, 3)
    vf = vt.float().cpu()[:, :, :lk].reshape(nb, heads, dh, lk).permute(0, 1, 3, 2)
    bidx = torch.arange(n) // clip
    pr = (qf @ kf[bidx].transpose(-1, -2) * scale).softmax(-1)
    of = (pr @ vf[bidx]).permute(0, 2, 1, 3).reshape(n, tokens, c).half().float()
    ref = of @ wo.float().t() + bo.float() + rf
    y, yln = got[0], got[1]
    sc = max(1.0, float(ref.abs().max()))
    err = float((y.float().cpu() - ref).abs().max())
    assert torch.isfinite(y.float()).all() and err < 6e-3 * sc, (err, sc)
    lref = F.layer_norm(y.float().cpu(), (c,), gam[1].float(), bet[1].float(), 1e-5)
    e_ln = float((yln.float().cpu() - lref).abs().max())
    assert e_ln < 2e-3 * max(1.0, float(lref.abs().max())), e_ln
    return {"max_err": err, "ln_vs_torch": e_ln}


def case_gemm_res_rows(device, *, entry, rows=512, res_rows=256, k=320, o=320, split_k=0, tile_cfg=0, seed=0):
    """FzGemmDesc.res_rows through fz_gemm / fz_gemm_lnout / fz_gemm_gn: output row r adds res[r % res_rows].  torch.equal to the same entry
    with the residual expanded (every output of the entry: y, LN(y), the GroupNorm partials).  Returns which outputs the launch produced."""
    g = torch.Generator().manual_seed(seed)
    rpf = 128
    x = torch.randn(rows // rpf, rpf, k, generator=g).half().to(device)
    w = (torch.randn(o, k, generator=g) * k ** -0.5).half().to(device)
    b = torch.randn(o, generator=g).half().to(device)
    res = (torch.randn(res_rows // rpf, rpf, o, generator=g) * 2 - 1).half().to(device)
    full = _rep(res, rows // res_rows)
    if entry == "gemm":
        got = (K.gemm(x, w, b, res=res, split_k=split_k, tile_cfg=tile_cfg),)
        want = (K.gemm(x, w, b, res=full, split_k=split_k, tile_cfg=tile_cfg),)
    elif entry == "lnout":
        gam = (1 + 0.1 * torch.randn(o, generator=g)).half().to(device)
        bet = (0.1 * torch.randn(o, generator=g)).half().to(device)
        got = K.gemm_lnout(x, w, b, (gam, bet, 1e-5), res=res, split_k=split_k, tile_cfg=tile_cfg)
        want = K.gemm_lnout(x, w, b, (gam, bet, 1e-5), res=full, split_k=split_k, tile_cfg=tile_cfg)
    else:
        got = K.gemm_gn(x, w, b, res=res, gn_groups=32, rows_per_frame=rpf, tile_cfg=tile_cfg)
        want = K.gemm_gn(x, w, b, res=full, gn_groups=32, rows_per_frame=rpf, tile_cfg=tile_cfg)
    assert got[0].shape == want[0].shape == (rows // rpf, rpf, o)
    for a, bb in zip(got, want):
        assert (a is None) == (bb is None)
        if a is not None:
            assert torch.equal(a, bb)
    ref = x.float().cpu().reshape(rows, k) @ w.float().cpu().t() + b.float().cpu() + full.float().cpu().reshape(rows, o)
    err = float((got[0].float().cpu().reshape(rows, o) - ref).abs().max())
    assert err < 4e-3 * max(1.0, float(ref.abs().max())), err  # (kernel_cases.case_gemm's bound: the residual really is the broadcast one)
    return [a is not None for a in got]


def case_groupnorm_cat_x2_frames(device, *, n=4, n2=2, span=2, tokens=128, c1=320, c2=320, groups=32, seed=0):
    """fz_groupnorm_cat with the second source broadcast (frame n reads frame n % n2 of it): torch.equal to the expanded call."""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(n, tokens, c1, generator=g).half().to(device)
    x2 = (torch.randn(n2, tokens, c2, generator=g) * 1.5 + 0.5).half().to(device)
    gam = (1 + 0.1 * torch.randn(c1 + c2, generator=g)).half().to(device)
    bet = (0.1 * torch.randn(c1 + c2, generator=g)).half().to(device)
    kw = dict(span=span, groups=groups, eps=1e-5, silu=True)
    got = K.groupnorm_cat(x1, x2, gam, bet, **kw)
    want = K.groupnorm_cat(x1, _rep(x2, n // n2), gam, bet, **kw)
    assert torch.equal(got, want)
    cat = torch.cat([x1, _rep(x2, n // n2)], -1).float().cpu()
    c = c1 + c2
    t = F.silu(F.group_norm(cat.view(n // span, span, tokens, c).permute(0, 3, 1, 2).reshape(n // span, c, -1), groups, gam.float().cpu(),
                            bet.float().cpu(), 1e-5))
    t = t.reshape(n // span, c, span, tokens).permute(0, 2, 3, 1).reshape(n, tokens, c)
    err = float((got.float().cpu() - t).abs().max())
    assert err < 4e-3 * max(1.0, float(t.abs().max())), err
    return err


# ---------------------------------------------------------------------------------------------------------------------------------------
def cfg_forward_pair(unet, device, *, frames, latent, ctx_dim, seed=0, t=481):
    """One CFG forward (batch 2, no controller) on the shared input (rep = 2) and on the expanded one (rep = 1): (shared, expanded) outputs."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(frames, latent * latent, 4, generator=g).half().to(device)
    ctx = torch.randn(2, 77, ctx_dim, generator=g).half().to(device)
    both = torch.cat([tok, tok], 0).contiguous()
    y_rep = unet.forward_tokens(Tokens(tok, 2, frames, latent, latent, rep=2), t, ctx).data
    y_exp = unet.forward_tokens(Tokens(both, 2, frames, latent, latent), t, ctx).data
    assert y_rep.shape == y_exp.shape == (2 * frames, latent * latent, 4)
    assert not torch.equal(y_rep[:frames], y_rep[frames:])  # (the two contexts differ: so must the halves)
    return y_rep, y_exp


def with_switch(value, fn):
    """fn() with unet_3d_condition.CFG_SHARED_HEAD = value."""
    old = U.CFG_SHARED_HEAD
    U.CFG_SHARED_HEAD = value
    try:
        return fn()
    finally:
        U.CFG_SHARED_HEAD = old


def _edit_maps(pipe):
    """Every map tensor the job left behind: the inversion's store and what the edit controller kept of its own pass."""
    out = []
    for st in pipe.store_controller.attention_store_all_step:
        for k in sorted(st):
            out += [(f"inv/{k}", m) for m in st[k]]
    ctrl = pipe.last_edit_controller
    for name in ("attention_store", "step_store"):
        d = getattr(ctrl, name, None)
        if isinstance(d, dict):
            for k in sorted(d):
                out += [(f"edit/{name}/{k}", m) for m in d[k] if isinstance(m, torch.Tensor)]
    return out


def pipeline_on_off(name, device, issue_plans=False, monkeypatch=None):
    """A recorded pipeline scenario (tests/pipeline_cases.py) with the shared head on (the default) against the same job with it off -- or, with
    `issue_plans`, the shared head under the native issue plans against the walked forward.  Returns the differences; the caller asserts."""
    import pipeline_cases as PC
    if issue_plans:
        res1, pipe1 = PC.run_pipeline_case(name, device, return_pipe=True)
        monkeypatch.setenv("FZ_ISSUE_PLANS", "1")
        res0, pipe0 = PC.run_pipeline_case(name, device, return_pipe=True)
        monkeypatch.delenv("FZ_ISSUE_PLANS")
    else:
        res1, pipe1 = with_switch(True, lambda: PC.run_pipeline_case(name, device, return_pipe=True))
        res0, pipe0 = with_switch(False, lambda: PC.run_pipeline_case(name, device, return_pipe=True))
    PC.check(res1)
    a, b = pipe1.last_edited_latents, pipe0.last_edited_latents
    out = {"edit_max_diff": float((a - b).abs().max()), "edit_scale": float(b.abs().max()), "edit_equal": bool(torch.equal(a, b)),
           "edit_q99_diff": float(torch.quantile((a - b).abs().flatten(), 0.99))}
    m1, m0 = _edit_maps(pipe1), _edit_maps(pipe0)
    assert [k for k, _ in m1] == [k for k, _ in m0] and [m.shape for _, m in m1] == [m.shape for _, m in m0]
    out["maps"] = len(m1)
    diff = {}
    for (k, x), (_, y) in zip(m1, m0):
        kind = ("inv" if k.startswith("inv/") else "edit") + ("_cross" if k.endswith("cross") else "_self")
        diff[kind] = max(diff.get(kind, 0.0), float((x.float() - y.float()).abs().max()))
    out["map_diffs"] = diff
    out["map_max_diff"] = max(list(diff.values()) or [0.0])
    c1, c0 = pipe1.last_edit_controller, pipe0.last_edit_controller
    if getattr(c1, "attention_blend", None) is not None:
        out["attn_mask_flips"], out["attn_mask_total"] = PC._mask_flips(c1.attention_blend.mask_list, c0.attention_blend.mask_list)
    out["stats"] = None if not issue_plans else dict(pipe0.unet._issuer.stats)
    return out


# max |on - off| allowed on the GPU, where the 8- and 16-frame launches of one op may take different tiles / split-K factors: what the existing
# full-width forward case allows between the GPU and the fp32 oracle (tests/test_pipeline_gpu.py on pipeline_cases.run_fullwidth_forward)
ON_OFF_MAX_TOL = 1.5e-2
ON_OFF_Q99_TOL = 4e-3


def check_on_off(a, b):
    """a (shared head) against b (expanded input / switch off): the figures, asserted against ON_OFF_*_TOL of b's scale."""
    d = (a.float() - b.float()).abs().flatten()
    sc = float(b.float().abs().max())
    r = {"max_diff": float(d.max()), "q99_diff": float(torch.quantile(d[:: max(1, d.numel() // 1000000)], 0.99)), "scale": sc,
         "equal": bool(torch.equal(a, b))}
    print(r)
    assert r["max_diff"] <= ON_OFF_MAX_TOL * sc and r["q99_diff"] <= ON_OFF_Q99_TOL * sc, r
    return r
