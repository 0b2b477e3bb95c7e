#!/usr/bin/env python3
"""Record the SD-2.x golden vectors (tests/golden/sd2_*) by running the UNMODIFIED reference on CPU.

TEST INFRASTRUCTURE, authoring machine only (the reference checkout does not travel with the tests).  It imports
oracle/gen_golden.py -- the refshim set-up, the procedural weights, the pipeline scenario -- without changing it, and runs the
same scenarios on SD-2-shaped tiny UNets: Linear proj_in / proj_out (use_linear_projection), a per-level head-count list, a
context width other than 768, and upcast_attention in one case.

    python scripts/gen_golden_sd2.py        # rewrites tests/golden/sd2_* byte-identically on the same torch build
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")

_spec = importlib.util.spec_from_file_location("_gen_golden", os.path.join(ROOT, "oracle", "gen_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
torch = G.torch
np = G.np

# SD-2.x-shaped tiny nets.  SD-2-base: use_linear_projection, heads (5, 10, 20, 20) = head dim 64 at every level, context 1024.
SD2_TINY = {
    # head dim 64 at every level, like SD-2
    "sd2_d64": dict(sample_size=64, block_out_channels=(64, 128, 128, 128), norm_num_groups=8, cross_attention_dim=96,
                    attention_head_dim=[1, 2, 2, 2], use_linear_projection=True),
    # a head list whose head dim changes with the level (32 / 64 / 32), upcast_attention on
    "sd2_mixed_upcast": dict(sample_size=64, block_out_channels=(64, 128, 128, 128), norm_num_groups=8, cross_attention_dim=96,
                             attention_head_dim=[2, 2, 4, 4], use_linear_projection=True, upcast_attention=True),
}
CTX = 96


def build_sd2_unet(kind, model_config, seed=0):
    torch.manual_seed(0)
    unet = G.UNetPseudo3DConditionModel(**SD2_TINY[kind], **model_config)
    shapes = [(k, tuple(v.shape)) for k, v in unet.state_dict().items()]
    unet.load_state_dict(G.procedural_state_dict(shapes, seed))
    unet.eval().requires_grad_(False)
    return unet, shapes


def gen_unet():
    meta = {}
    for name, kind, mc, F_, L in [("sd2_unet_d64", "sd2_d64", {"lora": 16}, 3, 16),
                                  ("sd2_unet_mixed_upcast", "sd2_mixed_upcast", {"lora": 16}, 2, 16)]:
        unet, shapes = build_sd2_unet(kind, mc)
        assert unet.down_blocks[0].attentions[0].proj_in.weight.dim() == 2  # the reference built the Linear form
        g = torch.Generator().manual_seed(1234)
        x = torch.randn(2, 4, F_, L, L, generator=g)
        ctx = torch.randn(2, 77, CTX, generator=g)
        store = G.attention_util.AttentionStore()
        store.LOW_RESOURCE = True

        class _P:
            pass
        p = _P()
        p.unet = unet
        G.attention_util.register_attention_control(p, store)
        with torch.no_grad():
            t0 = time.time()
            y = unet(x, torch.tensor(481), encoder_hidden_states=ctx).sample
            dt = time.time() - t0
        G.save_npz(name + ".npz", x=x, ctx=ctx, y=y, t=np.int64(481))
        meta[name] = {"kind": kind, "arch": {k: v for k, v in SD2_TINY[kind].items() if k != "sample_size"}, "model_config": mc,
                      "F": F_, "L": L, "state_dict_shapes": shapes,
                      "map_shapes": {k: [list(m.shape) for m in v] for k, v in store.step_store.items()}}
        print(f"  {name}: {dt:.1f}s  |y|={float(y.abs().mean()):.4f}")
    with open(os.path.join(GOLD, "sd2_unet_meta.json"), "w") as f:
        json.dump(meta, f)


def gen_pipeline(tok):
    """oracle/gen_golden.py's `pipe_replace_blend` scenario (teaser prompts, Replace controller, attention blend, T = 4 + 4, F = 2,
    64^2 latents) on the sd2_d64 net with a 96-wide context, recorded into a scratch folder and renamed sd2_*."""
    tmp = tempfile.mkdtemp()
    saved = G.GOLD, G.build_ref_unet, G.torch.randn
    G.GOLD = tmp
    G.build_ref_unet = lambda kind, mc, seed=0: build_sd2_unet("sd2_d64", mc, seed)

    def randn(*shape, **kw):
        # The scenario's text embeddings, 96 wide instead of 64: only the [*, 77, 64] draws that gen_pipeline's OWN body makes are widened
        # (the caller's code object is checked), so no draw of the reference or of any helper is touched.
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        if sys._getframe(1).f_code is G.gen_pipeline.__code__ and len(shape) == 3 and shape[1:] == (77, 64):
            shape = (shape[0], 77, CTX)
        return saved[2](*shape, **kw)
    G.torch.randn = randn
    try:
        G.gen_pipeline(tok, only={"pipe_replace_blend"})
    finally:
        G.GOLD, G.build_ref_unet, G.torch.randn = saved
    shutil.copyfile(os.path.join(tmp, "pipe_replace_blend.npz"), os.path.join(GOLD, "sd2_pipe_replace_blend.npz"))
    meta = json.load(open(os.path.join(tmp, "pipeline_meta.json")))
    meta["pipe_replace_blend"]["sd2_kind"] = "sd2_d64"
    for k in ("seconds_inversion", "seconds_edit"):  # (timings would make the fixture differ run to run)
        meta["pipe_replace_blend"].pop(k)
    with open(os.path.join(GOLD, "sd2_pipeline_meta.json"), "w") as f:
        json.dump({"sd2_pipe_replace_blend": meta["pipe_replace_blend"]}, f)
    shutil.rmtree(tmp)
    print("  wrote sd2_pipe_replace_blend.npz, sd2_pipeline_meta.json")


def main():
    torch.set_grad_enabled(False)
    which = set(sys.argv[1:]) or {"unet", "pipeline"}
    if "unet" in which:
        print("[sd2 unet]"); gen_unet()
    if "pipeline" in which:
        print("[sd2 pipeline]"); gen_pipeline(G.RecordingTokenizer(G.load_bpe_tokenizer()))


if __name__ == "__main__":
    main()
