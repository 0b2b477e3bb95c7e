"""`recompute_maps` under a frame shard (fatezero_amd.dist.FrameShard, 2 gloo ranks on the CPU emulation, the harness of
tests/test_map8u_emu.py): every rank recomputes its own frames through the sharded forward the inversion uses.  The sharded recomputed job
is bit-identical to the sharded resident job, and equals the single-process recomputed job within the tolerance of the sharded jobs."""
import os
import sys

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _job(frames, recompute, shard=None):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fatezero_amd import _native as N, build as B
    N.use_test_backend(B.build_emu())
    import pipeline_cases as PC
    from fatezero_amd.synthetic import WordTokenizer
    from fatezero_amd.video_diffusion.pipelines.p2p_ddim_spatial_temporal import P2pDDIMSpatioTemporalPipeline
    from fatezero_amd.video_diffusion.schedulers import DDIMScheduler
    unet = PC.build_unet("tiny16", {"lora": 16, "SparseCausalAttention_index": [-1, "first"]}, "cpu")
    pipe = P2pDDIMSpatioTemporalPipeline(vae=None, text_encoder=None, tokenizer=WordTokenizer(), unet=unet, scheduler=DDIMScheduler(),
                                         recompute_maps=recompute)
    pipe.frame_shard = shard
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(2, 77, 64, generator=g)
    pipe._encode_prompt = lambda *a, **k: emb
    z0 = torch.randn(1, 4, frames, 8, 8, generator=g)
    pipe.scheduler.set_timesteps(3)
    lat = pipe.prepare_latents_ddim_inverted(image=None, batch_size=1, num_images_per_prompt=1, text_embeddings=emb, store_attention=True,
                                             LOW_RESOURCE=True, latents=z0)
    out = pipe(prompt="a red car", source_prompt="a blue car", edit_type="swap", num_inference_steps=3, latents=lat[-1],
               output_type="latent", cross_replace_steps={"default_": 0.5}, self_replace_steps=0.5, use_inversion_attention=True,
               is_replace_controller=True, save_self_attention=False, guidance_scale=3.0)
    store = pipe.store_controller
    frames_held = {cm.storage.shape[0] for v in store.maps_of_step(0).values() for cm in v}
    return torch.stack([lat[-1], out["sdimage_output"].images]), store.arena_bytes, frames_held


def _worker(rank, world, port, frames, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      FZ_EMU_THREADS="2")
    torch.set_num_threads(2)
    sys.path.insert(0, ROOT)
    from fatezero_amd import dist as D
    import torch.distributed as dist
    D.init("gloo")
    shard = D.FrameShard(frames)
    rec, rec_bytes, rec_frames = _job(frames, True, shard)
    res, res_bytes, _ = _job(frames, False, shard)
    if rank == 0:
        q.put((rec.clone(), res.clone(), rec_bytes, res_bytes, sorted(rec_frames), shard.n_local))
    dist.barrier()
    dist.destroy_process_group()


def test_frame_sharded_recompute_job():
    frames, world = 4, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, world, port, frames, q)) for r in range(world)]
    for p in procs:
        p.start()
    rec, res, rec_bytes, res_bytes, rec_frames, n_local = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    for k in ("WORLD_SIZE", "RANK"):
        os.environ.pop(k, None)
    assert torch.isfinite(rec.float()).all()
    assert torch.equal(rec, res), float((rec.float() - res.float()).abs().max())  # sharded: recomputed == resident, bit for bit
    assert rec_bytes * 3 == res_bytes and rec_frames == [n_local] and n_local == frames // world  # one step, this rank's frames only
    single, _, _ = _job(frames, True)
    from fatezero_amd import _native
    _native.reset_backend()
    err, scale = float((rec.float() - single.float()).abs().max()), float(single.float().abs().max())
    assert err <= 1.5e-2 * scale, (err, scale)  # the tolerance of the sharded jobs against one process (tests/test_dist_gloo.py)
