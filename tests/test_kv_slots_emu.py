"""SparseCausalAttention_index lists of five to eight entries (FZ_MAX_KV_SLOTS = 8) WITHOUT a GPU, on the CPU emulation of the kernels (test
infrastructure): both attention kernels under five, six and eight slots, the launcher's dispatch order, the 8-bit maps, the frame-sharded kernel
form, the named limit, and the host layers that multiply by the list's length (issue plans, frame sharding, the YAML driver).  The MI355X versions
-- and the whole jobs against the fp32 oracle -- live in tests/test_kv_slots_gpu.py."""
import ctypes as C
import os

import pytest
import torch

from fatezero_amd import _native, build
from fatezero_amd import kernels as K

import kv_slots_cases as KS
import pipeline_cases as PC

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(build.build_emu())
    yield
    _native.reset_backend()


# ---------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,fold", KS.FLASH_HEAD_DIMS)
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_flash_five_and_eight_slots(name, d, fold):
    KS.flash_case(DEV, KS.LISTS[name], d, fold)


def test_flash_two_query_blocks_six_slots_moving_max():
    KS.flash_two_query_blocks(DEV)


def test_flash_eight_slots_on_one_source():
    KS.flash_all_slots_one_source(DEV)


def test_flash_dispatch_order_mixed_frames_five_slots():
    KS.flash_mixed_dispatch_order(DEV)


@pytest.mark.parametrize("d,lq", KS.CAPTURE_SHAPES)
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_capture_five_and_eight_slots(name, d, lq):
    KS.capture_case(DEV, KS.LISTS[name], d, lq)


@pytest.mark.parametrize("mask_kind", KS.MASK_KINDS)
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_inject_five_and_eight_slots(name, mask_kind):
    KS.inject_case(DEV, KS.LISTS[name], mask_kind)


@pytest.mark.parametrize("fmt", list(KS.MAP8_FORMATS))
@pytest.mark.parametrize("shape", list(KS.MAP8_SHAPES))
def test_8bit_maps_eight_slots(shape, fmt):
    KS.check_map8(KS.map8_case(shape, fmt, DEV))


def test_frame_sharded_kernel_form_six_slots():
    KS.sharded_six_slots(DEV)


def test_nine_entries_are_refused_by_name():
    KS.check_limits(DEV)


def test_entry_point_refuses_nine_slots_and_writes_nothing():
    """A hand-filled descriptor with n_kv = 9: FZ_ERR_BAD_ARG before any launch, the output keeps its sentinel.  (n_kv = 8 in the same
    descriptor runs.)"""
    heads, d, lq, clip = 2, 16, 64, 2
    c = heads * d
    g = torch.Generator().manual_seed(0)
    q, k, v = (KS.KC._mk((clip, lq, c), g, DEV) for _ in range(3))
    vt = K.transpose_pad(v, 64)
    o = torch.full((clip, lq, c), 77.0, dtype=torch.float16)
    desc = _native.FzAttnSelfDesc()
    desc.n_frames, desc.frame0, desc.clip_len, desc.heads, desc.head_dim, desc.lq, desc.lkf = clip, 0, clip, heads, d, lq, lq
    desc.scale, desc.mode = d ** -0.5, K.FZ_ATTN_FLASH
    desc.q_frame_stride, desc.q_row_stride = q.stride(0), q.stride(1)
    desc.k_frame_stride, desc.k_row_stride = k.stride(0), k.stride(1)
    desc.vt_frame_stride, desc.vt_chan_stride = vt.stride(0), vt.stride(1)
    desc.o_frame_stride, desc.o_row_stride = o.stride(0), o.stride(1)
    assert len(desc.kv_abs) == len(desc.kv_val) == 8
    for j in range(8):
        desc.kv_abs[j], desc.kv_val[j] = 0, j - 4
    ptr = lambda t: C.c_void_p(t.data_ptr())
    call = lambda: _native.lib().fz_attn_self(C.byref(desc), ptr(q), ptr(k), ptr(vt), ptr(o), None, None, None)
    for bad in (9, 0, -1, 1 << 20):
        desc.n_kv = bad
        assert call() == _native.FZ_ERR_BAD_ARG, bad
        assert (o == 77.0).all()
    desc.n_kv = 8
    assert call() == 0 and torch.isfinite(o.float()).all() and not (o == 77.0).all()


# ---------------------------------------------------------------------------------------------------------------
# pipeline level (what the issue asks of the emulator; the oracle comparisons run on MI355X)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.slow   # ~1.5 minutes of emulation per list
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_blend_threshold_splits_the_rows(name):
    """The whole-job case of tests/test_kv_slots_gpu.py, its capture inversion on the emulator: KS.BLEND_TH puts 20-80 % of the attention-blend
    masks of the self window on either side, i.e. the inject launches of that job run under a row mask that splits the rows."""
    frac = KS.blend_mask_fractions(DEV, name)[KS.BLEND_TH]
    print("kv slots", name, "mask ones fraction at th", KS.BLEND_TH, frac)
    lo, hi = PC.FULL_MASK_BAND
    assert lo <= frac <= hi, frac


def test_frame_sharded_job_five_slots_two_ranks():
    """13: 5 frames over two gloo ranks (ragged 3 + 2) with L5 -- halos of two frames on both sides and the 'first' anchor -- against the
    single process, with the harness and the bound of tests/test_dist_gloo.py."""
    import test_dist_gloo as TG
    got, n_maps, n_local, stats = TG._spawn(2, 5, KS.L5, True)
    TG._check_exchange_structure(stats)
    _, job = TG._frame_job_factory(5, KS.L5)
    ref = job()
    _native.use_test_backend(build.build_emu())  # (the factory pointed the backend at the same library)
    assert n_maps and all(n == n_local for n in n_maps), (n_maps, n_local)
    err, scale = float((got.float() - ref.float()).abs().max()), float(ref.float().abs().max())
    assert torch.isfinite(got.float()).all() and err <= 1.5e-2 * scale, (err, scale)


def _set_index_list(unet, index_list):
    from fatezero_amd.video_diffusion.models.attention import SpatioTemporalTransformerBlock
    for m in unet.modules():
        if isinstance(m, SpatioTemporalTransformerBlock):
            m.model_config["SparseCausalAttention_index"] = list(index_list)


def test_issue_plans_eight_slots_and_a_switch_of_the_list():
    """14: a forward under L8 is recorded and replayed, bit-identical to the walked forward; a model that switches from a two-entry list to the
    eight-entry one records a plan of its own instead of replaying the two-slot launch list."""
    g = torch.Generator().manual_seed(2)
    z = torch.randn(1, 4, 3, 16, 16, generator=g).half()
    ctx = torch.randn(1, 77, 64, generator=g).half()
    ref8 = PC.build_unet("tiny16", KS.model_config(KS.L8), DEV)
    want8 = ref8(z, 7, ctx).sample
    unet = PC.build_unet("tiny16", KS.model_config(KS.L8), DEV)
    unet.enable_issue_plans()
    ys = [unet(z, 7, ctx).sample for _ in range(3)]  # walked, recorded, replayed
    st = unet._issuer.stats
    assert st["walked"] == 1 and st["recorded"] == 1 and st["replayed"] == 1 and not st["unrecordable"] and not st["unsupported"], st
    assert all(torch.equal(y, want8) for y in ys)
    # the switch: the same weights under [-1, 'first'], then under L8
    ref2 = PC.build_unet("tiny16", KS.model_config([-1, "first"]), DEV)
    want2 = ref2(z, 7, ctx).sample
    assert not torch.equal(want2, want8)
    sw = PC.build_unet("tiny16", KS.model_config([-1, "first"]), DEV)
    sw.enable_issue_plans()
    y2 = [sw(z, 7, ctx).sample for _ in range(3)][-1]
    assert sw._issuer.stats["replayed"] == 1 and len(sw._issuer.plans) == 1 and torch.equal(y2, want2)
    _set_index_list(sw, KS.L8)
    y8 = [sw(z, 7, ctx).sample for _ in range(3)][-1]
    st = sw._issuer.stats
    assert st["walked"] == 2 and st["recorded"] == 2 and st["replayed"] == 2 and len(sw._issuer.plans) == 2, st
    assert torch.equal(y8, want8)
    _set_index_list(sw, [-1, "first"])
    assert torch.equal(sw(z, 7, ctx).sample, want2) and st["replayed"] == 3  # the first plan is still there, and still the two-slot one


YAML_LIST6 = "['first', -2, -1, 1, 2, 'last']"
YAML_LIST9 = "['first', -4, -3, -2, -1, 1, 2, 3, 'last']"


def _yaml_job(tmp_path, index_yaml):
    import dataset_cases as DC
    import test_cli_emu as TC
    ckpt, frames = str(tmp_path / "ckpt"), str(tmp_path / "frames")
    TC.synthetic_checkpoint(ckpt)
    DC.write_frames(frames, n=3, h=40, w=48)
    text = TC.YAML.format(ckpt=ckpt, frames=frames)
    assert "SparseCausalAttention_index: ['mid']" in text and "n_sample_frame: 2" in text
    text = text.replace("SparseCausalAttention_index: ['mid']", "SparseCausalAttention_index: " + index_yaml).replace("n_sample_frame: 2",
                                                                                                                   "n_sample_frame: 3")
    cfg_path = str(tmp_path / "config" / "job.yaml")
    os.makedirs(os.path.dirname(cfg_path))
    open(cfg_path, "w").write(text)
    return cfg_path, ckpt


def test_yaml_with_six_entries_runs_and_nine_are_refused_before_the_checkpoint(tmp_path):
    """15: through config_driver.load_config and test_fatezero.test."""
    import test_fatezero
    from fatezero_amd import config_driver
    cfg_path, _ = _yaml_job(tmp_path / "six", YAML_LIST6)
    cfg = config_driver.load_config(cfg_path)
    assert cfg["model_config"]["SparseCausalAttention_index"] == ["first", -2, -1, 1, 2, "last"]
    out = test_fatezero.test(config=cfg_path, device="cpu", **cfg)
    assert len(out["latents_all_step"]) == 4 and out["latents_all_step"][-1].shape == (1, 4, 3, 16, 16)
    assert all(torch.isfinite(x.float()).all() for x in out["latents_all_step"]) and len(out["samples"]) == 3
    assert os.path.exists(os.path.join(out["logdir"], "sample", "step_0_1_0.gif"))
    # nine entries: named, and before a checkpoint file is opened -- the checkpoint folder of this job is EMPTY
    cfg_path, ckpt = _yaml_job(tmp_path / "nine", YAML_LIST9)
    import shutil
    shutil.rmtree(ckpt)
    os.makedirs(ckpt)
    cfg = config_driver.load_config(cfg_path)
    with pytest.raises(ValueError) as e:
        test_fatezero.test(config=cfg_path, device="cpu", **cfg)
    assert "FZ_MAX_KV_SLOTS" in str(e.value) and "8" in str(e.value) and "'last'" in str(e.value)
    # ... and where the model is built, whoever builds it
    with pytest.raises(ValueError, match="FZ_MAX_KV_SLOTS"):
        PC.build_unet("tiny16", cfg["model_config"], "cpu")
