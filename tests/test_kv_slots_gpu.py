"""SparseCausalAttention_index lists of five to eight entries (FZ_MAX_KV_SLOTS = 8) on the MI355X: the kernel cases of
tests/test_kv_slots_emu.py through the C ABI of libfatezero_hip.so, whole 6-frame jobs against the fp32 oracle (run live, executed by torch on
the GPU), and the same jobs in every storage mode against their plain resident fp16 twin."""
import pytest
import torch

from fatezero_amd import _native

import cfg_shared_cases as CS
import kv_slots_cases as KS
import recompute_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,fold", KS.FLASH_HEAD_DIMS)
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_flash_five_and_eight_slots(name, d, fold):
    print(KS.flash_case(DEV, KS.LISTS[name], d, fold))
    assert _native.loaded_path().endswith("libfatezero_hip.so")


def test_flash_two_query_blocks_six_slots_moving_max():
    print(KS.flash_two_query_blocks(DEV))


def test_flash_eight_slots_on_one_source():
    print(KS.flash_all_slots_one_source(DEV))


def test_flash_dispatch_order_mixed_frames_five_slots():
    print(KS.flash_mixed_dispatch_order(DEV))


@pytest.mark.parametrize("d,lq", KS.CAPTURE_SHAPES)
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_capture_five_and_eight_slots(name, d, lq):
    print(KS.capture_case(DEV, KS.LISTS[name], d, lq))


@pytest.mark.parametrize("mask_kind", KS.MASK_KINDS)
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_inject_five_and_eight_slots(name, mask_kind):
    print(KS.inject_case(DEV, KS.LISTS[name], mask_kind))


@pytest.mark.parametrize("fmt", list(KS.MAP8_FORMATS))
@pytest.mark.parametrize("shape", list(KS.MAP8_SHAPES))
def test_8bit_maps_eight_slots(shape, fmt):
    KS.check_map8(KS.map8_case(shape, fmt, DEV))


def test_frame_sharded_kernel_form_six_slots():
    KS.sharded_six_slots(DEV)


def test_nine_entries_are_refused_by_name():
    KS.check_limits(DEV)


# ---------------------------------------------------------------------------------------------------------------
# whole jobs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_whole_job_vs_fp32_oracle(name):
    """10 + 11: tiny16, 6 frames, 40^2 latents, T = 4 + 4: inversion with capture, Replace edit with blend-masked self-attention; the inversion
    latents, every stored self map (len(L) * lq columns) and the edit on identical maps against the oracle, at the constants of
    pipeline_cases.py (LATENT_TOL, SELF_MAP_TOL, no attention-mask flip) and, for the edit on identical maps, kv_slots_cases.KV_EDIT_TOL_SAME_MAPS
    (EDIT_TOL_SAME_MAPS does not hold at this geometry, whatever the list: the figures stand there); the mask splits the rows."""
    res, shapes = KS.whole_job(DEV, name, oracle_device=DEV)
    KS.check_whole_job(res, shapes, KS.LISTS[name])
    assert _native.loaded_path().endswith("libfatezero_hip.so")


@pytest.mark.parametrize("name", list(KS.LISTS))
def test_recomputed_job_is_bit_identical(name):
    """recompute_maps=True under the row mask (40^2 latents): the one-step slab holds len(L) * lq columns per map."""
    rec, res = KS.job(DEV, name, L=KS.BLEND_L, recompute=True), KS.job(DEV, name, L=KS.BLEND_L)
    RC.assert_split(res)
    RC.assert_same_edit(rec, res, name)
    RC.assert_arena_is_one_step(rec, res, slabs=1)


@pytest.mark.parametrize("name", list(KS.LISTS))
def test_spilled_job_is_bit_identical(name, monkeypatch):
    """disk_store=True with no HBM budget: every step behind the first goes to the host tier and comes back for the edit (a staging ring of two
    slabs, so that the four steps of this job do not all stay in it)."""
    from fatezero_amd.video_diffusion.prompt_attention import attention_store as AS
    monkeypatch.setattr(AS, "SPILL_RING", 2)
    monkeypatch.setenv("FZ_ARENA_HBM_GB", "0")
    sp = KS.job(DEV, name, disk_store=True)
    monkeypatch.delenv("FZ_ARENA_HBM_GB")
    res = KS.job(DEV, name)
    arena = sp["pipe"].store_controller.arena
    assert arena.spilled and arena.spilled_bytes > 0 and arena.fetch_stats["h2d"] >= 1, (sorted(arena.spilled), arena.fetch_stats)
    RC.assert_same_edit(sp, res, name)


@pytest.mark.parametrize("fmt", ["e5m2", "ue4m4"])
@pytest.mark.parametrize("name", list(KS.LISTS))
def test_8bit_arena_job(name, fmt):
    """map_dtype: the inversion latents do not see the format, the stored bytes are the fp16 job's maps rounded, the arena is half the size;
    the edit reads the rounded maps: finite, its deviation from the fp16-arena job is printed."""
    r8, r16 = KS.job(DEV, name, map_dtype=fmt), KS.job(DEV, name)
    for a, b in zip(r8["inverted"], r16["inverted"]):
        assert torch.equal(a, b)
    s8, s16 = r8["pipe"].store_controller, r16["pipe"].store_controller
    encode = KS.MAP8_FORMATS[fmt][2]
    n = 0
    for key in ("down_self", "mid_self", "up_self"):
        for c8, c16 in zip(s8.maps_of_step(-1)[key], s16.maps_of_step(-1)[key]):
            assert c8.fmt == fmt and c8.storage.dtype == torch.uint8 and c8.storage.shape[-1] == len(KS.LISTS[name]) * c8.storage.shape[-2]
            assert torch.equal(c8.storage.cpu(), encode(c16.storage.cpu()))
            n += 1
    assert n > 0 and s8.arena_bytes < s16.arena_bytes
    e8, e16 = r8["edits"]["replace"]["latents"], r16["edits"]["replace"]["latents"]
    assert torch.isfinite(e8).all()
    print("kv slots", name, fmt, "edit vs the fp16 arena:", float((e8 - e16).abs().max()) / float(e16.abs().max()))


@pytest.mark.parametrize("name", list(KS.LISTS))
def test_cfg_shared_head_on_vs_off(name):
    """Same stored maps and inversion; the edited latents within the on / off bound of tests/cfg_shared_cases.py."""
    on, off = KS.job(DEV, name), KS.job(DEV, name, shared_head=False)
    for a, b in zip(on["inverted"], off["inverted"]):
        assert torch.equal(a, b)
    print("kv slots", name, "shared head on vs off:", CS.check_on_off(on["edits"]["replace"]["latents"], off["edits"]["replace"]["latents"]))
