"""`recompute_maps` on the MI355X: the tiny job of tests/test_map8_gpu.py (tiny40 width, 4 frames, 64^2 latents, T = 4 + 4, Replace +
blend-masked self-attention) recomputed against resident, bit for bit, in fp16 and in the 8-bit formats, every variation of
tests/test_recompute_maps_emu.py as a job of its own, and fz_latent_tokens through the C ABI of libfatezero_hip.so."""
import pytest
import torch

import recompute_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TH = R.PC.GEOMETRY_SPLIT_TH["tiny40"]  # the threshold that splits the rows at this geometry (asserted below)


def _pair(**kw):
    return R.job(DEV, "gpu", True, **kw), R.job(DEV, "gpu", False, **kw)


@pytest.mark.parametrize("map_dtype", ["fp16", "e5m2", "ue4m4"])
def test_recomputed_job_is_bit_identical_to_the_resident_run(map_dtype):
    rec, res = _pair(map_dtype=map_dtype, blend_th=TH, blend_latents=False)
    R.assert_split(res)
    R.assert_same_edit(rec, res, map_dtype)
    R.assert_arena_is_one_step(rec, res, slabs=1)
    cms = rec["pipe"].store_controller.maps_of_step(0)["down_self"]
    assert cms and all(cm.fmt == map_dtype for cm in cms)


VARIATIONS = {
    "latent_blend_own_self_store": dict(blend_th=TH, blend_latents=True, save_self_attention=True),
    "refine_reweight": dict(edits=("refine_reweight",), blend_th=TH, blend_latents=True),
    "two_prompts": dict(edits=("replace", "refine_reweight"), blend_th=TH, blend_latents=False),
    "unshared_head": dict(blend_th=TH, blend_latents=False, shared_head=False),
    "fp16_latent_store": dict(blend_th=TH, blend_latents=False, z_dtype=torch.float16),
    "disk_store_spills_nothing": dict(blend_th=TH, blend_latents=False, disk_store=True),
}


@pytest.mark.parametrize("name", list(VARIATIONS))
def test_variation_is_bit_identical_to_its_resident_twin(name):
    kw = VARIATIONS[name]
    if name == "disk_store_spills_nothing":
        rec, res = R.job(DEV, "gpu", True, **kw), R.job(DEV, "gpu", False, **dict(kw, disk_store=False))
        assert not rec["pipe"].store_controller.arena.spilled and rec["pipe"].store_controller.arena.spilled_bytes == 0
    else:
        rec, res = _pair(**kw)
    R.assert_same_edit(rec, res, name)
    R.assert_arena_is_one_step(rec, res)
    if "latent_blend" in name:
        assert len(res["edits"]["replace"]["applied_masks"]) > 0


def test_issue_plans_are_refused_by_name(monkeypatch):
    """recompute_maps under FZ_ISSUE_PLANS=1 is refused (tests/test_recompute_maps_emu.py says why), before anything is launched."""
    monkeypatch.setenv("FZ_ISSUE_PLANS", "1")
    with pytest.raises(RuntimeError, match="recompute_maps") as e:
        R.run_job(DEV, R.GPU, recompute=True, blend_th=TH, blend_latents=False)
    assert "FZ_ISSUE_PLANS" in str(e.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("frames,hw", R.LATENT_TOKEN_SHAPES)
def test_latent_tokens_equals_permute_and_cast(frames, hw, dtype):
    R.check_latent_tokens(DEV, frames, hw, dtype)


def test_latent_tokens_bad_arguments():
    R.check_latent_tokens_bad_args(DEV)


def test_latent_tokens_beyond_2_31_elements():
    """4 * F * hw = 2^31 + 120 latent elements (F = 2, hw = 2^28 + 15; fp16 in: 4.3 GB in, 4.3 GB out): a 32-bit flat index would wrap in the
    last channel plane and in the last tokens.  Zeros with a few sentinels; the ends of the output and one plane boundary are compared."""
    from fatezero_amd import kernels as K
    frames, hw = 2, 2 ** 28 + 15
    z = torch.zeros(4, frames, hw, dtype=torch.float16, device=DEV)
    z[3, 1, -1], z[3, 1, 0], z[2, 1, -2], z[0, 0, 0], z[1, 0, 5] = 1.5, -2.5, 3.25, 0.75, -4.0
    out = K.latent_tokens(z)
    assert out.shape == (frames, hw, 4)
    assert out[1, -1].tolist() == [0.0, 0.0, 0.0, 1.5] and out[1, 0].tolist() == [0.0, 0.0, 0.0, -2.5]
    assert out[1, -2].tolist() == [0.0, 0.0, 3.25, 0.0] and out[0, 0].tolist() == [0.75, 0.0, 0.0, 0.0] and out[0, 5].tolist() == [0.0, -4.0, 0.0, 0.0]
    assert float(out.abs().sum(dtype=torch.float32)) ==1.5 + 2.5 + 3.25 + 0.75 + 4.0  # nothing landed anywhere else
