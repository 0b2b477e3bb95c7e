"""Run a FateZero YAML config (reference: test_fatezero.py:196-262 + P2pSampleLogger.log_sample_images,
video_diffusion/pipelines/p2p_validation_loop.py:68-128) on the MI355X pipeline, in latent space.

The reference drives one job as: encode `dataset_config.prompt`, DDIM-invert the clip while capturing attention
(`editing_config.use_invertion_latents` / `use_inversion_attention`), then call the pipeline once per entry of
`editing_config.editing_prompts` with `p2p_config[idx]` merged into the keyword arguments.  This module reproduces that
control flow without OmegaConf, accelerate, the dataset or the sample logger: images / VAE are optional,
clean latents can be handed in directly, and every edit returns latents unless the pipeline has a VAE.
"""
import copy
import re
from typing import Any, Dict, List, Optional

import torch

_INTERP = re.compile(r"\$\{(\.*)([^}]+)\}")


class Config(dict):
    """A loaded YAML config: a plain dict plus `.unresolved`, the dotted paths whose `${...}` interpolation points at a node
    that does not exist.  OmegaConf resolves lazily, so such a node only fails when it is READ -- and 24 of the reference's
    27 configs carry one that nothing reads (`test_pipeline_config.num_inference_steps:
    "${..validation_sample_logger.num_inference_steps}"`, e.g. config/teaser/jeep_posche.yaml:86).  They are kept as the raw
    string here instead of failing the load."""
    unresolved: List[str]


class _Unresolvable(KeyError):
    pass


def _lookup(root, path_keys):
    node = root
    for key in path_keys:
        if isinstance(node, list):
            try:
                node = node[int(key)]
            except (ValueError, IndexError):
                raise _Unresolvable(f"no list element {key!r} on the way to {'.'.join(map(str, path_keys))}")
        elif isinstance(node, dict):
            if key in node:
                node = node[key]
            elif isinstance(key, str) and key.lstrip("-").isdigit() and int(key) in node:
                node = node[int(key)]  # YAML maps with integer keys (p2p_config: {0: ..., 1: ...})
            else:
                raise _Unresolvable(f"no key {key!r} on the way to {'.'.join(map(str, path_keys))}")
        else:
            raise _Unresolvable(f"{'.'.join(map(str, path_keys))} descends into a scalar")
    return node


def _resolve(root, node, trail, unresolved, depth=0):
    """OmegaConf's interpolation subset used by the shipped configs: "${a.b}" from the root, "${.a}" relative to the
    mapping that holds the value, each further dot one level up ("${..dataset_config.n_sample_frame}")."""
    if depth > 32:
        raise ValueError(f"interpolation cycle at {'.'.join(map(str, trail))}")
    if isinstance(node, dict):
        return {k: _resolve(root, v, trail + [k], unresolved, depth) for k, v in node.items()}
    if isinstance(node, list):
        return [_resolve(root, v, trail + [i], unresolved, depth) for i, v in enumerate(node)]
    if not isinstance(node, str):
        return node

    def value_of(match):
        dots, dotted = match.group(1), match.group(2).split(".")
        if not dots:
            base = []
        else:
            up = len(dots)  # one dot = the mapping that holds this key
            if up > len(trail):
                raise _Unresolvable(f"interpolation {match.group(0)!r} climbs above the root")
            base = trail[:len(trail) - up]
        return _resolve(root, _lookup(root, base + dotted), base + dotted, unresolved, depth + 1)

    try:
        whole = _INTERP.fullmatch(node)
        if whole:  # the value IS the interpolation: keep the referenced type (int, list, ...)
            return value_of(whole)
        return _INTERP.sub(lambda m: str(value_of(m)), node)
    except _Unresolvable:
        unresolved.append(".".join(map(str, trail)))
        return node


def load_config(path: str) -> Config:
    import yaml
    with open(path, "r") as f:
        raw = yaml.safe_load(f)
    unresolved: List[str] = []
    cfg = Config(_resolve(raw, raw, [], unresolved))
    cfg.unresolved = unresolved
    return cfg


MAP_DTYPES = ("fp16", "e5m2", "ue4m4")


def map_dtype_of(editing_config: Optional[Dict[str, Any]], override: Optional[str] = None) -> str:
    """Storage of the captured self-attention maps: `override` (the --map-dtype switch), else the optional
    `editing_config.attention_map_dtype` key (an extension: no reference config has it), else "fp16"."""
    value = override if override is not None else (editing_config or {}).get("attention_map_dtype", "fp16")
    if value not in MAP_DTYPES:
        raise ValueError("attention_map_dtype must be one of %s, got %r" % (", ".join(repr(m) for m in MAP_DTYPES), value))
    return value


def recompute_maps_of(editing_config: Optional[Dict[str, Any]], override: Optional[bool] = None) -> bool:
    """The pipeline's `recompute_maps` mode: `override` (the --recompute-maps switch), else the optional
    `editing_config.recompute_attention_maps` key (an extension: no reference config has it), else off.  The mode re-runs inversion
    forwards, so it needs `use_inversion_attention: True`."""
    value = override if override is not None else (editing_config or {}).get("recompute_attention_maps", False)
    if not isinstance(value, bool):
        raise ValueError("recompute_attention_maps must be true or false, got %r" % (value,))
    if value and editing_config is not None and not editing_config.get("use_inversion_attention", False):
        raise ValueError("recompute_attention_maps: true needs use_inversion_attention: true (with use_inversion_attention: false the stored "
                         "maps come from an edit pass, there is no inversion forward to recompute them from)")
    return value


def temporal_window_of(model_config: Optional[Dict[str, Any]], override: Optional[int] = None) -> Optional[int]:
    """Temporal attention's window: `override` (the --temporal-window switch), else the optional `model_config.temporal_attention_window`
    key (an extension: no reference config has it), else None -- every frame of the clip.  W: a query frame attends the frames within W
    of it.  A value that is neither None nor a non-negative int is a ValueError."""
    from . import kernels
    value = override if override is not None else (model_config or {}).get("temporal_attention_window")
    kernels.check_temporal_window(value)
    return value


def image_size_of(dataset_config: Optional[Dict[str, Any]]):
    """`dataset_config.image_size`: an int (square frames, the reference's form) or a `[height, width]` pair (an extension: a clip edited at
    its own aspect ratio).  Returns the int, or the pair as a tuple of ints; 512 when the key is absent (the dataset's default)."""
    value = (dataset_config or {}).get("image_size", 512)
    if isinstance(value, bool):
        raise ValueError("image_size must be an int or a [height, width] pair, got %r" % (value,))
    if isinstance(value, int):
        return value
    if isinstance(value, (list, tuple)) and len(value) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in value):
        return int(value[0]), int(value[1])
    raise ValueError("image_size must be an int or a [height, width] pair, got %r" % (value,))


def plan_edits(editing_config: Dict[str, Any], source_prompt: Optional[str]) -> List[Dict[str, Any]]:
    """One dict of pipeline keyword arguments per (editing prompt, seed), in the order the reference runs them."""
    prompts = list(editing_config["editing_prompts"])
    p2p = editing_config.get("p2p_config")
    use_inv_attn = bool(editing_config.get("use_inversion_attention", False))
    p2p_edit = bool(editing_config.get("prompt2prompt_edit", False))
    calls = []
    for idx, prompt in enumerate(prompts):
        extra: Dict[str, Any] = {}
        edit_type = None
        if p2p_edit:
            extra = copy.deepcopy(p2p[idx] if not isinstance(p2p, dict) or idx in p2p else p2p[str(idx)])
            first_records = (idx == 0 and not use_inv_attn)  # without inversion attention the first prompt refreshes the store
            edit_type = "save" if first_records else "swap"
            extra["save_self_attention"] = first_records
            extra["use_inversion_attention"] = use_inv_attn
        for seed in (editing_config.get("sample_seeds") or [0]):
            kw = dict(prompt=prompt, source_prompt=prompts[0] if source_prompt is None else source_prompt,
                      edit_type=edit_type, strength=editing_config.get("strength"),
                      num_inference_steps=editing_config.get("num_inference_steps", 20),
                      clip_length=editing_config.get("clip_length"), guidance_scale=editing_config.get("guidance_scale", 7.5),
                      num_images_per_prompt=1)
            kw.update(extra)
            calls.append({"prompt_index": idx, "seed": int(seed), "kwargs": kw})
    return calls


@torch.no_grad()
def run_config(pipe, config: Dict[str, Any], *, latents: Optional[torch.Tensor] = None, images: Optional[torch.Tensor] = None,
               device=None, output_type: str = "latent") -> Dict[str, Any]:
    """Inversion + every edit of `config`.  latents: clean latents [1, 4, F, h, w] (or pass `images` [(F), 3, H, W] and a
    pipeline with a VAE).  Returns {"inverted": [...], "edits": [{"prompt_index", "seed", "output"}]}."""
    device = device if device is not None else pipe._execution_device
    editing = config["editing_config"]
    source_prompt = config.get("dataset_config", {}).get("prompt")
    steps = editing.get("num_inference_steps", 20)
    pipe.scheduler.set_timesteps(steps)
    if hasattr(pipe, "set_map_dtype"):  # the key is optional: without it the format the pipeline was built with applies (again)
        pipe.set_map_dtype(map_dtype_of(editing) if "attention_map_dtype" in editing else pipe.default_map_dtype)
    if hasattr(pipe, "set_recompute_maps"):  # (likewise: without the key, the mode the pipeline was built with)
        pipe.set_recompute_maps(recompute_maps_of(editing) if "recompute_attention_maps" in editing else pipe.default_recompute_maps)
    init = None
    inverted = None
    if editing.get("use_invertion_latents", False):  # (sic) the reference's spelling
        emb = pipe._encode_prompt(source_prompt, device, 1, True, None)
        inverted = pipe.prepare_latents_ddim_inverted(images, batch_size=1, num_images_per_prompt=1, text_embeddings=emb,
                                                      prompt=source_prompt, LOW_RESOURCE=True, latents=latents,
                                                      store_attention=bool(editing.get("use_inversion_attention", False)))
        init = inverted[-1]
    results = []
    for call in plan_edits(editing, source_prompt):
        kw = dict(call["kwargs"])
        gen = torch.Generator(device="cpu").manual_seed(call["seed"])
        out = pipe(image=images, latents=init, generator=gen, output_type=output_type, **kw)
        results.append({"prompt_index": call["prompt_index"], "seed": call["seed"], "output": out})
    return {"inverted": inverted, "edits": results}
