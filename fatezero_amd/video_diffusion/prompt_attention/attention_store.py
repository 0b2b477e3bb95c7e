"""Attention controllers, base + capture store (reference: video_diffusion/prompt_attention/attention_store.py).

Same public attributes and call protocol as the reference (`__call__(attn, is_cross, place_in_unet)`,
`step_callback`, `between_steps`, `step_store`, `attention_store`, `attention_store_all_step`, `latents_store`,
`LOW_RESOURCE`, `cur_step`, `cur_att_layer`, `num_att_layers`, `get_average_attention`, `reset`) but the maps are
never copied to the host: every captured probability map is written by the attention kernel itself, coalesced,
into an fp16 slab of HBM (`MapArena`), and `attention_store_all_step[step][key][i]` is a *view* of that slab with
the reference's shape [F, heads, Lq, Lk].  Cross maps are stored with a row stride of 80 halves (16-byte aligned
rows) and exposed as `[..., :77]` views.

Two entry points:
  * `attention_plan(...)`  -- what the fused kernels use (fatezero_amd/video_diffusion/models/attention.py);
  * `__call__(attn, ...)`   -- the reference's tensor protocol, kept for drop-in use with foreign attention code.
Differences, by design: the running sum `attention_store` (attention_store.py:95-101) is kept in fp32 and only for
cross maps unless `accumulate_self=True` (its self-attention entries have no live consumer in the reference);
`latents_store` stays on the device; `disk_store=True` spills the steps that do not fit the HBM budget to pinned host memory (MapArena)
instead of writing .pt files.

`map_dtype="e5m2"` (opt-in; the default "fp16" is the layout above) stores the SELF-attention maps at one byte per probability: the
attention kernel rounds each fp16 value to E5M2 -- the top byte of the half -- as it writes (FZ_ATTN_CAPTURE8) and the edit reads the bytes
back (FZ_ATTN_INJECT8).  Cross maps stay fp16.  Every reference-shaped reader (`attention_store_all_step`, `CapturedMap.view`, the running
sum with `accumulate_self`) sees fp16 tensors dequantised exactly from the bytes, built when they are read.
`map_dtype="ue4m4"` is the same arena with the byte holding bits 13..6 of the half instead of bits 15..8 (a probability never sets bits 15
and 14): 4 mantissa bits instead of 2 (FZ_ATTN_CAPTURE8U / FZ_ATTN_INJECT8U).  A uint8 slab does not say which format it holds: every
CapturedMap carries its format.
"""
import abc
import math
import os
from typing import Dict, List, Optional

import torch

from ... import kernels as K
from ..models.attention import AttnPlan

KEYS = ("down_cross", "mid_cross", "up_cross", "down_self", "mid_self", "up_self")
MAP_DTYPES = ("fp16", "e5m2", "ue4m4")  # storage of the captured self-attention maps
MAX_CONTROLLED_TOKENS = 32 ** 2  # attention_store.py:83, attention_util.py:104


def map_hw(lq: int, extent=None):
    """(h, w) of an attention level with `lq` query tokens (token y * w + x), given an extent (H, W) of the same aspect ratio (the latent
    size, or the size a mask is resized to): h = round(sqrt(lq * H / W)), w = lq // h, with h * w == lq and h * W == w * H required.
    `extent=None` (a controller nobody told the latent size): the reference's square, int(sqrt(lq)) on both sides."""
    if extent is None:
        h = int(math.sqrt(lq))
        return h, h
    H, W = int(extent[0]), int(extent[1])
    h = int(round(math.sqrt(lq * H / W))) if H > 0 and W > 0 else 0
    w = lq // h if h > 0 else 0
    if h <= 0 or h * w != lq or h * W != w * H:
        raise ValueError(f"an attention map of lq={lq} tokens is no (h, w) grid with the aspect ratio of (H, W)=({H}, {W})")
    return h, w


class AttentionControl(abc.ABC):
    def __init__(self):
        self.LOW_RESOURCE = False  # assume the edit has classifier-free guidance (attention_store.py:56)
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0

    # -- reference protocol ------------------------------------------------------------------------------
    def step_callback(self, x_t):
        self.cur_att_layer = 0
        self.cur_step += 1
        self.between_steps()
        return x_t

    def between_steps(self):
        return

    @property
    def num_uncond_att_layers(self):
        return 0

    @abc.abstractmethod
    def forward(self, attn, is_cross: bool, place_in_unet: str):
        raise NotImplementedError

    def __call__(self, attn, is_cross: bool, place_in_unet: str):
        if self.cur_att_layer >= self.num_uncond_att_layers:
            if self.LOW_RESOURCE:
                attn = self.forward(attn, is_cross, place_in_unet)
            else:
                h = attn.shape[0]
                attn[h // 2:] = self.forward(attn[h // 2:], is_cross, place_in_unet)
        self.cur_att_layer += 1
        return attn

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0

    # -- kernel protocol ---------------------------------------------------------------------------------
    def attention_plan(self, is_cross, place, n_frames, clip_len, heads, lq, lk, device) -> AttnPlan:
        n_plain = 0 if self.LOW_RESOURCE else n_frames // 2
        plan = self.plan_controlled(is_cross, place, n_frames - n_plain, clip_len, heads, lq, lk, device)
        plan.n_plain = n_plain
        self.cur_att_layer += 1
        return plan

    def plan_controlled(self, is_cross, place, n_ctrl, clip_len, heads, lq, lk, device) -> AttnPlan:
        return AttnPlan(0)

    def issue_signature(self):
        """What, beside the clip geometry, decides the LAUNCH LIST of a UNet forward under this controller (fatezero_amd/issue.py: forwards of
        one signature share a recorded plan; pointers and data may differ between them, kernels and modes may not).  None: not known --
        every forward is walked in Python."""
        return None


SPILL_RING = 3  # HBM staging slabs of the spill tier: the step in use, the step being copied, one spare (a latent blend reads a neighbour)


def _is_gpu(device):
    return torch.device(device).type == "cuda"


class SpilledStep:
    """One step's maps in the host tier: `host` is the step's slab (pinned on a GPU box), `layout` = [(key, byte offset, storage shape, lk)]
    in capture order; `slot` is the staging slab of the HBM ring that currently holds a copy (None: host only)."""
    __slots__ = ("host", "layout", "slot", "d2h_event")

    def __init__(self, host, layout):
        self.host, self.layout, self.slot = host, layout, None
        self.d2h_event = None  # copy-stream event behind the device-to-host copy that fills `host` (None: complete)

    def wait_host(self):
        """Block the HOST until `host` holds the step (readers of the reference-shaped host views come through here)."""
        ev, self.d2h_event = self.d2h_event, None
        if ev is not None:
            ev.synchronize()


class MapArena:
    """HBM slabs for captured maps. The first step sizes the slab; later steps take one allocation each (or a
    single pre-reserved block when the number of steps is known).  Reserved blocks (tens of GB) are recycled
    through a process-wide pool when their store dies, so a second job never pays hipMalloc/hipFree for them.

    Spill tier (`spill=True`: the store was built with the reference's `disk_store=True`, attention_store.py:103-108 / attention_util.py:115-116
    -- there each step's maps go to a .pt file and come back with torch.load).  Here steps stay in HBM while they fit `hbm_budget`; the steps
    beyond it are captured into a ring of SPILL_RING staging slabs and copied to (pinned) host memory on a copy stream behind the step that
    wrote them, so the capture pass never waits for PCIe unless the ring wraps onto a copy still in flight.  `fetch(step)` brings a spilled
    step back into a ring slab (copy stream, the compute stream waits on its event) and starts the copy of the step the consumer will ask
    for next, so that an edit pass walks the spilled steps with one step of H2D always under the previous step's UNet forward."""
    _pool = []  # released reserved blocks (uint8 tensors), largest reuse wins
    _host_pool = []  # released host slabs of the spill tier (pinning tens of GB is seconds: recycle)

    @classmethod
    def reset_pools(cls):
        """Give every recycled block (HBM and host) back to the allocator: a process that wants a clean slate between jobs, and the tests."""
        cls._pool = []
        cls._host_pool = []

    @classmethod
    def _take(cls, nbytes, device, hint="disk_store=True (spills the steps that do not fit to pinned host memory), ", at_most=None):
        """A block of >= nbytes: the smallest recycled one that fits -- and, with `at_most` (the spill tier's budget), is not larger than
        that: a recycled block must never raise what a budgeted arena holds -- else a fresh one."""
        best = None
        for i, t in enumerate(cls._pool):
            if t.device == torch.device(device) and t.numel() >= nbytes and (at_most is None or t.numel() <= at_most) \
                    and (best is None or t.numel() < cls._pool[best].numel()):
                best = i
        if best is not None:
            return cls._pool.pop(best)
        cls._pool.clear()  # nothing fits: let the allocator have the old blocks back before asking for a bigger one
        try:
            return torch.empty(nbytes, dtype=torch.uint8, device=device)
        except torch.OutOfMemoryError as e:  # e.g. 32 frames x 512^2 x 50 steps with index [-1, 'first']: 299 GB
            raise RuntimeError(
                f"the attention-map arena of this job needs {nbytes / 1e9:.1f} GB of HBM in one block and does not fit on {device}: "
                f"use {hint}fewer frames or DDIM steps, a one-frame SparseCausalAttention_index (e.g. ['mid'] halves the self-attention "
                "maps), save_self_attention=False, or split the clip's frames over GPUs (fatezero_amd.dist.FrameShard)") from e

    @classmethod
    def _take_host(cls, nbytes, pinned):
        for i, t in enumerate(cls._host_pool):
            if t.numel() == nbytes and t.is_pinned() == pinned:
                return cls._host_pool.pop(i)
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=pinned)

    def release(self):
        if self._block is not None:
            MapArena._pool.append(self._block)
            self._block = self.reserved = None
        if self.spilled:
            self._drain_copies()
            MapArena._host_pool = [sp.host for sp in self.spilled.values()]  # (only the latest job's: a pool, not a second arena)
        self.spilled, self.ring, self.ring_step = {}, [], []

    def __init__(self, spill=False, hbm_budget=None):
        self.step_bytes = 0
        self.cur = None
        self.cur_off = 0
        self.reserved = None              # the part of `_block` this arena hands out: exactly step_bytes * (steps reserved)
        self._block = None                # the allocation behind it (a recycled block may be larger; the whole of it goes back to the pool)
        self.reserved_off = 0
        self.first_step_done = False
        self.total_bytes = 0
        # spill tier
        self.spill = spill
        self.hbm_budget = hbm_budget      # bytes of HBM this arena may hold (None: what the device has free when the block is reserved)
        self.step = 0                     # index of the step being captured
        self.spilled = {}                 # step -> SpilledStep
        self.spilled_bytes = 0
        self.ring = []                    # SPILL_RING staging slabs (uint8 [step_bytes]), allocated with the first spilled step
        self.ring_step = []               # the step whose maps each slab holds (None: free)
        self.ring_event = []              # copy-stream event after which the slab's content / the host copy of it is complete
        self.ring_clock = []              # last use, for the least-recently-used choice
        self._clock = 0
        self._cur_slot = None             # ring slot the step being captured writes to (None: resident)
        self._copy_stream = None
        self._last_fetch = None
        self.fetch_stats = {"h2d": 0, "hits": 0}

    # -- residency --------------------------------------------------------------------------------------
    def _budget(self, device):
        if self.hbm_budget is not None:
            return int(self.hbm_budget)
        env = os.environ.get("FZ_ARENA_HBM_GB")
        if env:
            return int(float(env) * 1e9)
        if not _is_gpu(device):
            return None
        free, _ = torch.cuda.mem_get_info(device)
        recyclable = sum(t.numel() for t in MapArena._pool if t.device == torch.device(device))
        return self.total_bytes + int(0.9 * (free + recyclable))

    def reserve(self, n_steps, device):
        if self.first_step_done and self.step_bytes and n_steps > 0 and self.reserved is None:
            at_most = None
            if self.spill:
                budget = self._budget(device)
                if budget is not None:
                    at_most = max(0, budget - self.total_bytes - SPILL_RING * self.step_bytes)
                    n_steps = min(n_steps, at_most // self.step_bytes)
                    if n_steps == 0:
                        return
            self._block = MapArena._take(self.step_bytes * n_steps, device, hint="" if self.spill else
                                         "disk_store=True (spills the steps that do not fit to pinned host memory), ", at_most=at_most)
            # a recycled block may be larger than asked for: the arena hands out n_steps slabs of it and no more (residency is what the
            # budget said), and counts what it really holds
            self.reserved = self._block[: self.step_bytes * n_steps]
            self.reserved_off = 0
            self.total_bytes += self._block.numel()

    def _resident_slab(self, nbytes, device):
        """The HBM slab of the next step, or None when the step goes to the spill tier."""
        if self.reserved is not None and self.reserved_off + self.step_bytes <= self.reserved.numel():
            slab = self.reserved[self.reserved_off: self.reserved_off + self.step_bytes]
            self.reserved_off += self.step_bytes
            return slab
        want = max(self.step_bytes, nbytes)
        if self.spill:  # (a block reserved for the known number of steps was sized to the budget: what comes after it lands here as well)
            budget = self._budget(device)
            if budget is not None and self.total_bytes + want + (0 if self.ring else SPILL_RING * self.step_bytes) > budget:
                return None
        slab = torch.empty(want, dtype=torch.uint8, device=device)
        self.total_bytes += want
        return slab

    def alloc(self, shape, device, itemsize=2):
        """A map of `shape` in the step being captured: fp16 (itemsize 2) or one byte per element (itemsize 1: a uint8 tensor)."""
        dtype = torch.float16 if itemsize == 2 else torch.uint8
        nbytes = itemsize
        for s in shape:
            nbytes *= s
        nbytes = (nbytes + 255) // 256 * 256
        if not self.first_step_done:
            self.step_bytes += nbytes
            self.total_bytes += nbytes
            return torch.empty(shape, dtype=dtype, device=device)
        if self.cur is None or self.cur_off + nbytes > self.cur.numel():
            if self.cur is not None and self._cur_slot is not None:
                raise RuntimeError("spill tier: a step overflows its staging slab (the capture layout grew after the first step): the host copy "
                                   "of a step is ONE slab")
            self.cur = self._resident_slab(nbytes, device)
            self._cur_slot = None
            if self.cur is None:
                if nbytes > self.step_bytes:
                    raise RuntimeError("spill tier: a step larger than the first one cannot be staged (the capture layout changed between steps)")
                self._cur_slot = self._claim_slot(device, for_step=self.step)
                self.cur = self.ring[self._cur_slot]
            self.cur_off = 0
        out = self.cur[self.cur_off: self.cur_off + itemsize * _numel(shape)].view(dtype).view(shape)
        self.cur_off += nbytes
        return out

    def end_step(self):
        """Close the step being captured.  Returns the ring slab of a step that goes to the host tier (the caller describes its layout with
        `spill_step`) or None for a resident step."""
        slab = self.ring[self._cur_slot] if self._cur_slot is not None else None
        self.first_step_done = True
        self.cur = None
        self.cur_off = 0
        if slab is None:
            self.step += 1
        return slab

    # -- spill tier -------------------------------------------------------------------------------------
    def _streams(self, device):
        if not _is_gpu(device):
            return None, None
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=device)
        return torch.cuda.current_stream(device), self._copy_stream

    def _drain_copies(self):
        if self._copy_stream is not None:
            self._copy_stream.synchronize()

    def _claim_slot(self, device, for_step, keep=()):
        """A ring slab for `for_step`: the least recently used one outside `keep`.  The compute stream is made to wait for the copy that last
        touched it (the D2H of the step captured into it, or an H2D prefetch), and whatever the compute stream has queued on it so far is
        ordered in front of the next copy into it by an event the caller records (`_copy_in`)."""
        if not self.ring:
            self.ring = [torch.empty(self.step_bytes, dtype=torch.uint8, device=device) for _ in range(SPILL_RING)]
            self.total_bytes += SPILL_RING * self.step_bytes
            self.ring_step, self.ring_event, self.ring_clock = [None] * SPILL_RING, [None] * SPILL_RING, [0] * SPILL_RING
        slot = min((j for j in range(SPILL_RING) if j not in keep), key=lambda j: self.ring_clock[j])
        old = self.ring_step[slot]
        if old is not None and old in self.spilled:
            self.spilled[old].slot = None
        compute, _ = self._streams(device)
        if compute is not None and self.ring_event[slot] is not None:
            compute.wait_event(self.ring_event[slot])
        self.ring_step[slot] = for_step
        self._clock += 1
        self.ring_clock[slot] = self._clock
        return slot

    def spill_step(self, layout, device):
        """The step just closed was captured into a ring slab: queue its copy to the host tier behind the kernels that wrote it."""
        slot, step = self._cur_slot, self.step
        pinned = _is_gpu(device)
        sp = SpilledStep(MapArena._take_host(self.step_bytes, pinned), layout)
        compute, copy = self._streams(device)
        if copy is None:
            sp.host.copy_(self.ring[slot])
        else:
            copy.wait_event(compute.record_event())
            with torch.cuda.stream(copy):
                sp.host.copy_(self.ring[slot], non_blocking=True)
                self.ring_event[slot] = sp.d2h_event = copy.record_event()
        sp.slot = slot  # the slab still holds the step until it is claimed again
        self.spilled[step] = sp
        self.spilled_bytes += self.step_bytes
        self._cur_slot = None
        self.step += 1
        return sp

    def _copy_in(self, step, slot, device):
        sp = self.spilled[step]
        compute, copy = self._streams(device)
        if copy is None:
            self.ring[slot].copy_(sp.host)
        else:
            copy.wait_event(compute.record_event())  # the slab's previous readers are queued in front of this point
            with torch.cuda.stream(copy):
                self.ring[slot].copy_(sp.host, non_blocking=True)
                self.ring_event[slot] = copy.record_event()
        sp.slot = slot
        self.fetch_stats["h2d"] += 1

    def fetch(self, step, device):
        """The ring slab that holds spilled `step`, valid for everything queued on the compute stream from here on; starts the copy of the
        step the caller is walking towards."""
        sp = self.spilled[step]
        if sp.slot is None:
            self._copy_in(step, self._claim_slot(device, for_step=step), device)
            compute, _ = self._streams(device)
            if compute is not None:
                compute.wait_event(self.ring_event[sp.slot])
        elif self._last_fetch != step:
            self.fetch_stats["hits"] += 1
            compute, _ = self._streams(device)
            if compute is not None and self.ring_event[sp.slot] is not None:
                compute.wait_event(self.ring_event[sp.slot])
        self._clock += 1
        self.ring_clock[sp.slot] = self._clock
        if self._last_fetch != step:
            direction = -1 if self._last_fetch is None or step < self._last_fetch else 1
            nxt = step + direction
            if nxt in self.spilled and self.spilled[nxt].slot is None:
                self._copy_in(nxt, self._claim_slot(device, for_step=nxt, keep=(sp.slot,)), device)
            self._last_fetch = step
        return self.ring[sp.slot]


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class CapturedMap:
    """One captured map: `storage` is what the kernels address ([F, heads, Lq, 80] for cross maps), `view` is the
    reference-shaped tensor handed to users ([F, heads, Lq, 77]).  An 8-bit self map (`map_dtype="e5m2"` / "ue4m4") has uint8 `storage`;
    its `view` is the fp16 tensor the bytes stand for, dequantised (exactly) at every read -- no fp16 copy is kept.  `fmt` names what
    the bytes are ("fp16" | "e5m2" | "ue4m4"; 8-bit storage without a name is E5M2)."""
    __slots__ = ("storage", "lk", "fmt", "_view")

    def __init__(self, storage, lk, fmt=None):
        self.storage, self.lk = storage, lk
        self.fmt = fmt if fmt is not None else ("e5m2" if self.is_8bit else "fp16")
        assert (self.fmt != "fp16") == self.is_8bit and self.fmt in MAP_DTYPES, (self.fmt, storage.dtype)
        self._view = None if self.is_8bit else (storage[..., :lk] if storage.shape[-1] != lk else storage)

    @property
    def is_8bit(self):
        return self.storage.dtype in K.MAP8_DTYPES

    @property
    def map8_format(self):
        """The `map8_format` of kernels.self_mode_for (without meaning for an fp16 map)."""
        return self.fmt if self.is_8bit else "e5m2"

    def half(self):
        """`storage` as fp16 (itself, or the dequantised bytes)."""
        if self.fmt == "ue4m4":
            return K.ue4m4_to_half(self.storage)
        return K.e5m2_to_half(self.storage) if self.is_8bit else self.storage

    def quantise(self, attn):
        """An fp16 map as this 8-bit map's bytes, rounded the way the capture kernel of its format rounds."""
        return K.half_to_ue4m4(attn) if self.fmt == "ue4m4" else K.half_to_e5m2(attn)

    @property
    def view(self):
        if self._view is not None:
            return self._view
        h = self.half()
        return h[..., :self.lk] if h.shape[-1] != self.lk else h


class LazyStepMaps(dict):
    """One step's maps as the reference's API promises them -- {key: [fp16 tensors]} -- over CapturedMap entries whose fp16 form exists only
    while it is read (8-bit storage).  Every read of a key (`d[key]`, `get`, `items`, `values`) returns a NEW plain list of real fp16
    tensors, dequantised at that moment: it can go to torch.cat / torch.stack, be concatenated, copied or kept; dropping it frees the fp16
    copies.  The entries themselves (`raw(key)`) are what the store appends to."""

    @staticmethod
    def _tensors(items):
        return [x.view if isinstance(x, CapturedMap) else x for x in items]

    def raw(self, k):
        return dict.__getitem__(self, k)

    def __getitem__(self, k):
        return self._tensors(dict.__getitem__(self, k))

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def copy(self):
        return {k: self[k] for k in self.keys()}


class HostStepMaps(LazyStepMaps):
    """`attention_store_all_step[step]` of a spilled step: {key: [host views]} whose first read waits for the device-to-host copy that is
    still in flight when the capture pass hands the views out (the reference's `.cpu()` blocks at once, attention_store.py:86-87)."""

    def __init__(self, items, spilled_step):
        super().__init__(items)
        self._sp = spilled_step

    def __getitem__(self, k):
        self._sp.wait_host()
        return super().__getitem__(k)


def _views(cms):
    """fp16 maps: the views themselves; 8-bit maps: the entries, dequantised when the step dict is read (LazyStepMaps)."""
    return list(cms) if any(cm.is_8bit for cm in cms) else [cm.view for cm in cms]


class _StepSlab:
    """The maps of ONE step, written again by every pass that captures into it (`AttentionStore(recompute=True)`): the first pass allocates
    them in capture order, every later pass is handed the same CapturedMap objects by position -- the kernels' pointers never change."""
    __slots__ = ("maps", "pos", "complete")

    def __init__(self):
        self.maps = {k: [] for k in KEYS}
        self.pos = {k: 0 for k in KEYS}
        self.complete = False

    def rewind(self):
        self.pos = {k: 0 for k in KEYS}


class AttentionStore(AttentionControl):
    def __init__(self, save_self_attention: bool = True, disk_store=False, accumulate_self: bool = False, hbm_budget_bytes=None,
                 map_dtype: str = "fp16", recompute: bool = False):
        super().__init__()
        if map_dtype not in MAP_DTYPES:
            raise ValueError("map_dtype must be one of %s, got %r" % (", ".join(repr(m) for m in MAP_DTYPES), map_dtype))
        self.map_dtype = map_dtype  # "e5m2" / "ue4m4": self-attention maps at one byte per probability (cross maps stay fp16)
        # recompute=True (opt-in, the pipeline's `recompute_maps`): the store keeps NO map of the inversion -- only what the inversion forward
        # of every iteration was fed (the first input latent + `latents_store`, the source context, the timesteps) -- and holds one step's
        # maps at a time in a slab that the pipeline refills with `begin_recompute` / source forward / `end_recompute` right before the edit
        # step that reads it.  `maps_of_step(s)` serves that slab; `attention_store_all_step` keeps its length (one entry per inversion
        # step) but only the entry of the step in the slab holds tensors.  With it `disk_store` spills nothing: there is one step to hold.
        self.recompute = bool(recompute)
        # The reference's disk_store=True writes every step's maps to ./trash/attention_cache_*/NNN.pt and loads them back in the edit
        # (attention_store.py:103-108, attention_util.py:115-116).  Here it switches the arena's spill tier on: steps stay in HBM while they
        # fit (`hbm_budget_bytes`, or FZ_ARENA_HBM_GB, or 90 % of what the device has free), the rest goes to pinned host memory behind the
        # capture and comes back one step ahead of the edit (MapArena).  Nothing is written to disk; `store_dir` stays None.
        self.disk_store = disk_store
        self.hbm_budget_bytes = hbm_budget_bytes
        self.store_dir = None
        self.save_self_attention = save_self_attention
        self.accumulate_self = accumulate_self
        self.expected_steps = None  # optional hint (pipeline sets it) so the arena is one allocation
        self.latents_store: List[torch.Tensor] = []
        self._init_state()

    def _init_state(self):
        self.step_store = self.get_empty_store()
        self.attention_store: Dict[str, List[torch.Tensor]] = {}
        self.attention_store_all_step: List[Dict[str, List[torch.Tensor]]] = []
        self._step_maps = {k: [] for k in KEYS}       # CapturedMap objects of the current step
        self._all_step_maps: List[Dict[str, List[CapturedMap]]] = []
        self._sum_storage: Dict[str, List[torch.Tensor]] = {}
        self.arena = MapArena(spill=bool(self.disk_store) and not self.recompute, hbm_budget=self.hbm_budget_bytes)
        self._fetched = (None, None)  # (step, its maps in the ring slab) of the latest spilled step handed out
        self._reset_recompute_state()

    def _reset_recompute_state(self):
        self._slab = None            # recompute mode: the step slab (every controlled map of one step)
        self._slab_step = None       # the store step whose maps it holds (None: none / being written)
        self._writing = False        # a forward is capturing into it
        self.source_latent = None   # [1, 4, F(local), h, w]: the input of inversion iteration 0 (iteration k > 0 reads latents_store[k - 1])
        self.source_context = None   # [1, 77, D] fp16: the conditional embedding of the source prompt the inversion ran with
        self.source_timesteps = []   # the timestep of every inversion iteration

    @staticmethod
    def get_empty_store():
        return {k: [] for k in KEYS}

    @staticmethod
    def get_empty_cross_store():
        return {"down_cross": [], "mid_cross": [], "up_cross": []}

    # -- capture -------------------------------------------------------------------------------------------
    def _wants(self, is_cross, lq):
        return lq <= MAX_CONTROLLED_TOKENS and (is_cross or self.save_self_attention)

    def _slab_slot(self, shape, lk, device, map8, key) -> CapturedMap:
        """recompute mode: the next map of the step slab -- allocated by the first pass over the slab, the same object in every later one."""
        if not self._writing:
            self._open_slab()
        slab = self._slab
        pos = slab.pos[key]
        slab.pos[key] = pos + 1
        if slab.complete:
            cm = slab.maps[key][pos] if pos < len(slab.maps[key]) else None
            if cm is None or tuple(cm.storage.shape) != tuple(shape) or cm.is_8bit != map8 or cm.storage.device != torch.device(device):
                raise RuntimeError(f"recompute_maps: {key}[{pos}] of this forward is {tuple(shape)}, the step slab holds "
                                   f"{None if cm is None else tuple(cm.storage.shape)}: the clip geometry changed after the first captured step")
            return cm
        cm = CapturedMap(self.arena.alloc(shape, device, itemsize=1 if map8 else 2), lk, self.map_dtype if map8 else "fp16")
        slab.maps[key].append(cm)
        return cm

    def new_slot(self, key, frames, heads, lq, lk, is_cross, device) -> CapturedMap:
        width = K.CROSS_P_STRIDE if is_cross else lk
        self._device = device
        map8 = self.map_dtype != "fp16" and not is_cross
        if self.recompute:
            cm = self._slab_slot((frames, heads, lq, width), lk, device, map8, key)
        else:
            cm = CapturedMap(self.arena.alloc((frames, heads, lq, width), device, itemsize=1 if map8 else 2), lk,
                             self.map_dtype if map8 else "fp16")
        self._step_maps[key].append(cm)
        if self.map_dtype != "fp16":
            if not isinstance(self.step_store, LazyStepMaps):
                self.step_store = LazyStepMaps(self.step_store)
            self.step_store.raw(key).append(cm if map8 else cm.view)  # 8-bit entries are read back as fp16, dequantised at the read
        else:
            self.step_store[key].append(cm.view)
        return cm

    def plan_controlled(self, is_cross, place, n_ctrl, clip_len, heads, lq, lk, device) -> AttnPlan:
        if not self._wants(is_cross, lq):
            return AttnPlan(0)
        key = f"{place}_{'cross' if is_cross else 'self'}"
        cm = self.new_slot(key, n_ctrl, heads, lq, lk, is_cross, device)
        return AttnPlan(0, K.self_mode_for(K.FZ_ATTN_CAPTURE, cm.storage, cm.map8_format), p=cm.storage)

    @property
    def issue_events_first(self):
        """plan_controlled hands out a slot of the arena per captured layer: nothing of the forward is read."""
        return type(self).plan_controlled is AttentionStore.plan_controlled

    def issue_signature(self):
        if type(self).plan_controlled is not AttentionStore.plan_controlled:
            return None  # a subclass that plans differently says so itself
        sig = ("store", bool(self.LOW_RESOURCE), bool(self.save_self_attention), self.map_dtype)
        if self.recompute:  # (every step is captured into ONE slab)
            sig += ("recompute",)
        return sig

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        """Reference tensor protocol (attention_store.py:81-93): keep a copy of the map."""
        if self._wants(is_cross, attn.shape[-2]):
            key = f"{place_in_unet}_{'cross' if is_cross else 'self'}"
            f, heads, lq, lk = attn.shape
            cm = self.new_slot(key, f, heads, lq, lk, is_cross, attn.device)
            if cm.storage.shape[-1] != lk:
                cm.storage[..., lk:] = 0
            if cm.is_8bit:
                cm.storage.copy_(cm.quantise(attn))
            else:
                cm.view.copy_(attn)
        return attn

    def _sum_step(self):
        # running sum (attention_store.py:95-101), fp32, cross maps (+ self maps on request)
        keys = [k for k in KEYS if k.endswith("cross") or self.accumulate_self]
        if len(self.attention_store) == 0:
            self.attention_store = self.get_empty_store()
            self._sum_storage = {k: [] for k in KEYS}
            for k in keys:
                for cm in self._step_maps[k]:
                    s = cm.half().float()
                    self._sum_storage[k].append(s)
                    self.attention_store[k].append(s[..., : cm.view.shape[-1]] if s.shape[-1] != cm.view.shape[-1] else s)
        else:
            for k in keys:
                for acc, cm in zip(self._sum_storage[k], self._step_maps[k]):
                    K.accumulate(acc, cm.half())

    # -- recompute mode --------------------------------------------------------------------------------------
    # The inversion of this mode IS the resident inversion -- the store registered, the capturing launches, the running sum of the cross maps
    # (so `show_cross_attention` renders the same strips) -- except that every iteration captures into the same slab: a plain-flash inversion
    # would not do, its attention outputs differ from the capturing launches' in the last bits and the edit could not reproduce a resident job.
    def begin_source_pass(self, latent, context):
        """In front of the inversion loop: keep what iteration 0 is fed (`latent` [1, 4, F, h, w], this rank's frames) and the source
        context; the later inputs are `latents_store`, the timesteps are appended by the loop."""
        if self.latents_store or self._all_step_maps:
            self.reset()  # an earlier inversion's latents: the step indices of this one start at 0
        self.source_latent = latent.detach().clone(memory_format=torch.contiguous_format)  # (a VAE-encoded clip arrives as a permuted view)
        self.source_context = context.detach().to(torch.float16).clone()
        self.source_timesteps = []

    @property
    def slab_step(self):
        """The store step whose maps are resident (None: none)."""
        return self._slab_step

    def _open_slab(self):
        if self._slab is None:
            self._slab = _StepSlab()
        if self._slab_step is not None:
            self.attention_store_all_step[self._slab_step] = self.get_empty_store()  # (its views would show the step that overwrites them)
        self._slab_step = None
        self._slab.rewind()
        self._writing = True

    def _close_slab(self, step_in_store):
        slab = self._slab
        if self._writing:
            if slab.complete and any(slab.pos[k] != len(slab.maps[k]) for k in KEYS):
                raise RuntimeError("recompute_maps: this forward captured fewer maps than the step slab holds")
            slab.complete = True
            self._writing = False
            self._slab_step = step_in_store
            self.attention_store_all_step[step_in_store] = self.step_store
        self.step_store = self.get_empty_store()
        self._step_maps = {k: [] for k in KEYS}

    def source_input(self, step_in_store):
        """(input latent [1, 4, F, h, w], timestep, context) of inversion iteration `step_in_store`."""
        lat = self.source_latent if step_in_store == 0 else self.latents_store[step_in_store - 1]
        return lat, self.source_timesteps[step_in_store], self.source_context

    def begin_recompute(self, step_in_store):
        """The source forward that follows (this store registered, LOW_RESOURCE) writes the maps of inversion iteration `step_in_store` into
        the step slab."""
        if not self.recompute or self.source_latent is None:
            raise RuntimeError("begin_recompute needs AttentionStore(recompute=True) after an inversion in that mode")
        self.cur_att_layer = 0
        self.step_store = self.get_empty_store()
        self._step_maps = {k: [] for k in KEYS}
        self._open_slab()

    def end_recompute(self, step_in_store):
        self._close_slab(step_in_store)
        self.cur_att_layer = 0

    def _between_steps_recompute(self):
        """An inversion step in recompute mode: the running sum as ever, then the step's maps stay where they are -- in the slab the next
        iteration overwrites.  The per-step lists get an entry all the same: their length is what the edit controller counts its way back
        from (`_step_in_store`)."""
        self._sum_step()
        step = len(self._all_step_maps)
        self.attention_store_all_step.append(self.get_empty_store())
        self._all_step_maps.append(None)
        self._close_slab(step)

    def between_steps(self):
        if self.recompute:
            return self._between_steps_recompute()
        self._sum_step()
        self.attention_store_all_step.append(self.step_store)
        self._all_step_maps.append(self._step_maps)
        self.step_store = self.get_empty_store()
        self._step_maps = {k: [] for k in KEYS}
        first = not self.arena.first_step_done
        slab = self.arena.end_step()
        if slab is not None:
            self._spill_last_step(slab)
        if first and self.expected_steps and self.latents_store is not None:
            dev = None
            for k in KEYS:
                if self._all_step_maps[0][k]:
                    dev = self._all_step_maps[0][k][0].storage.device
                    break
            if dev is not None:
                self.arena.reserve(self.expected_steps - 1, dev)

    def step_callback(self, x_t):
        x_t = super().step_callback(x_t)
        self.latents_store.append(x_t.detach().clone())
        return x_t

    def _spill_last_step(self, slab):
        """The step just appended was captured into a staging slab of the spill tier: describe its layout, queue the copy to the host
        tier, and hand the reference-shaped views of `attention_store_all_step` over to the host copy (the reference keeps a file path
        there; its 32 x 32 maps are host tensors even without disk_store, attention_store.py:86-87)."""
        step = len(self._all_step_maps) - 1
        maps, layout, base = self._all_step_maps[step], [], slab.data_ptr()
        for k in KEYS:
            for cm in maps[k]:
                layout.append((k, cm.storage.data_ptr() - base, tuple(cm.storage.shape), cm.lk, cm.storage.element_size()))
        sp = self.arena.spill_step(layout, slab.device)
        self.attention_store_all_step[step] = HostStepMaps({k: _views(v) for k, v in self._maps_over(sp.host, layout, self.map_dtype).items()}, sp)
        self._all_step_maps[step] = None  # resolved through the arena from here on (maps_of_step)

    @staticmethod
    def _maps_over(slab, layout, map_dtype="e5m2"):
        out = {k: [] for k in KEYS}
        for k, off, shape, lk, itemsize in layout:  # (the 8-bit slabs travel through the spill tier as they are: `map_dtype` names them)
            raw = slab[off: off + itemsize * _numel(shape)]
            out[k].append(CapturedMap((raw.view(torch.float16) if itemsize == 2 else raw).view(shape), lk,
                                      "fp16" if itemsize == 2 else map_dtype))
        return out

    def with_map_dtype(self, map_dtype: str):
        """A fresh store of this one's settings with another map format (this one's maps are not carried over)."""
        st = AttentionStore(save_self_attention=self.save_self_attention, disk_store=self.disk_store, accumulate_self=self.accumulate_self,
                            hbm_budget_bytes=self.hbm_budget_bytes, map_dtype=map_dtype, recompute=self.recompute)
        st.LOW_RESOURCE = self.LOW_RESOURCE
        return st

    def with_recompute(self, recompute: bool):
        """A fresh store of this one's settings with the recompute mode switched (this one's maps are not carried over)."""
        st = AttentionStore(save_self_attention=self.save_self_attention, disk_store=self.disk_store, accumulate_self=self.accumulate_self,
                            hbm_budget_bytes=self.hbm_budget_bytes, map_dtype=self.map_dtype, recompute=recompute)
        st.LOW_RESOURCE = self.LOW_RESOURCE
        return st

    def maps_of_step(self, step_in_store) -> Dict[str, List[CapturedMap]]:
        if step_in_store < 0:
            step_in_store += len(self._all_step_maps)
        if self.recompute:
            if self._slab_step != step_in_store:
                raise RuntimeError(f"recompute_maps: the maps of store step {step_in_store} are not resident (the step slab holds "
                                   f"{'no step' if self._slab_step is None else 'step %d' % self._slab_step}): the pipeline recomputes a "
                                   "step right before the edit step that reads it")
            return self._slab.maps
        maps = self._all_step_maps[step_in_store]
        if maps is not None:
            return maps
        if self._fetched[0] != step_in_store:  # a spilled step: into a staging slab of the ring, the next one behind it
            sp = self.arena.spilled[step_in_store]
            slab = self.arena.fetch(step_in_store, self._device)
            self._fetched = (step_in_store, self._maps_over(slab, sp.layout, self.map_dtype))
        return self._fetched[1]

    def get_average_attention(self):
        return {key: [item / self.cur_step for item in self.attention_store[key]] for key in self.attention_store}

    def reset(self):
        super().reset()
        self.release_arena()
        self._init_state()

    def release_arena(self):
        """Drop every captured map and hand the reserved HBM block back to the pool."""
        arena = getattr(self, "arena", None)
        if arena is not None:
            self.step_store = self.get_empty_store()
            self.attention_store_all_step = []
            self._all_step_maps = []
            self._step_maps = {k: [] for k in KEYS}
            self.attention_store = {}
            self.latents_store = []
            if hasattr(self, "_sum_storage"):
                self._sum_storage = None
            arena.cur = None
            arena.release()
            # tensors handed out earlier (attention_store_all_step views, CapturedMap.storage) alias the released block and are
            # invalid from here on; a store that is used again reserves a fresh arena instead of allocating per step
            self.arena = type(arena)(spill=arena.spill, hbm_budget=arena.hbm_budget)
            self._fetched = (None, None)
            self._reset_recompute_state()

    def __del__(self):
        try:
            self.release_arena()
        except Exception:
            pass

    @property
    def arena_bytes(self):
        return self.arena.total_bytes
