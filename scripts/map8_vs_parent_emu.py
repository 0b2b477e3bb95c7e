#!/usr/bin/env python3
"""fp16 capture / inject of this tree against an emulator library built from ANOTHER revision of csrc/attn_self.hip (bit for bit).

Build the other revision's library by compiling its attn_self.hip with the emulator flags of fatezero_amd/build.py and linking it with this
tree's other emulator objects (fatezero_amd/build/emu/*.o), then:

    python scripts/map8_vs_parent_emu.py /path/to/libfatezero_emu_other.so
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from fatezero_amd import _native, build, kernels as K  # noqa: E402
import kernel_cases as KC  # noqa: E402

CASES = [(40, 64, [-1, "first"], 2), (64, 80, ["mid"], 3), (80, 144, [-1, "first"], 2), (160, 72, [-1, "first"], 2), (16, 200, [-1, "mid", 1], 3)]


def run(lib):
    _native.use_test_backend(lib)
    outs = []
    for (d, lq, idx, clip) in CASES:
        g = torch.Generator().manual_seed(d + lq)
        heads, n = 2, 2 * clip
        c = heads * d
        q, k, v = KC._mk((n, lq, c), g, "cpu", 1.5), KC._mk((n, lq, c), g, "cpu", 1.5), KC._mk((n, lq, c), g, "cpu")
        vt = K.transpose_pad(v, K.pad64(lq))
        p = torch.full((clip + 1, heads, lq, max(1, len(idx)) * lq), float("nan"), dtype=torch.float16)
        kw = dict(clip_len=clip, heads=heads, index_list=idx, frame0=clip, n_frames=clip, p_frame_off=1)
        o = torch.zeros(n, lq, c, dtype=torch.float16)
        K.attn_self(q, k, vt, o, mode=K.FZ_ATTN_CAPTURE, p=p, **kw)
        outs += [o.clone(), p[1:].clone()]
        mask = (torch.rand(clip, lq, generator=g) > 0.5).float()
        for m in (None, mask):
            o = torch.zeros(n, lq, c, dtype=torch.float16)
            K.attn_self(q, k if m is not None else None, vt, o, mode=K.FZ_ATTN_INJECT, p=p, row_mask=m, **kw)
            outs.append(o.clone())
    _native.reset_backend()
    return outs


if __name__ == "__main__":
    a, b = run(sys.argv[1]), run(build.build_emu())
    print("tensors compared:", len(a))
    print("all torch.equal:", all(torch.equal(x, y) for x, y in zip(a, b)))
