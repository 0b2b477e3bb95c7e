#!/usr/bin/env python3
"""This tree against ANOTHER checkout of the project (the parent commit, say, exported with `git archive`), bit for bit on the emulator:
the unet_tiny40_default forward and one tiny whole job (pipe_f3_mid_next: DDIM inversion with capture, then the edit).  Each tree runs in a
process of its own -- its Python, its emulator library (built if missing) -- and the outputs are compared with torch.equal.

    python scripts/tree_vs_parent_emu.py /path/to/other/tree
"""
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(root, out):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    from fatezero_amd import _native, build
    import pipeline_cases as PC
    _native.use_test_backend(build.build_emu())
    meta = PC.load_json("unet_meta.json")
    m, g = meta["unet_tiny40_default"], PC.load_npz("unet_tiny40_default.npz")
    shapes = m["state_dict_shapes"] or meta[m.get("shapes_from", "unet_tiny16_default")]["state_dict_shapes"]
    unet = PC.UNetPseudo3DConditionModel(sample_size=g["x"].shape[-1], **PC.TINY[m["kind"]], **m["model_config"])
    unet.load_state_dict(PC.procedural_state_dict([(n, tuple(s)) for n, s in shapes]))
    unet = unet.half().eval()
    y = unet(torch.from_numpy(g["x"]), int(g["t"]), torch.from_numpy(g["ctx"])).sample
    res, pipe = PC.run_pipeline_case("pipe_f3_mid_next", "cpu", return_pipe=True)
    maps = pipe.store_controller.attention_store_all_step[0]
    torch.save({"unet_tiny40_default": y, "job_edited_latents": pipe.last_edited_latents,
                "job_inversion_maps_step0": {k: [t.clone() for t in v] for k, v in maps.items()},
                "job_errors_vs_golden": {k: v for k, v in res.items() if isinstance(v, (int, float))}}, out)


def same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


if __name__ == "__main__":
    if sys.argv[1] == "--dump":
        dump(sys.argv[2], sys.argv[3])
        sys.exit(0)
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for root in (os.path.abspath(sys.argv[1]), ROOT):
            out = os.path.join(d, "out%d.pt" % len(outs))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", root, out], check=True, cwd=root)
            outs.append(torch.load(out))
    ok = True
    for k in outs[1]:
        eq = same(outs[0][k], outs[1][k])
        ok = ok and eq
        print("%-28s %s" % (k, "torch.equal" if eq else "DIFFERENT"))
    print("job errors vs the golden recording:", outs[1]["job_errors_vs_golden"])
    sys.exit(0 if ok else 1)
