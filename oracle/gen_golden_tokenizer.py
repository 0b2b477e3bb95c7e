"""Golden vectors for the OpenAI-CLIP tokenizer test (tests/test_clip_emu.py; TEST INFRASTRUCTURE, needs a checkout of the reference).

    python oracle/gen_golden_tokenizer.py <reference checkout>

Runs the reference's SimpleTokenizer (CLIP/clip/simple_tokenizer.py, imported by file path with a pass-through ftfy stub -- ftfy only
repairs mojibake) on the test's prompts and records its ids.  Its merges file (CLIP/clip/bpe_simple_vocab_16e6.txt.gz, 1.3 MB) is
reduced to a file of the same layout that keeps, at their ranks, the merges tokenizing these prompts can reach -- every pair that is
ever adjacent while their words are merged -- and holds a pair of symbols that never occurs in byte-encoded text at every other rank.
A token's id is 512 + the rank of its merge, and a greedy lowest-rank merge never picks a pair that is not adjacent, so the reduced file
gives these prompts the full vocabulary's ids (special tokens included: the vocabulary keeps its size).
"""
import gzip
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(os.path.dirname(HERE), "tests", "golden")
N_MERGES = 49152 - 256 - 2
PROMPTS = ["a silver jeep driving down a curvy road in the countryside", "a Porsche car driving down a curvy road in the countryside",
           "watercolor painting of a silver jeep driving down a curvy road", "A squirrel, eating a carrot!", "van gogh style: rabbit's jump",
           "  two   spaces\tand tabs ", "swarovski crystal swan swimming in a river near a wall and bushes", "3 cats & 12 tigers (cartoon)"]


def reachable_ranks(mod, tok, text):
    """Ranks of every merge whose pair is adjacent at some point while `text`'s words are merged lowest rank first."""
    ranks = set()
    text = mod.whitespace_clean(mod.basic_clean(text)).lower()
    for word in tok.pat.findall(text):
        w = "".join(tok.byte_encoder[b] for b in word.encode("utf-8"))
        sym = list(w[:-1]) + [w[-1] + "</w>"]
        while len(sym) > 1:
            pairs = {(sym[i], sym[i + 1]) for i in range(len(sym) - 1)}
            known = [p for p in pairs if p in tok.bpe_ranks]
            ranks.update(tok.bpe_ranks[p] for p in known)
            if not known:
                break
            a, b = min(known, key=tok.bpe_ranks.get)
            out, i = [], 0
            while i < len(sym):
                if i < len(sym) - 1 and sym[i] == a and sym[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(sym[i])
                    i += 1
            sym = out
    return ranks


if __name__ == "__main__":
    ref_root = sys.argv[1]
    bpe = os.path.join(ref_root, "CLIP", "clip", "bpe_simple_vocab_16e6.txt.gz")
    sys.modules.setdefault("ftfy", types.SimpleNamespace(fix_text=lambda s: s))
    spec = importlib.util.spec_from_file_location("ref_simple_tokenizer", os.path.join(ref_root, "CLIP", "clip", "simple_tokenizer.py"))
    tok_module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tok_module)
    tok = tok_module.SimpleTokenizer(bpe)
    sot, eot = tok.encoder["<|startoftext|>"], tok.encoder["<|endoftext|>"]
    ids = {p: [sot] + tok.encode(p) + [eot] for p in PROMPTS}
    keep = set()
    for p in PROMPTS:
        keep |= reachable_ranks(tok_module, tok, p)
    lines = gzip.open(bpe, "rt", encoding="utf-8").read().split("\n")
    out = [lines[0]]
    for r in range(N_MERGES):
        out.append(lines[1 + r] if r in keep else chr(0x4E00 + r // 256) + " " + chr(0x5000 + r % 256))
    with gzip.GzipFile(os.path.join(GOLD, "clip_bpe_prompts.txt.gz"), "wb", mtime=0) as f:
        f.write(("\n".join(out) + "\n").encode("utf-8"))
    json.dump({"prompts": PROMPTS, "ids": [ids[p] for p in PROMPTS], "merges_kept": len(keep), "sot": sot, "eot": eot},
              open(os.path.join(GOLD, "clip_tokenizer_ids.json"), "w"), indent=1)
    print(f"{len(keep)} of {N_MERGES} merges kept; ids of {len(PROMPTS)} prompts recorded")
