"""Return codes of the four GEMM entry points (fz_gemm, fz_gemm_qkvt, fz_gemm_gn, fz_gemm_lnout) are part of the ABI, WITHOUT a GPU:
one table of descriptors and operand sets, each row with the code it must return -- every single rejection the entries contain, one
valid call per entry at a small shape, and rows where TWO checks fail at once with different codes (they pin the order of the checks).

The expected codes are those of the library BEFORE the four entries shared one FzGemmDesc -> IgArgs translator (csrc/igemm.hip,
ig_from_desc): the table was run against that build and its answers written down here as literals."""
import ctypes as C
import os

import pytest
import torch

from fatezero_amd import _native, build

OK, NO_STATS, BAD, UNSUP = 0, _native.FZ_GEMM_NO_STATS, -1, -2
GEGLU = _native.FZ_GEMM_GEGLU
BIG = 1 << 31


@pytest.fixture(scope="module", autouse=True)
def emu_backend():
    _native.use_test_backend(os.environ.get("FZ_EMU_LIB") or build.build_emu())
    yield
    _native.reset_backend()


# operands: one pool, large enough for every valid row (128 rows x 320 columns at the most)
_g = torch.Generator().manual_seed(0)
_h = lambda *s: (torch.randn(*s, generator=_g) * 0.1).to(torch.float16)
POOL = {
    "x": _h(128, 64), "w": _h(320, 64), "bias": _h(320), "res": _h(128, 320), "res2": _h(128, 320), "y": torch.zeros(128 * 320 + 64, dtype=torch.float16),
    "yt": torch.zeros(2 * 64 * 64, dtype=torch.float16), "gamma": _h(320), "beta": _h(320), "y_ln": torch.zeros(128, 320, dtype=torch.float16),
    "partial": torch.zeros(32 * 3, dtype=torch.float32), "ws": torch.zeros(8 * 128 * 320, dtype=torch.float32),
}

# the valid call of each entry: descriptor fields, operands (names of POOL, None = null pointer) and the entry's own scalars
BASE = {
    "gemm": (dict(rows=16, in_features=64, out_features=64, ldx=64, ldw=64, ldy=64, batch=1),
             dict(x="x", w="w", bias="bias", res=None, res2=None, y="y", ws=None)),
    "qkvt": (dict(rows=128, in_features=64, out_features=128, ldx=64, ldw=64, ldy=64, batch=1),
             dict(x="x", w="w", y="y", yt="yt", split_col=64, rows_per_frame=64, yt_frame_stride=64 * 64, ldyt=64)),
    "gn": (dict(rows=128, in_features=64, out_features=320, ldx=64, ldw=64, ldy=320, batch=1),
           dict(x="x", w="w", bias="bias", res=None, res2=None, y="y", partial="partial", groups=32, rows_per_frame=128)),
    "lnout": (dict(rows=128, in_features=64, out_features=320, ldx=64, ldw=64, ldy=320, batch=1),
              dict(x="x", w="w", bias="bias", res=None, res2=None, y="y", gamma="gamma", beta="beta", y_ln="y_ln", ld_ln=320, ws=None)),
}
RESTRICTED = ("qkvt", "gn", "lnout")
GEGLU_D = dict(epilogue=GEGLU, out_features=128)                          # fz_gemm, GEGLU: y is 64 wide
VT_D = dict(transpose_out=1, rows_store=16, ldy=16)                       # fz_gemm, V^T: y [64][16]
VT_O = dict(bias=None)

# (id, entry, descriptor overrides, operand overrides, expected code)
ROWS = [
    # ---- valid calls
    ("gemm-valid", "gemm", {}, {}, OK),
    ("gemm-valid-res", "gemm", {}, dict(res="res", res2="res2"), OK),
    ("gemm-valid-res-rows", "gemm", dict(res_rows=8), dict(res="res"), OK),
    ("gemm-valid-geglu", "gemm", GEGLU_D, {}, OK),
    ("gemm-valid-geglu-ignores-split-k", "gemm", dict(GEGLU_D, split_k=2), {}, OK),
    ("gemm-valid-vt", "gemm", VT_D, VT_O, OK),
    ("gemm-valid-vt-ignores-split-k", "gemm", dict(VT_D, split_k=2), VT_O, OK),
    ("gemm-valid-batch0-is-1", "gemm", dict(batch=0), {}, OK),
    ("gemm-valid-rows8-k8", "gemm", dict(rows=8, in_features=8, ldx=8, ldw=8), {}, OK),
    ("qkvt-valid", "qkvt", {}, {}, OK),
    ("qkvt-valid-res-rows-not-read", "qkvt", dict(res_rows=-1), {}, OK),
    ("qkvt-valid-pinned-64", "qkvt", dict(tile_cfg=212222), {}, OK),
    ("gn-valid", "gn", dict(tile_cfg=254122), {}, OK),
    ("gn-valid-library-picks-another-tile", "gn", {}, {}, NO_STATS),
    ("gn-valid-ignores-split-k", "gn", dict(split_k=2, tile_cfg=254122), {}, OK),
    ("gn-valid-res-rows", "gn", dict(res_rows=64, tile_cfg=254122), dict(res="res"), OK),
    ("gn-no-stats-groups", "gn", {}, dict(groups=5), NO_STATS),
    ("gn-no-stats-rows-per-frame", "gn", {}, dict(rows_per_frame=64), NO_STATS),
    ("lnout-valid", "lnout", dict(tile_cfg=254122), {}, OK),
    ("lnout-valid-library-picks-another-tile", "lnout", {}, {}, NO_STATS),
    ("lnout-valid-res", "lnout", dict(tile_cfg=254122), dict(res="res", res2="res2"), OK),
    ("lnout-no-ln-ld-ln", "lnout", {}, dict(ld_ln=324), NO_STATS),
    # ---- fz_gemm: single rejections
    ("gemm-null-x", "gemm", {}, dict(x=None), BAD),
    ("gemm-null-w", "gemm", {}, dict(w=None), BAD),
    ("gemm-null-y", "gemm", {}, dict(y=None), BAD),
    ("gemm-rows0", "gemm", dict(rows=0), {}, BAD),
    ("gemm-k0", "gemm", dict(in_features=0), {}, BAD),
    ("gemm-o-neg", "gemm", dict(out_features=-64), {}, BAD),
    ("gemm-res-rows-neg", "gemm", dict(res_rows=-1), {}, BAD),
    ("gemm-res-rows-batch", "gemm", dict(res_rows=8, batch=2), dict(res="res"), BAD),
    ("gemm-res-rows-vt", "gemm", dict(VT_D, res_rows=8), VT_O, BAD),
    ("gemm-res-rows-big", "gemm", dict(rows=BIG, res_rows=8), dict(res="res"), BAD),
    ("gemm-ldx-small", "gemm", dict(ldx=56), {}, BAD),
    ("gemm-ldw-small", "gemm", dict(ldw=56), {}, BAD),
    ("gemm-ldx-mod8", "gemm", dict(ldx=68), {}, BAD),
    ("gemm-ldw-mod8", "gemm", dict(ldw=68), {}, BAD),
    ("gemm-epilogue", "gemm", dict(epilogue=7), {}, BAD),
    ("gemm-ldy-small", "gemm", dict(ldy=56), {}, BAD),
    ("gemm-geglu-ldy-small", "gemm", dict(GEGLU_D, ldy=56), {}, BAD),
    ("gemm-geglu-o-mod64", "gemm", dict(GEGLU_D, out_features=96), {}, UNSUP),
    ("gemm-geglu-res", "gemm", GEGLU_D, dict(res="res"), UNSUP),
    ("gemm-geglu-res2", "gemm", GEGLU_D, dict(res2="res2"), UNSUP),
    ("gemm-vt-geglu", "gemm", dict(VT_D, epilogue=GEGLU), VT_O, UNSUP),
    ("gemm-vt-bias", "gemm", VT_D, {}, UNSUP),
    ("gemm-vt-res", "gemm", VT_D, dict(VT_O, res="res"), UNSUP),
    ("gemm-vt-res2", "gemm", VT_D, dict(VT_O, res2="res2"), UNSUP),
    ("gemm-vt-rows-big", "gemm", dict(VT_D, rows=BIG), VT_O, UNSUP),
    ("gemm-vt-ldy-small", "gemm", dict(VT_D, rows_store=24), VT_O, BAD),
    ("gemm-k-mod8", "gemm", dict(in_features=12, ldx=16, ldw=16), {}, UNSUP),
    ("gemm-tile-cfg", "gemm", dict(tile_cfg=123), {}, BAD),
    ("gemm-split-k-no-workspace", "gemm", dict(split_k=2), {}, UNSUP),
    ("gemm-split-k-small-workspace", "gemm", dict(split_k=2, workspace_floats=64), dict(ws="ws"), BAD),
    ("gemm-split-k-beyond-k", "gemm", dict(split_k=64, workspace_floats=1 << 18), dict(ws="ws"), BAD),
    # ---- fz_gemm: two checks fail, different codes
    ("gemm-2-vt-res+ldx-small", "gemm", dict(VT_D, ldx=56), dict(VT_O, res="res"), BAD),
    ("gemm-2-geglu-o-mod64+ldy-small", "gemm", dict(GEGLU_D, out_features=96, ldy=40), {}, BAD),
    ("gemm-2-vt-bias+ldy-small", "gemm", dict(VT_D, rows_store=24), {}, UNSUP),
    ("gemm-2-geglu-res+res-rows-neg", "gemm", dict(GEGLU_D, res_rows=-1), dict(res="res"), BAD),
    ("gemm-2-vt-geglu+ldw-mod8", "gemm", dict(VT_D, epilogue=GEGLU, ldw=68), VT_O, BAD),
    ("gemm-2-vt-rows-big+ldy-small", "gemm", dict(VT_D, rows=BIG), VT_O, UNSUP),
    ("gemm-2-k-mod8+ldy-small", "gemm", dict(in_features=12, ldx=16, ldw=16, ldy=56), {}, BAD),
    # ---- fz_gemm_qkvt: single rejections
    ("qkvt-null-x", "qkvt", {}, dict(x=None), BAD),
    ("qkvt-null-w", "qkvt", {}, dict(w=None), BAD),
    ("qkvt-null-y", "qkvt", {}, dict(y=None), BAD),
    ("qkvt-null-yt", "qkvt", {}, dict(yt=None), BAD),
    ("qkvt-rows0", "qkvt", dict(rows=0), {}, BAD),
    ("qkvt-k0", "qkvt", dict(in_features=0), {}, BAD),
    ("qkvt-o0", "qkvt", dict(out_features=0), {}, BAD),
    ("qkvt-split0", "qkvt", {}, dict(split_col=0), BAD),
    ("qkvt-split-neg", "qkvt", {}, dict(split_col=-64), BAD),
    ("qkvt-split-all", "qkvt", {}, dict(split_col=128), BAD),
    ("qkvt-split-mod64", "qkvt", dict(ldy=96), dict(split_col=96), BAD),
    ("qkvt-split-pinned-320", "qkvt", dict(tile_cfg=254222), {}, BAD),
    ("qkvt-split-pinned-128", "qkvt", dict(tile_cfg=222222), {}, BAD),
    ("qkvt-pinned-unknown", "qkvt", dict(tile_cfg=244222), {}, BAD),
    ("qkvt-rpf0", "qkvt", {}, dict(rows_per_frame=0), BAD),
    ("qkvt-rpf-mod8", "qkvt", {}, dict(rows_per_frame=4), BAD),
    ("qkvt-rows-mod-rpf", "qkvt", {}, dict(rows_per_frame=48), BAD),
    ("qkvt-ldyt-small", "qkvt", {}, dict(ldyt=56), BAD),
    ("qkvt-ldyt-mod8", "qkvt", {}, dict(ldyt=68), BAD),
    ("qkvt-yt-stride-mod8", "qkvt", {}, dict(yt_frame_stride=64 * 64 + 4), BAD),
    ("qkvt-ldy-small", "qkvt", dict(ldy=56), {}, BAD),
    ("qkvt-ldy-mod8", "qkvt", dict(ldy=68), {}, BAD),
    ("qkvt-rows-big", "qkvt", dict(rows=BIG), {}, BAD),
    ("qkvt-k-mod8", "qkvt", dict(in_features=12, ldx=16, ldw=16), {}, UNSUP),
    # ---- fz_gemm_gn: single rejections
    ("gn-null-partial", "gn", {}, dict(partial=None), BAD),
    ("gn-ldy-small", "gn", dict(ldy=312), {}, BAD),
    ("gn-res-rows-big", "gn", dict(rows=BIG, res_rows=8), dict(res="res"), BAD),
    # ---- fz_gemm_lnout: single rejections
    ("lnout-null-gamma", "lnout", {}, dict(gamma=None), BAD),
    ("lnout-null-beta", "lnout", {}, dict(beta=None), BAD),
    ("lnout-null-y-ln", "lnout", {}, dict(y_ln=None), BAD),
    ("lnout-ldy-small", "lnout", dict(ldy=312), {}, BAD),
    ("lnout-ld-ln-small", "lnout", {}, dict(ld_ln=312), BAD),
    ("lnout-res-rows-big", "lnout", dict(rows=BIG, res_rows=8), dict(res="res"), BAD),
    ("lnout-split-k-no-workspace", "lnout", dict(split_k=2), {}, UNSUP),
    ("lnout-split-k-small-workspace", "lnout", dict(split_k=2, workspace_floats=64), dict(ws="ws"), BAD),
    # ---- the three restricted entries: two checks fail, different codes
    ("qkvt-2-vt+split-mod64", "qkvt", dict(transpose_out=1, ldy=96), dict(split_col=96), UNSUP),
    ("qkvt-2-batch+ldx-small", "qkvt", dict(batch=2, ldx=56), {}, UNSUP),
    ("qkvt-2-geglu+ldyt-small", "qkvt", dict(epilogue=GEGLU), dict(ldyt=56), UNSUP),
    ("qkvt-2-w-stride+rows0", "qkvt", dict(w_batch_stride=64, rows=0), {}, BAD),
    ("qkvt-2-null-yt+vt", "qkvt", dict(transpose_out=1), dict(yt=None), BAD),
    ("qkvt-2-k-mod8+split-mod64", "qkvt", dict(in_features=12, ldx=16, ldw=16, ldy=96), dict(split_col=96), BAD),
    ("gn-2-vt+ldy-small", "gn", dict(transpose_out=1, ldy=312), {}, UNSUP),
    ("gn-2-batch+res-rows-neg", "gn", dict(batch=2, res_rows=-1), {}, UNSUP),
    ("gn-2-null-partial+geglu", "gn", dict(epilogue=GEGLU), dict(partial=None), BAD),
    ("gn-2-w-stride+ldw-mod8", "gn", dict(w_batch_stride=64, ldw=68), {}, UNSUP),
    ("gn-2-k-mod8+ldy-small", "gn", dict(in_features=12, ldx=16, ldw=16, ldy=312), {}, BAD),
    ("lnout-2-vt+ld-ln-small", "lnout", dict(transpose_out=1), dict(ld_ln=312), UNSUP),
    ("lnout-2-null-gamma+batch", "lnout", dict(batch=2), dict(gamma=None), BAD),
    ("lnout-2-geglu+ldx-small", "lnout", dict(epilogue=GEGLU, ldx=56), {}, UNSUP),
    ("lnout-2-w-stride+res-rows-neg", "lnout", dict(w_batch_stride=64, res_rows=-1), {}, UNSUP),
    ("lnout-2-split-k-no-workspace+ld-ln-small", "lnout", dict(split_k=2), dict(ld_ln=312), BAD),
]
# ---- what the three restricted entries share, row by row
for _e in RESTRICTED:
    ROWS += [
        (_e + "-null-desc", _e, None, {}, BAD),
        (_e + "-epilogue-geglu", _e, dict(epilogue=GEGLU), {}, UNSUP),
        (_e + "-epilogue-unknown", _e, dict(epilogue=7), {}, UNSUP),
        (_e + "-transpose-out", _e, dict(transpose_out=1), {}, UNSUP),
        (_e + "-batch2", _e, dict(batch=2), {}, UNSUP),
        (_e + "-w-batch-stride", _e, dict(w_batch_stride=64), {}, UNSUP),
        (_e + "-ldx-small", _e, dict(ldx=56), {}, BAD),
        (_e + "-ldw-small", _e, dict(ldw=56), {}, BAD),
        (_e + "-ldx-mod8", _e, dict(ldx=68), {}, BAD),
        (_e + "-ldw-mod8", _e, dict(ldw=68), {}, BAD),
        (_e + "-tile-cfg", _e, dict(tile_cfg=123), {}, BAD),
    ]
for _e in ("gn", "lnout"):
    ROWS += [
        (_e + "-null-x", _e, {}, dict(x=None), BAD),
        (_e + "-null-w", _e, {}, dict(w=None), BAD),
        (_e + "-null-y", _e, {}, dict(y=None), BAD),
        (_e + "-rows0", _e, dict(rows=0), {}, BAD),
        (_e + "-k0", _e, dict(in_features=0), {}, BAD),
        (_e + "-o0", _e, dict(out_features=0), {}, BAD),
        (_e + "-res-rows-neg", _e, dict(res_rows=-1), {}, BAD),
        (_e + "-k-mod8", _e, dict(in_features=12, ldx=16, ldw=16), {}, UNSUP),
    ]
ROWS.append(("gemm-null-desc", "gemm", None, {}, BAD))


def call(entry, d_over, o_over):
    lib = _native.lib()
    base_d, base_o = BASE[entry]
    d = None
    if d_over is not None:
        d = _native.FzGemmDesc()
        for k, v in dict(base_d, **d_over).items():
            setattr(d, k, v)
    o = dict(base_o, **o_over)
    p = lambda name: None if o[name] is None else POOL[o[name]].data_ptr()
    dref = None if d is None else C.byref(d)
    if entry == "gemm":
        return lib.fz_gemm(dref, p("x"), p("w"), p("bias"), p("res"), p("res2"), p("y"), p("ws"), None)
    if entry == "qkvt":
        return lib.fz_gemm_qkvt(dref, p("x"), p("w"), p("y"), p("yt"), o["split_col"], o["rows_per_frame"], o["yt_frame_stride"], o["ldyt"], None)
    if entry == "gn":
        return lib.fz_gemm_gn(dref, p("x"), p("w"), p("bias"), p("res"), p("res2"), p("y"), p("partial"), o["groups"], o["rows_per_frame"], None)
    return lib.fz_gemm_lnout(dref, p("x"), p("w"), p("bias"), p("res"), p("res2"), p("y"), p("gamma"), p("beta"), 1e-5, p("y_ln"), o["ld_ln"],
                             p("ws"), None)


def test_table_ids_are_unique():
    ids = [r[0] for r in ROWS]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("rid,entry,d_over,o_over,expected", ROWS, ids=[r[0] for r in ROWS])
def test_entry_code(rid, entry, d_over, o_over, expected):
    assert call(entry, d_over, o_over) == expected
