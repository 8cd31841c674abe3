"""The captions, the parts that need no GPU: the entry point as the binding reads it from include/fod_ext.h and its
argument checks, the text of a caption on a table of inputs, the font, the CPU form (visualization.draw_labels / render
with captions) against the numpy restatement of tests/label_cases.py byte for byte, and the Trainer's switch."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import label_cases as LC
from future_od.native import abi
from future_od.utils import visualization as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = "pointer", "int"
ENTRY = "fod_render_labels"
CASES = LC.all_cases(V.FONT_5X7.numpy())
IDS = [c["name"] for c in CASES]


def _t(array):
    return None if array is None else torch.from_numpy(array)


# ---- ABI and binding ---------------------------------------------------------------------------------------------------
def test_prototype_is_read_from_the_second_header():
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P, I, I, I, P, P, I, P, P, P, I, I, P, I, P, I, I, I, I, I, I, P])
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in open(abi.HEADER_PATH).read()
    from future_od.native import lib as L
    assert ENTRY in L.EXT_SIGNATURES and ENTRY not in L.SIGNATURES and ENTRY not in L.FAST
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]


def test_abi_version_moved_with_the_entry_point():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 15


def _entry(pictures=1, B=1, H=16, W=16, boxes=1, labels=1, N=1, idents=1, scores=1, names=1, n_names=4, stride=8,
           palette=1, P=125, font=1, first=32, G=95, FW=5, FH=7, scale=2, t=3):
    """The non-null 'pointers' are the address 1: a launch would fault, so a clean non-zero return is the check itself."""
    from future_od.native import lib
    rc = getattr(lib.LIB, ENTRY)(pictures, B, H, W, boxes, labels, N, idents, scores, names, n_names, stride, palette, P,
                                 font, first, G, FW, FH, scale, t, None)
    return rc, lib.last_error()


@pytest.mark.parametrize("kw, text", [
    (dict(t=0), "thickness"), (dict(H=5), "thickness 3"), (dict(W=5), "thickness 3"),
    (dict(N=1025), "1025 labels"), (dict(N=-1), "-1 labels"), (dict(P=0), "palette"),
    (dict(scale=0), "scale 0"), (dict(scale=9), "scale 9"),
    (dict(FW=0), "font cell"), (dict(FW=9), "font cell"), (dict(FH=0), "font cell"), (dict(FH=17), "font cell"),
    (dict(first=-1), "glyphs"), (dict(G=0), "glyphs"), (dict(first=200, G=95), "glyphs"), (dict(first=0, G=257), "glyphs"),
    (dict(n_names=0), "name table"), (dict(stride=0), "name table"), (dict(stride=33), "name table"),
    (dict(pictures=None), "null"), (dict(font=None), "null"), (dict(boxes=None), "null"), (dict(labels=None), "null"),
    (dict(palette=None), "null"), (dict(B=0), "pictures"), (dict(B=65536), "pictures"),
])
def test_arguments_are_refused_before_any_launch(kw, text):
    from future_od.native import lib as L
    rc, err = _entry(**kw)
    assert rc == L.ERR_ARG and "render_labels" in err and text in err, (kw, rc, err)


def test_nothing_to_draw_is_no_launch():
    """N == 0, or no operand that gives a text: success with the address 1 for every pointer, so nothing was launched."""
    from future_od.native import lib as L
    assert _entry(N=0)[0] == L.OK and _entry(N=0, boxes=None, labels=None, palette=None)[0] == L.OK
    assert _entry(idents=None, scores=None, names=None)[0] == L.OK


def test_wrapper_has_no_cpu_fallback():
    from future_od.native import lib as L
    from future_od.native import ops
    with pytest.raises(L.FodError, match="render_labels.*no CPU fallback"):
        ops.render_labels(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 0, 4),
                          torch.zeros(1, 0, dtype=torch.int32), palette=torch.zeros(4, 3, dtype=torch.uint8), font=V.FONT_5X7)


# ---- the text ----------------------------------------------------------------------------------------------------------
NAMES = torch.from_numpy(LC.NAMES)


@pytest.mark.parametrize("ident, label, score, names, want", [
    (0, 0, None, None, b"0"), (9, 0, None, None, b"9"), (10, 0, None, None, b"10"), (999, 0, None, None, b"999"),
    (1023, 0, None, None, b"1023"), (-1, 0, None, None, b""), (None, 0, None, None, b""),
    (None, 0, 0.0, None, b"00"), (None, 0, 0.07, None, b"07"), (None, 0, 0.995, None, b"99"), (None, 0, 1.0, None, b"99"),
    (None, 0, 7.0, None, b"99"), (None, 0, -1.0, None, b"00"), (None, 0, float("inf"), None, b"99"),
    (None, 0, float("-inf"), None, b"00"), (None, 0, float("nan"), None, b""), (None, 0, 0.5, None, b"50"),
    (None, 0, 0.289, None, b"28"),                    # truncated, not rounded
    (None, 0, None, NAMES, b"car"), (None, 8, None, NAMES, b""), (None, -1, None, NAMES, b""),
    (3, 8, 0.5, NAMES, b"3 50"),                      # a label outside the name table: the part is absent
    (3, 3, 0.5, NAMES, b"3  50"),                     # an empty name is present: its space stays
    (-1, 0, float("nan"), NAMES, b"car"),
    (17, 1, 0.875, NAMES, b"17 ConstructionVehicle 87"),
    (None, 1, None, NAMES, b"ConstructionVehicle"),
    (None, 4, None, NAMES, LC.LONG_NAME.encode()),    # a row without a 0 is `stride` bytes long
    (5, 4, 0.5, NAMES, b"5 " + LC.LONG_NAME.encode()[:30]),                       # cut at 32
    (1023, 1, 0.5, NAMES, b"1023 ConstructionVehicle 50"),
    (2147483647, 1, 0.5, NAMES, b"2147483647 ConstructionVehicle 5"),             # cut inside the score
])
def test_label_text(ident, label, score, names, want):
    assert V.label_text(ident, label, score, names) == want
    assert len(want) <= V.LABEL_MAX_CHARS == LC.MAX_CHARS == 32
    assert LC.text_of(ident, label, score, None if names is None else names.numpy()) == want
    if score is not None:                             # a tensor element, as draw_labels hands it in
        assert V.label_text(ident, label, torch.tensor([score], dtype=torch.float32)[0], names) == want


def test_encode_names():
    table = V.encode_names(["car", "ConstructionVehicle", ""])
    assert table.dtype == torch.uint8 and tuple(table.shape) == (3, 19)
    assert bytes(table[0].tolist()) == b"car" + bytes(16) and bytes(table[1].tolist()) == b"ConstructionVehicle"
    table = V.encode_names({0: "a", 2: "x" * 40})
    assert tuple(table.shape) == (3, 32) and bytes(table[1].tolist()) == bytes(32) and bytes(table[2].tolist()) == b"x" * 32
    assert tuple(V.encode_names({}).shape) == (1, 1) and tuple(V.encode_names([]).shape) == (1, 1)
    assert np.array_equal(V.encode_names(LC.NAME_LIST).numpy(), LC.NAMES)


# ---- the font ----------------------------------------------------------------------------------------------------------
def test_font_5x7():
    font = V.FONT_5X7
    assert font.dtype == torch.uint8 and tuple(font.shape) == (95, 7)
    assert int((font & 7).max()) == 0                 # the glyph lies in bits 7..3
    assert int(font[0].max()) == 0                    # space
    rows = [tuple(g) for g in font.tolist()]
    assert all(any(g) for g in rows[1:]) and len(set(rows)) == 95


def test_font_file_shows_the_font():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from font_art import font_art
    finally:
        sys.path.pop(0)
    art = font_art(V.FONT_5X7)
    assert open(os.path.join(ROOT, "profiles", "font_5x7.txt")).read() == art
    assert "code 65 'A'\n.###.\n#...#\n#...#\n#...#\n#####\n#...#\n#...#\n" in art


# ---- the CPU form ------------------------------------------------------------------------------------------------------
def test_the_restatement_paints_what_it_says():
    """Pixels worked out by hand: the text "1" at scale 2, thickness 1, on a 30 x 24 picture; box corner (9, 20)."""
    img = np.full((30, 24, 3), 7, dtype=np.uint8)
    LC.paint(img, np.array([[9, 20, 20, 28]], dtype=np.float32), [124], np.array([1]), None, None, LC.PALETTE,
             V.FONT_5X7.numpy(), 32, 5, 2, 1)
    # Wp = (1 * 6 + 1) * 2 = 14, Hp = 9 * 2 = 18; x0 = 9 - 1 = 8, y0 = 20 - 1 - 18 = 1
    plate = np.zeros((30, 24), dtype=bool)
    plate[1:19, 8:22] = True
    assert np.array_equal((img != 7).any(axis=2), plate)
    ink = np.zeros((30, 24), dtype=bool)
    glyph = ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."]
    for v, row in enumerate(glyph):
        for col, mark in enumerate(row):
            if mark == "#":
                ink[1 + 2 * (1 + v):1 + 2 * (2 + v), 8 + 2 * (1 + col):8 + 2 * (2 + col)] = True
    assert np.array_equal((img == 0).all(axis=2), ink)                    # white plate: black ink
    assert np.array_equal((img == 255).all(axis=2), plate & ~ink)


def _draw(case, b):
    picture = torch.from_numpy(case["picture"][b].copy())
    pick = lambda key: None if case[key] is None else torch.from_numpy(case[key][b])
    got = V.draw_labels(picture, torch.from_numpy(case["boxes"][b]), torch.from_numpy(case["labels"][b]), pick("idents"),
                        pick("scores"), _t(case["names"]), torch.from_numpy(case["palette"]), torch.from_numpy(case["font"]),
                        case["font_first"], case["font_width"], case["scale"], case["thickness"])
    assert got is picture
    return got.numpy()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_draw_labels_equals_the_restatement(case):
    want = LC.expected(case)
    for b in range(want.shape[0]):
        assert np.array_equal(_draw(case, b), want[b]), b


def captions_of(case):
    """(Captions, palette as `render` takes it) of a case."""
    captions = V.Captions(names=_t(case["names"]), ident=_t(case["idents"]), scores=_t(case["scores"]), scale=case["scale"],
                          font=torch.from_numpy(case["font"]), font_first=case["font_first"], font_width=case["font_width"])
    palette = V.COLOURS if case["palette"] is LC.PALETTE else torch.from_numpy(case["palette"]).float() / 255   # 0 and 255 only
    return captions, palette


def clip_of(case):
    return torch.from_numpy(LC.clip_of(case))


@pytest.mark.parametrize("case", [c for c in CASES if c["labels"].shape[1] <= 300],
                         ids=[c["name"] for c in CASES if c["labels"].shape[1] <= 300])
def test_cpu_render_with_captions_equals_the_restatement(case):
    captions, palette = captions_of(case)
    got = V.render(clip_of(case), torch.from_numpy(case["boxes"]), torch.from_numpy(case["labels"]), None, case["thickness"],
                   palette, captions=captions)
    assert got.dtype == torch.uint8 and got.is_contiguous()
    assert np.array_equal(got.numpy(), LC.expected_over_outlines(case))


def test_render_without_captions_is_unchanged():
    case = next(c for c in CASES if c["name"].startswith("two samples 40x300"))
    args = (clip_of(case), torch.from_numpy(case["boxes"]), torch.from_numpy(case["labels"]))
    plain = V.render(*args)
    assert torch.equal(V.render(*args, captions=None), plain)
    assert not torch.equal(V.render(*args, captions=V.Captions(ident="slot")), plain)


def test_ident_slot_numbers_the_positions_and_render_detections_takes_query_and_scores():
    case = next(c for c in CASES if c["name"].startswith("two samples 24x40"))
    video = clip_of(case)
    boxes, labels = torch.from_numpy(case["boxes"]), torch.from_numpy(case["labels"])
    B, K = labels.shape
    slots = torch.arange(K, dtype=torch.int32)[None].expand(B, K)
    assert torch.equal(V.render(video, boxes, labels, captions=V.Captions(ident="slot")),
                       V.render(video, boxes, labels, captions=V.Captions(ident=slots)))
    det = {"scores": torch.linspace(0.05, 0.95, B * K).view(B, K), "labels": labels.clamp(0, 124), "boxes": boxes,
           "query": torch.from_numpy(case["idents"]).clamp_min(0), "count": torch.tensor([K, K - 3], dtype=torch.int32)}
    shown = det["labels"].masked_fill((det["scores"] < 0.5) | (torch.arange(K)[None] >= det["count"][:, None]), -1)
    names = LC.NAME_LIST
    for ident, idents in (("slot", slots), ("query", det["query"])):
        got = V.render_detections(video, det, captions=V.Captions(names=names, ident=ident, scores=True))
        want = V.render(video, boxes, shown, captions=V.Captions(names=names, ident=idents, scores=det["scores"]))
        assert torch.equal(got, want) and not torch.equal(got, V.render_detections(video, det))
    with pytest.raises(ValueError, match="query"):
        V.render(video, boxes, labels, captions=V.Captions(ident="query"))
    with pytest.raises(ValueError, match="scores"):
        V.render(video, boxes, labels, captions=V.Captions(scores=True))
    with pytest.raises(ValueError, match="ident"):
        V.Captions(ident="index")


def test_draw_labels_checks_its_arguments():
    picture = torch.zeros(12, 12, 3, dtype=torch.uint8)
    boxes, labels = torch.tensor([[2.0, 2, 8, 8]]), torch.tensor([1])
    for kw in (dict(scale=0), dict(scale=9), dict(thickness=0), dict(thickness=7), dict(font_width=9),
               dict(font_first=200), dict(font=torch.zeros(3, 17, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="draw_labels"):
            V.draw_labels(picture, boxes, labels, torch.tensor([1]), **kw)


def test_trainer_has_the_switch_and_keeps_its_constructor():
    import inspect
    from future_od.trainer import Trainer
    assert "captions" not in inspect.signature(Trainer.__init__).parameters
    assert list(inspect.signature(Trainer.set_captions).parameters) == ["self", "flag"]
