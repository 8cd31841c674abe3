"""The caption font as text (profiles/font_5x7.txt): every glyph of visualization.FONT_5X7 as `#` / `.` art beside its
character and code, so that the font can be read without rendering a picture.

    python tools/font_art.py [--out FILE]

`font_art` reads the uint8 table the kernel is handed (one byte per glyph row, column col in bit 7 - col), not the
strings the table was made from: what the file shows is what fod_render_labels draws.  Needs no GPU."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "future-object-detection_amd")]


def font_art(font, first=32, width=5):
    """uint8 [G, FH] -> the text: per glyph a line `code <n> '<character>'`, then FH lines of `width` marks, then a
    blank line."""
    lines = []
    for g, rows in enumerate(font.tolist()):
        lines.append(f"code {first + g} '{chr(first + g)}'")
        lines += ["".join("#" if byte >> (7 - col) & 1 else "." for col in range(width)) for byte in rows]
        lines.append("")
    return "\n".join(lines)


def main():
    from future_od.utils.visualization import FONT_5X7
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "font_5x7.txt"))
    args = ap.parse_args()
    with open(args.out, "w") as f:
        f.write(font_art(FONT_5X7))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
