#!/usr/bin/env python3
"""Writes tests/golden/fonts/: the three Inter faces the reference bundles (smelter-render/fonts/*.ttf, SIL OFL 1.1, no reserved font
name), cut down to the characters the text tests lay out.

  python tests/golden/gen_font_fixtures.py --reference <smelter checkout>

Subset with fontTools: Basic Latin, Latin-1, Latin Extended-A and General Punctuation (every string of tests/test_text_capi.py), every
name record and every layout feature (GPOS kern pairs included), hinting removed — the faces hold outlines, metrics and lookup tables
only, no TrueType instructions (neither reader here executes them).  Run once; the output is committed.
"""
import argparse
import os
import shutil

from fontTools import subset

FACES = ("Inter_18pt-Bold.ttf", "Inter_18pt-Italic.ttf", "Inter_18pt-Regular.ttf")
UNICODES = list(range(0x20, 0x7F)) + list(range(0xA0, 0x180)) + list(range(0x2000, 0x2070))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fonts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the smelter checkout")
    args = ap.parse_args()
    src = os.path.join(args.reference, "smelter-render", "fonts")
    os.makedirs(OUT, exist_ok=True)
    opts = subset.Options()
    opts.hinting = False
    opts.name_IDs = ["*"]
    opts.name_languages = ["*"]
    opts.notdef_outline = True
    opts.glyph_names = True
    for face in FACES:
        font = subset.load_font(os.path.join(src, face), opts)
        sub = subset.Subsetter(opts)
        sub.populate(unicodes=UNICODES)
        sub.subset(font)
        assert not {"fpgm", "prep", "cvt "} & set(font.keys()), face
        subset.save_font(font, os.path.join(OUT, face), opts)
        print(face, os.path.getsize(os.path.join(OUT, face)), "bytes")
    shutil.copyfile(os.path.join(src, "LICENSE-Inter.txt"), os.path.join(OUT, "LICENSE-Inter.txt"))


if __name__ == "__main__":
    main()
