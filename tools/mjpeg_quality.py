#!/usr/bin/env python3
"""PSNR and size of the Motion-JPEG stream contract against Pillow's encoder (libjpeg-turbo), per case: the
figures behind the bars of tests/test_mjpeg_host.py.  Host only: the streams come from the NumPy restatement
(tests/mjpeg_cases.py), which the GPU tests prove byte-equal to the kernels' output.

    python tools/mjpeg_quality.py [--out profiles/mjpeg_quality.json]

``quality_cases``: the cases the test holds to its bars (PSNR >= Pillow's - 0.5 dB, size <= 1.06 x Pillow's).
``byte_equality_cases``: the same figures for the GPU tests' case list, for the record only: a 24-row frame pads
a third of its luma blocks, which libjpeg codes as dummies and this contract as replicated pixels."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import s2v_import  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_quality.json"))
    a = ap.parse_args()
    import PIL

    import mjpeg_cases as MC
    import test_mjpeg_host as T

    def rows(cases):
        out = []
        for c in cases:
            ours, theirs, ratio = T.figures(c)
            fin = ours != float("inf") and theirs != float("inf")
            out.append({"case": MC.case_id(c), "images": T.phases(c),
                        "psnr_db": None if ours == float("inf") else round(ours, 3),
                        "pillow_psnr_db": None if theirs == float("inf") else round(theirs, 3),
                        "psnr_gap_db": round(ours - theirs, 3) if fin else None, "size_ratio": round(ratio, 4)})
        return out
    q, b = rows(MC.QUALITY_CASES), rows(MC.CASES)
    res = {"pillow": PIL.__version__, "bars": {"psnr_gap_db_min": -0.5, "size_ratio_max": 1.06},
           "psnr_null": "lossless: no error against the source",
           "worst_quality_case": {"psnr_gap_db": min(r["psnr_gap_db"] for r in q),
                                  "size_ratio": max(r["size_ratio"] for r in q)},
           "quality_cases": q, "byte_equality_cases": b}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["worst_quality_case"]), "->", a.out)


if __name__ == "__main__":
    main()
