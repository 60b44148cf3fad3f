"""Generates tests/golden/coded_x640.json: the fp32 CPU oracle's CSV (oracle/pipeline.py::run_video) of the YOLOv5x clip that
tests/yolov5x_case.py adds to the coded cases.  Run from the repo root:  python tests/golden/make_coded_golden_x.py

Same recipe and same file layout as make_coded_golden.py (whose `main` does the work); this script only registers the variant
with the oracle first, and refuses to write a golden that the GPU test's own guard (more than 8 rows per frame) would reject."""
import make_coded_golden as mg          # puts the repo root and tests/ on sys.path

import coded_case as cc  # noqa: E402
import yolov5x_case  # noqa: E402,F401   (registers "yolov5x" with the oracle and "x640" with the coded cases)

if __name__ == "__main__":
    mg.main(["x640"])
    g = cc.load_golden("x640")
    assert len(g["rows"]) > 8 * cc.CASES["x640"]["T"], (len(g["rows"]), "rows: too few for the GPU test to compare anything")
