"""Shared by tests/test_yolov5x_host.py, tests/test_gpu_yolov5x.py and tests/golden/make_coded_golden_x.py: YOLOv5x
(depth 1.33, width 1.25: 80..1280 channels, 4-8-12-4 bottlenecks) registered with the oracle and with the coded clips.

oracle/yolov5.py lists s, m and l; its graph builder is a pure function of the (depth, width) pair, so the fourth variant
is one more row of data, added here at import time."""
import coded_case as cc
from oracle import yolov5 as oy

VARIANT = "yolov5x"
oy.VARIANTS.setdefault(VARIANT, (1.33, 1.25))

# YOLOv5x, 640 x 640 frames through the stream path.  T = 16: a track reaches the CSV from its N_INIT = 3rd frame on, so an object
# gives at most T - 2 = 14 rows.  n_obj = 12 like every other coded case: the GPU test's guard against an empty comparison asks for
# more than 8 T = 128 rows, which 8 objects (at most 112 rows) cannot give and 12 do (159).
cc.CASES.setdefault("x640", dict(variant=VARIANT, size=640, H=640, W=640, T=16, n_obj=12, seed=1702, zone="cam_04_halfres.json"))
