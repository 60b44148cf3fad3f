"""The nine-box scene of the detection hand-over tests and what the reference keeps of it, composed from the oracle alone
(oracle.yolov5.marshal_like_reference, oracle.deepsort.dsort_nms, the filter lines of DeepSortOracle.update).  Shared by
tests/test_det_prep_host.py (CPU: vehicle-counting_amd/csrc/det_prep.h compiled for the host) and tests/test_gpu_embed_kept.py (GPU: the
same header inside the library)."""
import numpy as np

from oracle import deepsort as od
from oracle import yolov5 as oy

NC = 3

# [x1, y1, x2, y2, conf, class] in frame 0; every box moves (+2, +1) pixels per frame, so the overlaps below hold in every frame.
# DeepSORT's overlap is intersection / area of the LOWER-scoring box with the +1 pixel convention, threshold '>' 0.5 (Q6).
BOXES = [
    (5, 5, 75, 95, 0.9, 0),        # 0 A: large, kept
    (20, 20, 50, 60, 0.8, 0),      # 1 B: nested in A, same class: overlap 1 -> dropped
    (20, 20, 50, 60, 0.8, 1),      # 2 B in another class: kept
    (10, 40, 110, 140, 0.5, 2),    # 3 low-confidence large box ...
    (40, 70, 70, 110, 0.95, 2),    # 4 ... around a high-confidence small one: 31 * 41 / (101 * 101) = 0.12 of the large box -> both kept
    (55, 30, 105, 70, 0.7, 0),     # 5 21 * 41 of its 51 * 41 pixels (41 %) inside A -> kept
    (100, 100, 130, 140, 0.25, 1),  # 6 conf == min_confidence: '>' fails -> dropped
    (85, 5, 135, 50, 0.6, 1),      # 7 equal confidence, different geometry, each suppresses the other (1.0 of box 8, 0.72 of box 7):
    (90, 8, 135, 48, 0.6, 1),      # 8 the stable ascending sort picks the later one; box 7 is dropped
]
DROPPED, KEPT_PER_FRAME = {1, 6, 7}, 6


def kept_of_label(det_f, label, min_conf, nms_overlap):
    """Box indices of one frame that the DeepSort.update of class `label` turns into Detections, in the order it creates them: the
    reference's filter on the rows marshalled like networks/yolo.py:72-97 (oracle.deepsort.DeepSortOracle.update lines :31-37)."""
    m = oy.marshal_like_reference(det_f)
    xywh, labels, scores = np.asarray(m["bboxes"], np.float64).reshape(-1, 4), np.asarray(m["classes"]), np.asarray(m["scores"], np.float64)
    idx = [i for i in np.flatnonzero(labels == label) if scores[i] > min_conf]
    keep = od.dsort_nms(xywh[idx], nms_overlap, scores[idx]) if idx else []      # xywh here is top-left + size = tlwh
    return [int(idx[k]) for k in keep]


def kept_indices(det_f, min_conf, nms_overlap, nc=NC):
    """The same over the classes 0 .. nc - 1, as sorted box indices."""
    return sorted(i for c in range(nc) for i in kept_of_label(det_f, c, min_conf, nms_overlap))
