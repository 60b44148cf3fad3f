"""Inputs and CPU references for the detector's tail (detect_post.hip): the decode / gather kernels and the NMS kernels.

Decode: logits are multiples of 0.25 in [-8, 8] (bf16-representable, so the f32, bf16 and sparse modes see the same numbers); objectness
logits stay in [-4, 8] so that two different class logits of one anchor always give scores more than 1e-6 apart (the smallest step of
sigmoid on the grid is 9.5e-5 at +-8, the smallest objectness 0.018).  The reference is float64 NumPy: Detect.forward (inference) + the
filter of non_max_suppression with multi_label=False and first-maximum argmax.  Anchors whose best score falls within 1e-3 of conf
are redrawn by the builder, so no candidate's membership depends on rounding and none has to be left out of a comparison.

NMS: box corners on a quarter-pixel grid, sizes up to 200 px, classes up to 79: the class-offset add, the areas and the unions are exact
in float32 and only the division rounds.  The reference is oracle.yolov5.box_iou_greedy_nms (float32) + scale_coords;
`nms_keep64` is the float64 greedy walk tests/test_detect_post_cases.py holds it against.

tests/test_detect_post_cases.py asserts the builders' conditions on the CPU; tests/test_gpu_detect_post.py runs the kernels on them."""
import functools

import numpy as np

from oracle import yolov5 as oy

ANCHORS = np.asarray(oy.ANCHORS, dtype=np.float64).reshape(3, 3, 2)
STRIDES = (8, 16, 32)
CONF = 0.25
MARGIN = 1e-3          # no objectness and no best class score within this of CONF (float64)
CLS_GAP = 1e-6         # two class scores of an anchor: equal logits or further apart than this


def lcs_of(nc):
    return (3 * (nc + 5) + 7) // 8 * 8


def _sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def _draw(rng, lo, hi, size=None):
    """multiples of 0.25 in [lo, hi]"""
    return rng.integers(int(round(lo * 4)), int(round(hi * 4)) + 1, size=size) * 0.25


class DecodeCase:
    """name, nc, shapes ((ny, nx) per level), max_cand, logits (three float32 [B][ny][nx][lcs]), planted (dict of notes for the tests)"""

    def __init__(self, name, nc, shapes, max_cand, logits, planted=None):
        self.name, self.nc, self.shapes, self.max_cand, self.logits, self.planted = name, nc, shapes, max_cand, logits, planted or {}
        self.B = logits[0].shape[0]
        self.bases = np.cumsum([0] + [3 * ny * nx for ny, nx in shapes])

    def anchors(self, level):
        """[B][3][ny][nx][nc + 5]: a level's logits in the reference's (anchor, y, x) order (a copy)"""
        ny, nx = self.shapes[level]
        no = self.nc + 5
        return self.logits[level][..., :3 * no].reshape(self.B, ny, nx, 3, no).transpose(0, 3, 1, 2, 4)

    def locate(self, idx):
        """flattened prediction index -> (level, a, y, x)"""
        level = int(np.searchsorted(self.bases, idx, side="right") - 1)
        ny, nx = self.shapes[level]
        li = idx - self.bases[level]
        return level, li // (ny * nx), (li // nx) % ny, li % nx


def _near_conf(obj_logit, cls_logits):
    best = (_sig(cls_logits) * _sig(obj_logit)[..., None]).max(-1)
    return np.abs(best - CONF) <= MARGIN


def random_decode_case(name, seed, B, nc, shapes, max_cand, pixel_p, anchor_p=0.6, cls_pass_p=0.7, all_pass=False):
    """pixel_p: per frame, the share of pixels with at least one passing objectness."""
    rng = np.random.default_rng(seed)
    no, lcs = nc + 5, lcs_of(nc)
    pixel_p = np.broadcast_to(np.asarray(pixel_p, dtype=np.float64), (B,))
    logits = []
    for ny, nx in shapes:
        arr = np.zeros((B, ny, nx, lcs), np.float32)                  # channels past 3 * no stay zero
        v = np.zeros((B, ny, nx, 3, no), np.float32)
        pix = rng.random((B, ny, nx)) < pixel_p[:, None, None]
        anc = rng.random((B, ny, nx, 3)) < anchor_p
        forced = rng.integers(0, 3, (B, ny, nx))
        anc |= np.arange(3) == forced[..., None]
        anc &= pix[..., None]
        cls_ok = rng.random((B, ny, nx, 3)) < cls_pass_p
        v[..., 0:4] = _draw(rng, -8, 8, (B, ny, nx, 3, 4))
        obj = np.where(anc, _draw(rng, 1 if all_pass else -1, 8, anc.shape), _draw(rng, -4, -1.25, anc.shape))
        cls = np.where(cls_ok[..., None], _draw(rng, -8, 8, (B, ny, nx, 3, nc)), _draw(rng, -8, -2, (B, ny, nx, 3, nc)))
        hot = rng.integers(0, nc, (B, ny, nx, 3))
        hot_v = _draw(rng, 1 if all_pass else 2, 8, hot.shape)
        sel = (np.arange(nc) == hot[..., None]) & (cls_ok | all_pass)[..., None]
        cls = np.where(sel, hot_v[..., None], cls)
        for _ in range(64):                                           # best score too close to conf: redraw that anchor's classes
            bad = _near_conf(obj, cls)
            if not bad.any():
                break
            cls[bad] = _draw(rng, -8, 8, (int(bad.sum()), nc))
        else:
            raise AssertionError("could not separate the scores from conf")
        v[..., 4] = obj
        v[..., 5:] = cls
        arr[..., :3 * no] = v.reshape(B, ny, nx, 3 * no)
        logits.append(arr)
    return DecodeCase(name, nc, shapes, max_cand, logits)


def _quiet(case):
    """every anchor's objectness below conf (redrawn from the failing range, seeded by the case's shape)"""
    rng = np.random.default_rng(case.B * 1000 + case.nc)
    for level in range(3):
        for a in range(3):
            case.logits[level][..., a * (case.nc + 5) + 4] = _draw(rng, -4, -1.25, case.logits[level].shape[:3])


def _plant(case, frame, idx, obj, cls_logits, box=None):
    level, a, y, x = case.locate(idx)
    row = case.logits[level][frame, y, x]
    c0 = a * (case.nc + 5)
    row[c0 + 4] = obj
    row[c0 + 5:c0 + 5 + case.nc] = cls_logits
    if box is not None:
        row[c0:c0 + 4] = box


@functools.lru_cache(maxsize=None)
def decode_cases():
    """name -> DecodeCase.  Built once; the tests must not write into the logits."""
    cases = []
    tiny = ((4, 4), (2, 2), (1, 1))
    # 63 anchors per frame: a 128-anchor run of decode_sparse_kernel spans three frames and all three levels; M = 144 / 36 / 9 leave
    # partial waves in head_compact_kernel
    cases.append(random_decode_case("tiny", 11, 9, 3, tiny, 64, 1.0, anchor_p=1.0, all_pass=True))
    cases.append(random_decode_case("ragged", 12, 5, 80, ((12, 20), (6, 10), (3, 5)), 1024, [0.3, 0.0, 0.3, 1.0, 0.3]))
    for nc in (3, 59, 80, 123, 251):                                  # C / 8 = 3, 24, 32, 48, 96 chunks per gathered row
        cases.append(random_decode_case(f"width_nc{nc}", 20 + nc, 3, nc, ((5, 7), (3, 4), (2, 2)), 256, 0.5))
    big = ((40, 40), (20, 20), (10, 10))
    cases.append(random_decode_case("passes4", 13, 8, 8, big, 8192, 1.0, cls_pass_p=0.25))          # 50 400 gathered anchors: passes = 4
    cases.append(random_decode_case("round2", 14, 32, 8, big, 8192, 1.0, cls_pass_p=0.25))          # 201 600 > 8 * 16 * 1024: second round

    # class ties: equal logits, the smaller class wins.  Lane of class c in decode_sparse_kernel's reduction = c % 16.
    c = random_decode_case("ties", 15, 2, 80, tiny, 64, 1.0, anchor_p=1.0, all_pass=True)
    pairs = [(5, 17), (17, 34), (15, 16), (3, 19), None]             # None: all classes equal
    rng = np.random.default_rng(150)
    planted = {}
    for frame in range(2):
        for k, idx in enumerate(range(0, 63, 4)):                     # 16 anchors per frame over the three levels
            pr = pairs[(k + frame) % len(pairs)]
            cl = _draw(rng, -8, 2, 80)
            if pr is None:
                cl[:] = 1.0
            else:
                cl[list(pr)] = 4.0
            _plant(c, frame, idx, 2.0, cl)
            planted[(frame, idx)] = 0 if pr is None else min(pr)
    c.planted = planted
    cases.append(c)

    # edges of the value range, nc = 3, one frame
    c = random_decode_case("edges", 16, 1, 3, tiny, 64, 1.0, anchor_p=1.0, all_pass=True)
    _plant(c, 0, 0, 2.0, [-2.0, -2.0, -2.0])                          # objectness passes, best class fails
    _plant(c, 0, 50, 2.0, [-8.0, -2.0, -4.0])                         # (level 1)
    _plant(c, 0, 5, 2.0, [4.0, 0.0, 0.0], box=[0.0, 0.0, -8.0, -8.0])   # tiny box
    _plant(c, 0, 21, 2.0, [0.0, 4.0, 0.0], box=[1.0, -1.0, 8.0, 8.0])   # largest box
    _plant(c, 0, 52, 2.0, [0.0, 0.0, 4.0], box=[-8.0, 8.0, 8.0, -8.0])
    _plant(c, 0, 7, 2.0, [4.0, 0.0, 0.0], box=[0.5, 0.25, -200.0, -200.0])    # sigmoid -> 0 in float32: zero-area box
    _plant(c, 0, 61, 2.0, [0.0, 4.0, 0.0], box=[-1.0, 2.0, -200.0, 3.0])      # zero width only (level 2)
    c.planted = {"class_fails": [0, 50], "zero_w": [7, 61], "zero_h": [7]}
    cases.append(c)

    # overflow: max_cand = 64; 10, exactly 64 and 70 candidates
    c = random_decode_case("overflow", 17, 3, 3, ((8, 8), (4, 4), (2, 2)), 64, 1.0, anchor_p=1.0, all_pass=True)
    _quiet(c)
    rng = np.random.default_rng(170)
    for frame, k in enumerate((10, 64, 70)):
        for idx in rng.choice(252, k, replace=False):
            _plant(c, frame, int(idx), float(_draw(rng, 1, 8)), np.concatenate([_draw(rng, 2, 8, 1), _draw(rng, -8, 1, 2)])[rng.permutation(3)])
    c.planted = {"counts": [10, 64, 70]}
    cases.append(c)
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def decode_ref(name):
    """float64 Detect.forward + candidate filter.  Per frame: idx (ascending), cls, box [n][4], conf, scale [n] (the coordinate scale of the
    tolerance: stride * (nx + 2) of the anchor's level); `gathered`: per level the sorted pixel indices with any objectness > conf;
    `obj` / `best`: every anchor's objectness and best class score (for the builder-condition tests)."""
    case = decode_cases()[name]
    rows = [[] for _ in range(case.B)]
    gathered, objs, bests = [], [], []
    for level, (ny, nx) in enumerate(case.shapes):
        t = _sig(case.anchors(level))                            # [B][3][ny][nx][no]
        yv, xv = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        cx = (t[..., 0] * 2.0 - 0.5 + xv) * STRIDES[level]
        cy = (t[..., 1] * 2.0 - 0.5 + yv) * STRIDES[level]
        w = (t[..., 2] * 2.0) ** 2 * ANCHORS[level, :, 0][None, :, None, None]
        h = (t[..., 3] * 2.0) ** 2 * ANCHORS[level, :, 1][None, :, None, None]
        obj = t[..., 4]
        score = t[..., 5:] * obj[..., None]
        j = score.argmax(-1)                                          # first maximum
        best = np.take_along_axis(score, j[..., None], -1)[..., 0]
        keep = (obj > CONF) & (best > CONF)
        box = np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), -1)
        idx = case.bases[level] + np.arange(3 * ny * nx).reshape(3, ny, nx)
        for b in range(case.B):
            k = keep[b]
            rows[b].append((idx[k], j[b][k], box[b][k], best[b][k], np.full(int(k.sum()), float(STRIDES[level] * (nx + 2)))))
        gathered.append(np.flatnonzero((obj > CONF).any(1).reshape(-1)))     # [B][ny][nx] flattened = the kernel's pixel index
        objs.append(obj)
        bests.append(best)
    frames = []
    for b in range(case.B):
        frames.append({"idx": np.concatenate([r[0] for r in rows[b]]), "cls": np.concatenate([r[1] for r in rows[b]]),
                       "box": np.concatenate([r[2] for r in rows[b]]), "conf": np.concatenate([r[3] for r in rows[b]]),
                       "scale": np.concatenate([r[4] for r in rows[b]])})
    return {"frames": frames, "gathered": gathered, "obj": objs, "best": bests}


# ------------------------------------------------------------------------------------------------------------------------------ NMS
class NmsCase:
    """frames: list of (boxes [n][4] f32, conf [n] f32, cls [n] i32); geoms: per frame (net_h, net_w, src_h, src_w) or None"""

    def __init__(self, name, frames, iou=0.45, max_det=300, max_cand=8192, geoms=None, notes=None):
        self.name, self.frames, self.iou, self.max_det, self.max_cand, self.geoms, self.notes = name, frames, iou, max_det, max_cand, geoms, notes or {}

    @property
    def counts(self):
        return [len(f[1]) for f in self.frames]


def _frame(boxes, conf, cls):
    return (np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(conf, np.float32).reshape(-1), np.asarray(cls, np.int32).reshape(-1))


@functools.lru_cache(maxsize=None)
def rand_frame(seed, n, ncls, extent=640, smin=8, smax=200, lo=0):
    """n boxes with quarter-pixel corners: top-left in [lo, extent), sides in [smin, smax]"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(4 * lo, 4 * extent, (n, 2)) / 4.0
    wh = rng.integers(4 * smin, 4 * smax + 1, (n, 2)) / 4.0
    conf = rng.uniform(0.25, 1.0, n)
    cls = rng.integers(0, ncls, n)
    return _frame(np.concatenate([xy, xy + wh], 1), conf, cls)


def offset_boxes(boxes, cls):
    return (boxes + (cls[:, None].astype(np.float32) * np.float32(oy.MAX_WH)).astype(np.float32)).astype(np.float32)


def nms_keep32(frame, iou):
    """the float32 oracle's kept indices, all of them (no max_det cut)"""
    boxes, conf, cls = frame
    with np.errstate(invalid="ignore"):                               # 0 / 0 of two zero-area boxes: not > thr
        return oy.box_iou_greedy_nms(offset_boxes(boxes, cls), conf, iou)


def nms_keep64(frame, iou):
    """the same greedy walk in float64 with the float32-rounded threshold"""
    boxes, conf, cls = frame
    n = len(conf)
    if n == 0:
        return np.zeros((0,), np.int64)
    b = boxes.astype(np.float64) + cls[:, None].astype(np.float64) * float(oy.MAX_WH)
    order = np.argsort(-conf, kind="stable")
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr = float(np.float32(iou))
    dead = np.zeros(n, bool)
    keep = []
    for a in range(n):
        if dead[a]:
            continue
        keep.append(order[a])
        r = slice(a + 1, n)
        w = np.maximum(0.0, np.minimum(b[a, 2], b[r, 2]) - np.maximum(b[a, 0], b[r, 0]))
        h = np.maximum(0.0, np.minimum(b[a, 3], b[r, 3]) - np.maximum(b[a, 1], b[r, 1]))
        inter = w * h
        with np.errstate(invalid="ignore"):
            dead[r] |= inter / (area[a] + area[r] - inter) > thr
    return np.asarray(keep, dtype=np.int64)


def nms_rows(frame, keep, max_det, geom=None):
    """[x1, y1, x2, y2, conf, cls] float32 of the first max_det kept boxes, through scale_coords when the frame has a geometry"""
    boxes, conf, cls = frame
    k = keep[:max_det]
    rows = np.concatenate([boxes[k], conf[k, None], cls[k, None].astype(np.float32)], 1).astype(np.float32).reshape(-1, 6)
    if geom is not None and len(rows):
        rows[:, :4] = oy.scale_coords((geom[0], geom[1]), rows[:, :4], (geom[2], geom[3]))
    return rows


COUNT_EDGES = (0, 1, 63, 64, 65, 512, 513, 4096, 4097, 8192)
ACROSS_RANKS = (1, 63, 64, 127, 128, 511, 512, 4095, 4096, 8191)


# (classes, extent, smallest side) of the large frames.  512 / 513 / 4096 keep more than max_det = 300; 4097 and 8192 are dense enough to
# keep fewer, so the walk reaches their last word and every keep / drop above candidate 4096 shows in the output.
_EDGE_DENSITY = {513: (80, 160, 60), 4096: (80, 160, 60), 4097: (3, 200, 80), 8192: (2, 300, 80)}


def count_edge_frame(i):
    """frame i of the count-edge batch"""
    ncls, extent, smin = _EDGE_DENSITY.get(COUNT_EDGES[i], (3, 640, 40))
    return rand_frame(100 + i, COUNT_EDGES[i], ncls, extent, smin)


def _across_words():
    """8192 candidates; copies of the top box with lower scores at the sorted ranks ACROSS_RANKS.  Returns (frame, frame without the
    copies, positions of the copies, position map from the copy-free frame)."""
    n = 8192
    boxes, _, cls = rand_frame(200, n - len(ACROSS_RANKS), 2, 300, 80)     # dense: fewer than max_det kept
    rng = np.random.default_rng(201)
    is_copy = np.zeros(n, bool)
    is_copy[list(ACROSS_RANKS)] = True
    sb, sc = np.zeros((n, 4), np.float32), np.zeros(n, np.int32)
    sb[~is_copy], sc[~is_copy] = boxes, cls
    sb[is_copy], sc[is_copy] = sb[0], sc[0]
    score = (1.0 - np.arange(n) / 16384.0).astype(np.float32)         # distinct in float32, rank r = position r
    perm = rng.permutation(n)                                         # candidate position p holds sorted rank perm[p]
    full = _frame(sb[perm], score[perm], sc[perm])
    plain_pos = np.flatnonzero(~is_copy[perm])
    plain = _frame(full[0][plain_pos], full[1][plain_pos], full[2][plain_pos])
    return full, plain, np.flatnonzero(is_copy[perm]), plain_pos


@functools.lru_cache(maxsize=None)
def nms_cases():
    cases = []
    edge = [count_edge_frame(i) for i in range(len(COUNT_EDGES))]
    for mc in (8192, 4096, 512, 64):                                  # the same frames at every capacity that holds them
        cases.append(NmsCase(f"counts_mc{mc}", [f for f in edge if len(f[1]) <= mc], max_cand=mc))

    # a capacity that is no multiple of rank_sort_kernel's 256-thread block, filled to the last slot
    cases.append(NmsCase("full_mc320", [rand_frame(330, 320, 3), rand_frame(331, 257, 80, 160, 60)], max_cand=320))

    # max_det cut: 130 disjoint boxes (a 13 x 10 lattice of 20 px boxes, 40 px apart), shuffled scores
    rng = np.random.default_rng(300)
    gx, gy = np.meshgrid(np.arange(13) * 40.0, np.arange(10) * 40.0)
    xy = np.stack([gx.reshape(-1), gy.reshape(-1)], 1) + 0.25
    lattice = _frame(np.concatenate([xy, xy + 20.0], 1), rng.permutation(130) / 256.0 + 0.3, rng.integers(0, 3, 130))
    for md in (1, 63, 64, 65, 128):
        cases.append(NmsCase(f"maxdet{md}", [lattice], max_det=md, max_cand=256))

    full, plain, copies, plain_pos = _across_words()
    cases.append(NmsCase("across_words", [full], notes={"plain": plain, "copies": copies, "plain_pos": plain_pos}))

    # one batch of small frames, iou 0.45
    small = []
    small.append(_frame([[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]], [0.9, 0.8, 0.7], [2, 2, 2]))           # greedy chain: A kills B, C stays
    b, _, c = rand_frame(310, 200, 3, extent=300)
    small.append(_frame(b, np.full(200, 0.5), c))                                                                # every score equal: idx order
    b, s, c = rand_frame(311, 200, 3, extent=300)
    small.append(_frame(b, np.floor(s * 64) / 64, c))                                                            # scores k / 64
    ids = np.array([0, 1, 2, 15, 16, 40, 77, 78, 79, 79])
    small.append(_frame(np.tile([[10.25, 20.5, 110.75, 90.0]], (10, 1)), 0.9 - np.arange(10) / 32.0, ids))       # one box, ten class ids (79 twice)
    b, s, _ = rand_frame(312, 300, 1, extent=200)
    small.append(_frame(b, s, np.where(np.arange(300) % 2 == 0, 79, 78)))                                        # dense boxes at the largest offsets
    small.append(_frame([[50, 60, 50, 60], [50, 60, 50, 60], [5, 5, 5, 9], [5, 5, 5, 9]], [0.9, 0.8, 0.7, 0.6], [1, 1, 79, 79]))   # 0 / 0 is not > thr
    cases.append(NmsCase("small", small, max_cand=512,
                         notes={"chain": 0, "equal": 1, "quantised": 2, "classes": 3, "cls79": 4, "degenerate": 5}))

    # threshold 0.5: pairs at IoU exactly 0.5 stay, pairs one quarter-pixel step above go
    boxes, conf, cls, pair_kept = [], [], [], []
    for k, (w, h, cl) in enumerate([(2, 1, 0), (100, 50, 3), (200, 100, 79), (64, 200, 41)]):
        for step, kept in ((0.0, True), (0.25, False)):
            ox, oy_ = 300.0 * (len(boxes) // 2 % 3), 250.0 * (len(boxes) // 2 // 3)
            boxes += [[ox, oy_, ox + w, oy_ + h], [ox, oy_, ox + w / 2 + step, oy_ + h]]
            conf += [0.9 - 0.01 * k, 0.6 - 0.01 * k]
            cls += [cl, cl]
            pair_kept.append(kept)
    cases.append(NmsCase("threshold", [_frame(boxes, conf, cls)], iou=0.5, max_cand=64, notes={"pair_kept": pair_kept}))

    # per-frame scale_coords geometry; boxes reach past every edge of the network frame
    geoms = [(384, 640, 720, 1280), (384, 640, 360, 640), (384, 640, 180, 320), (448, 640, 333, 500), (384, 640, 384, 640)]
    gframes = []
    for i, g in enumerate(geoms):
        b, s, c = rand_frame(320 + i, 200, 3, extent=g[1] + 150, smin=8, smax=200)
        gframes.append(_frame(b - np.float32(120.0), s, c))
    cases.append(NmsCase("geometry", gframes, max_cand=256, geoms=geoms))
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def _keep32_of_edge(i, iou):
    return nms_keep32(count_edge_frame(i), iou)


@functools.lru_cache(maxsize=None)
def nms_ref(name):
    """per frame: (all kept indices of the float32 oracle, the expected output rows)"""
    case = nms_cases()[name]
    out = []
    for f, frame in enumerate(case.frames):
        if name.startswith("counts_mc"):
            keep = _keep32_of_edge(COUNT_EDGES.index(len(frame[1])), case.iou)      # one walk per frame, shared by the four capacities
        else:
            keep = nms_keep32(frame, case.iou)
        out.append((keep, nms_rows(frame, keep, case.max_det, case.geoms[f] if case.geoms else None)))
    return out
