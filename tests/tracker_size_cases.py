"""Scenes that take the device tracker (track_kernels.hip, track_core.h, tracker.hip) to the LARGE side of its size switches, and the
proof, from the oracle alone, that each scene gets there.  Shared by tests/test_tracker_size_cases.py (CPU: every regime claim and the
margin condition) and tests/test_gpu_tracker_sizes.py (the kernels against oracle.deepsort on these scenes).  NumPy and the oracle only.

The switches (constants restated here, the kernels are not imported):
  gallery length 64      appearance_row_wave's second `s0 += 64` pass, appearance_row_dev's second round over its four waves,
                         appearance_row_table's repeated 16-entry unroll, track_plan_kernel's row numbers past 64 per slot
  D > VC_SMALL_D (12)    appearance_row_dev instead of appearance_row_wave when a tracker has no table
  D > 64                 appearance_row_table's `d0 += 64` loop
  T <= VC_STEP_STATE     the step's Kalman state in LDS (use_st) or in the pool
  T * D <= 512           cost rows in LDS (small_cost) or in the workgroup's scratch
  T + D <= cap           work arrays in LDS (w_lds) or in the scratch (w_glb); cap comes from the host's plan (walk_cap below)
  table fit              per tracker, against the arena (dot_arena_mb): some trackers of a launch with a table, some without

`Probe` is oracle.deepsort.TrackerState with a notebook: per step the sizes, and for every matched (track, detection) pair the PHYSICAL
ring position of the gallery sample that attains the minimum cosine distance.  The device writes every feature of a track into a ring
from the track's first detection on, so the k-th feature (0-based) sits at k % budget, and a track has received `hits` features.
With `noise_seed` it perturbs its appearance costs by +-NOISE instead: the margin condition (`regime(...)["margin_ok"]`) asks that three
such runs leave every id and FSM counter of every frame unchanged -- a condition on the scene, so that exact equality is a fair demand
of a kernel whose cosine costs differ from the oracle's in the last digits."""
import functools

import numpy as np

from oracle import deepsort as od

VC_SMALL_D, VC_STEP_STATE, SMALL_COST, TC_HARD_CAP = 12, 64, 512, 512
ARENA_FLOATS_PER_MB = 262144
FRAME_HW = (720, 1280)
NOISE = 1e-5              # five times the 2e-6 tolerance of the kernels' cosine rows
GAP = 1e-3                # a deep minimum counts when the runner-up sample is at least this much farther (500 x the tolerance)
K_ARC = 16                # frames per quarter of a great circle: consecutive samples are 1 - cos(pi / 32) = 4.8e-3 apart


def walk_cap(dmax, known_tracks=0):
    """TrackBatchArgs::cap as track_batch_plan.h::plan_track_batch sizes it: need = max(8, 2 * known_tracks + 2 * dmax + 16) over the
    launch's trackers (known_tracks: the tracker's size at its last collect, dmax: its largest step of the launch), then 32 when
    need <= 32, else need rounded up to a multiple of 64, at most TC_HARD_CAP."""
    need = max(8, 2 * known_tracks + 2 * dmax + 16)
    return 32 if need <= 32 else min(TC_HARD_CAP, (need + 63) // 64 * 64)


def table_need(old_rows, dets):
    """Floats of one tracker's appearance table: (gallery rows it holds + the launch's detections) x the launch's detections
    (track_plan_kernel; plan_track_batch bounds old_rows by known_tracks * budget)."""
    return (old_rows + dets) * dets


# ------------------------------------------------------------------------------------------------ the oracle with a notebook
class Probe(od.TrackerState):
    def __init__(self, p, noise_seed=None):
        super().__init__(p["max_dist"], p["budget"], max_iou_distance=p["max_iou_distance"], max_age=p["max_age"], n_init=p["n_init"])
        self.rng = None if noise_seed is None else np.random.default_rng(noise_seed)
        self.steps, self.trace, self._near = [], [], {}

    def _appearance_cost(self, dets, tidx, didx):
        cost = super()._appearance_cost(dets, tidx, didx)
        if self.rng is not None:
            return np.where(cost != od.GATED_COST, cost + self.rng.uniform(-NOISE, NOISE, cost.shape), cost)
        f = np.array([dets[i]["feature"] for i in didx], np.float64)
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        for r, k in enumerate(tidx):
            t = self.tracks[k]
            g = np.asarray(self.gallery[t.tid], np.float64)
            g /= np.linalg.norm(g, axis=1, keepdims=True)
            dist = 1.0 - g @ f.T                                           # [samples, detections]
            j = dist.argmin(axis=0)
            srt = np.sort(dist, axis=0)
            gap = srt[1] - srt[0] if len(g) > 1 else np.full(len(didx), np.inf)
            first = t.hits - len(g)                                        # insertion number of the oldest sample still held
            for c, d in enumerate(didx):
                self._near[(k, d)] = ((first + int(j[c])) % self.budget, float(gap[c]), float(cost[r, c]))
        return cost

    def update(self, dets):
        T, D = len(self.tracks), len(dets)
        tsu = [t.tsu for t in self.tracks]                                 # after predict(): 1 = seen in the last frame
        self._near = {}
        super().update(dets)
        near = [self._near[m] for m in self.last_matches if m in self._near and self._near[m][2] <= self.max_cos]
        self.steps.append({"T": T, "D": D, "deep": any(pos >= 64 and gap >= GAP for pos, gap, _ in near),
                           "deep_any": any(pos >= 64 for pos, _, _ in near),
                           "gallery": max([len(g) for g in self.gallery.values()], default=0),
                           "wraps": max([t.hits // self.budget for t in self.tracks], default=0),
                           "ring_rows": sum(min(t.hits, self.budget) for t in self.tracks),
                           "reid": sum(tsu[k] > 1 for k, _ in self.last_matches)})       # matches only the cascade's appearance rows can make
        self.trace.append(state_of(self))


def state_of(trk):
    """What the device's tracker_state must equal exactly, as plain tuples."""
    tr = trk.tracks
    return (tuple(t.tid for t in tr), tuple(t.state for t in tr), tuple(t.hits for t in tr), tuple(t.age for t in tr), tuple(t.tsu for t in tr),
            tuple(len(trk.gallery.get(t.tid, [])) for t in tr))


def sizes(steps):
    T, D = np.array([s["T"] for s in steps]), np.array([s["D"] for s in steps])
    return {"T": T, "D": D, "reid": np.array([s["reid"] for s in steps]), "max_T": int(T.max()), "max_D": int(D.max()), "max_TD": int((T * D).max()), "max_T_plus_D": int((T + D).max()),
            "gallery": max(s["gallery"] for s in steps), "wraps": max(s["wraps"] for s in steps),
            "deep_steps": sum(s["deep"] for s in steps), "deep_any_steps": sum(s["deep_any"] for s in steps)}


def crosses(flags):
    """True when a step on the small side (flag set) is followed, later in the walk, by one on the large side."""
    flags = np.asarray(flags, bool)
    return bool(flags.any() and (~flags[int(np.argmax(flags)):]).any())


# ------------------------------------------------------------------------------------------------ scene pieces
def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _layout(rng, n, cols, rows, wh_lo, wh_hi, vmax, W=FRAME_HW[1], H=FRAME_HW[0]):
    """n objects in distinct cells of a cols x rows grid over W x H: start centres, velocities, box sizes."""
    cell = rng.permutation(cols * rows)[:n]
    cw, ch = W / cols, H / rows
    pos = np.stack([(cell % cols + 0.5) * cw, (cell // cols + 0.5) * ch], axis=1) + rng.uniform(-0.1, 0.1, (n, 2)) * [cw, ch]
    return pos, rng.uniform(-vmax, vmax, (n, 2)), rng.uniform(wh_lo, wh_hi, (n, 2))


def _det(rng, c, wh, feat):
    c = c + rng.normal(0, 0.5, 2)
    s = wh * (1 + rng.normal(0, 0.01, 2))
    return {"tlwh": np.concatenate([c - s / 2, s]), "conf": float(rng.uniform(0.3, 0.99)), "feature": feat}


def _clutter(rng, k, W=FRAME_HW[1], H=FRAME_HW[0]):
    return [{"tlwh": np.concatenate([rng.uniform([0, 0], [W - 60, H - 60]), rng.uniform([20, 20], [50, 50])]), "conf": float(rng.uniform(0.3, 0.9)),
             "feature": _unit(rng.standard_normal(512))} for _ in range(k)]


def _protos(rng, n, twin_share=0.2):
    pr = _unit(rng.standard_normal((n, 512)))
    tw = np.nonzero(rng.random(n) < twin_share)[0]
    for i in tw[1:]:
        pr[i] = pr[tw[0]]                                                  # look-alikes: the appearance is ambiguous, the gate decides
    return pr


class _ArcPath:
    """An appearance that drifts along great-circle arcs: K_ARC frames from one direction of an orthonormal set to the next.  Phases on
    different arcs are far apart, so the path never comes back by itself -- only where the scene says so."""

    def __init__(self, rng, n_phases):
        q, _ = np.linalg.qr(rng.standard_normal((512, n_phases // K_ARC + 2)))
        self.e = q.T

    def at(self, phase):
        seg, a = phase // K_ARC, (phase % K_ARC) / K_ARC * (np.pi / 2)
        return np.cos(a) * self.e[seg] + np.sin(a) * self.e[seg + 1]


# ------------------------------------------------------------------------------------------------ deep galleries
def _deep(seed, budget, n, frames, grid):
    """n objects (0 and 1 appearance twins) seen in nearly every frame, appearance on an _ArcPath.  Every n + 1 frames an object shows
    what it showed in an earlier frame whose sample is still in its ring: at a ring position >= 64 when there is one (70 - 90 frames
    back when the budget allows), else 40 - 60 frames back.  A sample is gone back to once, so the nearest younger sample is its
    neighbour on the path, 4.8e-3 away."""
    rng = np.random.default_rng(seed)
    pos, vel, wh = _layout(rng, n, grid[0], grid[1], [40, 50], [70, 90], 0.3)
    paths = [_ArcPath(rng, frames) for _ in range(n)]
    paths[1] = paths[0]
    miss = {(int(rng.integers(0, n)), int(rng.integers(10, frames))) for _ in range(n)}
    held = [[] for _ in range(n)]                                          # per object: (phase, may be gone back to) of every feature, in ring order
    out = []
    for t in range(frames):
        dets = []
        for i in range(n):
            phase, back = t, False
            if t % (n + 1) == i and t >= 48:
                k0 = max(0, len(held[i]) - budget)
                cand = [j for j in range(k0, len(held[i]) - 8) if held[i][j][1]]
                deep = [j for j in cand if j % budget >= 64]
                pick = [j for j in deep if 70 <= len(held[i]) - j <= 90] or deep or [j for j in cand if 40 <= len(held[i]) - j <= 60]
                if pick:
                    j = int(rng.choice(pick))
                    phase, back = held[i][j][0], True
                    held[i][j] = (phase, False)
            if (i, t) in miss and not back:
                continue
            held[i].append((phase, not back))
            f = _unit(paths[i].at(phase) + 5e-4 * rng.standard_normal(512))
            dets.append(_det(rng, pos[i] + vel[i] * t, wh[i], f))
        dets += _clutter(rng, int(rng.integers(0, 3)))
        out.append([dets[k] for k in rng.permutation(len(dets))])
    return out


DEEP_SEEDS = {64: 6401, 65: 6501, 100: 10001, "wide": 10101}
P_DEEP = dict(max_dist=0.2, max_iou_distance=0.7, max_age=30, n_init=3)


def deep_gallery(budget):
    n = {64: 4, 65: 6, 100: 5}[budget]
    return {"name": f"deep_gallery_{budget}", "seed": DEEP_SEEDS[budget], "p": dict(P_DEEP, budget=budget),
            "frames": _deep(DEEP_SEEDS[budget], budget, n, round(2.3 * budget), (3, 2))}


def deep_gallery_wide():
    return {"name": "deep_gallery_wide", "seed": DEEP_SEEDS["wide"], "p": dict(P_DEEP, budget=100), "frames": _deep(DEEP_SEEDS["wide"], 100, 14, 106, (5, 4))}


# ------------------------------------------------------------------------------------------------ more than 64 detections
MANY_SEED = 7501


def many_dets():
    rng = np.random.default_rng(MANY_SEED)
    n = 75
    pos, vel, wh = _layout(rng, n, 10, 8, [30, 40], [50, 60], 1.0)
    pr = _protos(rng, n)
    frames = []
    for t in range(12):
        dets = [_det(rng, pos[i] + vel[i] * t, wh[i], _unit(pr[i] + 0.02 * rng.standard_normal(512))) for i in range(n)]
        dets += _clutter(rng, int(rng.integers(0, 3)))
        frames.append([dets[k] for k in rng.permutation(len(dets))])
    return {"name": "many_dets", "seed": MANY_SEED, "p": dict(max_dist=0.2, max_iou_distance=0.7, max_age=30, n_init=3, budget=5), "frames": frames}


# ------------------------------------------------------------------------------------------------ walks: several trackers, one launch
def _walk_frame(rng, per_label):
    """One frame of a videotracker_run_features call: rows of all labels shuffled together (a label's boxes keep their order)."""
    lab = np.concatenate([np.full(len(d), c, np.int64) for c, d in enumerate(per_label)])
    dets = [x for d in per_label for x in d]
    order = rng.permutation(len(dets))
    tl = np.array([dets[k]["tlwh"] for k in order]).reshape(-1, 4)
    xyxy = np.concatenate([tl[:, :2], tl[:, :2] + tl[:, 2:]], axis=1)
    return {"label": lab[order], "xyxy": xyxy, "conf": np.array([dets[k]["conf"] for k in order]),
            "feat": np.array([dets[k]["feature"] for k in order], np.float32).reshape(-1, 512)}


def walk_rows(frames, first_key=1):
    """rows7 [n, 7] = frame key, x1, y1, x2, y2, conf, label, and the matching features [n, 512]."""
    rows = [np.column_stack([np.full(len(f["conf"]), first_key + k, np.float64), f["xyxy"], f["conf"], f["label"].astype(np.float64)]) for k, f in enumerate(frames)]
    return np.concatenate(rows), np.concatenate([f["feat"] for f in frames])


def run_walk(params, frames, states=None, noise_seed=None, hw=FRAME_HW):
    """VideoTracker.run over the frames with one DeepSortOracle per label, fed the supplied features (a label without boxes in a frame is
    not stepped).  states: trackers to continue from.  Returns (the TrackerStates, per frame the rows [m, 6] in label order)."""
    img = np.zeros((hw[0], hw[1], 3), np.uint8)
    cur, ds = {}, []
    for c, p in enumerate(params):
        o = od.DeepSortOracle(lambda crops, c=c: cur[c], p["max_dist"], p["min_confidence"], p["nms_max_overlap"], p["max_iou_distance"], p["max_age"],
                              p["n_init"], p["budget"])
        o.trk = states[c] if states is not None else Probe(p, noise_seed)
        ds.append(o)
    rows = []
    for f in frames:
        out = []
        for c in range(len(params)):
            m = f["label"] == c
            if not m.any():
                continue
            cur[c] = f["feat"][m]
            out += [list(r[:5]) + [c] for r in ds[c].update(f["xyxy"][m], f["conf"][m], img)]
        rows.append(np.array(out, np.int64).reshape(-1, 6))
    return [o.trk for o in ds], rows


P_WALK = dict(min_confidence=0.0, nms_max_overlap=1.0, max_dist=0.2, max_iou_distance=0.7)
WALK_SEED, WALK_GROUP, WALK_FRAMES = 1201, 12, 11


def growing_walk(group=WALK_GROUP):
    """Label 0: a new group of `group` objects every frame, seen for two frames (three when the group's number is odd) and gone; n_init 1
    and a max_age longer than the clip keep every track.  Every third group shows itself once more four frames after its first: by then
    only the cascade can claim its detections, on appearance rows whose samples were written earlier in the same launch.  Label 1: two
    objects in every frame."""
    rng = np.random.default_rng(WALK_SEED)
    F = WALK_FRAMES
    n = F * group + 2
    pos, vel, wh = _layout(rng, n, 14, 10, [25, 25], [45, 45], 1.0)
    pr = _protos(rng, n, 0.1)
    frames = []
    for t in range(F):
        heavy = [i for g in range(F) for i in range(g * group, (g + 1) * group) if g <= t <= g + 1 + g % 2 or (g % 3 == 0 and t == g + 4)]
        per = [[_det(rng, pos[i] + vel[i] * t, wh[i], _unit(pr[i] + 0.02 * rng.standard_normal(512))) for i in grp] for grp in (heavy, [n - 2, n - 1])]
        frames.append(_walk_frame(rng, per))
    params = [dict(P_WALK, max_age=50, n_init=1, budget=5), dict(P_WALK, max_age=30, n_init=3, budget=10)]
    return {"name": "growing_walk", "seed": WALK_SEED, "params": params, "frames": frames}


MIXED_SEED, MIXED_BUILD, MIXED_ARENA_MB = 3301, (20, 5), 1


def mixed_fit():
    """Two trackers built up frame by frame (`build`: per tracker the tracker_step detections), then one launch of three frames (`frames`).
    Label 0: 100 objects with a 60-deep budget, half of them in each frame of the launch; label 1: three objects."""
    rng = np.random.default_rng(MIXED_SEED)
    n = (100, 3)
    pos, vel, wh = _layout(rng, sum(n), 12, 9, [30, 30], [50, 55], 0.5)
    pr = _protos(rng, sum(n))
    ids = [list(range(n[0])), list(range(n[0], sum(n)))]

    def dets(t, who):
        return [_det(rng, pos[i] + vel[i] * t, wh[i], _unit(pr[i] + 0.02 * rng.standard_normal(512))) for i in who]

    build = [[[d[k] for k in rng.permutation(len(d))] for d in (dets(t, ids[c]) for t in range(MIXED_BUILD[c]))] for c in range(2)]
    frames = [_walk_frame(rng, [dets(MIXED_BUILD[0] + t, sorted(rng.permutation(n[0])[:50])), dets(MIXED_BUILD[1] + t, ids[1])]) for t in range(3)]
    params = [dict(P_WALK, max_age=30, n_init=3, budget=60), dict(P_WALK, max_age=30, n_init=3, budget=60)]
    return {"name": "mixed_fit", "seed": MIXED_SEED, "params": params, "build": build, "frames": frames, "arena_floats": MIXED_ARENA_MB * ARENA_FLOATS_PER_MB}


def run_mixed(scene, noise_seed=None):
    """(the TrackerStates after the launch, the launch's rows per frame, the TrackerStates' sizes when the launch begins)."""
    trk = [Probe(p, noise_seed) for p in scene["params"]]
    for k, b in zip(trk, scene["build"]):
        for d in b:
            k.predict(); k.update(d)
    before = [{"tracks": len(k.tracks), "ring_rows": k.steps[-1]["ring_rows"]} for k in trk]
    trk, rows = run_walk(scene["params"], scene["frames"], states=trk)
    return trk, rows, before


# ------------------------------------------------------------------------------------------------ capacity stops
P_LINGER = dict(P_WALK, max_age=100, n_init=1, budget=1)
LINGER_WH = (3000, 4000)


def lingering(groups, per, seed, extra=0):
    """Frames f = 0 .. groups: groups f - 1 and f of `per` objects each are seen, so every group is seen twice, confirmed (n_init 1) and
    kept (max_age 100): groups * per lingering confirmed tracks after the last frame.  Also returns `extra` detections of objects never
    seen before, and the objects' detections at a later time (who, t) -> dets."""
    rng = np.random.default_rng(seed)
    n = groups * per + extra
    pos, vel, wh = _layout(rng, n, 27, 20, [40, 50], [70, 90], 0.5, W=LINGER_WH[1], H=LINGER_WH[0])
    pr = _unit(rng.standard_normal((n, 512)))

    def dets(who, t):
        return [_det(rng, pos[i] + vel[i] * t, wh[i], _unit(pr[i] + 0.02 * rng.standard_normal(512))) for i in who]

    frames = [dets([i for g in (f - 1, f) if 0 <= g < groups for i in range(g * per, (g + 1) * per)], f) for f in range(groups + 1)]
    return frames, dets(range(groups * per, n), groups + 1), dets


def run_single(p, frames, noise_seed=None):
    trk = Probe(p, noise_seed)
    for d in frames:
        trk.predict(); trk.update(d)
    return trk


POOL_SLOTS = 8


def pool_clip():
    """Two trackers, three frames, a pool of POOL_SLOTS (which is also the most tracks + detections a step may hold there).  A (label 0):
    an object and a clutter box in frame 0 (slots 1-2; the clutter's tentative track dies in frame 1 and its slot goes to the freed
    list), three more objects in frame 1 (slots 3-5), two more in frame 2.  B (label 1): two objects, slots of frame 0.  A's frame 2
    asks for the eighth and ninth slot of the launch.  `eight`: one frame of eight objects, `after`: four frames of four, for the time
    after a reset."""
    rng = np.random.default_rng(808)
    pos, vel, wh = _layout(rng, 17, 6, 4, [40, 50], [70, 90], 0.5)
    pr = _unit(rng.standard_normal((17, 512)))

    def dets(who, t):
        return [_det(rng, pos[i] + vel[i] * t, wh[i], _unit(pr[i] + 0.02 * rng.standard_normal(512))) for i in who]

    a = [[0, 8], [0, 2, 3, 4], [0, 2, 5, 6]]
    frames = [_walk_frame(rng, [dets(a[t], t), dets([15, 16], t)]) for t in range(3)]
    params = [dict(P_WALK, max_age=30, n_init=3, budget=4), dict(P_WALK, max_age=30, n_init=3, budget=4)]
    return {"params": params, "frames": frames, "eight": dets(range(7, 15), 0), "after": [dets(range(9, 13), t) for t in range(4)]}


# ------------------------------------------------------------------------------------------------ regimes
SINGLE = {"deep_gallery_64": lambda: deep_gallery(64), "deep_gallery_65": lambda: deep_gallery(65), "deep_gallery_100": lambda: deep_gallery(100),
          "deep_gallery_wide": deep_gallery_wide, "many_dets": many_dets}


@functools.lru_cache(maxsize=None)
def scene(name):
    return {**SINGLE, "growing_walk": growing_walk, "mixed_fit": mixed_fit}[name]()


def regime_of(sc):
    """What a scene reaches, from oracle.deepsort alone (see the module's header), and whether it meets the margin condition."""
    if "p" in sc:
        run = lambda seed: [run_single(sc["p"], sc["frames"], seed)]
    elif "build" in sc:
        run = lambda seed: run_mixed(sc, seed)[0]
    else:
        run = lambda seed: run_walk(sc["params"], sc["frames"], noise_seed=seed)[0]
    mixed = run_mixed(sc) if "build" in sc else None
    base = mixed[0] if mixed else run(None)
    r = sizes(base[0].steps)
    r["margin_ok"] = all([k.trace for k in run(seed)] == [k.trace for k in base] for seed in (1, 2, 3))
    if "p" not in sc:
        r["others"] = [sizes(k.steps) for k in base[1:]]
    if "build" in sc:
        before, dets = mixed[2], [sum(int((f["label"] == c).sum()) for f in sc["frames"]) for c in range(2)]
        r["host_need"] = [table_need(b["tracks"] * p["budget"], d) for b, p, d in zip(before, sc["params"], dets)]
        r["device_need"] = [table_need(b["ring_rows"], d) for b, d in zip(before, dets)]
        r["launch"] = sizes(base[0].steps[MIXED_BUILD[0]:])
    elif "params" in sc:
        dmax = max(int(k["D"].max()) for k in [r] + r["others"])
        r["cap"] = walk_cap(dmax)
    return r


@functools.lru_cache(maxsize=None)
def regime(name):
    return regime_of(scene(name))
