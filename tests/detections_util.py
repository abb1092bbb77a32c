"""The scripted scene of the per-frame detection tests (test_associate_cpu, test_associate_gpu, test_stream_detections_gpu): S = 3 slots,
D = 4 detections per frame, K = 17 joints, 42 frames in pixel coordinates (all multiples of 0.25, so shifts by whole pixels are exact).
A plain module: nothing here is collected.

    A, B   two people whose paths cross (A walks right, B walks left, 40 px apart where they meet)
    C      stands still; missed for max_age = 2 frames (8, 9: keeps slot and id) and for max_age + 1 frames (20 .. 22: dies at 22); back
           at 23 under a new id, in the slot it had (the lowest free one)
    E      a fourth person at frames 12 .. 14 while three slots are full: dropped, three times
    16     a frame with count = 0
    22     a detection with min_common - 1 = 2 observed joints (the others NaN) while a slot is free: ignored
    26     A with two NaN joints: still matched
    30     B twice, mirrored about its slot's reference (B's detection of frame 29 shifted by +8 and by -8 px): an exact tie
    rows beyond ``counts[t]`` hold a copy of A: reading them would show
The rows of every frame are permuted, differently per frame."""
import numpy as np

S, D, K, FRAMES, MAX_AGE = 3, 4, 17, 42, 2
RULE = dict(max_age=MAX_AGE, max_dist=0.5, min_common=3)
RESOLUTION = (1920, 1080)
A, B, C, E, FEW, B_PLUS, B_MINUS = 0, 1, 2, 3, 4, 5, 6                 # labels of the rows
C_MISSED, C_GONE, E_FRAMES, EMPTY, FEW_FRAME, NAN_FRAME, TIE_FRAME = (8, 9), (20, 21, 22), (12, 13, 14), 16, 22, 26, 30


def _quantise(a):
    return (np.round(np.asarray(a, np.float64) * 4.0) / 4.0).astype(np.float32)


def scene(seed=0, swap_tie=False):
    """-> (dets (FRAMES, D, K, 2) float32, counts (FRAMES,) int32, labels (FRAMES, D): who each row is, -1 for a row beyond the count).
    ``seed`` chooses the per-frame permutations (the tie frame keeps its own); ``swap_tie``: the two tied rows change places."""
    rng = np.random.default_rng(1234)
    body = _quantise(rng.uniform(-1.0, 1.0, size=(K, 2)) * [50.0, 100.0])
    jitter = _quantise(rng.uniform(-2.0, 2.0, size=(FRAMES, 4, K, 2)))
    perm_rng = np.random.default_rng(100 + seed)
    tie_perm = np.random.default_rng(7).permutation(4)
    dets, counts, labels = np.zeros((FRAMES, D, K, 2), np.float32), np.zeros(FRAMES, np.int32), np.full((FRAMES, D), -1, np.int64)
    last_b = None
    for t in range(FRAMES):
        where = {A: (200.0 + 17.0 * t, 300.0), B: (900.0 - 17.0 * t, 340.0), C: (1400.0, 700.0), E: (300.0, 900.0), FEW: (1700.0, 200.0)}
        pose = {k: (body + np.array(v, np.float32) + jitter[t, min(k, 3)]).astype(np.float32) for k, v in where.items()}
        rows = [A, B] + ([C] if t not in C_MISSED + C_GONE else []) + ([E] if t in E_FRAMES else [])
        if t == EMPTY:
            rows = []
        if t == FEW_FRAME:
            pose[FEW][2:] = np.nan
            rows.append(FEW)
        if t == NAN_FRAME:
            pose[A][3:5] = np.nan
        if t == TIE_FRAME:
            pose[B_PLUS], pose[B_MINUS] = last_b + np.float32(8.0), last_b - np.float32(8.0)
            rows = [A, B_MINUS, B_PLUS, C] if swap_tie else [A, B_PLUS, B_MINUS, C]
            order = tie_perm                                          # (its own permutation: only ``swap_tie`` moves the tied rows)
        else:
            order = perm_rng.permutation(len(rows))
        rows = [rows[k] for k in order]
        counts[t] = len(rows)
        dets[t] = pose[A]                                             # rows beyond the count: a copy of A
        for d, r in enumerate(rows):
            dets[t, d], labels[t, d] = pose[r], r
        if B in rows:
            last_b = pose[B]
    return dets, counts, labels


def tracks_as_sets(labels, track_of):
    """The tracks as a set of frozensets of (frame, label): who was followed when, whatever the ids and slots."""
    tracks = {}
    for t, d in zip(*np.nonzero(track_of >= 0)):
        tracks.setdefault(int(track_of[t, d]), set()).add((int(t), int(labels[t, d])))
    return {frozenset(v) for v in tracks.values()}


def slot_frames(dets, result, per_joint):
    """What a plain session is pushed at every tick to follow ``associate_host``'s result -> (kp (T, S, K, 2) float32: the slot's detection,
    zeros without one; valid (T, S) bool, or (T, S, K) with ``per_joint``: set for a slot with a detection)."""
    T = len(dets)
    kp = np.zeros((T, S) + dets.shape[2:], np.float32)
    t, s = np.nonzero(result.slot_det >= 0)
    kp[t, s] = dets[t, result.slot_det[t, s]]
    valid = result.slot_full.copy()
    return kp, (np.repeat(valid[:, :, None], dets.shape[2], axis=2) if per_joint else valid)
