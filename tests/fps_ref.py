"""Float64 reference of greedy farthest-point sampling with the lowest-index tie rule (csrc/fps.hip states the semantics; reference
geometry/util.py:5-27 is the torch statement).  numpy only, one cloud at a time; shared by tests/test_fps_cpu.py and test_fps_gpu.py.

greedy(pts, k, start)         -> (indices int64 [k], gaps float64 [k]: per pick the relative gap between the best and the second-best
                                 candidate, inf where none is defined -- pick 0, a single point, a maximum of 0 or a non-finite one);
                                 a prefix of the result is the result for a smaller k
pick_shortfall(pts, picks)    -> for every pick after the first, how far (relative) its distance to the EARLIER picks of the same
                                 sequence falls short of the largest such distance of any point: 0 for a pick that is a true maximum
greedy32(pts, k, start)       -> indices int64 [k] of the SAME statement evaluated in float32, operation by operation as csrc/fps.hip
                                 states it (px - x, the three squares added from the left, a correctly rounded square root, minimum,
                                 first maximum): numpy rounds every one of these correctly, so a kernel that does equals it exactly
NaN is ordered as numpy and torch order it: argmax takes the first NaN, minimum keeps it.
"""
import numpy as np


def _dist(pts, v):
    d = pts - pts[v]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def greedy(pts, k, start):
    pts = np.asarray(pts, dtype=np.float64)
    V = pts.shape[0]
    picks = np.empty(k, dtype=np.int64)
    picks[0] = cur = min(max(int(start), 0), V - 1)
    gaps = np.full(k, np.inf)
    with np.errstate(invalid="ignore"):
        m = _dist(pts, cur)
        for i in range(1, k):
            cur = int(np.argmax(m))  # (the first of equal maxima; the first NaN if there is one)
            best = m[cur]
            if V > 1 and best > 0 and np.isfinite(best):
                m[cur] = -np.inf
                rest = m.max()
                m[cur] = best
                gaps[i] = (best - rest) / best
            picks[i] = cur
            m = np.minimum(m, _dist(pts, cur))
    return picks, gaps


def pick_shortfall(pts, picks):
    pts = np.asarray(pts, dtype=np.float64)
    picks = np.asarray(picks)
    out = np.zeros(len(picks))
    m = _dist(pts, int(picks[0]))
    for i in range(1, len(picks)):
        top = m.max()
        got = m[int(picks[i])]
        out[i] = 0.0 if top == 0 else (top - got) / top
        m = np.minimum(m, _dist(pts, int(picks[i])))
    return out


def greedy32(pts, k, start):
    pts = np.asarray(pts, dtype=np.float32)
    V = pts.shape[0]
    picks = np.empty(k, dtype=np.int64)
    picks[0] = cur = min(max(int(start), 0), V - 1)

    def dist(v):
        d = pts[v] - pts
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])

    with np.errstate(invalid="ignore", over="ignore"):
        m = dist(cur)
        for i in range(1, k):
            picks[i] = cur = int(np.argmax(m))
            m = np.minimum(m, dist(cur))
    assert m.dtype == np.float32
    return picks
