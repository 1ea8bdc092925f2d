"""Float64 reference of estimate_bones (a3d_estimate_bones: csrc/bones.hip eb_kernel, csrc/bones_wide.hip, csrc/eb_common.h) and the
hard point sets tests/test_estimate_bones_cpu.py and tests/test_estimate_bones_adversarial_gpu.py run it on.

The reference is written from the definition of the operation in the reference project (model/geometry/skinning.py:50-248), not from
this repository's torch restatement: numpy float64, plain and slow -- a sort per quantile over the pooled values of the call, boolean
indexing for the low set of the Fauna variant, loops over instances and quadrants.

    spine      point_a / point_b = the vertices of largest / smallest z ('z_minmax_y+': among those with y > mean(y) - 0.5, strictly),
               first index on ties, x snapped to 0; mid = the centroid with x = 0 (y lifted by 0.5 with legs);
               joints = a (1 - t) + mid t  ++  b t + mid (1 - t), t = linspace(0, 1, n_body / 2 + 1); body bone k = (joint k + 1, joint k)
               for the first half, then (joint i, joint i + 1) for i = n_body - 1 .. n_body / 2
    quantiles  torch.quantile over ALL values of the call: pos = float32(q) * float32(n - 1), the values of ranks floor(pos) and ceil(pos)
               interpolated with the weight pos - floor(pos)
    quadrants  margin = (q95(x) - q05(x)) 0.2;  0: x > m, z > 0   1: x > m, z < 0   2: x < -m, z < 0   3: x < -m, z > 0
               Fauna: low = y < q_thr(y); x0, z0 = medians of x[low], z[low]; mx, mz = 0.2 (q95 - q05) of x[low], z[low];
               0: x - x0 > mx, z - z0 > mz   1: x - x0 > mx, z < z0   2: x - x0 < -mx, z < z0   3: x - x0 < -mx, z - z0 > mz
    feet       per instance and quadrant the vertex of lowest y, first index on ties
    legs       attachment of legs 0 / 1 = the body bone whose end [1] is nearest in z to the foot OF INSTANCE 0 (first index on ties) unless
               prescribed; legs 2 / 3 reuse those of legs 1 / 0; a cached chain brings its own four; leg joints = foot (1 - r) + end r,
               r = linspace(0, 1, n_leg + 1); leg bone i = (joint i + 1, joint i)

``reference`` returns the bones with their MAGNITUDE (the same expression over absolute values; errors are measured in units of 2^-24 x
magnitude, tests/deriv_ref.py) and every decision: spine indices, the quantiles with the two neighbours they interpolate, the low
count, the foot per (instance, quadrant), the attachment joints and, for every kind of comparison the algorithm makes, the smallest
slack over all vertices in the same units (``slack``; the operand magnitude of ``a > b`` is |a| + the magnitude of b).

The only float32 product in front of a strict comparison is the margin (q95 - q05) * 0.2: ``f32_margin`` evaluates it as float32 does
(one rounding).  The lattice family uses it: its coordinates are multiples of 2^-3 / 2^-2, its quantile neighbours are tied and its
coordinate sums are exact in float32 in any order, so every float32 operation in front of a decision is exact or that one rounding, and
vertices can sit ON a boundary (slack exactly 0) or one float32 step beyond it.  Outside that family every slack is at least 64 units,
except where ``exact_zero_slacks`` allows exactly 0: a quantile of weight 0, or between equal neighbours, IS the value of a vertex,
copied without arithmetic in every precision, so that vertex sits on ``y < threshold`` / ``z < z0`` with slack 0 in every implementation.

MUTATIONS are deliberate mistakes behind the ``mutate`` switch; tests/test_estimate_bones_cpu.py checks that each of them moves a
selected vertex, an attachment joint or a bone by more than the kernels' bound on at least one case.

MEASURED holds, per case, what the torch float32 restatement (model/geometry/skinning.py on the CPU) reaches against this reference, in
units; the kernels' bound is 4 x that figure plus 4 ulp of the float64 value (``violations``).  Cases are seeded, cached and never
modified by a test.
"""
import functools
import math

import numpy as np
import torch

from deriv_ref import EPS, units, violations  # noqa: F401  (the same unit and the same bound as the other float64 suites)

FACTOR = 4.0
MIN_SLACK = 64.0
MUTATIONS = ("per_instance", "rank_off_by_one", "ge_upper", "ge_margin", "ge_zero", "ge_thr", "ge_mx", "ge_mz", "ge_z0", "last_index",
             "neg_zero_below", "attach_instance1", "blend_off_by_one", "ramp_off_by_one")
TINY = float(np.float32(2.0 ** -149))


# ---------------------------------------------------------------------------------------------------------------- the reference
def quantile(values, q, mutate=None):
    """torch.quantile(values, q) in float64 -> (value, lower neighbour, upper neighbour, weight, ranks agree in float32 and float64)."""
    s = np.sort(np.asarray(values, dtype=np.float64))
    n = s.shape[0]
    assert n > 0
    p32 = float(np.float32(q) * np.float32(n - 1))
    p64 = q * (n - 1)
    lo, hi = int(math.floor(p32)), int(math.ceil(p32))
    same = (lo, hi) == (int(math.floor(p64)), int(math.ceil(p64)))
    if mutate == "rank_off_by_one":
        lo, hi = min(lo + 1, n - 1), min(hi + 1, n - 1)
    w = p32 - math.floor(p32)
    return dict(value=s[lo] + w * (s[hi] - s[lo]), lo=s[lo], hi=s[hi], w=w, ranks_agree=same, n=n)


def _arg(values, want_max, mutate=None):
    """First index of the extreme value (torch.argmax / argmin; -0.0 == +0.0)."""
    v = np.asarray(values, dtype=np.float64)
    best = v.max() if want_max else v.min()
    tied = np.nonzero(v == best)[0]
    if mutate == "neg_zero_below" and not want_max and best == 0.0:
        neg = [i for i in tied if np.signbit(v[i])]
        tied = np.array(neg) if neg else tied
    return int(tied[-1] if mutate == "last_index" else tied[0])


def _gt(a, b, mutate, name):
    return a >= b if mutate == name else a > b


def _lt(a, b, mutate, name):
    return a <= b if mutate == name else a < b


def _slack(diff, mag):
    """min |diff| / (2^-24 mag) over the vertices."""
    diff, mag = np.abs(np.asarray(diff, dtype=np.float64)).reshape(-1), np.asarray(mag, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(mag > 0, diff / (EPS * mag), np.where(diff > 0, np.inf, 0.0))
    return float(u.min())


def body_pairs(n_body):
    half = n_body // 2
    return [(i + 1, i) for i in range(half)] + [(i, i + 1) for i in range(n_body - 1, half - 1, -1)]


def chain_of(n_body, n_leg, leg_attach, attach_legs_to_body=True):
    """The kinematic chain [(bone, [dependent bones])], parents in front: the two halves of the spine leaf -> root, then every leg."""
    half = n_body // 2
    chain = []
    for first, count in ((0, half), (half, n_body - half)):
        below = []
        for k in range(first, first + count):
            chain.insert(0, (k, below))
            below = below + [k]
    start = n_body
    for l in range(4 if n_leg > 0 else 0):
        ids = list(range(start, start + n_leg))
        if attach_legs_to_body:
            for bone, dep in chain:
                if bone == leg_attach[l] or leg_attach[l] in dep:
                    dep += ids
        leg, below = [], []
        for k in ids:
            leg.insert(0, (k, below))
            below = below + [k]
        chain = chain + leg
        start += n_leg
    return chain


def reference(seq, n_body, n_leg, mode, thr=None, prescribed=None, cached=None, f32_margin=False, mutate=None):
    """seq [B,F,V,3] (float32 values) -> dict: bones, mag [N,K,2,3] float64 and the decisions (see the module docstring).
    ``prescribed``: legs_to_body_joint_indices of a chain rebuild (None entries are found); ``cached``: the four body_bone_idx of a cached chain."""
    assert mutate is None or mutate in MUTATIONS
    p = np.asarray(seq, dtype=np.float64).reshape(-1, seq.shape[2], 3)
    N, V = p.shape[:2]
    xs, ys, zs = p[..., 0], p[..., 1], p[..., 2]
    out = dict(slack={}, quantiles={}, ranks_agree=True)
    # ---- spine
    mid = p.mean(1)
    mid_mag = np.abs(p).mean(1)
    va, vb = [], []
    for n in range(N):
        if mode == "z_minmax_y+":
            bound = mid[n, 1] - 0.5
            upper = _gt(ys[n], bound, mutate, "ge_upper")
            ka, kb = np.where(upper, zs[n], -1e6), np.where(upper, zs[n], 1e6)
            out["slack"]["upper"] = min(out["slack"].get("upper", np.inf), _slack(ys[n] - bound, np.abs(ys[n]) + mid_mag[n, 1] + 0.5))
        else:
            assert mode == "z_minmax"
            ka = kb = zs[n]
        va.append(_arg(ka, True, mutate))
        vb.append(_arg(kb, False, mutate))
    out["spine"] = np.array([va, vb]).T  # [N,2]
    mid, mid_mag = mid.copy(), mid_mag.copy()
    mid[:, 0] = 0
    mid_mag[:, 0] = 0
    if n_leg > 0:
        mid[:, 1] += 0.5
        mid_mag[:, 1] += 0.5
    nb2 = n_body // 2 + 1
    t = np.linspace(0.0, 1.0, nb2)
    if mutate == "blend_off_by_one":
        t = np.concatenate([t[1:], t[-1:]])
    joints, joints_mag = np.zeros((N, n_body + 1, 3)), np.zeros((N, n_body + 1, 3))
    for n in range(N):
        a, b = p[n, va[n]].copy(), p[n, vb[n]].copy()
        a[0] = b[0] = 0
        for i in range(nb2):
            if i < nb2 - 1:
                joints[n, i] = a * (1 - t[i]) + mid[n] * t[i]
                joints_mag[n, i] = np.abs(a) * (1 - t[i]) + mid_mag[n] * t[i]
            joints[n, nb2 - 1 + i] = b * t[i] + mid[n] * (1 - t[i])
            joints_mag[n, nb2 - 1 + i] = np.abs(b) * t[i] + mid_mag[n] * (1 - t[i])
    pairs = body_pairs(n_body)
    K = n_body + 4 * n_leg
    bones, mag = np.zeros((N, K, 2, 3)), np.zeros((N, K, 2, 3))
    for k, (ja, jb) in enumerate(pairs):
        bones[:, k, 0], bones[:, k, 1] = joints[:, ja], joints[:, jb]
        mag[:, k, 0], mag[:, k, 1] = joints_mag[:, ja], joints_mag[:, jb]
    out.update(n_body=n_body, n_leg=n_leg, N=N, V=V)
    if n_leg == 0:
        out.update(bones=bones, mag=mag, chain=chain_of(n_body, 0, None), bones_to_joints=pairs)
        return out
    # ---- quadrants
    pooled = mutate != "per_instance"
    quad = np.zeros((N, 4, V), dtype=bool)
    sl = out["slack"]

    def note(name, value):
        sl[name] = min(sl.get(name, np.inf), value)

    def margin_of(q95, q05):
        if f32_margin:
            return float(np.float32(np.float32(q95["value"]) - np.float32(q05["value"])) * np.float32(0.2))
        return (q95["value"] - q05["value"]) * 0.2

    def qs_of(name, values, q):
        r = quantile(values, q, mutate)
        out["quantiles"].setdefault(name, r)
        out["ranks_agree"] = out["ranks_agree"] and r["ranks_agree"]
        return r

    def amag(r):
        return (abs(r["lo"]) + abs(r["hi"])) * 0.5

    def stats(sel):
        """The quantiles of the values the rule pools (the whole call; one instance under the 'per_instance' mistake)."""
        st = {}
        if thr is None:
            st["x95"], st["x05"] = qs_of("x95", xs[sel].reshape(-1), 0.95), qs_of("x05", xs[sel].reshape(-1), 0.05)
        else:
            st["y_thr"] = qy = qs_of("y_thr", ys[sel].reshape(-1), thr)
            low = _lt(ys[sel], qy["value"], mutate, "ge_thr")
            y_mag = (1 - qy["w"]) * abs(qy["lo"]) + qy["w"] * abs(qy["hi"])
            note("y_thr", _slack(ys[sel] - qy["value"], np.abs(ys[sel]) + y_mag))
            out.setdefault("y_threshold", qy["value"])
            out.setdefault("n_low", int(low.sum()))
            xl, zl = xs[sel][low], zs[sel][low]  # boolean indexing: the low set
            for name, col in (("xl", xl), ("zl", zl)):
                for tag, q in (("50", 0.5), ("95", 0.95), ("05", 0.05)):
                    st[name + tag] = qs_of(name + tag, col, q)
        return st

    shared = stats(slice(None)) if pooled else None
    for n in range(N):
        st = shared if pooled else stats(slice(n, n + 1))
        if thr is None:
            q95, q05 = st["x95"], st["x05"]
            m = margin_of(q95, q05)
            m_mag = (amag(q95) + amag(q05)) * 0.2
            out.setdefault("margin", m)
            right, left = _gt(xs[n], m, mutate, "ge_margin"), _lt(xs[n], -m, mutate, "ge_margin")
            front, back = _gt(zs[n], 0.0, mutate, "ge_zero"), _lt(zs[n], 0.0, mutate, "ge_zero")
            quad[n] = [right & front, right & back, left & back, left & front]
            note("margin", min(_slack(xs[n] - m, np.abs(xs[n]) + m_mag), _slack(xs[n] + m, np.abs(xs[n]) + m_mag)))
            note("zero", _slack(zs[n], np.abs(zs[n])))
        else:
            x50, x95, x05, z50, z95, z05 = (st[k] for k in ("xl50", "xl95", "xl05", "zl50", "zl95", "zl05"))
            x0, z0, mx, mz = x50["value"], z50["value"], margin_of(x95, x05), margin_of(z95, z05)
            out.setdefault("centre", (x0, z0, mx, mz))
            mx_mag, mz_mag = (amag(x95) + amag(x05)) * 0.2, (amag(z95) + amag(z05)) * 0.2
            dx, dz = xs[n] - x0, zs[n] - z0
            right, left = _gt(dx, mx, mutate, "ge_mx"), _lt(dx, -mx, mutate, "ge_mx")
            front, back = _gt(dz, mz, mutate, "ge_mz"), _lt(zs[n], z0, mutate, "ge_z0")
            quad[n] = [right & front, right & back, left & back, left & front]
            note("mx", min(_slack(dx - mx, np.abs(xs[n]) + amag(x50) + mx_mag), _slack(dx + mx, np.abs(xs[n]) + amag(x50) + mx_mag)))
            note("mz", _slack(dz - mz, np.abs(zs[n]) + amag(z50) + mz_mag))
            note("z0", _slack(zs[n] - z0, np.abs(zs[n]) + amag(z50)))
    out["population"] = quad.sum(-1)  # [N,4]
    assert out["population"].min() > 0, "a quadrant without a vertex"
    feet = np.zeros((N, 4), dtype=np.int64)
    for n in range(N):
        for k in range(4):
            inside = np.nonzero(quad[n, k])[0]
            feet[n, k] = inside[_arg(ys[n, inside], False, mutate)]
    out["feet"] = feet
    # ---- attachment joints and leg bones
    if cached is not None:
        attach = [int(v) for v in cached]
    else:
        given = list(prescribed) if prescribed is not None else [None] * 4
        src = 1 if (mutate == "attach_instance1" and N > 1) else 0
        found = []
        for l in (0, 1):
            if given[l] is None:
                d = np.abs(bones[src, :n_body, 1, 2] - zs[src, feet[src, l]])
                j = _arg(d, False, mutate)
                d_mag = mag[src, :n_body, 1, 2] + abs(zs[src, feet[src, l]])
                rest = np.delete(np.arange(n_body), j)
                note("attach", _slack(d[rest] - d[j], d_mag[rest] + d_mag[j]))
                found.append(j)
            else:
                found.append(int(given[l]))
        attach = [found[0], found[1], found[1], found[0]]
    out["attach"] = attach
    r = np.linspace(0.0, 1.0, n_leg + 1)
    if mutate == "ramp_off_by_one":
        r = np.concatenate([r[1:], r[-1:]])
    for n in range(N):
        for l in range(4):
            foot, end, end_mag = p[n, feet[n, l]], bones[n, attach[l], 1], mag[n, attach[l], 1]
            lj = np.stack([foot * (1 - r[i]) + end * r[i] for i in range(n_leg + 1)])
            lm = np.stack([np.abs(foot) * (1 - r[i]) + end_mag * r[i] for i in range(n_leg + 1)])
            for i in range(n_leg):
                k = n_body + l * n_leg + i
                bones[n, k, 0], bones[n, k, 1] = lj[i + 1], lj[i]
                mag[n, k, 0], mag[n, k, 1] = lm[i + 1], lm[i]
    out.update(bones=bones, mag=mag, chain=chain_of(n_body, n_leg, attach), bones_to_joints=pairs)
    return out


def selected(ref):
    """The bone ends that are copies of input vertices -> (index array [M,4] into bones [N,K,2,3], vertex per row [M] as (n, v), snap x)."""
    N, n_body, n_leg = ref["N"], ref["n_body"], ref["n_leg"]
    rows = []
    for n in range(N):
        rows.append((n, 0, 1, int(ref["spine"][n, 0]), True))            # joint 0: end 1 of bone 0
        rows.append((n, n_body // 2, 1, int(ref["spine"][n, 1]), True))  # joint n_body: end 1 of the first bone of the second half
        for l in range(4 if n_leg > 0 else 0):
            rows.append((n, n_body + l * n_leg, 1, int(ref["feet"][n, l]), False))
    return rows


def selected_points(seq, ref):
    """-> (got-indexable list of (n, bone, end), float32 array [M,3] of the vertices the reference selects, x snapped on the spine)."""
    p = np.asarray(seq, dtype=np.float32).reshape(-1, seq.shape[2], 3)
    rows = selected(ref)
    want = np.stack([p[n, v] * (np.array([0, 1, 1], dtype=np.float32) if snap else np.float32(1)) for n, _, _, v, snap in rows])
    return [(n, b, e) for n, b, e, _, _ in rows], want


# ---------------------------------------------------------------------------------------------------------------- case builders
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[:, None].contiguous()  # [N,V,3] -> [N,1,V,3]


def exact_zero_slacks(ref):
    """The comparisons a vertex sits on EXACTLY in every precision: a quantile whose neighbours are equal, or whose weight is 0, is the
    value of a vertex, copied without arithmetic -- that vertex has slack 0 on ``y < threshold`` / ``z < z0``; with one low vertex the six
    quantiles are its own coordinates, so that mx = mz = 0 and x - x0 = z - z0 = 0 for it."""
    q, ok = ref["quantiles"], set()
    exact = lambda r: r["w"] == 0 or r["lo"] == r["hi"]  # noqa: E731
    if "y_thr" in q and exact(q["y_thr"]):
        ok.add("y_thr")
    if "zl50" in q and exact(q["zl50"]):
        ok.add("z0")
    if ref.get("n_low") == 1:
        ok |= {"mx", "mz"}
    return ok


def acceptable(ref):
    """The conditions on a case outside the lattice family."""
    zero_ok = exact_zero_slacks(ref)
    return ref["ranks_agree"] and all(v >= MIN_SLACK or (v == 0 and k in zero_ok) for k, v in ref["slack"].items())


def _settle(make, thr, mode="z_minmax_y+", n_body=8, n_leg=3, tries=200):
    """make(0), make(1), .. until the conditions hold (every quadrant populated, every slack at least 64 units): deterministic."""
    for s in range(tries):
        c = make(s).astype(np.float32)
        try:
            ref = reference(c[:, None], n_body, n_leg, mode, thr)
        except AssertionError:
            continue
        if acceptable(ref):
            return _t(c)
    raise AssertionError("no seed gives a case that meets the conditions")


def _clear_upper(c, room=0.02):
    """Moves the y within ``room`` of an instance's mean(y) - 0.5 to that distance, symmetrically (the mean barely moves)."""
    for n in range(c.shape[0]):
        for _ in range(3):
            b = c[n, :, 1].mean() - 0.5
            d = c[n, :, 1] - b
            c[n, :, 1] = np.where(np.abs(d) < room, b + np.where(d >= 0, room, -room) * 1.25, c[n, :, 1])
    return c


def _cloud(N, V, seed):
    """Five clusters per instance, vertex v in cluster v % 5: a body along z above four legs, one per top-view quadrant (float64 [N,V,3]).
    The legs start a little off the axes; the spine ends are fixed body vertices."""
    rng = np.random.default_rng(seed)
    u = rng.random((N, V, 3))
    k = np.arange(V) % 5
    sx = np.where((k == 1) | (k == 2), 1.0, -1.0)
    sz = np.where((k == 1) | (k == 4), 1.0, -1.0)
    leg = np.stack([sx * (0.05 + 0.55 * u[..., 0] ** 0.5), -1.4 + 0.8 * u[..., 1], sz * (0.05 + 0.75 * u[..., 2] ** 0.5)], -1)
    body = np.stack([-0.1 + 0.2 * u[..., 0], 0.2 + 0.4 * u[..., 1], -1.0 + 2.0 * u[..., 2]], -1)
    out = np.where((k == 0)[None, :, None], body, leg)
    if V >= 6:  # distinct spine ends, inside the body
        out[:, 0] = [0.03, 0.45, 1.25]
        out[:, 5] = [-0.03, 0.35, -1.25]
    return _clear_upper(out)


@functools.lru_cache(maxsize=None)
def pooled(N, thr, V=200, seed=101):
    """Instance n scaled by 0.5 .. 2 in y (by the fourth root of that in x and z: a pooled margin is a fifth of the pooled width, so a
    four times narrower instance would have no vertex beyond it) and shifted in x: its own quantiles are far from the pooled ones.
    Odd instances carry their legs further to +z: their feet would choose other attachment joints than instance 0's."""
    def make(s):
        c = _cloud(N, V, seed + s)
        k = np.arange(V) % 5
        for n in range(N):
            f = 0.5 * 4.0 ** (n / (N - 1)) if N > 1 else 1.0
            c[n, :, 1] *= f
            c[n, :, 0] = c[n, :, 0] * f ** 0.25 + 0.15 * ((n % 3) - 1)
            c[n, :, 2] = c[n, :, 2] * f ** 0.25 + np.where(k == 0, 0.0, 0.4 * (n % 2))
        return _clear_upper(c)
    return _settle(make, thr)


def _spread(count, rng, top, bottom=1e-20, sign=0):
    """``count`` values of magnitudes 1e-20 .. top (log-uniform) with zeros and denormals among them; sign: -1, +1 or 0 = both."""
    v = 10.0 ** rng.uniform(math.log10(bottom), math.log10(top), count)
    v *= rng.choice([-1.0, 1.0], count) if sign == 0 else sign
    special = {0: [0.0, -0.0, 3e-41, -7e-42], 1: [0.0, 3e-41], -1: [-0.0, -7e-42]}[sign]
    v[: len(special)] = special
    return v


def _split_column(rng, n, qs, edges, fillers):
    """n values, ascending: the ranks up to floor(q (n - 1)) of every q in ``qs`` (ascending) end a part; part j is drawn by
    fillers[j] ((lo, hi) uniform, or a callable count -> values) and the two values either side of boundary j are edges[j]."""
    cuts = [int(math.floor(float(np.float32(q) * np.float32(n - 1)))) + 1 for q in qs] + [n]
    out, first = [], 0
    for j, last in enumerate(cuts):
        v = np.sort(fillers[j](last - first) if callable(fillers[j]) else rng.uniform(*fillers[j], last - first))
        assert len(v) >= 2
        if j > 0:
            v[0] = edges[j - 1][1]
        if j < len(qs):
            v[-1] = edges[j][0]
        out.append(v)
        first = last
    return np.concatenate(out)


def _assign(flat, col, members, values, bottom, top, rng):
    """flat[members, col] = the ascending ``values`` in a random order, but ``bottom`` receive the smallest and ``top`` the largest."""
    fixed = set(int(v) for v in bottom) | set(int(v) for v in top)
    rest = rng.permutation(np.array([m for m in members if int(m) not in fixed], dtype=np.int64))
    order = np.concatenate([np.array(bottom, dtype=np.int64), rest, np.array(top, dtype=np.int64)])
    assert len(order) == len(values) == len(set(order.tolist()))
    flat[order, col] = values


def _corner_sets(flat, inst, N, members, signed):
    """Per instance four distinct members, one per quadrant (q0: +x +z, q1: +x -z, q2: -x -z, q3: -x +z): with ``signed`` the z of the
    member already has the quadrant's sign (the default rule tests z itself); else the first four members (Fauna: z is assigned)."""
    Q = [[], [], [], []]
    for i in range(N):
        idx = [m for m in members if inst[m] == i]
        if signed:
            pos, neg = [m for m in idx if flat[m, 2] > 0], [m for m in idx if flat[m, 2] < 0]
            pick = [pos[0], neg[0], neg[1], pos[1]]
        else:
            pick = idx[:4]
        assert len(set(pick)) == 4
        for q in range(4):
            Q[q].append(pick[q])
    return Q


BYTE_EDGE = 2.0 ** 65  # a float whose exponent field is even: the top byte of the key changes here


@functools.lru_cache(maxsize=None)
def exponents(N, thr, narrow=False, V=180, seed=202):
    """The ranked columns over the whole exponent range: both signs, +-0.0, denormals, 1e-20 .. 1e20.  Default rule: the x of every
    vertex (x reaches no inexact output: the centroid's x is snapped to 0); the neighbours of the two quantiles straddle +-2^65, where
    the top byte of the key changes: four targets, four first-pass bins.  Fauna: the x and z of the LOW vertices; the six neighbours of a
    coordinate are -2^65 (1 +- 0.01), -0.0 / +0.0 and 2^65 (1 +- 0.01): six first-pass bins.  ``narrow`` (Fauna): the low vertices' x and
    z in [2, 7.9): the twelve targets share their top byte."""
    B = BYTE_EDGE

    def make(s):
        rng = np.random.default_rng(seed + s)
        c = _cloud(N, V, seed + s)
        flat = c.reshape(-1, 3)
        n, inst = N * V, np.repeat(np.arange(N), V)
        outer = lambda sign: (lambda count: sign * 10.0 ** rng.uniform(math.log10(1.02 * B), 20.0, count))  # noqa: E731
        if thr is None:
            Q = _corner_sets(flat, inst, N, range(n), True)
            vals = _split_column(rng, n, (0.05, 0.95), [(-1.01 * B, -0.99 * B), (0.99 * B, 1.01 * B)],
                                 [outer(-1.0), lambda count: _spread(count, rng, 0.98 * B), outer(1.0)])
            _assign(flat, 0, np.arange(n), vals, Q[2] + Q[3], Q[0] + Q[1], rng)
            zeros = np.nonzero(flat[:, 0] == 0)[0]
            flat[zeros[0], 0], flat[zeros[1], 0] = 0.0, -0.0  # (a vectorised sort may hand back zeros of one sign)
            return c
        low = np.nonzero(flat[:, 1] < quantile(flat[:, 1].astype(np.float32), thr)["value"])[0]
        if narrow:
            flat[low, 0], flat[low, 2] = rng.uniform(2.0, 7.9, len(low)), rng.uniform(2.0, 7.9, len(low))
            return c
        Q = _corner_sets(flat, inst, N, low, False)
        for col, bottom, top in ((0, Q[2] + Q[3], Q[0] + Q[1]), (2, Q[1] + Q[2], Q[0] + Q[3])):
            vals = _split_column(rng, len(low), (0.05, 0.5, 0.95), [(-1.01 * B, -0.99 * B), (-0.0, 0.0), (0.99 * B, 1.01 * B)],
                                 [outer(-1.0), lambda count: _spread(count, rng, 0.98 * B, sign=-1),
                                  lambda count: _spread(count, rng, 0.98 * B, sign=1), outer(1.0)])
            _assign(flat, col, low, vals, bottom, top, rng)
        return c
    return _settle(make, thr)


def top_byte(f):
    return key_of(f) >> 24


def key_of(f):
    """The monotone 32-bit key of the radix select."""
    u = int(np.array([f], dtype=np.float32).view(np.uint32)[0])
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def first_differing_byte(a, b):
    """The first byte (0 = top) in which the select keys of two float32 values differ; 4: equal."""
    x = key_of(a) ^ key_of(b)
    return 4 if x == 0 else (32 - x.bit_length()) // 8


@functools.lru_cache(maxsize=None)
def duplicates(N, thr, distinct, V, seed=303):
    """Every column drawn from ``distinct`` values per side: the neighbours of every quantile are equal, all targets of a coordinate share
    one histogram through all four passes; with N V > 1024 values some first-pass bin holds more than 1024.  Unique spine ends."""
    lv = np.array([0.5, 0.75, 1.0, 1.25, 1.5])[:distinct]

    def make(s):
        rng = np.random.default_rng(seed + s)
        k = np.arange(V) % 5
        sx = np.where((k == 1) | (k == 2), 1.0, -1.0)
        sz = np.where((k == 1) | (k == 4), 1.0, -1.0)
        c = np.zeros((N, V, 3))
        for n in range(N):
            body = k == 0
            c[n, :, 0] = np.where(body, rng.choice([-0.0625, 0.0625], V), sx * rng.choice(lv, V))
            c[n, :, 1] = np.where(body, rng.choice(lv, V), -rng.choice(lv, V))
            c[n, :, 2] = np.where(body, rng.choice(np.concatenate([-lv, lv]), V), sz * rng.choice(lv, V))
            o = 5 * ((7 * n) % (V // 5 - 2))
            c[n, o] = [0.0625, 0.5, 1.75]
            c[n, o + 5] = [-0.0625, 0.75, -1.75]
        return c
    return _settle(make, thr)


def _up(base, byte):
    """The float above ``base`` (> 0, mantissa bits clear) whose key first differs from base's in byte ``byte`` (1..3; 0 = top byte)."""
    bits = np.array([base], dtype=np.float32).view(np.uint32)
    bits |= np.uint32({1: 0x400000, 2: 0xFF00, 3: 0xFF}[byte])
    return float(bits.view(np.float32)[0])


@functools.lru_cache(maxsize=None)
def byte_split(byte, N, thr, V=150, seed=404):
    """The two neighbours of every ranked quantile first differ in byte ``byte`` (0 = top) of their keys, and agree above it: the targets
    of a coordinate leave their shared histogram at that pass.  Default rule: the pooled x column; Fauna: the pooled y column and the x
    and z of the low vertices.  (N V = 300 or 4950: the weights of the threshold and of the medians are 0.6 and 0.5 -- the low count is
    even --, so a pair 255 ulp apart still leaves both neighbours 64 units from the interpolated value.)"""
    if byte == 0:
        e3 = [(-0.75, 0.001), (0.9, 2.5)]
        f3 = [(-1.5, -0.8), (0.01, 0.85), (2.6, 3.0)]
        e4 = [(-0.75, 0.001), (0.4, 0.6), (1.9, 2.5)]
        f4 = [(-1.5, -0.8), (0.01, 0.39), (0.61, 1.89), (2.6, 3.0)]
        e2, f2 = [(-0.75, 0.001)], [(-1.5, -0.8), (0.01, 1.0)]
    else:
        h, e = _up(0.5, byte), _up(0.125, byte)
        e3 = [(-h, -0.5), (0.5, h)]
        f3 = [(-1.5, -0.8), (-0.45, 0.45), (0.8, 1.5)]
        e4 = [(-h, -0.5), (0.125, e), (0.5, h)]
        f4 = [(-1.5, -0.8), (-0.45, 0.1), (0.2, 0.45), (0.8, 1.5)]
        e2, f2 = [(-h, -0.5)], [(-1.5, -0.8), (-0.45, 1.0)]

    def make(s):
        rng = np.random.default_rng(seed + 10 * s + byte)
        c = _cloud(N, V, seed + s)
        flat = c.reshape(-1, 3)  # (a view: c is contiguous)
        n, inst = N * V, np.repeat(np.arange(N), V)
        if thr is None:
            Q = _corner_sets(flat, inst, N, range(n), True)
            _assign(flat, 0, np.arange(n), _split_column(rng, n, (0.05, 0.95), e3, f3), Q[2] + Q[3], Q[0] + Q[1], rng)
            return c
        order = rng.permutation(n)
        flat[order, 1] = _split_column(rng, n, (thr,), e2, f2)
        n_low = int(math.floor(float(np.float32(thr) * np.float32(n - 1)))) + 1
        low = order[:n_low]
        for col in (0, 2):
            flat[rng.permutation(low), col] = _split_column(rng, n_low, (0.05, 0.5, 0.95), e4, f4)
        return _clear_upper(c)
    return _settle(make, thr)


def _counts_cloud(rng, n_total, n_low):
    """n_total vertices, vertex v in top-view quadrant v % 4, of which the first n_low lie far below the others in y."""
    c = np.zeros((n_total, 3))
    quadrant = np.arange(n_total) % 4
    c[:, 0] = np.where(quadrant < 2, 1.0, -1.0) * (0.3 + 0.6 * rng.random(n_total))
    c[:, 2] = np.where((quadrant == 0) | (quadrant == 3), 1.0, -1.0) * (0.3 + 0.6 * rng.random(n_total))
    c[:, 1] = 0.1 + 0.8 * rng.random(n_total)
    c[:n_low, 1] -= 2.0
    return c


@functools.lru_cache(maxsize=None)
def counts(n_total, thr, seed=505):
    """ONE instance of n_total points: small pooled counts, weights exactly 0 (n = 21, 41: q (n - 1) is whole for 0.05, 0.95 and 0.5) and
    both branches of the interpolation.  (Four quadrants need four points: the counts 2 and 3 appear as LOW counts, ``low_counts``.)"""
    return _settle(lambda s: _counts_cloud(np.random.default_rng(seed + 100 * s + n_total), n_total, n_total // 2)[None], thr)


def low_threshold(n_low, total):
    """A quantile q whose position q (total - 1) lies between the ranks n_low - 1 and n_low: the threshold falls into the wide gap above
    the n_low lowest y, so that exactly n_low vertices are low."""
    return (n_low - 0.25) / (total - 1)


@functools.lru_cache(maxsize=None)
def low_counts(n_low, N=2, V=40, seed=606):
    """Fauna calls whose low set has exactly n_low members, with every quadrant of every instance populated (by the vertices that are not
    low: the quadrant tests run over all vertices)."""
    def make(s):
        c = _counts_cloud(np.random.default_rng(seed + 100 * s + n_low), N * V, n_low)
        c[0, 0], c[0, 2] = 0.5, 0.5  # (the single low vertex of n_low = 1 sits inside its cluster: something lies beyond it on every side)
        return c.reshape(N, V, 3)
    return _settle(make, low_threshold(n_low, N * V))


@functools.lru_cache(maxsize=None)
def layout(N, V, thr, seed=707):
    return _settle(lambda s: _cloud(N, V, seed + 1000 * s + 31 * N + V), thr)


def compaction_thr(kind):
    if kind == "empty_chunk":
        return 0.3
    if kind == "full_wave":
        return low_threshold(64, 3 * 1024)
    j = np.arange(1000 - 48)
    return low_threshold(int((((48 + j) % 5 != 0) & (j % 13 == 0)).sum()), 3 * 1000)


@functools.lru_cache(maxsize=None)
def compaction(kind, N=3, seed=808):
    """Fauna ballot compaction of the one-group kernel (1024 points per trip, 64 per wave): ``empty_chunk`` -- instance 1 (V = 1024: one
    whole trip) has no low vertex; ``full_wave`` -- the 64 points of one wave are the low set; ``last_partial`` -- V = 1000: every low
    vertex lies in the last, partial trip (points 2048 .. 2999)."""
    V = 1000 if kind == "last_partial" else 1024

    def make(s):
        c = _cloud(N, V, seed + s)
        k = np.arange(V) % 5
        if kind == "empty_chunk":
            c[1, :, 1] += 1.0
        elif kind == "full_wave":
            c[:, :, 1] += 1.0
            j = np.arange(64)
            c[0, 128:192, 1] -= 2.0
            c[0, 128:192, 0] = np.where(j % 2 == 0, 1.0, -1.0) * (0.2 + 0.01 * j)
            c[0, 128:192, 2] = np.where(j % 4 < 2, 1.0, -1.0) * (0.2 + 0.011 * j)
        else:
            c[:, :, 1] += 1.0
            tail = np.arange(48, V)  # points 2048.. of the call = vertices 48.. of instance 2
            c[2, tail, 1] -= np.where(k[tail] != 0, 2.0, 0.0) * (np.arange(len(tail)) % 13 == 0)
        return _clear_upper(c)
    return _settle(make, compaction_thr(kind))


def wpi_of(N):
    w = 16
    while w > 1 and 16 // w < N:
        w >>= 1
    return w


@functools.lru_cache(maxsize=None)
def ties(N, kind, thr, seed=909):
    """Tied spine maxima, spine minima and feet of quadrant 0 in every instance.  kind: ``wave`` -- the pair is (v, v + 64): another wave
    of the instance when wpi > 1; ``trip`` -- (v, v + 64 wpi): the same lane one trip later; ``lane`` -- lane 63 against lane 0 of the next
    wave.  The members of a pair differ by >= 0.1 in their other coordinates.  (N = 33: the wide path, 256 threads per trip.)"""
    wpi = wpi_of(N) if N <= 32 else 4
    V = 64 * wpi * 2 + 70
    pairs = tie_pairs(N, kind)

    def make(s):
        c = _cloud(N, V, seed + 50 * s + N)
        for n in range(N):
            for j, v in enumerate(pairs["z_max"]):
                c[n, v] = [0.05, 0.3 + 0.2 * j, 1.5]
            for j, v in enumerate(pairs["z_min"]):
                c[n, v] = [-0.05, 0.5 - 0.2 * j, -1.5]
            for j, v in enumerate(pairs["foot0"]):
                c[n, v] = [0.4 + 0.1 * j, -2.0, 0.5 + 0.2 * j]
        return c
    return _settle(make, thr)


def tie_pairs(N, kind):
    wpi = wpi_of(N) if N <= 32 else 4
    d = {"wave": 64, "trip": 64 * wpi}.get(kind)
    if kind == "lane":
        return {"z_max": (63, 64), "z_min": (63 + 64 * max(wpi, 2), 64 + 64 * max(wpi, 2)), "foot0": (127, 128)}
    return {"z_max": (5, 5 + d), "z_min": (10, 10 + d), "foot0": (16, 16 + d)}


def _balance(col, free, target_sum, step, lo, hi, most=0.25):
    """Moves ``free`` entries of ``col`` by multiples of ``step`` (at most ``most`` each, staying in [lo, hi]) until the column sums to
    ``target_sum`` exactly."""
    d = target_sum - col.sum()
    assert abs(d / step - round(d / step)) < 1e-9
    d = round(d / step) * step
    for v in free:
        if d == 0:
            break
        move = max(min(d, hi - col[v], most), lo - col[v], -most)
        move = math.trunc(move / step) * step
        col[v] += move
        d -= move
    assert d == 0, "not enough free vertices to balance the column"


CY, CZ = -0.5, 0.25  # the lattice family's centroid (y, z) of every instance


@functools.lru_cache(maxsize=None)
def lattice(N, fauna, V=256, seed=1010):
    """See the module docstring.  x, z multiples of 2^-2 in [-1.5, 1.5] / [-2, 2], y multiples of 2^-3 in [-2, 1): ties everywhere; the
    column sums are exact in float32 in any order and the centroid is (., CY, CZ) exactly.  Instance n is instance 0 with its vertices
    rotated by 37 n places.  Special vertices (indices in ``lattice_specials``) sit on the boundaries and one float32 step beyond."""
    rng = np.random.default_rng(seed + int(fauna))
    c = np.zeros((V, 3))
    c[:, 0] = rng.choice(np.arange(-6, 7) * 0.25, V)
    c[:, 1] = rng.choice(np.arange(-16, 8) * 0.125, V)
    c[:, 2] = rng.choice(np.arange(-8, 9) * 0.25, V)
    c[c[:, 2] == 0, 2] = 0.25
    sp = lattice_specials(fauna)
    if fauna:
        # the low set, in blocks wide enough that the ranks of every quantile fall inside one (for every N: instances are copies):
        # 84 free low vertices + 6 special ones below the 30 vertices ON the threshold (pooled ranks 90 N .. 120 N hold 0.4 (256 N - 1))
        low = [v for v in range(V) if v not in sp["all"]][:84]
        c[low, 0] = rng.permutation(np.repeat([-1.5, -0.5, 0.0, 0.5, 1.5], [13, 25, 8, 25, 13]))
        c[low, 2] = rng.permutation(np.repeat([-1.5, -0.75, 0.25, 1.0, 2.0], [13, 25, 8, 25, 13]))
        c[low, 1] = rng.choice([-2.0, -1.75, -1.5], 84)
        rest = [v for v in range(V) if v not in sp["all"] and v not in low]
        c[rest, 1] = rng.choice([0.25, 0.5, 0.75], len(rest))
        c[sp["on_thr"]] = [1.5, -1.25, 2.0]  # counted as low they would move the medians of x and z
    thr = 0.4 if fauna else None
    nxt = lambda v, to: float(np.nextafter(np.float32(v), np.float32(to)))  # noqa: E731
    for _ in range(8):
        r = reference(_t(c[None]).numpy(), 8, 3, "z_minmax_y+", thr, f32_margin=True)
        before = c.copy()
        if not fauna:
            m = r["margin"]
            c[sp["on_margin"]] = [m, -3.0, 1.0]
            c[sp["past_margin"]] = [nxt(m, 9), -2.75, -1.3125]  # z: midway between the ends of body bones 5 and 6
            c[sp["on_neg_margin"]] = [-m, -3.0, -1.0]
            c[sp["past_neg_margin"]] = [nxt(-m, -9), -2.75, 1.0]
            c[sp["zero"]] = [1.5, -3.25, 0.0]
            c[sp["neg_zero"]] = [-1.5, -3.25, -0.0]
            c[sp["past_zero"]] = [1.5, -2.875, TINY]
            c[sp["past_neg_zero"]] = [-1.5, -2.875, -TINY]
            c[sp["tied_foot_a"]] = [-1.25, -2.75, 1.5]  # quadrant 3: three vertices share the lowest y (with past_neg_margin, the first)
            c[sp["tied_foot_b"]] = [-1.0, -2.75, 1.75]
        else:
            x0, z0, mx, mz = r["centre"]
            c[sp["on_mx"]] = [x0 + mx, -3.0, z0 - 1.0]
            c[sp["past_mx"]] = [nxt(x0 + mx, 9), -2.75, z0 - 1.0]
            c[sp["on_mz"]] = [1.5, -3.25, z0 + mz]
            c[sp["past_mz"]] = [1.5, -2.875, nxt(z0 + mz, 9)]
            c[sp["on_z0"]] = [-1.5, -3.0, z0]
            c[sp["past_z0"]] = [-1.5, -2.75, nxt(z0, -9)]
            assert r["y_threshold"] == -1.25 and (x0, z0) == (0.0, 0.25)
        c[sp["on_upper"]] = [0.25, CY - 0.5, 2.25]      # the largest z of all, ON y == cy - 0.5: not upper
        c[sp["head"]] = [0.25, 0.5, 2.0]
        c[sp["head_twin"]] = [-0.5, 0.75, 2.0]           # tied with ``head``, a higher index
        c[sp["tail"]] = [0.25, CY - 0.5 + 0.125, -2.25]  # the smallest z of all, one lattice step above the bound: upper
        free = [v for v in range(V) if v not in sp["all"] and not (fauna and v in low)]
        _balance(c[:, 1], free, CY * V, 0.125, -0.75 if fauna else -2.0, 0.875)
        if not fauna:  # (Fauna: two z values one float32 step off the lattice -- the centroid's z feeds no decision there)
            _balance(c[:, 2], [v for v in free if 0.5 <= abs(c[v, 2]) <= 1.5], CZ * V, 0.0625, -1.75, 1.75)
        if np.array_equal(before, c):
            break
    else:
        raise AssertionError("the lattice case did not settle")
    return _t(np.stack([np.roll(c, 37 * n, axis=0) for n in range(N)]))


def lattice_specials(fauna):
    if not fauna:
        names = ["on_margin", "past_margin", "on_neg_margin", "past_neg_margin", "zero", "neg_zero", "past_zero", "past_neg_zero",
                 "tied_foot_a", "tied_foot_b"]
    else:
        names = ["on_mx", "past_mx", "on_mz", "past_mz", "on_z0", "past_z0"]
    sp = {k: 20 + 9 * i for i, k in enumerate(names)}
    sp.update(on_upper=150, head=120, head_twin=190, tail=140)
    if fauna:
        sp["on_thr"] = list(range(200, 230))
    sp["all"] = set(v for k, val in sp.items() for v in (val if isinstance(val, list) else [val]))
    return sp


@functools.lru_cache(maxsize=None)
def lattice_negzero(N, V=128, seed=1111):
    """The arg-min among signed zeros: every y >= 0 on a lattice, and in every quadrant the lowest y is 0 twice -- +0.0 at the lower index
    and -0.0 at the higher one, different in x and z.  The smallest z (the spine minimum, 'z_minmax') is likewise +0.0 then -0.0 ...
    of a column shifted to z >= 0 would empty two quadrants, so the spine keeps ordinary values."""
    rng = np.random.default_rng(seed)
    c = np.zeros((V, 3))
    c[:, 0] = rng.choice(np.array([-1.5, -1.25, -1.0, 1.0, 1.25, 1.5]), V)
    c[:, 1] = rng.choice(np.arange(1, 16) * 0.125, V)
    c[:, 2] = rng.choice(np.array([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5]), V)
    c[3] = [0.25, 1.0, 2.0]
    c[4] = [0.25, 1.0, -2.0]
    for q, (sx, sz) in enumerate([(1, 1), (1, -1), (-1, -1), (-1, 1)]):
        c[10 + q] = [1.0 * sx, 0.0, 0.5 * sz]
        c[80 + q] = [1.5 * sx, -0.0, 1.5 * sz]
    return _t(np.stack([np.roll(c, 37 * n, axis=0) for n in range(N)]))


@functools.lru_cache(maxsize=None)
def ordinary(N, thr, V=300, seed=1212):
    return _settle(lambda s: _cloud(N, V, seed + s), thr)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _case(maker, args, mode="z_minmax_y+", thr=None, n_body=8, n_leg=3, prescribed=None, cached=None, f32_margin=False):
    return dict(maker=maker, args=args, mode=mode, thr=thr, n_body=n_body, n_leg=n_leg, prescribed=prescribed, cached=cached,
                f32_margin=f32_margin)


def _build_cases():
    c = {}
    D, FA = dict(thr=None), dict(thr=0.4)
    variants = (("", None), ("_fauna", 0.4))
    for N in (1, 6, 32, 33):
        for tag, thr in variants:
            c[f"pooled{tag}_N{N}"] = _case("pooled", (N, thr), thr=thr)
    for N in (3, 33):
        c[f"exponents_N{N}"] = _case("exponents", (N, None), **D)
        c[f"exponents_fauna_N{N}"] = _case("exponents", (N, 0.4), **FA)
        c[f"exponents_fauna_narrow_N{N}"] = _case("exponents", (N, 0.4, True), **FA)
    for N, V in ((2, 1500), (33, 150)):
        for d in (3, 5):
            for tag, thr in variants:
                c[f"duplicates_{d}{tag}_N{N}"] = _case("duplicates", (N, thr, d, V), thr=thr)
    for byte in range(4):
        for N in (2, 33):
            for tag, thr in variants:
                c[f"bytes_{byte}{tag}_N{N}"] = _case("byte_split", (byte, N, thr), thr=thr)
    for n in COUNTS:
        c[f"counts_n{n}"] = _case("counts", (n, None), **D)
        if n > 4:  # (two low vertices of four leave one of the +x quadrants empty)
            c[f"counts_fauna_n{n}"] = _case("counts", (n, 0.5), thr=0.5)
    for n_low in LOW_COUNTS:
        c[f"low_counts_{n_low}"] = _case("low_counts", (n_low,), thr=low_threshold(n_low, 80))
    for N, V in LAYOUTS:
        for tag, thr in variants:
            c[f"layout{tag}_N{N}_V{V}"] = _case("layout", (N, V, thr), thr=thr)
    for kind in ("empty_chunk", "full_wave", "last_partial"):
        c[f"compaction_{kind}"] = _case("compaction", (kind,), thr=compaction_thr(kind))
    for N in (1, 5, 20, 33):
        for kind in ("wave", "trip", "lane"):
            c[f"ties_{kind}_N{N}"] = _case("ties", (N, kind, None), **D)
        c[f"ties_wave_fauna_N{N}"] = _case("ties", (N, "wave", 0.4), **FA)
    for N in (1, 5, 20, 33):
        c[f"lattice_N{N}"] = _case("lattice", (N, False), f32_margin=True, **D)
        c[f"lattice_fauna_N{N}"] = _case("lattice", (N, True), f32_margin=True, **FA)
        c[f"lattice_negzero_N{N}"] = _case("lattice_negzero", (N,), mode="z_minmax", f32_margin=True, **D)
    for N in (3, 33):
        for nb in (2, 4, 6, 32):
            c[f"skeleton_body{nb}_N{N}"] = _case("ordinary", (N, None), n_body=nb, n_leg=2 if nb != 32 else 8, **D)
        for nl in (1, 2, 8):
            c[f"skeleton_leg{nl}_N{N}"] = _case("ordinary", (N, 0.4), n_leg=nl, **FA)
        c[f"skeleton_nolegs_N{N}"] = _case("ordinary", (N, None), n_body=6, n_leg=0, mode="z_minmax")
        c[f"skeleton_prescribed_N{N}"] = _case("ordinary", (N, None), prescribed=(1, 6, None, None), **D)
        c[f"skeleton_half_prescribed_N{N}"] = _case("ordinary", (N, 0.4), prescribed=(None, 4, None, None), **FA)
        c[f"skeleton_cached4_N{N}"] = _case("ordinary", (N, None), cached=(0, 7, 5, 2), **D)
    return c


COUNTS = (4, 5, 21, 41, 27, 35)           # pooled counts: the smallest that populate four quadrants, weight 0 (21, 41), both lerp branches
LOW_COUNTS = (1, 2, 3, 21, 41, 27, 35)    # low counts
LAYOUTS = ((1, 65), (1, 2049), (2, 1025), (3, 1024), (5, 1023), (9, 65), (9, 2049), (16, 1025), (17, 65), (17, 1024), (32, 1023), (32, 2049))
CASES = _build_cases()
LATTICE = tuple(n for n in CASES if n.startswith("lattice"))
# Every family runs on the one-group kernel (N <= 32) and on the wide path (N = 33) against this same reference.  Where the instances
# of the two are literally shared AND the pooled quantities coincide, the two results can also be held against each other: the lattice
# family (instance n = instance 0 rotated by 37 n places; the pooled quantiles sit inside blocks of equal values for every N).
TWINS = [(f"lattice{tag}_N{N}", f"lattice{tag}_N33") for tag in ("", "_fauna", "_negzero") for N in (1, 5, 20)]


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]
    seq = globals()[c["maker"]](*c["args"])
    assert seq.dtype == torch.float32 and seq.dim() == 4 and seq.shape[0] * seq.shape[1] * seq.shape[2] <= 70000
    return seq


@functools.lru_cache(maxsize=None)
def expected(name, mutate=None):
    c = CASES[name]
    return reference(build(name).numpy(), c["n_body"], c["n_leg"], c["mode"], c["thr"], c["prescribed"], c["cached"], c["f32_margin"], mutate)


def kwargs(name):
    """The arguments of skinning.estimate_bones for a chain rebuild of the case (a cached-aux case rebuilds with its first two joints)."""
    c = CASES[name]
    kw = dict(n_body_bones=c["n_body"], n_legs=4, n_leg_bones=c["n_leg"], body_bones_mode=c["mode"], bone_y_threshold=c["thr"])
    if c["prescribed"] is not None:
        kw["legs_to_body_joint_indices"] = list(c["prescribed"])
    return kw


def cached_aux(name):
    """The hand-built aux of a cached-chain case: bones_to_joints, chain and four legs with their own body_bone_idx."""
    c = CASES[name]
    assert c["cached"] is not None
    legs = [{"body_bone_idx": int(j), "leg_bones_to_joints": [(i + 1, i) for i in range(c["n_leg"])]} for j in c["cached"]]
    return {"bones_to_joints": body_pairs(c["n_body"]), "kinematic_chain": chain_of(c["n_body"], c["n_leg"], list(c["cached"])), "legs": legs}


MEASURED = {
    "pooled_N1": 2.305,
    "pooled_fauna_N1": 2.434,
    "pooled_N6": 2.799,
    "pooled_fauna_N6": 2.633,
    "pooled_N32": 2.827,
    "pooled_fauna_N32": 2.827,
    "pooled_N33": 2.849,
    "pooled_fauna_N33": 2.849,
    "exponents_N3": 2.638,
    "exponents_fauna_N3": 2.245,
    "exponents_fauna_narrow_N3": 2.424,
    "exponents_N33": 2.83,
    "exponents_fauna_N33": 2.819,
    "exponents_fauna_narrow_N33": 2.803,
    "duplicates_3_N2": 2.0,
    "duplicates_3_fauna_N2": 2.0,
    "duplicates_5_N2": 2.0,
    "duplicates_5_fauna_N2": 2.0,
    "duplicates_3_N33": 2.0,
    "duplicates_3_fauna_N33": 2.0,
    "duplicates_5_N33": 2.0,
    "duplicates_5_fauna_N33": 2.0,
    "bytes_0_N2": 2.476,
    "bytes_0_fauna_N2": 2.462,
    "bytes_0_N33": 2.788,
    "bytes_0_fauna_N33": 2.827,
    "bytes_1_N2": 2.819,
    "bytes_1_fauna_N2": 2.704,
    "bytes_1_N33": 2.66,
    "bytes_1_fauna_N33": 2.85,
    "bytes_2_N2": 2.817,
    "bytes_2_fauna_N2": 2.653,
    "bytes_2_N33": 2.836,
    "bytes_2_fauna_N33": 3.076,
    "bytes_3_N2": 2.578,
    "bytes_3_fauna_N2": 2.674,
    "bytes_3_N33": 2.786,
    "bytes_3_fauna_N33": 2.842,
    "counts_n4": 2.306,
    "counts_n5": 2.359,
    "counts_fauna_n5": 2.472,
    "counts_n21": 2.467,
    "counts_fauna_n21": 2.607,
    "counts_n41": 2.678,
    "counts_fauna_n41": 2.678,
    "counts_n27": 2.562,
    "counts_fauna_n27": 2.493,
    "counts_n35": 2.78,
    "counts_fauna_n35": 2.194,
    "low_counts_1": 2.463,
    "low_counts_2": 2.359,
    "low_counts_3": 2.42,
    "low_counts_21": 2.293,
    "low_counts_41": 2.514,
    "low_counts_27": 2.557,
    "low_counts_35": 2.551,
    "layout_N1_V65": 2.746,
    "layout_fauna_N1_V65": 2.746,
    "layout_N1_V2049": 1.984,
    "layout_fauna_N1_V2049": 1.984,
    "layout_N2_V1025": 2.575,
    "layout_fauna_N2_V1025": 2.284,
    "layout_N3_V1024": 2.607,
    "layout_fauna_N3_V1024": 2.28,
    "layout_N5_V1023": 2.819,
    "layout_fauna_N5_V1023": 2.844,
    "layout_N9_V65": 2.634,
    "layout_fauna_N9_V65": 2.638,
    "layout_N9_V2049": 2.705,
    "layout_fauna_N9_V2049": 2.705,
    "layout_N16_V1025": 2.825,
    "layout_fauna_N16_V1025": 2.825,
    "layout_N17_V65": 2.608,
    "layout_fauna_N17_V65": 2.608,
    "layout_N17_V1024": 2.664,
    "layout_fauna_N17_V1024": 2.822,
    "layout_N32_V1023": 2.755,
    "layout_fauna_N32_V1023": 2.776,
    "layout_N32_V2049": 2.81,
    "layout_fauna_N32_V2049": 2.856,
    "compaction_empty_chunk": 2.785,
    "compaction_full_wave": 2.778,
    "compaction_last_partial": 2.684,
    "ties_wave_N1": 2.5,
    "ties_trip_N1": 2.5,
    "ties_lane_N1": 2.5,
    "ties_wave_fauna_N1": 2.5,
    "ties_wave_N5": 2.638,
    "ties_trip_N5": 2.638,
    "ties_lane_N5": 2.638,
    "ties_wave_fauna_N5": 2.638,
    "ties_wave_N20": 2.786,
    "ties_trip_N20": 2.786,
    "ties_lane_N20": 2.786,
    "ties_wave_fauna_N20": 2.786,
    "ties_wave_N33": 2.83,
    "ties_trip_N33": 2.833,
    "ties_lane_N33": 2.83,
    "ties_wave_fauna_N33": 2.833,
    "lattice_N1": 2.0,
    "lattice_fauna_N1": 2.0,
    "lattice_negzero_N1": 2.0,
    "lattice_N5": 2.0,
    "lattice_fauna_N5": 2.0,
    "lattice_negzero_N5": 2.0,
    "lattice_N20": 2.0,
    "lattice_fauna_N20": 2.0,
    "lattice_negzero_N20": 2.0,
    "lattice_N33": 2.0,
    "lattice_fauna_N33": 2.0,
    "lattice_negzero_N33": 2.0,
    "skeleton_body2_N3": 0.573,
    "skeleton_body4_N3": 0.785,
    "skeleton_body6_N3": 1.757,
    "skeleton_body32_N3": 1.359,
    "skeleton_leg1_N3": 1.007,
    "skeleton_leg2_N3": 1.007,
    "skeleton_leg8_N3": 1.419,
    "skeleton_nolegs_N3": 2.026,
    "skeleton_prescribed_N3": 2.625,
    "skeleton_half_prescribed_N3": 2.653,
    "skeleton_cached4_N3": 2.625,
    "skeleton_body2_N33": 0.99,
    "skeleton_body4_N33": 1.119,
    "skeleton_body6_N33": 1.798,
    "skeleton_body32_N33": 1.525,
    "skeleton_leg1_N33": 1.007,
    "skeleton_leg2_N33": 1.119,
    "skeleton_leg8_N33": 1.602,
    "skeleton_nolegs_N33": 2.338,
    "skeleton_prescribed_N33": 2.838,
    "skeleton_half_prescribed_N33": 2.838,
    "skeleton_cached4_N33": 2.838,
}
