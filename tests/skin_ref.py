"""Float64 restatement of the posing path (csrc/skin.hip, csrc/bones.hip, csrc/bones_common.h), written from its definition:

    rest frame of a bone a -> b   f = normalize(b - a), up = normalize(f x (1,0,0)), right = up x f, R = [right | up | f]  (columns)
    link                          L_i = [ R_i Rot_i R_i^T | a_i - R_i Rot_i R_i^T a_i ],  Rot = Rx(x) Ry(y) Rz(z)
    transform of bone k           M_k = L_c0 L_c1 ... L_k over the bone's chain (root first; the int table [K,D], -1 = no link)
    weights                       w_k(p) = softmax_k( -sqrt(|closest point of segment k - p|^2 + 1e-6) / temperature ),  p detached
    posed vertex                  sum_k w_k(p) (M_k [p, 1])

normalize() is torch's (x / max(|x|, 1e-12)), so a zero-length bone or a bone along +-x yields the same singular frame as the kernel
and the reference: nothing is special-cased.  Plain torch; every function takes a dtype; gradients come from autograd.

Beside each value the module evaluates its MAGNITUDE (tests/deriv_ref.py: the same expression with absolute values and additions for
subtractions), and errors are measured in units of 2^-24 x magnitude.  Two magnitudes are not a plain absolute-value restatement:

  * a logit's magnitude is what a float32 rounding of its inputs moves it by, over 2^-24: (|s| . (t |d| + |r|)) / dist / temperature + |l|
    with r = p - a, s = t d - r (the difference of two long vectors for a vertex near a bone);
  * a weight's magnitude carries the softmax's conditioning, w_k (1 + sum_j |delta_kj - w_j| mag(l_j)): at temperature 1e-3 a logit is
    ~1000 and one ulp of it moves a near-tied weight by 1e-4 -- in these units that is still O(1), so one table serves every
    temperature.  Wherever a weight enters another quantity's magnitude, this magnitude stands for it.

MEASURED holds, per case and quantity, what the torch float32 path (model/geometry/skinning.py: bone_transforms_torch, and the torch
blend of tests/test_gpu_parity.py) reaches against this restatement; tests/test_skin_cpu.py measures it afresh and compares.  The
kernels' bound for a case and quantity is 4 x that measured figure in these units plus 4 ulp of the float64 value (``violations``, as
in the derivative suite); nothing else enters it.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from deriv_ref import EPS, units, violations  # noqa: F401  (the same unit and the same bound as the derivative suite)

F64 = torch.float64
TINY = 2.0 ** -102  # 2^-126 / 2^-24: a weight below the float32 normal range may come back as zero
FACTOR = 4.0
KEYS = ("out", "T", "w", "g_v", "g_T", "g_angles")


# ---------------------------------------------------------------------------------------------------------------- restatement
def bcast(x, B):
    """The 1-or-B rule: a leading dimension of 1 is shared by the B images."""
    assert x.shape[0] in (1, B), (tuple(x.shape), B)
    return x.expand(B, *x.shape[1:])


def logits(v, bones, temperature, dtype=F64):
    """(l, mag_l) [Bw,K,V], Bw = max(batch of v, batch of bones); the vertices are detached."""
    v, bones = v.detach().to(dtype), bones.detach().to(dtype)
    Bw = max(v.shape[0], bones.shape[0])
    p = bcast(v, Bw)[:, None]                    # [Bw,1,V,3]
    a = bcast(bones, Bw)[:, :, 0][:, :, None]    # [Bw,K,1,3]
    d = (bcast(bones, Bw)[:, :, 1] - bcast(bones, Bw)[:, :, 0])[:, :, None]
    r = p - a
    t = ((r * d).sum(-1) / (d * d).sum(-1).clamp_min(1e-6)).clamp(0.0, 1.0)
    s = t[..., None] * d - r
    dist = torch.sqrt((s * s).sum(-1) + 1e-6)
    mag = ((s.abs() * (t[..., None] * d.abs() + r.abs())).sum(-1) / dist + dist) / temperature
    return -dist / temperature, mag


def weights(v, bones, temperature, dtype=F64):
    """[K,Bw,V]"""
    return torch.softmax(logits(v, bones, temperature, dtype)[0], dim=1).permute(1, 0, 2)


def weights_mag(v, bones, temperature):
    """[K,Bw,V] float64: w_k (1 + (1 - w_k) mag(l_k) + sum_{j != k} w_j mag(l_j)) + TINY."""
    l, ml = logits(v, bones, temperature)
    w = torch.softmax(l, dim=1)
    tot = (w * ml).sum(1, keepdim=True)
    return (w * (1.0 + (1.0 - w) * ml + (tot - w * ml)) + TINY).permute(1, 0, 2)


def top_two_gap(v, bones, temperature):
    """[Bw,V]: difference of a vertex's two largest logits (0 with a single bone: nothing to tie with)."""
    l = logits(v, bones, temperature)[0]
    if l.shape[1] == 1:
        return torch.full_like(l[:, 0], float("inf"))
    top = l.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _cross(a, b, mag):
    ax, ay, az = a.unbind(-1)
    bx, by, bz = b.unbind(-1)
    sub = (lambda p, q: p + q) if mag else (lambda p, q: p - q)
    return torch.stack([sub(ay * bz, az * by), sub(az * bx, ax * bz), sub(ax * by, ay * bx)], -1)


def rest_frame(bones, dtype=F64, mag=False):
    """bones [Bb,K,2,3] -> R [Bb,K,3,3] (columns right, up, forward), joint [Bb,K,3]."""
    bones = bones.detach().to(dtype)
    f = F.normalize(bones[:, :, 1] - bones[:, :, 0], dim=-1, eps=1e-12)
    x = torch.tensor([1.0, 0.0, 0.0], dtype=dtype).expand_as(f)
    up = F.normalize(_cross(f, x, False), dim=-1, eps=1e-12)
    if mag:
        f, up = f.abs(), up.abs()
    right = _cross(up, f, mag)
    joint = bones[:, :, 0]
    return torch.stack([right, up, f], -1), (joint.abs() if mag else joint)


def euler_xyz(angles, mag=False):
    """[...,3] -> [...,3,3]: Rx Ry Rz.  ``mag``: |sin|, |cos| with derivatives |cos|, |sin| (every term positive)."""
    s, c = angles.sin(), angles.cos()
    if mag:
        da = angles - angles.detach()
        s, c = s.abs().detach() + c.abs().detach() * da, c.abs().detach() + s.abs().detach() * da
    neg = (lambda q: q) if mag else (lambda q: -q)
    (sx, sy, sz), (cx, cy, cz) = s.unbind(-1), c.unbind(-1)
    o, z = torch.ones_like(sx), torch.zeros_like(sx)
    m = lambda *e: torch.stack(e, -1).reshape(*sx.shape, 3, 3)
    return m(o, z, z, z, cx, neg(sx), z, sx, cx) @ m(cy, z, sy, z, o, z, neg(sy), z, cy) @ m(cz, neg(sz), z, sz, cz, z, z, z, o)


def links(bones, angles, dtype=F64, mag=False):
    """bones [1|N,K,2,3], angles [N,K,3] -> L [N,K,4,4]."""
    angles = angles.to(dtype)
    N, K = angles.shape[:2]
    R, a = rest_frame(bones, dtype, mag)
    Lr = bcast(R, N) @ euler_xyz(angles, mag) @ bcast(R, N).transpose(-1, -2)
    La = (Lr @ bcast(a, N)[..., None])[..., 0]
    Lt = bcast(a, N) + La if mag else bcast(a, N) - La
    last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dtype).expand(N, K, 1, 4)
    return torch.cat([torch.cat([Lr, Lt[..., None]], -1), last], -2)


def bone_transforms(bones, chain, angles, dtype=F64, mag=False):
    """-> [N,K,12] (row-major 3x4), link by link from the int table ``chain`` [K,D] (root first, -1 = no link at this position)."""
    L = links(bones, angles, dtype, mag)
    N, K = L.shape[:2]
    rows = []
    for k in range(K):
        M = torch.eye(4, dtype=dtype).expand(N, 4, 4)
        for i in chain[k].tolist():
            if i >= 0:
                M = M @ L[:, i]
        rows.append(M[:, :3].reshape(N, 12))
    return torch.stack(rows, 1)


def skin(v, bones, T, temperature, dtype=F64, w=None):
    """v [1|B,V,3], bones [1|B,K,2,3], T [B,K,12] -> [B,V,3]; the weights (``w`` [K,Bw,V] if given) see detached vertices."""
    T = T.to(dtype)
    B, K = T.shape[:2]
    if w is None:
        w = weights(v, bones, temperature, dtype)
    w = bcast(w.permute(1, 0, 2), B)
    T34 = T.reshape(B, K, 3, 4)
    p = bcast(v.to(dtype), B)
    posed = torch.einsum("bkij,bvj->bkvi", T34[..., :3], p) + T34[..., 3][:, :, None]
    return (w[..., None] * posed).sum(1)


def skin_pose(v, bones, angles, chain, temperature, dtype=F64):
    """-> (posed [B,V,3], T [B,K,12])"""
    T = bone_transforms(bones, chain, angles, dtype)
    return skin(v, bones, T, temperature, dtype), T


def evaluate(c, with_grads=True):
    """Float64 values and magnitudes of everything case ``c`` produces: dict key -> (value, magnitude) over KEYS (those that apply).
    The loss is sum(out * c['g_out']) + sum(T * c['g_T']) with whichever upstream gradients the case has."""
    op, bones, temp = c["op"], c["bones"], c["temperature"]
    res = {}
    if op == "weights":
        res["w"] = (weights(c["v"], bones, temp), weights_mag(c["v"], bones, temp))
        return res
    posed = op in ("pose", "bones", "skinning")
    ang = c["angles"].double().requires_grad_(True) if posed else None
    angm = c["angles"].double().requires_grad_(True) if posed else None
    if posed:
        T, Tm = bone_transforms(bones, c["chain"], ang), bone_transforms(bones, c["chain"], angm, mag=True)
    else:
        T, Tm = c["T"].double().requires_grad_(True), c["T"].double().abs().requires_grad_(True)
    res["T"] = (T.detach(), Tm.detach())
    loss, lossm, leaves, leavesm = 0.0, 0.0, [T], [Tm]
    if op != "bones":
        v, va = c["v"].double().requires_grad_(True), c["v"].double().abs().requires_grad_(True)
        out = skin(v, bones, T, temp)
        outm = skin(va, bones, Tm, temp, w=weights_mag(c["v"], bones, temp))
        res["out"] = (out.detach(), outm.detach())
        leaves, leavesm = [T, v], [Tm, va]
        if c.get("g_out") is not None:
            loss, lossm = (out * c["g_out"].double()).sum(), (outm * c["g_out"].double().abs()).sum()
    if c.get("g_T") is not None:
        loss, lossm = loss + (T * c["g_T"].double()).sum(), lossm + (Tm * c["g_T"].double().abs()).sum()
    if not with_grads:
        return res
    if posed:
        leaves, leavesm = leaves + [ang], leavesm + [angm]
    g = torch.autograd.grad(loss, leaves, allow_unused=True)
    gm = torch.autograd.grad(lossm, leavesm, allow_unused=True)
    zero = lambda x, like: torch.zeros_like(like) if x is None else x
    names = ["g_T"] + (["g_v"] if op != "bones" else []) + (["g_angles"] if posed else [])
    for n, a, b, leaf in zip(names, g, gm, leaves):
        res[n] = (zero(a, leaf), zero(b, leaf))
    return res


# the operation a case's operator computes: the fused ops.skin_pose and skinning()'s two launches compute the same posed mesh
OPERATION = {"skin": "blend", "weights": "weights", "bones": "chain", "pose": "posed", "skinning": "posed"}


def figure(name, key):
    """What the torch float32 path reaches on quantity ``key`` of case ``name`` (units of 2^-24 x magnitude)."""
    return MEASURED[name][key]


def allowed_units(name, key):
    """The kernels' bound on quantity ``key`` of case ``name`` in units of 2^-24 x magnitude: 4 x the measured figure."""
    return FACTOR * figure(name, key)


def bad_elements(got, ref, mag, name, key):
    """Indices where |got - ref| > 2^-24 (4 x figure(name, key) x magnitude + 4 |ref|); non-finite values violate."""
    return violations(got, ref, mag, figure(name, key), factor=FACTOR, floor_ulp=4.0)


# ---------------------------------------------------------------------------------------------------------------- skeletons
def _tree_of(parent):
    """[(bone, [every descendant])] in bone order (a parent has a smaller index than its children: ancestors are listed root first)."""
    K = len(parent)
    desc = [[] for _ in range(K)]
    for k in range(K):
        p = parent[k]
        while p >= 0:
            desc[p].append(k)
            p = parent[p]
    return [(k, desc[k]) for k in range(K)]


def chain_table(tree):
    """int32 [K,D]: row k = the chain root -> ... -> k, front-padded with -1 (what the kernels take)."""
    chains = {b: [p for p, ch in tree if b in ch] + [b] for b, _ in tree}
    K, D = len(tree), max(len(c) for c in chains.values())
    t = torch.full((K, D), -1, dtype=torch.int32)
    for k, c in chains.items():
        t[k, D - len(c):] = torch.tensor(c, dtype=torch.int32)
    return t


def quadruped_tree():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skinning_b1f1_t1.npz"), allow_pickle=False)
    return eval(str(g["chain"]))


def skeleton(family, K):
    """The kinematic tree of a family: quadruped20 (the golden tree), line8 (one chain, D = 8), roots (no parents, D = 1), star (one
    root, K - 1 children, D = 2), wide (bones 0..7 a line, the rest a random forest no deeper than 8: D = 8)."""
    if family == "quadruped20":
        assert K == 20
        return quadruped_tree()
    if family == "line8":
        assert K == 8
        return _tree_of([k - 1 for k in range(8)])
    if family == "roots":
        return _tree_of([-1] * K)
    if family == "star":
        return _tree_of([-1] + [0] * (K - 1))
    assert family == "wide" and K > 8
    rng = np.random.default_rng(1000 + K)
    parent, depth = [k - 1 for k in range(8)], list(range(1, 9))
    for k in range(8, K):
        while True:
            p = int(rng.integers(-1, k))
            if p < 0 or depth[p] < 8:
                break
        parent.append(p)
        depth.append(1 if p < 0 else depth[p] + 1)
    return _tree_of(parent)


# ---------------------------------------------------------------------------------------------------------------- case parts
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def make_bones(kind, Bb, K, rng):
    """[Bb,K,2,3] float32.  random | zero (one zero-length bone) | xaxis (one bone along +x, one along -x) | coincident (bone 1 = bone
    0) | tiny (one bone 1e-4 long: |d|^2 below the 1e-6 clamp)."""
    b = rng.uniform(-1.0, 1.0, (Bb, K, 2, 3)).astype(np.float32)
    m = K // 2
    if kind == "zero":
        b[:, m, 1] = b[:, m, 0]
    elif kind == "xaxis":
        b[:, 0, 1] = b[:, 0, 0] + np.float32([0.75, 0, 0])
        b[:, K - 1, 1] = b[:, K - 1, 0] - np.float32([0.5 if K > 1 else -0.75, 0, 0])
    elif kind == "coincident":
        b[:, min(1, K - 1)] = b[:, 0]
    elif kind == "tiny":
        d = b[:, m, 1] - b[:, m, 0]
        b[:, m, 1] = b[:, m, 0] + np.float32(1e-4) * d / np.linalg.norm(d, axis=-1, keepdims=True)
    else:
        assert kind == "random", kind
    return _f32(b)


VERTEX_KINDS = ("random", "joint", "interior", "past", "equidistant", "far")


def make_vertices(kind, Bv, V, bones, rng):
    """[Bv,V,3] float32 around the bones of image 0.  random in [-1,1]^3 | joint (exactly on a bone end) | interior (on a segment) | past
    (beyond either end: t clamps to exactly 0 and 1) | equidistant (midway between two bones' start joints) | far (|p| ~ 1e3) | mixed
    (vertex i takes kind i mod 6)."""
    bn = bones[0].numpy().astype(np.float64)
    K = bn.shape[0]
    a, d = bn[:, 0], bn[:, 1] - bn[:, 0]
    out = np.empty((Bv, V, 3), np.float64)
    for i in range(V):
        kd = VERTEX_KINDS[i % 6] if kind == "mixed" else kind
        k = (i // 6 if kind == "mixed" else i) % K
        if kd == "random":
            p = rng.uniform(-1, 1, (Bv, 3))
        elif kd == "joint":
            p = np.broadcast_to(bn[k, (i // K) % 2], (Bv, 3))
        elif kd == "interior":
            p = a[k] + rng.uniform(0.1, 0.9, (Bv, 1)) * d[k]
        elif kd == "past":
            p = (a[k] - 0.5 * d[k] if (i // K) % 2 else a[k] + 1.5 * d[k]) + rng.uniform(-0.05, 0.05, (Bv, 3))
        elif kd == "equidistant":
            p = np.broadcast_to(0.5 * (a[k] + a[(k + 1) % K]), (Bv, 3)) + (rng.uniform(-0.3, 0.3, (Bv, 3)) if K == 1 else 0.0)
        else:
            assert kd == "far", kd
            p = rng.uniform(-1e3, 1e3, (Bv, 3))
        out[:, i] = p
    return _f32(out)


def make_angles(kind, N, K, rng):
    """[N,K,3] float32.  zeros | uniform (+-0.6) | special (entries cycle through +-pi/2, +-pi, 10.0, 1e-8) | zero_row (uniform, one
    bone's row zero)."""
    if kind == "zeros":
        return torch.zeros(N, K, 3)
    a = rng.uniform(-0.6, 0.6, (N, K, 3))
    if kind == "special":
        vals = np.array([np.pi / 2, -np.pi / 2, np.pi, -np.pi, 10.0, 1e-8])
        a = vals[(np.arange(N * K * 3) * 5 + 1) % 6].reshape(N, K, 3) * np.where(rng.uniform(size=(N, K, 3)) < 0.25, 0.3, 1.0)
    elif kind == "zero_row":
        a[:, K // 2] = 0.0
    else:
        assert kind == "uniform", kind
    return _f32(a)


def make_upstream(kind, B, V, K, rng, op):
    """(g_out [B,V,3] or None, g_T [B,K,12] or None).  random / verts: on the vertices | onehot: one vertex, one component (op bones: one
    bone row per instance) | T: on the transforms only | both."""
    g_out = g_T = None
    if op == "bones":
        g_T = np.zeros((B, K, 12))
        if kind == "onehot":
            for n in range(B):
                g_T[n, (n * 7 + 3) % K] = rng.normal(size=12)
        else:
            g_T = rng.normal(size=(B, K, 12))
        return None, _f32(g_T)
    if kind in ("random", "verts", "both"):
        g_out = rng.normal(size=(B, V, 3))
    if kind == "onehot":
        g_out = np.zeros((B, V, 3))
        g_out[B - 1, (V * 2) // 3, 0] = 1.0
    if kind in ("T", "both"):
        g_T = rng.normal(size=(B, K, 12))
    return (None if g_out is None else _f32(g_out)), (None if g_T is None else _f32(g_T))


# ---------------------------------------------------------------------------------------------------------------- cases
# name -> dict(op, family, K, B, V, vb, bb, bones, verts, angles, up, temp[, grad]).  op: skin (ops.skin: the blend, T given) | weights
# (ops.skin_weights) | bones (ops.bone_transforms) | pose (ops.skin_pose) | skinning (model.geometry.skinning.skinning).  vb / bb: True =
# vertices / bones per image, False = shared.  B = 1 cases have nothing to share.  A case's seed is its rank among the sorted names.
def _c(op, family, K, B, V, vb, bb, bones, verts, angles, up, temp, **kw):
    return dict(op=op, family=family, K=K, B=B, V=V, vb=vb, bb=bb, bones=bones, verts=verts, angles=angles, up=up, temp=temp, **kw)


CASES = {
    # ---- ops.skin: every K of {1,3,19,20,21,32,33,64}, every V of {1,3,63,64,65,257}; each kernel size (<= 20, <= 32, <= 64) with a
    # ragged V; the four v_batch x bones_batch combinations at B = 3
    "skin_k1_v1": _c("skin", "roots", 1, 1, 1, True, True, "random", "random", None, "random", 1.0),
    "skin_k3_v3_shared_shared": _c("skin", "roots", 3, 3, 3, False, False, "zero", "mixed", None, "random", 0.05),
    "skin_k19_v63_batched_shared": _c("skin", "roots", 19, 3, 63, True, False, "xaxis", "mixed", None, "random", 0.05),
    "skin_k20_v65_shared_batched": _c("skin", "roots", 20, 3, 65, False, True, "coincident", "mixed", None, "random", 1e-3),
    "skin_k21_v257_batched_batched": _c("skin", "roots", 21, 3, 257, True, True, "tiny", "mixed", None, "random", 0.05),
    "skin_k32_v64": _c("skin", "roots", 32, 1, 64, True, True, "random", "mixed", None, "onehot", 1.0),
    "skin_k33_v65_shared_batched": _c("skin", "roots", 33, 3, 65, False, True, "coincident", "mixed", None, "random", 50.0),
    "skin_k64_v257_batched_shared": _c("skin", "roots", 64, 3, 257, True, False, "zero", "mixed", None, "random", 1e-3),
    "skin_k32_v63_shared_shared": _c("skin", "roots", 32, 3, 63, False, False, "xaxis", "mixed", None, "random", 0.05),
    "skin_k20_v257_T_only": _c("skin", "roots", 20, 3, 257, True, True, "random", "mixed", None, "random", 0.05, grad="T"),
    # ---- ops.skin_weights: temperatures {1e-3, 0.05, 1, 50}, Bw = 1 and Bw = B, coincident bones
    "w_t1e-3_shared": _c("weights", "roots", 20, 1, 257, False, False, "coincident", "mixed", None, None, 1e-3),
    "w_t0.05_bones_batched": _c("weights", "roots", 33, 3, 65, False, True, "coincident", "mixed", None, None, 0.05),
    "w_t1_verts_batched": _c("weights", "roots", 3, 3, 63, True, False, "coincident", "mixed", None, None, 1.0),
    "w_t50_shared": _c("weights", "roots", 64, 1, 65, False, False, "coincident", "mixed", None, None, 50.0),
    # ---- ops.bone_transforms: every family, N in {1, 33}, bones shared and per instance, every angle set, one-hot g_M rows
    "bn_quadruped_n33_batched": _c("bones", "quadruped20", 20, 33, 0, True, True, "random", None, "uniform", "onehot", 1.0),
    "bn_quadruped_n33_shared_special": _c("bones", "quadruped20", 20, 33, 0, True, False, "xaxis", None, "special", "onehot", 1.0),
    "bn_line8_n1_special": _c("bones", "line8", 8, 1, 0, True, True, "zero", None, "special", "onehot", 1.0),
    "bn_line8_n33_zero_row": _c("bones", "line8", 8, 33, 0, True, False, "random", None, "zero_row", "random", 1.0),
    "bn_roots1_n1_zeros": _c("bones", "roots", 1, 1, 0, True, True, "random", None, "zeros", "onehot", 1.0),
    "bn_roots3_n33_zero_row": _c("bones", "roots", 3, 33, 0, True, True, "xaxis", None, "zero_row", "onehot", 1.0),
    "bn_roots19_n1_uniform": _c("bones", "roots", 19, 1, 0, True, True, "tiny", None, "uniform", "onehot", 1.0),
    "bn_star2_n33_special": _c("bones", "star", 2, 33, 0, True, False, "coincident", None, "special", "onehot", 1.0),
    "bn_star20_n1_uniform": _c("bones", "star", 20, 1, 0, True, True, "zero", None, "uniform", "onehot", 1.0),
    "bn_wide21_n33_uniform": _c("bones", "wide", 21, 33, 0, True, True, "random", None, "uniform", "onehot", 1.0),
    "bn_wide32_n1_special": _c("bones", "wide", 32, 1, 0, True, True, "xaxis", None, "special", "onehot", 1.0),
    "bn_wide33_n33_zero_row": _c("bones", "wide", 33, 33, 0, True, False, "tiny", None, "zero_row", "onehot", 1.0),
    "bn_wide64_n33_uniform": _c("bones", "wide", 64, 33, 0, True, True, "coincident", None, "uniform", "onehot", 1.0),
    "bn_wide64_n1_zeros": _c("bones", "wide", 64, 1, 0, True, True, "random", None, "zeros", "random", 1.0),
    # ---- ops.skin_pose: K in {1,2,3,8,19} the guarded instances, K = 20 the unguarded one at D = 1, 2 and the tree's own depth
    "pose_roots1_v1": _c("pose", "roots", 1, 1, 1, True, True, "random", "random", "uniform", "verts", 1.0),
    "pose_star2_v3_zero_bone": _c("pose", "star", 2, 3, 3, False, False, "zero", "mixed", "special", "both", 0.05),
    "pose_roots3_v63_xaxis_T": _c("pose", "roots", 3, 3, 63, True, False, "xaxis", "mixed", "uniform", "T", 0.05),
    "pose_line8_v65_coincident": _c("pose", "line8", 8, 3, 65, False, True, "coincident", "mixed", "zero_row", "both", 1e-3),
    "pose_roots19_v257_tiny": _c("pose", "roots", 19, 3, 257, True, True, "tiny", "mixed", "special", "both", 0.05),
    "pose_roots20_v64_zeros": _c("pose", "roots", 20, 1, 64, True, True, "random", "mixed", "zeros", "verts", 50.0),
    "pose_star20_v65_onehot": _c("pose", "star", 20, 3, 65, True, False, "xaxis", "mixed", "uniform", "onehot", 0.05),
    "pose_quadruped_v257_shared_verts": _c("pose", "quadruped20", 20, 3, 257, False, True, "zero", "mixed", "uniform", "both", 0.05),
    "pose_quadruped_v63_angles_only": _c("pose", "quadruped20", 20, 3, 63, True, True, "coincident", "mixed", "special", "both", 1e-3,
                                          grad="angles"),
    "pose_quadruped_v3_T": _c("pose", "quadruped20", 20, 1, 3, True, True, "tiny", "far", "zero_row", "T", 1.0),
    # ---- model.geometry.skinning.skinning with K = 21: the two-launch path
    "skinning_wide21_v65": _c("skinning", "wide", 21, 3, 65, False, False, "random", "mixed", "uniform", "verts", 0.05),
    # ---- the loop branches of the four launchers (the launch geometry is recomputed in tests/test_skin_adversarial_gpu.py)
    "loop_skin_fwd_v8200_b2": _c("skin", "roots", 20, 2, 8200, True, True, "random", "random", None, "random", 0.05),
    "loop_pose_fwd_b16_v4100": _c("pose", "quadruped20", 20, 16, 4100, False, False, "random", "random", "uniform", "both", 0.05),
    "loop_pose_bwd_b16_v12289": _c("pose", "line8", 8, 16, 12289, False, True, "random", "random", "uniform", "both", 0.05),
    "loop_skin_bwd_b3_v349701_k3": _c("skin", "roots", 3, 3, 349701, True, False, "random", "random", None, "random", 0.05),
}
LARGE = ("loop_pose_bwd_b16_v12289", "loop_skin_bwd_b3_v349701_k3")  # the float64 side of these may run on the device


def build(name):
    """The tensors of a case (float32, CPU): v, bones, T or angles + chain + tree, g_out, g_T, temperature, and the spec's fields."""
    s = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 7000)
    K, B, V, op = s["K"], s["B"], s["V"], s["op"]
    c = dict(s, name=name, temperature=float(s["temp"]))
    c["bones"] = make_bones(s["bones"], B if s["bb"] else 1, K, rng)
    if op != "bones":
        c["v"] = make_vertices(s["verts"], B if s["vb"] else 1, V, c["bones"], rng)
    if op in ("pose", "bones", "skinning"):
        c["tree"] = skeleton(s["family"], K)
        c["chain"] = chain_table(c["tree"])
        c["angles"] = make_angles(s["angles"], B, K, rng)
    elif op == "skin":
        c["T"] = _f32(np.eye(3, 4).reshape(1, 1, 12) + 0.3 * rng.uniform(-1, 1, (B, K, 12)))
    if s["up"] is not None:
        c["g_out"], c["g_T"] = make_upstream(s["up"], B, V, K, rng, op)
    return c


def keys_of(c):
    """The quantities a case is compared on."""
    op = c["op"]
    if op == "weights":
        return ("w",)
    if op == "bones":
        return ("T", "g_angles")
    if op == "skin":
        return ("out", "g_T") if c.get("grad") == "T" else ("out", "g_v", "g_T")
    if op == "skinning":  # (the transforms stay inside skinning())
        return ("out", "g_v", "g_angles")
    return ("out", "T", "g_angles") if c.get("grad") == "angles" else ("out", "T", "g_v", "g_angles")


# what the torch float32 path reaches against the restatement, in units of 2^-24 x magnitude (maximum over the elements; CPU, one
# thread; third decimal rounded up): written by tests/test_skin_cpu.py::measure_all, asserted by test_measured_table_is_current
MEASURED = {
    "skin_k1_v1": {"out": 0.211, "g_v": 0.695, "g_T": 0.69},
    "skin_k3_v3_shared_shared": {"out": 1.32, "g_v": 0.934, "g_T": 1.478},
    "skin_k19_v63_batched_shared": {"out": 4.067, "g_v": 4.023, "g_T": 0.604},
    "skin_k20_v65_shared_batched": {"out": 1.893, "g_v": 1.455, "g_T": 2.015},
    "skin_k21_v257_batched_batched": {"out": 3.4, "g_v": 7.067, "g_T": 0.516},
    "skin_k32_v64": {"out": 0.53, "g_v": 0.698, "g_T": 0.97},
    "skin_k33_v65_shared_batched": {"out": 2.607, "g_v": 3.756, "g_T": 0.311},
    "skin_k64_v257_batched_shared": {"out": 2.162, "g_v": 2.217, "g_T": 2.874},
    "skin_k32_v63_shared_shared": {"out": 3.378, "g_v": 2.611, "g_T": 0.376},
    "skin_k20_v257_T_only": {"out": 3.848, "g_T": 0.488},
    "w_t1e-3_shared": {"w": 0.893},
    "w_t0.05_bones_batched": {"w": 5.646},
    "w_t1_verts_batched": {"w": 0.937},
    "w_t50_shared": {"w": 4.306},
    "bn_quadruped_n33_batched": {"T": 4.869, "g_angles": 0.972},
    "bn_quadruped_n33_shared_special": {"T": 3.59, "g_angles": 1.542},
    "bn_line8_n1_special": {"T": 0.633, "g_angles": 0.058},
    "bn_line8_n33_zero_row": {"T": 2.05, "g_angles": 0.008},
    "bn_roots1_n1_zeros": {"T": 2.001, "g_angles": 0.232},
    "bn_roots3_n33_zero_row": {"T": 4.0, "g_angles": 2.238},
    "bn_roots19_n1_uniform": {"T": 3.018, "g_angles": 0.778},
    "bn_star2_n33_special": {"T": 2.906, "g_angles": 1.425},
    "bn_star20_n1_uniform": {"T": 2.068, "g_angles": 0.203},
    "bn_wide21_n33_uniform": {"T": 4.421, "g_angles": 0.927},
    "bn_wide32_n1_special": {"T": 2.379, "g_angles": 0.409},
    "bn_wide33_n33_zero_row": {"T": 2.306, "g_angles": 0.434},
    "bn_wide64_n33_uniform": {"T": 4.821, "g_angles": 0.873},
    "bn_wide64_n1_zeros": {"T": 3.292, "g_angles": 0.505},
    "pose_roots1_v1": {"out": 0.163, "T": 2.469, "g_v": 1.05, "g_angles": 0.595},
    "pose_star2_v3_zero_bone": {"out": 1.271, "T": 3.477, "g_v": 0.956, "g_angles": 0.402},
    "pose_roots3_v63_xaxis_T": {"out": 2.116, "T": 2.434, "g_v": 0.0, "g_angles": 1.65},
    "pose_line8_v65_coincident": {"out": 0.349, "T": 1.95, "g_v": 0.093, "g_angles": 0.01},
    "pose_roots19_v257_tiny": {"out": 3.732, "T": 3.906, "g_v": 4.736, "g_angles": 0.145},
    "pose_roots20_v64_zeros": {"out": 0.755, "T": 4.001, "g_v": 3.165, "g_angles": 0.092},
    "pose_star20_v65_onehot": {"out": 3.718, "T": 3.223, "g_v": 3.309, "g_angles": 0.665},
    "pose_quadruped_v257_shared_verts": {"out": 0.519, "T": 2.602, "g_v": 0.027, "g_angles": 0.019},
    "pose_quadruped_v63_angles_only": {"out": 1.212, "T": 3.906, "g_angles": 0.132},
    "pose_quadruped_v3_T": {"out": 0.001, "T": 1.239, "g_v": 0.0, "g_angles": 0.087},
    "skinning_wide21_v65": {"out": 0.179, "g_v": 0.223, "g_angles": 0.018},
    "loop_skin_fwd_v8200_b2": {"out": 4.863, "g_v": 7.191, "g_T": 0.064},
    "loop_pose_fwd_b16_v4100": {"out": 1.393, "T": 2.813, "g_v": 0.579, "g_angles": 0.001},
    "loop_pose_bwd_b16_v12289": {"out": 1.631, "T": 3.72, "g_v": 0.003, "g_angles": 0.001},
    "loop_skin_bwd_b3_v349701_k3": {"out": 5.418, "g_v": 6.729, "g_T": 0.019},
}

# the three reference goldens (tests/golden/skinning_*.npz), largest absolute error over the three: the torch float32 path's grad_angles
# against float64, the goldens' own grad_angles against float64, and the torch chain's angle gradient (the loss of
# test_bone_transforms_kernel_vs_torch_chain) against float64.  tests/test_gpu_parity.py derives its absolute tolerances from these.
GOLDEN_ABS = {"grad_angles_fp32": 8.7e-6, "grad_angles_golden": 1.1e-5, "chain_grad_fp32": 3.3e-6}
