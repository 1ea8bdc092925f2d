"""The per-point shading (csrc/shade.hip, shade_common.h: sh_forward) restated in plain torch, its input makers, hand-placed kink points
and the bound of the per-image reduction, shared by tests/test_shade_cpu.py and tests/test_shade_adversarial_gpu.py.

``shade`` follows the reference line by line: shading normal = prepare_shading_normal with the (0, 0, 1) perturbation (reference
model/render/render.py:71-72 -> renderutils/ops.py:194-227 -> renderutils/bsdf.py:28-51: normalize, the two-sided flip of bsdf.py:19-26,
the bend toward the geometric normal with NORMAL_THRESHOLD = 0.1 of bsdf.py:13), camera-space normal = safe_normalize(w2c rotation x
normal) (render.py:73-74, render/util.py:28-32) and the directional light ambient + diffuse * clamp(L . n_cam, min=0) (light.py:186-190),
shaded = shading * kd (render.py:93).  Run in float64 it is the reference (gradients by autograd); run in float32 it is the twin of the
parity rule (bsdf_cases.parity).
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
NORMAL_THRESHOLD = 0.1
KINK_EPS = 1e-5
WG = 256  # sh_bwd_kernel's work-group: 256 consecutive points


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def shade(gb, rot, view, light, kd, two_sided=True):
    """gb [P,12] (position | face normal | smooth normal | canonical position), rot [P,3,3], view [P,3], light [P,5] | None (direction 3,
    ambient, diffuse), kd [P,3] -> (nrm [P,3], shading [P,1] | None, shaded [P,3] | None), in the dtype of the inputs."""
    pos, g, a = gb[:, 0:3], gb[:, 3:6], gb[:, 6:9]
    n = F.normalize(F.normalize(a, dim=-1), dim=-1)  # ops.py:214 and bsdf.py:44 (the perturbed normal is the smooth normal, re-normalised)
    v = F.normalize(view - pos, dim=-1)
    if two_sided:  # bsdf.py:19-26
        front = _dot(g, v) > 0
        n = torch.where(front, n, -n)
        g = torch.where(front, g, -g)
    t = torch.clamp(_dot(v, n) / NORMAL_THRESHOLD, 0, 1)  # bsdf.py:28-33
    nrm = torch.lerp(g, n, t)
    if light is None:
        return nrm, None, None
    q = (rot * nrm[:, None, :]).sum(-1)
    cam = q / torch.sqrt(torch.clamp(_dot(q, q), min=1e-20))  # util.py:28-32
    shading = light[:, 3:4] + light[:, 4:5] * torch.clamp(_dot(light[:, 0:3], cam), min=0)  # light.py:186-190
    return nrm, shading, shading * kd


def run(inputs, weights, two_sided, dtype, lit=True):
    """Values and all input gradients of ``shade`` in ``dtype`` on the CPU: inputs = (gb, rot [P,3,3], view, light, kd), weights =
    (w_nrm [P,3] | None, w_shading [P,1] | None, w_shaded [P,3]) the upstream gradients.  -> ([nrm, shading, shaded],
    [g_gb, g_rot, g_view, g_light, g_kd])."""
    xs = [x.detach().to(dtype).clone().requires_grad_(True) for x in inputs]
    gb, rot, view, light, kd = xs
    outs = shade(gb, rot, view, light if lit else None, kd, two_sided)
    loss = 0.0
    for o, w in zip(outs, weights):
        if o is not None and w is not None:
            loss = loss + (o * w.to(dtype)).sum()
    used = xs if lit else xs[:3]
    grads = torch.autograd.grad(loss, used, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, used)]
    return [o.detach() if o is not None else None for o in outs], [g.detach() for g in grads]


def make_points(P, seed):
    """Generated inputs, float32: positions and smooth normals uniform in [-1, 1]^3 (smooth normals NOT unit), unit face normals, a
    rotation-like 3x3 of uniform entries, view positions in [-3, 3]^3, unit light directions, ambient and diffuse in [0, 1], kd in
    [0, 1].  Nothing is placed on a kink: the share near_kink finds is ~1e-4 (checked by test_shade_cpu.py to stay under 1 %)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    gb = torch.cat((r(P, 3), F.normalize(r(P, 3), dim=-1), r(P, 3), r(P, 3)), -1)
    rot, view = r(P, 3, 3), r(P, 3) * 3
    light = torch.cat((F.normalize(r(P, 3), dim=-1), torch.rand(P, 2, generator=g)), -1)
    kd = torch.rand(P, 3, generator=g)
    return gb, rot, view, light, kd


def make_weights(P, seed):
    g = torch.Generator().manual_seed(seed + 77)
    return torch.randn(P, 3, generator=g), torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g)


def near_kink(inputs, two_sided=True):
    """[P] bool, float64: points within KINK_EPS of a kink -- dot(geo, v) = 0 (two-sided only), t_raw = 0 or 1, l = 0, |a| or |view - pos|
    at the 1e-12 floor of normalize, qq at the 1e-20 floor of safe_normalize.  (t = 0.5 is no kink: value and gradient are continuous.)"""
    gb, rot, view, light, kd = [x.double() for x in inputs]
    pos, g, a = gb[:, 0:3], gb[:, 3:6], gb[:, 6:9]
    v = F.normalize(view - pos, dim=-1)
    n = F.normalize(F.normalize(a, dim=-1), dim=-1)
    gv = _dot(g, v)
    bad = (gv.abs() <= KINK_EPS) if two_sided else torch.zeros_like(gv, dtype=torch.bool)
    sigma = torch.where(gv > 0, 1.0, -1.0) if two_sided else torch.ones_like(gv)
    t_raw = _dot(v, n * sigma) / NORMAL_THRESHOLD
    bad = bad | (t_raw.abs() <= KINK_EPS) | ((t_raw - 1).abs() <= KINK_EPS)
    bad = bad | (a.norm(dim=-1, keepdim=True) <= 1e-11) | ((view - pos).norm(dim=-1, keepdim=True) <= 1e-11)
    nrm, _, _ = shade(gb, rot, view, light, kd, two_sided)
    q = (rot * nrm[:, None, :]).sum(-1)
    qq = _dot(q, q)
    cam = q / torch.sqrt(torch.clamp(qq, min=1e-20))
    bad = bad | (qq <= 1e-19) | (_dot(light[:, 0:3], cam).abs() <= KINK_EPS)
    return bad.reshape(-1)


# ------------------------------------------------------------------------------------------------ hand-placed kinks
def kink_points():
    """Points a few ulps (and 1e-3) to either side of every kink, and on it, built so that the side taken does not depend on rounding
    (axis-aligned: pos = 0, view = (0, 0, 2) so v = (0, 0, 1) exactly, rot = identity unless the kink is the rotation's).
    -> (inputs as make_points, group [n] int: the kink each point belongs to, names)."""
    u = 2.0 ** -23
    side = [-1e-3, -64 * u, -4 * u, 4 * u, 64 * u, 1e-3]
    rows, group, names = [], [], []
    base = dict(pos=(0.0, 0.0, 0.0), geo=(0.0, 0.6, 0.8), a=(0.3, 0.2, 0.9), view=(0.0, 0.0, 2.0), rot=1.0, L=(0.3, 0.4, 0.5))

    def add(name, **kw):
        if name not in names:
            names.append(name)
        rows.append(dict(base, **kw))
        group.append(names.index(name))

    for d in side + [0.0]:
        add("dot(geo, v) = 0", geo=(0.8, 0.6, d))
        add("t_raw = 0", a=(1.0, 0.5, d), geo=(0.0, 0.0, 1.0))
        add("l = 0", a=(0.0, 0.6, 0.8), L=(1.0, 0.0, d))
    c1, c5 = (1 - 0.01) ** 0.5, (1 - 0.0025) ** 0.5
    for d in side:
        add("t_raw = 1", a=(c1, 0.0, 0.1 * (1 + d)), geo=(0.0, 0.0, 1.0))
        add("t = 0.5", a=(c5, 0.0, 0.05 * (1 + d)), geo=(0.0, 0.0, 1.0))
    for a in [(0.0, 0.0, 0.0), (5e-13, 0.0, 0.0), (0.0, 0.0, 2e-12), (1e-12 * (1 - 1e-3), 0.0, 0.0), (1e-12 * (1 + 1e-3), 0.0, 0.0)]:
        add("|a| at 1e-12", a=a)
    for s in [0.0, 5e-11, 2e-10, 1e-10 * (1 - 1e-3), 1e-10 * (1 + 1e-3)]:
        add("qq at 1e-20", rot=s)
    p = (0.3, -0.2, 0.5)
    add("view == pos", pos=p, view=p)
    for dz in [1e-13, -5e-13, 1e-12 * (1 - 1e-3), 1e-12 * (1 + 1e-3), 1e-11]:  # |view - pos| below, at and above normalize's 1e-12 floor
        add("view == pos", view=(0.0, 0.0, dz))
    n = len(rows)
    t = lambda k: torch.tensor([r[k] for r in rows], dtype=torch.float64)
    gb = torch.cat((t("pos"), t("geo"), t("a"), torch.zeros(n, 3, dtype=torch.float64)), -1).float()
    rot = (torch.eye(3, dtype=torch.float64)[None] * t("rot")[:, None, None]).float()
    light = torch.cat((t("L"), torch.full((n, 1), 0.2, dtype=torch.float64), torch.full((n, 1), 0.7, dtype=torch.float64)), -1).float()
    kd = torch.tensor([0.4, 0.5, 0.6]).expand(n, 3).contiguous()
    return (gb, rot, t("view").float(), light, kd), torch.tensor(group), names


def kink_violations(hip, twin32, x64, group):
    """The per-element rule of test_bsdf_gpu.test_kinks_hand_placed_on_either_side_of_every_clamp, applied per kink group: |hip - x64|
    <= 16 |twin32 - x64| + 4 * 2^-24 |x64| + 1e-6 max|x64| (the maximum over the group), and a row the twin zeroes exactly (float32 and
    float64) is exactly zero.  A wrong subgradient is off by the whole derivative.  -> list of (row, column, hip, twin32, x64)."""
    n = hip.shape[0]
    hip, twin32, x64 = hip.reshape(n, -1).double(), twin32.reshape(n, -1).double(), x64.reshape(n, -1).double()
    bad = []
    for k in group.unique().tolist():
        sel = (group == k).nonzero().reshape(-1)
        a, b, c = hip[sel], twin32[sel], x64[sel]
        lim = 16 * (b - c).abs() + 4 * EPS * c.abs() + 1e-6 * c.abs().max()
        dead = ((b == 0) & (c == 0)).all(-1, keepdim=True)
        wrong = ((a - c).abs() > lim) | (dead & (a != 0)) | ~torch.isfinite(a)
        for i, j in wrong.nonzero().tolist():
            bad.append((int(sel[i]), j, float(a[i, j]), float(b[i, j]), float(c[i, j])))
    return bad


# ------------------------------------------------------------------------------------------------ per-image lists and the reduction
def image_list(P, B=10):
    """img [P] int64, non-decreasing (the kernel's precondition: the covered-pixel list is image-major; unsorted lists are not a case).
    B = 10: images of 16, 48, 192, 0, 100, 1, 99, 0, 301 points and the rest -- image boundaries at list positions 15/16, 63/64 and
    255/256, a first work-group that holds three images, two images without points, and image 5 with exactly one point (list position
    356) in the middle of the second work-group.  Shorter lists are its prefix.  B = 1: one image."""
    if B == 1:
        return torch.zeros(P, dtype=torch.int64)
    assert B == 10
    sizes = [16, 48, 192, 0, 100, 1, 99, 0, 301]
    img = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)] + [torch.full((max(P, 1),), 9, dtype=torch.int64)])
    return img[:P].contiguous()


def pix_of(img, pixels_per_image, seed=0):
    """A covered-pixel list whose entry p lies in image img[p]: img * pixels_per_image + an offset inside the image."""
    g = torch.Generator().manual_seed(seed)
    return img * pixels_per_image + torch.randint(0, pixels_per_image, img.shape, generator=g)


def reduction_reference(per_point, img, B, shared=False):
    """The per-image sums of the kernel's OWN per-point row gradients, in float64, and their bound: (sum [B|1,C], bound [B|1,C]).

    sh_bwd_kernel adds a point's term in a chain of at most 4 (the 16-lane DPP sum, a tree) + 15 (the 16 row sums, added in sequence
    from LDS) + n_atomics additions, n_atomics = the (work-group, image) pairs that reach the destination row -- every image of every
    work-group when the row is shared.  A term that passes through d additions picks up at most d * 2^-24 of the partial sums, each at
    most sum |term|: bound = (19 + n_atomics) * 2^-24 * sum |term|.  The terms themselves are the per-point form's fp32 values (held to
    float64 by the parity rule); a point lost, doubled or sent to another image moves the sum by a whole term."""
    x = per_point.double()
    C = x.shape[1]
    idx = torch.zeros_like(img) if shared else img
    rows = 1 if shared else B
    s = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, idx, x)
    mag = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, idx, x.abs())
    pairs = torch.unique(torch.stack([torch.arange(img.numel()) // WG, img], -1), dim=0) if img.numel() else torch.zeros(0, 2, dtype=torch.int64)
    n_atomics = torch.zeros(rows, dtype=torch.float64).index_add_(0, torch.zeros_like(pairs[:, 1]) if shared else pairs[:, 1],
                                                                   torch.ones(pairs.shape[0], dtype=torch.float64))
    return s, (19 + n_atomics)[:, None] * EPS * mag
