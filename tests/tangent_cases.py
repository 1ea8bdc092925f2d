"""Input builders shared by tests/golden/make_golden_tangent.py, tests/test_tangent_cpu.py, tests/test_shading_normal_gpu.py and
tests/test_tangents_gpu.py.  The parity rule is bsdf_cases.parity.

Shading normal, inputs in the public order (pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm):
'cond'  conditioned BY CONSTRUCTION away from every kink: unit normals and tangents, perturbation z >= 0.05, the view direction placed
        relative to the PERTURBED normal with dot(view, n) / 0.1 either in [2, 9.5] (clamped, margin 1) or in [0.2, 0.8] (every fourth
        pixel, inside the ramp), the geometric normal within the hemisphere of both (dot(g, view) >= 0.3).
'wild'  the reference's own test pattern, torch.rand everything (renderutils/tests/test_bsdf.py).
'bcast' a planar patch [2,16,16] seen at grazing angles (the ramp of the bend is live, so view_pos receives a gradient) from view_pos
        [2,1,1,3], with one constant perturbation [1,1,1,3]: both reduce shapes.

Meshes for the tangents: (v_pos [B,V,3], v_tex [1|B,Nuv,2], v_nrm [B,V,3], faces [F,3], uv_idx [F,3]).
"""
import math
import os

import numpy as np
import torch

GOLDEN_PIXELS = 512
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]  # (two_sided_shading, opengl)
SN_GOLDEN_CASES = [(kind, ts, gl, 100 + 10 * k + v) for k, kind in enumerate(("cond", "wild", "bcast")) for v, (ts, gl) in enumerate(VARIANTS)]
KINK_EPS = 1e-5
KINK_CAP = 0.01
NORMAL_THRESHOLD = 0.1
HERE = os.path.dirname(os.path.abspath(__file__))

_nz = torch.nn.functional.normalize


def _unit(g, n):
    return _nz(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)


def _perp(a, g):
    """a unit vector perpendicular to each row of a, random azimuth"""
    r = torch.randn(a.shape, generator=g, dtype=torch.float64)
    return _nz(r - (r * a).sum(-1, keepdim=True) * a, dim=-1)


def perturbed_normal(p, n, t, opengl):
    """the perturbed shading normal in the inputs' dtype (used to place the view in 'cond')"""
    n, t = _nz(n, dim=-1), _nz(t, dim=-1)
    bt = _nz(torch.cross(t, n, dim=-1), dim=-1)
    sign = -1.0 if opengl else 1.0
    return _nz(t * p[..., 0:1] + sign * bt * p[..., 1:2] + n * p[..., 2:3].clamp(min=0.0), dim=-1)


def make_sn_inputs(kind, n, seed, opengl=True):
    """float32 CPU inputs of one shading-normal case ('cond' places the view relative to the normal perturbed under ``opengl``)."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    if kind == "wild":
        return [rand(n, 3) for _ in range(6)]
    if kind == "bcast":
        B, H, W = 2, 16, 16
        assert n == B * H * W
        ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, H), torch.linspace(-0.5, 0.5, W), indexing="ij")
        pos = torch.stack([xs, ys, torch.zeros_like(xs)], -1)[None].repeat(B, 1, 1, 1) + 0.004 * (rand(B, H, W, 3) - 0.5)
        nrm = _nz(torch.tensor([0.0, 0.0, 1.0]) + 0.02 * (rand(B, H, W, 3) - 0.5), dim=-1)
        tng = _nz(torch.tensor([1.0, 0.0, 0.0]) + 0.1 * (rand(B, H, W, 3) - 0.5), dim=-1)
        geo = _nz(torch.tensor([0.0, 0.0, 1.0]) + 0.02 * (rand(B, H, W, 3) - 0.5), dim=-1)
        view = torch.tensor([[3.0, 0.5, 0.21], [2.8, -0.4, 0.25]]).view(B, 1, 1, 3)
        per = torch.tensor([-0.02, 0.0, 0.9]).view(1, 1, 1, 3)
        return [pos, view, per, nrm, tng, geo]
    assert kind == "cond"
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    nrm = _unit(g, n)
    tng = _nz(_perp(nrm, g) + 0.3 * u(-1, 1) * nrm, dim=-1)  # unit, up to ~17 degrees off the tangent plane
    per = torch.cat([u(-0.3, 0.3), u(-0.1, 0.1), u(0.05, 1.0)], -1)
    n1 = perturbed_normal(per, nrm, tng, opengl)
    ramp = (torch.arange(n) % 4 == 0)[:, None]
    c = torch.where(ramp, u(0.02, 0.08), u(0.2, 0.95))
    view = n1 * c + _perp(n1, g) * torch.sqrt(1 - c * c)
    geo = _nz(n1 + 0.5 * view + 0.1 * _unit(g, n), dim=-1)
    pos = torch.randn(n, 3, generator=g, dtype=torch.float64)
    view_pos = pos + view * u(1.0, 4.0)
    return [t.float() for t in (pos, view_pos, per, nrm, tng, geo)]


def sn_near_kink(inputs, two_sided, opengl):
    """[leading shape] bool: pixels within KINK_EPS of a kink (dot(g, view) at 0 when two sided, dot(view, n) / 0.1 at 0 or 1, the
    perturbation's z at 0), evaluated in float64 from the inputs."""
    pos, view_pos, per, nrm, tng, geo = [t.double() for t in inputs]
    view = _nz(view_pos - pos, dim=-1)
    n = perturbed_normal(per, nrm, tng, opengl)
    gv = (geo * view).sum(-1)
    if two_sided:
        n = torch.where((gv > 0)[..., None], n, -n)
    d = (view * n).sum(-1) / NORMAL_THRESHOLD
    bad = (d.abs() <= KINK_EPS) | ((d - 1).abs() <= KINK_EPS) | (per[..., 2].abs() <= KINK_EPS).expand_as(d)
    if two_sided:
        bad = bad | (gv.abs() <= KINK_EPS)
    return bad


def sn_out_shape(inputs):
    return (*torch.broadcast_shapes(*[t.shape[:-1] for t in inputs]), 3)


# ---------------------------------------------------------------------------------------------- meshes
TETRA_FACES = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
FAN_RIM = 70
MESH_NAMES = ("mesh_b1", "mesh_b4", "mesh_isolated", "tetra", "fan", "degenerate")


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name), allow_pickle=False)


def dmtet_atlas(n_tets):
    """The DMTet uv atlas (reference dmtet.py:69-84: one quad per cell of an N x N grid, N = ceil(sqrt((2 n_tets + 1) // 2)), side
    0.9 / N), float32 [4 N N, 2] -- restated so that the cases need neither a GPU nor the oracle package."""
    N = int(math.ceil(math.sqrt((2 * n_tets + 1) // 2)))
    tex_y, tex_x = torch.meshgrid(torch.linspace(0, 1 - (1 / N), N, dtype=torch.float32), torch.linspace(0, 1 - (1 / N), N, dtype=torch.float32),
                                  indexing="ij")
    pad = 0.9 / N
    uvs = torch.stack([tex_x, tex_y, tex_x + pad, tex_y, tex_x + pad, tex_y + pad, tex_x, tex_y + pad], dim=-1).view(-1, 2)
    return uvs


def make_mesh_case(name):
    """-> dict(v_pos, v_tex, v_nrm, faces, uv_idx), float32 / int64 CPU tensors."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name in ("mesh_b1", "mesh_b4", "mesh_isolated"):
        m = _golden(name + ".npz")
        src = _golden("mesh_b1.npz")
        v_pos, v_nrm = torch.from_numpy(m["v_pos"]), torch.from_numpy(m["v_nrm"])
        return dict(v_pos=v_pos, v_tex=dmtet_atlas(6 * 8 ** 3)[None], v_nrm=v_nrm, faces=torch.from_numpy(m["faces"]),
                    uv_idx=torch.from_numpy(src["uv_idx"]))
    if name == "tetra":
        B = 2
        base = torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
        v_pos = base[None] + 0.2 * (torch.rand(B, 4, 3, generator=g) - 0.5)
        v_nrm = _nz(v_pos + 0.1 * torch.randn(B, 4, 3, generator=g), dim=-1)
        v_tex = torch.rand(B, 12, 2, generator=g)  # every face its own three uvs, another atlas per image
        return dict(v_pos=v_pos, v_tex=v_tex, v_nrm=v_nrm, faces=torch.tensor(TETRA_FACES), uv_idx=torch.arange(12).view(4, 3))
    if name == "fan":
        B, R = 3, FAN_RIM
        ang = torch.arange(R) * (2 * math.pi / R)
        rim = torch.stack([torch.cos(ang), torch.sin(ang), 0.1 * torch.sin(3 * ang)], -1)
        base = torch.cat([torch.tensor([[0.0, 0.0, 0.3]]), rim], 0)
        v_pos = base[None] + 0.02 * (torch.rand(B, R + 1, 3, generator=g) - 0.5)
        v_nrm = _nz(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(B, R + 1, 3, generator=g), dim=-1)
        i = torch.arange(R)
        faces = torch.stack([torch.zeros(R, dtype=torch.int64), 1 + i, 1 + (i + 1) % R], -1)
        v_tex = (0.5 + 0.4 * base[:, :2] + 0.01 * (torch.rand(R + 1, 2, generator=g) - 0.5))[None]  # a planar chart, shared
        return dict(v_pos=v_pos, v_tex=v_tex, v_nrm=v_nrm, faces=faces, uv_idx=faces.clone())
    assert name == "degenerate"
    B, n = 2, 4
    ys, xs = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(n, dtype=torch.float32), indexing="ij")
    base = torch.stack([xs, ys, 0.2 * torch.sin(xs + ys)], -1).view(-1, 3)
    v_pos = base[None] + 0.1 * (torch.rand(B, n * n, 3, generator=g) - 0.5)
    v_nrm = _nz(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(B, n * n, 3, generator=g), dim=-1)
    faces = []
    for y in range(n - 1):
        for x in range(n - 1):
            a = y * n + x
            faces += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    faces = torch.tensor(faces)
    F = faces.shape[0]
    chart = base[:, :2] / n + 0.01 * (torch.rand(n * n, 2, generator=g) - 0.5)
    v_tex = chart[faces.reshape(-1)].clone()  # every corner its own uv
    uv_idx = torch.arange(3 * F).view(F, 3)
    v_tex[3 * 2: 3 * 2 + 3] = torch.tensor([[0.0, 0.0], [0.1, 0.1], [0.2, 0.2]])  # collinear: denom == 0 exactly -> the -1e-6 branch
    v_tex[3 * 9: 3 * 9 + 3] = torch.tensor([[0.3, 0.3], [0.3, 0.3], [0.3, 0.3]])  # one point: denom == 0, nom == 0
    v_tex[3 * 5: 3 * 5 + 3] = v_tex[3 * 5: 3 * 5 + 3].flip(0)  # mirrored: denom < 0
    return dict(v_pos=v_pos, v_tex=v_tex[None], v_nrm=v_nrm, faces=faces, uv_idx=uv_idx)


def mesh_weights(case, seed=0):
    """the upstream gradient of v_tng for a mesh case"""
    return torch.randn(case["v_pos"].shape, generator=torch.Generator().manual_seed(4000 + seed))


def isolated_vertices(case):
    """[V] bool: vertices no face refers to (their tangent is 0 / 0)"""
    used = torch.zeros(case["v_pos"].shape[1], dtype=torch.bool)
    used[case["faces"].reshape(-1)] = True
    return ~used
