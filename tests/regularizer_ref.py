"""The mesh regularisers restated for the tests: the edge rule with explicit loops, the losses in the dtype of their input (float64 in
the tests) through torch's autograd.

A triangle list tri[F,3] has 3F directed occurrences: s = 3f + c runs (i, j) = (tri[f][c], tri[f][(c+1)%3]); key (min, max); forward if
i <= j (a self edge is forward), backward otherwise.  Unique edges are the distinct keys, in ascending (lexicographic) order --
torch.unique's.  col0 / col1 of an edge: the face of its highest forward / backward slot, 0 where there is none.
"""
import torch

EPS = 1e-20


def edge_tables(tri):
    """tri: int [F,3] -> (edges int64 [E,2], tris_per_edge int64 [E,2])."""
    best = {}  # key -> [highest forward slot, highest backward slot]
    for f, row in enumerate(tri.tolist()):
        for c in range(3):
            i, j = row[c], row[(c + 1) % 3]
            slots = best.setdefault((min(i, j), max(i, j)), [-1, -1])
            d = 0 if i <= j else 1
            slots[d] = max(slots[d], 3 * f + c)
    keys = sorted(best)
    edges = torch.tensor(keys, dtype=torch.int64).reshape(-1, 2)
    cols = torch.tensor([[s // 3 if s >= 0 else 0 for s in best[k]] for k in keys], dtype=torch.int64).reshape(-1, 2)
    return edges, cols


def length(x):
    return torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=EPS))


def safe_normalize(x):
    return x / length(x)


def laplace_term(v_pos, tri):
    """[B,V,3]: sum over the corner entries (c,f) of v of ((v_{c+1} - v) + (v_{c+2} - v)) / max(2 n_v, 1)."""
    B, V = v_pos.shape[:2]
    term = torch.zeros_like(v_pos)
    n = torch.zeros(V, dtype=v_pos.dtype)
    for c in range(3):
        a, b, d = tri[:, c], tri[:, (c + 1) % 3], tri[:, (c + 2) % 3]
        term = term.index_add(1, a, (v_pos[:, b] - v_pos[:, a]) + (v_pos[:, d] - v_pos[:, a]))
        n = n.index_add(0, a, torch.ones(tri.shape[0], dtype=v_pos.dtype))
    return term / torch.clamp(2 * n, min=1.0)[None, :, None]


def laplace_regularizer_const(v_pos, tri):
    return torch.mean(laplace_term(v_pos, tri) ** 2)


def laplace_term_loops(v_pos, tri):
    """the same with one loop per corner entry (small meshes: the known-answer tests)"""
    B, V = v_pos.shape[:2]
    rows = [[torch.zeros(B, 3, dtype=v_pos.dtype), 0] for _ in range(V)]
    for row in tri.tolist():
        for c in range(3):
            v, a, b = row[c], row[(c + 1) % 3], row[(c + 2) % 3]
            rows[v][0] = rows[v][0] + (v_pos[:, a] - v_pos[:, v]) + (v_pos[:, b] - v_pos[:, v])
            rows[v][1] += 1
    return torch.stack([t / max(2 * n, 1) for t, n in rows], 1)


def face_normals(v_pos, tri):
    v0, v1, v2 = v_pos[:, tri[:, 0]], v_pos[:, tri[:, 1]], v_pos[:, tri[:, 2]]
    return safe_normalize(torch.cross(v1 - v0, v2 - v0, dim=-1))


def normal_consistency(v_pos, tri, tables=None):
    _, cols = tables if tables is not None else edge_tables(tri)
    n = face_normals(v_pos, tri)
    d = (n[:, cols[:, 0]] * n[:, cols[:, 1]]).sum(-1, keepdim=True)
    t = (1.0 - torch.clamp(d, min=-1.0, max=1.0)) * 0.5
    return torch.mean(torch.abs(t))


def get_edge_length(v_pos, tri, tables=None):
    edges, _ = tables if tables is not None else edge_tables(tri)
    return length(v_pos[:, edges[:, 0]] - v_pos[:, edges[:, 1]])


def avg_edge_length(v_pos, tri, tables=None):
    return torch.mean(get_edge_length(v_pos, tri, tables))


LOSSES = {"laplace": lambda v, tri, tables=None: laplace_regularizer_const(v, tri), "normal_consistency": normal_consistency,
          "avg_edge_length": avg_edge_length}
