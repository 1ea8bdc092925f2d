"""Geometry helpers mirroring /root/reference/model/geometry/util.py (public API kept; torch, any device).

``line_segment_distance`` is what the skinning kernel fuses (csrc/skin.hip); the torch form stays for callers
that import it directly.
"""
import torch


def line_segment_distance(a, b, points, sqrt=True):
    """Distance from ``points`` [..., N, D] to the segments a-b [..., D] (reference geometry/util.py:30-53)."""
    a, b = a[..., None, :], b[..., None, :]
    ab = b - a
    denom = torch.clamp((ab * ab).sum(-1, keepdim=True), min=1e-6)
    t = (((points - a) * ab).sum(-1, keepdim=True) / denom).clamp(0.0, 1.0)
    closest = a + t * ab
    dist = ((closest - points) ** 2).sum(-1)
    return torch.sqrt(dist + 1e-6) if sqrt else dist


def sample_farthest_points(pts, k, return_index=False, start=None):
    """Greedy farthest-point sampling, pts [B,3,N] -> [B,3,k] (reference geometry/util.py:5-27).

    float32 input on the GPU within the sampler's limits goes to the HIP kernel (csrc/fps.hip, ops.farthest_point_sample: one launch for
    the whole batch; skinning.DEVICE_FPS / A3D_DEVICE_FPS switches it off); everything else runs the reference's loop, one argmax,
    gather, norm and minimum per pick.  Both draw the first picks with the same torch.randint (the generator is consumed identically)
    and both return ``pts.gather`` of the indices, so gradients reach ``pts`` the same way.  ``start`` [B]: first picks already drawn
    by the caller (then nothing is drawn here)."""
    b, c, n = pts.shape
    idx = torch.randint(n, [b], device=pts.device) if start is None else start
    from . import skinning  # (the switch lives with estimate_bones' other switches; skinning imports this module)
    from ... import ops

    if skinning.DEVICE_FPS and c == 3 and ops.fps_device_ok(pts.transpose(1, 2), k):
        indexes = ops.farthest_point_sample(pts.transpose(1, 2), k, idx)
        out = pts.gather(2, indexes[:, None, :].expand(b, c, k))
        return (out, indexes) if return_index else out
    chosen = [idx]
    picked = pts.gather(2, idx[:, None, None].expand(b, c, 1))
    dist = (picked - pts).norm(dim=1)
    for _ in range(1, k):
        idx = dist.argmax(dim=1)
        chosen.append(idx)
        picked = pts.gather(2, idx[:, None, None].expand(b, c, 1))
        dist = torch.minimum(dist, (picked - pts).norm(dim=1))
    indexes = torch.stack(chosen, 1)
    out = pts.gather(2, indexes[:, None, :].expand(b, c, k))
    return (out, indexes) if return_index else out
