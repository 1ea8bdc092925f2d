"""The 'depth' render mode as the reference states it (model/render/render.py:101-108 of the reference, then :258-268 and :311-315), in
whatever dtype the inputs have -- float64 in the tests:

    hom   = [pos, 1]                                  for EVERY pixel of the frame; an uncovered pixel has pos = 0
    z     = (hom @ w2c^T)[..., 2]                     camera-space depth, = w2c[b,2,3] where nothing was rasterised
    d     = (z - amin z) / (amax z - amin z)          extremes per image over all H W pixels
    image = antialias(lerp(0, [d, 1], coverage))      composited over zeros, antialiased, cut to 1 channel

Dense, every pixel, torch.amin / amax (which share an extreme's gradient equally among all elements that attain it), autograd for the
gradient.  tests/test_depth_tangent_cpu.py holds `depth` against the package's generic shade(); the GPU tests use all of it.
"""
import torch


def dense_positions(rows, pix, bhw):
    """[B,H,W,3] interpolated positions from the rows of the covered pixels ``pix`` (flat indices): zeros where nothing was rasterised --
    what dr.interpolate returns there.  Differentiable in ``rows``."""
    b, h, w = bhw
    return torch.zeros(b * h * w, 3, dtype=rows.dtype, device=rows.device).index_copy(0, pix, rows).view(b, h, w, 3)


def camera_z(gb_pos, w2c):
    """[B,H,W] camera-space z of every pixel (reference :103-105); w2c [B,4,4] or [1,4,4]."""
    b, h, w, _ = gb_pos.shape
    hom = torch.cat([gb_pos, torch.ones_like(gb_pos[..., :1])], dim=-1)
    return torch.matmul(hom.view(b, -1, 4), w2c.transpose(-1, -2)).view(b, h, w, 4)[..., 2]


def depth(gb_pos, w2c):
    """[B,H,W,1] normalised depth of every pixel (reference :103-108)."""
    z = camera_z(gb_pos, w2c)
    lo, hi = z.amin(dim=(1, 2), keepdim=True), z.amax(dim=(1, 2), keepdim=True)
    return ((z - lo) / (hi - lo)).unsqueeze(-1)


def composite(d, cover):
    """[B,H,W,2] = lerp(0, [d, 1], coverage) (reference :258-268 with the zero background of a mode that has none); coverage is 0 or 1."""
    alpha = cover.to(d.dtype)[..., None]
    return torch.lerp(torch.zeros_like(d).expand(-1, -1, -1, 2), torch.cat((d, torch.ones_like(d)), dim=-1), alpha)


def image(rows, pix, cover, w2c, antialias):
    """The mode's image [B,H,W,1]: ``antialias`` maps the composited [B,H,W,2] image to the antialiased one (the caller's operator: the
    float64 oracle, or the package's dense float32 one)."""
    d = depth(dense_positions(rows, pix, cover.shape), w2c)
    return antialias(composite(d, cover).contiguous())[..., :1]


def extreme_gaps(rows, pix, cover, w2c):
    """Per image with a covered pixel: (gap at the minimum, gap at the maximum) in z between the extreme and the nearest DIFFERENT
    candidate, where all uncovered pixels together count as one candidate (they tie by construction, and their share of the gradient
    is w2c's).  float64 on the host.  A case whose gaps are >= 1e-4 has no tie among the covered pixels in any float32 evaluation."""
    b, h, w = cover.shape
    z = camera_z(dense_positions(rows.double().cpu(), pix.cpu(), (b, h, w)), w2c.double().cpu().expand(b, -1, -1)).view(b, -1)
    cov = cover.cpu().view(b, -1)
    gaps = []
    for i in range(b):
        if not bool(cov[i].any()):
            continue
        cand = z[i][cov[i]]
        if not bool(cov[i].all()):
            cand = torch.cat((cand, z[i][~cov[i]][:1]))
        s = torch.sort(cand).values
        assert s.numel() >= 2, "an image with one covered pixel and nothing else has no range"
        gaps.append((float(s[1] - s[0]), float(s[-1] - s[-2])))
    return gaps
