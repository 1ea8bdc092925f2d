"""What render_mesh(spp = s > 1, msaa = True, num_layers = 1) of the reference does BEHIND the shading, statement by statement, in torch
(float32 or float64; reference model/render/render.py):

    :170-171  the raster is minified to the shading grid with nearest sampling: texel (y s, x s) of every s x s block;
    :66       shade() gives EVERY low-resolution pixel alpha 1 -- a pixel without a triangle is shaded from all-zero attributes;
    :217-219  the shaded buffers are magnified back with nearest sampling: the block is a replica of its shading pixel;
    :258-262  lerp(background, [value, 1], full-resolution coverage * alpha);
    :264-267  dr.antialias at full resolution (the modes of render.py:311 only);
    :318      avg_pool2d over the blocks.

Two forms of the same chain: over the CPU oracle's antialias (oracle/raster_ref.py) and over the project's dense ops.antialias on the
GPU.  Both are differentiable by autograd.  Test infrastructure only.
"""
import torch
import torch.nn.functional as F


def minify_nearest(rast, s):
    """F.interpolate(mode='nearest') from [B,h s,w s,C] to [B,h,w,C] reads source index floor(dst * s) = dst * s (render.py:170-171 via
    util.scale_img_nhwc): the TOP-LEFT sample of every block."""
    return rast[:, ::s, ::s]


def magnify_nearest(x, s):
    """F.interpolate(mode='nearest') from [B,h,w,C] to [B,h s,w s,C] reads source index floor(dst / s): block replication."""
    return x.repeat_interleave(s, dim=1).repeat_interleave(s, dim=2)


def avg_pool(x, s):
    return F.avg_pool2d(x.permute(0, 3, 1, 2), s).permute(0, 2, 3, 1)  # util.avg_pool_nhwc


def shaded_from_rows(vals, null_vals, pix, bhw):
    """[B,h,w,C+1], what shade() returns on the shading grid: row ``vals[i]`` at flat pixel ``pix[i]``, the image's ``null_vals`` row where
    the shading sample has no triangle, alpha 1 everywhere."""
    b, h, w = bhw
    C = null_vals.shape[1]
    lo = null_vals[:, None, :].expand(b, h * w, C).reshape(b * h * w, C)
    if pix.shape[0]:
        lo = lo.index_copy(0, pix, vals[: pix.shape[0]])
    return torch.cat((lo, torch.ones_like(lo[:, :1])), dim=-1).view(b, h, w, C + 1)


def compose(shaded_lo, rast_full, background_lo, s, antialias=None):
    """The chain above from the shading grid's buffer [B,h,w,C+1] to the averaged image [B,h,w,C+1].  ``background_lo`` [1|B,h,w,<= C+1]
    (missing trailing channels zero) or None; ``antialias``: callable(full-resolution image) or None (a mode that is not antialiased)."""
    up = magnify_nearest(shaded_lo, s)
    bg = torch.zeros_like(up)
    if background_lo is not None:
        g = magnify_nearest(background_lo.to(up.dtype), s)
        bg = torch.cat((g, g.new_zeros(*g.shape[:3], up.shape[3] - g.shape[3])), dim=-1).expand_as(up)
    cover = (rast_full[..., 3:4] > 0).to(up.dtype) * up[..., -1:]
    acc = torch.lerp(bg, torch.cat((up[..., :-1], torch.ones_like(up[..., -1:])), dim=-1), cover)
    if antialias is not None:
        acc = antialias(acc.contiguous())
    return avg_pool(acc, s)


def oracle_form(shaded_lo, rast_full, background_lo, s, clip, tri, aa=True, opp=None):
    """compose() over oracle.raster_ref.antialias (CPU tensors; ``clip`` in the dtype of ``shaded_lo``)."""
    from oracle import raster_ref

    fn = (lambda img: raster_ref.antialias(img, rast_full, clip, tri, opp)) if aa else None
    return compose(shaded_lo, rast_full, background_lo, s, fn)


def dense_form(ops, shaded_lo, rast_full, background_lo, s, clip, tri, analysis, aa=True):
    """compose() over the project's dense ops.antialias (GPU tensors, float32)."""
    fn = (lambda img: ops.antialias(img, rast_full, clip, tri, analysis=analysis)) if aa else None
    return compose(shaded_lo, rast_full, background_lo, s, fn)


def null_sample_blocks(rast_full, s):
    """bool [B,h,w]: blocks whose shading sample is uncovered while another of their samples is covered."""
    cov = rast_full[..., 3] > 0
    B, H, W = cov.shape
    any_cov = cov.view(B, H // s, s, W // s, s).any(dim=4).any(dim=2)
    return any_cov & ~cov[:, ::s, ::s]
