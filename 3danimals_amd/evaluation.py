"""Keypoint-transfer evaluation (PCK@0.1), the mirror of the reference's evaluation/evaluate.py plus the ``evaluate_keypoint`` branch
of visualization/visualize_results.py:213-272 -- without their text files, plots and dataset download: every input and output is a
tensor, and on the GPU nothing synchronises with the host before the final scalar.

Stage 1, ``project_and_occlude``: clip.xy / clip.w and, from one rasterize call, which vertices each image shows
(ops.vertex_visibility, csrc/keypoints.hip).  Stage 2, ``keypoint_transfer_pck``: the nearest visible vertex of every keypoint ONCE per
image (ops.nearest_visible_vertex; the reference recomputes it for every sampled pair), then the pair stage -- gathers, un-crop,
error over the box size, PCK -- as the reference's statements in float64 torch, in the same operation order.

CUDA tensors take the HIP kernels (no fallback: a missing library raises).  CPU tensors take the same float32 rule written in torch
(``_nearest_visible_vertex_torch``), which is what the CPU tests compare with the recorded reference.
"""
import torch

__all__ = ["project_and_occlude", "transfer_keypoints", "crop_keypoints_with_box", "uncrop_keypoints_with_box", "compute_pck",
           "keypoint_transfer_pck"]


def _ops():
    from . import ops

    return ops


def project_and_occlude(v_pos, tri, mvp, resolution):
    """v_pos [B,V,3] posed vertices, tri [F,3], mvp [B|1,4,4], resolution (H, W) -> (uv [B,V,2] = clip.xy / clip.w, visibility [B,V]
    float32 in {0, 1}).  visualize_results.py:219-246: xfm_points, one rasterize, the vertices of the triangles that own a pixel.  No
    host synchronisation; a bad triangle id or corner is reported at the next host read-back (_lib.defer_check)."""
    ops = _ops()
    with torch.no_grad():
        clip = ops.xfm_points(v_pos, mvp)
        uv = clip[..., :2] / clip[..., 3:]
        rast = ops.rasterize(clip, tri, resolution)
        visibility = ops.vertex_visibility(rast, tri, clip.shape[1])
    return uv, visibility


def _nearest_visible_vertex_torch(uv, visibility, keypoints):
    """ops.nearest_visible_vertex's rule in torch (float32, one operation per statement; for CPU tensors): [N,V,2], [N,V], [N,K,2] ->
    int64 [N,K].  The [N,K,V] matrix the kernel avoids is built here."""
    uv, visibility, keypoints = uv.float(), visibility.float(), keypoints.float()
    src = torch.where((visibility == 0)[..., None], torch.full_like(uv, float("inf")), uv)
    dx = src[:, None, :, 0] - keypoints[:, :, None, 0]
    dy = src[:, None, :, 1] - keypoints[:, :, None, 1]
    xx, yy = dx * dx, dy * dy
    d2 = xx + yy
    order = torch.where(torch.isnan(d2), torch.zeros((), dtype=torch.int64, device=d2.device), d2.contiguous().view(torch.int32).long() + 1)
    key = (order << 32) | torch.arange(uv.shape[1], device=uv.device)
    return key.min(dim=2).values & 0xFFFFFFFF


def _nearest(uv, visibility, keypoints):
    if uv.is_cuda:
        return _ops().nearest_visible_vertex(uv, visibility, keypoints)
    return _nearest_visible_vertex_torch(uv, visibility, keypoints)


def transfer_keypoints(source_verts, source_verts_visibility, target_verts, source_kp):
    """evaluate.py:461-472: for each source keypoint the closest VISIBLE source vertex, and that vertex in the target frame.
    source_verts [V,2], source_verts_visibility [V], target_verts [V,2], source_kp [K,2] -> (target_kp_pred [K,2], {"vert_idx": [K]});
    or all four with a leading pair dimension [P,...].  The distances are float32 (ops.nearest_visible_vertex; the reference's are
    float64: a float32 near-tie may pick another vertex).  Unlike the reference, which overwrites the invisible rows of its
    ``source_verts`` argument with inf, this leaves its arguments as they are."""
    source_verts, source_verts_visibility, target_verts, source_kp = (torch.as_tensor(t) for t in (source_verts, source_verts_visibility, target_verts, source_kp))
    single = source_verts.dim() == 2
    if single:
        source_verts, source_verts_visibility, target_verts, source_kp = source_verts[None], source_verts_visibility[None], target_verts[None], source_kp[None]
    if source_verts.dim() != 3 or target_verts.shape != source_verts.shape or source_verts_visibility.shape != source_verts.shape[:2]:
        raise ValueError(f"transfer_keypoints: source_verts {list(source_verts.shape)}, visibility {list(source_verts_visibility.shape)} and "
                         f"target_verts {list(target_verts.shape)} do not belong together")
    vert_idx = _nearest(source_verts, source_verts_visibility, source_kp)
    target_kp_pred = torch.gather(target_verts, 1, vert_idx[..., None].expand(-1, -1, 2))
    if single:
        target_kp_pred, vert_idx = target_kp_pred[0], vert_idx[0]
    return target_kp_pred, {"vert_idx": vert_idx}


def _box(box, like):
    box = torch.as_tensor(box, dtype=torch.float64, device=like.device)
    return tuple(box[..., i, None] if box.dim() > 1 else box[i] for i in range(4))  # xmin, ymin, w, h; a batch of boxes broadcasts over K


def crop_keypoints_with_box(kp, box):
    """evaluate.py:192-204 in float64: kp [...,K,2] in the image frame, box (xmin, ymin, w, h) or [...,4] -> the box's [-1, 1] frame."""
    kp = torch.as_tensor(kp).double()
    xmin, ymin, w, h = _box(box, kp)
    x = kp[..., 0] - xmin
    y = kp[..., 1] - ymin
    x = x / w * 2 - 1
    y = y / h * 2 - 1
    return torch.stack([x, y], dim=-1)


def uncrop_keypoints_with_box(kp, box):
    """evaluate.py:207-224 in float64: kp [...,K,2] in the box's [-1, 1] frame -> the image frame."""
    kp = torch.as_tensor(kp).double()
    xmin, ymin, w, h = _box(box, kp)
    x = (kp[..., 0] + 1) / 2
    y = (kp[..., 1] + 1) / 2
    x = x * w
    y = y * h
    x = x + xmin
    y = y + ymin
    return torch.stack([x, y], dim=-1)


def _pck_per_keypoint(kps_err_all, visible_all, threshold):
    kps_err_all, visible_all = torch.as_tensor(kps_err_all).double(), torch.as_tensor(visible_all).double()
    return ((kps_err_all < threshold) * visible_all).sum(0) / visible_all.sum(0)  # (sums of zeros and ones: exact in any order)


def compute_pck(kps_err_all, visible_all, threshold):
    """evaluate.py:234-237 in float64: [P,K] errors and visibilities -> the mean over keypoints of the visible share below the
    threshold, a 0-dim tensor.  A keypoint visible in no pair divides 0 by 0: the result is NaN, as numpy's is.  The per-keypoint
    shares are numpy's bits; the mean over them is torch's sum, whose order is not numpy's (the last bit may differ)."""
    return _pck_per_keypoint(kps_err_all, visible_all, threshold).mean()


def keypoint_transfer_pck(uv, visibility, keypoints, kp_visible, boxes, pairs, threshold=0.1, box_pad_frac=0):
    """PCK of keypoint transfer over sampled image pairs (the loop of evaluate.py:557-587 without its files).
    Per image: uv [N,V,2] projected vertices, visibility [N,V], keypoints [N,K,2] in the image's cropped [-1, 1] frame, kp_visible
    [N,K], boxes [N,4] (xmin, ymin, w, h); pairs [P,2] int64 (source, target).
    One nearest_visible_vertex call over the N images, then over the pairs in float64: the target's vertices at the source's indices,
    un-cropped with the target's box, against the target's un-cropped keypoints; the error over max(w, h) * (1 + 2 * box_pad_frac);
    visible = source_visible * target_visible.
    -> (pck: Python float, kps_err [P,K] float64, visible [P,K] float64, vert_idx [N,K] int64).  One host read-back, for the scalar
    (the K per-keypoint shares travel; their mean is taken on the host)."""
    pairs = torch.as_tensor(pairs, device=uv.device).long()
    if pairs.dim() != 2 or pairs.shape[1] != 2 or boxes.shape != (uv.shape[0], 4) or kp_visible.shape != keypoints.shape[:2]:
        raise ValueError(f"keypoint_transfer_pck: pairs {list(pairs.shape)}, boxes {list(boxes.shape)}, kp_visible {list(kp_visible.shape)} for "
                         f"{uv.shape[0]} images of {keypoints.shape[1]} keypoints")
    vert_idx = _nearest(uv, visibility, keypoints)
    s, t = pairs[:, 0], pairs[:, 1]
    target_kp_pred = uv[t[:, None], vert_idx[s]]  # [P,K,2]: target_verts[vert_idx], without a [P,V,2] intermediate
    boxes = boxes.double()
    target_box = boxes[t]
    pred_image = uncrop_keypoints_with_box(target_kp_pred, target_box)
    gt_image = uncrop_keypoints_with_box(keypoints[t], target_box)
    dx = gt_image[..., 0] - pred_image[..., 0]
    dy = gt_image[..., 1] - pred_image[..., 1]
    kps_err = torch.sqrt(dx * dx + dy * dy)
    box_size = torch.maximum(target_box[:, 2], target_box[:, 3]) * (1 + 2 * box_pad_frac)
    kps_err = kps_err / box_size[:, None]
    kp_visible = kp_visible.double()
    visible = kp_visible[s] * kp_visible[t]
    shares = _pck_per_keypoint(kps_err, visible, threshold)
    if shares.is_cuda:
        from . import _lib

        shares = _lib.read_back(shares)  # THE read-back: K numbers (+ any pending device-side check)
    return float(shares.numpy().mean()), kps_err, visible, vert_idx  # (the mean of the K shares on the host, in numpy's order: the reference's bits)
