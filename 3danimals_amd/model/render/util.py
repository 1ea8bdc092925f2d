"""Small math helpers on the hot path -- the subset of /root/reference/model/render/util.py that the
replaced modules (and their callers) use.  Plain torch; fused into kernels where it matters: the environment-probe resamplers
(latlong_to_cubemap / cubemap_to_latlong) are one HIP launch each on CUDA float32 maps.  Image files: Radiance .hdr through
3danimals_amd.hdrio, the rest through Pillow where it is installed (stand-alone only)."""
import importlib
import os

import numpy as np
import torch

from ... import hdrio, ops


def dot(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return torch.sum(x * y, -1, keepdim=True)


def reflect(x: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    return 2 * dot(x, n) * n - x


def length(x: torch.Tensor, eps: float = 1e-20) -> torch.Tensor:
    """sqrt(max(x.x, eps)): the clamp keeps the gradient finite at 0 (reference util.py:28-29)."""
    return torch.sqrt(torch.clamp(dot(x, x), min=eps))


def safe_normalize(x: torch.Tensor, eps: float = 1e-20) -> torch.Tensor:
    return x / length(x, eps)


def to_hvec(x: torch.Tensor, w: float) -> torch.Tensor:
    return torch.nn.functional.pad(x, pad=(0, 1), mode="constant", value=w)


# ---------------------------------------------------------------------------------------------- sRGB colour transforms (reference :41-57)
def _rgb_to_srgb(f: torch.Tensor) -> torch.Tensor:
    return torch.where(f <= 0.0031308, f * 12.92, torch.pow(torch.clamp(f, 0.0031308), 1.0 / 2.4) * 1.055 - 0.055)


def rgb_to_srgb(f: torch.Tensor) -> torch.Tensor:
    assert f.shape[-1] == 3 or f.shape[-1] == 4
    return torch.cat((_rgb_to_srgb(f[..., 0:3]), f[..., 3:4]), dim=-1) if f.shape[-1] == 4 else _rgb_to_srgb(f)


def _srgb_to_rgb(f: torch.Tensor) -> torch.Tensor:
    return torch.where(f <= 0.04045, f / 12.92, torch.pow((torch.clamp(f, 0.04045) + 0.055) / 1.055, 2.4))


def srgb_to_rgb(f: torch.Tensor) -> torch.Tensor:
    assert f.shape[-1] == 3 or f.shape[-1] == 4
    return torch.cat((_srgb_to_rgb(f[..., 0:3]), f[..., 3:4]), dim=-1) if f.shape[-1] == 4 else _srgb_to_rgb(f)


# ---------------------------------------------------------------------------------------------- environment probes (reference :96-133)
HIP_ENVMAP = True  # the two resamplers on CUDA float32 maps: one launch each way (False: the torch statements, ~90 launches for a cube)


def _dr():
    return importlib.import_module(__package__.rsplit(".", 2)[0] + ".shims.nvdiffrast.torch")


def cube_to_dir(s, x, y):
    """The direction of face coordinates (x, y) in -1..1 on cube face ``s`` (+x -x +y -y +z -z); ops.texture's cube lookup inverts it."""
    if s == 0:   rx, ry, rz = torch.ones_like(x), -y, -x
    elif s == 1: rx, ry, rz = -torch.ones_like(x), -y, x
    elif s == 2: rx, ry, rz = x, torch.ones_like(x), y
    elif s == 3: rx, ry, rz = x, -torch.ones_like(x), -y
    elif s == 4: rx, ry, rz = x, -y, torch.ones_like(x)
    elif s == 5: rx, ry, rz = -x, -y, -torch.ones_like(x)
    return torch.stack((rx, ry, rz), dim=-1)


def _latlong_to_cubemap_torch(latlong_map, res):
    """The reference's statements (:105-118), on the map's device and in its dtype: the specification of ops.latlong_to_cubemap."""
    dr, dev, dt = _dr(), latlong_map.device, latlong_map.dtype
    faces = []
    for s in range(6):
        gy, gx = torch.meshgrid(torch.linspace(-1.0 + 1.0 / res[0], 1.0 - 1.0 / res[0], res[0], device=dev, dtype=dt),
                                torch.linspace(-1.0 + 1.0 / res[1], 1.0 - 1.0 / res[1], res[1], device=dev, dtype=dt), indexing="ij")
        v = safe_normalize(cube_to_dir(s, gx, gy))

        tu = torch.atan2(v[..., 0:1], -v[..., 2:3]) / (2 * np.pi) + 0.5
        tv = torch.acos(torch.clamp(v[..., 1:2], min=-1, max=1)) / np.pi
        texcoord = torch.cat((tu, tv), dim=-1)

        faces.append(dr.texture(latlong_map[None, ...], texcoord[None, ...], filter_mode="linear")[0])
    return torch.stack(faces, dim=0)


def _cubemap_to_latlong_torch(cubemap, res):
    """The reference's statements (:120-133): the specification of ops.cubemap_to_latlong."""
    dr, dev, dt = _dr(), cubemap.device, cubemap.dtype
    gy, gx = torch.meshgrid(torch.linspace(0.0 + 1.0 / res[0], 1.0 - 1.0 / res[0], res[0], device=dev, dtype=dt),
                            torch.linspace(-1.0 + 1.0 / res[1], 1.0 - 1.0 / res[1], res[1], device=dev, dtype=dt), indexing="ij")

    sintheta, costheta = torch.sin(gy * np.pi), torch.cos(gy * np.pi)
    sinphi, cosphi = torch.sin(gx * np.pi), torch.cos(gx * np.pi)

    reflvec = torch.stack((sintheta * sinphi, costheta, -sintheta * cosphi), dim=-1)
    return dr.texture(cubemap[None, ...], reflvec[None, ...].contiguous(), filter_mode="linear", boundary_mode="cube")[0]


def latlong_to_cubemap(latlong_map, res):
    """[H,W,C] lat-long map -> [6,res[0],res[1],C] cube.  A CUDA float32 map takes ops.latlong_to_cubemap (one HIP launch, one more
    for the gradient of the map); CPU tensors, float64 and HIP_ENVMAP = False take the torch statements above."""
    if HIP_ENVMAP and ops.envmap_device_ok(latlong_map):
        return ops.latlong_to_cubemap(latlong_map, res)
    return _latlong_to_cubemap_torch(latlong_map, res)


def cubemap_to_latlong(cubemap, res):
    """[6,S,S,C] cube -> [res[0],res[1],C] lat-long map.  Routes like latlong_to_cubemap; there is no cube tap for CPU tensors
    (NotImplementedError, the shim's)."""
    if HIP_ENVMAP and ops.envmap_device_ok(cubemap):
        return ops.cubemap_to_latlong(cubemap, res)
    return _cubemap_to_latlong_torch(cubemap, res)


# ---------------------------------------------------------------------------------------------- image files (reference :423-447)
# Stand-alone only: overlaid on the reference tree, its callers keep the reference's imageio versions.
_STANDALONE_ONLY = ("load_image", "load_image_raw", "save_image", "save_image_raw")


def _is_hdr(fn):
    return os.path.splitext(fn)[1].lower() == ".hdr"


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("only Radiance .hdr files are read and written without the Pillow package") from e
    return Image


def load_image_raw(fn) -> np.ndarray:
    """.hdr: float32 [H,W,3] (3danimals_amd.hdrio); every other format through Pillow, in the file's own dtype."""
    if _is_hdr(fn):
        return hdrio.read_hdr(fn)
    with _pil().open(fn) as im:
        return np.asarray(im).copy()


def load_image(fn) -> np.ndarray:
    img = load_image_raw(fn)
    if img.dtype == np.float32:  # HDR image
        return img
    return img.astype(np.float32) / 255  # LDR image


def save_image(fn, x: np.ndarray):
    """An LDR image through Pillow: rint(x * 255) clipped to uint8.  Failures raise (the reference prints a warning)."""
    _pil().fromarray(np.clip(np.rint(np.asarray(x) * 255.0), 0, 255).astype(np.uint8)).save(fn)


def save_image_raw(fn, x: np.ndarray):
    """A float image as it is: Radiance .hdr (3danimals_amd.hdrio) is the one format written; anything else raises."""
    if not _is_hdr(fn):
        raise ValueError(f"save_image_raw: only Radiance .hdr files are written, got {fn!r}")
    hdrio.write_hdr(fn, x)


def perspective(fovy=0.7854, aspect=1.0, n=0.1, f=1000.0, device=None):
    """gluPerspective with y flipped so images come out upright (reference util.py:189-194)."""
    y = np.tan(fovy / 2)
    return torch.tensor([[1 / (y * aspect), 0, 0, 0], [0, 1 / -y, 0, 0], [0, 0, -(f + n) / (f - n), -(2 * f * n) / (f - n)], [0, 0, -1, 0]],
                        dtype=torch.float32, device=device)


def fovx_to_fovy(fovx, aspect):
    return np.arctan(np.tan(fovx / 2) / aspect) * 2.0


def focal_length_to_fovy(focal_length, sensor_height):
    return 2 * np.arctan(0.5 * sensor_height / focal_length)


def scale_img_nhwc(x: torch.Tensor, size, mag="bilinear", min="area") -> torch.Tensor:
    """Resize an NHWC image (reference util.py:97-108); only reached when spp > 1."""
    assert (x.shape[1] >= size[0] and x.shape[2] >= size[1]) or (x.shape[1] < size[0] and x.shape[2] < size[1])
    y = x.permute(0, 3, 1, 2)
    if x.shape[1] > size[0] and x.shape[2] > size[1]:
        y = torch.nn.functional.interpolate(y, size, mode=min)
    elif mag in ("bilinear", "bicubic"):
        y = torch.nn.functional.interpolate(y, size, mode=mag, align_corners=True)
    else:
        y = torch.nn.functional.interpolate(y, size, mode=mag)
    return y.permute(0, 2, 3, 1).contiguous()


def avg_pool_nhwc(x: torch.Tensor, size) -> torch.Tensor:
    y = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), size)
    return y.permute(0, 2, 3, 1).contiguous()


def checkerboard(res, checker_size) -> np.ndarray:
    tiles_y, tiles_x = (res[0] + checker_size * 2 - 1) // (checker_size * 2), (res[1] + checker_size * 2 - 1) // (checker_size * 2)
    check = np.kron([[1, 0] * tiles_x, [0, 1] * tiles_x] * tiles_y, np.ones((checker_size, checker_size))) * 0.33 + 0.33
    check = check[: res[0], : res[1]]
    return np.stack((check, check, check), axis=-1)
