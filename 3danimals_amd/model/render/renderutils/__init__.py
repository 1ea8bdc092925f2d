"""The renderutils entry points this package serves (reference model/render/renderutils/ops.py): ``xfm_points`` (:515-531),
``xfm_vectors`` and ``prepare_shading_normal`` (:194-227) on the hot path, called there with use_python=True (render.py:72,278), and the
two cube-map prefilters of the environment light, ``diffuse_cubemap`` (:404-411) and ``specular_cubemap`` (:446-458), which the
reference has only inside its CUDA plugin and which run here as HIP kernels (csrc/envlight.hip).  The rest of that plugin has torch
paths in the reference (use_python=True) and is not provided."""
from .ops import diffuse_cubemap, prepare_shading_normal, specular_cubemap, xfm_points, xfm_vectors  # noqa: F401
