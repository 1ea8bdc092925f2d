"""The renderutils entry points this package serves (reference model/render/renderutils/ops.py): ``xfm_points`` (:515-531),
``xfm_vectors`` and ``prepare_shading_normal`` (:194-227) on the hot path, called there with use_python=True (render.py:72,278), the
two cube-map prefilters of the environment light, ``diffuse_cubemap`` (:404-411) and ``specular_cubemap`` (:446-458), which the
reference has only inside its CUDA plugin and which run here as HIP kernels (csrc/envlight.hip), and the shading BSDFs ``lambert``,
``frostbite_diffuse``, ``pbr_specular``, ``pbr_bsdf`` (:244-386) and ``image_loss`` (:476-498) as fused HIP kernels (csrc/bsdf.hip) with
their torch twins behind use_python=True.  The four test-only terms ``_fresnel_shlick``, ``_ndf_ggx``, ``_lambda_ggx`` and
``_masking_smith`` (:101-176) are torch.  Every name of the reference's ``renderutils.__all__`` is served."""
from .ops import (_fresnel_shlick, _lambda_ggx, _masking_smith, _ndf_ggx, diffuse_cubemap, frostbite_diffuse, image_loss, lambert,  # noqa: F401
                  pbr_bsdf, pbr_specular, prepare_shading_normal, specular_cubemap, xfm_points, xfm_vectors)
