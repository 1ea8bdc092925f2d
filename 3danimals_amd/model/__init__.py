"""Mirror of the reference's ``model`` package for the replaced hot-path modules only:
``model.geometry.{dmtet,skinning,util}`` and ``model.render.{mesh,render,util,light,renderutils}``
(SURVEY.md section 8b), plus ``model.dataset.util.compute_distance_transform`` (not part of the overlay: INTEGRATION.md).
Predictors, networks, the dataset classes and the Trainer stay the reference's own."""
