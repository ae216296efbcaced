"""Datasets of the evaluation (mirror of the reference's `lidargen/metrics/datasets`): the foreground objects (NuscObject)
and the objects of the RGF metric (object_uncertainty_dataset.NuscObjUncertainty, kfold_indices)."""
