"""Datasets of the evaluation (mirror of the reference's `lidargen/metrics/datasets`): the foreground objects (NuscObject)."""
