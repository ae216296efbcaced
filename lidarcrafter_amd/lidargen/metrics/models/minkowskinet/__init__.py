"""MinkUNet feature extractor of the Frechet Sparse Volume Distance: `model.Model`."""
