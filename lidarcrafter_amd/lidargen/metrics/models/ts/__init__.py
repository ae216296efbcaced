"""Sparse building blocks (the reference's `models/ts`): `basic_blocks`."""
