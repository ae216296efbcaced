"""Evaluation front-end on the device (SURVEY.md section 8f-3 ii): `bev`, `chamfer`, `emd`, `eval_utils.evaluate`, and the
Frechet Point Distance (`extractor.pointnet`, `distribution`, `eval_utils.compute_fpd`).  The other learned-feature
metrics of the reference (FRID / FSVD / FPVD: RangeNet, MinkowskiNet, SPVCNN, PTv3 backbones + checkpoints) are out of
scope."""
# a score line as the reference prints it: a 50-column rule above and below `|<16 blanks>NAME:1.2345E+00<17 blanks>|`
_RULE = "-" * 50
OUTPUT_TEMPLATE = f"{_RULE}\n|{'':16}{{}}:{{:.4E}}{'':17}|\n{_RULE}"

from . import bev, chamfer, distribution, emd, eval_utils, extractor  # noqa: E402,F401
