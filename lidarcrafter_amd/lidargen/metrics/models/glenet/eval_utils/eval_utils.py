"""Mirror of the reference's `lidargen/metrics/models/glenet/eval_utils/eval_utils.py` for what the RGF metric takes from it:
`iou3d`.  `eval_one_epoch` (a data-loader loop that pickles per-draw results) is replaced by `fg_object.compute_rgf_fold`."""
from lidarcrafter_amd.ops_glenet import riou3d_paired


def iou3d(gboxes, qboxes):
    """[N]: the IoU of the paired boxes (x, y, z, dx, dy, dz, ry) as the reference computes it -- clamp to +-200, the corners,
    the float32 polygon intersection with its quirks (two identical boxes give 0), the height overlap.  CUDA(HIP) float32
    [N, >= 7]; one kernel (lc_riou3d_paired_fwd), no host loop."""
    return riou3d_paired(gboxes.contiguous(), qboxes.contiguous())
