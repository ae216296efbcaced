"""lidargen.ops.iou3d_nms timing, one process, JSON lines (profiles/iou3d_nms.txt).
  * the device's overlap error against the float64 restatement over the float32 restatement's own (the yardstick of
    tests/test_iou3d*.py), on that test's 3000 rotated pairs;
  * the pairwise kernel at 4096 x 4096 in its three modes (device events around `reps` back-to-back calls);
  * NMS at N = 512, 4096 and 16 384 over clustered boxes (hubs of about 20 boxes, so that most candidates are suppressed, as
    in a detector's post-processing), threshold 0.1: a mask call and a selection call on their own (`mask_call`,
    `select_call`: device events around `reps` back-to-back Python calls, so PER-CALL times that include the launch gaps
    and, for the mask, the allocation of its tensor -- not kernel times from a trace), then end to end (host clock around
    a synchronise, one call per sample) two ways on the SAME mask kernel, alternating --
      device   : mask kernel, selection kernel, 4 bytes back           (ops.nms)
      host walk: mask kernel, the whole mask copied to the host, the greedy walk there in numpy (a Python loop over the
                 boxes; the reference's compiled C++ walk is NOT measured and would be faster than this loop).
    The two keep lists are compared.  The end-to-end samples are single calls of 0.4-10 ms: read them with their spread.
After warm-up, `rounds` rounds; median (min ... max).
python devtools/iou3d_time.py [out_path reps rounds]"""
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _iou3d_oracle as O  # noqa: E402
from lidarcrafter_amd import ops_iou3d as K  # noqa: E402


def per_call_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def clustered(n, seed):
    rng = np.random.default_rng(seed)
    hubs = rng.uniform(-80, 80, (max(1, n // 20), 2))
    centres = hubs[rng.integers(0, len(hubs), n)] + rng.normal(0, 1.5, (n, 2))
    boxes = O.general_boxes(rng, n, centres=centres)
    return boxes[np.argsort(-rng.random(n), kind="stable")]          # already in score order


def host_walk(mask):
    """The reference's walk over the mask on the host (numpy): one pass over the boxes, an OR of a row of words per kept box."""
    n, words = mask.shape
    remv = np.zeros(words, np.uint64)
    keep = []
    for i in range(n):
        nblock, inblock = divmod(i, 64)
        if not (int(remv[nblock]) >> inblock) & 1:
            keep.append(i)
            remv[nblock:] |= mask[i, nblock:]
    return keep


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "iou3d_nms.txt")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    assert torch.cuda.is_available(), "the timing needs the GPU; nothing is measured without it"
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    emit({"device": torch.cuda.get_device_name(0), "host": platform.processor() or platform.machine(),
          "torch": torch.__version__, "reps": reps, "rounds": rounds})

    # the device against the yardstick
    rng = np.random.default_rng(0)
    a, b = O.general_boxes(rng, 3000), O.general_boxes(rng, 3000)
    s32, c32 = O.box_overlap(a, b, np.float32)
    s64, c64 = O.box_overlap(a, b, np.float64)
    same = c32 == c64
    yard = float(np.abs(s32.astype(np.float64) - s64)[same].max())
    got = K.boxes_aligned_iou3d(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), overlap_only=True).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - s64)[same].max())
    emit({"pairs": 3000, "left_out": int((~same).sum()), "yardstick_f32_vs_f64": yard, "device_vs_f64": err,
          "device_over_yardstick": round(err / yard, 3), "device_bits_equal_f32_restatement": int((got == s32).sum())})

    # pairwise 4096 x 4096
    rng = np.random.default_rng(1)
    n = 4096
    ta = torch.from_numpy(O.general_boxes(rng, n, spread=60.0)).to(dev)
    tb = torch.from_numpy(O.general_boxes(rng, n, spread=60.0)).to(dev)
    fns = {"overlap_bev": lambda: K.boxes_overlap_bev(ta, tb), "iou_bev": lambda: K.boxes_iou_bev(ta, tb),
           "iou3d": lambda: K.boxes_iou3d(ta, tb)}
    times = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(per_call_ms(fn, reps))
    share = float((fns["overlap_bev"]() > 0).float().mean())
    emit({"pairwise": [n, n], "share_overlapping": round(share, 4), **{k: stats(v) for k, v in times.items()},
          "iou3d_ns_per_pair": round(statistics.median(times["iou3d"]) * 1e6 / (n * n), 4)})

    # NMS
    for n in (512, 4096, 16384):
        boxes = torch.from_numpy(clustered(n, n)).to(dev)
        thresh = 0.1
        mask = K.nms_mask(boxes, thresh)

        def device():
            return K.nms(boxes, thresh)

        def host():
            m = K._mask(boxes, thresh, False, n, zero=False)
            return host_walk(m.cpu().numpy().view(np.uint64))

        keep_d, keep_h = device(), host()
        agree = keep_d.tolist() == keep_h
        t_mask = [per_call_ms(lambda: K._mask(boxes, thresh, False, n, zero=False), reps) for _ in range(rounds)]
        keep_buf = torch.empty(n, device=dev, dtype=torch.int64)
        count = torch.empty(1, device=dev, dtype=torch.int32)
        lib = K.lib()

        def select_only():
            K.check(lib.lc_nms_select_fwd(mask.data_ptr(), n, keep_buf.data_ptr(), count.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "lc_nms_select_fwd")

        select_only()
        t_sel = [per_call_ms(select_only, reps) for _ in range(rounds)]
        w_dev, w_host = [], []
        for _ in range(rounds):
            w_dev.append(wall_ms(device)[0])
            w_host.append(wall_ms(host)[0])
        emit({"nms_boxes": n, "thresh": thresh, "kept": len(keep_h), "keep_lists_equal": agree,
              "mask_words": int(mask.numel()), "mask_call": stats(t_mask), "select_call": stats(t_sel),
              "end_to_end_device": stats(w_dev), "end_to_end_host_walk": stats(w_host),
              "host_walk_over_device": round(statistics.median(w_host) / statistics.median(w_dev), 2)})

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
