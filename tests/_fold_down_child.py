"""Child process of tests/test_error_profiles.py::test_fold_down_first_form: the launcher of the stride-2 conv reads
LC_S2_FORM once per process, so the form that is not the default runs in a process of its own.  Computes
ops.conv_down2 at every shape of _profile_cases.FOLD_SHAPES and saves the results to the file named on the command line;
the parent applies the profile conditions."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main(out_path):
    from lidarcrafter_amd import ops as K
    from tests import _profile_cases as PC

    dev = torch.device("cuda:0")
    out = {"form": os.environ.get("LC_S2_FORM", "")}
    for shape in PC.FOLD_SHAPES:
        t = PC.fold_case(shape, "down").dev(dev)
        y = K.conv_down2(t["x"], K.PackedConv("down"), t["w"], t["b"], emit_stats=True)
        assert not K.range_poll(dev)
        out[str(shape)] = y.cpu()
    torch.save(out, out_path)
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1])
