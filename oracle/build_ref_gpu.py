"""Build the REFERENCE's own GPU kernels for gfx950 (TEST INFRASTRUCTURE).

Where the reference lies under /root/reference (the build container), its CUDA extensions are
run through `hipify-perl` and compiled with `hipcc --offload-arch=gfx950` against the installed
torch headers; nothing of the reference is edited, copied into the repository or committed:
the hipified text and the modules live only under oracle/_ref/, which git ignores.

  roiaware_pool3d_gpu_ref{,_fc}  <- lidargen/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu
                                    + roiaware_pool3d.cpp   (forward, backward, points_in_boxes_gpu/_cpu)
  chamfer_3d_ref{,_fc}           <- lidargen/metrics/modules/chamfer3D/chamfer3D.cu
                                    + chamfer_cuda.cpp      (forward, backward)

Each extension is built twice: the plain name with -ffp-contract=off (the arithmetic the product
kernels promise), the `_fc` name with hipcc's default contraction (the closest match to nvcc's
default --fmad=true, which the reference was written for).  oracle/_ref/gpu_ref_stamp.json lists
what was built; `load_gpu_ref(name)` returns None while it is absent.  The extensions launch on the
null stream: callers synchronise around every call.  Nothing in the product imports this module."""
from __future__ import annotations

import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = "/root/reference"
REF_DIR = os.path.join(HERE, "_ref")
STAMP = os.path.join(REF_DIR, "gpu_ref_stamp.json")
ARCH = "gfx950"

# extension name -> (reference directory, sources relative to it, functions it must expose)
EXTENSIONS = {
    "roiaware_pool3d_gpu_ref": (
        "lidargen/ops/roiaware_pool3d/src",
        ["roiaware_pool3d_kernel.cu", "roiaware_pool3d.cpp"],
        ["forward", "backward", "points_in_boxes_gpu", "points_in_boxes_cpu"]),
    "chamfer_3d_ref": (
        "lidargen/metrics/modules/chamfer3D",
        ["chamfer3D.cu", "chamfer_cuda.cpp"],
        ["forward", "backward"]),
}
# build suffix -> extra hipcc flags
MODES = {"": ["-ffp-contract=off"], "_fc": []}


def module_names():
    return [base + sfx for base in EXTENSIONS for sfx in MODES]


def expected_functions(name):
    base = name[:-len("_fc")] if name.endswith("_fc") else name
    return EXTENSIONS[base][2]


def _sources(base):
    d, files, _ = EXTENSIONS[base]
    return [os.path.join(REF_ROOT, d, f) for f in files]


def _hipify(base):
    """hipify-perl each source of `base` into oracle/_ref/src/<base>/ (.cu -> .hip); returns paths."""
    out_dir = os.path.join(REF_DIR, "src", base)
    os.makedirs(out_dir, exist_ok=True)
    outs = []
    for src in _sources(base):
        stem, ext = os.path.splitext(os.path.basename(src))
        dst = os.path.join(out_dir, stem + (".hip" if ext == ".cu" else ext))
        if not os.path.exists(dst) or os.path.getmtime(src) > os.path.getmtime(dst):
            txt = subprocess.run(["hipify-perl", "-quiet-warnings", src], check=True,
                                 stdout=subprocess.PIPE).stdout
            with open(dst + ".tmp", "wb") as f:
                f.write(txt)
            os.replace(dst + ".tmp", dst)
        outs.append(dst)
    return outs


def _flags():
    import sysconfig

    import torch
    from torch.utils.cpp_extension import include_paths

    tl = os.path.join(os.path.dirname(torch.__file__), "lib")
    inc = [f"-I{p}" for p in include_paths("cuda")] + [f"-I{sysconfig.get_paths()['include']}"]
    defs = ["-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DHIPBLAS_V2",
            "-D__HIP_NO_HALF_OPERATORS__=1", "-D__HIP_NO_HALF_CONVERSIONS__=1",
            "-DTORCH_API_INCLUDE_EXTENSION_H",
            f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}"]
    libs = [f"-L{tl}", "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu", "-ltorch_hip",
            "-ltorch_python", f"-Wl,-rpath,{tl}"]
    return inc, defs, libs


def _hipcc():
    from lidarcrafter_amd.build import hipcc  # the same compiler lookup as the product build

    return hipcc()


def _stamp_ok(recipe_mtime):
    if not os.path.exists(STAMP):
        return False
    try:
        with open(STAMP) as f:
            st = json.load(f)
    except (OSError, ValueError):
        return False
    if sorted(st.get("modules", {})) != sorted(module_names()):
        return False
    for name in module_names():
        so = os.path.join(REF_DIR, name + ".so")
        if not os.path.exists(so) or os.path.getmtime(so) < recipe_mtime:
            return False
        base = name[:-len("_fc")] if name.endswith("_fc") else name
        if any(os.path.getmtime(s) > os.path.getmtime(so) for s in _sources(base)):
            return False
    return True


def build(verbose=True):
    """Only where the reference exists; elsewhere leave whatever oracle/_ref/ holds alone.
    Returns the stamp path, or None where the reference is absent."""
    if not all(os.path.exists(s) for base in EXTENSIONS for s in _sources(base)):
        return None
    recipe_mtime = os.path.getmtime(os.path.abspath(__file__))
    if _stamp_ok(recipe_mtime):
        return STAMP
    os.makedirs(REF_DIR, exist_ok=True)
    if os.path.exists(STAMP):
        os.remove(STAMP)               # a half-finished rebuild must not look complete
    inc, defs, libs = _flags()
    cc = _hipcc()
    procs, record = [], {}
    for base in EXTENSIONS:
        srcs = _hipify(base)
        for sfx, mode_flags in MODES.items():
            name = base + sfx
            so = os.path.join(REF_DIR, name + ".so")
            cmd = [cc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", "-w",
                   f"-DTORCH_EXTENSION_NAME={name}"] + mode_flags + defs + inc + srcs + \
                  ["-o", so + ".tmp"] + libs
            procs.append((name, so, cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE,
                                                          stderr=subprocess.STDOUT)))
            record[name] = {"sources": [os.path.relpath(s, REF_ROOT) for s in _sources(base)],
                            "fp_contract": "off" if mode_flags else "default",
                            "functions": expected_functions(name)}
    failed = []
    for name, so, cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed.append(f"{name}: {' '.join(cmd)}\n{out.decode(errors='replace')}")
            continue
        os.replace(so + ".tmp", so)
        if verbose:
            print("built", os.path.relpath(so, os.path.dirname(HERE)))
    if failed:
        raise RuntimeError("reference GPU build failed:\n" + "\n".join(failed))
    with open(STAMP, "w") as f:
        json.dump({"arch": ARCH, "modules": record}, f, indent=1, sort_keys=True)
    return STAMP


def stamp():
    """The stamp's contents, or None where nothing was built."""
    if not os.path.exists(STAMP):
        return None
    with open(STAMP) as f:
        return json.load(f)


def load_gpu_ref(name):
    """Import oracle/_ref/<name>.so; None while the stamp is absent.  Raises if the stamp lists the
    module and it does not load."""
    st = stamp()
    if st is None:
        return None
    if name not in st["modules"]:
        raise KeyError(f"{name} is not listed in {STAMP}")
    import importlib.util

    import torch  # noqa: F401  (libtorch and its HIP half must be loaded first)

    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_DIR, name + ".so"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    print(build())
