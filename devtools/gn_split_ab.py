"""One-off A/B of the pre-split writers between two or more builds of the library, in one process:
    python devtools/gn_split_ab.py REF.so NEW.so [NEW2.so ...]
Runs lc_groupnorm_apply_os_split, lc_groupnorm_apply_split and lc_split_act_fwd of every library on the same inputs -- the
three C2 level shapes at batch 8 and the cases of tests/test_gn_split_stores.py -- and reports torch.equal of the planes and
of the range record against the first library, then times the C2 shapes (HIP events around 50 launches, best of 5)."""
import ctypes as ct
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lidarcrafter_amd._lib import SIGNATURES, OctStats  # noqa: E402
from lidarcrafter_amd.testing import seeded_randn  # noqa: E402
from tests.test_gn_split_stores import GN_CASES, PLAIN_CASES, _entries  # noqa: E402

NAMES = ("lc_groupnorm_apply_os_split", "lc_groupnorm_apply_split", "lc_split_act_fwd", "lc_groupnorm_stats",
         "lc_groupnorm_partials_elems", "lc_split_act_units")
dev = torch.device("cuda:0")
libs = []
for path in sys.argv[1:]:
    h = ct.CDLL(os.path.abspath(path))
    for n in NAMES:
        f = getattr(h, n)
        f.restype, f.argtypes = SIGNATURES[n]
    libs.append((os.path.basename(path), h))
st = torch.cuda.current_stream().cuda_stream
p = lambda t: None if t is None else t.data_ptr()  # noqa: E731


def make(B, C, G, H, W, route, act, adagn, affine, wide, seed):
    HW = H * W
    big = (seeded_randn(B, C + (24 if wide else 0), HW, seed=seed) * 3 + 0.5).to(dev)
    x = big[:, 8:8 + C] if wide else big
    gamma = (1 + 0.3 * seeded_randn(C, seed=2)).to(dev) if affine else None
    beta = (0.3 * seeded_randn(C, seed=3)).to(dev) if affine else None
    ss = (0.3 * seeded_randn(B, 2 * C, seed=4)).to(dev) if adagn else None
    segs, c = [], 0
    if route != "os0":
        for ch, unit, slots in route[1]:
            e = _entries(x[:, c:c + ch], unit, slots)
            segs.append((e, OctStats(e.data_ptr(), ch, slots, unit)))
            c += ch
    return dict(B=B, C=C, G=G, H=H, W=W, x=x, gamma=gamma, beta=beta, ss=ss, segs=segs, act=act, keep=big)


def run(h, a, what):
    B, C, G, H, W, x = a["B"], a["C"], a["G"], a["H"], a["W"], a["x"]
    buf = torch.full((int(h.lc_split_act_units(B, C, H, W)), 8), -7.0, device=dev, dtype=torch.float16)
    rng = torch.tensor([16.0, 1 / 16.0, 0.0, 0.0], device=dev)
    ss = a["ss"]
    sc, sf, ss_bs = (ss[:, :C], ss[:, C:], 2 * C) if ss is not None else (None, None, 0)
    if what == "plain":
        rc = h.lc_split_act_fwd(x.data_ptr(), x.stride(0), buf.data_ptr(), B, C, H, W, rng.data_ptr(), st)
        go = lambda: h.lc_split_act_fwd(x.data_ptr(), x.stride(0), buf.data_ptr(), B, C, H, W, rng.data_ptr(), st)  # noqa: E731
    elif a["segs"]:
        s = a["segs"]
        go = lambda: h.lc_groupnorm_apply_os_split(  # noqa: E731
            x.data_ptr(), x.stride(0), ct.byref(s[0][1]), ct.byref(s[1][1]) if len(s) > 1 else None, p(a["gamma"]), p(a["beta"]),
            p(sc), p(sf), ss_bs, buf.data_ptr(), B, a["C"], H, W, G, 1e-6, int(a["act"]), rng.data_ptr(), st)
        rc = go()
    else:
        part = torch.empty(int(h.lc_groupnorm_partials_elems(B, C, H, W, G)), device=dev, dtype=torch.float64)
        rc = h.lc_groupnorm_stats(x.data_ptr(), x.stride(0), part.data_ptr(), B, C, H, W, G, st)
        assert rc == 0, rc
        go = lambda: h.lc_groupnorm_apply_split(  # noqa: E731
            x.data_ptr(), x.stride(0), part.data_ptr(), p(a["gamma"]), p(a["beta"]), p(sc), p(sf), ss_bs, buf.data_ptr(), B,
            a["C"], H, W, G, 1e-6, int(a["act"]), rng.data_ptr(), st)
        rc = go()
        a["part"] = part
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    return buf, rng.clone(), go


def clock(go):
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            go()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 50 * 1e3)
    return best


cases = [("C2 level %d" % (i + 1), (8, Cc, 8, H, W, ("os", [(Cc, 8, sl)]), True, True, False, False), True)
         for i, (Cc, H, W, sl) in enumerate(((128, 16, 512, 32), (256, 8, 256, 8), (512, 4, 128, 2)))]
cases += [("test case %d" % i, (2,) + c, False) for i, c in enumerate(GN_CASES)]
ok = True
for tag, c, timed in cases:
    a = make(*c, seed=11)
    for what in ("gn",) + (("plain",) if a["H"] * a["W"] % 4 == 0 and not a["x"].stride(0) % 4 else ()):
        ref, line = None, []
        for name, h in libs:
            buf, rng, go = run(h, a, what)
            if ref is None:
                ref = (buf, rng)
                same = "ref"
            else:
                eq = torch.equal(buf, ref[0]) and torch.equal(rng, ref[1])
                ok &= eq
                same = "equal" if eq else "DIFFERENT"
            line.append(f"{name} {same}" + (f" {clock(go):6.2f} us" if timed else ""))
        print(f"{tag:14s} {what:5s} B {c[0]} C {c[1]:3d} G {c[2]:2d} {c[3]:2d}x{c[4]:<4d} {str(c[5])[:26]:26s} | " + " | ".join(line),
              flush=True)
for i, (Cc, H, W, wide) in enumerate(PLAIN_CASES):
    a = make(2, Cc, 1, H, W, "os0", False, False, False, wide, seed=13)
    ref, line = None, []
    for name, h in libs:
        buf, rng, _ = run(h, a, "plain")
        eq = ref is None or (torch.equal(buf, ref[0]) and torch.equal(rng, ref[1]))
        ok &= eq
        ref = ref or (buf, rng)
        line.append(f"{name} {'equal' if eq else 'DIFFERENT'}")
    print(f"plain case {i:2d}  C {Cc:3d} {H:2d}x{W:<4d} wide {int(wide)} | " + " | ".join(line), flush=True)
print("BIT-IDENTICAL" if ok else "OUTPUTS DIFFER")
sys.exit(0 if ok else 1)
