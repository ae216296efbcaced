"""Shapes, seeded inputs and CPU references of the error-profile tests (tests/test_error_profiles.py on the GPU,
tests/test_error_profiles_host.py on the CPU): one place, so the two files cannot drift apart.

Every case gives its inputs (float32, seeded) and `ref(dtype)`, the same operation in plain torch / the oracle's
restatement evaluated in float32 or float64.  `check_profiles` applies the two conditions of DESIGN.md
("Error profiles") to a kernel result:

  bound        every slice error  <=  tol * max(1, r_ref)         r_ref = worst slice / whole tensor of ref32 - ref64
  uniformity   worst slice / median slice  <=  margin * u_ref     u_ref = worst slice / median slice of ref32 - ref64

`tol` is the whole-tensor tolerance of the kernel's existing test, taken from that file; r_ref and u_ref are computed at
run time at the same shape and slicing.  UNIFORMITY_MARGIN = 2 covers a summation order other than the CPU's."""
import functools

import torch
import torch.nn.functional as F

from lidarcrafter_amd.testing import error_profiles, seeded_randn

MIN_ELEMS = 64
UNIFORMITY_MARGIN = 2.0


def _marks(fn, name):
    """The values of one `parametrize` mark of an existing test: its list is used as it stands there."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == name:
            return list(m.args[1])
    raise KeyError(name)


def existing_lists():
    """Tile configurations and tolerances of the existing kernel tests (imported, not copied)."""
    from tests import test_hip_parity as P

    return {"conv_cfgs": _marks(P.test_conv, "cfg"), "gn_cfgs": _marks(P.test_conv_fused_groupnorm, "cfg"),
            "attn_tol": dict(P.ATTN_TOL)}


# tolerances of the existing tests (file::test in the comment); no new figure.  Those tests state them as literals inside
# their assertions, so they are restated here; the two that have a name there (KERNEL_TOL, ATTN_TOL) are imported
TOL_CONV = 2e-6          # test_hip_parity::test_conv
TOL_CONV_GN = 3e-6       # test_hip_parity::test_conv_fused_groupnorm
TOL_CONV_PS = 2e-6       # test_presplit::test_conv_presplit_vs_oracle, test_conv_presplit_split_k
TOL_FOLD = 2e-6          # test_fold_down / test_fold_up ::*_vs_oracle_and_unfolded_route
TOL_RESAMPLE = 1e-6      # test_hip_parity::test_resample, test_groupnorm_resample_pair
TOL_GN = 2e-6            # test_hip_parity::test_groupnorm
TOL_GN_LARGE_MEAN = 1e-4  # test_hip_parity::test_groupnorm_large_mean
TOL_NA = 1e-5            # test_hdit::test_neighbourhood_attention_against_float64
TOL_NA_BWD = 5e-5        # test_hdit_training::test_neighbourhood_backward_against_float64
from tests.test_layout_gen import KERNEL_TOL as TOL_SKINNY      # the one source with a named constant (ATTN_TOL: existing_lists)
TOL_CONV_BWD = 2e-6      # test_training::test_conv_gradients
TOL_ATTN_BWD = 3e-6      # test_training::test_flash_attention_gradients
TOL_GN_BWD = 5e-6        # test_training::test_groupnorm_gradients

# (B, Ci, Co, H, W, ks): the ping-pong kernel's conditions; the tall kernel walks two strips; everything ragged
# (partial channel chunks in and out, H and W off every tile size); 1x1 with a partial last 64-channel chunk and with
# three output blocks
CONV_SHAPES = [(2, 64, 128, 8, 128, 3), (1, 64, 64, 16, 256, 3), (2, 42, 70, 5, 50, 3), (2, 96, 64, 4, 64, 1),
               (2, 128, 192, 8, 128, 1)]
NCHW_KEEPS = ((0,), (1,), (2,), (3,), (2, 3))          # sample, channel, row, column, pixel map
FOLD_SHAPES = [(2, 64, 64, 8, 128), (2, 64, 64, 4, 128)]          # (B, Ci, Co, H, W) of the fold's INPUT
RESAMPLE_SHAPES = [(2, 64, 8, 256), (2, 11, 6, 10)]               # the vector kernels; ragged, scalar kernels (66 per output column)
GN_SHAPES = [(3, 96, 5, 50, 32), (2, 64, 8, 128, 8)]
ATTN_CASES = [("mha", 2, 4, 32, 300), ("two_seg", 8, 8, 64, 500)]  # (kind, B, heads, d_qk, L)
# attention_units needs whole 32-key tiles of image keys: the two-segment operands of the 8-wave block at L = 512
ATTN_UNITS_CASE = ("two_seg", 8, 8, 64, 512)
NA_GRIDS = [(5, 12, 5, 7), (6, 5, 5, 7), (8, 64, 3, 9)]           # (h, w, kh, kw): h == kh; w < kw; the level-2 grid
NA_D = [32, 64]
SKINNY_CASES = [(7, 20, 512), (37, 512, 20), (33, 1664, 256)]
CONV_BWD_SHAPES = [(1, 64, 64, 8, 128, 3), (2, 96, 130, 5, 50, 3)]
ATTN_BWD_CASE = (2, 4, 32, 32, 100, 113)                          # (B, heads, d_qk, d_v, Lq, Lk)
GN_BWD_SHAPE = (3, 96, 5, 50, 32)


def gn_groups(C):
    return 8 if C % 64 == 0 else (32 if C % 32 == 0 else 2)


def usable(shape, keeps, min_elems=MIN_ELEMS):
    """The profiles of `keeps` whose slices hold at least `min_elems` elements at `shape`; the rest are left out by the
    helper's own rule (it refuses them), never by lowering the rule."""
    out = []
    n = 1
    for s in shape:
        n *= s
    for keep in keeps:
        m = 1
        for a in keep:
            m *= shape[a]
        if n // m >= min_elems:
            out.append(tuple(keep))
    return tuple(out)


def check_profiles(got, ref32, ref64, keeps, tol, margins=None, name=""):
    """-> (lines, failures).  lines: one per profile with every figure; failures: the violated conditions, each naming
    the worst slice.  margins: {keep: uniformity factor} for profiles with a derived exception (default 2)."""
    asked = tuple(tuple(kp) for kp in keeps)
    keeps = usable(ref64.shape, asked)
    k = error_profiles(got, ref64, keeps, MIN_ELEMS)
    r = error_profiles(ref32, ref64, keeps, MIN_ELEMS)
    lines = [f"{name}: whole {k['whole']:.3e} (ref32 {r['whole']:.3e}, tol {tol:.1e})"]
    for keep in asked:
        if keep not in keeps:
            lines.append(f"  axes {keep}: NOT CHECKED, its slices hold fewer than {MIN_ELEMS} elements at {tuple(ref64.shape)}")
    fails = []
    if not k["whole"] <= tol:
        fails.append(f"{name}: whole-tensor error {k['whole']:.3e} > {tol:.1e}")
    for keep in keeps:
        pk, pr = k["profiles"][keep], r["profiles"][keep]
        r_ref = pr["worst"] / r["whole"] if r["whole"] > 0 else 1.0
        u_ref = pr["worst"] / pr["median"] if pr["median"] > 0 else float("inf")
        bound = tol * max(1.0, r_ref)
        u = 1.0 if pk["worst"] == 0 else (pk["worst"] / pk["median"] if pk["median"] > 0 else float("inf"))
        ratio = pk["worst"] / k["whole"] if k["whole"] > 0 else 1.0
        margin = (margins or {}).get(keep, UNIFORMITY_MARGIN)
        lines.append(f"  axes {keep}: worst {pk['worst']:.3e} at {pk['index']} = {ratio:.2f} x whole (r_ref {r_ref:.2f}, "
                     f"bound {bound:.2e}); worst / median {u:.2f} (u_ref {u_ref:.2f}, limit {margin * u_ref:.2f})")
        if not (u_ref < float("inf") and r["whole"] > 0):      # (nan fails too)
            fails.append(f"{name}: axes {keep}: the float32 reference is exact in its median slice (or everywhere): no u_ref, "
                         f"the uniformity condition would pass vacuously -- change the input")
        if not pk["worst"] <= bound:
            fails.append(f"{name}: axes {keep} slice {pk['index']} error {pk['worst']:.3e} > bound {bound:.3e}")
        if not u <= margin * u_ref:
            fails.append(f"{name}: axes {keep} slice {pk['index']} is {u:.2f} x the median slice, limit {margin * u_ref:.2f}")
    return lines, fails


class Case:
    """Seeded float32 inputs `t` (a dict) + `fn(t in dtype) -> result or tuple of results`; `ref(dtype)` is cached."""

    def __init__(self, t, fn):
        self.t, self._fn, self._refs = t, fn, {}

    def ref(self, dtype):
        if dtype not in self._refs:
            with torch.no_grad():
                c = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in self.t.items()}
                self._refs[dtype] = self._fn(c)
        return self._refs[dtype]

    @property
    def ref32(self):
        return self.ref(torch.float32)

    @property
    def ref64(self):
        return self.ref(torch.float64)

    def dev(self, dev):
        return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in self.t.items()}


def _D():
    from oracle import denoiser as D

    return D


def _ada(D, c, G, C):
    h = D.group_norm(c["x"], G, c["ga"], c["be"], 1e-6)
    return D.silu(h * (1 + c["ss"][:, :C, None, None]) + c["ss"][:, C:, None, None])


@functools.lru_cache(maxsize=None)
def conv_case(shape, mode):
    """mode "plain": (conv_ring(x, w, b) + res) * 0.7071 (test_conv's operands).
    mode "gn": the same behind SiLU(AdaGN(GroupNorm(x))) -- what the fused-GroupNorm kernels and the pre-split route
    (GroupNorm apply + split, then the LDS-DMA conv) both compute."""
    B, Ci, Co, H, W, ks = shape
    D = _D()
    t = dict(x=seeded_randn(B, Ci, H, W, seed=1), w=seeded_randn(Co, Ci, ks, ks, seed=2) / (Ci * ks * ks) ** 0.5,
             b=seeded_randn(Co, seed=3), res=seeded_randn(B, Co, H, W, seed=4))
    if mode == "plain":
        return Case(t, lambda c: (D.conv_ring(c["x"], c["w"], c["b"]) + c["res"]) * 0.7071)
    G = gn_groups(Ci)
    t.update(x=seeded_randn(B, Ci, H, W, seed=50) * 1.3 + 0.4, ga=1 + 0.1 * seeded_randn(Ci, seed=53),
             be=0.1 * seeded_randn(Ci, seed=54), ss=0.3 * seeded_randn(B, 2 * Ci, seed=55))
    return Case(t, lambda c: (D.conv_ring(_ada(D, c, G, Ci), c["w"], c["b"]) + c["res"]) * 0.7071)


@functools.lru_cache(maxsize=None)
def fold_case(shape, kind):
    """kind "down": Resample(down=2)(conv_ring(x) + b); "up": conv_ring(Resample(up=2)(x)) + b, plus Resample(up=2)(x2)."""
    B, Ci, Co, H, W = shape
    D = _D()
    t = dict(x=seeded_randn(B, Ci, H, W, seed=7 * Ci + H) * 1.3 - 0.2, w=seeded_randn(Co, Ci, 3, 3, seed=62) / (Ci * 9) ** 0.5,
             b=seeded_randn(Co, seed=63), x2=seeded_randn(B, Co, H, W, seed=64) + 0.3)
    if kind == "down":
        return Case(t, lambda c: D.resample_down2(D.conv_ring(c["x"], c["w"], c["b"])))
    return Case(t, lambda c: (D.conv_ring(D.resample_up2(c["x"]), c["w"], c["b"]), D.resample_up2(c["x2"])))


@functools.lru_cache(maxsize=None)
def resample_case(shape, up):
    D = _D()
    t = dict(x=seeded_randn(*shape, seed=12) + 0.3)
    return Case(t, lambda c: D.resample_up2(c["x"]) if up else D.resample_down2(c["x"]))


def gn_apply(c, G, eps=1e-6):
    """SiLU(AdaGN(GroupNorm(x))) with affine and scale / shift in the dtype of c["x"]."""
    D = _D()
    C = c["x"].shape[1]
    h = D.group_norm(c["x"], G, c.get("ga"), c.get("be"), eps)
    if c.get("ss") is not None:
        h = h * (1 + c["ss"][:, :C, None, None]) + c["ss"][:, C:, None, None]
    return D.silu(h)


def gn_params(B, C):
    return dict(ga=1 + 0.1 * seeded_randn(C, seed=8), be=0.1 * seeded_randn(C, seed=9), ss=seeded_randn(B, 2 * C, seed=10) * 0.3)


@functools.lru_cache(maxsize=None)
def gn_case(shape):
    B, C, H, W, G = shape
    t = dict(x=seeded_randn(B, C, H, W, seed=7) * 1.7 + 0.3, **gn_params(B, C))
    return Case(t, lambda c: gn_apply(c, G))


@functools.lru_cache(maxsize=None)
def gn_large_mean_case():
    """test_groupnorm_large_mean's input at a quarter of its width: |mean| = 3000 std."""
    D = _D()
    t = dict(x=seeded_randn(1, 64, 32, 256, seed=12) * 0.01 + 30.0)
    return Case(t, lambda c: D.group_norm(c["x"], 8, None, None, 1e-6))


def gn_views(y, G):
    """[B, C, H, W] -> [B, G, C / G, H, W]: axes (0, 1) = (sample, group), 3 = row, 4 = column."""
    B, C, H, W = y.shape
    return y.reshape(B, G, C // G, H, W)


GN_KEEPS = ((0, 1), (3,), (4,))          # on gn_views; the channel profile is (1,) of the plain [B, C, H, W]


@functools.lru_cache(maxsize=None)
def attn_case(kind, B, heads, d, L):
    """"mha": test_attention_mha's operands (d_v = d); "two_seg": test_attention_two_segments_and_spike's (d_qk = d,
    d_v = d / 2, 13 further keys, one huge score late in the key sequence).  Result [B, heads, d_v, L]."""
    if kind == "mha":
        qkv = seeded_randn(B, 3 * heads * d, L, seed=16)
        q, k, v = qkv.chunk(3, dim=1)
        t = dict(q=q.contiguous(), k=k.contiguous(), v=v.contiguous(), k2=None, v2=None)
        dv, L2 = d, 0
    else:
        dv, L2 = d // 2, 13
        t = dict(q=seeded_randn(B, heads * d, L, seed=17), k=seeded_randn(B, heads * d, L, seed=18),
                 v=seeded_randn(B, heads * dv, L, seed=19), k2=seeded_randn(B, heads * d, L2, seed=20),
                 v2=seeded_randn(B, heads * dv, L2, seed=21))
        t["k"][:, :, 170] = t["q"][:, :, 5] * 3.0
    scale = d ** -0.5

    def fn(c):
        qh = c["q"].reshape(B, heads, d, L)
        kh, vh = c["k"].reshape(B, heads, d, L), c["v"].reshape(B, heads, dv, L)
        if L2:
            kh = torch.cat([kh, c["k2"].reshape(B, heads, d, L2)], -1)
            vh = torch.cat([vh, c["v2"].reshape(B, heads, dv, L2)], -1)
        s = torch.einsum("bhct,bhcs->bhts", qh, kh) * scale
        return torch.einsum("bhts,bhcs->bhct", s.softmax(-1), vh)

    case = Case(t, fn)
    case.scale, case.dv = scale, dv
    return case


ATTN_KEEPS = ((3,), (0, 1), (2,))        # query position, (sample, head), value channel of [B, heads, d_v, L]


def na_ref(q, k, v, heads, h, w, kh, kw):
    """Clamped-H, circular-W neighbourhood attention in the dtype of q; q, k, v [B, heads * d, h * w] -> the same."""
    B, C, L = q.shape
    d = C // heads
    r0 = (torch.arange(h) - kh // 2).clamp(0, h - kh)
    rows = r0[:, None] + torch.arange(kh)[None]
    cols = (torch.arange(w)[:, None] - kw // 2 + torch.arange(kw)[None]) % w
    key = (rows[:, None, :, None] * w + cols[None, :, None, :]).reshape(L, kh * kw)
    f = lambda t: t.reshape(B, heads, d, L)
    qd, kd, vd = f(q), f(k), f(v)
    kg, vg = kd[..., key], vd[..., key]
    s = torch.einsum("bhdl,bhdln->bhln", qd, kg)
    return torch.einsum("bhln,bhdln->bhdl", s.softmax(-1), vg).reshape(B, C, L)


NA_HEADS, NA_B = 3, 2


@functools.lru_cache(maxsize=None)
def na_case(grid, d, backward=False):
    """test_neighbourhood_attention_against_float64's operands (q * 3: sharper scores).  backward: (o, dq, dk, dv)."""
    h, w, kh, kw = grid
    C, L = NA_HEADS * d, h * w
    qkv = seeded_randn(NA_B, 3 * C, L, seed=800 + d + h * w + kh)
    t = dict(q=qkv[:, :C] * 3.0, k=qkv[:, C:2 * C].contiguous(), v=qkv[:, 2 * C:].contiguous(),
             do=seeded_randn(NA_B, C, L, seed=900 + d + h * w))
    if not backward:
        return Case(t, lambda c: na_ref(c["q"], c["k"], c["v"], NA_HEADS, h, w, kh, kw))

    def fn(c):
        with torch.enable_grad():
            ts = [c[n].clone().requires_grad_() for n in ("q", "k", "v")]
            o = na_ref(*ts, NA_HEADS, h, w, kh, kw)
            o.backward(c["do"])
        return (o.detach(),) + tuple(x.grad for x in ts)

    return Case(t, fn)


def na_view(y, grid):
    """[B, heads * d, h * w] -> [B, heads, d, h, w]: axes 3 = grid row, 4 = grid column, 1 = head."""
    return y.reshape(NA_B, NA_HEADS, -1, grid[0], grid[1])


NA_KEEPS = ((3,), (4,), (1,))


@functools.lru_cache(maxsize=None)
def skinny_case(M, K, N):
    """test_skinny_linear_against_float64's operands: relu(x W^T + b) + vec[idx] + res."""
    t = dict(x=seeded_randn(M, K, seed=1), w=seeded_randn(N, K, seed=2) / K ** 0.5, b=seeded_randn(N, seed=3),
             res=seeded_randn(M, N + 8, seed=4), vec=seeded_randn(3, N, seed=5), vidx=(torch.arange(M) % 3).to(torch.int32))
    return Case(t, lambda c: torch.relu(c["x"] @ c["w"].t() + c["b"]) + c["vec"][c["vidx"].long()] + c["res"][:, 8:])


@functools.lru_cache(maxsize=None)
def skinny_geglu_case():
    """test_skinny_linear_gathered_segments_and_geglu's operands: three gathered segments, GEGLU."""
    O, T = 9, 23
    t = dict(obj=seeded_randn(O, 768, seed=1), pred=seeded_randn(T, 128 + 5, seed=2), w=seeded_randn(512, 1664, seed=3) / 40,
             s=(torch.arange(T) * 7 % O).to(torch.int32), o=(torch.arange(T) * 5 % O).to(torch.int32))

    def fn(c):
        x = torch.cat([c["obj"][c["s"].long()], c["pred"][:, 5:], c["obj"][c["o"].long()]], 1)
        a, g = (x @ c["w"].t()).chunk(2, dim=-1)
        return a * F.gelu(g)

    return Case(t, fn)


@functools.lru_cache(maxsize=None)
def rowprep_case(M, C, G):
    """test_rowprep_against_float64's operands: SiLU(GroupNorm(cat of two gathered segments))."""
    t = dict(a=seeded_randn(M, C // 2, seed=1) * 3 + 1, b=seeded_randn(M, C // 2 + 4, seed=2),
             ga=1 + 0.1 * seeded_randn(C, seed=3), be=0.1 * seeded_randn(C, seed=4))

    def fn(c):
        x = torch.cat([c["a"], c["b"][:, 4:]], 1)
        return F.silu(F.group_norm(x[:, :, None], G, c["ga"], c["be"], 1e-5)[:, :, 0])

    return Case(t, fn)


SKINNY_KEEPS = ((0,), (1,))              # row, output column


@functools.lru_cache(maxsize=None)
def conv_bwd_case(shape):
    """test_conv_gradients's operands -> (dx, dw)."""
    B, Ci, Co, H, W, ks = shape
    D = _D()
    t = dict(x=seeded_randn(B, Ci, H, W, seed=1), w=seeded_randn(Co, Ci, ks, ks, seed=2) / (Ci * ks * ks) ** 0.5,
             b=seeded_randn(Co, seed=3), g=seeded_randn(B, Co, H, W, seed=4))

    def fn(c):
        with torch.enable_grad():
            x, w = c["x"].clone().requires_grad_(), c["w"].clone().requires_grad_()
            D.conv_ring(x, w, c["b"]).backward(c["g"])
        return x.grad, w.grad

    return Case(t, fn)


DX_KEEPS = ((2,), (3,), (1,))            # row, column, channel of dx [B, Ci, H, W]
DW_KEEPS = ((2, 3), (0,), (1,))          # tap, output channel, input channel of dw [Co, Ci, 3, 3]


@functools.lru_cache(maxsize=None)
def attn_bwd_case():
    """test_flash_attention_gradients's operands -> (o, dq, dk, dv), each [B, heads, d, L]."""
    B, h, dqk, dv, Lq, Lk = ATTN_BWD_CASE
    t = dict(q=seeded_randn(B, h, dqk, Lq, seed=501) * 1.7, k=seeded_randn(B, h, dqk, Lk, seed=502) * 1.3,
             v=seeded_randn(B, h, dv, Lk, seed=503), g=seeded_randn(B, h, dv, Lq, seed=504) * (3e-5 if (B + h) % 2 else 40.0))
    scale = dqk ** -0.5

    def fn(c):
        with torch.enable_grad():
            ts = [c[n].clone().requires_grad_() for n in ("q", "k", "v")]
            p = (torch.einsum("bhct,bhcs->bhts", ts[0], ts[1]) * scale).softmax(-1)
            o = torch.einsum("bhts,bhcs->bhct", p, ts[2])
            o.backward(c["g"])
        return (o.detach(),) + tuple(x.grad for x in ts)

    case = Case(t, fn)
    case.scale = scale
    return case


@functools.lru_cache(maxsize=None)
def gn_bwd_case():
    """test_groupnorm_gradients's operands (AdaGN + SiLU) -> dx."""
    B, C, H, W, G = GN_BWD_SHAPE
    t = dict(x=seeded_randn(B, C, H, W, seed=11) * 2 + 0.3, g=seeded_randn(B, C, H, W, seed=12),
             scale=0.3 * seeded_randn(B, C, seed=15), shift=0.3 * seeded_randn(B, C, seed=16))

    def fn(c):
        D = _D()
        with torch.enable_grad():
            x = c["x"].clone().requires_grad_()
            y = D.group_norm(x, G, None, None, 1e-6) * (1 + c["scale"][:, :, None, None]) + c["shift"][:, :, None, None]
            D.silu(y).backward(c["g"])
        return x.grad

    return Case(t, fn)


def host_cases():
    """Every (name, thunk) of the lists above, thunk() -> (ref32, ref64, keeps, tol): what the CPU file checks the
    reference alone on.  The references are evaluated when a thunk is called, not when the names are listed."""
    out = []

    def add(name, case, pick, keeps, tol, view=None):
        def thunk():
            a, b = pick(case.ref32), pick(case.ref64)
            return (view(a), view(b), keeps, tol) if view else (a, b, keeps, tol)
        out.append((name, thunk))

    whole = lambda r: r
    item = lambda i: (lambda r: r[i])
    attn_tol = existing_lists()["attn_tol"]
    for s in CONV_SHAPES:
        for mode, tol in (("plain", TOL_CONV), ("gn", TOL_CONV_GN)):
            add(f"conv-{mode}-{s}", conv_case(s, mode), whole, NCHW_KEEPS, tol)
    for s in FOLD_SHAPES:
        add(f"fold-down-{s}", fold_case(s, "down"), whole, NCHW_KEEPS, TOL_FOLD)
        add(f"fold-up-{s}", fold_case(s, "up"), item(0), NCHW_KEEPS, TOL_FOLD)
        add(f"fold-up-xup-{s}", fold_case(s, "up"), item(1), NCHW_KEEPS, TOL_RESAMPLE)
    for s in RESAMPLE_SHAPES:
        for up in (True, False):
            add(f"resample-{'up' if up else 'down'}-{s}", resample_case(s, up), whole, ((2,), (3,)), TOL_RESAMPLE)
    for s in GN_SHAPES:
        add(f"gn-{s}", gn_case(s), whole, GN_KEEPS, TOL_GN, lambda y, G=s[4]: gn_views(y, G))
        add(f"gn-channel-{s}", gn_case(s), whole, ((1,),), TOL_GN)
    add("gn-large-mean", gn_large_mean_case(), whole, GN_KEEPS, TOL_GN_LARGE_MEAN, lambda y: gn_views(y, 8))
    for a in ATTN_CASES + [ATTN_UNITS_CASE]:
        add(f"attn-{a}", attn_case(*a), whole, ATTN_KEEPS, attn_tol["f32"])
    for g in NA_GRIDS:
        for d in NA_D:
            add(f"na-{g}-{d}", na_case(g, d), whole, NA_KEEPS, TOL_NA, lambda y, g=g: na_view(y, g))
            for i, n in ((1, "dq"), (2, "dk"), (3, "dv")):
                add(f"na-{n}-{g}-{d}", na_case(g, d, True), item(i), NA_KEEPS[:2], TOL_NA_BWD, lambda y, g=g: na_view(y, g))
    for s in SKINNY_CASES:
        add(f"skinny-{s}", skinny_case(*s), whole, SKINNY_KEEPS, TOL_SKINNY)
    add("skinny-geglu", skinny_geglu_case(), whole, SKINNY_KEEPS, TOL_SKINNY)
    add("rowprep", rowprep_case(37, 1024, 32), whole, SKINNY_KEEPS, TOL_SKINNY)
    for s in CONV_BWD_SHAPES:
        add(f"conv-dx-{s}", conv_bwd_case(s), item(0), DX_KEEPS, TOL_CONV_BWD)
        add(f"conv-dw-{s}", conv_bwd_case(s), item(1), DW_KEEPS, TOL_CONV_BWD)
    for i, n in ((1, "dq"), (2, "dk"), (3, "dv")):
        add(f"attn-{n}", attn_bwd_case(), item(i), ((3,),), TOL_ATTN_BWD)
    G = GN_BWD_SHAPE[4]
    add("gn-dx", gn_bwd_case(), whole, ((0, 1),), TOL_GN_BWD, lambda y: gn_views(y, G))
    return out
