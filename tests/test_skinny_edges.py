"""The skinny dense-layer kernels at their tile edges, K tails and segment seams.  `pytest -m gpu`.

csrc/layout_gen.hip (product + combine, rowprep, pool, time embedding) through lidarcrafter_amd.ops_skinny, row by row of
the tables in tests/_skinny_edges.py; tests/test_skinny_edges_host.py proves on the CPU that the tables reach every edge,
that the references are right and that a designed defect is 16 bounds.  Every output is a NaN-filled view between NaN guard
words (a NaN that survives inside an output, or a word that changes outside one, fails the row), the split-K workspace is
NaN before every call, once exactly sized and once three times oversized, and every figure is printed before it is
asserted (profiles/skinny_edges.txt)."""
import pytest
import torch

from tests import _skinny_edges as SE

pytestmark = pytest.mark.gpu
NAN = float("nan")
ids = lambda c: c.name


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _out(M, No, pad, dev):
    """A NaN-filled [M, No] output, a column slice of a [M, No + pad] tensor between NaN guards -> (view, intact())."""
    ld = No + pad
    v, buf = SE.guarded(M * ld, dev, NAN)
    full = v.view(M, ld)
    G = SE.GUARD

    def intact():
        return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + M * ld:]).all() and torch.isnan(full[:, No:]).all())

    return full[:, :No], intact


# ------------------------------------------------------------------------------------------------ skinny linear
def _lin_call(dev, c, t, nparts, oversize, last_row_alone=False):
    """One skinny_linear call on fresh NaN-filled buffers -> the output [M', No] (a clone).  `last_row_alone`: row M - 1
    as an operand of one row (plain segments sliced, gathered ones with a one-element index)."""
    from lidarcrafter_amd import ops_skinny as S

    K, No = SE.lin_K(c), SE.lin_No(c)
    lo, M = (c.M - 1, 1) if last_row_alone else (0, c.M)
    d = lambda a: a.to(dev)
    checks = []
    if c.out == "inplace":
        wide = K + No + 3
        v, buf = SE.guarded(M * wide, dev, NAN)
        full = v.view(M, wide)
        x = SE.gather_x(t["src"], t["idx"], c.segs, c.M)[lo:lo + M]
        full[:, :K] = d(x)
        segs, out = [(full, 0, K, None)], full[:, K:K + No]
        G = SE.GUARD
        checks.append(lambda: bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + M * wide:]).all() and
                                   torch.isnan(full[:, K + No:]).all() and torch.equal(full[:, :K].cpu(), x)))
    else:
        src = {k: d(a) for k, a in t["src"].items()}
        segs = []
        for j, s in enumerate(c.segs):
            if s.idx:
                segs.append((src[s.src], s.c0, s.w, d(t["idx"][j][lo:lo + M]).contiguous()))
            else:
                segs.append((src[s.src][lo:lo + M], s.c0, s.w, None))
        out, ok = _out(M, No, 5 if c.out == "pad" else 0, dev)
        checks.append(ok)
        checks.append(lambda: all(torch.equal(src[k].cpu().nan_to_num(7e7), t["src"][k].nan_to_num(7e7)) for k in src))
    size = nparts * M * c.N
    parts = torch.full((size * (3 if oversize else 1),), NAN, device=dev)
    vec = res = None
    if c.vec:
        vec = (d(t["vec"]), SE.VEC_C0, d(t["vidx"][lo:lo + M]).contiguous() if c.vec == "idx" else None)
    if c.res:
        res = (d(t["res"])[lo:lo + M], SE.RES_C0)
    S.skinny_linear(segs, M, d(t["w"]), d(t["bias"]) if c.bias else None, c.act, vec=vec, res=res, out=out, parts=parts, nparts=nparts)
    torch.cuda.synchronize()
    assert all(f() for f in checks), "a word outside the output was written, or an operand changed"
    assert bool(torch.isnan(parts[size:]).all()), "the workspace was written past nparts * M * N"
    assert not bool(torch.isnan(parts[:size]).any()), "a partial sum was never written"
    return out.clone()


@pytest.mark.parametrize("c,tier", SE.LIN_RUNS, ids=[f"{c.name}-{tier}" for c, tier in SE.LIN_RUNS])
def test_skinny_linear_row(dev, c, tier):
    r = SE.lin_ref(c, tier)
    K = SE.lin_K(c)
    route, nch = SE.lib_parts(c.M, c.N, K), SE.nchunks(K)
    assert route in (1, nch)
    other = nch if route == 1 else 1
    y = _lin_call(dev, c, r.t, route, oversize=False)
    y2 = _lin_call(dev, c, r.t, other, oversize=True)
    one = _lin_call(dev, c, r.t, route, oversize=True, last_row_alone=True)
    nan = int(torch.isnan(y).sum())
    if tier == "exact":
        want = r.y.float()
        wrong = int((y.cpu() != want).sum())
        print(f"skinny-edges linear {c.name} exact nparts={route} (chunks {nch}) wrong elements {wrong} of {want.numel()} "
              f"(NaN {nan}) ref32 0 bound 0")
        assert wrong == 0, "an element differs from the int64 evaluation"
    else:
        e = SE.elem_err(y, r.y, r.S)
        print(f"skinny-edges linear {c.name} round nparts={route} (chunks {nch}) worst {e:.3e} (NaN {nan}) ref32 {r.e32:.3e} "
              f"bound {r.bound:.3e}")
        assert nan == 0, "an element was never written, or a NaN column / row of an operand was read"
        assert e <= r.bound, (e, r.bound)
    assert torch.equal(y2, y), f"nparts = {other} with an oversized workspace gives other bits than nparts = {route}"
    assert torch.equal(one[0], y[c.M - 1]), "row M - 1 run alone gives other bits"


def test_skinny_linear_refusals(dev):
    from lidarcrafter_amd import ops_skinny as S
    from lidarcrafter_amd._lib import HipError

    x, w = torch.zeros(5, 300, device=dev), torch.zeros(7, 300, device=dev)
    seg = [(x, 0, 300, None)]
    with pytest.raises(HipError, match="lc_skinny_gemm_fwd: invalid argument"):
        S.skinny_linear(seg, 5, w, nparts=2)                                  # 3 chunks: 1 or 3
    with pytest.raises(HipError, match="lc_skinny_combine_fwd: invalid argument"):
        S.skinny_linear(seg, 5, w, act="geglu")                               # N = 7
    with pytest.raises(ValueError, match="workspace too small"):
        S.skinny_linear(seg, 5, w, parts=torch.zeros(3 * 5 * 7 - 1, device=dev), nparts=3)
    with pytest.raises(ValueError, match="out too small"):
        S.skinny_linear(seg, 5, w, out=torch.zeros(5, 6, device=dev))
    with pytest.raises(ValueError, match="out too small"):
        S.skinny_linear(seg, 5, w, out=torch.zeros(4, 7, device=dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ rowprep
def _row_call(dev, c, t, last_row_alone=False):
    from lidarcrafter_amd import ops_skinny as S

    lo, M = (c.M - 1, 1) if last_row_alone else (0, c.M)
    src = {k: a.to(dev) for k, a in t["src"].items()}
    segs = []
    for j, s in enumerate(c.segs):
        if s.idx:
            segs.append((src[s.src], s.c0, s.w, t["idx"][j][lo:lo + M].to(dev).contiguous()))
        else:
            segs.append((src[s.src][lo:lo + M], s.c0, s.w, None))
    C = SE.row_C(c)
    out, ok = _out(M, C, c.pad, dev)
    p = lambda k: None if t[k] is None else t[k].to(dev)
    S.rowprep(segs, M, c.G, SE.EPS, p("gamma"), p("beta"), c.silu, out=out)
    torch.cuda.synchronize()
    assert ok(), "a word outside the output was written"
    assert all(torch.equal(src[k].cpu().nan_to_num(7e7), t["src"][k].nan_to_num(7e7)) for k in src), "an operand changed"
    return out.clone()


@pytest.mark.parametrize("c", SE.ROW_CASES, ids=ids)
def test_rowprep_row(dev, c):
    r = SE.row_ref(c)
    y = _row_call(dev, c, r.t)
    one = _row_call(dev, c, r.t, last_row_alone=True)
    nan = int(torch.isnan(y).sum())
    e = float(SE.row_group_err(y, r.y, c).max())
    line = f"skinny-edges rowprep {c.name} G={c.G} C={SE.row_C(c)} worst {e:.3e} (NaN {nan}) ref32 {r.e32:.3e} bound {r.bound:.3e}"
    const = None
    if SE.row_is_const(c):
        closed, b = SE.row_const(c, r.t, r.x)
        dev_y = (y.double().cpu() - closed).abs()
        const = bool((dev_y <= b).all())
        line += f" constant groups: |y - closed| / bound {float((dev_y / b.clamp_min(1e-300)).max()):.2e}"
    same = torch.equal(y.cpu(), r.x) if (c.G == 0 and not c.silu) else None
    if same is not None:
        line += f" bit-equal to the gathered input: {same}"
    print(line)
    assert nan == 0, "an element was never written, or a NaN column / row of an operand was read"
    if const is not None:                                          # (only the closed form: see SE.row_ref)
        assert const, "a constant group is off its closed form silu?(beta)"
    else:
        assert e <= r.bound, (e, r.bound)
    if same is not None:
        assert same
    assert torch.equal(one[0], y[c.M - 1]), "row M - 1 run alone gives other bits"


def test_rowprep_refusals(dev):
    from lidarcrafter_amd import ops_skinny as S
    from lidarcrafter_amd._lib import HipError

    for name, C, G, _ in SE.ROW_REFUSED:
        x = torch.zeros(2, C, device=dev)
        with pytest.raises(HipError, match="lc_rowprep_fwd: unsupported shape"):
            S.rowprep([(x, 0, C, None)], 2, G)
    x, b = torch.zeros(2, 64, device=dev), torch.zeros(64, device=dev)
    with pytest.raises(ValueError, match="beta without gamma"):
        S.rowprep([(x, 0, 64, None)], 2, 4, beta=b)
    with pytest.raises(ValueError, match="out too small"):
        S.rowprep([(x, 0, 64, None)], 2, 4, out=torch.zeros(2, 63, device=dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("c", SE.POOL_CASES, ids=ids)
def test_graph_pool_row(dev, c):
    from lidarcrafter_amd import ops_skinny as S
    from lidargen.models.unets.graph import edge_csr

    t, s, o = SE.pool_operands(c)
    want = SE.pool_ref(t, s, o, c)
    row_ptr, slots = edge_csr(s, o, c.O)
    td = t.to(dev)
    out, ok = _out(c.O, c.H, c.pad, dev)
    S.graph_pool(td, c.s_col, c.o_col, c.H, row_ptr.to(dev), slots.to(dev), out=out)
    torch.cuda.synchronize()
    y = out.clone().cpu()
    wrong, nan = int((y != want).sum()), int(torch.isnan(y).sum())
    print(f"skinny-edges pool {c.name} O={c.O} H={c.H} t_ld={t.shape[1]} wrong elements {wrong} of {want.numel()} (NaN {nan}) "
          f"ref32 0 bound 0")
    assert ok(), "a word outside the output was written"
    assert torch.equal(td.cpu(), t), "the operand changed"
    assert wrong == 0, "an element differs from two sequential float32 scatter_add calls over the clamped count"
    if c.O > 1:
        assert torch.equal(y[2], torch.zeros(c.H)), "an object in no triple is not zero"


# ------------------------------------------------------------------------------------------------ time embedding
@pytest.mark.parametrize("c", SE.TIME_CASES, ids=ids)
def test_time_embed_row(dev, c):
    from lidarcrafter_amd import ops_skinny as S

    r = SE.time_ref(c)
    v, buf = SE.guarded(c.U * 2 * c.half, dev, NAN)
    out = v.view(c.U, 2 * c.half)
    S.time_embed(r.t.to(dev), r.f.to(dev), out=out)
    torch.cuda.synchronize()
    G, n = SE.GUARD, c.U * 2 * c.half
    y = out.clone().cpu()
    nan = int(torch.isnan(y).sum())
    e = float((y.double() - r.y).abs().nan_to_num(float("inf")).max())
    print(f"skinny-edges time-embed {c.name} U={c.U} half={c.half} worst {e:.3e} (NaN {nan}) ref32 {r.e32:.3e} bound {r.bound:.3e}")
    assert bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all()), "a word outside the output was written"
    assert nan == 0 and e <= r.bound, (e, r.bound)
