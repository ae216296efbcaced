"""Host logic of the graphs kept across runs (no GPU): the key under which a sampler may replay an earlier run's captured
step, the packing of a run's per-step parameters, the eligibility rules of the unit-form attention and the redirect of a
prepared condition to its static view.  The GPU side -- bit-equality with the uncached paths, capture counts -- is
tests/test_graph_cache.py."""
import torch

from lidarcrafter_amd import ops as K


def _sampler():
    from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion
    from lidargen.models.unets import EfficientUNet
    from lidargen.utils.lidar import get_linear_ray_angles

    m = EfficientUNet(2, (8, 64), base_channels=16, coords_encoding="fourier_features", num_residual_blocks=(1, 1, 1, 1),
                      gn_num_groups=8, gn_eps=1e-6, attn_num_heads=8, ring=True)
    m.coords = get_linear_ray_angles(8, 64, 10.0, -30.0)
    return ContinuousTimeGaussianDiffusion(m, torch.nn.Identity()).eval()


def _state(ddpm, B=2, S=5, tf=True):
    x = torch.zeros(B, 2, 8, 64)
    return dict(x=x, B=B, n=S, i=0, cond=None, needs_noise=False, obj=0, mid=1,
                lam=torch.arange(S * B, dtype=torch.float32).reshape(S, B),
                coef=torch.arange(S * B * 8, dtype=torch.float32).reshape(S, B, 8),
                tf=(torch.ones(S * B, 7), 2 * torch.ones(S * B, 10)) if tf else None)


def test_graph_key_names_what_a_captured_step_depends_on(monkeypatch):
    ddpm = _sampler()
    st = _state(ddpm)
    k0 = ddpm._graph_key(st)
    assert k0 == ddpm._graph_key(st) and hash(k0) is not None
    assert ddpm._graph_key(_state(ddpm, B=1)) != k0                                  # batch
    st2 = _state(ddpm)
    st2["needs_noise"] = True
    assert ddpm._graph_key(st2) != k0                                                 # DDPM / DDIM eta > 0: a noise operand
    st2 = _state(ddpm)
    st2["mid"] = 0
    assert ddpm._graph_key(st2) != k0                                                 # another update kernel
    assert ddpm._graph_key(_state(ddpm, tf=False)) != k0                              # time features hoisted or not
    assert ddpm._graph_key(_state(ddpm, S=9))[:2] == k0[:2]                           # the step count is NOT part of it
    monkeypatch.setattr(K, "PRODUCER_GN_STATS", not K.PRODUCER_GN_STATS)
    assert ddpm._graph_key(st) != k0                                                  # a routing switch of ops
    monkeypatch.undo()
    assert ddpm._graph_key(st) == k0
    with torch.no_grad():
        ddpm.model.in_conv.bias.add_(1.0)                                             # weights moved in place (optimizer step)
    assert ddpm._graph_key(st) != k0
    k1 = ddpm._graph_key(st)
    ddpm.model.in_conv.weight = torch.nn.Parameter(ddpm.model.in_conv.weight.detach().clone())   # a parameter REPLACED
    assert ddpm._graph_key(st) != k1
    # a condition the denoiser does not expose through graph_operands(): the run keeps its graph to itself
    st3 = _state(ddpm)
    st3["cond"] = {"other_condition": {"anything": torch.zeros(1)}}
    assert ddpm._graph_key(st3) is None
    st3["cond"] = {"other_condition": torch.zeros(2, 5)}                              # a tensor: kept in the entry's buffer
    assert ddpm._graph_key(st3) is not None and ddpm._graph_key(st3) != k0


def test_fingerprint_covers_every_parameter_and_buffer():
    ddpm = _sampler()
    fp = ddpm._weights_fingerprint()
    n = sum(1 for _ in ddpm.model.parameters()) + sum(1 for _ in ddpm.model.buffers())
    assert len(fp) == n and len(set(p for p, _ in fp)) == n                           # every tensor once, none shared


def test_pack_rows_layout():
    ddpm = _sampler()
    st = _state(ddpm, B=3, S=4)
    table, offs, widths, shapes = ddpm._pack_rows(st)
    assert widths == [3, 24, 21, 30] and all(o % 4 == 0 for o in offs)                # every view 16-byte aligned
    assert shapes == [(3,), (3, 8), (3, 7), (3, 10)]
    assert table.shape == (4, offs[-1] + 32)
    for i in range(4):
        assert torch.equal(table[i, offs[0]:offs[0] + 3], st["lam"][i])
        assert torch.equal(table[i, offs[1]:offs[1] + 24].view(3, 8), st["coef"][i])
        assert torch.equal(table[i, offs[2]:offs[2] + 21].view(3, 7), st["tf"][0][3 * i:3 * i + 3])
        assert torch.equal(table[i, offs[3]:offs[3] + 30].view(3, 10), st["tf"][1][3 * i:3 * i + 3])


def test_unit_form_eligibility():
    ok = K.AttnUnits.eligible
    assert ok(8, 2048, 13, 32, 32, 32) and ok(16, 512, 13, 32, 32, 32) and ok(4, 64, 0, 64, 0, 8) and ok(2, 128, 32, 40, 16, 24)
    assert not ok(8, 2000, 13, 32, 32, 32)          # image keys in whole 32-key tiles
    assert not ok(8, 2048, 33, 32, 32, 32)          # at most one further tile
    assert not ok(8, 2048, 13, 32, 32, 64)          # values: 32 channels per head
    assert not ok(8, 2048, 13, 20, 32, 32)          # channels in whole octets
    assert not ok(8, 2048, 13, 16, 16, 16)          # <= 32 q/k channels: the 32-channel kernel of attention.hip is the cheaper one
    assert K.qkv_units_ok(256, 8, 2048) and K.qkv_units_ok(512, 16, 512)
    assert not K.qkv_units_ok(192, 6, 512) and not K.qkv_units_ok(256, 4, 512) and not K.qkv_units_ok(256, 8, 500)


class _FakeGraph:
    def replay(self):
        pass


def _host_capture(ddpm, monkeypatch):
    """`_capture` without a device: the graph object and the capture context are stand-ins, the step body only records
    the condition dict it was given."""
    import contextlib

    seen = []
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", lambda g: contextlib.nullcontext())
    monkeypatch.setattr(ddpm, "_step_body", lambda st, lam, tf, coef, noise: seen.append(st["cond"]))
    return seen


def test_tensor_condition_never_assigned_into_the_callers_dict(monkeypatch):
    """A tensor condition lives in the cache entry's buffer: the run reads it through a dict of its own, the caller's
    dict keeps its tensor through a capture and through hits in the order A, B, A."""
    ddpm = _sampler()
    body = _host_capture(ddpm, monkeypatch)
    x = torch.zeros(2, 2, 8, 64)
    conds = [{"other_condition": torch.full((2, 5), float(v))} for v in (1, 2)]
    mine = [c["other_condition"] for c in conds]

    def state(c):
        st = _state(ddpm)
        st["x"], st["cond"] = x, c
        return st

    st = state(conds[0])
    g = ddpm._capture(st)
    assert conds[0]["other_condition"] is mine[0] and g["other"] is not mine[0] and torch.equal(g["other"], mine[0])
    assert st["cond"] is not conds[0] and st["cond"]["other_condition"] is g["other"] and body == [st["cond"]]
    assert conds[0]["time_condition"] is g["lam"]                   # what a step leaves in the caller's dict, as before
    ddpm._remember_graph(st, g)
    for i in (1, 0, 1, 1, 0):
        st = state(conds[i])
        hit = ddpm._cached_graph(st)
        assert hit is not None and hit["other"] is g["other"]
        assert torch.equal(g["other"], mine[i])                     # the buffer holds THIS run's condition
        assert st["cond"] is not conds[i] and st["cond"]["other_condition"] is g["other"]
        assert all(c["other_condition"] is t for c, t in zip(conds, mine))
        assert torch.equal(mine[0], torch.full((2, 5), 1.0)) and torch.equal(mine[1], torch.full((2, 5), 2.0))
        assert conds[i]["time_condition"] is g["lam"]


def test_remember_graph_evicts_the_least_recently_used(monkeypatch):
    from lidargen.models.diffusion import continuous_time as CT

    ddpm = _sampler()
    _host_capture(ddpm, monkeypatch)
    states = {B: _state(ddpm, B=B) for B in range(1, 8)}
    keys = {B: ddpm._graph_key(st) for B, st in states.items()}

    def remember(B):
        ddpm._remember_graph(states[B], ddpm._capture(states[B]))

    for B in (1, 2, 3, 4):
        remember(B)
    assert list(CT._GRAPH_CACHES[ddpm]) == [keys[B] for B in (1, 2, 3, 4)]
    remember(5)
    assert list(CT._GRAPH_CACHES[ddpm]) == [keys[B] for B in (2, 3, 4, 5)]           # the oldest goes
    assert ddpm._cached_graph(states[2]) is not None                                 # a hit makes an entry the newest
    remember(6)
    assert list(CT._GRAPH_CACHES[ddpm]) == [keys[B] for B in (4, 5, 2, 6)]
    assert ddpm._cached_graph(states[3]) is None and ddpm._cached_graph(states[1]) is None
    monkeypatch.setattr(ddpm, "graph_cache_size", 2)
    remember(7)
    assert list(CT._GRAPH_CACHES[ddpm]) == [keys[B] for B in (6, 7)]                 # a smaller bound holds at once
    monkeypatch.setattr(ddpm, "graph_cache_size", 0)
    remember(1)
    assert list(CT._GRAPH_CACHES[ddpm]) == [keys[B] for B in (6, 7)]                 # 0: nothing is kept


def test_clear_graph_cache_drops_every_graph():
    from lidargen.models.diffusion import continuous_time as CT

    ddpm = _sampler()
    CT._GRAPH_CACHES[ddpm] = {"key": {"graph": object()}}
    ddpm.model.__dict__["_prep"] = {"graph": object()}
    ddpm.condition_model.__dict__["_core_graph"] = {"graph": object()}
    ddpm.clear_graph_cache()
    assert not CT._GRAPH_CACHES.get(ddpm)
    assert ddpm.model.__dict__["_prep"] is None and ddpm.condition_model.__dict__["_core_graph"] is None
    ddpm.clear_graph_cache()                                                          # nothing kept: still fine
    bare = _sampler()
    bare.clear_graph_cache()
    assert "_prep" not in bare.model.__dict__ and bare not in CT._GRAPH_CACHES


def test_patch_embedding_tag_tells_inference_mode_from_grad_mode():
    """The kept patch embedding of a FROZEN `obj_bbox_2d_embedding`: the one made inside inference mode (a sampling run)
    is never handed to a caller in grad mode, who must be able to save it for backward."""
    from tests.test_oracle_vs_golden import build_cond_pair

    _, enc = build_cond_pair((8, 64), 8, 32)
    for p in enc.obj_bbox_2d_embedding.parameters():
        p.requires_grad_(False)
    key = "resolution2"
    assert key in enc.image_patch_bbox_embedding
    with torch.inference_mode():
        e_inf, tag_inf = enc._patch_embedding(key, torch.device("cpu"))
        assert enc._patch_embedding(key, torch.device("cpu"))[0] is e_inf            # kept within a mode
    e, tag = enc._patch_embedding(key, torch.device("cpu"))
    assert tag != tag_inf and tag[:-1] == tag_inf[:-1]
    assert e_inf.is_inference() and not e.is_inference() and torch.equal(e, e_inf)
    w = torch.ones(e.shape[0], 3, requires_grad=True)
    (e.t() @ w).sum().backward()                                                      # saved for backward: no complaint
    assert w.grad is not None
    assert enc._patch_embedding(key, torch.device("cpu"))[0] is e
    with torch.no_grad():
        enc.obj_bbox_2d_embedding.weight.mul_(2.0)
    assert enc._patch_embedding(key, torch.device("cpu"))[1] != tag                  # the weights moved


def test_operand_graph_targets_are_checked_by_identity():
    """LayoutUnetV1._holds_targets: the operand graph may be replayed only while every attention layer still holds the
    very tensors (and unit buffer) it held at capture."""
    from types import SimpleNamespace as NS

    from lidargen.models.unets.layout_unet_v1 import LayoutUnetV1 as U

    def layer(units=True):
        t = [torch.zeros(2) for _ in range(4)]
        return NS(_cond_cache=("key", *t, None, None, None, NS(buf=torch.zeros(3)) if units else None))

    layers = [layer(), layer(units=False)]
    dst = U._operand_targets(layers)
    assert [len(d) for d in dst] == [5, 5] and dst[1][4] is None
    assert U._holds_targets(layers, dst) and not U._holds_targets(layers, None)
    c = layers[0]._cond_cache
    layers[0]._cond_cache = c[:2] + (c[2].clone(),) + c[3:]                          # equal values, another tensor
    assert not U._holds_targets(layers, dst)
    layers[0]._cond_cache = c
    assert U._holds_targets(layers, dst)
    layers[0]._cond_cache = c[:8] + (NS(buf=torch.zeros(3)),)                        # another unit buffer
    assert not U._holds_targets(layers, dst)
    layers[0]._cond_cache = None                                                      # nothing prepared
    assert not U._holds_targets(layers, dst) and not U._holds_targets(layers, U._operand_targets(layers))


def test_static_condition_redirect():
    """LayoutUnetV1._static_condition: only THE condition prepare_condition last saw (same three tensors) is swapped for
    its static view; any other dict passes through untouched."""
    from lidargen.models.unets.layout_unet_v1 import LayoutUnetV1

    m = LayoutUnetV1.__new__(LayoutUnetV1)
    torch.nn.Module.__init__(m)
    keys = LayoutUnetV1._PREP_KEYS
    a = {k: torch.zeros(2, 4, 3) for k in keys}
    a["concat_cond"] = torch.zeros(1)
    assert m._static_condition(a) is a                                                # nothing prepared
    static = dict(a)
    static.update({k: torch.ones(2, 4, 3) for k in keys})
    m.__dict__["_prep"] = dict(lay=static, src=tuple(a[k] for k in keys),
                               src_id=tuple((a[k].data_ptr(), tuple(a[k].shape)) for k in keys))
    assert m._static_condition(a) is static and m._static_condition(dict(a)) is static
    b = {k: torch.zeros(2, 4, 3) for k in keys}
    assert m._static_condition(b) is b                                                # another condition
    assert m._static_condition({"xf_out": a["xf_out"]}) is not static                 # not a layout condition at all
