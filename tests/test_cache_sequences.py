"""Call sequences through everything that outlives a call: the step graphs a sampler keeps (continuous_time.py::
_GRAPH_CACHES), the condition buffer of a cache entry, the operand graph of LayoutUnetV1 (`_prep`), the core graph and the
patch-embedding cache of the layout encoder.  A result must not depend on which calls came before it.

The yardstick is always the cache-free path (`graph_cache_size = 0`, `layout_unet_v1.PREPARE_GRAPH = False`,
`layout_encoder.CORE_GRAPH = False`: what the golden tests of rounds 1-5 pin on the reference), on a freshly built model
wherever weights moved; every comparison is `torch.equal`.  The named tests hold one finding each; the seeded walks at the
end drive three samplers through random orders of every operation a caller has.  `pytest -m gpu` (one CPU test checks
that the walks leave no operation out)."""
import contextlib
import copy
import gc
import random

import pytest
import torch

from lidarcrafter_amd.testing import seeded_fill, seeded_randn, synth_layout_batch, synth_object_batch, synth_text_features

gpu = pytest.mark.gpu
STEPS = 5
KINDS = ("uncond", "layout", "object")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _gens(n, seed):
    return [torch.Generator().manual_seed(seed + i) for i in range(n)]


@contextlib.contextmanager
def _caches(on):
    """The operand graph and the encoder-core graph on or off (module switches); the step graphs follow the sampler's
    own `graph_cache_size`."""
    import lidargen.models.unets.layout_encoder as LE
    import lidargen.models.unets.layout_unet_v1 as LU

    old = LU.PREPARE_GRAPH, LE.CORE_GRAPH
    LU.PREPARE_GRAPH = LE.CORE_GRAPH = bool(on)
    try:
        yield
    finally:
        LU.PREPARE_GRAPH, LE.CORE_GRAPH = old


def _build(kind, dev, base=0, cached=True):
    """The small samplers of tests/test_graph_cache.py; `base` picks one of two seeded weight states."""
    if kind == "uncond":
        from lidargen.models.diffusion import ContinuousTimeGaussianDiffusion
        from tests.test_hip_parity import _uncond

        m = _uncond(16, (8, 64), dev)
        if base:
            seeded_fill(m, salt=100 + 10 * base)
        ddpm = ContinuousTimeGaussianDiffusion(m, torch.nn.Identity())
    elif kind == "layout":
        from lidargen.models.diffusion import CondContinuousTimeGaussianDiffusion
        from tests.test_oracle_vs_golden import build_cond_pair

        m, enc = build_cond_pair((8, 64), 8, 32)
        if base:
            seeded_fill(m, salt=200 + 10 * base), seeded_fill(enc, salt=201 + 10 * base)
        ddpm = CondContinuousTimeGaussianDiffusion(m, enc, cond_mode="concat")
    else:
        from lidargen.utils import inference
        from lidargen.utils.configs import __all__ as C

        ddpm, model = inference.load_model_object_duffusion_training(C["nuscenes-object"]())
        seeded_fill(model, salt=300 + 10 * base), seeded_fill(ddpm.condition_model, salt=301 + 10 * base)
    ddpm = ddpm.eval().to(dev)
    if kind == "object":
        ddpm.condition_model.set_text_features(synth_text_features(), dev)
    ddpm.graph_cache_size = 4 if cached else 0
    return ddpm


def _batch(kind, i, B, dev):
    """Condition i at batch size B (None for the unconditional sampler, where i only picks the noise)."""
    if kind == "uncond":
        return None
    if kind == "layout":
        b = {k: v.to(dev) for k, v in synth_layout_batch(B, 8, 64, seed=51 + 6 * i).items()}
        b["concat_cond"] = torch.randn(B, 10, 8, 64, generator=torch.Generator().manual_seed(51 + 6 * i)).to(dev)
        return b
    return {k: v.to(dev) for k, v in synth_object_batch(B, seed=95 + 2 * i).items()}


def _sample(ddpm, batch, B, mode, seed, steps=STEPS):
    if batch is None:
        return ddpm.sample(B, steps, progress=False, rng=_gens(B, seed), mode=mode)
    return ddpm.sample(dict(batch), B, steps, progress=False, rng=_gens(B, seed), mode=mode)


def _precompute(ddpm, batch):
    if batch is None:
        return None
    with torch.inference_mode():
        return ddpm.get_network_condition(input_dict=batch, only_custom_condition=True)


def _stepwise(ddpm, cdict, B, mode, seed, steps=STEPS):
    """The run `sample()` makes, through begin_sampling / sampling_step with a condition dict computed beforehand."""
    with torch.inference_mode():
        rng = _gens(B, seed)
        x_T = ddpm.randn(B, *ddpm.sampling_shape, rng=rng, device=ddpm.device)
        st = ddpm.begin_sampling(B, steps, rng, mode, 0.0, x_T=x_T, condition_dict=cdict)
        for _ in range(steps):
            ddpm.sampling_step(st)
        ddpm.finish_sampling(st)
        return st["x"].clone()


def _forward(ddpm, batch, B, seed):
    """One denoiser forward on a condition computed in the caller's mode (the caller sets no_grad / inference mode)."""
    x = seeded_randn(B, *ddpm.sampling_shape, seed=seed).to(ddpm.device)
    lam = torch.linspace(-3.0, 2.5, B).to(ddpm.device)
    if batch is None:
        return ddpm.model(x, lam).clone()
    return ddpm.model(x, {"time_condition": lam, "other_condition": ddpm.condition_model(dict(batch))}).clone()


class _Captures:
    def __init__(self, ddpm):
        self.n = 0
        inner = ddpm._capture

        def counted(st):
            self.n += 1
            return inner(st)

        ddpm._capture = counted


# ------------------------------------------------------------------ finding 1: the condition buffer of a cache entry
@gpu
def test_tensor_condition_dicts_survive_any_order(dev):
    """Two precomputed TENSOR conditions (object branch) in the order A, B, A, B, B, A: each run samples under its own
    condition, and the caller's dicts keep their tensors -- same object, same address, same values.  (The entry's buffer
    used to be assigned into the caller's dict: after a run with B, dict A named a buffer holding B.)"""
    ddpm = _build("object", dev)
    B, order = 3, (0, 1, 0, 1, 1, 0)
    batches = [_batch("object", i, B, dev) for i in (0, 1)]
    with _caches(False):
        ddpm.graph_cache_size = 0
        ref_step = [_stepwise(ddpm, _precompute(ddpm, b), B, "ddpm", 600) for b in batches]
        ref_sample = [_sample(ddpm, b, B, "ddpm", 600) for b in batches]
    assert not torch.equal(ref_step[0], ref_step[1])
    ddpm.graph_cache_size = 4
    conds = [_precompute(ddpm, b) for b in batches]
    assert all(isinstance(c["other_condition"], torch.Tensor) for c in conds)
    held = [(c["other_condition"], c["other_condition"].data_ptr(), c["other_condition"].clone()) for c in conds]
    problems = []
    for n, i in enumerate(order):
        if not torch.equal(_stepwise(ddpm, conds[i], B, "ddpm", 600), ref_step[i]):
            problems.append(f"run {n} (condition {'AB'[i]}): not the cache-free sample of that condition")
        for j, (c, (t, ptr, val)) in enumerate(zip(conds, held)):
            now = c["other_condition"]
            if now is not t or now.data_ptr() != ptr or not torch.equal(now, val):
                problems.append(f"after run {n}: the caller's dict {'AB'[j]} no longer holds its own condition tensor")
    assert not problems, "\n".join(problems)
    # the same order through sample(): caller-owned batch dicts
    snap = [{k: (v, v.data_ptr(), v.clone()) for k, v in b.items()} for b in batches]
    for n, i in enumerate(order):
        assert torch.equal(ddpm.sample(batches[i], B, STEPS, progress=False, rng=_gens(B, 600), mode="ddpm"),
                           ref_sample[i]), (n, i)
        for b, s in zip(batches, snap):
            assert set(b) == set(s)
            assert all(b[k] is t and b[k].data_ptr() == p and torch.equal(b[k], v) for k, (t, p, v) in s.items())


# ------------------------------------------------------------------ finding 2: the operand graph's destinations
@gpu
@pytest.mark.parametrize("between", ["no_grad_forward", "other_batch_size", "inpaint"])
def test_operand_graph_follows_replaced_condition_cache(dev, between):
    """sample(A), sample(B), sample(A): the operand graph exists and writes to the addresses of the layers' operand tensors.  Then
    a call that gives the layers other tensors; then prepare_condition(D): the layers must hold D's operands (the graph
    used to be replayed into the tensors of before, the layers kept what they saw last).  Only tensors the layers hold
    are read, and the operands of before are kept alive here, so nothing depends on freed memory."""
    ddpm = _build("layout", dev)
    with _caches(True):
        _sample(ddpm, _batch("layout", 0, 2, dev), 2, "ddim", 0)
        _sample(ddpm, _batch("layout", 1, 2, dev), 2, "ddim", 0)
        _sample(ddpm, _batch("layout", 0, 2, dev), 2, "ddim", 0)     # (the route signature settles in a model's first run,
        assert ddpm.model._prep["graph"]                             #  so the graph is captured at the third condition)
        before = list(ddpm.model.graph_operands())               # kept alive until the end of the test
        if between == "no_grad_forward":
            with torch.no_grad():
                _forward(ddpm, _batch("layout", 2, 2, dev), 2, 9)
        elif between == "other_batch_size":
            _sample(ddpm, _batch("layout", 2, 3, dev), 3, "ddim", 0)
        else:
            known = seeded_randn(3, 2, 8, 64, seed=5).clamp(-1, 1).to(dev)
            mask = (seeded_randn(3, 1, 8, 64, seed=6) > 0).float().to(dev).expand(3, 2, 8, 64)
            ddpm.inpaint(known, mask, _batch("layout", 2, 3, dev), 3, progress=False, rng=_gens(3, 0))
        D = _batch("layout", 3, 2, dev)
        with torch.inference_mode():
            ddpm.model.prepare_condition(ddpm.get_network_condition(input_dict=D, only_custom_condition=True)["other_condition"])
            got = [t.clone() for t in ddpm.model.graph_operands()]
        got_x = _sample(ddpm, D, 2, "ddim", 3)
    with _caches(False):
        fresh = _build("layout", dev, cached=False)
        with torch.inference_mode():
            fresh.model.prepare_condition(fresh.get_network_condition(input_dict=D, only_custom_condition=True)["other_condition"])
            want = [t.clone() for t in fresh.model.graph_operands()]
        want_x = _sample(fresh, D, 2, "ddim", 3)
    assert len(got) == len(want) and len(before) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), f"operand {n} of graph_operands() is not the operand of condition D"
    assert torch.equal(got_x, want_x)


# ------------------------------------------------------------------ finding 3: training after sampling
@gpu
@pytest.mark.parametrize("B", [1, 2])
def test_training_step_after_sampling_with_frozen_patch_embedding(dev, B):
    """sample() in eval mode, then train() with `obj_bbox_2d_embedding` frozen and one loss.backward(): no exception (the
    patch embedding cached inside sample() is an inference tensor, which autograd refuses to save), every gradient equal
    to that of a model that never sampled (dropout and the noise draw are seeded; the backward kernels are deterministic),
    and the sample after the step equal to that of a fresh model with the stepped weights.  Batch size 1 is the case that
    raised: there the encoder's stride-0 batch view of the kept tensor is contiguous, so the training graph saves the kept
    tensor itself; from batch size 2 on it saves a copy."""
    A = _batch("layout", 0, B, dev)
    item = dict(_batch("layout", 1, B, dev))
    item["x_0"] = seeded_randn(B, 2, 8, 64, seed=35).clamp(-1, 1).to(dev)

    def step(ddpm):
        ddpm.train()
        for p in ddpm.condition_model.obj_bbox_2d_embedding.parameters():
            p.requires_grad_(False)
        torch.manual_seed(7)
        loss = ddpm(dict(item))
        loss.backward()
        grads = {k: None if p.grad is None else p.grad.clone() for k, p in ddpm.named_parameters()}
        with torch.no_grad():
            for p in ddpm.parameters():
                if p.grad is not None:
                    p.add_(p.grad, alpha=-1e-2)
        ddpm.eval()
        return loss.detach().clone(), grads

    with _caches(True):
        ddpm = _build("layout", dev)
        _sample(ddpm, A, B, "ddim", 0)
        loss, grads = step(ddpm)
        after = _sample(ddpm, A, B, "ddim", 0)
    with _caches(False):
        fresh = _build("layout", dev, cached=False)
        loss_f, grads_f = step(fresh)
        after_f = _sample(fresh, A, B, "ddim", 0)
        untouched = _sample(_build("layout", dev, cached=False), A, B, "ddim", 0)
    assert torch.equal(loss, loss_f)
    assert set(grads) == set(grads_f) and sum(g is not None for g in grads.values()) > 200
    for k, g in grads.items():
        assert (g is None) == (grads_f[k] is None), k
        assert g is None or torch.equal(g, grads_f[k]), k
    assert torch.equal(after, after_f) and not torch.equal(after, untouched)


# ------------------------------------------------------------------ finding 4: bounded and droppable graphs
@gpu
@pytest.mark.parametrize("kind", ["uncond", "layout"])
def test_graphs_are_bounded_and_droppable(dev, kind):
    """Batch sizes 1-6 in both modes on one sampler: never more than `graph_cache_size` entries, an evicted key captures
    again and gives the cache-free result, and after clear_graph_cache() the sampler holds no more device memory than
    after the same runs without any cache (measured here, in the same process state)."""
    from lidargen.models.diffusion import continuous_time as CT

    seq = [(B, mode) for B in range(1, 7) for mode in ("ddim", "ddpm")] + [(1, "ddim")]
    batches = {B: _batch(kind, B % 3, B, dev) for B in range(1, 7)}
    ddpm = _build(kind, dev, cached=False)

    def settle():
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.memory_allocated()

    with _caches(False):
        ref = [_sample(ddpm, batches[B], B, mode, 40 + B).cpu() for B, mode in seq]
        bound = settle()
    with _caches(True):
        ddpm.graph_cache_size = 4
        cap = _Captures(ddpm)
        for n, (B, mode) in enumerate(seq):
            before = cap.n
            got = _sample(ddpm, batches[B], B, mode, 40 + B).cpu()
            assert torch.equal(got, ref[n]), (B, mode)
            assert cap.n == before + 1, (B, mode)             # every key new, the last one evicted long ago: a capture
            assert 1 <= len(CT._GRAPH_CACHES[ddpm]) <= ddpm.graph_cache_size
            del got
        held = settle()
        ddpm.clear_graph_cache()
        assert not CT._GRAPH_CACHES.get(ddpm) and ddpm.model.__dict__.get("_prep") is None
        assert getattr(ddpm.condition_model, "__dict__", {}).get("_core_graph") is None
        freed = settle()
        print(f"{kind}: allocated {held} B with 4 step graphs, {freed} B after clear_graph_cache(), {bound} B cache-free")
        assert freed <= bound, (freed, bound)
        assert torch.equal(_sample(ddpm, batches[2], 2, "ddim", 42).cpu(), ref[2])     # and it captures again


# ------------------------------------------------------------------ copies with warm caches
@gpu
@pytest.mark.parametrize("kind", ["layout", "object"])
def test_conditioned_sampler_copies_with_warm_caches(dev, kind):
    """copy.deepcopy of a conditioned sampler whose step graphs (and, for the layout model, `_prep` and the encoder's
    core graph) exist: twin and original alternate, each keeps giving the cache-free result."""
    from lidargen.models.diffusion import continuous_time as CT

    B = 2
    batches = [_batch(kind, i, B, dev) for i in (0, 1)]
    with _caches(False):
        fresh = _build(kind, dev, cached=False)
        ref = [_sample(fresh, b, B, "ddim", 11) for b in batches]
    assert not torch.equal(ref[0], ref[1])
    with _caches(True):
        ddpm = _build(kind, dev)
        for i in (0, 1, 1):
            assert torch.equal(_sample(ddpm, batches[i], B, "ddim", 11), ref[i])
        assert CT._GRAPH_CACHES.get(ddpm)
        if kind == "layout":
            assert ddpm.model._prep["graph"] and ddpm.condition_model._core_graph["graph"]
        twin = copy.deepcopy(ddpm)
        assert torch.equal(_sample(twin, batches[0], B, "ddim", 11), ref[0])
        for rnd in range(3):
            for who, i in ((twin, rnd % 2), (ddpm, 1 - rnd % 2), (twin, 1 - rnd % 2), (ddpm, rnd % 2)):
                assert torch.equal(_sample(who, batches[i], B, "ddim", 11), ref[i]), (rnd, who is twin, i)


# ------------------------------------------------------------------ seeded random walks
# name -> weight in the draw.  Every name applies to every sampler except where dropped below, by name.
_OPS = {"sample": 5, "stepwise": 5, "no_grad_forward": 2, "inference_forward": 2, "deepcopy": 1, "mul_denoiser": 1,
        "mul_condition": 1, "load_state_dict": 1}
OP_SETS = {
    # the unconditional sampler has no condition model: nothing for `mul_condition` to move (its `stepwise` runs carry no
    # dict, condition i picks the noise seed)
    "uncond": [n for n in _OPS if n != "mul_condition"],
    "layout": list(_OPS),
    "object": list(_OPS),
}
WALK_LEN = 48
WALK_SEEDS = {"uncond": (1, 2, 4), "layout": (1, 2, 3), "object": (1, 2, 4)}    # (picked by test_walks_cover_every_operation)


def make_walk(kind, seed, length=WALK_LEN):
    r = random.Random(f"{kind}-{seed}")
    names = OP_SETS[kind]
    ops = []
    for _ in range(length):
        name = r.choices(names, [_OPS[n] for n in names])[0]
        if name in ("sample", "stepwise"):
            ops.append((name, r.randrange(3), r.choice((1, 2)), r.choice(("ddim", "ddpm"))))
        elif name in ("no_grad_forward", "inference_forward"):
            ops.append((name, r.randrange(3), r.choice((1, 2))))
        elif name == "load_state_dict":
            ops.append((name, r.randrange(2)))
        else:
            ops.append((name,))
    return ops


def _weight_states(ops):
    """The weights each operation runs on: (seeded state, in-place scalings of a denoiser tensor, of a condition-model
    tensor) -- a host-side replay of the walk."""
    ws, out = (0, 0, 0), []
    for op in ops:
        if op[0] == "mul_denoiser":
            ws = (ws[0], ws[1] + 1, ws[2])
        elif op[0] == "mul_condition":
            ws = (ws[0], ws[1], ws[2] + 1)
        elif op[0] == "load_state_dict":
            ws = (op[1], 0, 0)
        out.append(ws)
    return out


def test_walks_cover_every_operation():
    """Host only: every walk is at least 40 operations long and holds every operation of its sampler's set, both batch
    sizes, both modes and all three conditions."""
    for kind in KINDS:
        assert len(set(WALK_SEEDS[kind])) == 3
        for seed in WALK_SEEDS[kind]:
            ops = make_walk(kind, seed)
            assert len(ops) >= 40 and ops == make_walk(kind, seed)
            assert {op[0] for op in ops} == set(OP_SETS[kind]), (kind, seed)
            runs = [op for op in ops if op[0] in ("sample", "stepwise")]
            assert {op[1] for op in runs} == {0, 1, 2} and {op[2] for op in runs} == {1, 2}
            assert {op[3] for op in runs} == {"ddim", "ddpm"}
            assert len(set(_weight_states(ops))) >= 3


def _mul_target(ddpm, which):
    if which == "denoiser":
        return next(p for p in ddpm.model.parameters() if p.dim() > 1)
    lin = getattr(ddpm.condition_model, "obj_bbox_2d_embedding", None)     # (behind the layout encoder's patch cache)
    return lin.weight if lin is not None else next(p for p in ddpm.condition_model.parameters() if p.dim() > 1)


def _scale(ddpm, which):
    with torch.no_grad():
        _mul_target(ddpm, which).mul_(1.25)


_STATE_DICTS = {}


def _state_dict(kind, dev, base):
    if (kind, base) not in _STATE_DICTS:
        _STATE_DICTS[kind, base] = {k: v.detach().clone() for k, v in _build(kind, dev, base).state_dict().items()}
    return _STATE_DICTS[kind, base]


_REFS = {}          # (kind, weight state, op) -> the cache-free result, shared by the walks of a sampler


def _run_op(kind, ddpm, op, dev, cdict=None):
    name, i, B = op[0], op[1], op[2]
    batch = _batch(kind, i, B, dev)
    if name == "sample":
        return _sample(ddpm, batch, B, op[3], 70 + i)
    if name == "stepwise":
        return _stepwise(ddpm, _precompute(ddpm, batch) if cdict is None else cdict, B, op[3], 70 + i)
    if name == "no_grad_forward":
        with torch.no_grad():
            return _forward(ddpm, batch, B, 80 + i)
    with torch.inference_mode():
        return _forward(ddpm, batch, B, 80 + i)


def _references(kind, dev, ops):
    """Every distinct (operation, weights) of the walk, once, with all caches off, on a model built for those weights."""
    todo = {}
    for op, ws in zip(ops, _weight_states(ops)):
        if len(op) >= 3 and (kind, ws, op) not in _REFS:
            todo.setdefault(ws, []).append(op)
    with _caches(False):
        for ws, wops in todo.items():
            ref = _build(kind, dev, ws[0], cached=False)
            for _ in range(ws[1]):
                _scale(ref, "denoiser")
            for _ in range(ws[2]):
                _scale(ref, "condition")
            for op in dict.fromkeys(wops):
                _REFS[kind, ws, op] = _run_op(kind, ref, op, dev)
    return {(ws, op): _REFS[kind, ws, op] for op, ws in zip(ops, _weight_states(ops)) if len(op) >= 3}


@gpu
@pytest.mark.parametrize("caches", ["on", "off"])
@pytest.mark.parametrize("seed_no", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_seeded_walk(dev, kind, seed_no, caches):
    """A seeded walk over every operation of the sampler's set with all caches on: each result equals the cache-free
    result of the same operation on the same weights.  `caches == "off"` runs the same walk with the caches off: the same
    verdict there says the reference table is right."""
    ops = make_walk(kind, WALK_SEEDS[kind][seed_no])
    states = _weight_states(ops)
    refs = _references(kind, dev, ops)
    on = caches == "on"
    seen = set()
    with _caches(on):
        cur = _build(kind, dev, cached=on)
        dicts = {}                                   # conditions computed once per (condition-model weights, i, B), reused
        for n, (op, ws) in enumerate(zip(ops, states)):
            trail = f"{kind} walk, seed {WALK_SEEDS[kind][seed_no]}, caches {caches}: failed at operation {n} of\n" + \
                "\n".join(f"  {j:2d} {o}" for j, o in enumerate(ops[:n + 1]))
            seen.add(op[0])
            if op[0] == "deepcopy":
                cur = copy.deepcopy(cur)             # on with the twin, the original is dropped
            elif op[0] == "mul_denoiser":
                _scale(cur, "denoiser")
            elif op[0] == "mul_condition":
                _scale(cur, "condition")
            elif op[0] == "load_state_dict":
                cur.load_state_dict(_state_dict(kind, dev, op[1]))
            else:
                cdict = None
                if op[0] == "stepwise" and kind != "uncond":
                    key = (ws[0], ws[2], op[1], op[2])
                    if key not in dicts:
                        dicts[key] = _precompute(cur, _batch(kind, op[1], op[2], dev))
                    cdict = dicts[key]
                got = _run_op(kind, cur, op, dev, cdict)
                assert got.shape == refs[ws, op].shape and torch.equal(got, refs[ws, op]), trail
    assert seen == set(OP_SETS[kind]), sorted(set(OP_SETS[kind]) - seen)
