"""Scene-graph layout generator (nuscenes-layout) on the HIP path against tests/golden/layout_gen.npz (the reference's
outputs, made by tests/golden/make_layout_gen_fixtures.py) and against float64 evaluations of the single kernels.

Tolerances: everything that is a single forward -- the full denoiser, one module of it, the graph network, p_step from
fixed (x_t, noise), the eval-mode loss -- within 5e-6 relative L2 of the reference's float32 output (the project's fp32
parity bound) when the fixture's `ref_err_*`, the reference's own float32-vs-float64 deviation, is below 2.5e-6; otherwise
within twice that `ref_err` of the float64 twin (`near_reference`).  The recorded values are 7.4e-8 (loss) ... 1.04e-6
(per-scene forward), so the float32 branch applies to every item.  Trajectory states within the 1e-3 frame tolerance of
SURVEY.md §8d.
Kernels against float64: 2e-6 (a K = 2048 fp32 dot product in chunks of 128 carries about sqrt(K) * 2^-24 ~ 3e-6 worst
case per element, far less in L2 over random data).
Rows of different scenes: bit-equal, the kernels' summation order does not depend on M."""
import copy
import os

import numpy as np
import pytest
import torch

from lidarcrafter_amd.testing import (LAYOUT_GEN_VOCAB, rel_l2, seeded_fill, seeded_fill_layout_gen, seeded_randn,
                                      synth_scene_graph_batch)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_gen.npz")
SALT = 11
FWD_TOL, TRAJ_TOL, KERNEL_TOL = 5e-6, 1e-3, 2e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def build(salt=SALT):
    from lidargen.utils import inference
    from lidargen.utils.configs import __all__ as CONFIGS

    cfg = CONFIGS["nuscenes-layout"]()
    cfg.condition_model.params["vocab"] = LAYOUT_GEN_VOCAB
    d, _ = inference.load_model_layout_duffusion_training(cfg)
    seeded_fill(d, salt=salt)
    seeded_fill_layout_gen(d, salt=salt)
    return d.eval().cuda()


@pytest.fixture(scope="module")
def ddpm():
    return build()


def near_reference(gold, name, y):
    """The forward rule of this file's header; prints the figure before it asserts."""
    ref_err = float(gold["ref_err_" + name])
    if ref_err < 2.5e-6:
        r, bound, what = rel_l2(y, torch.from_numpy(gold[name])), FWD_TOL, "float32"
    else:
        r, bound, what = rel_l2(y, torch.from_numpy(gold[name + "_f64"])), 2 * ref_err, "float64"
    print(f"{name}: rel L2 vs reference {what} {r:.3e} (bound {bound:.1e}, ref_err {ref_err:.3e})")
    assert r < bound, (name, r, bound)


def gens(n, base):
    return [torch.Generator().manual_seed(base + i) for i in range(n)]


# ------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("M,K,N", [(1, 512, 512), (7, 20, 512), (37, 512, 20), (33, 1664, 256), (50, 2048, 11328),
                                   (300, 1536, 512), (3000, 256, 640), (5, 1280, 512), (64, 768, 1280)])
def test_skinny_linear_against_float64(M, K, N):
    from lidarcrafter_amd import ops_skinny as S

    x, w, b = seeded_randn(M, K, seed=1).cuda(), (seeded_randn(N, K, seed=2) / K ** 0.5).cuda(), seeded_randn(N, seed=3).cuda()
    res, vec = seeded_randn(M, N + 8, seed=4).cuda(), seeded_randn(3, N, seed=5).cuda()
    vidx = (torch.arange(M) % 3).to(torch.int32).cuda()
    y = S.skinny_linear([(x, 0, K, None)], M, w, b, "relu", vec=(vec, 0, vidx), res=(res, 8))
    want = torch.relu(x.double() @ w.double().t() + b.double()) + vec.double()[vidx.long()] + res.double()[:, 8:]
    assert rel_l2(y, want) < KERNEL_TOL
    # the split-K form and the single-block form give the same bits
    nchunks = (K + 127) // 128
    a = S.skinny_linear([(x, 0, K, None)], M, w, b, nparts=1)
    c = S.skinny_linear([(x, 0, K, None)], M, w, b, nparts=nchunks)
    assert torch.equal(a, c)
    # a row's result does not depend on how many rows there are
    one = S.skinny_linear([(x[M // 2:M // 2 + 1], 0, K, None)], 1, w, b)
    assert torch.equal(one[0], a[M // 2])


def test_skinny_linear_gathered_segments_and_geglu():
    from lidarcrafter_amd import ops_skinny as S

    O, T = 9, 23
    obj, pred = seeded_randn(O, 768, seed=1).cuda(), seeded_randn(T, 128 + 5, seed=2).cuda()
    s = (torch.arange(T) * 7 % O).to(torch.int32).cuda()
    o = (torch.arange(T) * 5 % O).to(torch.int32).cuda()
    w = (seeded_randn(512, 1664, seed=3) / 40).cuda()
    y = S.skinny_linear([(obj, 0, 768, s), (pred, 5, 128, None), (obj, 0, 768, o)], T, w, None, "geglu")
    x = torch.cat([obj[s.long()], pred[:, 5:], obj[o.long()]], 1).double()
    a, g = (x @ w.double().t()).chunk(2, dim=-1)
    assert y.shape == (T, 256) and rel_l2(y, a * torch.nn.functional.gelu(g)) < KERNEL_TOL


@pytest.mark.parametrize("M,C,G,silu", [(1, 512, 32, True), (37, 1024, 32, True), (5, 512, 1, False), (300, 512, 32, False),
                                         (3, 2048, 0, True)])
def test_rowprep_against_float64(M, C, G, silu):
    from lidarcrafter_amd import ops_skinny as S

    a, b = seeded_randn(M, C // 2, seed=1).cuda() * 3 + 1, seeded_randn(M, C // 2 + 4, seed=2).cuda()
    gamma, beta = (1 + 0.1 * seeded_randn(C, seed=3)).cuda(), (0.1 * seeded_randn(C, seed=4)).cuda()
    y = S.rowprep([(a, 0, C // 2, None), (b, 4, C // 2, None)], M, G, 1e-5, gamma if G else None, beta if G else None, silu)
    x = torch.cat([a, b[:, 4:]], 1).double()
    if G:
        x = torch.nn.functional.group_norm(x[:, :, None], G, gamma.double(), beta.double(), 1e-5)[:, :, 0]
    want = torch.nn.functional.silu(x) if silu else x
    assert rel_l2(y, want) < KERNEL_TOL


def test_graph_pool_is_exact_ordered_and_repeatable():
    from lidarcrafter_amd import ops_skinny as S
    from lidargen.models.unets.graph import edge_csr

    O, T, H = 11, 40, 256
    s, o = torch.arange(T) * 3 % (O - 1), torch.arange(T) * 7 % (O - 1)          # object O-1: in no triple
    row_ptr, slots = edge_csr(s, o, O)
    t = seeded_randn(T, 2 * H + 128, seed=1)
    y1 = S.graph_pool(t.cuda(), 0, H + 128, H, row_ptr.cuda(), slots.cuda())
    y2 = S.graph_pool(t.cuda(), 0, H + 128, H, row_ptr.cuda(), slots.cuda())
    assert torch.equal(y1, y2)
    assert torch.equal(y1[O - 1], torch.zeros(H, device="cuda"))
    # the order of two sequential scatter_add calls on the CPU (the reference): the same float32 bits
    pooled = torch.zeros(O, H).scatter_add(0, s.view(-1, 1).expand(T, H), t[:, :H])
    pooled = pooled.scatter_add(0, o.view(-1, 1).expand(T, H), t[:, H + 128:])
    cnt = (torch.bincount(s, minlength=O) + torch.bincount(o, minlength=O)).clamp(min=1).float()
    assert torch.equal(y1.cpu(), pooled / cnt.view(-1, 1))


def test_time_embed():
    from lidarcrafter_amd import ops_skinny as S
    from lidargen.models.unets.unet_1d import timestep_freqs

    t, f = torch.tensor([-15.0, -0.3, 0.0, 4.2, 15.0]), timestep_freqs(512)
    y = S.time_embed(t.cuda(), f.cuda())
    a = (t[:, None] * f[None]).double()
    assert rel_l2(y, torch.cat([a.cos(), a.sin()], -1)) < KERNEL_TOL


# ------------------------------------------------------------------------------------------------------ fixtures
def _cond(d, batch):
    sg = d.get_scenegraph_input(batch["scenegraph_input"])
    np.random.seed(5)
    with torch.no_grad():
        lat, emb = d.condition_model(*sg)
    return sg, lat, emb


@pytest.mark.parametrize("name,seed,manip", [("sg_plain", 1, False), ("sg_manip", 2, True)])
def test_scene_graph_on_device(ddpm, gold, name, seed, manip):
    _, lat, emb = _cond(ddpm, synth_scene_graph_batch(3, seed=seed, manipulate=manip))
    assert lat.is_cuda and rel_l2(lat, torch.from_numpy(gold[name + "_latent"])) < FWD_TOL
    assert rel_l2(emb, torch.from_numpy(gold[name + "_embed"])) < FWD_TOL


@pytest.mark.parametrize("name,seed,manip,times,xs", [("unet_uniform", 1, False, [0.7, 0.7, 0.7], 31),
                                                      ("unet_per_scene", 2, True, [-3.0, 0.4, 5.5], 32)])
def test_unet_forward(ddpm, gold, name, seed, manip, times, xs):
    sg, lat, emb = _cond(ddpm, synth_scene_graph_batch(3, seed=seed, manipulate=manip))
    t = torch.tensor(times)[sg[9]].cuda()
    other = ddpm.prepare_df_input(sg[5], emb, relation_cond=lat, scene_ids=sg[9])
    with torch.no_grad():
        y = ddpm.model(seeded_randn(emb.shape[0], 20, seed=xs).cuda(), dict(time_condition=t, other_condition=other))
    near_reference(gold, name, y)


def test_unet_forward_single_object(ddpm, gold):
    other = ddpm.prepare_df_input(torch.tensor([[0, 3, 0]]).cuda(), seeded_randn(1, 640, seed=33).cuda(), relation_cond=None)
    with torch.no_grad():
        y = ddpm.model(seeded_randn(1, 20, seed=34).cuda(), dict(time_condition=torch.tensor([1.25]).cuda(),
                                                                 other_condition=other))
    near_reference(gold, "unet_single", y)


def test_graph_network_alone(ddpm, gold):
    """box_graph_cov through the program's graph section: the context buffer of a plan whose object rows are given."""
    from lidargen.models.unets.unet_1d import Program, _Plan

    batch = synth_scene_graph_batch(3, seed=1)
    sg = ddpm.get_scenegraph_input(batch["scenegraph_input"])
    O, T = sg[4].shape[0], sg[5].shape[0]
    plan = ddpm.model.make_plan(torch.zeros(O, 640, device="cuda"), sg[5])
    P = plan.P
    first = next(i for i, op in enumerate(P.ops) if op[1] == "g_t1")
    last = max(i for i, op in enumerate(P.ops) if op[1].startswith("g_obj"))
    sub = Program()
    sub.ops, sub.bufs, sub.w = P.ops[first:last + 1], P.bufs, P.w
    plan.B["obj0"].copy_(seeded_randn(O, 768, seed=35))
    plan.B["pred0"].copy_(seeded_randn(T, 128, seed=36))
    plan.P = sub
    plan.run()
    near_reference(gold, "gcn", plan.B[P.ops[last][1]])


@pytest.mark.parametrize("name,path,seeds", [("mod_resblock", "output_blocks.0.0", (51, 52)),
                                             ("mod_transformer", "input_blocks.4.1", (53, 54)),
                                             ("mod_downsample", "input_blocks.3.0", (55,)),
                                             ("mod_upsample", "output_blocks.2.1", (56,))])
def test_single_modules(ddpm, gold, name, path, seeds):
    """One torso module through ITS ops of the program on the kernels (Program.modules): the ResBlock with the fused
    [n2 | h | skip] x [W_out | W_skip] product and the 1024-channel GroupNorm, a SpatialTransformer1D, the stride-2
    Downsample conv (centre tap) and Upsample (identity + conv).  7 rows, every row with a time embedding of its own."""
    from lidargen.models.unets.unet_1d import Program

    O = 7
    plan = ddpm.model.make_plan(torch.zeros(O, 640, device="cuda"), torch.tensor([[0, 1, 1]]), O, torch.arange(O))
    P = plan.P
    first, last, segs, out = P.modules[path]
    x = seeded_randn(O, sum(w for _, _, w, _ in segs), seed=seeds[0])
    c = 0
    for buf, c0, w, _ in segs:                               # the module's input, split over its source buffers
        plan.B[buf][:, c0:c0 + w].copy_(x[:, c:c + w])
        c += w
    ops = list(P.ops[first:last + 1])
    if name == "mod_resblock":                               # emb -> SiLU -> all emb_layers at once (the hoisted time path)
        plan.B["emb"].copy_(seeded_randn(O, 2048, seed=seeds[1]))
        ops = [op for op in P.ops if op[1] in ("embs", "embproj")] + ops
    if name == "mod_transformer":
        plan.B[P.context].copy_(seeded_randn(O, 1280, seed=seeds[1]))
    sub = Program()
    sub.ops, sub.bufs, sub.w = ops, P.bufs, P.w
    plan.P = sub
    plan.run()
    near_reference(gold, name, plan.B[out])


@pytest.mark.parametrize("mode", ["ddpm", "ddim"])
def test_p_step_and_trajectory(ddpm, gold, mode):
    batch = synth_scene_graph_batch(3, seed=2, manipulate=True)
    sg, lat, emb = _cond(ddpm, batch)
    O = emb.shape[0]
    cd = dict(other_condition=ddpm.prepare_df_input(sg[5], emb, relation_cond=lat, scene_ids=sg[9]))
    y = ddpm.p_step(seeded_randn(O, 20, seed=41).cuda(), cd, torch.full((O,), 0.6), torch.full((O,), 0.5),
                    rng=gens(O, 500), mode=mode)
    near_reference(gold, f"pstep_{mode}", y)
    np.random.seed(5)
    traj = ddpm.sample(batch, 8, progress=False, rng=gens(O, 700), return_all=True, mode=mode)
    want = torch.from_numpy(gold[f"traj_{mode}"])
    assert traj.shape == want.shape and torch.equal(traj[0].cpu(), want[0])           # x_T: CPU generators
    for i in range(1, 9):
        assert rel_l2(traj[i], want[i]) < TRAJ_TOL, i
    print(f"traj_{mode}: last state rel L2 {rel_l2(traj[8], want[8]):.3e} (ref_err {float(gold[f'ref_err_traj_{mode}']):.3e})")


def test_eval_loss(ddpm, gold, monkeypatch):
    batch = synth_scene_graph_batch(3, seed=2, manipulate=True)
    sg = ddpm.get_scenegraph_input(batch["scenegraph_input"])
    O = sg[4].shape[0]
    noise = seeded_randn(O, 20, seed=42).cuda()
    monkeypatch.setattr(ddpm, "randn_like", lambda x, rng=None: noise.clone(), raising=False)
    steps = torch.tensor([0.2, 0.55, 0.9])[sg[9]].cuda()
    np.random.seed(5)
    with torch.no_grad():
        loss = ddpm.p_loss(dict(x_0=sg[6][:, :20], scenegraph_input=sg), steps, sg[6][:, 20:])
    near_reference(gold, "loss", loss.reshape(1))
    monkeypatch.undo()
    before, inner = dict(batch), dict(batch["scenegraph_input"])
    with torch.no_grad():                                     # the whole forward: draws its own t and noise
        assert torch.isfinite(ddpm(batch))
    assert batch.keys() == before.keys() and all(batch[k] is before[k] for k in before)     # forward(): a shallow copy too
    assert batch["scenegraph_input"].keys() == inner.keys()
    assert all(batch["scenegraph_input"][k] is inner[k] for k in inner)


# ------------------------------------------------------------------------------------------------------ the sampler
def _sample(d, batch, steps=6, mode="ddpm", base=900, **kw):
    np.random.seed(5)
    O = batch["scenegraph_input"]["decoder"]["objs"].numel()
    return d.sample(batch, steps, progress=False, rng=gens(O, base), mode=mode, **kw)


def test_graph_replay_equals_eager_loop(ddpm, monkeypatch):
    batch = synth_scene_graph_batch(3, seed=4, manipulate=True)
    monkeypatch.setattr(ddpm, "use_hip_graph", True, raising=False)
    a = _sample(ddpm, batch, return_all=True)
    monkeypatch.setattr(ddpm, "use_hip_graph", False, raising=False)
    b = _sample(ddpm, batch, return_all=True)
    assert torch.equal(a, b)


def test_repeat_calls_and_callers_dict(ddpm):
    batch, other = synth_scene_graph_batch(3, seed=4, manipulate=True), synth_scene_graph_batch(5, seed=9)
    before, inner = dict(batch), dict(batch["scenegraph_input"])
    a = _sample(ddpm, batch)
    _sample(ddpm, other, mode="ddim")                          # other O, T in between
    b = _sample(ddpm, batch)
    assert torch.equal(a, b)
    assert batch.keys() == before.keys() and all(batch[k] is before[k] for k in before)
    assert all(batch["scenegraph_input"][k] is inner[k] for k in inner)


def test_weight_changes_are_seen(ddpm):
    batch = synth_scene_graph_batch(2, seed=6)
    d = copy.deepcopy(ddpm)
    base = _sample(d, batch)
    conv = d.model.input_blocks[1][0].in_layers[2]
    with torch.no_grad():
        conv.weight[:, :, 0].add_(1.0)                         # an outer tap: dead
        for blk in d.model.modules():
            if hasattr(blk, "to_q"):
                blk.to_q.weight.normal_()
                blk.to_k.weight.normal_()
    assert torch.equal(_sample(d, batch), base)
    with torch.no_grad():
        conv.weight[:, :, 1].mul_(1.5)                         # the centre tap: live
    changed = _sample(d, batch)
    fresh = build()
    fresh.load_state_dict(d.state_dict())
    assert not torch.equal(changed, base) and torch.equal(changed, _sample(fresh, batch))
    other = build(salt=12)
    d.load_state_dict(other.state_dict())
    assert torch.equal(_sample(d, batch), _sample(other, batch))


def test_inference_mode_weights_are_repacked(ddpm):
    """Parameters made under torch.inference_mode() carry no version counter: the pack is rebuilt on every call, so an
    in-place change of such a weight is seen."""
    batch = synth_scene_graph_batch(2, seed=6)
    d = copy.deepcopy(ddpm)
    with torch.inference_mode():
        conv = d.model.input_blocks[1][0].in_layers[2]
        conv.weight = torch.nn.Parameter(conv.weight.clone(), requires_grad=False)
    assert conv.weight.is_inference() and d.model._fingerprint() is None
    base = _sample(d, batch)
    with torch.inference_mode():
        conv.weight[:, :, 1].mul_(1.5)
    assert not torch.equal(_sample(d, batch), base)


def test_scenes_do_not_influence_each_other(ddpm):
    """The denoiser: bit-equal -- the summation order of every kernel is fixed per output element and does not depend
    on M.  A whole sample(): within the trajectory tolerance only, because the condition model in front of it runs on
    the BLAS library, whose kernel choice (and so its rounding) may change with the number of rows."""
    a, b = synth_scene_graph_batch(1, seed=3), synth_scene_graph_batch(1, seed=4)
    sa, sb = a["scenegraph_input"], b["scenegraph_input"]
    na, nb = sa["decoder"]["objs"].numel(), sb["decoder"]["objs"].numel()
    both = {"missing_nodes": [], "manipulated_subs": [], "manipulated_objs": []}
    for side in ("encoder", "decoder"):
        off = sa[side]["objs"].numel()
        tb = sb[side]["tripltes"].clone()
        tb[:, 0] += off
        tb[:, 2] += off
        both[side] = {k: torch.cat([sa[side][k], tb if k == "tripltes" else sb[side][k] + (1 if k.endswith("to_scene") else 0)])
                      for k in sa[side]}
    ta, tb_ = sa["decoder"]["tripltes"].cuda(), sb["decoder"]["tripltes"].cuda()
    tab = both["decoder"]["tripltes"].cuda()
    ua, ub = seeded_randn(na, 640, seed=1).cuda(), seeded_randn(nb, 640, seed=2).cuda()
    xa, xb = seeded_randn(na, 20, seed=3).cuda(), seeded_randn(nb, 20, seed=4).cuda()

    def fwd(x, u, tr, t):
        with torch.no_grad():
            return ddpm.model(x, dict(time_condition=t.cuda(), other_condition=dict(uc_b=u, preds=tr, c_b=None)))

    ya, yb = fwd(xa, ua, ta, torch.full((na,), 0.3)), fwd(xb, ub, tb_, torch.full((nb,), -2.0))
    yab = fwd(torch.cat([xa, xb]), torch.cat([ua, ub]), tab, torch.cat([torch.full((na,), 0.3), torch.full((nb,), -2.0)]))
    assert torch.equal(yab[:na], ya) and torch.equal(yab[na:], yb)
    sa_ = ddpm.sample(a, 5, progress=False, rng=gens(na, 100))
    sb_ = ddpm.sample(b, 5, progress=False, rng=gens(nb, 200))
    sab = ddpm.sample({"scenegraph_input": both}, 5, progress=False, rng=gens(na, 100) + gens(nb, 200))
    assert rel_l2(sab[:na], sa_) < TRAJ_TOL and rel_l2(sab[na:], sb_) < TRAJ_TOL
