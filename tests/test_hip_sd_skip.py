"""GPU: per-step layer skipping on the Stable-Diffusion latent UNet -- the skipped forward against the float
reference (tests/sd_skip_ref.py) and against the unskipped network with the skipped block's last layer zeroed, the graph cache of
skip sets, the samplers' routing of the per-step lists, split guidance, and the evaluator / command line on the tiny networks.

Shapes are those of the ``sd_unet_tiny`` golden (n = 2, 4 x 16 x 16 latents, 15 layers); one case runs ``sd_unet_w320`` (320-wide maps,
40-wide heads: the resident-tile 1x1 picks).  Tolerance: ``test_hip_sd.check``'s bound of the unskipped network (relative Frobenius
error <= 2e-2, max error <= 6e-2 of max |ref|) -- skipping removes launches, it adds no rounding.  Every set is first shown, on the
CPU, to move the float reference by more than ten times that Frobenius bound, so that returning the unskipped network cannot pass.
"""
import functools

import numpy as np
import pytest
import torch

from sd_skip_ref import sd_unet_forward_skip, tiny_sets
from test_hip_sd import _model, check
from test_hip_sd_search import _cli, _cli_flags, _leading_fid  # noqa: F401  (the tiny networks' command line; the 64-feature host FID)
from test_sd_oracle import sd_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRO_TOL = 2e-2        # check()'s default, restated for the condition against a vacuous pass
W320_MIXED = [2, 6, 7]   # an identity ResBlock of the middle block, a transformer and a two-source ResBlock of the output path


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _case(name):
    g, plan, P = sd_case(name)
    x, t, ctx = (torch.from_numpy(g[k]) for k in ("x", "t", "context"))
    return plan, P, x, t, ctx


@functools.lru_cache(maxsize=None)
def _ref(name, skip):
    """The float reference with `skip` (a sorted tuple) bypassed: computed once per set, shared, never written to."""
    plan, P, x, t, ctx = _case(name)
    return sd_unet_forward_skip(P, plan, x, t, ctx, skip).numpy()


@functools.lru_cache(maxsize=None)
def _net(name):
    plan, P, x, t, ctx = _case(name)
    return _model(plan, P), x.to(DEV), t.to(DEV), ctx.to(DEV)


def _sets():
    return tiny_sets(_case("sd_unet_tiny")[0])


# ------------------------------------------------------------------ the UNet against the float reference
@pytest.mark.parametrize("name,what", [("sd_unet_tiny", k) for k in ("identity ResBlock of the input path", "input ResBlock with a skip conv",
                                                                    "output ResBlock (two-source 1x1)", "one transformer",
                                                                    "the middle block", "every layer")] + [("sd_unet_w320", "mixed")])
def test_skipped_unet_matches_the_float_reference(name, what):
    skip = tuple(sorted(W320_MIXED if what == "mixed" else _sets()[what]))
    ref, full = _ref(name, skip), _ref(name, ())
    moved = np.linalg.norm(ref - full) / np.linalg.norm(full)
    print(f"{name} {what} {skip}: the skip moves the float reference by fro {moved:.3f}")
    assert moved > 10 * FRO_TOL, (what, moved)          # on the CPU side: a swallowed keyword cannot pass below
    m, x, t, ctx = _net(name)
    m.enable_graph(False)
    out = m(x, t, ctx, skip_layer=list(skip))
    assert out.dtype == torch.float32 and out.shape == ref.shape
    check(out, ref, f"{name}, skip {what} {list(skip)}")
    assert torch.equal(m(x, t, ctx, skip_layer=list(reversed(skip)) + [skip[0]]), out)   # order and repeats do not matter


def test_ids_outside_the_plan_are_refused_before_anything_is_launched(monkeypatch):
    from autodiffusion_amd import ops
    m, x, t, ctx = _net("sd_unet_tiny")
    assert m.layer_num == 15
    launched = []
    monkeypatch.setattr(ops, "conv", lambda *a, **kw: launched.append("conv"))
    monkeypatch.setattr(ops, "timestep_embedding", lambda *a, **kw: launched.append("emb"))
    for bad in ([15], [-1], [3, 99], [1.5]):
        with pytest.raises(ValueError, match="skip_layer"):
            m(x, t, ctx, skip_layer=bad)
    assert launched == []


# ------------------------------------------------------------------ independent of the reference
def _zeroed(prefixes):
    """The tiny network with the named tensors' weight and bias zeroed."""
    plan, P, *_ = _case("sd_unet_tiny")
    Q = dict(P)
    for p in prefixes:
        Q[p + ".weight"], Q[p + ".bias"] = torch.zeros_like(P[p + ".weight"]), torch.zeros_like(P[p + ".bias"])
    return _model(plan, Q)


def test_skipping_is_the_unskipped_network_with_the_blocks_last_layer_zeroed():
    plan = _case("sd_unet_tiny")[0]
    by_id = {b.layer_id: b for b in plan.all_blocks() if hasattr(b, "layer_id")}
    m, x, t, ctx = _net("sd_unet_tiny")
    m.enable_graph(False)
    sets = _sets()
    # a transformer returns x + proj_out(...), an identity-skip ResBlock x + out_layers(...): with that last layer zero the block is x
    for what, leaf in (("one transformer", "proj_out"), ("identity ResBlock of the input path", "out_layers.3")):
        (i,) = sets[what]
        assert torch.equal(m(x, t, ctx, skip_layer=[i]), _zeroed([f"{by_id[i].prefix}.{leaf}"])(x, t, ctx)), what
    # with a skip conv the zeroed block is skip_connection(x) through the folded conv, the skipped one through the unfused 1x1:
    # the same sum in another fp32 order
    (i,) = sets["input ResBlock with a skip conv"]
    assert by_id[i].has_skip_conv
    want = _zeroed([f"{by_id[i].prefix}.out_layers.3"])(x, t, ctx)
    check(m(x, t, ctx, skip_layer=[i]), want.cpu().numpy(), "skip-conv ResBlock skipped vs out_layers.3 zeroed")


# ------------------------------------------------------------------ the empty set is the path as it was
def test_an_empty_set_changes_nothing_eager_and_graph():
    plan, P, *_ = _case("sd_unet_tiny")
    m = _model(plan, P)
    _, x, t, ctx = _net("sd_unet_tiny")
    want = m(x, t, ctx)
    for graph in (False, True):
        m.enable_graph(graph)
        for empty in ((), [], None):
            assert torch.equal(m(x, t, ctx, skip_layer=empty), want)
    assert torch.equal(m(x, t, ctx), want)
    keys = list(m._packed.graphs)
    assert len(keys) == 1 and len(keys[0]) == 9 and len(m._packed.skip_graphs) == 0     # the key and the cache it has always had


# ------------------------------------------------------------------ graphs of skip sets
def test_graph_replay_of_skip_sets_is_the_eager_path_within_a_bounded_cache(monkeypatch):
    from autodiffusion_amd import logger
    from autodiffusion_amd.sd_unet import UNetModel
    plan, P, *_ = _case("sd_unet_tiny")
    m = _model(plan, P)
    _, x, t, ctx = _net("sd_unet_tiny")
    a, b, c = [1], [2, 12], [0, 5, 13]
    eager = {tuple(s): m(x, t, ctx, skip_layer=s) for s in (a, b, c, ())}
    assert len({o.cpu().numpy().tobytes() for o in eager.values()}) == 4
    m.enable_graph()
    for s in (a, b, a, b, a):                                        # two alternating sets: capture, capture, replays
        assert torch.equal(m(x, t, ctx, skip_layer=s), eager[tuple(s)])
    assert len(m._packed.skip_graphs) == 2 and len(m._packed.graphs) == 0
    assert torch.equal(m(x, t, ctx), eager[()]) and len(m._packed.graphs) == 1
    # more distinct sets than the bound: the oldest leave, the results stay right
    monkeypatch.setattr(UNetModel, "SKIP_GRAPH_CACHE", 2)
    m.plan_graphs(1)
    for s in (a, b, c, a, c, b):
        assert torch.equal(m(x, t, ctx, skip_layer=s), eager[tuple(s)])
        assert len(m._packed.skip_graphs) <= 2
    assert len(m._packed.graphs) == 1                                # the empty set's graph is not part of the LRU
    # per-image results do not depend on the batch (ragged batch), through a graph of its own shape
    x3, t3, c3 = torch.cat([x, x[:1]]), torch.cat([t, t[:1]]), torch.cat([ctx, ctx[:1]])
    out3 = m(x3, t3, c3, skip_layer=b)
    assert torch.equal(out3[:2], eager[tuple(b)]) and torch.equal(out3[2], eager[tuple(b)][0])
    assert len(m._packed.skip_graphs) <= 2
    # a candidate announced with more sets than fit is evaluated eagerly, with one log line, and captures nothing
    lines = []
    monkeypatch.setattr(logger, "log", lambda *args: lines.append(" ".join(str(v) for v in args)))
    monkeypatch.setattr(UNetModel, "SKIP_GRAPH_CACHE_MAX", 3)
    held = list(m._packed.skip_graphs)
    m.plan_graphs(2, streams=2)
    assert m._graph_eager
    for s in (a, b, c, a):
        assert torch.equal(m(x, t, ctx, skip_layer=s), eager[tuple(s)])
    m.plan_graphs(2, streams=2)
    assert list(m._packed.skip_graphs) == held
    off = [l for l in lines if "hipGraph replay off" in l]
    assert len(off) == 1 and "2 distinct layer-skip sets x 2 stream(s)" in off[0]
    assert torch.equal(m(x, t, ctx), eager[()])                      # the unskipped evaluation keeps its graph
    m.plan_graphs(1)
    assert not m._graph_eager and m.SKIP_GRAPH_CACHE == 2
    # the byte budget: a candidate whose graphs' private pools would not fit together replays the one just captured, keeps none
    # and goes eager, with one more log line
    monkeypatch.setattr(UNetModel, "GRAPH_POOL_FRACTION", 1e-12)
    m2 = _model(plan, P).enable_graph()
    m2.plan_graphs(2)
    assert not m2._graph_eager and m2._pool_bytes_seen == 0           # no capture has told the pool's size yet
    assert torch.equal(m2(x, t, ctx, skip_layer=a), eager[tuple(a)])  # captured, replayed once, dropped
    assert m2._pool_bytes_seen > 0 and m2._graph_eager and len(m2._packed.skip_graphs) == 0
    assert torch.equal(m2(x, t, ctx, skip_layer=b), eager[tuple(b)]) and len(m2._packed.skip_graphs) == 0
    off = [l for l in lines if "hipGraph replay off" in l]
    assert len(off) == 2 and "of private pool" in off[1]


# ------------------------------------------------------------------ samplers
class _Recorder:
    """LatentDiffusion's tables around the oracle's toy model: records (timestep, skip list) of every evaluation."""

    def __init__(self):
        from autodiffusion_amd.sd_sampler import LatentDiffusion
        base = LatentDiffusion(None, device=DEV)
        self.num_timesteps, self.device = base.num_timesteps, base.device
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = base.betas, base.alphas_cumprod, base.alphas_cumprod_prev
        self.seen = []

    def apply_model(self, x, t, c, skip_layer=()):
        from oracle.sd_sampler import toy_model
        self.seen.append((round(float(t[0]), 3), tuple(skip_layer), x.shape[0]))
        return toy_model(x, t, c)


def test_every_evaluation_at_a_timestep_carries_that_timesteps_list():
    from autodiffusion_amd.sd_sampler import DDIMSampler, DPMSolverSampler, PLMSSampler, UniPCSampler
    g = torch.Generator().manual_seed(2)
    x_T, c, uc = (torch.randn(3, 4, 8, 8, generator=g).to(DEV) for _ in range(3))
    kw = dict(batch_size=3, shape=[4, 8, 8], conditioning=c, verbose=False, x_T=x_T)
    cand, lists = [690, 153, 926, 424], [[6], [1, 5], [], [4]]
    by_t = dict(zip(cand, (tuple(s) for s in lists)))
    m = _Recorder()
    DDIMSampler(m).sample(S=4, sampled_timestep=np.array(cand), skip_layers=lists, unconditional_guidance_scale=3.0,
                          unconditional_conditioning=uc, **kw)
    assert [s[:2] for s in m.seen] == [(float(t), by_t[t]) for t in sorted(cand, reverse=True)]
    assert all(s[2] == 6 for s in m.seen)                                # batched guidance: both halves in the one call
    # PLMS takes the list as given (ascending); the first step's second evaluation is at t_next and carries t_next's list
    asc = sorted(cand)
    m.seen = []
    PLMSSampler(m).sample(S=4, sampled_timestep=np.array(asc), skip_layers=[list(by_t[t]) for t in asc], **kw)
    assert [s[:2] for s in m.seen] == [(float(t), by_t[t]) for t in (926, 690, 690, 424, 153)]
    # ... and the unguided evaluation of a prompt_mask step carries its step's list too
    m.seen = []
    PLMSSampler(m).sample(S=4, sampled_timestep=np.array(asc), skip_layers=[list(by_t[t]) for t in asc], prompt_mask=[1, 0, 1, 0],
                          unconditional_guidance_scale=3.0, unconditional_conditioning=uc, **kw)
    assert [s for s in m.seen] == [(926.0, by_t[926], 6), (690.0, by_t[690], 6), (690.0, by_t[690], 3), (424.0, by_t[424], 6),
                                   (153.0, by_t[153], 3)]
    # DPM-Solver / UniPC: K + 1 times, K evaluations, list j at evaluation j
    times, klists = [999, 600, 300, 50, 1], [[1], [2], [], [3, 4]]
    for cls in (DPMSolverSampler, UniPCSampler):
        m.seen = []
        cls(m).sample(S=4, sampled_timestep=times, skip_layers=klists, **kw)
        assert [s[1] for s in m.seen] == [tuple(s) for s in klists], cls.__name__
        assert [s[0] for s in m.seen] == sorted((s[0] for s in m.seen), reverse=True)
        with pytest.raises(ValueError, match="skip_layers holds 5 lists for 4"):
            cls(m).sample(S=4, sampled_timestep=times, skip_layers=klists + [[]], **kw)
    # a wrong length raises before any evaluation; None changes nothing (the model is called without the keyword)
    m.seen = []
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(ValueError, match="skip_layers holds 3 lists for 4"):
            cls(m).sample(S=4, sampled_timestep=np.array(asc), skip_layers=lists[:3], **kw)
    assert m.seen == []
    plain = _Recorder()
    plain.apply_model = lambda x, t, c: m.apply_model(x, t, c)
    a, _ = DDIMSampler(plain).sample(S=4, sampled_timestep=np.array(cand), **kw)
    b, _ = DDIMSampler(m).sample(S=4, sampled_timestep=np.array(cand), skip_layers=[[]] * 4, **kw)
    assert torch.equal(a, b) and all(s[1] == () for s in m.seen)
    # decode(): one list per entry of the schedule's table, entries [:t_start] used
    s = DDIMSampler(m)
    s.make_schedule(ddim_num_steps=4, verbose=False, sampled_timestep=asc)
    m.seen = []
    s.decode(x_T, c, 3, skip_layers=[list(by_t[t]) for t in asc])
    assert [v[:2] for v in m.seen] == [(float(t), by_t[t]) for t in (690, 424, 153)]
    with pytest.raises(ValueError):
        s.decode(x_T, c, 3, skip_layers=[[]] * 3)


def _tiny_ld():
    from autodiffusion_amd.sd_sampler import LatentDiffusion
    m, x, t, ctx = _net("sd_unet_tiny")
    return m, LatentDiffusion(m, device=DEV), x, ctx, ctx.flip(1).contiguous() * 0.5


def test_ddim_with_skip_lists_matches_the_oracle_steps_over_the_skip_reference():
    from autodiffusion_amd.sd_sampler import DDIMSampler
    from oracle import sd_sampler as S
    plan, P, x_T, _, ctx = _case("sd_unet_tiny")
    unet, ld, x_dev, ctx_dev, _ = _tiny_ld()
    unet.enable_graph(False)
    cand, lists = [690, 153, 424], [[1], [2, 12], [0, 5, 13]]            # unsorted: each list moves with its timestep
    by_t = dict(zip(cand, lists))
    kw = dict(S=3, batch_size=2, shape=[4, 16, 16], conditioning=ctx_dev, verbose=False, x_T=x_dev, sampled_timestep=np.array(cand))
    got, _ = DDIMSampler(ld).sample(skip_layers=lists, **kw)
    ref = S.ddim_sample(lambda x, t, c: sd_unet_forward_skip(P, plan, x, t, c, by_t[int(t[0])]), S.alphas_cumprod_f32(), x_T, ctx,
                        sorted(cand))
    check(got, ref.numpy(), "DDIM 3-step with per-step skip lists, tiny latent UNet", 3e-2, 8e-2)
    swapped, _ = DDIMSampler(ld).sample(skip_layers=[lists[1], lists[0], lists[2]], **kw)
    none, _ = DDIMSampler(ld).sample(**kw)
    assert not torch.equal(swapped, got) and not torch.equal(none, got)


def test_split_and_batched_guidance_agree_bitwise_with_skip_lists():
    from autodiffusion_amd.sd_sampler import DDIMSampler, PLMSSampler
    unet, ld, x_T, ctx, uc = _tiny_ld()
    cand, lists = [153, 424, 690], [[2, 12], [], [1]]
    for cls in (DDIMSampler, PLMSSampler):
        outs = []
        for split, graph in ((True, False), (False, False), (True, True), (False, True)):
            unet.enable_graph(graph)
            s = cls(ld)
            s.split_guidance = split
            out, _ = s.sample(S=3, batch_size=2, shape=[4, 16, 16], conditioning=ctx, verbose=False, x_T=x_T,
                              unconditional_guidance_scale=3.0, unconditional_conditioning=uc, sampled_timestep=np.array(cand),
                              skip_layers=lists)
            torch.cuda.synchronize()
            outs.append(out.clone())
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), cls.__name__
    unet.enable_graph(False)
    plain, _ = DDIMSampler(ld).sample(S=3, batch_size=2, shape=[4, 16, 16], conditioning=ctx, verbose=False, x_T=x_T,
                                      unconditional_guidance_scale=3.0, unconditional_conditioning=uc, sampled_timestep=np.array(cand))
    assert not torch.equal(plain, outs[0])


# ------------------------------------------------------------------ evaluator and command line
def test_cli_evaluates_dict_candidates_and_runs_the_joint_search(_leading_fid, tmp_path):  # noqa: F811
    cli, flags = _cli(), _cli_flags(tmp_path)
    plain = cli.main(flags + ["--evaluate", "[100, 500, 900]"])
    empty = cli.main(flags + ["--evaluate", "{'timesteps': [100, 500, 900], 'skip_layers': [[], [], []]}"])
    skipped = cli.main(flags + ["--evaluate", "{'timesteps': [100, 500, 900], 'skip_layers': [[1], [], [2, 12]]}"])
    print("FID plain", plain, "all-empty dict", empty, "non-empty dict", skipped)
    assert np.isfinite(plain) and empty == plain and np.isfinite(skipped) and skipped != plain
    lines = (tmp_path / "out" / "log.txt").read_text().splitlines()
    assert any(l.startswith("cand: {'timesteps': [100, 500, 900], 'skip_layers': [[1], [], [2, 12]]}, fid: ") for l in lines)
    out = tmp_path / "joint"
    s = cli.main([f if f != str(tmp_path / "out") else str(out) for f in flags]
                 + ["--use_dynamic_unet", "True", "--max_prun", "0.5", "--min_prun", "0.1"])
    from autodiffusion_amd.sd_search import DynamicEvolutionSearcher, parse_sd_candidate
    assert isinstance(s, DynamicEvolutionSearcher) and s.model_layers == 15 and s.max_index_number == 3 * 15
    lines = (out / "log.txt").read_text().splitlines()
    final = lines.index("epoch = 1 : top {} result".format(len(s.keep_top_k[50])))
    tops = lines[final + 1:final + 1 + len(s.keep_top_k[50])]
    assert tops and all(l.startswith("No.") and isinstance(parse_sd_candidate(l.split(" ", 1)[1].split(" fid = ")[0]), dict) for l in tops)
    assert all(np.isfinite(s.vis_dict[c]["fid"]) for c in s.keep_top_k[50])
    assert lines[-1].startswith("total searching time = ")
